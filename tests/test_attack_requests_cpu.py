"""CPU: what spaa() and spaa_sweep() answer to every combination of their request arguments -- one PCNet, a sequence of one, two views,
the same view twice; one classifier, an ensemble, a foreign callable, a ViT, the same member twice; both storages; focus; jitter (also
of the wrong type); pose (also with other draws than the jitter); attention with and without rollout; transfer -- is what the commit
before the request check became one function answered: 'ok', or the exception's type and message, combination by combination against
tests/golden/attack_request_outcomes.json (written by tools/attack_requests.py --write from that commit).  The attack states and the
foreign-callable route are stubbed, nothing is allocated or launched; the full product is what holds the ORDER of the checks."""
import importlib.util
import json
import os

import pytest

from spaa_amd import projector_based_attack as A

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'attack_request_outcomes.json')
_spec = importlib.util.spec_from_file_location('attack_requests', os.path.join(os.path.dirname(HERE), 'tools', 'attack_requests.py'))
req = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(req)


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope='module')
def axes():
    return req.axes()


def test_fixture_holds_the_product(golden, axes):
    assert golden['axes'] == [[name, [n for n, _ in values]] for name, values in axes]
    n = 4 * 5 * 2 * 2 * 3 * 3 * 3 * 2
    assert len(golden['spaa']) == len(golden['spaa_sweep']) == n == len(list(req.combinations(axes)))
    outcomes = golden['outcomes']
    assert 'ok' in outcomes and len(outcomes) == len({json.dumps(o) for o in outcomes})
    # every kind of refusal occurs, and both callers are named
    kinds = {o[0] for o in outcomes if o != 'ok'}
    assert kinds == {'TypeError', 'ValueError', 'NotImplementedError'}
    assert any(o[1].startswith('spaa: ') for o in outcomes if o != 'ok') and any(o[1].startswith('spaa_sweep: ') for o in outcomes if o != 'ok')


def test_every_request_is_answered_as_before(golden, axes):
    before = (A._attack_state, A._spaa_foreign_classifier)
    got = req.outcomes(A, axes)
    assert (A._attack_state, A._spaa_foreign_classifier) == before
    names = [n for n, _ in req.combinations(axes)]
    for who in ('spaa', 'spaa_sweep'):
        want = [golden['outcomes'][i] for i in golden[who]]
        assert len(got[who]) == len(want)
        wrong = [(names[i], g, w) for i, (g, w) in enumerate(zip(got[who], want)) if g != w]
        assert not wrong, f'{who}: {len(wrong)} of {len(want)} requests answered otherwise, the first: {wrong[0]}'
