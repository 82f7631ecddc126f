"""GPU: the attack states launch what they launched before the states moved to spaa_amd/attack_state.py and the draw attacks became one
chain of stages: two eager iterations of every configuration of tools/attack_sequences.py -- the plain attack on scalar and on
per-sample settings and in fp16 storage, the ensemble with and without focus, two views, capture jitter, pose jitter, both, attention,
transfer -- launch by launch, with every integer and float argument and every pointer labelled by first appearance, against
tests/golden/attack_launch_sequences.json, recorded by that tool from the commit before the change."""
import importlib.util
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'attack_launch_sequences.json')
_spec = importlib.util.spec_from_file_location('attack_sequences', os.path.join(os.path.dirname(HERE), 'tools', 'attack_sequences.py'))
seq = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(seq)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as fh:
        return seq.sequences_of(json.load(fh))


@pytest.fixture(scope='module')
def world():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return seq.World()


def names(launches):
    return [launch[0] for launch in launches]


def test_fixture_holds_the_configurations(golden):
    assert sorted(golden) == sorted(seq.CONFIGS) and all(len(v) > 20 for v in golden.values())
    # the launch forms the configurations are there for
    plain = names(golden['plain-uniform'])
    assert 'spaa_decide' in plain and not any(n.endswith('_ps') for n in plain)
    mixed = names(golden['plain-mixed-prjl2'])
    assert {'spaa_prjl2_fwd', 'spaa_stealth_loss_fwd_bwd_ps', 'spaa_decide_ps'} <= set(mixed) and 'spaa_decide' not in mixed
    jitter = names(golden['jitter'])
    assert 'spaa_jitter_fwd' in jitter and 'spaa_jitter_fwd_each' not in jitter
    both = names(golden['pose-jitter'])
    half = len(both) // 2      # (two iterations of the same launches)
    assert both[:half] == both[half:]
    one = both[:half]
    order = [one.index(n) for n in ('spaa_pose_draw', 'spaa_pose_fwd', 'spaa_jitter_draw', 'spaa_jitter_fwd_each', 'spaa_decide_ens',
                                    'spaa_jitter_bwd', 'spaa_pose_bwd', 'spaa_ens_sumsq')]
    assert order == sorted(order) and order[1] == order[0] + 1 and order[3] == order[2] + 1   # (each draw directly before its transform)
    assert 'spaa_jitter_fwd' not in one and one.count('spaa_jitter_bwd') == one.count('spaa_pose_bwd') == 1


@pytest.mark.parametrize('name', list(seq.CONFIGS))
def test_launches_are_the_recorded_ones(golden, world, name):
    got, want = seq.record(world, seq.CONFIGS[name]), golden[name]
    assert names(got) == names(want), name
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'{name}: launch {i} ({w[0]})'
    assert len(got) == len(want)
