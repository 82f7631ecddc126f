"""CPU: the One-pixel DE attacker's host side.  spaa_amd.de against scipy.optimize.differential_evolution (same decisions, same
objective values consumed, same numpy RNG state afterwards, every update mode and batch size); perturb_image against the
reference's outputs; the foreign route of DigitalOnePixelAttacker with the oracle classifier against every case of the
reference fixture tests/golden/onepixel_*.npz (tests/golden/make_golden_onepixel.py)."""
import glob
import os

import numpy as np
import pytest
import torch
from scipy.optimize import differential_evolution as scipy_de

import spaa_oracle as so
from spaa_amd import de, synthetic as syn
from spaa_amd.one_pixel_attacker import DigitalOnePixelAttacker, perturb_image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[len('onepixel_'):-4] for p in glob.glob(os.path.join(GOLDEN, 'onepixel_*.npz')))


def energy_of(v):
    """Cheap deterministic energy of the truncated integer vector, with many exact ties (17 levels)."""
    v = np.asarray(v).astype(int)
    return np.float32(((v * np.arange(1, v.size + 1)).sum() % 17) / 17.0)


def bounds_for(n):
    return [(2, 61), (2, 45), (0, 255), (0, 255), (0, 255)] * (n // 5)


def run_both(n, popmul, maxiter, updating, max_batch, seeding, stop_after=None):
    bounds = bounds_for(n)
    ref_calls = []

    def f(x):
        e = energy_of(x)
        ref_calls.append((x.astype(int), e))
        return e

    def batched(params):
        return np.array([energy_of(x) for x in params], dtype=np.float32)

    def make_cb():
        count = [0]

        def cb(x, convergence):
            count[0] += 1
            return stop_after is not None and count[0] >= stop_after
        return cb

    def seed():
        if seeding == 'global':
            np.random.seed(3)
            return None
        return np.random.RandomState(5) if seeding == 'randomstate' else 11

    r = scipy_de(f, bounds, maxiter=maxiter, popsize=popmul, recombination=1, atol=-1, callback=make_cb(), polish=False,
                 seed=seed(), updating=updating)
    st_ref = np.random.get_state()
    solver = de.DifferentialEvolution(batched, bounds, maxiter=maxiter, popsize=popmul, recombination=1, atol=-1,
                                      callback=make_cb(), polish=False, seed=seed(), updating=updating, max_batch=max_batch)
    solver.consumed = []
    got = solver.solve()
    st = np.random.get_state()
    assert np.array_equal(got.x, r.x) and got.fun == r.fun
    assert (got.nfev, got.nit, got.success, got.message) == (r.nfev, r.nit, r.success, r.message)
    assert len(solver.consumed) == len(ref_calls)
    for (p, e), (xr, er) in zip(solver.consumed, ref_calls):
        assert np.array_equal(p.astype(int), xr) and e == er
    assert st[0] == st_ref[0] and np.array_equal(st[1], st_ref[1]) and st[2:] == st_ref[2:]
    assert got.evaluated >= got.nfev
    return got


@pytest.mark.parametrize('n', [5, 10])
@pytest.mark.parametrize('popmul', [1, 2, 10])
@pytest.mark.parametrize('maxiter', [1, 4])
@pytest.mark.parametrize('updating', ['immediate', 'deferred'])
@pytest.mark.parametrize('max_batch', [1, 7, None])
def test_de_matches_scipy(n, popmul, maxiter, updating, max_batch):
    for seeding in ('global', 'randomstate', 'int'):
        run_both(n, popmul, maxiter, updating, max_batch, seeding)


@pytest.mark.parametrize('popmul,maxiter', [(80, 4), (10, 50), (2, 50)])
@pytest.mark.parametrize('max_batch', [1, 7, None])
def test_de_matches_scipy_long(popmul, maxiter, max_batch):
    run_both(5, popmul, maxiter, 'immediate', max_batch, 'global')


@pytest.mark.parametrize('updating', ['immediate', 'deferred'])
@pytest.mark.parametrize('max_batch', [1, 7, None])
def test_de_callback_stops_early(updating, max_batch):
    got = run_both(5, 10, 50, updating, max_batch, 'global', stop_after=3)
    assert got.nit == 3 and not got.success


def test_de_redraws_and_ties_happen():
    """The objective above exercises both things the speculation must get right: out-of-bounds redraws (their count depends on
    the trial) and exact ties (accepted by <=)."""
    redraws = []

    class Count(de.DifferentialEvolution):
        def _ensure_constraint(self, trial):
            redraws.append(np.count_nonzero((trial > 1) | (trial < 0)))
            super()._ensure_constraint(trial)

        def _accept(self, e_trial, e_orig, trial, orig):
            ties.append(e_trial == e_orig)
            return super()._accept(e_trial, e_orig, trial, orig)

    ties = []
    Count(lambda p: np.array([energy_of(x) for x in p]), bounds_for(5), maxiter=10, popsize=10, recombination=1, atol=-1,
          seed=1).solve()
    assert sum(r > 0 for r in redraws) > 10 and sum(ties) > 10


def test_de_speculation_counts():
    got = run_both(5, 10, 10, 'immediate', None, 'int')
    assert got.evaluated > got.nfev    # speculation discarded something, and nfev did not count it
    got1 = run_both(5, 10, 10, 'immediate', 1, 'int')
    assert got1.evaluated == got1.nfev


def test_de_rejects_unsupported():
    f = lambda p: np.zeros(len(p))   # noqa: E731
    with pytest.raises(NotImplementedError):
        de.differential_evolution(f, bounds_for(5), strategy='rand1bin')
    with pytest.raises(NotImplementedError):
        de.differential_evolution(f, bounds_for(5), polish=True)
    with pytest.raises(ValueError):
        de.differential_evolution(f, bounds_for(5), max_batch=0)


def _expected_perturb(x, im, pixel_size):
    """Expected image by per-element numpy writes: uint8 truncation, squares of side 2 * (pixel_size // 2) + 1 in order,
    negative indices wrapping as Python's do."""
    u8 = im.numpy().copy() if im.dtype == torch.uint8 else (im * 255).type(torch.uint8).numpy()
    _, h, w = u8.shape
    d = pixel_size // 2
    v = x.astype(int).reshape(-1, 5)
    for r, c, cr, cg, cb in v:
        for i in range(r - d, r + d + 1):
            for j in range(c - d, c + d + 1):
                u8[:, i + h if i < 0 else i, j + w if j < 0 else j] = (cr, cg, cb)
    return torch.from_numpy(u8)


@pytest.mark.parametrize('case', CASES)
def test_perturb_image_fixture(case):
    z = np.load(os.path.join(GOLDEN, f'onepixel_{case}.npz'))
    im = torch.from_numpy(z['im'])
    got = perturb_image(z['x'], im, int(z['pixel_size'])).type(torch.float32) / 255
    assert torch.equal(got, torch.from_numpy(z['im_adv']))
    for xv in z['calls_x'][:8]:
        xf = xv.astype(float) + 0.7
        assert torch.equal(perturb_image(xf, im, int(z['pixel_size'])), _expected_perturb(xf, im, int(z['pixel_size'])))


def test_perturb_image_overlap_and_bounds():
    im = syn.scenes(4, 1, (32, 40))[0]
    x = np.array([2.9, 2.2, 10, 20, 30, 28.5, 36.99, 200, 100, 50, 3.0, 3.0, 255, 0, 7], dtype=float)
    # (squares at the edges -- with d = 3 one reaches index -1 and wraps, as in the reference -- and an overlap)
    for ps in (1, 5, 6):
        got = perturb_image(x, im, ps)
        assert torch.equal(got, _expected_perturb(x, im, ps))
        assert got.dtype == torch.uint8
    u8 = (im * 255).type(torch.uint8)
    assert torch.equal(perturb_image(x, u8, 5), _expected_perturb(x, u8, 5))
    # the later square wins where two overlap
    assert perturb_image(x, im, 5)[:, 3, 3].tolist() == [255, 0, 7]


@pytest.fixture(scope='module')
def oracle_clf():
    z = np.load(os.path.join(GOLDEN, f'onepixel_{CASES[0]}.npz'))
    sd = syn.resnet18_state_dict(int(z['sd_seed']), logit_gain=float(z['logit_gain']))
    return so.OracleClassifier('resnet18', sd, sort_results=False, input_sz=tuple(z['input_sz']))


@pytest.mark.parametrize('case', CASES)
def test_foreign_route_reproduces_reference(case, oracle_clf, capsys):
    z = np.load(os.path.join(GOLDEN, f'onepixel_{case}.npz'))
    att = DigitalOnePixelAttacker({i: f'class{i}' for i in range(1000)}, tuple(z['crop']))
    trace = []
    np.random.seed(int(z['seed']))
    df, im_adv = att(torch.from_numpy(z['im']), oracle_clf, targeted_attack=bool(z['targeted']), target_idx=int(z['target_idx']),
                     pixel_count=int(z['pixel_count']), pixel_size=int(z['pixel_size']), maxiter=int(z['maxiter']),
                     popsize=int(z['popsize']), verbose=True, true_label=int(z['target_idx']), trace=trace)
    r = att.last_result
    assert np.array_equal(r.x, z['x']) and r.fun == z['fun'] and r.nfev == int(z['nfev']) and r.nit == int(z['nit'])
    assert r.success == bool(z['success_de'])
    calls = ~z['calls_cb']
    assert len(trace) == int(calls.sum())
    for (xv, e, am), xr, er, ar in zip(trace, z['calls_x'][calls], z['calls_e'][calls], z['calls_argmax'][calls]):
        assert np.array_equal(xv, xr) and e == er and am == ar
    row = df.iloc[0]
    assert list(df.columns) == ['classifier', 'pixel_count', 'true_idx', 'pred_idx', 'success', 'true_p', 'pred_p', 'cdiff']
    assert row.classifier == str(z['df_classifier']) and row.pixel_count == int(z['df_pixel_count'])
    assert row.true_idx == z['df_true_idx'] and row.pred_idx == z['df_pred_idx'] and row.success == z['df_success']
    assert row.true_p == z['df_true_p'] and row.pred_p == z['df_pred_p'] and row.cdiff == z['df_cdiff']
    assert torch.equal(im_adv, torch.from_numpy(z['im_adv']))
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == int(z['calls_cb'].sum()) and out[0].startswith('Target:' if z['targeted'] else 'Untargeted |')


def test_no_valid_centre_raises(oracle_clf):
    att = DigitalOnePixelAttacker({}, (24, 24))
    with pytest.raises(ValueError, match='no valid square centre'):
        att(torch.rand(3, 24, 24), oracle_clf, target_idx=0, pixel_size=25, maxiter=1, popsize=5)
