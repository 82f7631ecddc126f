"""GPU: the three multi-view entry points of csrc/group_ops.hip through the C-ABI against float64 (tests/multiview_oracle.py):
spaa_decide_views on engineered logits and loss tables, spaa_views_combine on every size around the 256-pixel block, and
spaa_views_track's gated copies."""
import numpy as np
import pytest
import torch

import multiview_oracle as mo
from spaa_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'
P_THRESH = 0.9
ADV_SCALE = 0.25


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    _lib.load()
    return _lib


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def decide_case(V, ncls, HW, seed):
    """B = 4 samples (targeted, targeted, untargeted, untargeted) with mixed loss weights and d_thr.  Sample 0's target wins in every
    view, with p1 ~ 1 in view 0 only (all succ, one view fooled); sample 1's wins confidently everywhere (all fooled: on the colour step
    when its d_thr is 5, at HW = 4096, and below its d_thr of 9 at HW = 3120; its colour loss never beats its best so far); sample 2
    (untargeted) keeps its class in view 0 only; sample 3 is fooled in every view and sets a new best.  The loss tables put
    caml2 * 255 near 7, between the d_thr values."""
    rng = np.random.default_rng(seed)
    B, nblk = 4, (HW + 255) // 256
    target = np.array([3, 5, 2, 7])
    targeted = np.array([True, True, False, False])
    logits = []
    for v in range(V):
        lg = rng.standard_normal((B, ncls)).astype(np.float32)
        lg[0, 3] = 14.0 if v == 0 else 6.0
        if v > 0:
            lg[0, 0] = 5.0                                   # (a rival: p1 ~ 0.7 at 10 classes, ~ 0.2 at 1000)
        lg[1, 5] = 14.0
        lg[2, 2] = 14.0 if v == 0 else -2.0
        lg[3, 7] = -5.0
        logits.append(lg)
    # per-block sums of 256 pixels' |scene - y| ~ 256 * 7 / 255, dE ~ 256 * 3; the third column is not read
    partial = [(rng.uniform(0.8, 1.2, (B, nblk, 3)) * np.array([256 * 7.0 / 255.0, 256 * 3.0, 1.0]) * HW / (256.0 * nblk)).astype(np.float32)
               for _ in range(V)]
    params = np.array([[0.1, 1.0, 1.0, 5.0], [0.0, 1.0, 0.0, 5.0 if HW == 4096 else 9.0], [0.1, 0.0, 1.0, 9.0], [0.0, 1.0, 1.0, 2.0]],
                      dtype=np.float32)
    prjl2 = rng.uniform(0.01, 0.05, B).astype(np.float32)
    col_best = np.array([1e6, 1e-3, 1e6, 1e6], dtype=np.float32)      # (sample 1: a best that this iteration does not beat)
    return dict(B=B, V=V, ncls=ncls, HW=HW, nblk=nblk, target=target, targeted=targeted, logits=logits, partial=partial, params=params,
                prjl2=prjl2, col_best=col_best)


def _tables(c):
    """The case's per-sample inputs on the device: target, prjl2, params, flags."""
    return (_dev(c['target'], torch.int32), _dev(c['prjl2']), _dev(c['params']), _dev(c['targeted'].astype(np.int32), torch.int32))


def run_decide_views(lib, c, focus, V=None, logits=None, partial=None):
    """Launches spaa_decide_views on the case (V / logits / partial as given instead, for the identical-view and error cases);
    returns the output tensors, prefilled with sentinels."""
    B, ncls = c['B'], c['ncls']
    V = c['V'] if V is None else V
    lg = [_dev(a) for a in (c['logits'] if logits is None else logits)]
    pt = [_dev(a) for a in (c['partial'] if partial is None else partial)]
    n = len(lg)
    out = dict(state=torch.full((B, 4), -7, dtype=torch.int32, device=DEV), stats=torch.full((B, 8), -7.0, device=DEV),
               view_state=torch.full((B, n, 2), -7, dtype=torch.int32, device=DEV), view_stats=torch.full((B, n, 4), -7.0, device=DEV),
               view_w=torch.full((B, n), -7.0, device=DEV), seeds=[torch.full((B, ncls), -7.0, device=DEV) for _ in range(n)])
    out['stats'][:, 5] = _dev(c['col_best'])
    p = lib.ptr
    target, prjl2, params, flags = _tables(c)                               # (held until the launch has run)
    lib.call('spaa_decide_views', lib.ptr_array(lg), V, ncls, p(target), lib.ptr_array(pt), c['nblk'], c['HW'], p(prjl2), p(params),
             p(flags), P_THRESH, ADV_SCALE, int(focus), p(out['state']), p(out['stats']), p(out['view_state']), p(out['view_stats']),
             p(out['view_w']), lib.ptr_array(out['seeds']), B)
    torch.cuda.synchronize()
    return out


def reference(c, focus):
    HW = c['HW']
    caml2_v = np.stack([pt.astype(np.float64)[:, :, 0].sum(axis=1) / HW for pt in c['partial']], axis=1)
    camdE_v = np.stack([pt.astype(np.float64)[:, :, 1].sum(axis=1) / HW for pt in c['partial']], axis=1)
    ref = mo.decide_views(c['logits'], c['target'], c['targeted'], caml2_v, camdE_v, c['params'][:, :3], c['params'][:, 3], P_THRESH, focus,
                          prjl2=c['prjl2'], col_best=c['col_best'])
    top2 = [np.sort(lg.astype(np.float64), axis=1)[:, -2:] for lg in c['logits']]
    ref['gap'] = np.stack([t[:, 1] - t[:, 0] for t in top2], axis=1)
    ref['p_margin'] = np.where(c['targeted'][:, None], np.abs(ref['p1'] - P_THRESH), np.inf)
    ref['d_margin'] = np.abs(ref['caml2'] * 255.0 - c['params'][:, 3].astype(np.float64))
    return ref


@pytest.mark.parametrize('HW', [4096, 3120])
@pytest.mark.parametrize('ncls', [10, 1000])
@pytest.mark.parametrize('V', [2, 3, 4])
def test_decide_views_against_float64(lib, V, ncls, HW):
    c = decide_case(V, ncls, HW, seed=100 * V + ncls + HW)
    B = c['B']
    for focus in (False, True):
        ref = reference(c, focus)
        clear = (ref['gap'] > 1e-3) & (ref['p_margin'] > 1e-3)              # [B][V], the rule of test_ensemble_gpu.clear_pairs
        clear_d = ref['d_margin'] > 1e-3
        assert (~clear).sum() <= 1 and clear_d.all(), 'the case itself is near a tie: choose other inputs'
        # the case mix: some views fooled and some not, all fooled above and below d_thr, a new best and none
        assert ref['nfooled'].tolist() == [1, V, V - 1, V] and ref['state_succ'].tolist() == [True, True, False, True]
        assert ref['best_adv'].tolist() == [False, HW == 4096, False, True] and ref['best'].tolist() == [False, False, False, True]
        o = run_decide_views(lib, c, focus)
        vs, vf = o['view_state'].cpu().numpy(), o['view_stats'].cpu().numpy().astype(np.float64)
        state, stats, vw = o['state'].cpu().numpy(), o['stats'].cpu().numpy().astype(np.float64), o['view_w'].cpu().numpy()
        assert (vs[clear] == ref['view_state'][clear]).all(), (vs, ref['view_state'])
        row = clear.all(axis=1)
        assert (state[row, 0] == ref['state_succ'][row]).all() and (state[row, 3] == ref['nfooled'][row]).all()
        assert (state[row & clear_d, 1] == ref['best_adv'][row & clear_d]).all()
        assert (state[row & clear_d, 2] == ref['best'][row & clear_d]).all()
        assert (vw[row] == ref['view_w'][row]).all()
        p1_err = np.abs(vf[..., 0] / ref['p1'] - 1.0)[clear].max()
        print(f'V {V} ncls {ncls} HW {HW} focus {focus}: p1 rel err {p1_err:.2e}, caml2_v rel err '
              f'{np.abs(vf[..., 2] / ref["view_stats"][..., 2] - 1).max():.2e}, col rel err {np.abs(stats[:, 3] / ref["col"] - 1).max():.2e}')
        assert np.allclose(vf[..., 0][clear], ref['p1'][clear], rtol=1e-3) and np.allclose(vf[..., 1], ref['tl'], rtol=1e-3, atol=1e-3)
        assert np.allclose(vf[..., 2], ref['view_stats'][..., 2], rtol=1e-4) and np.allclose(vf[..., 3], ref['view_stats'][..., 3], rtol=1e-4)
        assert np.allclose(stats[:, 0], ref['p_min'], rtol=1e-3) and np.allclose(stats[:, 6], ref['tl_mean'], rtol=1e-3, atol=1e-3)
        assert np.allclose(stats[:, 1], ref['caml2'], rtol=1e-4) and np.allclose(stats[:, 2], ref['camdE'], rtol=1e-4)
        assert np.allclose(stats[:, 3], ref['col'], rtol=1e-4) and np.allclose(stats[:, 4], ref['prjl2'], rtol=1e-6)
        assert np.allclose(stats[row & clear_d, 5], ref['col_best_after'][row & clear_d], rtol=1e-4)
        assert (stats[:, 7] == -7.0).all()                                   # (reserved: not written)
        # the sample values are the stated functions of the view table, in fp32
        assert np.array_equal(stats[:, 0], vf[..., 0].min(axis=1))
        for v in range(V):
            want = np.zeros((B, ncls), dtype=np.float32)
            want[np.arange(B), c['target']] = np.where(c['targeted'], -ADV_SCALE, ADV_SCALE)
            assert np.array_equal(o['seeds'][v].cpu().numpy(), want)


@pytest.mark.parametrize('V', [2, 4])
def test_identical_views_are_decide_ps_bitwise(lib, V):
    c = decide_case(V, 1000, 3120, seed=7)
    B, ncls = c['B'], c['ncls']
    for view in range(2):      # (a view with mixed outcomes, and sample 1's confident one)
        o = run_decide_views(lib, c, False, logits=[c['logits'][view]] * V, partial=[c['partial'][view]] * V)
        state = torch.full((B, 4), -7, dtype=torch.int32, device=DEV)
        stats = torch.full((B, 8), -7.0, device=DEV)
        stats[:, 5] = _dev(c['col_best'])
        seed = torch.full((B, ncls), -7.0, device=DEV)
        p = lib.ptr
        target, prjl2, params, flags = _tables(c)
        lg, pt = _dev(c['logits'][view]), _dev(c['partial'][view])
        lib.call('spaa_decide_ps', p(lg), ncls, p(target), p(pt), c['nblk'], c['HW'], p(prjl2), p(params), p(flags), P_THRESH, ADV_SCALE,
                 p(state), p(stats), p(seed), B)
        torch.cuda.synchronize()
        assert torch.equal(o['state'][:, 0:3], state[:, 0:3]) and torch.equal(o['stats'][:, 1:6], stats[:, 1:6])
        assert torch.equal(o['stats'][:, 0], stats[:, 0]) and all(torch.equal(s, seed) for s in o['seeds'])
        assert torch.equal(o['view_state'][:, :, 1], state[:, 3:4].expand(B, V))          # (each view's top-1 is the single top-1)
        assert torch.equal(o['view_stats'][:, :, 2], stats[:, 1:2].expand(B, V))


@pytest.mark.parametrize('V', [1, 5])
def test_decide_views_refuses_other_view_counts(lib, V):
    c = decide_case(2, 10, 4096, seed=3)
    many = max(V, 2)
    with pytest.raises(RuntimeError, match='spaa_decide_views failed with HIP error 1$'):
        run_decide_views(lib, c, False, V=V, logits=[c['logits'][0]] * many, partial=[c['partial'][0]] * many)
    # nothing was launched: every output keeps its sentinel
    B, ncls = c['B'], c['ncls']
    outs = dict(state=torch.full((B, 4), -7, dtype=torch.int32, device=DEV), stats=torch.full((B, 8), -7.0, device=DEV),
                vs=torch.full((B, many, 2), -7, dtype=torch.int32, device=DEV), vf=torch.full((B, many, 4), -7.0, device=DEV),
                vw=torch.full((B, many), -7.0, device=DEV))
    seeds = [torch.full((B, ncls), -7.0, device=DEV) for _ in range(many)]
    lg, pt = [_dev(c['logits'][0]) for _ in range(many)], [_dev(c['partial'][0]) for _ in range(many)]
    p = lib.ptr
    target, prjl2, params, flags = _tables(c)
    rc = getattr(lib.load(), 'spaa_decide_views')(
        lib.ptr_array(lg), V, ncls, p(target), lib.ptr_array(pt), c['nblk'], c['HW'], p(prjl2), p(params), p(flags), P_THRESH, ADV_SCALE, 0,
        p(outs['state']), p(outs['stats']), p(outs['vs']), p(outs['vf']), p(outs['vw']), lib.ptr_array(seeds), B, lib._stream())
    torch.cuda.synchronize()
    assert rc == 1                                                           # hipErrorInvalidValue
    assert all((t == -7).all() for t in list(outs.values()) + seeds)


def combine_case(V, HW, seed):
    """B = 3: sample 0 adversarial with view 1 all zero, sample 1 on the colour step, sample 2 adversarial with view 0's weight 0
    and the other weights not 1; the inputs' pad channel holds garbage."""
    rng = np.random.default_rng(seed)
    B = 3
    gs = [(rng.standard_normal((B, HW, 4)) * 10.0 ** rng.uniform(-6, -3)).astype(np.float32) for _ in range(V)]
    gs[1][0, :, :3] = 0.0
    w = rng.uniform(0.5, 1.5, (B, V)).astype(np.float32)
    w[0] = 1.0
    w[2, 0] = 0.0
    state = np.zeros((B, 4), dtype=np.int32)
    state[1, 1] = 1
    state[:, 0] = (1, 0, 1)             # (succ does not choose the rule)
    return gs, w, state


def run_combine(lib, gs, w, state, HW, V=None):
    B = w.shape[0]
    V = len(gs) if V is None else V
    nblk = (HW + 255) // 256
    g_dev = [_dev(g) for g in gs]
    arr = lib.ptr_array(g_dev)
    partial = torch.zeros(B, len(gs), nblk, device=DEV)
    out = torch.full((B, HW, 4), -7.0, device=DEV)
    w_dev, state_dev = _dev(w), _dev(state, torch.int32)
    lib.call('spaa_ens_sumsq', arr, V, lib.ptr(partial), B, HW)
    lib.call('spaa_views_combine', arr, V, lib.ptr(partial), nblk, lib.ptr(w_dev), lib.ptr(state_dev), lib.ptr(out), B, HW)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('HW', [1, 255, 256, 257, 3120])
@pytest.mark.parametrize('V', [2, 3, 4])
def test_views_combine_against_float64(lib, V, HW):
    gs, w, state = combine_case(V, HW, seed=10 * HW + V)
    out = run_combine(lib, gs, w, state, HW)
    got = out.cpu().numpy().astype(np.float64)
    want = mo.combine_views(gs, w, state[:, 1] != 0)
    err = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
    print(f'V {V} HW {HW}: error relative to the per-sample max {err.tolist()}')
    assert (err <= 2e-6).all() and (got[..., 3] == 0).all()
    assert np.abs(want).max(axis=(1, 2)).min() > 0
    assert torch.equal(run_combine(lib, gs, w, state, HW), out)              # two runs are bitwise equal
    if V == 2:   # two identical views on the colour step: (g + g) * 0.5 is g
        twin = run_combine(lib, [gs[0], gs[0]], w, state, HW).cpu().numpy()
        assert np.array_equal(twin[1, :, :3], gs[0][1, :, :3]) and (twin[..., 3] == 0).all()


@pytest.mark.parametrize('V', [1, 5])
def test_views_combine_refuses_other_view_counts(lib, V):
    gs, w, state = combine_case(2, 257, seed=1)
    many = max(V, 2)
    w = np.ones((3, many), dtype=np.float32)
    g_dev = [_dev(gs[0]) for _ in range(many)]
    partial = torch.ones(3, many, 2, device=DEV)
    out = torch.full((3, 257, 4), -7.0, device=DEV)
    w_dev, state_dev = _dev(w), _dev(state, torch.int32)
    rc = getattr(lib.load(), 'spaa_views_combine')(lib.ptr_array(g_dev), V, lib.ptr(partial), 2, lib.ptr(w_dev), lib.ptr(state_dev),
                                                   lib.ptr(out), 3, 257, lib._stream())
    torch.cuda.synchronize()
    assert rc == 1 and (out == -7.0).all()
    cams = [torch.zeros(3, 257, 4, device=DEV) for _ in range(many)]
    bests = [torch.full((3, 257, 4), -7.0, device=DEV) for _ in range(many)]
    rc = getattr(lib.load(), 'spaa_views_track')(lib.ptr_array(cams), lib.ptr_array(bests), V, lib.ptr(state_dev), 3, 257, lib._stream())
    torch.cuda.synchronize()
    assert rc == 1 and all((b == -7.0).all() for b in bests)


@pytest.mark.parametrize('V', [2, 3, 4])
def test_views_track_copies_exactly_and_per_sample(lib, V):
    B, HW = 3, 257
    gen = torch.Generator().manual_seed(V)
    cams = [torch.rand(B, HW, 4, generator=gen).to(DEV) for _ in range(V)]
    before = [torch.rand(B, HW, 4, generator=gen).to(DEV) for _ in range(V)]
    bests = [b.clone() for b in before]
    state = torch.tensor([[1, 0, 0, 0], [0, 1, 1, 3], [2, 0, 0, 0]], dtype=torch.int32, device=DEV)   # (column 0 alone gates; non-zero = set)
    lib.call('spaa_views_track', lib.ptr_array(cams), lib.ptr_array(bests), V, lib.ptr(state), B, HW)
    torch.cuda.synchronize()
    assert torch.equal(bests[0], before[0])                                  # view 0 goes through spaa_step_and_track_n
    for v in range(1, V):
        assert torch.equal(bests[v][0], cams[v][0]) and torch.equal(bests[v][2], cams[v][2]) and torch.equal(bests[v][1], before[v][1])
