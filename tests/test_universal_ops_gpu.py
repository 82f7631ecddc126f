"""GPU: the two universal entry points of csrc/universal_ops.hip through the C-ABI, with sentinel-filled outputs, against float64
(tests/universal_oracle.py) on the engineered cases of tests/universal_cases.py: spaa_decide_universal on every (B, N), class count,
loss-table length and rate, its member rows bitwise against spaa_decide_ps, spaa_universal_combine on every size around the
256-pixel block within the oracle's derived bar, and the argument checks of both."""
import numpy as np
import pytest
import torch

import universal_cases as uc
import universal_oracle as uo
from spaa_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'
P_THRESH, ADV_SCALE = uc.P_THRESH, uc.ADV_SCALE


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    _lib.load()
    return _lib


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def decide_inputs(c):
    """The case's inputs on the device, by the names of spaa_decide_universal's arguments."""
    return dict(logits=_dev(c['logits']), target=_dev(c['target'], torch.int32), partial=_dev(c['partial']), prjl2=_dev(c['prjl2']),
                params=_dev(c['params']), flags=_dev(c['targeted'].astype(np.int32), torch.int32))


def decide_outputs(c):
    """Sentinel-filled outputs; stats[:, 5] holds the best colour loss so far."""
    B, ncls = c['B'], c['ncls']
    out = dict(state=torch.full((B, 4), -7, dtype=torch.int32, device=DEV), stats=torch.full((B, 8), -7.0, device=DEV),
               uni_state=torch.full((B, 2), -7, dtype=torch.int32, device=DEV), uni_stats=torch.full((B, 4), -7.0, device=DEV),
               uni_w=torch.full((B,), -7.0, device=DEV), seeds=torch.full((B, ncls), -7.0, device=DEV))
    out['stats'][:, 5] = _dev(c['col_best'])
    return out


def decide_args(lib, c, i, o, focus, **over):
    """The argument list of spaa_decide_universal without the stream; `over` replaces arguments by name (None: a null pointer)."""
    p = lib.ptr
    a = dict(logits=p(i['logits']), ncls=c['ncls'], target=p(i['target']), partial=p(i['partial']), nblk=c['nblk'], HW=c['HW'],
             prjl2=p(i['prjl2']), params=p(i['params']), flags=p(i['flags']), N=c['N'], need=c['need'], p_thresh=P_THRESH,
             adv_scale=ADV_SCALE, focus=int(focus), state=p(o['state']), stats=p(o['stats']), uni_state=p(o['uni_state']),
             uni_stats=p(o['uni_stats']), uni_w=p(o['uni_w']), g_logits=p(o['seeds']), B=c['B'])
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def run_decide(lib, c, focus):
    i, o = decide_inputs(c), decide_outputs(c)
    lib.call('spaa_decide_universal', *decide_args(lib, c, i, o, focus))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize('BN,ncls,HW,rate', uc.DECIDE_CASES)
def test_decide_universal_against_float64(lib, BN, ncls, HW, rate):
    c = uc.decide_case(BN, ncls, HW, rate)
    B, N = BN
    for focus in (False, True):
        ref = uc.decide_reference(c, focus)
        clear = (ref['gap'] > 1e-3) & (ref['p_margin'] > 1e-3)              # [B], the rule of test_decide_views_against_float64
        clear_d = ref['d_margin'] > 1e-3
        assert (~clear).sum() <= 1 and clear_d.all(), 'the case itself is near a tie: choose other inputs'
        o = run_decide(lib, c, focus)
        us, uf = o['uni_state'].cpu().numpy(), o['uni_stats'].cpu().numpy().astype(np.float64)
        state, stats, uw = o['state'].cpu().numpy(), o['stats'].cpu().numpy().astype(np.float64), o['uni_w'].cpu().numpy()
        assert (us[clear] == ref['uni_state'][clear]).all(), (us, ref['uni_state'])
        if c['tie'] is not None:
            assert us[c['tie'][0], 1] == c['tie'][1]                         # two equal maxima: the first one wins
        row = np.repeat(clear.reshape(B // N, N).all(axis=1), N)             # the rows of groups whose members are all clear
        assert (state[row, 0] == ref['state_succ'][row]).all() and (state[row, 3] == ref['nfooled'][row]).all()
        assert (state[row & clear_d, 1] == ref['best_adv'][row & clear_d]).all()
        assert (state[row & clear_d, 2] == ref['best'][row & clear_d]).all()
        assert (uw[row] == ref['uni_w'][row]).all() and np.isin(uw, (0.0, 1.0)).all()
        p1_err = np.abs(uf[:, 0] / ref['p1'] - 1.0)[clear].max()
        print(f'B {B} N {N} need {c["need"]} ncls {ncls} HW {HW} focus {focus}: p1 rel err {p1_err:.2e}, caml2_b rel err '
              f'{np.abs(uf[:, 2] / ref["uni_stats"][:, 2] - 1).max():.2e}, col rel err {np.abs(stats[:, 3] / ref["col"] - 1).max():.2e}')
        assert np.allclose(uf[:, 0][clear], ref['p1'][clear], rtol=1e-3) and np.allclose(uf[:, 1], ref['tl'], rtol=1e-3, atol=1e-3)
        assert np.allclose(uf[:, 2], ref['uni_stats'][:, 2], rtol=1e-4) and np.allclose(uf[:, 3], ref['uni_stats'][:, 3], rtol=1e-4)
        assert np.allclose(stats[:, 0], ref['p_min'], rtol=1e-3) and np.allclose(stats[:, 6], ref['tl_mean'], rtol=1e-3, atol=1e-3)
        assert np.allclose(stats[:, 1], ref['caml2'], rtol=1e-4) and np.allclose(stats[:, 2], ref['camdE'], rtol=1e-4)
        assert np.allclose(stats[:, 3], ref['col'], rtol=1e-4) and np.allclose(stats[:, 4], ref['prjl2'], rtol=1e-6)
        assert np.allclose(stats[row & clear_d, 5], ref['col_best_after'][row & clear_d], rtol=1e-4)
        # the N rows of a group hold equal words, and the reserved word is not written
        for t in (o['state'], o['stats'][:, :7]):
            g = t.reshape(B // N, N, -1)
            assert torch.equal(g, g[:, :1].expand_as(g))
        assert (stats[:, 7] == -7.0).all()
        # the group's values are the stated functions of the member table, in fp32
        assert np.array_equal(stats[:, 0], np.repeat(uf[:, 0].reshape(B // N, N).min(axis=1), N))
        assert np.array_equal(state[:, 3], np.repeat(((us[:, 0] >> 1) & 1).reshape(B // N, N).sum(axis=1), N))
        assert np.array_equal(stats[:, 4], np.where(c['params'][:, 0] != 0, np.repeat(c['prjl2'][::N], N), 0).astype(np.float64))
        want = np.zeros((B, ncls), dtype=np.float32)
        want[np.arange(B), c['target']] = np.where(c['targeted'], -ADV_SCALE, ADV_SCALE)
        assert np.array_equal(o['seeds'].cpu().numpy(), want)


@pytest.mark.parametrize('BN,ncls,HW,rate', [((6, 3), 1000, 3120, 0.5), ((64, 64), 1000, 65537, 1.0), ((4, 2), 10, 1, 1.0), ((5, 5), 10, 3120, 0.5)])
def test_member_rows_are_decide_ps_bitwise(lib, BN, ncls, HW, rate):
    """The same inputs through spaa_decide_ps: each sample's top-1, p1, target logit, caml2, camdE and seed row, bit for bit."""
    c = uc.decide_case(BN, ncls, HW, rate)
    B = c['B']
    o = run_decide(lib, c, False)
    i = decide_inputs(c)
    state = torch.full((B, 4), -7, dtype=torch.int32, device=DEV)
    stats = torch.full((B, 8), -7.0, device=DEV)
    stats[:, 5] = _dev(c['col_best'])
    seed = torch.full((B, ncls), -7.0, device=DEV)
    p = lib.ptr
    lib.call('spaa_decide_ps', p(i['logits']), ncls, p(i['target']), p(i['partial']), c['nblk'], HW, p(i['prjl2']), p(i['params']),
             p(i['flags']), P_THRESH, ADV_SCALE, p(state), p(stats), p(seed), B)
    torch.cuda.synchronize()
    assert torch.equal(o['uni_state'][:, 1], state[:, 3]) and torch.equal(o['uni_state'][:, 0] & 1, state[:, 0])
    assert torch.equal(o['uni_stats'][:, 0], stats[:, 0]) and torch.equal(o['uni_stats'][:, 1], stats[:, 6])
    assert torch.equal(o['uni_stats'][:, 2], stats[:, 1]) and torch.equal(o['uni_stats'][:, 3], stats[:, 2])
    assert torch.equal(o['seeds'], seed) and (o['uni_stats'] != -7.0).all()


def test_decide_universal_refuses_bad_arguments(lib):
    """Every bad argument returns hipErrorInvalidValue (1) and leaves every sentinel in place: nothing was launched."""
    c = uc.decide_case((6, 3), 10, 3120, 0.5)
    i = decide_inputs(c)
    fn = getattr(lib.load(), 'spaa_decide_universal')
    pointers = ('logits', 'target', 'partial', 'params', 'flags', 'state', 'stats', 'uni_state', 'uni_stats', 'uni_w', 'g_logits')
    bad = [{name: None} for name in pointers]
    bad += [dict(N=1, need=1), dict(N=65, need=65), dict(N=0, need=1), dict(N=4), dict(N=4, need=2), dict(need=0), dict(need=4), dict(need=-1),
            dict(B=65536, N=2, need=2), dict(B=0), dict(HW=0, nblk=0), dict(HW=-5), dict(nblk=12), dict(nblk=14), dict(nblk=1), dict(ncls=0)]
    for over in bad:
        o = decide_outputs(c)
        before = {k: v.clone() for k, v in o.items()}
        rc = fn(*decide_args(lib, c, i, o, False, **over), lib._stream())
        torch.cuda.synchronize()
        assert rc == 1, over
        assert all(torch.equal(o[k], before[k]) for k in o), over
    o = decide_outputs(c)                                                    # (prjl2 alone may be missing: it reads as 0)
    assert fn(*decide_args(lib, c, i, o, False, prjl2=None), lib._stream()) == 0
    torch.cuda.synchronize()
    assert (o['stats'][:, 4] == 0).all() and (o['state'] != -7).all()
    with pytest.raises(RuntimeError, match='spaa_decide_universal failed with HIP error 1$'):
        lib.call('spaa_decide_universal', *decide_args(lib, c, i, decide_outputs(c), False, need=0))


def run_combine(lib, g, w, state, N, HW):
    B = w.shape[0]
    nblk = (HW + 255) // 256
    g_dev, w_dev, state_dev = _dev(g), _dev(w), _dev(state, torch.int32)
    partial = torch.full((B, nblk), -7.0, device=DEV)
    coef = torch.full((B,), -7.0, device=DEV)
    out = torch.full((B, HW, 4), -7.0, device=DEV)
    lib.call('spaa_universal_combine', lib.ptr(g_dev), N, lib.ptr(w_dev), lib.ptr(state_dev), lib.ptr(partial), lib.ptr(coef), lib.ptr(out),
             B, HW)
    torch.cuda.synchronize()
    assert torch.equal(g_dev, _dev(g))                                       # (the members' images are not written)
    return out


@pytest.mark.parametrize('HW', uc.COMBINE_HW)
@pytest.mark.parametrize('N', uc.COMBINE_N)
def test_universal_combine_against_float64(lib, N, HW):
    g, w, state = uc.combine_case(N, HW, seed=10 * HW + N)
    out = run_combine(lib, g, w, state, N, HW)
    got = out.cpu().numpy().astype(np.float64)
    want, mag = uo.combine_universal(g, w, state[:, 1] != 0, N)
    bar = uo.combine_bar(N, HW)
    err = np.abs(got - want)[..., :3]
    worst = (err / np.where(mag > 0, mag, 1.0)).reshape(3, -1).max(axis=1)
    print(f'N {N} HW {HW}: error relative to the sum of the terms\' magnitudes, per group {worst.tolist()}, bar {bar:.2e}')
    assert (err <= bar * mag).all() and (got[..., 3] == 0).all()
    assert np.abs(want).max(axis=(1, 2)).min() > 0
    rows = out.reshape(3, N, HW, 4)
    assert torch.equal(rows, rows[:, :1].expand_as(rows))                    # the N rows of a group are bitwise equal
    assert torch.equal(run_combine(lib, g, w, state, N, HW), out)            # two runs are bitwise equal
    if N == 2:   # two equal members on the colour step: (g + g) * 0.5 is g
        twin = g.copy()
        twin[1::2] = twin[0::2]
        got2 = run_combine(lib, twin, w, state, N, HW).cpu().numpy()
        assert np.array_equal(got2[2, :, :3], twin[2, :, :3]) and np.array_equal(got2[3], got2[2]) and (got2[..., 3] == 0).all()


def test_universal_combine_refuses_bad_arguments(lib):
    """Every bad argument returns hipErrorInvalidValue (1) and leaves every sentinel in place: nothing was launched."""
    N, HW = 3, 257
    g, w, state = uc.combine_case(N, HW, seed=1)
    B = w.shape[0]
    g_dev, w_dev, state_dev = _dev(g), _dev(w), _dev(state, torch.int32)
    fn = getattr(lib.load(), 'spaa_universal_combine')
    names = ('g', 'N', 'uni_w', 'state', 'partial', 'coef', 'g_out', 'B', 'HW')
    bad = [{name: None} for name in ('g', 'uni_w', 'state', 'partial', 'coef', 'g_out')]
    bad += [dict(N=1), dict(N=65), dict(N=0), dict(N=2), dict(N=4), dict(B=65536, N=2), dict(B=0), dict(HW=0), dict(HW=-1)]
    for over in bad:
        partial, coef = torch.full((B, 2), -7.0, device=DEV), torch.full((B,), -7.0, device=DEV)
        out = torch.full((B, HW, 4), -7.0, device=DEV)
        a = dict(zip(names, (lib.ptr(g_dev), N, lib.ptr(w_dev), lib.ptr(state_dev), lib.ptr(partial), lib.ptr(coef), lib.ptr(out), B, HW)))
        assert set(over) <= set(a)
        a.update(over)
        rc = fn(*a.values(), lib._stream())
        torch.cuda.synchronize()
        assert rc == 1, over
        assert (partial == -7.0).all() and (coef == -7.0).all() and (out == -7.0).all(), over
