"""GPU: the ensemble entry points (csrc/group_ops.hip) one by one against their float64 restatement (tests/ensemble_oracle.py):
spaa_decide_ens on planted logits that hold every decision case, and spaa_ens_sumsq + spaa_ens_combine on gradient images with a
zero member, a zero weight, garbage in the pad channel and magnitudes 1e6 apart."""
import ctypes as C

import numpy as np
import pytest
import torch

import ensemble_oracle as eo
from test_gpu_parity import hip  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
P_THRESH = 0.9
HW_IMG = 64 * 64


def _planted(K, ncls, variant, seed):
    """B = 3 samples x K members of logits (float32 values) with planted decisions.  Noise in [-0.5, 0.5]; `hit` lifts a class 12
    above it (top-1 with p1 > 0.99), `weak` 2.5 above it (top-1 with p1 far below P_THRESH), so every planted top-2 gap is >= 1.5.
    variant 0:  sample 0 targeted: member 0 top-1 right but p1 below p_thresh, member 1 fooled, member 2 wrong  (some fooled)
                sample 1 untargeted: every member fooled, caml2 below d_thr; member 0 through an exact tie that the first maximum decides
                sample 2 targeted: every member fooled, caml2 above d_thr
    variant 1:  sample 0 targeted: no member fooled (wrong top-1s, and one right with p1 below p_thresh)
                sample 1 untargeted: no member fooled (every top-1 is the true class; member 1 through an exact tie that it wins)
                sample 2 untargeted: every member fooled, caml2 above d_thr, col not below its best so far"""
    rng = np.random.default_rng(seed)
    lg = (rng.random((K, 3, ncls)) - 0.5).astype(np.float32)
    target = np.array([5, 20, 33])
    other = np.array([9, 3, 30])                 # a class that is not the target (3 < 20: the tie of variant 0 is won by 3)
    hit, weak = np.float32(12.0), np.float32(2.5)
    if variant == 0:
        targeted = [True, False, True]
        lg[0, 0, target[0]] = weak
        lg[1, 0, target[0]] = hit
        if K > 2:
            lg[2:, 0, other[0]] = hit
        lg[:, 1, other[1]] = hit
        lg[0, 1, target[1]] = hit                # member 0: classes 3 and 20 tie exactly; the first maximum, 3, is not the true class
        lg[:, 2, target[2]] = hit
        caml2_over_thr = [1.2, 0.8, 1.2]
        col_best = [1e6, 1e6, 1e6]
    else:
        targeted = [True, False, False]
        lg[:, 0, other[0]] = hit
        lg[0, 0, other[0]] = lg[0, 0, other[0]] - hit   # (back to noise)
        lg[0, 0, target[0]] = weak
        lg[:, 1, target[1]] = hit
        lg[1, 1, 25] = hit                       # member 1: classes 20 and 25 tie exactly; the first maximum, 20, is the true class
        lg[:, 2, other[2]] = hit
        caml2_over_thr = [1.2, 1.2, 1.2]
        col_best = [1e6, 1e6, 1e-6]
    return lg, target, targeted, caml2_over_thr, col_best


@pytest.mark.parametrize('focus', [0, 1])
@pytest.mark.parametrize('variant', [0, 1])
@pytest.mark.parametrize('ncls', [37, 1000])
@pytest.mark.parametrize('K', [2, 3])
def test_decide_ens_against_float64(hip, K, ncls, variant, focus):
    lib = hip['lib']
    p = lib.ptr
    B, HW = 3, HW_IMG
    nblk = (HW + 255) // 256
    lg, target, targeted, over, col_best = _planted(K, ncls, variant, seed=10 * K + variant)
    g = torch.Generator().manual_seed(K + ncls)
    partial = (torch.rand(B, nblk, 3, generator=g) * 256 * 0.05).float()
    caml2 = partial[:, :, 0].double().sum(1).numpy() / HW
    camdE = partial[:, :, 1].double().sum(1).numpy() / HW
    d_thr = np.array([caml2[b] * 255 / over[b] for b in range(B)], dtype=np.float32)     # caml2 * 255 = over * d_thr: 20 % either side
    w = np.array([[0.1, 1.0, 1.0], [0.0, 1.0, 0.0], [0.0, 1.0, 1.0]], dtype=np.float32)     # (prjl2_w, caml2_w, camdE_w) per sample
    prjl2 = np.array([0.25, 0.5, 0.75], dtype=np.float32)
    pl2 = np.where(w[:, 0] != 0, prjl2, 0.0)
    col = w[:, 0].astype(np.float64) * pl2 + w[:, 1] * caml2 + w[:, 2] * camdE
    ref = eo.decide_ens(list(lg.astype(np.float64)), target, targeted, caml2, d_thr.astype(np.float64), P_THRESH, bool(focus), col=col,
                        col_best=col_best)
    # the planted cases are there, and none is near a tie (but the exact ones)
    srt = np.sort(lg.astype(np.float64), axis=2)
    gap = (srt[..., -1] - srt[..., -2]).T                      # [B][K]
    exact_tie = gap == 0
    assert exact_tie.sum() == 1 and (gap[~exact_tie] >= 0.5).all() and (np.abs(ref['p1'] - P_THRESH) >= 0.05).all()
    nf = ref['nfooled'].tolist()
    if variant == 0:
        assert nf == [1, K, K] and ref['best_adv'].tolist() == [False, False, True] and ref['best'].tolist() == [False, False, True]
        assert ref['succ'][0, 0] and not ref['fooled'][0, 0]   # top-1 right, p1 below p_thresh
        assert ref['top1'][1, 0] == 3                          # the tie's first maximum
        assert ref['ens_w'].tolist() == ([[0.0 if (focus and k == 1) else 1.0 for k in range(K)]] + [[1.0] * K] * 2)
    else:
        assert nf == [0, 0, K] and ref['best_adv'].tolist() == [False, False, True] and ref['best'].tolist() == [False, False, False]
        assert ref['succ'][0].tolist() == [True] + [False] * (K - 1) and ref['top1'][1, 1] == 20
        assert (ref['ens_w'] == 1).all()

    logits = [torch.from_numpy(lg[k]).to(DEV) for k in range(K)]
    tgt = torch.from_numpy(target.astype(np.int32)).to(DEV)
    params = torch.from_numpy(np.concatenate([w, d_thr[:, None]], axis=1)).to(DEV).contiguous()
    flags = torch.tensor([int(t) for t in targeted], dtype=torch.int32, device=DEV)
    part_d, prjl2_d = partial.to(DEV), torch.from_numpy(prjl2).to(DEV)

    def launch():
        state = torch.full((B, 4), -7, dtype=torch.int32, device=DEV)
        stats = torch.full((B, 8), -7.0, device=DEV)
        stats[:, 5] = torch.tensor(col_best, dtype=torch.float32)
        es, ef, ew = (torch.full((B, K, 2), -7, dtype=torch.int32, device=DEV), torch.full((B, K, 2), -7.0, device=DEV),
                      torch.full((B, K), -7.0, device=DEV))
        gl = [torch.full((B, ncls), 7.0, device=DEV) for _ in range(K)]
        lib.call('spaa_decide_ens', lib.ptr_array(logits), K, ncls, p(tgt), p(part_d), nblk, HW, p(prjl2_d), p(params), p(flags),
                 P_THRESH, focus, p(state), p(stats), p(es), p(ef), p(ew), lib.ptr_array(gl), B)
        return state.cpu().numpy(), stats.cpu().numpy(), es.cpu().numpy(), ef.cpu().numpy(), ew.cpu().numpy(), [t.cpu().numpy() for t in gl]

    state, stats, es, ef, ew, gl = launch()
    # integer outputs and weights: exact
    assert np.array_equal(es, ref['ens_state']) and np.array_equal(ew, ref['ens_w'])
    want_state = np.stack([ref['state_succ'], ref['best_adv'], ref['best'], ref['nfooled']], axis=1).astype(np.int64)
    assert np.array_equal(state, want_state), (state, want_state)
    # p1: the arithmetic of spaa_decide (expf, a 256-way strided sum, a block sum, one division): 4 ulp-sized steps of float64's value
    e_p1 = np.abs(ef[..., 0] - ref['p1']) / ref['p1']
    print(f'decide_ens K {K} ncls {ncls}: p1 max rel error {e_p1.max():.2e}')
    assert (e_p1 <= 5e-7).all()
    assert np.array_equal(ef[..., 1].astype(np.float64), ref['tl'])                      # (a copy of a float32 logit)
    assert np.array_equal(stats[:, 0], ef[..., 0].min(axis=1))
    # mean target logit: K - 1 additions and one division in fp32, each within 2^-24 of the sum of magnitudes
    assert (np.abs(stats[:, 6] - ref['tl_mean']) <= K * 2.0 ** -24 * np.abs(ref['tl']).sum(axis=1)).all()
    # the loss columns are spaa_decide's (nblk strided additions, a block sum, a division, up to three multiply-adds)
    for c, want in ((1, caml2), (2, camdE), (3, col), (4, pl2)):
        assert np.allclose(stats[:, c], want, rtol=2e-6, atol=0), (c, stats[:, c], want)
    want5 = np.where(ref['best'], stats[:, 3], np.asarray(col_best, dtype=np.float32))
    assert np.array_equal(stats[:, 5], want5) and (stats[:, 7] == -7).all()
    # seeds: exact
    for k in range(K):
        want = np.zeros((B, ncls), dtype=np.float32)
        want[np.arange(B), target] = np.where(targeted, -1.0, 1.0)
        assert np.array_equal(gl[k], want), k
    # run to run
    again = launch()
    assert all(np.array_equal(a, b) for a, b in zip((state, stats, es, ef, ew), again[:5]))

    # K members fed the SAME logits: each member's row is bitwise what spaa_decide_ps writes for that sample
    for m in range(K):
        same = [logits[m]] * K
        state1 = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
        stats1 = torch.zeros(B, 8, device=DEV)
        stats1[:, 5] = torch.tensor(col_best, dtype=torch.float32)
        gl1 = torch.zeros(B, ncls, device=DEV)
        lib.call('spaa_decide_ps', p(logits[m]), ncls, p(tgt), p(part_d), nblk, HW, p(prjl2_d), p(params), p(flags), P_THRESH, 1.0,
                 p(state1), p(stats1), p(gl1), B)
        state2 = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
        stats2 = stats1.clone()
        stats2[:, 5] = torch.tensor(col_best, dtype=torch.float32)
        es2, ef2, ew2 = (torch.zeros(B, K, 2, dtype=torch.int32, device=DEV), torch.zeros(B, K, 2, device=DEV), torch.zeros(B, K, device=DEV))
        gl2 = [torch.zeros(B, ncls, device=DEV) for _ in range(K)]
        lib.call('spaa_decide_ens', lib.ptr_array(same), K, ncls, p(tgt), p(part_d), nblk, HW, p(prjl2_d), p(params), p(flags),
                 P_THRESH, focus, p(state2), p(stats2), p(es2), p(ef2), p(ew2), lib.ptr_array(gl2), B)
        for k in range(K):
            assert torch.equal(ef2[:, k, 0], stats1[:, 0]) and torch.equal(ef2[:, k, 1], stats1[:, 6]), (m, k)     # p1, target logit
            assert torch.equal(es2[:, k, 1], state1[:, 3]) and torch.equal(es2[:, k, 0] & 1, state1[:, 0]), (m, k)  # top1, succ
            assert torch.equal(gl2[k], gl1)                                                                         # (adv_scale 1)
        # identical members are fooled together: the sample's flags and loss columns are the single decision's as well
        assert torch.equal(state2[:, :3], state1[:, :3]) and torch.equal(stats2[:, :6], stats1[:, :6]), m


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def test_decide_ens_refuses_other_member_counts(hip):
    lib = hip['lib']
    raw = lib.load()
    B, ncls, HW = 2, 37, 256
    lg = [torch.zeros(B, ncls, device=DEV) for _ in range(5)]
    gl = [torch.full((B, ncls), 7.0, device=DEV) for _ in range(5)]
    tgt = torch.zeros(B, dtype=torch.int32, device=DEV)
    part, params, flags = torch.zeros(B, 1, 3, device=DEV), torch.ones(B, 4, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    out = [torch.full((B, 4), -7, dtype=torch.int32, device=DEV), torch.full((B, 8), -7.0, device=DEV),
           torch.full((B, 5, 2), -7, dtype=torch.int32, device=DEV), torch.full((B, 5, 2), -7.0, device=DEV), torch.full((B, 5), -7.0, device=DEV)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for K in (0, 1, 5):
        rc = raw.spaa_decide_ens(_ptrs(lg[:max(K, 1)]), K, ncls, tgt.data_ptr(), part.data_ptr(), 1, HW, None, params.data_ptr(),
                                 flags.data_ptr(), 0.9, 0, *[t.data_ptr() for t in out], _ptrs(gl[:max(K, 1)]), B, stream)
        assert rc != 0, K
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in out) and all((t == 7).all() for t in gl)


def _gradient_images(K, HW, seed):
    """B = 3 samples x K members [HW][4] float32: member k scaled by 1e3^k-ish so that the members' magnitudes differ by up to 1e6
    (K = 2: 1e-3 and 1e3), the pad channel NaN / 1e30 / -1e30, member 1 of sample 1 all zero; weights with one 0."""
    rng = np.random.default_rng(seed)
    scales = {2: [1e-3, 1e3], 4: [1e-3, 1.0, 37.0, 1e3]}[K]
    gs = [(rng.standard_normal((3, HW, 4)) * s).astype(np.float32) for s in scales]
    for k, g in enumerate(gs):
        g[..., 3] = (np.nan, 1e30, -1e30)[k % 3]
    gs[1][1, :, :3] = 0.0
    w = np.ones((3, K), dtype=np.float32)
    w[2, K - 1] = 0.0
    return gs, w


@pytest.mark.parametrize('K', [2, 4])
@pytest.mark.parametrize('HW', [35, 2240])
def test_sumsq_and_combine_against_float64(hip, K, HW):
    """Per sample max |out - ref| <= 2e-6 max |ref|.  The sum of squares passes at most 3 (a pixel's channels) + 8 (wave and block sum)
    + ceil(nblk / 256) + 8 (the re-reduction) rounding steps of 2^-24 relative each, about 1.2e-6, halved by the square root; the
    division by the norm, the weight and the addition add 3 roundings per member."""
    lib = hip['lib']
    p = lib.ptr
    B = 3
    nblk = (HW + 255) // 256
    gs, w = _gradient_images(K, HW, seed=K * HW)
    ref = eo.combine([g.astype(np.float64) for g in gs], w)
    n_ref = np.stack([eo.unit_images(g)[1] for g in gs], axis=1)                        # [B][K]
    assert n_ref[1, 1] == 0 and n_ref.max() / n_ref[n_ref > 0].min() > 1e5
    gd = [torch.from_numpy(g).to(DEV) for g in gs]
    wd = torch.from_numpy(w).to(DEV)

    def launch():
        part = torch.full((B, K, nblk), 3.0, device=DEV)
        out = torch.full((B, HW, 4), 3.0, device=DEV)
        lib.call('spaa_ens_sumsq', lib.ptr_array(gd), K, p(part), B, HW)
        lib.call('spaa_ens_combine', lib.ptr_array(gd), K, p(part), nblk, p(wd), p(out), B, HW)
        return part.cpu().numpy(), out.cpu().numpy()

    part, out = launch()
    assert np.isfinite(part).all() and np.isfinite(out).all()                           # (the pad channel's garbage went nowhere)
    assert np.allclose(np.sqrt(part.astype(np.float64).sum(axis=2)), n_ref, rtol=1e-6, atol=0)
    assert (out[..., 3] == 0).all()
    err = np.abs(out[..., :3] - ref[..., :3]).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))
    print(f'ens_combine K {K} HW {HW}: max |out - ref| / max |ref| per sample {err.tolist()}')
    assert (err <= 2e-6).all()
    # sample 1 without its zero member, sample 2 without its zero-weight member: exactly the remaining members' sum
    assert np.abs(ref[1]).max() > 0
    part2, out2 = launch()
    assert np.array_equal(part, part2) and np.array_equal(out, out2)


def test_sumsq_and_combine_refuse_other_member_counts(hip):
    lib = hip['lib']
    raw = lib.load()
    B, HW = 2, 35
    g = [torch.ones(B, HW, 4, device=DEV) for _ in range(5)]
    part = torch.full((B, 5, 1), 3.0, device=DEV)
    out = torch.full((B, HW, 4), 3.0, device=DEV)
    w = torch.ones(B, 5, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for K in (1, 5):
        assert raw.spaa_ens_sumsq(_ptrs(g[:K]), K, part.data_ptr(), B, HW, stream) != 0
        assert raw.spaa_ens_combine(_ptrs(g[:K]), K, part.data_ptr(), 1, w.data_ptr(), out.data_ptr(), B, HW, stream) != 0
        with pytest.raises(RuntimeError, match='spaa_ens_sumsq failed'):
            lib.call('spaa_ens_sumsq', _ptrs(g[:K]), K, lib.ptr(part), B, HW)
    assert raw.spaa_ens_combine(_ptrs(g[:2]), 2, part.data_ptr(), 2, w.data_ptr(), out.data_ptr(), B, HW, stream) != 0   # (nblk is not ceil(HW / 256))
    torch.cuda.synchronize()
    assert (part == 3).all() and (out == 3).all()
