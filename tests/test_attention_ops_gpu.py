"""GPU: the attention kernels (csrc/attention_ops.hip) alone against their float64 restatement (tests/attention_oracle.py):
spaa_cam_alpha + spaa_cam_map on planted feature maps and gradients, spaa_attention_apply on gradient images with garbage in the pad
channel and outside the crop.  B = 3 samples per case, drawn from four planted kinds: a targeted sample (negative seed), an untargeted
one (positive seed), one whose every sum_k alpha A is negative and one whose seed is 0 -- the last two must get their gradient image
back bit for bit.

Tolerances are derived, not measured (attention_oracle.bound_c / tol_map / tol_image): with S = sum_k |alpha_k A_k| of the oracle,
|c - c_ref| <= 2 (C + h w) 2^-24 S; M may differ by twice that over the reference maximum plus 4 * 2^-24; a weighted value by
|g| (1 - floor) times that plus 4 * 2^-24 |g W|.  The planted maxima are at least S / 16 (checked on the CPU, without a GPU), so the
bound on M stays below 32 (C + h w) 2^-24."""
import numpy as np
import pytest
import torch

import attention_oracle as ao

DEV = 'cuda'
NCLS = 37
TARGET = [5, 20, 33]
KINDS_A, KINDS_B = ('neg', 'pos', 'allneg'), ('pos', 'zero', 'neg')
# (h, w, C), camera, crop, the three samples' kinds, the gradient as g_pooled (else as a map), floor, channel stride of the map
CASES = [((1, 1, 8), (24, 32), (20, 20), KINDS_A, False, 0.0, 8),
         ((1, 1, 8), (16, 16), (16, 16), KINDS_B, True, 0.25, 8),
         ((2, 3, 12), (24, 32), (20, 20), KINDS_B, False, 0.25, 16),
         ((2, 3, 12), (16, 16), (16, 16), KINDS_A, True, 0.0, 12),
         ((7, 7, 512), (24, 32), (20, 20), KINDS_A, True, 0.1, 512),
         ((7, 7, 512), (16, 16), (16, 16), KINDS_B, False, 0.0, 512),
         ((8, 8, 2048), (24, 32), (20, 20), KINDS_B, True, 0.0, 2048),
         ((8, 8, 2048), (16, 16), (16, 16), KINDS_A, False, 0.5, 2048),
         ((8, 8, 2048), (8, 10), (6, 6), KINDS_A, False, 0.25, 2048),          # down-sampling: 8 x 8 features onto a 6 x 6 crop
         ((32, 32, 8), (40, 40), (36, 36), KINDS_B, False, 0.0, 8)]            # h w = 1024
IDS = [f'{s[0]}x{s[1]}x{s[2]}-cam{c[0]}x{c[1]}-crop{k[0]}-{"pooled" if p else "map"}' for s, c, k, _, p, _, _ in CASES]


def planted(case):
    """fp32 inputs of a case and their oracle.  A in [0.05, 1]; a sample's channel weights have magnitudes in [0.5, 1.5], every fourth
    one negative (`allneg`: all of them); its gradient map is sign(seed) alpha (1 + 0.25 r), r in [-1, 1], so that no channel's
    spatial mean cancels.  With `pooled` the kernel gets g_pooled = h w mean G in fp32, and the oracle the map that this stands for."""
    (h, w, C), cam_hw, crop, kinds, pooled, floor, cstride = case
    rng = np.random.default_rng(h * 1000 + C + cam_hw[0])
    B, hw = 3, h * w
    A = rng.uniform(0.05, 1.0, (B, h, w, C)).astype(np.float32)
    seed = np.array([{'neg': -1 / 3, 'pos': 1 / 3, 'allneg': 1 / 3, 'zero': 0.0}[k] for k in kinds], dtype=np.float32)
    alpha = rng.uniform(0.5, 1.5, (B, C))
    alpha[:, 3::4] *= -1
    for b, k in enumerate(kinds):
        if k == 'allneg':
            alpha[b] = -np.abs(alpha[b])
    sgn = np.where(seed == 0, 1.0, np.sign(seed))
    Gbuf = rng.normal(size=(B, h, w, cstride)).astype(np.float32)             # (channels past C: garbage that nobody may read)
    Gbuf[..., :C] = (sgn[:, None, None, None] * alpha[:, None, None, :] * (1 + 0.25 * rng.uniform(-1, 1, (B, h, w, C)))).astype(np.float32)
    g_logits = rng.normal(size=(B, NCLS)).astype(np.float32)
    g_logits[np.arange(B), TARGET] = seed
    g_pooled = Gbuf[..., :C].astype(np.float64).sum(axis=(1, 2)).astype(np.float32)
    G_ref = np.broadcast_to((g_pooled.astype(np.float64) / hw)[:, None, None, :], A.shape) if pooled else Gbuf[..., :C]
    ref = ao.cam(A, G_ref, seed)
    H, W = cam_hw
    g_y = rng.normal(size=(B, H, W, 4)).astype(np.float32)                    # (pad channel and the pixels outside the crop: garbage)
    return dict(A=A, Gbuf=Gbuf, g_pooled=g_pooled, g_logits=g_logits, seed=seed, g_y=g_y, ref=ref, M=ao.camera_map(ref['m'], cam_hw, crop))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_planted_cases_are_well_conditioned(case):
    """CPU: every kind is what its name says, and a live sample's maximum is at least S / 16 there."""
    p, kinds = planted(case), case[3]
    ref = p['ref']
    for b, k in enumerate(kinds):
        if k in ('neg', 'pos'):
            i = np.unravel_index(ref['c'][b].argmax(), ref['c'][b].shape)
            assert ref['cmax'][b] > 0 and ref['cmax'][b] >= ref['S'][b][i] / 16 and ref['m'][b].max() == 1.0
            assert np.sign(p['seed'][b]) == (-1 if k == 'neg' else 1)
        elif k == 'allneg':
            assert (ref['pre'][b] < 0).all() and ref['cmax'][b] == 0 and (ref['m'][b] == 1).all() and p['seed'][b] != 0
        else:
            assert p['seed'][b] == 0 and (ref['alpha'][b] == 0).all() and (ref['m'][b] == 1).all()
    assert {k for c in CASES for k in c[3]} == {'neg', 'pos', 'allneg', 'zero'}


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    _lib.load()
    return _lib


def _cam_launch(lib, p, case):
    (h, w, C), _, _, _, pooled, _, cstride = case
    B, hw, ptr = 3, h * w, lib.ptr
    A, g_logits = torch.from_numpy(p['A']).to(DEV), torch.from_numpy(p['g_logits']).to(DEV)
    target = torch.tensor(TARGET, dtype=torch.int32, device=DEV)
    c, cmax = torch.full((B, hw), -7.0, device=DEV), torch.full((B,), -7.0, device=DEV)
    if pooled:
        alpha, scale = torch.from_numpy(p['g_pooled']).to(DEV), 1.0 / hw
    else:
        G = torch.from_numpy(p['Gbuf']).to(DEV)
        alpha, scale = torch.full((B, C), -7.0, device=DEV), 1.0
        lib.call('spaa_cam_alpha', ptr(G), ptr(alpha), B, hw, C, cstride)
    lib.call('spaa_cam_map', ptr(A), ptr(alpha), scale, ptr(g_logits), NCLS, ptr(target), ptr(c), ptr(cmax), B, hw, C)
    return alpha, c, cmax


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_kernels_against_the_oracle(lib, case):
    (h, w, C), (H, W), crop, kinds, pooled, floor, cstride = case
    p = planted(case)
    ref, B, ptr = p['ref'], 3, lib.ptr
    alpha, c, cmax = _cam_launch(lib, p, case)
    _, c2, cmax2 = _cam_launch(lib, p, case)
    assert torch.equal(c, c2) and torch.equal(cmax, cmax2)                     # a run is bitwise repeatable
    live = np.array([k in ('neg', 'pos') for k in kinds])
    if not pooled:   # the channel means: h w additions and one division
        a = alpha.cpu().numpy().astype(np.float64) * np.where(p['seed'] == 0, 0, np.sign(p['seed']))[:, None]
        assert (np.abs(a - ref['alpha'])[live] <= (h * w + 1) * ao.U * np.abs(ref['alpha'])[live]).all()
    cg, mg = c.cpu().numpy().astype(np.float64).reshape(B, h, w), cmax.cpu().numpy().astype(np.float64)
    bc = ao.bound_c(ref, C)
    err = np.abs(cg - ref['c'])
    print(f'c: worst error / bound {np.max(err[live] / bc[live]):.3e}; bound / reference maximum {bc[live].max(axis=(1, 2)) / ref["cmax"][live]}')
    assert (err <= bc).all() and (np.abs(mg - ref['cmax']) <= bc.reshape(B, -1).max(axis=1)).all()
    assert (cg[~live] == 0).all() and (mg[~live] == 0).all() and (cg >= 0).all()
    # the weighting, with the map written alongside
    cy0, cx0 = ao.center_crop_origin(H, W, crop)
    geo = (B, H, W, cy0, cx0, crop[0], crop[1], h, w)
    g0 = torch.from_numpy(p['g_y']).to(DEV)
    g1, M1 = g0.clone(), torch.full((B, H, W), -7.0, device=DEV)
    lib.call('spaa_attention_apply', ptr(c), ptr(cmax), floor, ptr(g1), ptr(M1), *geo)
    g2, M3 = g0.clone(), torch.full((B, H, W), -7.0, device=DEV)
    lib.call('spaa_attention_apply', ptr(c), ptr(cmax), floor, ptr(g2), None, *geo)
    lib.call('spaa_attention_apply', ptr(c), ptr(cmax), floor, None, ptr(M3), *geo)
    assert torch.equal(g1, g2) and torch.equal(M1, M3)
    inside = np.zeros((H, W), dtype=bool)
    inside[cy0:cy0 + crop[0], cx0:cx0 + crop[1]] = True
    Mg, gg = M1.cpu().numpy().astype(np.float64), g1.cpu().numpy()
    tm = ao.tol_map(ref, bc)
    errM = np.abs(Mg - p['M']).reshape(B, -1).max(axis=1)
    print(f'M: worst error {errM.tolist()}, tolerance {tm.tolist()}')
    assert (errM <= tm).all() and (Mg[:, ~inside] == 0).all() and (Mg[~live][:, inside] == 1).all() and Mg.max() <= 1.0 and Mg.min() >= 0.0
    want, wgt = ao.apply(p['g_y'], p['M'], floor, crop)
    ti = ao.tol_image(p['g_y'], wgt, floor, tm)
    errg = np.abs(gg[..., :3].astype(np.float64) - want[..., :3])
    print(f'g_y: worst error / tolerance {np.max(errg[live] / ti[live]):.3e}')
    assert (errg <= ti).all()
    assert np.array_equal(gg[..., 3], p['g_y'][..., 3])                        # garbage in the pad channel survives
    assert np.array_equal(gg[:, ~inside], p['g_y'][:, ~inside])                # nothing outside the crop is written
    assert np.array_equal(gg[~live], p['g_y'][~live])                          # m = 1: bit for bit
    # floor = 1 is the identity, bit for bit, for every sample
    g4 = g0.clone()
    lib.call('spaa_attention_apply', ptr(c), ptr(cmax), 1.0, ptr(g4), None, *geo)
    assert torch.equal(g4, g0)


@pytest.mark.gpu
def test_a_target_that_is_no_class_counts_as_a_zero_seed(lib):
    case = CASES[2]
    p = planted(case)
    (h, w, C) = case[0]
    ptr = lib.ptr
    A, gl = torch.from_numpy(p['A']).to(DEV), torch.from_numpy(p['g_logits']).to(DEV)
    alpha = torch.from_numpy(p['g_pooled']).to(DEV)
    c, cmax = torch.full((3, h * w), -7.0, device=DEV), torch.full((3,), -7.0, device=DEV)
    target = torch.tensor([-1, NCLS, 1 << 30], dtype=torch.int32, device=DEV)
    lib.call('spaa_cam_map', ptr(A), ptr(alpha), 1.0, ptr(gl), NCLS, ptr(target), ptr(c), ptr(cmax), 3, h * w, C)
    assert (c == 0).all() and (cmax == 0).all()


@pytest.mark.gpu
def test_refused_arguments(lib):
    """hipErrorInvalidValue (a RuntimeError from the binding) before any launch."""
    ptr = lib.ptr
    t = torch.zeros(3 * 64 * 16, device=DEV)
    tgt = torch.zeros(3, dtype=torch.int32, device=DEV)
    bad = [('spaa_cam_map', (ptr(t), ptr(t), 1.0, ptr(t), NCLS, ptr(tgt), ptr(t), ptr(t), 3, 4, 6)),          # C % 4 != 0
           ('spaa_cam_map', (ptr(t), ptr(t), 1.0, ptr(t), NCLS, ptr(tgt), ptr(t), ptr(t), 3, 0, 8)),          # no position
           ('spaa_cam_map', (ptr(t), ptr(t), 0.0, ptr(t), NCLS, ptr(tgt), ptr(t), ptr(t), 3, 4, 8)),          # scale not positive
           ('spaa_cam_map', (ptr(t), None, 1.0, ptr(t), NCLS, ptr(tgt), ptr(t), ptr(t), 3, 4, 8)),
           ('spaa_cam_alpha', (ptr(t), ptr(t), 3, 4, 8, 4)),                                                   # stride below C
           ('spaa_cam_alpha', (ptr(t), ptr(t), 3, 0, 8, 8)),
           ('spaa_attention_apply', (ptr(t), ptr(t), 0.0, None, None, 3, 8, 8, 1, 1, 6, 6, 2, 2)),            # nothing to write
           ('spaa_attention_apply', (ptr(t), ptr(t), 1.5, ptr(t), None, 3, 8, 8, 1, 1, 6, 6, 2, 2)),          # floor out of range
           ('spaa_attention_apply', (ptr(t), ptr(t), 0.0, ptr(t), None, 3, 8, 8, 3, 1, 6, 6, 2, 2)),          # crop past the frame
           ('spaa_attention_apply', (ptr(t), ptr(t), 0.0, ptr(t), None, 3, 8, 8, 1, 1, 6, 6, 0, 2))]
    for name, args in bad:
        with pytest.raises(RuntimeError, match=name):
            lib.call(name, *args)
    assert (t == 0).all()
