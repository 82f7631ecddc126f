"""GPU (-m gpu): the PerC-AL step kernels of csrc/perc_al.hip -- spaa_add_nhwc4, spaa_ce_grad, spaa_masked_step, spaa_scale_by_map,
spaa_perc_clamp_quant, spaa_perc_decide, spaa_track_where -- launch by launch through the C ABI against float64, and the loop body
that PerCALState.iteration chains from them (with spaa_grad_sumsq and spaa_stealth_loss_fwd_bwd) against a float64 restatement of
perc_al/__init__.py:179-245 built on the oracle's rgb2lab_diff / ciede2000_diff.

Part 1 runs each kernel alone: B = 3 (spaa_perc_decide: one row per case), HW in {1, 255, 256, 257, 1000} (1, 1, 1, 2, 4 blocks, the
last one ragged or full), ncls in {2, 3, 63, 64, 65, 256, 257, 1000, 1025}.  Every output buffer starts as NaN and carries PAD NaN
rows past its end, which must stay NaN; the fourth lane of an NHWC4 output is 0 where the kernel defines it and untouched where
it does not.  Arg-max ties go to the LOWEST index (the reference's order on ties is unspecified; this is the project's rule).

Part 2 drives PerCALState with a stub classifier: a fixed linear model for the pass that is differentiated (so the gradient is
exact and cheap in float64) and a scripted logit table for the decision pass, which prescribes six lives (LIVES below) in each
of the three modes.  The conditions on the float64 run alone (margins of every threshold comparison, every life present, few
near-tie pixels) are asserted before the GPU is compared with it.

Exact, no tolerance: integers, masks, copies, the add, delta of the clamp (the fp32 expression), quantised values off ties, margins
of dyadic logits, the bound in Part 1, zeros.  Bounds, each at most 4x the largest value measured on an MI355X (in brackets):
  * ce_grad: |err| <= 2e-7 |mult|  [5.38e-8]; each row's |sum| <= 4e-7 |mult|  [1.09e-7]
  * masked_step: |err| <= 1e-6 |step|  [2.69e-7: x itself is O(1) and rounds to 6e-8]
  * scale_by_map: |err| <= 4e-7 max|g_ref| of the sample  [1.08e-7]; color_dis: |err| <= 2e-7 max(1, value)  [5.05e-8]
  * clamp_quant: delta against the float64 expression: |err| <= 2e-7  [5.96e-8 = 2^-24]
  * block partials of clamp_quant and grad_sumsq: |err| <= 2e-7 max(1, sum)  [5.68e-8, 7.96e-8]
  * p1: |err| <= 3e-7  [7.62e-8 in Part 1, 1.65e-7 in the loop]; caml2: |err| <= 1.2e-7 max(1, value)  [3.28e-8, 1.01e-8]
  * the loop's delta: max |err| <= 6e-6 max|delta|  [1.73e-6; with storage='f16' against 'f32': 0]
  * the loop's color_dis and bound: |err| <= 8e-6 max(1, value)  [2.34e-6, 1.92e-6]
The same restatement run in fp32 on the CPU stays within 9.6e-7 (delta) and 1.4e-6 (color_dis) of float64 and takes every decision
alike; the smallest margins of the float64 run are 6.0e-2 (d_thr) and 1.04e-3 (the bound), 116 of 15732 pixels are near ties.
"""
import math

import numpy as np
import pytest
import torch

import spaa_oracle as so

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, F64, I32 = torch.float32, torch.float64, torch.int32
NAN = float('nan')
PAD = 7                       # NaN rows past the end of every output buffer: a kernel must not write them
IPAD = -12345                 # the same for int32 buffers

CE_TOL = 2e-7                 # x |mult|
CE_SUM_TOL = 4e-7             # x |mult|
STEP_TOL = 1e-6               # x |step|
MAP_TOL = 4e-7                # x max |g_ref| of the sample
CD_TOL = 2e-7                 # x max(1, color_dis)
CLAMP_TOL = 2e-7              # absolute (values in [-1, 1])
PART_TOL = 2e-7               # x max(1, block sum)
P1_TOL = 3e-7                 # absolute (p1 <= 1)
CAML2_TOL = 1.2e-7            # x max(1, caml2)
DELTA_TOL = 6e-6              # the loop, x max |delta|
CD_LOOP_TOL = 8e-6            # the loop's color_dis and bound, x max(1, value)

HWS = [1, 255, 256, 257, 1000]
NCLS = [2, 3, 63, 64, 65, 256, 257, 1000, 1025]
B3 = 3

MEASURED = {}


def record(key, v):
    """Largest finite value seen of a metric (non-finite ones fail their own check)."""
    v = torch.as_tensor(v, dtype=F64).reshape(-1)
    v = v[torch.isfinite(v)]
    if v.numel():
        MEASURED[key] = max(MEASURED.get(key, 0.0), float(v.max()))


def bounded(key, v, tol, what=''):
    """Records max(v) under `key`, then asserts that every value is finite and <= tol."""
    v = torch.as_tensor(v, dtype=F64).reshape(-1)
    record(key, v)
    assert torch.isfinite(v).all(), f'{key} {what}: non-finite at {int((~torch.isfinite(v)).sum())} of {v.numel()}'
    worst = float(v.max()) if v.numel() else 0.0
    assert worst <= tol, f'{key} {what}: {worst:.3e} > {tol:.1e} (element {int(v.argmax())})'


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    if MEASURED:
        print('\n[perc_al] largest over this module: ' + ', '.join(f'{k} {v:.2e}' for k, v in sorted(MEASURED.items())))


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    _lib.load()  # raises if the HIP library is missing: there is no fallback
    return _lib


def f32(x):
    """float64 array -> the nearest fp32 values, as float64."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def bits(t):
    return t.contiguous().view(I32)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# device plumbing: host tensors with `PAD` rows of NaN (int32: IPAD) behind them
def padded(t, dtype=None):
    """Host tensor [n, ...] -> device tensor [n + PAD, ...] whose last PAD rows are NaN (IPAD for integers)."""
    t = torch.as_tensor(t)
    t = t.to(dtype if dtype is not None else (I32 if not t.dtype.is_floating_point else F32))
    fill = NAN if t.dtype.is_floating_point else IPAD
    buf = torch.full((t.shape[0] + PAD,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    buf[:t.shape[0]] = t
    return buf.to(DEV)


def nan_buf(n, *rest):
    return torch.full((n + PAD,) + rest, NAN, dtype=F32, device=DEV)


def rows4(x3, lane3):
    """(n, 3) float64 -> (n, 4) fp32 host rows with the fourth lane set to `lane3` (a number or an (n,) tensor)."""
    x3 = torch.as_tensor(x3, dtype=F64)
    out = torch.empty(x3.shape[0], 4, dtype=F32)
    out[:, :3] = x3.to(F32)
    out[:, 3] = lane3
    return out


def unpad(buf, n):
    """Device buffer [n + PAD, ...] -> host [n, ...]; the PAD rows must be untouched."""
    h = buf.cpu()
    tail = h[n:]
    assert (tail.isnan().all() if h.dtype.is_floating_point else (tail == IPAD).all()), 'a row past the end was written'
    return h[:n]


def markers(n):
    """Distinct finite fp32 values for a fourth lane that a kernel must leave alone."""
    return (torch.arange(n, dtype=F64) * 0.25 + 1000.0).to(F32)


def state_rows(col, vals):
    """state [B][4]: column `col` holds `vals`; the other three hold the opposite truth value."""
    st = torch.zeros(len(vals), 4, dtype=I32)
    for b, v in enumerate(vals):
        st[b, :] = 0 if v != 0 else 1
        st[b, col] = v
    return st


# ---------------------------------------------------------------------------------------------------------------------------------
# spaa_add_nhwc4
@pytest.mark.parametrize('HW', HWS)
def test_add_nhwc4(lib, HW):
    n = B3 * HW
    rng = np.random.default_rng([1, HW])
    a, b = f32(rng.uniform(-1, 1, (n, 3))), f32(rng.uniform(-1, 1, (n, 3)) * rng.choice([1.0, 1e-3], (n, 3)))
    ad, bd, out = padded(rows4(a, NAN)), padded(rows4(b, NAN)), nan_buf(n, 4)
    lib.call('spaa_add_nhwc4', lib.ptr(ad), lib.ptr(bd), lib.ptr(out), n)
    h = unpad(out, n)
    assert (h[:, 3] == 0).all(), 'fourth lane not 0'
    assert torch.equal(h[:, :3], torch.from_numpy(a + b).to(F32)), 'not the fp32 rounding of the float64 sum'


# ---------------------------------------------------------------------------------------------------------------------------------
# spaa_ce_grad
def softmax64(l):
    e = np.exp(l - l.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def ce_labels(ncls):
    return [0, ncls - 1, 256 + (ncls - 256) // 2 if ncls > 256 else ncls // 2]


@pytest.mark.parametrize('ncls', NCLS)
def test_ce_grad_vs_fp64(lib, ncls):
    rng = np.random.default_rng([2, ncls])
    labels = ce_labels(ncls)
    if ncls > 256:
        assert labels[2] >= 256
    for variant in ('scale1', 'scale1e4', 'equal_row'):
        l = f32(rng.standard_normal((B3, ncls)) * (1e4 if variant == 'scale1e4' else 1.0))
        if variant == 'equal_row':
            l[1, :] = 3.25
        ref_p = softmax64(l)
        onehot = np.zeros_like(ref_p)
        onehot[np.arange(B3), labels] = 1.0
        ld, lab = padded(l), padded(torch.tensor(labels))
        for mult in (1.0, -1.0, 64.0, -64.0):
            g, g2 = nan_buf(B3, ncls), nan_buf(B3, ncls)
            lib.call('spaa_ce_grad', lib.ptr(ld), ncls, lib.ptr(lab), mult, lib.ptr(g), B3)
            lib.call('spaa_ce_grad', lib.ptr(ld), ncls, lib.ptr(lab), mult, lib.ptr(g2), B3)
            assert bits_equal(g, g2), 'two launches differ'
            gk = unpad(g, B3).to(F64)
            ref = torch.from_numpy(mult * (ref_p - onehot))
            name = f'ncls={ncls} {variant} mult={mult}'
            bounded('ce_grad err/|mult|', (gk - ref).abs() / abs(mult), CE_TOL, name)
            bounded('ce_grad |row sum|/|mult|', gk.sum(dim=1).abs() / abs(mult), CE_SUM_TOL, name)


# ---------------------------------------------------------------------------------------------------------------------------------
# spaa_masked_step
def step_inputs(HW, seed):
    rng = np.random.default_rng([3, HW, seed])
    n = B3 * HW
    nblk = (HW + 255) // 256
    x = f32(rng.uniform(0, 1, (n, 3)))
    g = f32(rng.standard_normal((n, 3)))
    part = f32(rng.uniform(0.5, 1.5, (B3, nblk)) * 3 * min(HW, 256))
    return x, g, part, nblk


def check_step(name, xk, x, g, nrm, stepped, step, HW, x4):
    """xk: host (n, 4) after the launch; stepped samples against float64, skipped ones and the fourth lane bitwise unchanged."""
    assert bits_equal(xk[:, 3], x4[:, 3]), f'{name}: fourth lane of x changed'
    for b in range(len(stepped)):
        sl = slice(b * HW, (b + 1) * HW)
        if stepped[b]:
            ref = torch.from_numpy(x[sl] + step * g[sl] / nrm[b])
            bounded('masked_step err/|step|', (xk[sl, :3].to(F64) - ref).abs() / abs(step), STEP_TOL, f'{name} sample {b}')
        else:
            assert bits_equal(xk[sl], x4[sl]), f'{name}: skipped sample {b} changed'


@pytest.mark.parametrize('HW', HWS)
def test_masked_step_vs_fp64(lib, HW):
    n = B3 * HW
    x, g, part, nblk = step_inputs(HW, 0)
    nrm = np.sqrt(part.sum(axis=1))
    x4 = rows4(x, markers(n))
    gd, pd = padded(rows4(g, NAN)), padded(part.reshape(-1))
    vals = [0, 7, -1]
    for col in range(4):
        for want in (0, 1):
            for step in (0.37, -0.21):
                xd, sd = padded(x4), padded(state_rows(col, vals))
                lib.call('spaa_masked_step', lib.ptr(xd), lib.ptr(gd), lib.ptr(pd), lib.ptr(sd), col, want, step, B3, HW)
                stepped = [(v != 0) == (want != 0) for v in vals]
                check_step(f'HW={HW} col={col} want={want} step={step}', unpad(xd, n), x, g, nrm, stepped, step, HW, x4)
                vals = vals[1:] + vals[:1]


def test_masked_step_with_grad_sumsq_partials(lib):
    """The partial sums really come from spaa_grad_sumsq on the same g (as in the loop): x + step g / ||g||_2."""
    HW = 257
    n = B3 * HW
    x, g, _, nblk = step_inputs(HW, 1)
    x4, g4 = rows4(x, markers(n)), rows4(g, 0.0)
    xd, gd, pd, sd = padded(x4), padded(g4), nan_buf(B3 * nblk), padded(state_rows(1, [0, 1, 0]))
    lib.call('spaa_grad_sumsq', lib.ptr(gd), lib.ptr(xd), 0.0, 0.0, lib.ptr(sd), lib.ptr(pd), B3, HW)
    assert bits_equal(unpad(gd, n), g4), 'spaa_grad_sumsq without a prjl2 term changed g'
    part = unpad(pd, B3 * nblk).to(F64).view(B3, nblk)
    ref_ss = torch.from_numpy(g * g).view(B3, HW, 3).sum(dim=(1, 2))
    bounded('grad_sumsq err/max(1,sum)', (part.sum(dim=1) - ref_ss).abs() / ref_ss.clamp_min(1.0), PART_TOL)
    lib.call('spaa_masked_step', lib.ptr(xd), lib.ptr(gd), lib.ptr(pd), lib.ptr(sd), 1, 0, 0.37, B3, HW)
    check_step('grad_sumsq partials', unpad(xd, n), x, g, np.sqrt(ref_ss.numpy()), [True, False, True], 0.37, HW, x4)


def test_masked_step_zero_gradient_is_nan(lib):
    """Inherited behaviour, recorded and not changed here: a stepped sample whose gradient is all zero becomes NaN, as the
    reference's g / ||g|| does (perc_al/__init__.py:193-195); the other samples are not affected."""
    HW = 257
    n = B3 * HW
    x, g, part, nblk = step_inputs(HW, 2)
    g[:HW] = 0.0
    part[0] = 0.0
    x4 = rows4(x, markers(n))
    xd, gd, pd, sd = padded(x4), padded(rows4(g, 0.0)), padded(part.reshape(-1)), padded(state_rows(1, [0, 0, 1]))
    lib.call('spaa_masked_step', lib.ptr(xd), lib.ptr(gd), lib.ptr(pd), lib.ptr(sd), 1, 0, 0.5, B3, HW)
    xk = unpad(xd, n)
    assert xk[:HW, :3].isnan().all()
    check_step('zero gradient', xk[HW:], x[HW:], g[HW:], np.sqrt(part.sum(axis=1))[1:], [True, False], 0.5, HW, x4[HW:])


# ---------------------------------------------------------------------------------------------------------------------------------
# spaa_scale_by_map
@pytest.mark.parametrize('HW', HWS)
def test_scale_by_map_vs_fp64(lib, HW):
    n = B3 * HW
    nblk = (HW + 255) // 256
    rng = np.random.default_rng([4, HW])
    g = f32(rng.standard_normal((n, 3)))
    de = f32(rng.uniform(0, 5, (B3, HW)))
    de[2] = 0.0                                           # an all-zero map with zero partial sums
    sq = np.concatenate([de * de, np.zeros((B3, nblk * 256 - HW))], axis=1).reshape(B3, nblk, 256).sum(axis=2)
    p3 = np.full((B3, nblk, 3), NAN)
    p3[:, :, 2] = f32(sq)                                 # only the third partial may be read
    nrm = np.sqrt(p3[:, :, 2].sum(axis=1))
    g4 = rows4(g, markers(n))
    gd, ded, pd, cd = padded(g4), padded(de.reshape(-1)), padded(p3.reshape(-1)), nan_buf(B3)
    lib.call('spaa_scale_by_map', lib.ptr(gd), lib.ptr(ded), lib.ptr(pd), lib.ptr(cd), B3, HW)
    gk, cdk = unpad(gd, n), unpad(cd, B3).to(F64)
    assert bits_equal(gk[:, 3], g4[:, 3]), 'fourth lane of g changed'
    bounded('scale_by_map color_dis err/max(1,v)', (cdk - torch.from_numpy(nrm)).abs() / torch.from_numpy(np.maximum(nrm, 1.0)), CD_TOL, f'HW={HW}')
    for b in range(2):
        sl = slice(b * HW, (b + 1) * HW)
        ref = torch.from_numpy(g[sl] * de[b][:, None] / nrm[b])
        bounded('scale_by_map err/max|g_ref|', (gk[sl, :3].to(F64) - ref).abs() / ref.abs().max().clamp_min(1e-300), MAP_TOL,
                f'HW={HW} sample {b}')
    assert (gk[2 * HW:, :3] == 0).all(), 'all-zero map: g must be exactly 0 (not NaN)'
    assert cdk[2] == 0, 'all-zero map: color_dis must be exactly 0'


# ---------------------------------------------------------------------------------------------------------------------------------
# spaa_perc_clamp_quant
def clamp_inputs(B, HW, seed):
    """inputs in [0, 1] and delta, channel by channel in turn: in + delta below 0, exactly 0, inside, exactly 1, above 1."""
    rng = np.random.default_rng([5, HW, seed])
    n = B * HW * 3
    cat = (np.arange(n) + seed) % 5
    x = np.where(cat == 3, rng.integers(0, 257, n) / 256.0, rng.uniform(0, 1, n))   # (k / 256: 1 - in and in + (1 - in) are exact)
    x = f32(x)
    u = rng.uniform(1e-3, 0.7, n)
    d = np.select([cat == 0, cat == 1, cat == 2, cat == 3], [-x - u, -x, (rng.uniform(0, 1, n) - x) * 0.999, 1.0 - x], 1.0 - x + u)
    d = f32(d)
    s = x.astype(np.float32) + d.astype(np.float32)
    assert (s[cat == 0] < 0).all() and (s[cat == 1] == 0).all() and (s[cat == 3] == 1).all() and (s[cat == 4] > 1).all()
    assert ((s[cat == 2] >= 0) & (s[cat == 2] <= 1)).all()
    return x.reshape(-1, 3), d.reshape(-1, 3)


def check_quant(name, xr, v255, tie_tol=1e-4):
    """xr (n, 3) fp32 host against rint of the float64 v255 = (in + delta) * 255; pixels within tie_tol of a half-integer are
    exempt.  Returns the number of exempt values."""
    k = torch.from_numpy(np.rint(v255))
    near = torch.from_numpy(np.abs(v255 - np.floor(v255) - 0.5) < tie_tol)
    kk = xr.to(F64) * 255
    assert ((kk - kk.round()).abs() < 1e-4).all() and (kk.round() >= 0).all() and (kk.round() <= 255).all(), \
        f'{name}: x_round * 255 is not an integer in 0..255'
    assert torch.equal(kk.round()[~near], k[~near]), f'{name}: quantised values differ off ties'
    assert torch.equal(xr[~near], (k.to(F32) / torch.tensor(255.0, dtype=F32))[~near]), f'{name}: x_round is not fp32 k / 255'
    return int(near.sum())


def block_sums(v, B, HW):
    """(B * HW,) float64 -> [B, nblk] sums over 256-pixel blocks (valid pixels only)."""
    nblk = (HW + 255) // 256
    v = torch.cat([v.view(B, HW), torch.zeros(B, nblk * 256 - HW, dtype=F64)], dim=1)
    return v.view(B, nblk, 256).sum(dim=2)


@pytest.mark.parametrize('HW', HWS)
def test_clamp_quant_vs_fp64(lib, HW):
    n = B3 * HW
    nblk = (HW + 255) // 256
    x, d = clamp_inputs(B3, HW, HW)
    xd, dd, xr, part = padded(rows4(x, 0.0)), padded(rows4(d, NAN)), nan_buf(n, 4), nan_buf(B3 * nblk)
    lib.call('spaa_perc_clamp_quant', lib.ptr(xd), lib.ptr(dd), lib.ptr(xr), lib.ptr(part), B3, HW)
    dk, xrk, pk = unpad(dd, n), unpad(xr, n), unpad(part, B3 * nblk)
    assert (dk[:, 3] == 0).all() and (xrk[:, 3] == 0).all(), 'fourth lane not 0'
    x32, d32 = x.astype(np.float32), d.astype(np.float32)
    want = np.minimum(np.maximum(x32 + d32, np.float32(0)), np.float32(1)) - x32      # the fp32 evaluation
    assert torch.equal(dk[:, :3], torch.from_numpy(want)), 'delta is not the fp32 evaluation of clamp(in + delta, 0, 1) - in'
    bounded('clamp_quant delta err vs fp64', (dk[:, :3].to(F64) - torch.from_numpy(np.clip(x + d, 0, 1) - x)).abs(), CLAMP_TOL,
            f'HW={HW}')
    dw = dk[:, :3].to(F64)
    check_quant(f'HW={HW}', xrk[:, :3], (x + dw.numpy()) * 255)
    assert torch.isfinite(pk).all(), 'fewer than B * nblk partial sums were written'
    ref = block_sums(dw.norm(dim=1), B3, HW)
    bounded('clamp_quant partial err/max(1,sum)', (pk.to(F64).view(B3, nblk) - ref).abs() / ref.clamp_min(1.0), PART_TOL, f'HW={HW}')


def test_clamp_quant_exact_ties_round_half_to_even(lib):
    """in = 0, delta = fp32((k + 0.5) / 255): (in + delta) * 255 is exactly k + 0.5 in fp32 for every k in 0..254, and the result
    must be the even neighbour (rintf; roundf would give k + 1 for the 128 even k)."""
    k = np.arange(255)
    d32 = ((k + 0.5) / 255).astype(np.float32)
    assert (d32 * np.float32(255) == (k + 0.5).astype(np.float32)).all() and (k % 2 == 0).sum() == 128
    HW = 85
    x = np.zeros((HW, 3))
    xd, dd, xr, part = padded(rows4(x, 0.0)), padded(rows4(d32.astype(np.float64).reshape(HW, 3), NAN)), nan_buf(HW, 4), nan_buf(1)
    lib.call('spaa_perc_clamp_quant', lib.ptr(xd), lib.ptr(dd), lib.ptr(xr), lib.ptr(part), 1, HW)
    dk, xrk = unpad(dd, HW), unpad(xr, HW)
    assert torch.equal(dk[:, :3].reshape(-1), torch.from_numpy(d32)), 'delta inside the box must not change'
    even = torch.from_numpy(np.rint(k + 0.5)).to(F32)
    assert (even % 2 == 0).all()
    got = (xrk[:, :3].reshape(-1).to(F64) * 255).round().to(F32)
    assert torch.equal(got, even), f'ties not rounded to even at k = {k[(got != even).numpy()][:8]}'
    assert torch.equal(xrk[:, :3].reshape(-1), even / torch.tensor(255.0, dtype=F32)) and (xrk[:, 3] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# spaa_perc_decide
def decide_ref(lg, label, mode, conf, part, HW, cd, d_thr, p_th, bound):
    """float64 restatement of the decision kernel; arg-max ties go to the lowest index."""
    B = lg.shape[0]
    state, stats = np.zeros((B, 4), dtype=np.int64), np.zeros((B, 5))
    for b in range(B):
        l, t = lg[b], int(label[b])
        am = int(np.argmax(l))                             # (first occurrence = lowest index)
        p1 = 1.0 / np.exp(l - l.max()).sum()
        caml2 = part[b].sum() / HW
        high = caml2 * 255 > d_thr
        other = np.delete(l, t).max() if l.size > 1 else -np.inf
        margin = l[t] - other
        isadv = (am == t) if mode == 0 else (am != t) if mode == 1 else (margin <= -conf)
        best_adv = isadv and high and (p1 > p_th if mode == 0 else True)
        best = best_adv and cd[b] < bound[b]
        state[b] = (isadv, best_adv, best, am)
        stats[b] = (p1, caml2, margin, cd[b], cd[b] if best else bound[b])
    return state, stats


def run_decide(lib, name, lg, label, mode, conf, part, HW, cd, d_thr, p_th, bound):
    """One launch against decide_ref: state exactly; p1, caml2 within their bounds; margin, color_dis and the bound exactly (fp32
    values); stats columns 4, 6, 7 and the PAD rows stay NaN.  Returns the reference's (state, stats)."""
    lg, part, cd, bound = f32(lg), f32(part), f32(cd), f32(bound)
    B, ncls = lg.shape
    nblk = part.shape[1]
    stats = torch.full((B, 8), NAN, dtype=F32)
    stats[:, 5] = torch.from_numpy(bound).to(F32)
    ld, lab, pd, cdd = padded(lg), padded(torch.as_tensor(label)), padded(part.reshape(-1)), padded(cd)
    sd, std = torch.full((B + PAD, 4), IPAD, dtype=I32, device=DEV), padded(stats)
    lib.call('spaa_perc_decide', lib.ptr(ld), ncls, lib.ptr(lab), mode, float(conf), lib.ptr(pd), nblk, HW, lib.ptr(cdd),
             float(d_thr), float(p_th), lib.ptr(sd), lib.ptr(std), B)
    sk, stk = unpad(sd, B), unpad(std, B)
    d32, p32 = float(np.float32(d_thr)), float(np.float32(p_th))
    ref_state, ref_stats = decide_ref(lg, label, mode, float(np.float32(conf)), part, HW, cd, d32, p32, bound)
    assert stk[:, [4, 6, 7]].isnan().all(), f'{name}: stats columns 4, 6, 7 were written'
    rs = torch.from_numpy(ref_stats)
    bounded('decide p1 err', (stk[:, 0].to(F64) - rs[:, 0]).abs(), P1_TOL, name)
    bounded('decide caml2 err/max(1,v)', (stk[:, 1].to(F64) - rs[:, 1]).abs() / rs[:, 1].clamp_min(1.0), CAML2_TOL, name)
    assert torch.equal(stk[:, 2], rs[:, 2].to(F32)), f'{name}: margin {stk[:, 2]} != {rs[:, 2]}'
    assert torch.equal(stk[:, 3], rs[:, 3].to(F32)), f'{name}: stats[3] is not color_dis'
    assert torch.equal(stk[:, 5], rs[:, 4].to(F32)), f'{name}: bound {stk[:, 5]} != {rs[:, 4]}'
    assert torch.equal(sk.to(torch.int64), torch.from_numpy(ref_state)), \
        f'{name}: state\n{sk}\n!= reference\n{ref_state}'
    return ref_state, ref_stats


def parts_for(rng, targets, nblk, HW):
    """[B, nblk] fp32 partial sums with sum / HW * 255 = targets (to fp32 rounding)."""
    p = rng.uniform(0.5, 1.5, (len(targets), nblk))
    return f32(p / p.sum(axis=1, keepdims=True) * (np.asarray(targets)[:, None] * HW / 255.0))


def argmax_rows(ncls, rng):
    """(logits, expected arg-max, label) rows: a unique maximum at 0, 63, 64, 255, 256, ncls - 1; ties of two and three positions
    in different lanes, waves and strides.  Labels alternate between the arg-max and another class; on ties also the highest tied
    index (isadv differs between the lowest-index and any other tie rule)."""
    rows = []
    for i, pos in enumerate(sorted({p for p in (0, 63, 64, 255, 256, ncls - 1) if p < ncls})):
        l = np.round(rng.standard_normal(ncls) * 8) / 8
        l[pos] = l.max() + 2
        rows.append((l, pos, pos if i % 2 == 0 else (pos + 1) % ncls))
    ties = [(0, 1), (0, 2), (1, 2), (0, 1, 2), (5, 9), (9, 40, 62), (5, 70), (70, 5 + 192), (5, 261), (261, 5 + 512), (70, 300),
            (300, 70 + 512), (3, 67, 259), (62, 64, 256), (255, 256), (63, 64), (ncls - 2, ncls - 1), (0, ncls - 1),
            (ncls // 2, ncls - 1)]
    for i, tie in enumerate(t for t in dict.fromkeys(ties) if max(t) < ncls and len(set(t)) == len(t) and min(t) >= 0):
        l = np.round(rng.standard_normal(ncls) * 8) / 8
        l[list(tie)] = l.max() + 2
        rows.append((l, min(tie), (min(tie), max(tie), (max(tie) + 1) % ncls)[i % 3]))
    return rows


@pytest.mark.parametrize('ncls', NCLS)
def test_decide_argmax_and_ties(lib, ncls):
    rng = np.random.default_rng([6, ncls])
    rows = argmax_rows(ncls, rng)
    lg = np.stack([r[0] for r in rows])
    am = np.array([r[1] for r in rows])
    label = np.array([r[2] for r in rows])
    B = len(rows)
    nblk, HW, d_thr = [1, 255, 256, 257][NCLS.index(ncls) % 4], 1000, 5.0
    part = parts_for(rng, np.where(np.arange(B) % 2 == 0, 0.8, 1.25) * d_thr, nblk, HW)
    cd = rng.uniform(1, 50, B)
    bound = cd * np.where(np.arange(B) % 3 == 0, 0.7, 1.4)
    for mode in (0, 1):
        state, _ = run_decide(lib, f'ncls={ncls} mode={mode}', lg, label, mode, 0.0, part, HW, cd, d_thr, 0.05 / ncls, bound)
        assert (state[:, 3] == am).all()
        assert set(state[:, 0]) == {0, 1}, 'both outcomes of isadv must occur'


@pytest.mark.parametrize('ncls', [2, 65, 1000])
def test_decide_mode0_p1_and_perturbation(lib, ncls):
    """Two-class-dominated logits: p1 = 1 / (1 + e^-g + (ncls - 2) e^-30) at least 1e-3 below / above p_thresh = 0.9, each with
    caml2 * 255 below / above d_thr; and the label not being the arg-max although its class is confident."""
    rng = np.random.default_rng([7, ncls])
    p_th, d_thr, HW = 0.9, 3.0, 437
    lg, label, tg = [], [], []
    for p1 in (0.898, 0.8985, 0.9015, 0.902):
        for pert in (0.8, 1.25):
            t = int(rng.integers(0, ncls))
            l = np.full(ncls, -30.0)
            l[t] = math.log(p1 / (1 - p1))
            l[(t + 1) % ncls] = 0.0
            lg.append(l), label.append(t), tg.append(pert * d_thr)
    l = np.full(ncls, -30.0)                               # confident, high perturbation, but the label is the runner-up
    l[0], l[1] = 5.0, 0.0
    lg.append(l), label.append(1), tg.append(2 * d_thr)
    lg, B = np.stack(lg), len(lg)
    state, stats = run_decide(lib, f'mode 0 ncls={ncls}', lg, np.array(label), 0, 0.0, parts_for(rng, tg, 2, HW), HW,
                              rng.uniform(1, 5, B), d_thr, p_th, np.full(B, 100000.0))
    assert (np.abs(stats[:, 0] - p_th) >= 1e-3).all() and (np.abs(stats[:, 1] * 255 - d_thr) >= 1e-3 * d_thr).all()
    assert state[:, 1].tolist() == [0, 0, 0, 0, 0, 1, 0, 1, 0], state[:, 1]
    assert state[:, 0].tolist() == [1] * 8 + [0]


def test_decide_strict_comparisons(lib):
    """The crisp edges, each exactly representable in fp32: caml2 * 255 > d_thr, p1 > p_thresh and color_dis < bound are strict."""
    HW = 512
    one = np.ones((3, 3)) * np.array([[4.0, 0.0, -2.0]])   # label 0 is the arg-max; fine for mode 0 (p1 ~ 0.98) and, with label 1, mode 1
    zero_p, cd, big = np.zeros((3, 2)), np.array([2.0, 2.0, 2.0]), np.full(3, 100000.0)
    # all-zero partial sums: 0 > 0 is false, 0 > -1 is true
    s, _ = run_decide(lib, 'zero partials, d_thr 0', one, [1, 1, 1], 1, 0.0, zero_p, HW, cd, 0.0, 0.9, big)
    assert s[:, :3].tolist() == [[1, 0, 0]] * 3
    s, st = run_decide(lib, 'zero partials, d_thr -1', one, [1, 1, 1], 1, 0.0, zero_p, HW, cd, -1.0, 0.9, big)
    assert s[:, :3].tolist() == [[1, 1, 1]] * 3 and (st[:, 4] == 2.0).all()
    # sum = HW: caml2 = 1 and caml2 * 255 = 255 exactly
    full = np.array([[HW / 2, HW / 2]] * 3)
    below = float(np.nextafter(np.float32(255), np.float32(0)))
    s, _ = run_decide(lib, 'caml2 * 255 == d_thr', one, [0, 0, 0], 0, 0.0, full, HW, cd, 255.0, 0.9, big)
    assert s[:, :3].tolist() == [[1, 0, 0]] * 3
    s, _ = run_decide(lib, 'caml2 * 255 one step above d_thr', one, [0, 0, 0], 0, 0.0, full, HW, cd, below, 0.9, big)
    assert s[:, :3].tolist() == [[1, 1, 1]] * 3
    # two equal logits: p1 = 0.5 exactly, and the tie goes to class 0
    eq = np.zeros((3, 2))
    s, st = run_decide(lib, 'p1 == p_thresh', eq, [0, 0, 1], 0, 0.0, full, HW, cd, 1.0, 0.5, big)
    assert (st[:, 0] == 0.5).all() and s.tolist() == [[1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]
    s, _ = run_decide(lib, 'p1 one step above p_thresh', eq, [0, 0, 1], 0, 0.0, full, HW, cd,
                      1.0, float(np.nextafter(np.float32(0.5), np.float32(0))), big)
    assert s.tolist() == [[1, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0]]
    # the bound: equal is not best; one fp32 step lower is; lower without best_adv leaves it alone
    cd = np.array([2.0, float(np.nextafter(np.float32(2), np.float32(0))), 1.0])
    s, st = run_decide(lib, 'bound, best_adv', one, [1, 1, 1], 1, 0.0, full, HW, cd, 1.0, 0.9, np.full(3, 2.0))
    assert s[:, :3].tolist() == [[1, 1, 0], [1, 1, 1], [1, 1, 1]] and st[:, 4].tolist() == [2.0, cd[1], 1.0]
    s, st = run_decide(lib, 'bound, adversarial without best_adv', one, [1, 1, 1], 1, 0.0, full, HW, cd, 300.0, 0.9, np.full(3, 2.0))
    assert s[:, :3].tolist() == [[1, 0, 0]] * 3 and (st[:, 4] == 2.0).all()
    s, st = run_decide(lib, 'bound, not adversarial', one, [0, 0, 0], 1, 0.0, full, HW, cd, 1.0, 0.9, np.full(3, 2.0))
    assert s[:, :3].tolist() == [[0, 0, 0]] * 3 and (st[:, 4] == 2.0).all()


@pytest.mark.parametrize('ncls', [2, 64, 257, 1025])
def test_decide_mode2_margin(lib, ncls):
    """Integer logits: a margin of exactly -confidence is adversarial, one fp32 step above it is not; the label's own logit, the
    largest of all, must not count as `other`."""
    rng = np.random.default_rng([8, ncls])
    HW, conf = 300, 40.0
    base = np.floor(rng.uniform(-20, 20, (6, ncls)))
    label = np.array([0, ncls - 1, ncls // 2, 0, ncls - 1, ncls // 2])
    o = (label + 1 + np.arange(6) * 7) % ncls
    o = np.where(o == label, (label + 1) % ncls, o)
    r = np.arange(6)
    lg = base.copy()
    lg[r, label] = 0.0
    lg[r, o] = [40.0, float(np.nextafter(np.float32(40), np.float32(0))), 41.0, 39.0, 40.0, 1000.0]
    lg[5, label[5]] = 960.0                                # 960 - 1000 = -40 at large logits
    part = parts_for(rng, [2.0] * 6, 3, HW)
    cd, big = rng.uniform(1, 5, 6), np.full(6, 100000.0)
    s, st = run_decide(lib, f'mode 2 ncls={ncls}', lg, label, 2, conf, part, HW, cd, 1.0, 0.9, big)
    assert s[:, 0].tolist() == [1, 0, 1, 0, 1, 1] and (s[:, 1] == s[:, 0]).all()
    assert st[:, 2].tolist() == [-40.0, -float(np.nextafter(np.float32(40), np.float32(0))), -41.0, -39.0, -40.0, -40.0]
    # the label's own logit is the largest of all: margin = 100 - 50; with confidence -60 (margin <= 60) adversarial, with 40 not
    lg2 = np.minimum(base, 19.0)
    lg2[r, label] = 100.0
    lg2[r, o] = 50.0
    for c, adv in ((conf, 0), (-60.0, 1), (-50.0, 1), (-49.0, 0)):
        s, st = run_decide(lib, f'mode 2 ncls={ncls} own logit largest, confidence {c}', lg2, label, 2, c, part, HW, cd, 1.0, 0.9, big)
        assert (st[:, 2] == 50.0).all() and (s[:, 0] == adv).all() and (s[:, 3] == label).all()


@pytest.mark.parametrize('nblk', [1, 255, 256, 257])
def test_decide_partial_sum_strides(lib, nblk):
    """caml2 = sum of nblk partial sums / HW, with HW passed independently of nblk."""
    rng = np.random.default_rng([9, nblk])
    HW = 777
    part = f32(rng.uniform(0, 2, (B3, nblk)))
    part[1, nblk // 2:] = 0.0
    lg = np.round(rng.standard_normal((B3, 37)) * 8) / 8
    d_thr = float(np.sort(part.sum(axis=1))[1] / HW * 255 * 1.1)
    s, st = run_decide(lib, f'nblk={nblk}', lg, [0, 1, 2], 1, 0.0, part, HW, rng.uniform(1, 5, B3), d_thr, 0.9, np.full(B3, 100000.0))
    assert (np.abs(st[:, 1] * 255 - d_thr) >= 1e-3 * d_thr).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# spaa_track_where
@pytest.mark.parametrize('HW', HWS)
def test_track_where(lib, HW):
    n = B3 * HW
    rng = np.random.default_rng([10, HW])
    src = rows4(f32(rng.uniform(0, 1, (n, 3))), 0.0)
    dst = rows4(f32(rng.uniform(0, 1, (n, 3))), markers(n))
    states = [[0, 1, 1, 1], [1, 0, 0, 0], [-3, 0, 0, 0], [0, 0, 1, 0], [7, 1, 1, 1]]   # copy iff column 0 != 0
    k = HWS.index(HW)
    st = torch.tensor([states[(k + b) % 5] for b in range(B3)] if HW != 257 else [states[3], states[1], states[0]], dtype=I32)
    sd, dd, std = padded(src), padded(dst), padded(st)
    lib.call('spaa_track_where', lib.ptr(sd), lib.ptr(dd), lib.ptr(std), B3, HW)
    out = unpad(dd, n)
    assert bits_equal(unpad(sd, n), src) and torch.equal(unpad(std, B3), st)
    for b in range(B3):
        sl = slice(b * HW, (b + 1) * HW)
        assert bits_equal(out[sl], src[sl] if st[b, 0] != 0 else dst[sl]), f'HW={HW} sample {b} state {st[b].tolist()}'


# ---------------------------------------------------------------------------------------------------------------------------------
# argument checks
def test_argument_checks(lib):
    """A bad mode / col / count or a null pointer fails the call (a non-zero status, which _lib.call raises) before anything is
    launched: the outputs stay NaN."""
    B, HW, ncls, n = 2, 5, 4, 10
    a, b, x = padded(torch.zeros(n, 4)), padded(torch.zeros(n, 4)), nan_buf(n, 4)
    lg, lab, gl = padded(torch.zeros(B, ncls)), padded(torch.zeros(B, dtype=I32)), nan_buf(B, ncls)
    part, st = padded(torch.ones(B)), padded(torch.zeros(B, 4, dtype=I32))
    de, p3, cd = padded(torch.ones(n)), padded(torch.ones(B * 3)), nan_buf(B)
    pout, stats = nan_buf(B), nan_buf(B, 8)
    state_out = torch.full((B + PAD, 4), IPAD, dtype=I32, device=DEV)
    p = lib.ptr
    good = {
        'spaa_add_nhwc4': [p(a), p(b), p(x), n],
        'spaa_ce_grad': [p(lg), ncls, p(lab), 1.0, p(gl), B],
        'spaa_masked_step': [p(x), p(a), p(part), p(st), 1, 0, 0.5, B, HW],
        'spaa_scale_by_map': [p(x), p(de), p(p3), p(cd), B, HW],
        'spaa_perc_clamp_quant': [p(a), p(x), p(x), p(pout), B, HW],
        'spaa_perc_decide': [p(lg), ncls, p(lab), 0, 0.0, p(part), 1, HW, p(de), 1.0, 0.9, p(state_out), p(stats), B],
        'spaa_track_where': [p(a), p(x), p(st), B, HW],
    }
    bad = [('spaa_perc_decide', 3, 3), ('spaa_perc_decide', 3, -1), ('spaa_masked_step', 4, 4), ('spaa_masked_step', 4, -1),
           ('spaa_add_nhwc4', 3, 0), ('spaa_ce_grad', 5, 0), ('spaa_ce_grad', 1, 0), ('spaa_masked_step', 7, 0),
           ('spaa_masked_step', 8, 0), ('spaa_scale_by_map', 4, 0), ('spaa_scale_by_map', 5, 0), ('spaa_perc_clamp_quant', 4, 0),
           ('spaa_perc_clamp_quant', 5, 0), ('spaa_perc_decide', 13, 0), ('spaa_perc_decide', 1, 0), ('spaa_perc_decide', 6, 0),
           ('spaa_track_where', 3, 0), ('spaa_track_where', 4, 0)]
    for name, args in good.items():                        # a null pointer in each pointer position
        bad += [(name, i, None) for i, v in enumerate(args) if not isinstance(v, (int, float))]
    assert len(bad) == 18 + 3 + 3 + 4 + 4 + 4 + 6 + 3
    for name, i, v in bad:
        args = list(good[name])
        args[i] = v
        with pytest.raises(RuntimeError, match=name):
            lib.call(name, *args)
    torch.cuda.synchronize()
    for out in (x, gl, cd, pout, stats):
        assert out.isnan().all(), 'a refused call wrote its output'
    assert (state_out == IPAD).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# Part 2: the loop body of PerCALState against a float64 restatement
LB, LH, LW, LNCLS, LITERS = 6, 23, 19, 37, 6
LHW = LH * LW
GAIN = 4.0
D_THR = 2.0
ALPHA_L, ALPHA_C = 0.3, 0.03
SEED = 8
ACTIVE = [LHW, 10, LHW, LHW, LHW, 60]                      # pixels that each sample's linear model reads (see LIVES)
# LIVES: per sample, per iteration, what the scripted decision pass says: 0 = not adversarial, 1 = adversarial but (mode 0) not
# confident, 2 = adversarial and confident.  With the perturbation size that the sample's model produces this gives:
#   0 never adversarial
#   1 adversarial, never confident (mode 0) nor high-perturbation (3 active pixels): x_best follows x_round, adversarial steps only
#   2 best_adv from iteration 1 on: the colour step only from iteration 2, the bound falls with color_dis
#   3 best_adv at iterations 1 and 2, then not adversarial: adversarial steps again, x_best keeps iteration 2's image, the bound stays
#   4 best_adv, not adversarial, then adversarial with a color_dis above the bound: not best, but tracked
#   5 adversarial and confident; high_pert turns true at a later iteration (40 active pixels)
LIVES = [[0, 0, 0, 0, 0, 0],
         [1, 1, 1, 1, 1, 1],
         [2, 2, 2, 2, 2, 2],
         [2, 2, 0, 0, 0, 0],
         [2, 0, 2, 2, 2, 2],
         [2, 2, 2, 2, 2, 2]]


def loop_problem():
    """x_in [B,3,H,W] fp32 values, labels, the linear model (s [B,HW], W [ncls,3]) -- all float64 holding fp32 values."""
    rng = np.random.default_rng([11, SEED])
    x_in = rng.uniform(0.1, 1, (LB, LHW, 3))
    # one pixel in five has one channel on the box (0 or 1) and the others bright: the clamp changes delta at every iteration (so
    # color_dis moves clearly between two iterations without a step), and no pixel leaves the gamut far enough for NaN in Lab
    sat, ch = rng.uniform(size=(LB, LHW)) < 0.2, rng.integers(0, 3, (LB, LHW))
    edge = rng.integers(0, 2, (LB, LHW)).astype(np.float64)
    s = np.zeros((LB, LHW))
    for b in range(LB):
        idx = rng.permutation(LHW)[:ACTIVE[b]]
        s[b, idx] = rng.uniform(0.5, 1.5, ACTIVE[b]) / ACTIVE[b]
        if ACTIVE[b] < LHW:                               # few active pixels take large steps: bright and only on the upper edge
            x_in[b, idx] = rng.uniform(0.5, 1, (ACTIVE[b], 3))
            edge[b] = 1.0
    x_in = np.where(sat[:, :, None] & (x_in < 0.3), rng.uniform(0.3, 1, (LB, LHW, 3)), x_in)
    x_in = np.where(sat[:, :, None] & (ch[:, :, None] == np.arange(3)), edge[:, :, None], x_in)
    x_in = f32(x_in.reshape(LB, LH, LW, 3).transpose(0, 3, 1, 2))
    w = f32(rng.standard_normal((LNCLS, 3)))
    labels = rng.integers(0, LNCLS, LB)
    return torch.from_numpy(x_in), torch.from_numpy(labels), torch.from_numpy(f32(s)), torch.from_numpy(w)


def loop_script(mode, labels):
    """[iterations, B, ncls] logits (multiples of 1/8) of the decision pass that realise LIVES in `mode`."""
    rng = np.random.default_rng([12, SEED, mode])
    tab = -np.round(rng.uniform(0, 1, (LITERS, LB, LNCLS)) * 8) / 8
    for i in range(LITERS):
        for b in range(LB):
            t, life = int(labels[b]), LIVES[b][i]
            o = (t + 1 + i + b) % LNCLS
            o = o if o != t else (t + 1) % LNCLS
            if mode == 0:      # adversarial = the label is the arg-max; confident = p1 > 0.9
                tab[i, b, t], tab[i, b, o] = ((0.0, 5.0), (2.0, 0.0), (8.0, 0.0))[life]
            elif mode == 1:    # adversarial = the arg-max is not the label
                tab[i, b, t], tab[i, b, o] = ((5.0, 0.0), (0.0, 3.0), (0.0, 6.0))[life]
            else:              # adversarial = label - best other <= -40 (an arg-max that is not the label is not enough)
                tab[i, b, t], tab[i, b, o] = ((0.0, 32.0), (0.0, 48.0), (0.0, 64.0))[life]
    return torch.from_numpy(tab)


def to_img(v):
    """[B, HW, 3] -> [B, 3, H, W]"""
    return v.view(LB, LH, LW, 3).permute(0, 3, 1, 2).contiguous()


def to_pix(v):
    """[B, 3, H, W] -> [B, HW, 3]"""
    return v.permute(0, 2, 3, 1).reshape(LB, LHW, 3)


def loop_reference(mode, dtype=F64):
    """perc_al/__init__.py:179-245 restated for the linear model and the scripted decision pass, in `dtype`; one dict per
    iteration.  (float32: the CPU check that the conditions below leave fp32 arithmetic room.)"""
    x_in, labels, s, w = loop_problem()
    x_in, s, w = x_in.to(dtype), s.to(dtype), w.to(dtype)
    script = loop_script(mode, labels).to(dtype)
    mult = -1.0 if mode == 0 else 1.0
    conf = 40.0
    lab_in = so.rgb2lab_diff(x_in)
    delta = torch.zeros_like(x_in)
    best_adv = torch.zeros(LB, dtype=torch.bool)
    bound = torch.full((LB,), 100000.0, dtype=dtype)
    tracked = [-1] * LB
    onehot = torch.zeros(LB, LNCLS, dtype=dtype)
    onehot[torch.arange(LB), labels] = 1.0
    a_l_min, a_c_min = ALPHA_L / 100, ALPHA_C / 10
    out = []
    for i in range(LITERS):
        alpha_c = a_c_min + 0.5 * (ALPHA_C - a_c_min) * (1 + math.cos(i / LITERS * math.pi))
        alpha_l = a_l_min + 0.5 * (ALPHA_L - a_l_min) * (1 + math.cos(i / LITERS * math.pi))
        logits = GAIN * torch.einsum('bp,bpc,kc->bk', s, to_pix(x_in + delta), w)
        gl = mult * (torch.softmax(logits, dim=1) - onehot)
        g_a = to_img(GAIN * s[:, :, None] * (gl @ w)[:, None, :])
        step = alpha_l * g_a / g_a.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
        delta = torch.where((~best_adv).view(-1, 1, 1, 1), delta + step, delta)
        x = (x_in + delta).requires_grad_(True)
        color_dis = so.ciede2000_diff(lab_in, so.rgb2lab_diff(x)).flatten(1).norm(dim=1)
        g_c, = torch.autograd.grad(color_dis.sum(), x)
        color_dis = color_dis.detach()
        step = alpha_c * g_c / g_c.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
        delta = torch.where(best_adv.view(-1, 1, 1, 1), delta - step, delta)
        delta = (x_in + delta).clamp(0, 1) - x_in
        v255 = (x_in + delta) * 255
        caml2 = delta.norm(dim=1).flatten(1).mean(dim=1)
        high = caml2 * 255 > D_THR
        lg = script[i]
        top1 = torch.tensor([int(np.argmax(r)) for r in lg.numpy()])
        p1 = torch.softmax(lg, dim=1).max(dim=1)[0]
        oth = lg.clone()
        oth[torch.arange(LB), labels] = -math.inf
        margin = lg[torch.arange(LB), labels] - oth.max(dim=1)[0]
        if mode == 0:
            isadv = top1 == labels
            best_adv = isadv & (p1 > 0.9) & high
        elif mode == 1:
            isadv = top1 != labels
            best_adv = isadv & high
        else:
            isadv = margin <= -conf
            best_adv = isadv & high
        bound_in = bound.clone()
        best = best_adv & (color_dis < bound)
        bound = torch.where(best, color_dis, bound)
        for b in range(LB):
            if isadv[b]:
                tracked[b] = i
        out.append(dict(delta=to_pix(delta), v255=to_pix(v255), caml2=caml2, high=high, p1=p1, margin=margin, top1=top1,
                        isadv=isadv, best_adv=best_adv, best=best, color_dis=color_dis, bound_in=bound_in, bound=bound.clone(),
                        tracked=list(tracked)))
    return out


def reference_conditions(mode, ref):
    """Conditions on the float64 run alone: the GPU comparison is meaningful only if they hold."""
    near = 0
    for i, r in enumerate(ref):
        m = (r['caml2'] * 255 - D_THR).abs() / D_THR
        assert (m >= 1e-3).all(), f'mode {mode} iteration {i}: caml2 * 255 within {float(m.min()):.1e} of d_thr'
        m = (r['color_dis'] - r['bound_in']).abs() / r['bound_in']
        assert (m >= 1e-3).all(), f'mode {mode} iteration {i}: color_dis within {float(m.min()):.1e} of the bound'
        if mode == 0:
            assert ((r['p1'] - 0.9).abs() >= 1e-3).all()
        near += int(((r['v255'] - r['v255'].floor() - 0.5).abs() < 1e-3).any(dim=2).sum())
    assert near <= 0.01 * LITERS * LB * LHW, f'{near} near-tie pixels'
    col = lambda k, b: [bool(r[k][b]) for r in ref]  # noqa: E731
    assert not any(col('isadv', 0))
    assert all(col('isadv', 1)) and not any(col('best_adv', 1)) and ref[-1]['tracked'][1] == LITERS - 1
    assert all(col('best_adv', 2)) and col('best', 2)[0]
    falls = [ref[i]['color_dis'][2] < ref[i]['bound_in'][2] for i in range(LITERS)]
    assert [bool(f) for f in falls] == col('best', 2) and sum(col('best', 2)) >= 2
    assert col('best_adv', 3)[:2] == [True, True] and not any(col('isadv', 3)[2:]) and ref[-1]['tracked'][3] == 1
    assert ref[-1]['bound'][3] == ref[1]['bound'][3] < 100000
    assert any(ba and not be and float(r['color_dis'][4]) > float(r['bound_in'][4]) for r, ba, be in
               zip(ref, col('best_adv', 4), col('best', 4))) and col('best', 4)[0] and not col('isadv', 4)[1]
    assert all(col('isadv', 5)) and not col('best_adv', 5)[0] and any(col('best_adv', 5)[1:])
    high5 = col('high', 5)
    assert high5 == sorted(high5), 'high_pert of life 5 must turn true once'


_REF = {}


def reference(mode):
    if mode not in _REF:
        _REF[mode] = loop_reference(mode)
    return _REF[mode]


class StubEngine:
    """What PerCALState needs of a classifier engine.  forward(need_grad=True): the linear model, from torch ops on the device;
    backward: its exact adjoint into an NHWC4 buffer; forward(need_grad=False): the next row of the scripted logit table.  It
    asserts what the glue hands it."""

    def __init__(self, owner, s, w, script):
        self.st, self.ncls = owner, LNCLS
        self.s, self.w, self.script = s.to(F32).to(DEV), w.to(F32).to(DEV), script.to(F32).to(DEV).contiguous()
        self.g = torch.zeros(LB, LH, LW, 4, device=DEV)
        self.calls, self.i = [], 0

    def forward(self, x4, need_grad=True):
        st = self.st
        assert x4.shape == (LB, LH, LW, 4) and x4.dtype == F32 and x4.is_contiguous()
        if need_grad:
            assert x4.data_ptr() == st.x.data_ptr()
            assert torch.equal(x4[..., :3], (st.x_in + st.delta)[..., :3]) and (x4[..., 3] == 0).all(), 'forward: not x_in + delta'
            self.calls.append('fwd')
            return (GAIN * torch.einsum('bp,bpc,kc->bk', self.s, x4.view(LB, LHW, 4)[..., :3], self.w)).contiguous()
        assert x4.data_ptr() == st.x_round.data_ptr(), 'the decision pass must see st.x_round'
        self.calls.append('decide')
        self.i += 1
        return self.script[self.i - 1]

    def backward(self, g_logits):
        assert g_logits.data_ptr() == self.st.g_logits.data_ptr() and self.calls[-1] == 'fwd'
        self.calls.append('bwd')
        self.g.view(LB, LHW, 4)[..., :3] = GAIN * self.s[:, :, None] * (g_logits @ self.w)[:, None, :]
        return self.g


class StubClassifier:
    def __init__(self, s, w, script):
        self.args, self.eng = (s, w, script), None

    def engine(self, batch, im_hw, crop_sz, owner=None, storage='f32'):
        assert (batch, tuple(im_hw)) == (LB, (LH, LW)) and owner is not None
        self.eng = StubEngine(owner, *self.args)
        return self.eng


def make_state(mode, storage='f32'):
    from spaa_amd.perc_al import PerC_AL, PerCALState
    x_in, labels, s, w = loop_problem()
    att = PerC_AL(max_iterations=LITERS, alpha_l_init=ALPHA_L, alpha_c_init=ALPHA_C, confidence=40 if mode == 2 else 0,
                  device=torch.device('cuda', torch.cuda.current_device()), storage=storage)
    clf = StubClassifier(s, w, loop_script(mode, labels))
    st = PerCALState(att, clf, x_in.to(F32), labels, D_THR, mode == 0, (LH, LW))
    assert st.mode == mode and st.nblk == 2 and st.mult == (-1.0 if mode == 0 else 1.0) * (64.0 if storage == 'f16' else 1.0)
    st.stats[:, [4, 6, 7]] = NAN                           # columns the kernels do not own
    return st, clf.eng


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_loop_reference_conditions(mode):
    reference_conditions(mode, reference(mode))


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_loop_vs_fp64(lib, mode):
    ref = reference(mode)
    reference_conditions(mode, ref)
    st, eng = make_state(mode)
    x_in = st.x_in.clone()
    snaps = {-1: x_in.view(LB, LHW, 4).clone()}
    for i, r in enumerate(ref):
        st.iteration(i)
        torch.cuda.synchronize()
        name = f'mode {mode} iteration {i + 1}'
        assert eng.calls[-3:] == ['fwd', 'bwd', 'decide'] and eng.i == i + 1
        state, stats = st.state.cpu(), st.stats.cpu().to(F64)
        want = torch.stack([r['isadv'].long(), r['best_adv'].long(), r['best'].long(), r['top1']], dim=1)
        assert torch.equal(state.long(), want), f'{name}: state\n{state}\n!= reference\n{want}'
        assert stats[:, [4, 6, 7]].isnan().all()
        bounded('loop p1 err', (stats[:, 0] - r['p1']).abs(), P1_TOL, name)
        bounded('loop caml2 err/max(1,v)', (stats[:, 1] - r['caml2']).abs() / r['caml2'].clamp_min(1.0), CAML2_TOL, name)
        assert torch.equal(stats[:, 2], r['margin']), f'{name}: margin'
        bounded('loop color_dis err/max(1,v)', (stats[:, 3] - r['color_dis']).abs() / r['color_dis'].clamp_min(1.0), CD_LOOP_TOL, name)
        bounded('loop bound err/max(1,v)', (stats[:, 5] - r['bound']).abs() / r['bound'].clamp_min(1.0), CD_LOOP_TOL, name)
        delta = st.delta.cpu().view(LB, LHW, 4)
        assert (delta[..., 3] == 0).all()
        bounded('loop delta err/max|delta|', (delta[..., :3].to(F64) - r['delta']).abs().max() / r['delta'].abs().max(), DELTA_TOL, name)
        xr = st.x_round.cpu().view(LB, LHW, 4)
        assert (xr[..., 3] == 0).all()
        k, kr = (xr[..., :3].to(F64) * 255).round(), r['v255'].round()
        near = (r['v255'] - r['v255'].floor() - 0.5).abs() < 1e-3
        assert torch.equal(k[~near], kr[~near]), f'{name}: x_round differs off ties'
        assert ((k - kr).abs() <= 1).all() and torch.equal(xr[..., :3], k.to(F32) / torch.tensor(255.0, dtype=F32))
        snaps[i] = st.x_round.view(LB, LHW, 4).clone()
        xb = st.x_best.view(LB, LHW, 4)
        for b in range(LB):
            assert bits_equal(xb[b], snaps[r['tracked'][b]][b]), f'{name}: x_best of sample {b} is not the image of iteration ' \
                                                                f'{r["tracked"][b] + 1}'
        assert bits_equal(st.x_in, x_in)
    assert torch.isfinite(st.result()).all()


def test_loop_f16_storage_loss_scale_cancels(lib):
    """storage='f16' only scales the logit gradient by 64 (the stub ignores the storage mode): the normalised step cancels it."""
    a, _ = make_state(0, 'f32')
    b, _ = make_state(0, 'f16')
    for i in range(LITERS):
        a.iteration(i)
        b.iteration(i)
        da, db = a.delta.cpu().to(F64), b.delta.cpu().to(F64)
        bounded('loop f16 delta diff/max|delta|', (da - db).abs().max() / da.abs().max(), DELTA_TOL, f'iteration {i + 1}')
        assert torch.equal(a.state, b.state)
