"""GPU (-m gpu): the colour kernels of csrc/color.hip -- spaa_rgb2lab, spaa_rgb2lab_bwd, spaa_ciede2000, spaa_ciede2000_bwd and the
fused stealthiness loss spaa_stealth_loss_fwd_bwd(_ps) -- launch by launch through the C ABI against the oracle's rgb2lab_diff /
ciede2000_diff evaluated and differentiated in float64.

Cases come from seeded generators that place inputs on either side of every branch of the formula: the sRGB knee (0.0405) and the
Lab knee (0.008856), exact black (f(0) = 0, L = -16), the +1e-4 guard of achromatic colours, C1 C2 == 0, the hue wrap of atan2,
|dh'| against 180, |h1' + h2'| against 360, chroma 1e-7 ... 1e-4 (where aC^7 underflows fp32), mean L = 50, mean hue near 275,
identical colours and colours one ulp apart.  Lab inputs are fp32 values, so the only error is the kernel's arithmetic.

The error is split into three parts, so that grey pixels (whose a*, b* are fp32 cancellation residues) are held as tightly as any:
  * Lab(rgb) within LAB_TOL Lab units of float64;
  * dE and d dE / d Lab at the kernel's own Lab (read back from spaa_rgb2lab) against float64 at that Lab;
  * d / d rgb against the chain through the float64 Jacobian J_lab(rgb)^T, relative to the pixel's |J|^T |g_lab|.
Where the float64 inputs lie within HUE_MARGIN degrees of the |dh'| = 180 or |h1' + h2'| = 360 switch (or a channel sits on the
sRGB knee), float64 is evaluated on both sides and either is accepted; the value and the gradient must come from the same side.

Bounds, each at most 4x the largest value measured on an MI355X (in brackets):
  * Lab: |err| <= 3e-4 Lab units  [1.45e-4]
  * dE: |err| <= 4e-5 * max(1, dE64)  [1.79e-5 on Lab inputs, 2.75e-5 in the fused loss]
  * d dE / d Lab, where dE64 >= 1e-3: max |err| <= (1e-5 + 8 cond) |g64|, cond = 2^-24 max|Lab| / dE64 (the rounding of a
    Lab difference, against dE)  [0.52 of the bound];  below 1e-3: finite and |g| <= 2 |g64|  [|g| / (2 |g64|) <= 0.87]
  * d / d rgb of the fused loss: max |err| <= (2e-4 + 16 cond) max(|J|^T |g_lab|)  [0.68 of the bound; below: 0.55]
  * rgb2lab_bwd: max |err| <= 1e-4 * max(|J|^T |g_lab|)  [6.6e-5: the reference's Lab knee has a 5e-5 slope step]
  * block partial sums of ||d||_2, dE, dE^2 and per-sample sums: |err| <= 4e-5 * sum of max(1, |term|)  [1.1e-5]
  * de_map against spaa_ciede2000(spaa_rgb2lab(y), scene_lab): <= 1e-5 * max(1, dE)  [3.0e-6]
Identical colours and identical pixels give exactly zero; every output is finite; outputs start as NaN and rows past `npix` must
stay NaN; the stealth launch is bitwise reproducible and de_map does not change g_y or the partial sums.
"""
import math

import numpy as np
import pytest
import torch

import spaa_oracle as so

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, F64 = torch.float32, torch.float64
NAN = float('nan')
PAD = 7                       # NaN rows past npix in every output buffer: a kernel must not write them

LAB_TOL = 3e-4                # Lab units
DE_TOL = 4e-5                 # x max(1, dE64)
G_TOL = 1e-5                  # d dE / d Lab, x |g64| where dE64 >= DE_TIGHT ...
G_COND = 8                    # ... plus G_COND * cond x |g64|, cond = 2^-24 max|Lab| / dE64 (fp32 rounding of the differences)
G_RGB_TOL = 2e-4              # d / d rgb, x max(|J|^T |g_lab|) (the reference's Lab knee has a 5e-5 slope step) ...
G_RGB_COND = 16               # ... plus G_RGB_COND * cond x the same scale
G_BWD_TOL = 1e-4              # rgb2lab_bwd, x max(|J|^T |g_lab|)  (likewise)
SUM_TOL = 4e-5                # block partial sums, x sum of max(1, |term|)
DEMAP_TOL = 1e-5              # the fused loss's de_map against spaa_ciede2000 at the same Lab, x max(1, dE)
DE_TIGHT = 1e-3
HUE_MARGIN = 1e-3             # degrees
KNEE = float(np.float32(0.0405))

MEASURED = {}


def record(key, v):
    """Largest finite value seen of a metric (non-finite ones fail their own check)."""
    v = torch.as_tensor(v, dtype=F64).view(-1)
    v = v[torch.isfinite(v)]
    if v.numel():
        MEASURED[key] = max(MEASURED.get(key, 0.0), float(v.max()))


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    if MEASURED:
        print('\n[color] largest over this module: ' + ', '.join(f'{k} {v:.2e}' for k, v in sorted(MEASURED.items())))


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    _lib.load()  # raises if the HIP library is missing: there is no fallback
    return _lib


def f32(x):
    """float64 array -> the nearest fp32 values, as float64."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# device plumbing: (N, 3) float64 <-> (N, 4) fp32 rows, alpha 0, PAD rows of NaN behind them
def dev4(x, alpha=0.0):
    n = x.shape[0]
    buf = torch.full((n + PAD, 4), NAN, dtype=F32)
    buf[:n, :3] = torch.as_tensor(x, dtype=F64).to(F32)
    buf[:n, 3] = alpha
    return buf.to(DEV)


def nan_rows(n, c=4):
    return torch.full((n + PAD, c), NAN, dtype=F32, device=DEV)


def host3(buf, n):
    """(N + PAD, 4) device buffer -> (N, 3) float64; the alpha lane must be 0 and the PAD rows untouched."""
    h = buf.cpu()
    assert (h[:n, 3] == 0).all(), 'alpha lane not 0'
    assert h[n:].isnan().all(), 'a row past npix was written'
    return h[:n, :3].to(F64)


def host1(buf, n):
    h = buf.cpu().view(-1)
    assert h[n:].isnan().all(), 'an element past npix was written'
    return h[:n].to(F64)


def k_rgb2lab(lib, rgb):
    n = rgb.shape[0]
    out, x = nan_rows(n), dev4(rgb)   # (device buffers held in locals: a temporary could hand its block to the next one)
    lib.call('spaa_rgb2lab', lib.ptr(x), lib.ptr(out), n)
    return host3(out, n)


def k_ciede(lib, l1, l2):
    n = l1.shape[0]
    out, a, b = torch.full((n + PAD,), NAN, dtype=F32, device=DEV), dev4(l1), dev4(l2)
    lib.call('spaa_ciede2000', lib.ptr(a), lib.ptr(b), lib.ptr(out), n)
    return host1(out, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references (the oracle, pixels laid out as a 1 x 3 x N x 1 image)
def img(x):
    return x.t().contiguous().view(1, 3, -1, 1)


def rows(x):
    return x.view(3, -1).t()


def lab64(rgb):
    """Lab(rgb) in float64 and the per-pixel Jacobian J[n, i, c] = d Lab_i / d rgb_c."""
    x = img(torch.as_tensor(rgb, dtype=F64)).requires_grad_(True)
    lab = rows(so.rgb2lab_diff(x))
    jac = torch.stack([rows(torch.autograd.grad(lab[:, i].sum(), x, retain_graph=True)[0]) for i in range(3)], dim=1)
    return lab.detach(), jac


def knee_other_side(rgb):
    """rgb with every channel that sits on the sRGB knee (within 1e-7) moved to the other side of it."""
    alt = rgb.clone()
    near = (rgb - KNEE).abs() < 1e-7
    alt[near & (rgb > 0.0405)] = 0.0405
    alt[near & (rgb <= 0.0405)] = math.nextafter(0.0405, 1.0)
    return alt, near.any(dim=1)


def _flipped(kind):
    """_dhpf / _ahpf of the oracle with the |dh'| <= 180 (kind 180) or |h1' + h2'| < 360 (kind 360) decision taken the other way
    where the float64 value lies within HUE_MARGIN of the switch."""
    def le180(d):
        le = d.abs() <= 180
        return le ^ ((d.abs() - 180).abs() < HUE_MARGIN) if kind == 180 else le

    def dhpf(c1, c2, h1p, h2p):
        d = h2p - h1p
        return torch.where(le180(d), d, torch.where(d > 0, d - 360, d + 360)) * ((c1 * c2) != 0)

    def ahpf(c1, c2, h1p, h2p):
        d, s = h2p - h1p, h1p + h2p
        lt = s.abs() < 360
        if kind == 360:
            lt = lt ^ ((s.abs() - 360).abs() < HUE_MARGIN)
        return torch.where(le180(d), s, torch.where(lt, s + 360, s - 360)) * ((c1 * c2) != 0) * 0.5
    return dhpf, ahpf


def de64(l1, l2, kind=None):
    """dE(l1, l2) and its gradients w.r.t. both colours in float64; `kind`: the hue decision flipped near its switch."""
    a = img(torch.as_tensor(l1, dtype=F64)).requires_grad_(True)
    b = img(torch.as_tensor(l2, dtype=F64)).requires_grad_(True)
    saved = so._dhpf, so._ahpf
    if kind is not None:
        so._dhpf, so._ahpf = _flipped(kind)
    try:
        d = so.ciede2000_diff(a, b)
    finally:
        so._dhpf, so._ahpf = saved
    d.sum().backward()
    return d.detach().view(-1), rows(a.grad), rows(b.grad)


def hue_near_switch(l1, l2):
    """(near |dh'| = 180, near |h1' + h2'| = 360) per pair, from the float64 hue angles of the oracle's formula."""
    l1, l2 = torch.as_tensor(l1, dtype=F64), torch.as_tensor(l2, dtype=F64)
    A1, B1, A2, B2 = l1[:, 1], l1[:, 2], l2[:, 1], l2[:, 2]
    m01, m02 = (A1 == 0) & (B1 == 0), (A2 == 0) & (B2 == 0)
    B1, B2 = B1 + 1e-4 * m01, B2 + 1e-4 * m02
    aC = (torch.sqrt(A1 ** 2 + B1 ** 2) + torch.sqrt(A2 ** 2 + B2 ** 2)) / 2
    G = 0.5 * (1 - torch.sqrt(aC ** 7 / (aC ** 7 + 25.0 ** 7)))
    h1 = so._hpf(B1, (1 + G) * A1) * ~m01
    h2 = so._hpf(B2, (1 + G) * A2) * ~m02
    d, s = (h2 - h1).abs(), (h1 + h2).abs()
    return (d - 180).abs() < HUE_MARGIN, ((s - 360).abs() < HUE_MARGIN) & (d > 180 - HUE_MARGIN)


def de_refs(l1, l2):
    """[(de, g1, g2), ...]: the float64 reference, plus the other side of a hue switch for pairs within HUE_MARGIN of one."""
    refs = [de64(l1, l2)]
    n180, n360 = hue_near_switch(l1, l2)
    if n180.any():
        refs.append(de64(l1, l2, 180))
    if n360.any():
        refs.append(de64(l1, l2, 360))
    return refs


# ---------------------------------------------------------------------------------------------------------------------------------
# per-pixel metrics: normalised so that <= 1 passes
def de_metric(dk, dr):
    return (dk - dr).abs() / (DE_TOL * dr.clamp_min(1.0))


def cond(l1, l2, dr):
    """Conditioning of d dE: an fp32 rounding of a Lab difference (2^-24 max|Lab|) against dE itself."""
    m = torch.maximum(l1.abs().amax(dim=1), l2.abs().amax(dim=1)).clamp_min(1.0)
    return 2.0 ** -24 * m / dr.clamp_min(1e-300)


def grad_metric(gk, gr, dr, scale, cnd, tol=G_TOL):
    """Where dr >= DE_TIGHT: max |gk - gr| / ((tol + G_COND cnd) scale).  Below: |gk| / (2 |gr|) (+ a tol * scale allowance).
    Non-finite kernel values give inf."""
    tight = dr >= DE_TIGHT
    err = (gk - gr).abs().amax(dim=1) / ((tol + G_COND * cnd) * scale).clamp_min(1e-300)
    loose = gk.norm(dim=1) / (2 * gr.norm(dim=1) + tol * scale).clamp_min(1e-300)
    m = torch.where(tight, err, loose)
    return torch.where(torch.isfinite(gk).all(dim=1), m, torch.full_like(m, math.inf)), torch.where(tight, err, 0 * err)


def best_side(per_ref):
    """per_ref: [(metric_de, metric_g), ...] for each reference side; per pixel, the side that fits best (both metrics from it)."""
    comb = torch.stack([torch.maximum(a, b) for a, b in per_ref])
    k = comb.argmin(dim=0)
    pick = lambda i: torch.stack([r[i] for r in per_ref]).gather(0, k[None])[0]  # noqa: E731
    return pick(0), pick(1), k


def check(name, metric, what):
    worst = float(metric.max()) if metric.numel() else 0.0
    assert math.isfinite(worst), f'{name}: non-finite {what} at {int((~torch.isfinite(metric)).sum())} of {metric.numel()} pixels'
    assert worst <= 1.0, f'{name}: {what} {worst:.3f} x its bound (pixel {int(metric.argmax())})'


# ---------------------------------------------------------------------------------------------------------------------------------
# case generators: float64 arrays of fp32 values
def lab_polar(L, C, h_deg):
    h = np.radians(h_deg)
    return f32(np.stack([L, C * np.cos(h), C * np.sin(h)], axis=1))


def hp_angles(l1, l2):
    """float64 h1', h2' of the formula (for rejection sampling)."""
    l1, l2 = torch.as_tensor(l1), torch.as_tensor(l2)
    A1, B1, A2, B2 = l1[:, 1], l1[:, 2], l2[:, 1], l2[:, 2]
    m01, m02 = (A1 == 0) & (B1 == 0), (A2 == 0) & (B2 == 0)
    B1, B2 = B1 + 1e-4 * m01, B2 + 1e-4 * m02
    aC = (torch.sqrt(A1 ** 2 + B1 ** 2) + torch.sqrt(A2 ** 2 + B2 ** 2)) / 2
    G = 0.5 * (1 - torch.sqrt(aC ** 7 / (aC ** 7 + 25.0 ** 7)))
    return (so._hpf(B1, (1 + G) * A1) * ~m01).numpy(), (so._hpf(B2, (1 + G) * A2) * ~m02).numpy()


def logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def sgn(rng, n):
    return rng.choice([-1.0, 1.0], n)


def lab_case(cat, n=2048, seed=0):
    rng = np.random.default_rng([seed, sum(map(ord, cat))])
    L = lambda k: rng.uniform(0, 100, k)  # noqa: E731
    if cat == 'random':
        l1 = f32(np.stack([L(n), rng.uniform(-128, 127, n), rng.uniform(-128, 127, n)], 1))
        far = f32(np.stack([L(n), rng.uniform(-128, 127, n), rng.uniform(-128, 127, n)], 1))
        near = f32(l1 + rng.standard_normal((n, 3)) * logu(rng, 1e-3, 5, n)[:, None])
        pick = rng.uniform(size=n) < 0.5
        return l1, np.where(pick[:, None], far, near)
    if cat == 'hue_wrap':
        C1, C2 = rng.uniform(0.5, 80, n), rng.uniform(0.5, 80, n)
        d1, d2 = logu(rng, 1e-6, 1, n) * sgn(rng, n), logu(rng, 1e-6, 1, n) * sgn(rng, n)
        l1, l2 = lab_polar(L(n), C1, d1), lab_polar(L(n), C2, d2)
        # b* = +-0.0 with a* < 0 (atan2 on the negative axis) and with a* > 0
        k = n // 4
        l1[:k, 1] = -np.abs(l1[:k, 1])
        l1[:k, 2] = np.where(rng.uniform(size=k) < 0.5, 0.0, -0.0)
        l2[k:2 * k, 2] = np.where(rng.uniform(size=k) < 0.5, 0.0, -0.0)
        return l1, l2
    if cat in ('dh180_below', 'dh180_above'):
        out1, out2 = [], []
        while sum(len(o) for o in out1) < n:
            m = 4 * n
            h1 = rng.uniform(0, 360, m)
            dlt = logu(rng, 1e-3, 2, m) * (-1 if cat == 'dh180_below' else 1)
            h2 = h1 + (180 + dlt) * sgn(rng, m)
            l1, l2 = lab_polar(L(m), rng.uniform(1, 100, m), h1), lab_polar(L(m), rng.uniform(1, 100, m), h2)
            a, b = hp_angles(l1, l2)
            d = np.abs(b - a)
            keep = (np.abs(d - 180) > 2 * HUE_MARGIN) & (np.abs(d - 180) < 3) & ((d < 180) == (cat == 'dh180_below'))
            out1.append(l1[keep])
            out2.append(l2[keep])
        return np.concatenate(out1)[:n], np.concatenate(out2)[:n]
    if cat in ('hs360_below', 'hs360_above'):
        out1, out2 = [], []
        while sum(len(o) for o in out1) < n:
            m = 4 * n
            h1 = rng.uniform(5, 85, m)
            eps = logu(rng, 1e-3, 2, m) * (-1 if cat == 'hs360_below' else 1)
            h2 = 360 - h1 + eps
            l1, l2 = lab_polar(L(m), rng.uniform(1, 100, m), h1), lab_polar(L(m), rng.uniform(1, 100, m), h2)
            sw = rng.uniform(size=m) < 0.5
            l1, l2 = np.where(sw[:, None], l2, l1), np.where(sw[:, None], l1, l2)
            a, b = hp_angles(l1, l2)
            s, d = a + b, np.abs(b - a)
            keep = (d > 180 + 2 * HUE_MARGIN) & (np.abs(s - 360) > 2 * HUE_MARGIN) & (np.abs(s - 360) < 3) & \
                   ((s < 360) == (cat == 'hs360_below'))
            out1.append(l1[keep])
            out2.append(l2[keep])
        return np.concatenate(out1)[:n], np.concatenate(out2)[:n]
    if cat == 'achromatic':
        l1 = lab_polar(L(n), rng.uniform(0.5, 80, n), rng.uniform(0, 360, n))
        l2 = lab_polar(L(n), rng.uniform(0.5, 80, n), rng.uniform(0, 360, n))
        q = n // 5
        l1[:q, 1:] = 0.0                                  # first achromatic
        l2[q:2 * q, 1:] = 0.0                             # second achromatic
        l1[2 * q:3 * q, 1:] = 0.0                         # both
        l2[2 * q:3 * q, 1:] = 0.0
        l1[3 * q:4 * q, 1] = 0.0                          # a* = 0 only
        l2[3 * q:4 * q, 2] = 0.0
        l1[4 * q:, 2] = 0.0                               # b* = 0 only
        l2[4 * q:, 1] = np.where(rng.uniform(size=n - 4 * q) < 0.5, 0.0, l2[4 * q:, 1])
        same_L = rng.uniform(size=n) < 0.3
        l2[same_L, 0] = l1[same_L, 0]
        return l1, l2
    if cat == 'low_chroma':
        L1 = L(n)
        dL = np.choose(rng.integers(0, 3, n), [np.zeros(n), rng.uniform(-1e-3, 1e-3, n), rng.uniform(-20, 20, n)])
        l1 = lab_polar(L1, logu(rng, 1e-7, 1e-4, n), rng.uniform(0, 360, n))
        l2 = lab_polar(np.clip(L1 + dL, 0, 100), logu(rng, 1e-7, 1e-4, n), rng.uniform(0, 360, n))
        q = n // 8                                        # one colour of ordinary chroma
        l2[:q] = lab_polar(L(q), rng.uniform(1, 60, q), rng.uniform(0, 360, q))
        l1[q:2 * q] = lab_polar(L(q), rng.uniform(1, 60, q), rng.uniform(0, 360, q))
        return l1, l2
    if cat == 'mean_L50_h275':
        L1 = f32(50 + rng.uniform(-40, 40, n))
        x = rng.uniform(0, 30, n)
        l1 = lab_polar(L1, rng.uniform(1, 80, n), 275 - x)
        l2 = lab_polar(100 - L1, rng.uniform(1, 80, n), 275 + x)
        l2[:, 0] = 100 - l1[:, 0]                         # exact in fp32: mean L is exactly 50
        return l1, l2
    if cat == 'identical':
        l1 = lab_polar(L(n), logu(rng, 1e-7, 100, n), rng.uniform(0, 360, n))
        l1[: n // 8, 1:] = 0.0
        return l1, l1.copy()
    if cat == 'one_ulp':
        l1 = lab_polar(L(n), logu(rng, 1e-6, 100, n), rng.uniform(0, 360, n))
        l1[: n // 8, 1:] = 0.0
        l2 = l1.astype(np.float32)
        c = rng.integers(0, 3, n)
        c[: n // 8] = 0                                   # (achromatic: L only; a step off a* = 0 would be a denormal)
        idx = np.arange(n)
        l2[idx, c] = np.nextafter(l2[idx, c], np.where(rng.uniform(size=n) < 0.5, np.float32(-np.inf), np.float32(np.inf)))
        return l1, l2.astype(np.float64)
    raise ValueError(cat)


LAB_CATS = ['random', 'hue_wrap', 'dh180_below', 'dh180_above', 'hs360_below', 'hs360_above', 'achromatic', 'low_chroma',
            'mean_L50_h275', 'identical', 'one_ulp']


def rgb_case(n, seed=0):
    """rgb in [0, 1]: exact black first, then the cube's corners, the sRGB knee and +-1 ulp, greys across the Lab knee (t = 0.008856
    at v ~ 0.0922), near-black and dark colours, then uniform colours."""
    rng = np.random.default_rng([seed, 11])
    kn = np.float32(KNEE)
    knees = np.array([np.nextafter(kn, np.float32(0)), kn, np.nextafter(kn, np.float32(1))], dtype=np.float64)
    sp = [np.zeros((1, 3)), np.array([[i >> 2 & 1, i >> 1 & 1, i & 1] for i in range(1, 8)], dtype=np.float64)]
    for c in range(3):
        r = rng.uniform(0, 1, (12, 3))
        r[:, c] = np.repeat(knees, 4)
        sp.append(r)
    sp.append(np.repeat(knees[:, None], 3, 1))
    g = 0.0922091470 + np.concatenate([rng.uniform(-2e-4, 2e-4, 40), np.arange(-8, 9) * 6e-9])
    sp.append(np.repeat(g[:, None], 3, 1))
    sp.append(logu(rng, 1e-7, 0.05, 60)[:, None] * np.ones((1, 3)))            # near-black greys
    sp.append(rng.uniform(0, 0.06, (60, 3)))
    sp.append(np.where(rng.uniform(size=(30, 3)) < 0.5, 0.0, rng.uniform(0, 1, (30, 3))))   # exact zeros in some channels
    spec = f32(np.clip(np.concatenate(sp), 0, 1))
    rest = f32(rng.uniform(0, 1, (max(n - len(spec), 0), 3)))
    return np.concatenate([spec, rest])[:n]


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('npix', [1, 255, 257, 262147])
def test_rgb2lab_and_bwd_vs_fp64(lib, npix):
    rgb = torch.from_numpy(rgb_case(npix, seed=npix))
    lab_k = k_rgb2lab(lib, rgb)
    alt, on_knee = knee_other_side(rgb)
    (l0, j0), (l1, j1) = lab64(rgb), lab64(alt)
    g_lab = torch.from_numpy(np.random.default_rng(npix).standard_normal((npix, 3)))
    out, x, gl = nan_rows(npix), dev4(rgb), dev4(g_lab, alpha=NAN)
    lib.call('spaa_rgb2lab_bwd', lib.ptr(x), lib.ptr(gl), lib.ptr(out), npix)
    g_k = host3(out, npix)
    sides = []
    for lab, jac in ((l0, j0), (l1, j1)):
        m_lab = (lab_k - lab).abs().amax(dim=1) / LAB_TOL
        g_ref = torch.einsum('nic,ni->nc', jac, g_lab)
        scale = torch.einsum('nic,ni->nc', jac.abs(), g_lab.abs()).amax(dim=1)
        m_g = (g_k - g_ref).abs().amax(dim=1) / (G_BWD_TOL * scale).clamp_min(1e-300)
        sides.append((m_lab, m_g))
    m_lab, m_g, side = best_side(sides)
    assert (side[~on_knee] == 0).all()
    record('rgb2lab lab_err', m_lab * LAB_TOL)
    record('rgb2lab_bwd g_err/scale', m_g * G_BWD_TOL)
    assert torch.isfinite(lab_k).all() and torch.isfinite(g_k).all()
    check(f'rgb2lab npix={npix}', m_lab, 'Lab error')
    check(f'rgb2lab_bwd npix={npix}', m_g, 'gradient error')
    assert (lab_k[0] == torch.tensor([-16.0, 0.0, 0.0], dtype=F64)).all()   # exact black: f(0) = 0 -> L = -16, a* = b* = 0
    assert (g_k[0] == 0).all()


def lab_pair_check(name, de_k, g1_k, g2_k, l1, l2, g_de=None):
    """The kernel's dE and (optionally) gradients against float64, either hue side near a switch; identical pairs exactly 0."""
    l1, l2 = torch.as_tensor(l1), torch.as_tensor(l2)
    gd = torch.ones(l1.shape[0], dtype=F64) if g_de is None else g_de
    sides, refs = [], de_refs(l1, l2)
    for dr, g1r, g2r in refs:
        m_de = de_metric(de_k, dr) if de_k is not None else torch.zeros_like(dr)
        m_g = torch.zeros_like(dr)
        for gk, gr in ((g1_k, g1r), (g2_k, g2r)):
            if gk is not None:
                gr = gr * gd[:, None]
                m, _ = grad_metric(gk, gr, dr, gr.norm(dim=1), cond(l1, l2, dr))
                m_g = torch.maximum(m_g, m)
        sides.append((m_de, m_g))
    m_de, m_g, _ = best_side(sides)
    if de_k is not None:
        record('ciede2000 de_err/max(1,dE)', m_de * DE_TOL)
        check(name, m_de, 'dE error')
    tight = refs[0][0] >= DE_TIGHT
    if g1_k is not None or g2_k is not None:
        record('ciede2000_bwd g_err/bound (dE>=1e-3)', m_g[tight])
        record('ciede2000_bwd |g|/(2|g64|) (dE<1e-3)', m_g[~tight])
        check(name, m_g, 'gradient error')
    same = (l1 == l2).all(dim=1)
    if de_k is not None:
        assert (de_k[same] == 0).all()
    for gk in (g1_k, g2_k):
        if gk is not None:
            assert (gk[same] == 0).all(), 'identical colours must have exactly zero gradient'


@pytest.mark.parametrize('cat', LAB_CATS)
def test_ciede2000_vs_fp64(lib, cat):
    l1, l2 = (torch.from_numpy(a) for a in lab_case(cat))
    de_k = k_ciede(lib, l1, l2)
    assert torch.isfinite(de_k).all()
    lab_pair_check(f'ciede2000[{cat}]', de_k, None, None, l1, l2)


@pytest.mark.parametrize('cat', LAB_CATS)
@pytest.mark.parametrize('which', ['lab1', 'lab2', 'both'])
def test_ciede2000_bwd_vs_fp64(lib, cat, which):
    l1, l2 = (torch.from_numpy(a) for a in lab_case(cat))
    n = l1.shape[0]
    g_de = torch.from_numpy(f32(np.random.default_rng(n).standard_normal(n)))
    gde_d = torch.full((n + PAD,), NAN, dtype=F32)
    gde_d[:n] = g_de.to(F32)
    gde_d, a, b = gde_d.to(DEV), dev4(l1), dev4(l2)
    o1 = nan_rows(n) if which in ('lab1', 'both') else None
    o2 = nan_rows(n) if which in ('lab2', 'both') else None
    lib.call('spaa_ciede2000_bwd', lib.ptr(a), lib.ptr(b), lib.ptr(gde_d), lib.ptr(o1), lib.ptr(o2), n)
    g1 = host3(o1, n) if o1 is not None else None
    g2 = host3(o2, n) if o2 is not None else None
    for g in (g1, g2):
        if g is not None:
            assert torch.isfinite(g).all(), f'{cat}: non-finite gradient at {int((~torch.isfinite(g).all(1)).sum())} of {n} pairs'
    lab_pair_check(f'ciede2000_bwd[{cat}, {which}]', None, g1, g2, l1, l2, g_de)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused stealthiness loss
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (0.3, 0.7), (0.0, 0.0)]
GSCALE = 0.37


def stealth_inputs(B, HW, seed):
    """y, scene (B*HW, 3) in [0, 1]: independent colours, small perturbations, identical pixels, grey pairs (v, v + 1e-3 / 1e-5 /
    1 ulp), dark colours; at HW >= 4001 the first 4001 pixels of sample 0 are the grey ramp v in [0, 0.2] against v + 1e-3."""
    rng = np.random.default_rng([seed, B, HW])
    n = B * HW
    s = rng.uniform(0, 1, (n, 3))
    kind = rng.choice(5, n, p=[0.35, 0.2, 0.15, 0.2, 0.1])
    y = rng.uniform(0, 1, (n, 3))
    pert = s + rng.standard_normal((n, 3)) * logu(rng, 1e-5, 0.1, n)[:, None]
    y = np.where((kind == 1)[:, None], pert, y)
    y = np.where((kind == 2)[:, None], s, y)
    v = rng.uniform(0, 0.2, n)
    step = np.choose(rng.integers(0, 3, n), [np.full(n, 1e-3), np.full(n, 1e-5), v * 2.0 ** -23])
    grey = kind == 3
    s[grey] = v[grey, None]
    y[grey] = (v + step)[grey, None]
    dark = kind == 4
    s[dark] = rng.uniform(0, 0.05, (dark.sum(), 3))
    y[dark] = rng.uniform(0, 0.05, (dark.sum(), 3))
    if HW >= 4001:
        ramp = np.linspace(0, 0.2, 4001)
        s[:4001] = ramp[:, None]
        y[:4001] = ramp[:, None] + 1e-3
    y, s = f32(np.clip(y, 0, 1)), f32(np.clip(s, 0, 1))
    y[y == s] = s[y == s]
    return torch.from_numpy(y), torch.from_numpy(s)


class StealthRef:
    """float64 per-pixel terms of one stealth case: ||scene - y|| and its gradient, dE at the kernel's Lab of y against the scene_lab
    buffer the launch reads (either hue side near a switch), d dE / d rgb through the float64 Jacobian, and its error scale."""

    def __init__(self, lib, y, s):
        n = y.shape[0]
        self.n = n
        self.lab_y = k_rgb2lab(lib, y)
        self.lab_s = k_rgb2lab(lib, s)
        d = s - y
        self.l2 = d.norm(dim=1)
        self.g_l2 = torch.where(self.l2[:, None] > 0, -d / self.l2.clamp_min(1e-300)[:, None], torch.zeros_like(d))
        self.same = (y == s).all(dim=1)
        # Lab(y) must agree with float64 before dE is judged at the kernel's Lab
        alt, _ = knee_other_side(y)
        knee_sides = [lab64(x) for x in (y, alt)]
        errs = [(self.lab_y - lab).abs().amax(dim=1) for lab, _ in knee_sides]
        record('stealth Lab(y) err', torch.minimum(*errs))
        assert float(torch.minimum(*errs).max()) <= LAB_TOL
        self.sides = []   # (either side of the sRGB knee for J) x (either hue side for dE)
        for dr, g1, _ in de_refs(self.lab_y, self.lab_s):
            dr = torch.where(self.same, torch.zeros_like(dr), dr)
            g1 = torch.where(self.same[:, None], torch.zeros_like(g1), g1)
            for _, jac in knee_sides:
                self.sides.append((dr, torch.einsum('nic,ni->nc', jac, g1),
                                   torch.einsum('nic,ni->nc', jac.abs(), g1.abs()).amax(dim=1), cond(self.lab_y, self.lab_s, dr)))

    def judge(self, name, de_k, g_k, cl2, cde, gscale):
        """Per pixel, the best hue side; returns the dE values of that side (for the partial sums)."""
        per = []
        for dr, gde, sc, cnd in self.sides:
            g_ref = gscale * (cl2 * self.g_l2 + cde * gde)
            scale = gscale * (abs(cl2) + abs(cde) * sc)
            m_de = de_metric(de_k, dr) if de_k is not None else torch.zeros_like(dr)
            if cde == 0:  # no dE term in the gradient: only the l2 one
                m_g = (g_k - g_ref).abs().amax(dim=1) / (G_RGB_TOL * scale).clamp_min(1e-300)
                m_g = torch.where(self.same, torch.zeros_like(m_g), m_g)
            else:
                tight = dr >= DE_TIGHT
                err = (g_k - g_ref).abs().amax(dim=1) / ((G_RGB_TOL + G_RGB_COND * cnd) * scale).clamp_min(1e-300)
                g_no_de = gscale * cl2 * self.g_l2
                loose = (g_k - g_no_de).norm(dim=1) / (2 * (g_ref - g_no_de).norm(dim=1) + G_RGB_TOL * scale).clamp_min(1e-300)
                m_g = torch.where(tight, err, loose)
            m_g = torch.where(torch.isfinite(g_k).all(dim=1), m_g, torch.full_like(m_g, math.inf))
            per.append((m_de, m_g))
        m_de, m_g, k = best_side(per)
        tight = torch.stack([s[0] for s in self.sides]).gather(0, k[None])[0] >= DE_TIGHT
        if cde != 0:
            record('stealth g_err/bound (dE>=1e-3)', m_g[tight])
            record('stealth |g|/(2|g64|) (dE<1e-3)', m_g[~tight])
        if de_k is not None:
            record('stealth de_err/max(1,dE)', m_de * DE_TOL)
            check(name, m_de, 'dE error')
        check(name, m_g, 'gradient error')
        return torch.stack([s[0] for s in self.sides]).gather(0, k[None])[0]


def partial_check(name, part, B, HW, l2, de):
    """partial[b][blk] = (sum ||d||, sum dE, sum dE^2) over a 256-pixel block, and the per-sample sums, against float64."""
    nblk = (HW + 255) // 256
    pad = nblk * 256 - HW
    def blocks(x):
        x = torch.cat([x.view(B, HW), torch.zeros(B, pad, dtype=F64)], dim=1)
        return x.view(B, nblk, 256)
    terms = [blocks(l2), blocks(de), blocks(de * de)]
    valid = blocks(torch.ones(B * HW, dtype=F64))
    ref = torch.stack([t.sum(dim=2) for t in terms], dim=2)
    bound = torch.stack([(t.abs().clamp_min(1.0) * valid).sum(dim=2) for t in terms], dim=2)
    m = (part.to(F64) - ref).abs() / (SUM_TOL * bound)
    record('stealth partial err/sum max(1,|t|)', m * SUM_TOL)
    assert torch.isfinite(part).all()
    check(name + ' block partials', m.view(-1), 'sum error')
    ps = part.to(F64).sum(dim=1)
    m_ps = (ps - ref.sum(dim=1)).abs() / (SUM_TOL * bound.sum(dim=1))
    check(name + ' per-sample sums', m_ps.view(-1), 'sum error')


def bits_equal(a, b):
    """Bitwise equal fp32 buffers (the NaN rows past the end included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_stealth(lib, yd, sd, labd, B, HW, w=None, params=None, de_map=True):
    n = B * HW
    nblk = (HW + 255) // 256
    g = nan_rows(n)
    dm = torch.full((n + PAD,), NAN, dtype=F32, device=DEV) if de_map else None
    part = torch.full((B * nblk * 3 + PAD,), NAN, dtype=F32, device=DEV)
    if params is None:
        lib.call('spaa_stealth_loss_fwd_bwd', lib.ptr(yd), lib.ptr(sd), lib.ptr(labd), float(w[0]), float(w[1]), GSCALE,
                 lib.ptr(g), lib.ptr(dm), lib.ptr(part), B, HW)
    else:
        lib.call('spaa_stealth_loss_fwd_bwd_ps', lib.ptr(yd), lib.ptr(sd), lib.ptr(labd), lib.ptr(params), GSCALE, lib.ptr(g),
                 lib.ptr(dm), lib.ptr(part), B, HW)
    torch.cuda.synchronize()
    pc = part.cpu()
    assert pc[B * nblk * 3:].isnan().all(), 'partial written past its end'
    return g, dm, pc[:B * nblk * 3].view(B, nblk, 3)


STEALTH_SHAPES = [(1, 1), (3, 1), (64, 1), (1, 257), (3, 257), (64, 257), (3, 44 * 68), (64, 44 * 68), (1, 240 * 320), (3, 240 * 320)]


@pytest.mark.parametrize('B,HW', STEALTH_SHAPES)
def test_stealth_loss_vs_fp64(lib, B, HW):
    y, s = stealth_inputs(B, HW, seed=1)
    n = B * HW
    ref = StealthRef(lib, y, s)
    yd, sd = dev4(y), dev4(s)
    labd = dev4(ref.lab_s)
    de_kc = k_ciede(lib, ref.lab_y, ref.lab_s)     # spaa_ciede2000(spaa_rgb2lab(y), scene_lab)
    for w in WEIGHTS:
        name = f'stealth B={B} HW={HW} w={w}'
        g, dm, part = run_stealth(lib, yd, sd, labd, B, HW, w)
        g_k, de_k = host3(g, n), host1(dm, n)
        assert torch.isfinite(g_k).all() and torch.isfinite(de_k).all()
        de_side = ref.judge(name, de_k, g_k, w[0], w[1], GSCALE)
        d_map = (de_k - de_kc).abs() / (DEMAP_TOL * de_kc.clamp_min(1.0))
        record('stealth de_map vs spaa_ciede2000 /max(1,dE)', d_map * DEMAP_TOL)
        check(name + ' de_map vs spaa_ciede2000', d_map, 'difference')
        assert (de_k[ref.same] == 0).all() and (g_k[ref.same] == 0).all(), 'identical pixels must give exactly zero'
        partial_check(name, part, B, HW, ref.l2, de_side)
        # bitwise reproducible, and de_map only adds a store
        g2, dm2, part2 = run_stealth(lib, yd, sd, labd, B, HW, w)
        assert bits_equal(g2, g) and bits_equal(dm2, dm) and bits_equal(part2, part)
        g3, _, part3 = run_stealth(lib, yd, sd, labd, B, HW, w, de_map=False)
        assert bits_equal(g3, g) and bits_equal(part3, part)


@pytest.mark.parametrize('B,HW', [(3, 44 * 68), (64, 257), (8, 240 * 320)])
def test_stealth_loss_ps_vs_fp64(lib, B, HW):
    """spaa_stealth_loss_fwd_bwd_ps: each sample's own (caml2_w, camdE_w), each sample against float64 with its weights."""
    y, s = stealth_inputs(B, HW, seed=2)
    n = B * HW
    ref = StealthRef(lib, y, s)
    rng = np.random.default_rng([B, HW])
    ws = [WEIGHTS[b] if b < len(WEIGHTS) else tuple(f32(rng.uniform(0, 1.5, 2) * (rng.uniform(size=2) < 0.8)))
          for b in range(B)]
    params = torch.tensor([[0.1 * (b % 2), ws[b][0], ws[b][1], 5.0 + b] for b in range(B)], dtype=F32, device=DEV)
    g, dm, part = run_stealth(lib, dev4(y), dev4(s), dev4(ref.lab_s), B, HW, params=params)
    g_k, de_k = host3(g, n), host1(dm, n)
    assert torch.isfinite(g_k).all() and torch.isfinite(de_k).all()
    de_all = torch.empty(n, dtype=F64)
    for b in range(B):
        sl = slice(b * HW, (b + 1) * HW)
        sub = StealthRef.__new__(StealthRef)
        sub.same, sub.g_l2 = ref.same[sl], ref.g_l2[sl]
        sub.sides = [tuple(t[sl] for t in side) for side in ref.sides]
        de_all[sl] = sub.judge(f'stealth_ps B={B} HW={HW} sample {b} w={ws[b]}', de_k[sl], g_k[sl], float(ws[b][0]),
                               float(ws[b][1]), GSCALE)
    partial_check(f'stealth_ps B={B} HW={HW}', part, B, HW, ref.l2, de_all)
