"""GPU (-m gpu): every pooling entry point -- csrc/pool_ops.hip and the global average pool of csrc/classifier_ops.hip -- launch by
launch against torch's CPU pooling and its autograd in float64 on the same inputs (fp16 storage: the inputs rounded to fp16 first).

Every launch route is reached directly: the generic max-pool gather (f32 / f16), the 2 x 2 one-thread-per-window path, the fp16
k3/s2/p1 quad adjoint, avg_pool2d with count_include_pad=True, adaptive_avg_pool2d with its +-1 window search, the global average
pool with its ReLU gate, the gate-byte writer, concatenation windows on either side and the launchers' argument checks.

Bounds.  A maximum is exact: pooled values and arg-max bytes are compared bitwise.  A gradient or an average is a sum in fp32:
  * fp32: max pool |err| <= 2^-22 * sum of |g| over the windows covering the element; averages within 1e-6 of max |ref|
  * fp16: within 1 fp16 ulp of the fp16-rounded float64 value (fp32 accumulation, one rounding on the way out)
Output buffers start as NaN, so an element a kernel does not write shows up; channels outside a concatenation window must stay NaN.
"""
import pytest
import torch
import torch.nn.functional as F

from tapconv_emu import nhwc, nchw

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F16, F32, F64 = torch.float16, torch.float32, torch.float64
NAN = float('nan')


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    _lib.load()  # raises if the HIP library is missing: there is no fallback
    return _lib


def sfx(dt):
    return '_f16' if dt == F16 else ''


def rnd(*shape, dt, quant=False):
    """float64 values representable in `dt`; `quant`: multiples of 1/4 -- many repeated values, so ties inside windows."""
    x = torch.randn(*shape, dtype=F64)
    if quant:
        x = torch.round(4 * x) / 4
    return x.to(dt).to(F64)


def nan_buf(*shape, dt):
    return torch.full(shape, NAN, device=DEV, dtype=dt)


def to_dev(x, dt, cs=None, coff=0):
    """NCHW float64 -> NHWC device buffer in `dt`; with `cs`: a NaN buffer of `cs` channels holding x at channels [coff, coff + C)."""
    y = nhwc(x).to(device=DEV, dtype=dt)
    if cs is None:
        return y
    buf = nan_buf(*y.shape[:3], cs, dt=dt)
    buf[..., coff:coff + y.shape[3]] = y
    return buf


def host(buf, c=None, coff=0):
    """NHWC device buffer (channel window [coff, coff + c)) -> NCHW float64 on the CPU."""
    c = buf.shape[3] - coff if c is None else c
    return nchw(buf[..., coff:coff + c].to(F64).cpu())


def outside_untouched(buf, coff, c):
    return bool(buf[..., :coff].isnan().all()) and bool(buf[..., coff + c:].isnan().all())


def same(a, b):
    """Equal values, NaN equal to NaN."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def ulp16(r):
    """Spacing of fp16 at the fp16 values r (float64): 2^-24 below the normal range."""
    a = r.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def err16(got, ref):
    """Largest distance of `got` from the fp16-rounded float64 `ref`, in fp16 ulps of the latter."""
    r = ref.to(F16).to(F64)
    assert not got.isnan().any(), 'element not written'
    return float(((got - r).abs() / ulp16(r)).max())


def err_rel(got, ref):
    """Largest |got - ref| relative to max |ref|."""
    assert not got.isnan().any(), 'element not written'
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# max pool
def maxpool_ref(x, g, k, s, p):
    """Reference of a launch on relu(x): pooled values, arg-max bytes (NHWC uint8), input gradients for relu_gate 1 (autograd of
    max_pool2d(relu(x)) w.r.t. x) and 0 (autograd of max_pool2d(xp) w.r.t. xp = relu(x)), and the sum of |g| over the windows
    covering each input element (the scale of the fp32 rounding bound)."""
    b, c, h, w = x.shape
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(F.relu(xr), k, s, p).backward(g)
    xp = F.relu(x).requires_grad_(True)
    pooled, idx = F.max_pool2d(xp, k, s, p, return_indices=True)
    pooled.backward(g)
    ho, wo = pooled.shape[2:]
    oy, ox = torch.arange(ho).view(1, 1, ho, 1), torch.arange(wo).view(1, 1, 1, wo)
    code = (idx // w - (oy * s - p)) * k + (idx % w - (ox * s - p))
    arg = nhwc(code + 128 * (pooled.detach() > 0)).to(torch.uint8)
    z = torch.zeros_like(x, requires_grad=True)
    (F.avg_pool2d(z, k, s, p, count_include_pad=True) * (k * k)).backward(g.abs())
    return pooled.detach(), arg, {1: xr.grad, 0: xp.grad}, z.grad


def run_maxpool(lib, x, g, k, s, p, dt, ocs=None, ocoff=0, gcs=None, gcoff=0):
    """spaa_maxpool_fwd(_f16) on relu(x), then spaa_maxpool_bwd(_f16) with relu_gate 1 and 0; the output and the output gradient in
    channel windows [ocoff, ocoff + C) of `ocs` and [gcoff, gcoff + C) of `gcs` channels.  Returns pooled values, arg-max bytes and
    {gate: input gradient} on the CPU (NCHW float64, NHWC uint8)."""
    b, c, h, w = x.shape
    ho, wo = out_size(h, k, s, p), out_size(w, k, s, p)
    ocs, gcs = ocs or c, gcs or c
    xin = to_dev(F.relu(x), dt)
    out = nan_buf(b, ho, wo, ocs, dt=dt)
    arg = torch.full((b, ho, wo, c), 0xff, dtype=torch.uint8, device=DEV)   # 0xff: no valid byte for k <= 11
    lib.call('spaa_maxpool_fwd' + sfx(dt), lib.hptr(xin), lib.hptr(out), lib.ptr(arg), b, h, w, c, ho, wo, k, s, p, ocs, ocoff)
    assert outside_untouched(out, ocoff, c), 'forward wrote outside its channel window'
    gbuf = to_dev(g, dt, gcs, gcoff)
    gin = {}
    for gate in (1, 0):
        buf = nan_buf(b, h, w, c, dt=dt)
        lib.call('spaa_maxpool_bwd' + sfx(dt), lib.hptr(gbuf), lib.ptr(arg), gate, lib.hptr(buf), b, h, w, c, ho, wo, k, s, p,
                 gcs, gcoff)
        gin[gate] = host(buf)
    return host(out, c, ocoff), arg.cpu(), gin


def check_maxpool(lib, x, g, k, s, p, dt, **win):
    """Launch and compare; returns the largest gradient error (fp32: in units of 2^-22 sum |g|; fp16: in ulps)."""
    geo = f'{dt} x{tuple(x.shape)} k{k} s{s} p{p} {win}'
    pooled, arg, gin = run_maxpool(lib, x, g, k, s, p, dt, **win)
    rp, rarg, rgin, sg = maxpool_ref(x, g, k, s, p)
    assert same(pooled, rp), f'pooled values: {geo}'
    assert torch.equal(arg, rarg), f'arg-max bytes: {geo}'
    worst = 0.0
    for gate in (1, 0):
        if dt == F16:
            e = err16(gin[gate], rgin[gate])
            assert e <= 1.0, f'gradient (gate {gate}): {e:.2f} ulp: {geo}'
        else:
            d = (gin[gate] - rgin[gate]).abs()
            assert bool((d <= 2.0 ** -22 * sg).all()), f'gradient (gate {gate}): {geo}'
            e = float((d / (2.0 ** -22 * sg).clamp_min(1e-300)).max())
        worst = max(worst, e)
    return worst


def grid():
    """k in {1, 2, 3, 4, 5, 11}, s in {1, 2, 3}, p in 0..k//2; Hin from the smallest valid size (Hin + 2p = k) up by 6, each paired
    with another Win of the same range: odd and even sides, partial last windows, padded borders, non-square maps."""
    i = 0
    for k in (1, 2, 3, 4, 5, 11):
        for s in (1, 2, 3):
            for p in range(k // 2 + 1):
                n0 = max(1, k - 2 * p)
                for j in range(7):
                    yield i, k, s, p, n0 + j, n0 + (3 * j + 1) % 7
                    i += 1


@pytest.mark.parametrize('dt', [F32, F16])
def test_maxpool_geometry_sweep(lib, dt):
    """Generic forward and backward kernels (and the 2 x 2 path where the sweep hits k2/s2/p0 on even sides) over the whole grid,
    C in {4, 8, 12}; every other geometry with quantised inputs (ties between positive values) -- zeros after the ReLU tie in
    every geometry.  The first maximum in row-major window order wins, as in ATen."""
    torch.manual_seed(11)
    worst = 0.0
    n = 0
    for i, k, s, p, h, w in grid():
        c = (4, 8, 12)[i % 3]
        x = rnd(2, c, h, w, dt=dt, quant=bool(i % 2))
        g = rnd(2, c, out_size(h, k, s, p), out_size(w, k, s, p), dt=dt)
        worst = max(worst, check_maxpool(lib, x, g, k, s, p, dt))
        n += 1
    unit = 'ulp' if dt == F16 else 'x 2^-22 sum|g|'
    print(f'maxpool sweep {dt}: {n} geometries, values and arg-max bitwise, largest gradient error {worst:.3f} {unit}')


@pytest.mark.parametrize('dt', [F32, F16])
def test_maxpool_nan_wins(lib, dt):
    """NaN contract of include/spaa_hip.h: a NaN of the input wins every window that holds it (ATen's max_pool2d).  Forward only;
    the generic kernel and the 2 x 2 path."""
    torch.manual_seed(12)
    for k, s, p, h, w, c in [(3, 2, 1, 9, 12, 8), (3, 2, 0, 11, 10, 4), (2, 2, 0, 7, 9, 12), (2, 2, 0, 8, 10, 16),
                             (3, 1, 1, 6, 5, 4), (5, 3, 2, 10, 13, 8)]:
        x = rnd(2, c, h, w, dt=dt)
        # one NaN per window at most: the corners (padded borders), and interior points k + 1 apart
        for bi, ci, yi, xi in [(0, 0, 0, 0), (0, 1, h - 1, w - 1), (1, c - 1, 0, w - 1), (1, 2, h - 1, 0), (0, 3, h // 2, w // 2)]:
            x[bi, ci, yi, xi] = NAN
        ho, wo = out_size(h, k, s, p), out_size(w, k, s, p)
        xin = to_dev(x, dt)
        out = nan_buf(2, ho, wo, c, dt=dt)
        arg = torch.full((2, ho, wo, c), 0xff, dtype=torch.uint8, device=DEV)
        lib.call('spaa_maxpool_fwd' + sfx(dt), lib.hptr(xin), lib.hptr(out), lib.ptr(arg), 2, h, w, c, ho, wo, k, s, p, c, 0)
        pooled, idx = F.max_pool2d(x, k, s, p, return_indices=True)
        oy, ox = torch.arange(ho).view(1, 1, ho, 1), torch.arange(wo).view(1, 1, 1, wo)
        code = (idx // w - (oy * s - p)) * k + (idx % w - (ox * s - p))
        assert pooled.isnan().any()
        assert same(host(out), pooled), (k, s, p, h, w, c)
        assert torch.equal(arg.cpu(), nhwc(code + 128 * (pooled > 0)).to(torch.uint8)), (k, s, p, h, w, c)
    print(f'maxpool NaN {dt}: NaN windows and arg-max bytes bitwise')


QUAD_SIDES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (3, 4), (4, 3), (5, 6), (6, 5), (7, 7), (8, 8), (9, 12), (13, 10), (28, 28),
              (29, 31), (56, 57)]


@pytest.mark.parametrize('dt', [F16, F32])
def test_maxpool_k3s2p1_routes(lib, dt):
    """k3/s2/p1, the ResNet-18 stem pool: spaa_maxpool_bwd_f16 takes the quad adjoint (a thread per 2 x 2 input block) on every
    side, odd and even, 1 x 1 included; fp32 takes the generic gather."""
    torch.manual_seed(13)
    worst = 0.0
    for i, (h, w) in enumerate(QUAD_SIDES):
        c = (4, 64)[i % 2]
        x = rnd(2, c, h, w, dt=dt, quant=bool(i % 3 == 0))
        g = rnd(2, c, out_size(h, 3, 2, 1), out_size(w, 3, 2, 1), dt=dt)
        worst = max(worst, check_maxpool(lib, x, g, 3, 2, 1, dt))
    print(f'maxpool k3/s2/p1 {dt}: largest gradient error {worst:.3f} {"ulp" if dt == F16 else "x 2^-22 sum|g|"}')


def test_maxpool2x2_f16_both_routes(lib):
    """k2/s2/p0 fp16 on even sides: C = 16 takes the one-thread-per-window path, C = 12 (not a multiple of 8) and C = 16 in a window
    at channel offset 4 take the generic kernels.  Same data: values, arg-max bytes and gradients bitwise those of the fast path."""
    torch.manual_seed(14)
    for h, w in [(2, 2), (6, 10), (14, 8), (32, 32)]:
        x = rnd(3, 16, h, w, dt=F16, quant=True)
        g = rnd(3, 16, h // 2, w // 2, dt=F16)
        fast = run_maxpool(lib, x, g, 2, 2, 0, F16)
        gen12 = run_maxpool(lib, x[:, :12].contiguous(), g[:, :12].contiguous(), 2, 2, 0, F16)
        gen_off = run_maxpool(lib, x, g, 2, 2, 0, F16, ocs=24, ocoff=4, gcs=24, gcoff=4)
        for gen, nc in ((gen12, 12), (gen_off, 16)):
            assert torch.equal(gen[0], fast[0][:, :nc]), (h, w, nc)
            assert torch.equal(gen[1], fast[1][..., :nc]), (h, w, nc)
            for gate in (1, 0):
                assert torch.equal(gen[2][gate], fast[2][gate][:, :nc]), (h, w, nc, gate)
        check_maxpool(lib, x[:, :12].contiguous(), g[:, :12].contiguous(), 2, 2, 0, F16)
    print('maxpool 2x2 fp16: generic routes bitwise equal to the window path')


# Inception-v3's branch pools that write into a concatenation: Mixed_6a (288 channels, 35 x 35 -> 17 x 17, at channel 480 of 768)
# and Mixed_7a (768 channels, 17 x 17 -> 8 x 8, at channel 512 of 1280)
CONCAT = [(288, 35, 768, 480), (768, 17, 1280, 512)]


@pytest.mark.parametrize('dt', [F32, F16])
def test_maxpool_concat_windows(lib, dt):
    torch.manual_seed(15)
    worst = 0.0
    for c, n, cs, coff in CONCAT:
        x = rnd(2, c, n, n, dt=dt)
        g = rnd(2, c, out_size(n, 3, 2, 0), out_size(n, 3, 2, 0), dt=dt)
        worst = max(worst, check_maxpool(lib, x, g, 3, 2, 0, dt, ocs=cs, ocoff=coff, gcs=cs, gcoff=coff))
    print(f'maxpool concat windows {dt}: largest gradient error {worst:.3f} {"ulp" if dt == F16 else "x 2^-22 sum|g|"}')


@pytest.mark.parametrize('b,c,h,k,s,p', [(64, 64, 147, 3, 2, 0), (64, 64, 112, 3, 2, 1)], ids=['inception_147', 'resnet_stem_112'])
def test_maxpool_f16_full_size(lib, b, c, h, k, s, p):
    """Full-size fp16 launches, many workgroups: Inception-v3's first pool (generic gather) and the ResNet-18 stem pool (quad)."""
    torch.manual_seed(16)
    ho = out_size(h, k, s, p)
    x = rnd(b, c, h, h, dt=F16)
    g = rnd(b, c, ho, ho, dt=F16)
    pooled, arg, gin = run_maxpool(lib, x, g, k, s, p, F16)
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(F.relu(xr), k, s, p).backward(g)
    xp = F.relu(x).requires_grad_(True)
    rp, idx = F.max_pool2d(xp, k, s, p, return_indices=True)
    rp.backward(g)
    oy, ox = torch.arange(ho).view(1, 1, ho, 1), torch.arange(ho).view(1, 1, 1, ho)
    code = (idx // h - (oy * s - p)) * k + (idx % h - (ox * s - p))
    assert torch.equal(pooled, rp.detach())
    assert torch.equal(arg, nhwc(code + 128 * (rp.detach() > 0)).to(torch.uint8))
    e = max(err16(gin[1], xr.grad), err16(gin[0], xp.grad))
    assert e <= 1.0
    print(f'maxpool fp16 {b}x{h}x{h}x{c} k{k}/s{s}/p{p}: values and arg-max bitwise, gradient {e:.3f} ulp')


# ---------------------------------------------------------------------------------------------------------------------------------
# avg_pool2d, count_include_pad=True
def check_avgpool(lib, x, g, k, s, p, dt, ocs=None, ocoff=0, gcs=None, gcoff=0):
    """spaa_avgpool2d_fwd / _bwd (_f16) against float64 avg_pool2d(count_include_pad=True) and its autograd; returns the largest
    error (fp32: relative to max |ref|; fp16: ulps)."""
    b, c, h, w = x.shape
    ho, wo = out_size(h, k, s, p), out_size(w, k, s, p)
    ocs, gcs = ocs or c, gcs or c
    geo = f'{dt} x{tuple(x.shape)} k{k} s{s} p{p} window {ocs, ocoff, gcs, gcoff}'
    xin, gbuf = to_dev(x, dt), to_dev(g, dt, gcs, gcoff)
    out = nan_buf(b, ho, wo, ocs, dt=dt)
    lib.call('spaa_avgpool2d_fwd' + sfx(dt), lib.hptr(xin), lib.hptr(out), b, h, w, c, ho, wo, k, s, p, ocs, ocoff)
    assert outside_untouched(out, ocoff, c), geo
    gin = nan_buf(b, h, w, c, dt=dt)
    lib.call('spaa_avgpool2d_bwd' + sfx(dt), lib.hptr(gbuf), lib.hptr(gin), b, h, w, c, ho, wo, k, s, p, gcs, gcoff)
    xr = x.clone().requires_grad_(True)
    y = F.avg_pool2d(xr, k, s, p, count_include_pad=True)
    y.backward(g)
    worst = 0.0
    for got, ref, what in ((host(out, c, ocoff), y.detach(), 'forward'), (host(gin), xr.grad, 'backward')):
        if dt == F16:
            e = err16(got, ref)
            assert e <= 1.0, f'{what}: {e:.2f} ulp: {geo}'
        else:
            e = err_rel(got, ref)
            assert e <= 1e-6, f'{what}: {e:.2e}: {geo}'
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize('dt', [F32, F16])
def test_avgpool2d_geometry_sweep(lib, dt):
    torch.manual_seed(21)
    worst = 0.0
    n = 0
    for i, k, s, p, h, w in grid():
        c = (4, 8, 12)[i % 3]
        x = rnd(2, c, h, w, dt=dt)
        g = rnd(2, c, out_size(h, k, s, p), out_size(w, k, s, p), dt=dt)
        worst = max(worst, check_avgpool(lib, x, g, k, s, p, dt))
        n += 1
    print(f'avgpool2d sweep {dt}: {n} geometries, largest error {worst:.3e} {"ulp" if dt == F16 else "rel"}')


@pytest.mark.parametrize('dt', [F32, F16])
def test_avgpool2d_inception_branch_pools(lib, dt):
    """Inception-v3's 3x3 / s1 / p1 branch pools at 35 x 35, 17 x 17 and 8 x 8 (their real channel counts), and the concatenation
    windows on the output side (forward) and on the gradient side (backward)."""
    torch.manual_seed(22)
    worst = 0.0
    for c, n in [(192, 35), (288, 35), (768, 17), (1280, 8), (2048, 8)]:
        worst = max(worst, check_avgpool(lib, rnd(2, c, n, n, dt=dt), rnd(2, c, n, n, dt=dt), 3, 1, 1, dt))
    for c, n, cs, coff in CONCAT:
        worst = max(worst, check_avgpool(lib, rnd(2, c, n, n, dt=dt), rnd(2, c, n, n, dt=dt), 3, 1, 1, dt, ocs=cs, ocoff=coff,
                                         gcs=cs, gcoff=coff))
        ho = out_size(n, 3, 2, 0)
        worst = max(worst, check_avgpool(lib, rnd(2, c, n, n, dt=dt), rnd(2, c, ho, ho, dt=dt), 3, 2, 0, dt, ocs=cs, ocoff=coff,
                                         gcs=cs, gcoff=coff))
    print(f'avgpool2d Inception branch pools {dt}: largest error {worst:.3e} {"ulp" if dt == F16 else "rel"}')


# ---------------------------------------------------------------------------------------------------------------------------------
# adaptive_avg_pool2d
def check_adaptive(lib, b, c, hin, win, hout, wout):
    """spaa_adaptive_avgpool_fwd / _bwd (without and with gate_in) against float64; returns the largest relative error.  A launch
    with Hin == Hout and Win == Wout must be bitwise the identity."""
    geo = (b, c, hin, win, hout, wout)
    x = rnd(b, c, hin, win, dt=F32)
    a = rnd(b, c, hin, win, dt=F32)        # random-sign gate
    g = rnd(b, c, hout, wout, dt=F32)
    xd, ad, gd = to_dev(x, F32), to_dev(a, F32), to_dev(g, F32)
    out = nan_buf(b, hout, wout, c, dt=F32)
    lib.call('spaa_adaptive_avgpool_fwd', lib.ptr(xd), lib.ptr(out), b, hin, win, c, hout, wout)
    gin = {}
    for gated in (False, True):
        buf = nan_buf(b, hin, win, c, dt=F32)
        lib.call('spaa_adaptive_avgpool_bwd', lib.ptr(gd), lib.ptr(ad if gated else None), lib.ptr(buf), b, hin, win,
                 c, hout, wout)
        gin[gated] = host(buf)
    y = F.adaptive_avg_pool2d(x, (hout, wout))
    xr = x.clone().requires_grad_(True)
    F.adaptive_avg_pool2d(xr, (hout, wout)).backward(g)
    ar = a.clone().requires_grad_(True)
    F.adaptive_avg_pool2d(F.relu(ar), (hout, wout)).backward(g)
    pairs = ((host(out), y, 'forward'), (gin[False], xr.grad, 'backward'), (gin[True], ar.grad, 'gated backward'))
    if (hin, win) == (hout, wout):
        assert torch.equal(host(out), x) and torch.equal(gin[False], g) and torch.equal(gin[True], g * (a > 0)), geo
    worst = 0.0
    for got, ref, what in pairs:
        e = err_rel(got, ref)
        assert e <= 1e-6, f'{what}: {e:.2e}: {geo}'
        worst = max(worst, e)
    return worst


def test_adaptive_avgpool_sweep(lib):
    """Every (Hin, Hout) with 1 <= Hin <= 24, 1 <= Hout <= 9, each with another (Win, Wout) of the same ranges (Win != Hin): upsampling
    (Hin < Hout), equal sizes and non-divisible downsampling -- the backward pass finds its windows through a +-1 search margin."""
    torch.manual_seed(31)
    worst = 0.0
    n = 0
    for hin in range(1, 25):
        for hout in range(1, 10):
            win = (hin - 1 + 7 * hout) % 24 + 1
            wout = (hout + hin) % 9 + 1
            worst = max(worst, check_adaptive(lib, 2, 8, hin, win, hout, wout))
            n += 1
    print(f'adaptive avgpool sweep: {n} launches, largest error {worst:.3e} rel')


def test_adaptive_avgpool_vgg(lib):
    """VGG-16's avgpool to 7 x 7: a 48 x 48 input (1 x 1 map, upsampled), 224 (7 x 7, the identity) and 256 (8 x 8)."""
    torch.manual_seed(32)
    worst = max(check_adaptive(lib, 3, 512, n, n, 7, 7) for n in (1, 7, 8))
    print(f'adaptive avgpool VGG-16 cases: largest error {worst:.3e} rel (7 x 7 -> 7 x 7 bitwise identity)')


# ---------------------------------------------------------------------------------------------------------------------------------
# global average pool (classifier heads)
@pytest.mark.parametrize('dt', [F32, F16])
def test_global_avgpool(lib, dt):
    """spaa_avgpool_fwd / _bwd (fp32) and _f16 (fp16 activation -> fp32 features; fp32 feature gradient -> fp16 input gradient),
    with the ReLU gate of `act` and without (NULL)."""
    torch.manual_seed(41)
    worst_f, worst_b = 0.0, 0.0
    b = 3
    for hw in (1, 4, 49, 64, 289):
        for c in (512, 2048):
            x = rnd(b, hw, c, dt=dt)
            g = rnd(b, c, dt=F32)
            xd = x.to(DEV, dt)
            out = torch.full((b, c), NAN, device=DEV, dtype=F32)
            lib.call('spaa_avgpool_fwd' + sfx(dt), lib.hptr(xd), lib.ptr(out), b, hw, c)
            e = err_rel(out.to(F64).cpu(), x.mean(1))
            assert e <= 1e-6, (hw, c, e)
            worst_f = max(worst_f, e)
            gd = g.to(DEV, F32)
            for gated in (False, True):
                gin = torch.full((b, hw, c), NAN, device=DEV, dtype=dt)
                lib.call('spaa_avgpool_bwd' + sfx(dt), lib.ptr(gd), lib.hptr(xd if gated else None), lib.hptr(gin), b, hw, c)
                xr = x.clone().requires_grad_(True)
                (F.relu(xr) if gated else xr).mean(1).backward(g)
                got = gin.to(F64).cpu()
                e = err16(got, xr.grad) if dt == F16 else err_rel(got, xr.grad)
                assert e <= (1.0 if dt == F16 else 1e-6), (hw, c, gated, e)
                worst_b = max(worst_b, e)
    print(f'global avgpool {dt}: forward {worst_f:.3e} rel, backward {worst_b:.3e} {"ulp" if dt == F16 else "rel"}')


# ---------------------------------------------------------------------------------------------------------------------------------
# gate bytes
@pytest.mark.parametrize('dt', [F32, F16])
def test_gate_mask_window(lib, dt):
    """spaa_gate_mask on a channel window: bit e of byte q = act[..., coff + 4q + e] > 0, bitwise; -0.0, +0.0 and NaN clear their
    bit, the smallest fp16 subnormal sets it; bytes outside the window are not touched; _lib.pack_gate_mask of the window slice
    gives the same bytes."""
    torch.manual_seed(51)
    tiny = 2.0 ** -24
    for m, cs, c, coff in [(7, 16, 8, 4), (578, 768, 288, 480), (128, 1280, 768, 512), (1000, 48, 20, 24), (3, 4, 4, 0)]:
        act = torch.randn(m, cs, dtype=F64)
        specials = torch.tensor([-0.0, 0.0, tiny, -tiny, NAN, float('inf'), -float('inf'), 1.0], dtype=F64)
        pos = torch.randint(0, m * cs, (4 * len(specials),))
        act.view(-1)[pos] = specials.repeat(4)
        act[0, coff:coff + min(8, c)] = specials[:min(8, c)]
        act = act.to(dt)
        assert dt == F32 or act[0, coff + 2].item() == tiny        # fp16 subnormal survives the conversion
        ad = act.to(DEV)
        fill = torch.randint(0, 256, (m, cs // 4), dtype=torch.uint8)
        mask = fill.to(DEV)
        lib.call('spaa_gate_mask', lib.hptr(ad), int(dt == F16), lib.ptr(mask), m, c, cs, coff)
        got = mask.cpu()
        bits = (act[:, coff:coff + c] > 0).view(m, c // 4, 4).to(torch.int32)
        want = (bits * torch.tensor([1, 2, 4, 8], dtype=torch.int32)).sum(-1).to(torch.uint8)
        q0, q1 = coff // 4, (coff + c) // 4
        assert torch.equal(got[:, q0:q1], want), (m, cs, c, coff)
        assert torch.equal(got[:, :q0], fill[:, :q0]) and torch.equal(got[:, q1:], fill[:, q1:]), (m, cs, c, coff)
        assert torch.equal(lib.pack_gate_mask(ad[:, coff:coff + c]).cpu(), want), (m, cs, c, coff)
        assert int(want[0, 0]) == 0x4                 # -0.0, +0.0, 2^-24, -2^-24: only the subnormal sets its bit
        if c >= 8:
            assert int(want[0, 1]) == 0xa             # NaN, +inf, -inf, 1.0
    print(f'gate mask {dt}: bitwise, window bytes only')


# ---------------------------------------------------------------------------------------------------------------------------------
# argument checks of the generic pool launchers
MAX_LAUNCHERS = ['spaa_maxpool_fwd', 'spaa_maxpool_fwd_f16', 'spaa_maxpool_bwd', 'spaa_maxpool_bwd_f16']
AVG_LAUNCHERS = ['spaa_avgpool2d_fwd', 'spaa_avgpool2d_fwd_f16', 'spaa_avgpool2d_bwd', 'spaa_avgpool2d_bwd_f16']


def launch_generic(lib, name, b, hin, win, c, hout, wout, k, s, p, cstride=None, coff=0):
    """One launch of a generic pool entry point on zeroed device buffers sized for the geometry exactly as given (channel window
    [coff, coff + C) of `cstride` channels on the pooled side; a buffer at least coff + C wide)."""
    dt = F16 if name.endswith('_f16') else F32
    cs = c if cstride is None else cstride
    big = torch.zeros(b, hin, win, c, device=DEV, dtype=dt)
    small = torch.zeros(b, hout, wout, max(cs, coff + c), device=DEV, dtype=dt)
    arg = torch.zeros(b, hout, wout, c, dtype=torch.uint8, device=DEV)
    geo = (b, hin, win, c, hout, wout, k, s, p, cs, coff)
    if name.startswith('spaa_maxpool_fwd'):
        lib.call(name, lib.hptr(big), lib.hptr(small), lib.ptr(arg), *geo)
    elif name.startswith('spaa_maxpool_bwd'):
        lib.call(name, lib.hptr(small), lib.ptr(arg), 1, lib.hptr(big), *geo)
    elif name.startswith('spaa_avgpool2d_fwd'):
        lib.call(name, lib.hptr(big), lib.hptr(small), *geo)
    else:
        lib.call(name, lib.hptr(small), lib.hptr(big), *geo)
    torch.cuda.synchronize()


@pytest.mark.parametrize('k', [12, 15])
@pytest.mark.parametrize('name', MAX_LAUNCHERS)
def test_maxpool_refuses_k_over_11(lib, name, k):
    """The arg-max byte holds the window offset ky * k + kx in bits 0-6 next to the sign flag in bit 7: k = 11 (offset <= 120) is
    the largest window it can encode."""
    launch_generic(lib, name, 1, 11, 12, 4, 1, 2, 11, 1, 0)       # k = 11 is accepted
    with pytest.raises(RuntimeError):
        launch_generic(lib, name, 1, k, k + 1, 4, 1, 2, k, 1, 0)


# (Hin, Win, Hout, Wout, k, s, p) that torch's pooling rejects: the input must cover one (padded) window, and the output size is
# floor((Hin + 2p - k) / s) + 1 -- the first three evaluate to 1 in C's truncating division
SHORT_INPUT = [(2, 5, 1, 2, 3, 2, 0), (5, 2, 2, 1, 3, 2, 0), (2, 5, 1, 1, 5, 3, 1)]
WRONG_SIZE = [(7, 7, 2, 3, 3, 2, 0), (7, 7, 4, 3, 3, 2, 0), (7, 8, 3, 4, 3, 2, 0), (7, 8, 3, 2, 3, 2, 0)]


@pytest.mark.parametrize('geo', SHORT_INPUT + WRONG_SIZE, ids=[f'short{i}' for i in range(len(SHORT_INPUT))] +
                         [f'size{i}' for i in range(len(WRONG_SIZE))])
@pytest.mark.parametrize('name', MAX_LAUNCHERS + AVG_LAUNCHERS)
def test_pool_refuses_bad_geometry(lib, name, geo):
    hin, win, hout, wout, k, s, p = geo
    with pytest.raises(RuntimeError):
        launch_generic(lib, name, 2, hin, win, 4, hout, wout, k, s, p)


@pytest.mark.parametrize('chan', [(6, 6, 0), (8, 8, 4), (8, 12, 8)], ids=['c_not_4', 'window_past_stride', 'window_past_stride2'])
@pytest.mark.parametrize('name', MAX_LAUNCHERS + AVG_LAUNCHERS)
def test_pool_refuses_bad_channels(lib, name, chan):
    c, cs, coff = chan
    with pytest.raises(RuntimeError):
        launch_generic(lib, name, 2, 7, 7, c, 3, 3, 3, 2, 0, cstride=cs, coff=coff)


@pytest.mark.parametrize('dt', [F32, F16])
def test_avgpool2d_large_windows(lib, dt):
    """The k <= 11 limit belongs to the arg-max byte: avg_pool2d keeps k up to 15, accepted and correct."""
    torch.manual_seed(61)
    worst = 0.0
    for k in (12, 13, 14, 15):
        for s, p in [(1, 0), (3, k // 2), (2, 1)]:
            h, w = max(1, k - 2 * p) + k % 3, max(1, k - 2 * p) + 4
            g = rnd(2, 8, out_size(h, k, s, p), out_size(w, k, s, p), dt=dt)
            worst = max(worst, check_avgpool(lib, rnd(2, 8, h, w, dt=dt), g, k, s, p, dt))
    print(f'avgpool2d k 12..15 {dt}: largest error {worst:.3e} {"ulp" if dt == F16 else "rel"}')
