"""GPU: the kernels of csrc/dwconv.hip through the C-ABI against float64.

Tolerances, with U = 2^-24.  The forward kernel accumulates acc = bias, then nine fmaf in a fixed order: at most 9 roundings, each of
relative size U on a partial sum bounded by |bias| + sum |w v|, so |out - out_64| <= 9 U (|bias| + sum |w v|) (1 + O(U)) before the
clamp; the tests allow 10 U (the clamp is 1-Lipschitz, so the bound holds after it).  The backward kernel likewise: 10 U sum |w g|.
Gate bytes are compared with 0 < out < 6 on the kernel's OWN output, exactly."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from spaa_amd import _lib
from spaa_amd.mobilenet import pack_gate6

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
SIZES = [(1, 1), (2, 3), (5, 7), (8, 8), (15, 17), (16, 16)]
CHANNELS = (4, 16, 36, 96)


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.load()


def osz(n, s):
    return (n - 1) // s + 1


def unpack(mask, c):
    """gate bytes [..., C / 4] -> bool [..., C]"""
    sh = torch.tensor([0, 1, 2, 3], device=mask.device)
    return ((mask.unsqueeze(-1).int() >> sh) & 1).bool().view(*mask.shape[:-1], c)


def nchw64(t):
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def w64(w):
    """[9][C] tap-major -> conv2d's depthwise weight [C, 1, 3, 3], float64"""
    return w.detach().cpu().double().t().reshape(-1, 1, 3, 3).contiguous()


def fwd(x, relu6, w, bias, stride, want_mask=True):
    b, h, wd, c = x.shape
    out = torch.full((b, osz(h, stride), osz(wd, stride), c), float('nan'), device=DEV)
    mask = torch.full((b, osz(h, stride), osz(wd, stride), c // 4), 0xAA, dtype=torch.uint8, device=DEV) if want_mask else None
    p = _lib.ptr
    _lib.call('spaa_dwconv3_fwd', p(x), int(relu6), p(w), p(bias), p(out), p(mask), b, h, wd, c, stride)
    return out, mask


def bwd(g_out, w, in_pre, shape, stride):
    b, h, wd, c = shape
    g_in = torch.full(shape, float('nan'), device=DEV)
    p = _lib.ptr
    _lib.call('spaa_dwconv3_bwd', p(g_out), p(w), p(in_pre), p(g_in), b, h, wd, c, stride)
    return g_in


def case(h, wd, c, b, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(b, h, wd, c, generator=g) * 4 + 2).to(DEV)          # both sides of [0, 6] are common
    w = (torch.randn(9, c, generator=g) * 0.5).to(DEV)
    bias = (torch.rand(c, generator=g) * 4 - 1).to(DEV)
    return x, w, bias


def ref_fwd(x, relu6, w, bias, stride):
    """float64 pre-clamp output and the bound's |bias| + sum |w v|, NHWC"""
    c = x.shape[3]
    x6 = nchw64(x)
    if relu6:
        x6 = x6.clamp(0, 6)
    pre = F.conv2d(x6, w64(w), bias.cpu().double(), stride, 1, 1, c)
    mag = F.conv2d(x6.abs(), w64(w).abs(), bias.cpu().double().abs(), stride, 1, 1, c)
    return nhwc(pre), nhwc(mag)


def ref_bwd(g_out, w, shape, stride):
    """float64 adjoint of the depthwise convolution applied to g_out, and sum |w g|, NHWC"""
    b, h, wd, c = shape
    outs = []
    for wt, go in ((w64(w), nchw64(g_out)), (w64(w).abs(), nchw64(g_out).abs())):
        xv = torch.zeros(b, c, h, wd, dtype=torch.float64, requires_grad=True)
        (F.conv2d(xv, wt, None, stride, 1, 1, c) * go).sum().backward()
        outs.append(nhwc(xv.grad))
    return outs


@pytest.mark.parametrize('h,wd', SIZES)
def test_forward_and_backward_against_float64(lib, h, wd):
    worst_f = worst_b = 0.0
    for c in CHANNELS:
        for stride in (1, 2):
            for b in (1, 3):
                x, w, bias = case(h, wd, c, b, 1000 * h + 10 * wd + c + stride + b)
                for relu6 in (0, 1):
                    out, mask = fwd(x, relu6, w, bias, stride)
                    pre, mag = ref_fwd(x, relu6, w, bias, stride)
                    o = out.cpu().double()
                    assert torch.isfinite(o).all() and o.shape == pre.shape
                    err = (o - pre.clamp(0, 6)).abs()
                    assert (err <= 10 * U * mag).all(), (c, stride, b, relu6, float((err / mag).max() / U))
                    worst_f = max(worst_f, float((err / mag).max() / U))
                    # gate bytes: 0 < out < 6 on the kernel's own output, exactly
                    assert torch.equal(mask, pack_gate6(out)), (c, stride, b, relu6)
                    # without a mask pointer the output is the same
                    assert torch.equal(fwd(x, relu6, w, bias, stride, want_mask=False)[0], out)
                    # two runs are bit for bit equal
                    out2, mask2 = fwd(x, relu6, w, bias, stride)
                    assert torch.equal(out2, out) and torch.equal(mask2, mask)
                    # backward: g_out arrives gated by the forward pass's own mask; in_pre gates the result (or does not)
                    gen = torch.Generator().manual_seed(7 + c + h)
                    g_out = torch.randn(out.shape, generator=gen).to(DEV) * unpack(mask, c)
                    want, gmag = ref_bwd(g_out, w, x.shape, stride)
                    for in_pre in ((x, None) if relu6 else (None,)):
                        g_in = bwd(g_out, w, in_pre, x.shape, stride)
                        gate = ((x > 0) & (x < 6)).cpu().double() if in_pre is not None else 1.0
                        gerr = (g_in.cpu().double() - want * gate).abs()
                        assert (gerr <= 10 * U * gmag).all(), (c, stride, b, in_pre is not None, float((gerr / gmag.clamp_min(1e-300)).max() / U))
                        worst_b = max(worst_b, float((gerr / gmag.clamp_min(1e-300)).max() / U))
                        if in_pre is not None:
                            assert (g_in[~((x > 0) & (x < 6))] == 0).all()
                        assert torch.equal(bwd(g_out, w, in_pre, x.shape, stride), g_in)
    print(f'{h} x {wd}: largest forward error {worst_f:.2f} U (|bias| + sum |w v|), largest backward error {worst_b:.2f} U sum |w g|')


@pytest.mark.parametrize('stride', (1, 2))
def test_adjoint_identity(lib, stride):
    """Gates off (every output strictly inside (0, 6), in_relu6 = 0, in_pre = NULL): <dw(x), g> = <x, dw^T(g)>, dw(x) = out - bias,
    evaluated in float64 on the kernels' outputs, within the two kernels' bounds summed against |g| and |x|."""
    for (h, wd) in SIZES:
        for c in (4, 36, 96):
            gen = torch.Generator().manual_seed(31 * h + wd + c)
            x = (torch.randn(3, h, wd, c, generator=gen) * 0.3).to(DEV)
            w = (torch.randn(9, c, generator=gen) * 0.3).to(DEV)
            bias = torch.full((c,), 3.0, device=DEV)
            out, mask = fwd(x, 0, w, bias, stride)
            assert (mask == 15).all(), 'the case must keep every output inside (0, 6)'
            g = torch.randn(out.shape, generator=gen).to(DEV)
            g_in = bwd(g, w, None, x.shape, stride)
            _, mag = ref_fwd(x, 0, w, bias, stride)
            _, gmag = ref_bwd(g, w, x.shape, stride)
            lhs = ((out.cpu().double() - 3.0) * g.cpu().double()).sum()
            rhs = (x.cpu().double() * g_in.cpu().double()).sum()
            tol = 10 * U * ((mag * g.cpu().double().abs()).sum() + (gmag * x.cpu().double().abs()).sum())
            assert abs(float(lhs - rhs)) <= float(tol), (h, wd, c, float(lhs), float(rhs), float(tol))


ULP6 = 2.0 ** -21      # spacing of fp32 just below 6 (above 6: 2^-21 as well up to 8)
PLANTED = [0.0, -0.0, 6.0, 6.0 - ULP6, 6.0 + ULP6, -2.5, 1e30]
# what a ReLU6 makes of them, and whether the gradient passes (0 < v < 6, strictly)
PLANTED_OUT = [0.0, 0.0, 6.0, 6.0 - ULP6, 6.0, 0.0, 6.0]
PLANTED_BIT = [False, False, False, True, False, False, False]


def planted_image():
    """[2, 5, 7, 8]: values strictly inside (0.5, 5.5) everywhere, the planted values in channel 1 along row 2 (of both samples; both strides read it), a NaN
    in channel 1 at the corner (0, 0)."""
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(2, 5, 7, 8, generator=gen) * 5 + 0.5
    x[:, 2, :, 1] = torch.tensor(PLANTED)
    x[:, 0, 0, 1] = float('nan')
    return x.to(DEV)


def check_planted(x, out, bits, rows, cols, nan_spreads):
    """`out` / `bits` against the input pixels x[:, rows][:, :, cols]: every channel but the planted one bit for bit, the planted channel
    by the table.  The NaN: a fmaxf / fminf clamp makes it 0 with a clear gate bit (include/spaa_hip.h); where the NaN reached its 3 x 3
    neighbours through 0 x NaN (in_relu6 = 0) those pixels of the planted channel are 0 with a clear bit too."""
    src = x[:, rows][:, :, cols]
    keep = [ch for ch in range(8) if ch != 1]
    assert torch.equal(out[..., keep].view(torch.int32), src[..., keep].view(torch.int32))      # neighbouring channels: bit for bit
    assert bits[..., keep].all()
    r3 = rows.index(2)
    planted = out[:, r3, :, 1]
    want = torch.tensor(PLANTED_OUT, device=DEV)[cols]
    wbit = torch.tensor(PLANTED_BIT, device=DEV)[cols]
    assert (planted == want).all(), planted.tolist()
    assert (bits[:, r3, :, 1] == wbit).all()
    assert (out[:, 0, 0, 1] == 0).all() and not bits[:, 0, 0, 1].any()                          # the NaN itself
    if not nan_spreads:   # every other pixel of the planted channel is an exact copy
        m = torch.ones(len(rows), len(cols), dtype=torch.bool)
        m[r3, :] = False
        m[0, 0] = False
        assert torch.equal(out[:, :, :, 1][:, m].view(torch.int32), src[:, :, :, 1][:, m].view(torch.int32))
        assert bits[:, :, :, 1][:, m].all()
    assert torch.isfinite(out).all()


@pytest.mark.parametrize('stride', (1, 2))
@pytest.mark.parametrize('relu6', (0, 1))
def test_planted_values_through_the_copying_convolution(lib, stride, relu6):
    x = planted_image()
    w = torch.zeros(9, 8, device=DEV)
    w[4] = 1.0                                   # the centre tap alone: the kernel copies its input
    bias = torch.zeros(8, device=DEV)
    out, mask = fwd(x, relu6, w, bias, stride)
    assert torch.equal(mask, pack_gate6(out))
    rows, cols = list(range(0, 5, stride)), list(range(0, 7, stride))
    check_planted(x, out, unpack(mask, 8), rows, cols, nan_spreads=not relu6)
    # backward with the same weight copies g_out to the pixels that were read, under the gate of in_pre
    g_out = torch.rand(out.shape, device=DEV) + 1.0
    g_in = bwd(g_out, w, x, x.shape, stride)
    gate = (x > 0) & (x < 6)
    want = torch.zeros_like(x)
    want[:, ::stride, ::stride] = g_out
    assert torch.equal(g_in, want * gate)
    assert (g_in[:, 2, :, 1][:, [0, 1, 2, 4, 5, 6]] == 0).all() and (g_in[:, 0, 0, 1] == 0).all()     # nothing passes at 0, 6 or beyond
    if stride == 1:
        assert torch.equal(g_in[:, 2, 3, 1], g_out[:, 2, 3, 1])       # 6 - ulp passes


def test_relu6_gate_and_pooled_gradient_on_the_planted_values(lib):
    x = planted_image()
    b, h, wd, c = x.shape
    act = x.clone()
    mask = torch.full((b, h, wd, c // 4), 0xAA, dtype=torch.uint8, device=DEV)
    _lib.call('spaa_relu6_gate', _lib.ptr(act), _lib.ptr(mask), b * h * wd, c)
    assert torch.equal(mask, pack_gate6(act))
    check_planted(x, act, unpack(mask, c), list(range(5)), list(range(7)), nan_spreads=False)
    act2 = x.clone()
    _lib.call('spaa_relu6_gate', _lib.ptr(act2), None, b * h * wd, c)                 # without gate bytes: the same values
    assert torch.equal(act2, act)
    # a larger one: more than one block, against torch
    y = (torch.randn(3, 15, 17, 96, generator=torch.Generator().manual_seed(2)) * 4 + 2).to(DEV)
    a = y.clone()
    m = torch.zeros(3, 15, 17, 24, dtype=torch.uint8, device=DEV)
    _lib.call('spaa_relu6_gate', _lib.ptr(a), _lib.ptr(m), 3 * 15 * 17, 96)
    assert torch.equal(a, y.clamp(0, 6)) and torch.equal(m, pack_gate6(y))
    # the head's backward step under these gate bytes: g_in = bit ? g_feat / HW : 0, a correctly rounded division (the float64
    # quotient of a 24-bit by an 8-bit number is never within 2^-53 of an fp32 rounding boundary without lying on it: rounding it to
    # fp32 gives the correctly rounded fp32 quotient)
    for (msk, shape) in ((mask, x.shape), (m, y.shape)):
        bb, hh, ww, cc = shape
        g_feat = torch.randn(bb, cc, generator=torch.Generator().manual_seed(3)).to(DEV)
        g_in = torch.full(shape, float('nan'), device=DEV)
        _lib.call('spaa_global_avgpool_bwd_bits', _lib.ptr(g_feat), _lib.ptr(msk), _lib.ptr(g_in), bb, hh * ww, cc)
        want = (g_feat.cpu().double() / (hh * ww)).float().to(DEV).view(bb, 1, 1, cc) * unpack(msk, cc)
        assert torch.equal(g_in, want.expand(shape).contiguous())
    g_in = torch.full(x.shape, float('nan'), device=DEV)
    g_feat = torch.ones(b, c, device=DEV)
    _lib.call('spaa_global_avgpool_bwd_bits', _lib.ptr(g_feat), _lib.ptr(mask), _lib.ptr(g_in), b, h * wd, c)
    assert (g_in[:, 2, :, 1] == torch.tensor(PLANTED_BIT, device=DEV) * (torch.ones(1, dtype=torch.float64) / 35).float().to(DEV)).all()


def test_invalid_arguments_are_refused_with_nothing_written(lib):
    st = _lib._stream
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    x = torch.rand(2, 5, 7, 8, device=DEV)
    w, bias = torch.rand(9, 8, device=DEV), torch.rand(8, device=DEV)
    out = torch.full((2, 5, 7, 8), -7.0, device=DEV)
    mask = torch.full((2, 5, 7, 2), 0x55, dtype=torch.uint8, device=DEV)
    g_in = torch.full((2, 5, 7, 8), -7.0, device=DEV)
    bad = [
        lib.spaa_dwconv3_fwd(P(x), 1, P(w), P(bias), P(out), P(mask), 2, 5, 7, 6, 1, st()),        # C % 4 != 0
        lib.spaa_dwconv3_fwd(P(x), 1, P(w), P(bias), P(out), P(mask), 2, 5, 7, 8, 3, st()),        # stride 3
        lib.spaa_dwconv3_fwd(None, 1, P(w), P(bias), P(out), P(mask), 2, 5, 7, 8, 1, st()),        # null pointers
        lib.spaa_dwconv3_fwd(P(x), 1, None, P(bias), P(out), P(mask), 2, 5, 7, 8, 1, st()),
        lib.spaa_dwconv3_fwd(P(x), 1, P(w), None, P(out), P(mask), 2, 5, 7, 8, 1, st()),
        lib.spaa_dwconv3_fwd(P(x), 1, P(w), P(bias), None, P(mask), 2, 5, 7, 8, 1, st()),
        lib.spaa_dwconv3_fwd(P(x), 1, P(w), P(bias), P(out), P(mask), 0, 5, 7, 8, 1, st()),        # empty batch
        lib.spaa_dwconv3_bwd(P(out), P(w), P(x), P(g_in), 2, 5, 7, 6, 1, st()),
        lib.spaa_dwconv3_bwd(P(out), P(w), P(x), P(g_in), 2, 5, 7, 8, 3, st()),
        lib.spaa_dwconv3_bwd(None, P(w), P(x), P(g_in), 2, 5, 7, 8, 1, st()),
        lib.spaa_dwconv3_bwd(P(out), None, P(x), P(g_in), 2, 5, 7, 8, 1, st()),
        lib.spaa_dwconv3_bwd(P(out), P(w), P(x), None, 2, 5, 7, 8, 1, st()),
        lib.spaa_relu6_gate(None, P(mask), 70, 8, st()),
        lib.spaa_relu6_gate(P(out), P(mask), 70, 6, st()),
        lib.spaa_relu6_gate(P(out), P(mask), 0, 8, st()),
        lib.spaa_global_avgpool_bwd_bits(None, P(mask), P(g_in), 2, 35, 8, st()),
        lib.spaa_global_avgpool_bwd_bits(P(bias), None, P(g_in), 2, 35, 8, st()),
        lib.spaa_global_avgpool_bwd_bits(P(bias), P(mask), None, 2, 35, 8, st()),
        lib.spaa_global_avgpool_bwd_bits(P(bias), P(mask), P(g_in), 2, 35, 6, st()),
    ]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad), bad
    assert (out == -7.0).all() and (mask == 0x55).all() and (g_in == -7.0).all()
    # ... and the wrapper turns a refusal into an exception
    with pytest.raises(RuntimeError, match='spaa_dwconv3_fwd failed'):
        _lib.call('spaa_dwconv3_fwd', P(x), 1, P(w), P(bias), P(out), P(mask), 2, 5, 7, 8, 3)
