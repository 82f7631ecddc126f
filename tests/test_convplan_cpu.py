"""CPU checks of the conv -> tap-list lowering (spaa_amd/convplan.py) against torch's own conv ops and autograd."""
import pytest
import torch
import torch.nn.functional as F

from spaa_amd import convplan as cp
from tapconv_emu import emulate, nhwc, nchw, packed_taps as cp_taps

torch.manual_seed(0)


@pytest.mark.parametrize('ci,co,k,s,p,h,w', [(3, 8, 3, 1, 1, 9, 11), (6, 5, 3, 2, 1, 12, 10), (4, 7, 1, 1, 0, 6, 5),
                                             (3, 4, 7, 2, 3, 20, 18), (5, 6, 1, 2, 0, 8, 8), (2, 3, 3, 2, 1, 9, 7)])
def test_conv_fwd_and_dgrad(ci, co, k, s, p, h, w):
    x = torch.randn(2, ci, h, w, requires_grad=True)
    wt = torch.randn(co, ci, k, k)
    b = torch.randn(co)
    y = F.conv2d(x, wt, b, s, p)
    plan = cp.conv_fwd_plan(wt, b, s, p, device='cpu')
    y2 = emulate(plan, nhwc(x.detach(), plan.cin_p), y.shape[2], y.shape[3])
    assert torch.allclose(nchw(y2), y, atol=1e-4)
    gy = torch.randn_like(y)
    y.backward(gy)
    dplan = cp.conv_dgrad_plan(wt, s, p, device='cpu')
    gx = emulate(dplan, nhwc(gy, dplan.cin_p), h, w)
    assert torch.allclose(nchw(gx), x.grad, atol=1e-4)


@pytest.mark.parametrize('ci,co,h,w', [(8, 32, 12, 10), (4, 64, 9, 7)])
def test_k3s2_classes_folded_into_gemm_rows(ci, co, h, w):
    """3x3 / stride-2 input gradient and transposed convolution with the four parity classes folded into the GEMM rows (zero
    weights where a class has no tap): the same result as the four separate classes."""
    x = torch.randn(2, ci, h, w, requires_grad=True)
    wt = torch.randn(co, ci, 3, 3)
    y = F.conv2d(x, wt, None, 2, 1)
    gy = torch.randn_like(y)
    y.backward(gy)
    dplan = cp.conv_dgrad_plan(wt, 2, 1, device='cpu', fold=True)
    assert dplan.nfold == 4 and dplan.ntaps_total == 4
    gx = emulate(dplan, nhwc(gy, dplan.cin_p), h, w)
    assert torch.allclose(nchw(gx), x.grad, atol=1e-4)
    xt = torch.randn(2, co, h, w)
    wtt = torch.randn(co, ci, 3, 3)
    yt = F.conv_transpose2d(xt, wtt, None, 2, 1, 1)
    tplan = cp.deconv_fwd_plan(wtt, None, 2, 1, device='cpu', fold=True)
    assert tplan.nfold == 4
    assert torch.allclose(nchw(emulate(tplan, nhwc(xt), yt.shape[2], yt.shape[3])), yt, atol=1e-4)


def test_conv_dgrad_channel_subset():
    x = torch.randn(1, 6, 8, 8, requires_grad=True)
    wt = torch.randn(5, 6, 3, 3)
    y = F.conv2d(x, wt, None, 2, 1)
    gy = torch.randn_like(y)
    y.backward(gy)
    dplan = cp.conv_dgrad_plan(wt, 2, 1, device='cpu', in_ch=(3, 6))
    gx = emulate(dplan, nhwc(gy, dplan.cin_p), 8, 8)
    assert torch.allclose(nchw(gx), x.grad[:, 3:6], atol=1e-4)


@pytest.mark.parametrize('ci,co,k,p,op,h,w', [(6, 4, 3, 1, 1, 5, 7), (5, 3, 2, 0, 0, 6, 4), (32, 8, 2, 0, 0, 5, 3)])
def test_deconv_fwd_and_dgrad(ci, co, k, p, op, h, w):
    x = torch.randn(2, ci, h, w, requires_grad=True)
    wt = torch.randn(ci, co, k, k)
    b = torch.randn(co)
    y = F.conv_transpose2d(x, wt, b, 2, p, op)
    plan = cp.deconv_fwd_plan(wt, b, 2, p, device='cpu')
    assert plan.nfold == (4 if (k == 2 and ci % 32 == 0) else 1)
    y2 = emulate(plan, nhwc(x.detach(), plan.cin_p), y.shape[2], y.shape[3])
    assert torch.allclose(nchw(y2), y, atol=1e-4)
    gy = torch.randn_like(y)
    y.backward(gy)
    dplan = cp.deconv_dgrad_plan(wt, 2, p, device='cpu')
    gx = emulate(dplan, nhwc(gy, dplan.cin_p), h, w)
    assert torch.allclose(nchw(gx), x.grad, atol=1e-4)


def test_linear_and_bn_fold():
    x = torch.randn(3, 10, requires_grad=True)
    w, b = torch.randn(7, 10), torch.randn(7)
    y = F.linear(x, w, b)
    plan = cp.linear_fwd_plan(w, b, device='cpu')
    y2 = emulate(plan, F.pad(x.detach(), (0, 2)).view(3, 1, 1, 12), 1, 1)
    assert torch.allclose(y2.view(3, 7), y, atol=1e-5)
    gy = torch.randn_like(y)
    y.backward(gy)
    dplan = cp.linear_dgrad_plan(w, device='cpu')
    gx = emulate(dplan, F.pad(gy, (0, 1)).view(3, 1, 1, 8), 1, 1)
    assert torch.allclose(gx.view(3, 10), x.grad, atol=1e-5)
    cw = torch.randn(4, 3, 3, 3)
    g, bb, m, v = torch.rand(4) + 0.5, torch.randn(4), torch.randn(4), torch.rand(4) + 0.5
    xi = torch.randn(1, 3, 6, 6)
    ref = F.batch_norm(F.conv2d(xi, cw, None, 1, 1), m, v, g, bb, False, 0.0, 1e-5)
    fw, fb = cp.fold_bn(cw, g, bb, m, v)
    assert torch.allclose(F.conv2d(xi, fw, fb, 1, 1), ref, atol=1e-5)


@pytest.mark.parametrize('ci,co,k,s,p,h,w', [(3, 64, 7, 2, 3, 14, 18), (3, 32, 3, 2, 1, 10, 12), (3, 64, 3, 1, 1, 7, 9), (3, 32, 3, 2, 0, 11, 9)])
def test_thin_fold_layout(ci, co, k, s, p, h, w):
    """The folded weight layout of the thin-output matrix-core kernel (ConvPlan.thin_fold, csrc/tapconv_thinmf.hip): emulated on the
    CPU exactly as the kernel reads it -- GEMM row = class * 4 + channel, [channel block][tap column][plane][tap row][16][32], the
    chunk swap of rows 8-15, output pixel (S y + class / S, S x + class % S) -- it gives the layer's input gradient; the three bf16
    planes sum to the fp32 weights exactly."""
    x = torch.randn(2, ci, h, w, requires_grad=True)
    wt = torch.randn(co, ci, k, k)
    y = F.conv2d(x, wt, None, s, p)
    gy = torch.randn_like(y)
    y.backward(gy)
    dplan = cp.conv_dgrad_plan(wt, s, p, device='cpu')
    assert dplan.thin_ok()
    S = dplan.s_out
    dy0, dy1, dx0, dx1 = dplan.tap_range
    tbh, tbw, nkb = max(dy1 - dy0 + 1, 2), dx1 - dx0 + 1, dplan.cin_p // 32
    planes = dplan.thin_fold(False).view(torch.bfloat16).view(nkb, tbw, 3, tbh, 16, 32).float()
    wsum = planes.sum(dim=2)                                           # h + m + l
    half = dplan.thin_fold(True).view(torch.float16).view(nkb, tbw, 1, tbh, 16, 32).float()[:, :, 0]
    assert (half - wsum).abs().max() <= 1e-3 * wsum.abs().max()
    un = wsum.view(nkb, tbw, tbh, 16, 4, 8).clone()                    # undo the chunk swap of rows 8-15
    un[..., 8:, 0, :], un[..., 8:, 2, :] = wsum.view(nkb, tbw, tbh, 16, 4, 8)[..., 8:, 2, :], wsum.view(nkb, tbw, tbh, 16, 4, 8)[..., 8:, 0, :]
    un[..., 8:, 1, :], un[..., 8:, 3, :] = wsum.view(nkb, tbw, tbh, 16, 4, 8)[..., 8:, 3, :], wsum.view(nkb, tbw, tbh, 16, 4, 8)[..., 8:, 1, :]
    wf = un.view(nkb, tbw, tbh, 16, 32).permute(3, 2, 1, 0, 4).reshape(16, tbh, tbw, dplan.cin_p)   # [row][dyi][dxi][c]
    g = nhwc(gy, dplan.cin_p)                                          # [B, Hm, Wm, cin_p] (class grid = its input grid)
    hm, wm = (h + S - 1) // S, (w + S - 1) // S                        # class grid; beyond gy: zeros
    gp = F.pad(g, (0, 0, max(-dx0, 0) + 4, dx1 + 4 + wm - g.shape[2], max(-dy0, 0) + 4, dy1 + 4 + hm - g.shape[1]))
    oy_, ox_ = max(-dy0, 0) + 4, max(-dx0, 0) + 4
    out = torch.zeros(2, h, w, 4)
    for cls in range(S * S):
        acc = torch.zeros(2, hm, wm, 4)
        for dyi in range(tbh):
            for dxi in range(tbw):
                patch = gp[:, oy_ + dy0 + dyi:oy_ + dy0 + dyi + hm, ox_ + dx0 + dxi:ox_ + dx0 + dxi + wm]
                acc += torch.einsum('bhwc,nc->bhwn', patch, wf[4 * cls:4 * cls + 4, dyi, dxi])
        cy, cx = cls // S, cls % S
        out[:, cy::S, cx::S] = acc[:, :(h - cy + S - 1) // S, :(w - cx + S - 1) // S]
    assert torch.allclose(nchw(out)[:, :ci], x.grad, atol=1e-3), float((nchw(out)[:, :ci] - x.grad).abs().max())
    assert (out[..., ci:] == 0).all()


@pytest.mark.parametrize('pad', [1, 0, 2])
def test_winograd_form_all_paddings(pad):
    """The Winograd F(2x2,3x3) form of a 3x3 / s1 plan (convplan.attach_winograd: U = G g G^T as a 16-'tap' matrix W[n][pos * Cin + c],
    run by csrc/tapconv_wino.hip) restated on the CPU: V = B^T d B of the 4 x 4 input patch whose origin is (2 ty - pad, 2 tx - pad),
    M[pos] = sum_c U[pos] V[pos], Y = A^T M A -- for the same-size layer (pad 1), the unpadded layer (pad 0: taps 0..2, output 2
    smaller) and its input gradient (pad 2: taps -2..0, output 2 larger), against torch's conv2d / autograd."""
    h, w = 9, 11
    torch.manual_seed(pad)
    if pad == 2:      # the unpadded layer 64 -> 32 read backwards: its output gradient [32, h, w] -> input gradient [64, h + 2, w + 2]
        wt = torch.randn(32, 64, 3, 3, dtype=torch.float64)
        src = torch.randn(2, 32, h, w, dtype=torch.float64)
        xin = torch.randn(2, 64, h + 2, w + 2, dtype=torch.float64, requires_grad=True)
        F.conv2d(xin, wt, None, 1, 0).backward(src)
        ref, plan = xin.grad, cp.conv_dgrad_plan(wt.float(), 1, 0, device='cpu')
    else:
        wt = torch.randn(64, 32, 3, 3, dtype=torch.float64)
        src = torch.randn(2, 32, h, w, dtype=torch.float64)
        ref, plan = F.conv2d(src, wt, None, 1, pad), cp.conv_fwd_plan(wt.float(), None, 1, pad, device='cpu')
    assert plan.wino is not None and plan.wino_pad == pad
    n_in, n_out = src.shape[1], ref.shape[1]
    kp = plan.wino.cls[0]['Kpad']
    U = plan.wino.weights[:plan.wino._npad * kp].view(plan.wino._npad, kp)[:n_out, :16 * n_in].double().view(n_out, 16, n_in)
    BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
    AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)
    ho, wo = ref.shape[2], ref.shape[3]
    big = F.pad(src, (pad, pad + 3, pad, pad + 3))          # zeros around: patches past the border read zeros, as the DMA does
    out = torch.zeros(2, n_out, ho + 1, wo + 1, dtype=torch.float64)
    for ty in range((ho + 1) // 2):
        for tx in range((wo + 1) // 2):
            d = big[:, :, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]                      # origin (2 ty - pad, 2 tx - pad) of the image
            V = torch.einsum('ij,bcjk,lk->bcil', BT, d, BT).reshape(2, n_in, 16)
            M = torch.einsum('npc,bcp->bnp', U, V).reshape(2, n_out, 4, 4)
            out[:, :, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = torch.einsum('ij,bnjk,lk->bnil', AT, M, AT)
    assert torch.allclose(out[:, :, :ho, :wo], ref.detach(), atol=1e-5)


def test_small_linear_plan_dispatch():
    """convplan.SmallLinearPlan (the classifiers' last layer at batch <= 64 on csrc/linear_small.hip): which calls take the dedicated
    kernel and which the wrapped 1 x 1 convolution plan; the wrapped plan's attributes stay reachable (flops, tune keys)."""
    w, b = torch.randn(12, 16), torch.randn(12)
    plan = cp.linear_fwd_plan(w, b, device='cpu')
    assert isinstance(plan, cp.SmallLinearPlan) and plan.n == 12 and plan.k == 16 and plan.cout == 12
    x, y = torch.zeros(3, 1, 1, 16), torch.zeros(3, 1, 1, 12)
    assert plan.applies(x, y, {})
    assert not plan.applies(x, y, {'act': 1})                                    # fused epilogue: the convolution tiles
    assert not plan.applies(x.half(), y, {})                                     # fp16 storage
    assert not plan.applies(torch.zeros(65, 1, 1, 16), torch.zeros(65, 1, 1, 12), {})   # more rows than the kernel is meant for
    assert not plan.applies(torch.zeros(3, 1, 1, 20), y, {})                     # a wider buffer (channel window)
    assert plan.flops(3, 1, 1) == plan.conv.flops(3, 1, 1)
    assert not isinstance(cp.linear_dgrad_plan(torch.randn(10, 16), device='cpu'), cp.SmallLinearPlan)   # 10 outputs: rows not 16-byte aligned


def _f64(t):
    return t.detach().double()


@pytest.mark.parametrize('kind', ['conv', 'conv_s2', 'dgrad_s2', 'dgrad_fold', 'deconv_fold', 'deconv_k3', 'deconv_dgrad', 'linear'])
def test_emulate_fp64_packed_taps(kind):
    """The fp64 reference of tests/test_tuned_launches_gpu.py: `emulate` in fp64 on the weights as the kernels read them (the packed
    fp32 matrix: packed_taps) equals torch's fp64 convolution ops of the fp32-rounded weights to the last bits, for every plan kind
    the benchmarked networks launch; the magnitude sum is the same op on |x| and |W|."""
    torch.manual_seed(7)
    b, h, w = 2, 9, 11
    if kind in ('conv', 'conv_s2'):
        s, co, ci = (1 if kind == 'conv' else 2), 40, 36
        wt, bias = torch.randn(co, ci, 3, 3), torch.randn(co)
        x = torch.randn(b, ci, h, w, dtype=torch.float64)
        plan = cp.conv_fwd_plan(wt, bias, s, 1, device='cpu')
        op = lambda x_, w_, b_: F.conv2d(x_, w_, b_, s, 1)   # noqa: E731
        wref, bref = _f64(wt), _f64(bias)
    elif kind in ('dgrad_s2', 'dgrad_fold'):
        co, ci = 64, 8
        wt = torch.randn(co, ci, 3, 3)
        x = torch.randn(b, co, (h + 1) // 2, (w + 1) // 2, dtype=torch.float64)
        plan = cp.conv_dgrad_plan(wt, 2, 1, device='cpu', fold=kind == 'dgrad_fold')
        assert (plan.nfold == 4) == (kind == 'dgrad_fold')
        op = lambda x_, w_, b_: torch.nn.grad.conv2d_input((b, ci, h, w), w_, x_, 2, 1)   # noqa: E731
        wref, bref = _f64(wt), None
    elif kind in ('deconv_fold', 'deconv_k3'):
        ci, co = 32, 12
        k, p, op_ = (2, 0, 0) if kind == 'deconv_fold' else (3, 1, 1)
        wt, bias = torch.randn(ci, co, k, k), torch.randn(co)
        x = torch.randn(b, ci, h, w, dtype=torch.float64)
        plan = cp.deconv_fwd_plan(wt, bias, 2, p, device='cpu', fold=True)
        assert plan.nfold == 4
        op = lambda x_, w_, b_: F.conv_transpose2d(x_, w_, b_, 2, p, op_)   # noqa: E731
        wref, bref = _f64(wt), _f64(bias)
    elif kind == 'deconv_dgrad':
        ci, co = 8, 12
        wt = torch.randn(ci, co, 3, 3)
        x = torch.randn(b, co, 2 * h, 2 * w, dtype=torch.float64)
        plan = cp.deconv_dgrad_plan(wt, 2, 1, device='cpu')
        op = lambda x_, w_, b_: F.conv2d(x_, w_, b_, 2, 1)   # noqa: E731
        wref, bref = _f64(wt), None
    else:
        wt, bias = torch.randn(24, 40), torch.randn(24)
        x = torch.randn(5, 40, 1, 1, dtype=torch.float64)
        plan = cp.linear_fwd_plan(wt, bias, device='cpu')
        plan = getattr(plan, 'conv', plan)
        op = lambda x_, w_, b_: F.linear(x_.flatten(1), w_, b_).view(5, -1, 1, 1)   # noqa: E731
        wref, bref = _f64(wt), _f64(bias)
    ref = op(x, wref, bref)
    sref = op(x.abs(), wref.abs(), None)
    y, sm = emulate(plan, nhwc(x, plan.cin_p), ref.shape[2], ref.shape[3], dtype=torch.float64, taps=cp_taps(plan), magnitude=True)
    assert y.dtype == torch.float64
    scale = sref.abs().max().item()
    assert (nchw(y) - ref).abs().max().item() <= 1e-12 * scale
    assert (nchw(sm) - sref).abs().max().item() <= 1e-12 * scale
    assert (nchw(emulate(plan, nhwc(x, plan.cin_p), ref.shape[2], ref.shape[3], dtype=torch.float64, taps=cp_taps(plan), bias=False))
            - op(x, wref, None)).abs().max().item() <= 1e-12 * scale
    # the fp16 plane: the same sums over the fp16-rounded weights
    yh = emulate(plan, nhwc(x, plan.cin_p), ref.shape[2], ref.shape[3], dtype=torch.float64, taps=cp_taps(plan, half=True))
    assert (nchw(yh) - op(x, wref.half().double(), bref)).abs().max().item() <= 1e-12 * scale


def test_bf16_planes_one_split_everywhere():
    """The three bf16 planes (w == h + m + l exactly) as `split_planes`, the constructor, `thin_fold(False)`, `c3_pack()` and
    `_winograd_weights` make them: each sums back to its fp32 matrix bit for bit and equals `split_planes` of that matrix; the
    planes of one small seeded weight are those kept in tests/golden/convplan_launches.json."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'convplan_launches.json')) as fh:
        want = json.load(fh)['planes']
    w = torch.randn(*want['shape'], generator=torch.Generator().manual_seed(want['seed']))

    def check(planes, fp32=None):
        pl = planes.view(torch.int16).reshape(3, -1)
        s = pl.view(torch.bfloat16).float()
        total = s[0] + s[1] + s[2]                      # (8 + 8 + 8 mantissa bits: exact in fp32)
        assert torch.equal(cp.split_planes(total).reshape(3, -1), pl)
        if fp32 is not None:
            assert torch.equal(total, fp32.reshape(-1))
        return total

    assert cp.split_planes(w).tolist() == want['int16']
    check(cp.split_planes(w), w)
    plan = cp.linear_dgrad_plan(w, device='cpu')            # [32 outputs, 4 inputs]: the constructor's planes, per class [3][Npad][Kpad]
    plan = getattr(plan, 'conv', plan)
    check(plan.w_split, plan.weights)
    assert torch.equal(plan.w_split.view(3, plan._npad, -1)[:, :32, :4], cp.split_planes(w.t().contiguous()))
    thin = cp.conv_dgrad_plan(torch.randn(32, 3, 3, 3), 2, 1, device='cpu')
    assert thin.thin_ok()
    t = thin.thin_fold(False)
    nkb, tbw = thin.cin_p // 32, thin.tap_range[3] - thin.tap_range[2] + 1
    check(t.view(nkb, tbw, 3, -1).permute(2, 0, 1, 3).contiguous())
    c3 = cp.conv_fwd_plan(torch.randn(64, 3, 3, 3), None, 1, 1, device='cpu')
    assert c3.c3_ok()
    tot = check(c3.c3_pack().view(1, 3, -1).permute(1, 0, 2).contiguous())
    assert sorted(tot[tot != 0].tolist()) == sorted(c3.weights[c3.weights != 0].tolist())
    wino = cp.conv_fwd_plan(torch.randn(64, 32, 3, 3), None, 1, 1, device='cpu').wino
    check(wino.w_split, wino.weights)


def test_debug_word_places_every_switch_in_its_field(monkeypatch):
    """`reserved0` of a launch (convplan.debug_word): 0 but for the Winograd padding code with no switch set; every DEBUG_* value that
    the tests and tools/lab use lands in its named field and nowhere else; a value that does not fit its field is refused instead of
    running over into the next one."""
    from spaa_amd import _lib
    assert cp.debug_word(37) == cp.debug_word(72) == 0
    assert [cp.debug_word(70, pad) >> _lib.WINO_PAD_SHIFT for pad in (1, 0, 2)] == [cp.wino_pad_code(pad) for pad in (1, 0, 2)] == [0, 1, 2]
    for cap in (8, 24, 128, 1 | 2 | 4 | 8 | 32, 255):     # (tests: 8 / 24 workgroups; tools/lab/x6p_stamps.py: its ablation masks, 128 = stamps on)
        monkeypatch.setattr(cp, 'DEBUG_PERSIST_CAP', cap)
        assert cp.debug_word(51) == cap << _lib.DBG_PERSIST_CAP_SHIFT == cp.debug_word(51) & _lib.DBG_PERSIST_CAP
    monkeypatch.setattr(cp, 'DEBUG_PERSIST_CAP', 256)
    with pytest.raises(ValueError, match='DEBUG_PERSIST_CAP'):
        cp.debug_word(51)
    monkeypatch.setattr(cp, 'DEBUG_PERSIST_CAP', 0)
    for dbg in (1, 33, 64, 96):                           # (tools/lab/wino_ablate.py: DEBUG_WINO = dbg << 2; wino_one.py: 256 = 64 << 2)
        monkeypatch.setattr(cp, 'DEBUG_WINO', dbg << 2 | 3)
        assert cp.debug_word(70) == dbg << _lib.DBG_WINO_ABLATE_SHIFT | _lib.DBG_WINO_VAR
    monkeypatch.setattr(cp, 'DEBUG_WINO', 128 << 2)      # past bit 24
    with pytest.raises(ValueError, match='DEBUG_WINO'):
        cp.debug_word(70)
    monkeypatch.setattr(cp, 'DEBUG_WINO', 0)
    monkeypatch.setattr(cp, 'DEBUG_THINMF', 1)
    assert cp.debug_word(72) == 1 << _lib.DBG_THINMF_SHIFT and cp.debug_word(70) == 0
    monkeypatch.setattr(cp, 'DEBUG_THINMF', 0)
    for nc, want in ((1, _lib.WINO_NO_CANVAS), (2, _lib.WINO_FORCE_CANVAS)):
        monkeypatch.setattr(cp, 'DEBUG_WINO_NOCANVAS', nc)
        assert cp.debug_word(71) == want and cp.debug_word(68) == 0
    monkeypatch.setattr(cp, 'DEBUG_WINO_NOCANVAS', 0)
    for name, flag in (('DEBUG_TAPMAJOR', _lib.DBG_X6D_TAPMAJOR), ('DEBUG_H16_2STAGE', _lib.DBG_H16_2STAGE), ('DEBUG_SMALLCIN_NOSLAB', _lib.DBG_SMALLCIN_NOSLAB)):
        monkeypatch.setattr(cp, name, 1)
        assert cp.debug_word(37) == flag
        monkeypatch.setattr(cp, name, 2)
        with pytest.raises(ValueError, match=name):
            cp.debug_word(37)
        monkeypatch.setattr(cp, name, 0)
