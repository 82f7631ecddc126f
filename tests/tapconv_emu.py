"""Test helper: a plain-PyTorch emulation of the tap-list convolution *semantics*
(include/spaa_hip.h, spaa_tapconv_t), used to check spaa_amd/convplan.py's tap/weight packing without a GPU and, in fp64 on the
GPU, as the reference of single kernel launches (tests/test_tuned_launches_gpu.py)."""
import torch
import torch.nn.functional as F


def packed_taps(plan, half=False):
    """Per class, the (dy, dx, W[n, c]) taps as the kernels read them: from the packed fp32 matrix `plan.weights` (on the plan's
    device), or with `half` from the fp16 plane `plan.half_plane()` (the operand of the fp16-storage kernels)."""
    out = []
    hp = plan.half_plane() if half else None
    off16 = 0
    for c, spec in zip(plan.cls, plan.classes_host):
        ngemm = plan.cout * getattr(plan, 'nfold', 1)
        if half:
            k64 = (c['K'] + 63) // 64 * 64
            wp = hp[off16:off16 + plan._npad * k64].view(plan._npad, k64)
            off16 += plan._npad * k64
        else:
            wp = plan.weights[c['w_off']:c['w_off'] + plan._npad * c['Kpad']].view(plan._npad, c['Kpad'])
        out.append([(dy, dx, wp[:ngemm, t * plan.cin_p:t * plan.cin_p + plan.cin])
                    for t, (dy, dx, _w) in enumerate(spec.taps)])
    return out


def emulate(plan, inp, hout, wout, dtype=torch.float32, device='cpu', taps=None, bias=True, magnitude=False):
    """inp [B,Hin,Win,Cs] (NHWC) -> out [B,hout,wout,cout] using plan.classes_host, in `dtype` on `device`.
    `taps`: per class a list of (dy, dx, W) to use instead of the host copies (packed_taps: what a kernel reads); `bias=False`: the
    bare sum of products; `magnitude`: also return s = sum |W| |x| over the same products (the scale of a rounding-error bound)."""
    b, hin, win, _ = inp.shape
    cin = plan.cin
    inp = inp[..., :cin].to(device=device, dtype=dtype)
    if taps is None:
        taps = [c.taps for c in plan.classes_host]
    taps = [[(dy, dx, w.to(device=device, dtype=dtype)) for dy, dx, w in t] for t in taps]
    ar = lambda n: torch.arange(n, device=device)   # noqa: E731
    out = torch.zeros(b, hout, wout, plan.cout, dtype=dtype, device=device)
    mag = torch.zeros_like(out) if magnitude else None

    def gather(iy, ix):
        vy, vx = (iy >= 0) & (iy < hin), (ix >= 0) & (ix < win)
        g = inp[:, iy.clamp(0, hin - 1)][:, :, ix.clamp(0, win - 1)]
        return g * (vy.view(1, -1, 1, 1) & vx.view(1, 1, -1, 1))

    if getattr(plan, 'nfold', 1) > 1:
        # spaa_tapconv_t.nfold: GEMM row c*Cout + n -> output pixel (2y + c//2, 2x + c%2), channel n
        # (k2/s2: the one tap (0, 0); k3/s2: the 2x2 neighbourhood, zero weights where a class has no tap)
        assert plan.s_in == 1 and plan.s_out == 2
        hm, wm = (hout + 1) // 2, (wout + 1) // 2
        acc = torch.zeros(b, hm, wm, 4 * plan.cout, dtype=dtype, device=device)
        sacc = torch.zeros_like(acc) if magnitude else None
        for dy, dx, w in taps[0]:
            g = gather(ar(hm) + dy, ar(wm) + dx)
            acc += g @ w.t()
            if magnitude:
                sacc += g.abs() @ w.abs().t()
        for c in range(4):
            oy, ox = 2 * ar(hm) + c // 2, 2 * ar(wm) + c % 2
            ky, kx = oy < hout, ox < wout
            out[:, oy[ky][:, None], ox[kx][None, :]] = acc[:, ky][:, :, kx][..., c * plan.cout:(c + 1) * plan.cout]
            if magnitude:
                mag[:, oy[ky][:, None], ox[kx][None, :]] = sacc[:, ky][:, :, kx][..., c * plan.cout:(c + 1) * plan.cout]
    else:
        for c, ctaps in zip(plan.classes_host, taps):
            if plan.s_out == 1:
                hm, wm = hout, wout
            else:
                hm, wm = (hout + 1) // 2, (wout + 1) // 2
            acc = torch.zeros(b, hm, wm, plan.cout, dtype=dtype, device=device)
            sacc = torch.zeros_like(acc) if magnitude else None
            ys, xs = ar(hm) * plan.s_in, ar(wm) * plan.s_in
            for dy, dx, w in ctaps:
                g = gather(ys + dy, xs + dx)
                acc += g @ w.t()
                if magnitude:
                    sacc += g.abs() @ w.abs().t()
            oy = c.oy0 + plan.s_out * ar(hm)
            ox = c.ox0 + plan.s_out * ar(wm)
            ky, kx = oy < hout, ox < wout
            out[:, oy[ky][:, None], ox[kx][None, :]] = acc[:, ky][:, :, kx]
            if magnitude:
                mag[:, oy[ky][:, None], ox[kx][None, :]] = sacc[:, ky][:, :, kx]
    if bias and plan.bias is not None:
        out = out + plan.bias.to(device=device, dtype=dtype)
    return (out, mag) if magnitude else out


def nhwc(x, cs=None):
    """NCHW -> NHWC with optional zero channel padding."""
    y = x.permute(0, 2, 3, 1).contiguous()
    if cs is not None and cs > y.shape[-1]:
        y = F.pad(y, (0, cs - y.shape[-1]))
    return y


def nchw(x, c=None):
    y = x.permute(0, 3, 1, 2)
    return (y[:, :c] if c is not None else y).contiguous()
