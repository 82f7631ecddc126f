"""One Python wrapper per pooling kernel family of include/spaa_hip.h (max, average, global average, adaptive average, and the
ReLU-gate bytes of a pooled activation).  A wrapper takes TENSORS plus the window (k, s, p) and channel offsets: every integer a
kernel gets is read off the tensors' shapes here, the entry point follows from their storage type, and what the kernels assume about
the buffers behind their pointers is checked on the host first -- a wrong size, channel stride or offset is a ValueError naming the
operand, not a wild write on the GPU.  The C side checks its integers against each other (pool_ops.hip geo_ok); it cannot see the
buffers.

All activations and gradients are contiguous NHWC, fp32 or fp16 (fp16 storage: the `_f16` entry points), of one storage type per
call.  A "window" is channels [coff, coff + C) of a wider buffer (the concatenations of Inception-v3)."""
import torch

from . import _lib

MAX_K, AVG_K = 11, 15      # max: the arg-max byte holds ky * k + kx <= 120 in bits 0-6; avg: the kernel's bound


def _acts(fn, **tensors):
    """`tensors`: the call's activations / gradients by operand name (None: absent).  4-D, one storage type, one batch, on the
    current GPU.  Returns whether that storage type is fp16."""
    first = None
    for name, t in tensors.items():
        if t is None:
            continue
        if t.ndim != 4 or t.dtype not in (torch.float32, torch.float16):
            raise ValueError(f'{fn}: `{name}` must be a 4-D NHWC tensor, fp32 or fp16 (got {tuple(t.shape)}, {t.dtype})')
        first = first or (name, t)
        if t.dtype != first[1].dtype or t.shape[0] != first[1].shape[0]:
            raise ValueError(f'{fn}: `{name}` ({t.dtype}, batch {t.shape[0]}) must have the storage type and batch of '
                             f'`{first[0]}` ({first[1].dtype}, batch {first[1].shape[0]})')
    _lib.check_dev(*tensors.values(), half_ok=True)
    return first[1].dtype == torch.float16


def _shaped(fn, name, t, shape, dtype):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f'{fn}: `{name}` must be {dtype} {tuple(shape)} (got {t.dtype} {tuple(t.shape)})')


def _bytes(fn, name, t, shape):
    """Pointer of an arg-max / gate-mask buffer."""
    _shaped(fn, name, t, shape, torch.uint8)
    _lib.check_mask(t)
    return _lib.ptr(t)


def _channels(fn, name, c, cstride, coff):
    if c < 4 or c % 4 or cstride % 4 or coff % 4 or coff < 0 or coff + c > cstride:
        raise ValueError(f'{fn}: channels [{coff}, {coff} + {c}) of `{name}` ({cstride} wide): C, offset and width must be '
                         'multiples of 4 and the window must lie inside the buffer')


def _window(fn, full, full_name, pooled, pooled_name, k, s, p, coff, kmax):
    """`full` [B, Hin, Win, C] and its pooled side, channels [coff, coff + C) of `pooled` [B, Hout, Wout, cstride]: the integer
    arguments B, Hin, Win, C, Hout, Wout, k, s, p, cstride, coff of the generic kernels."""
    b, hin, win, c = full.shape
    _, hout, wout, cstride = pooled.shape
    if not (1 <= k <= kmax and s >= 1 and 0 <= 2 * p <= k and hin + 2 * p >= k and win + 2 * p >= k):
        raise ValueError(f'{fn}: window k={k}, s={s}, p={p} on `{full_name}` {hin} x {win}: needs 1 <= k <= {kmax}, s >= 1, '
                         '2p <= k and one whole padded window')
    want = (hin + 2 * p - k) // s + 1, (win + 2 * p - k) // s + 1
    if (hout, wout) != want:
        raise ValueError(f'{fn}: `{pooled_name}` is {hout} x {wout}, the window k={k}, s={s}, p={p} on `{full_name}` '
                         f'{hin} x {win} gives {want[0]} x {want[1]}')
    _channels(fn, pooled_name, c, cstride, coff)
    return b, hin, win, c, hout, wout, k, s, p, cstride, coff


def _is_3s2(h16, k, s, p, geo):
    """fp32, MaxPool2d(3, 2, 1) into a whole buffer: the kernel pair written for ResNet-18's stem (spaa_maxpool3s2_*; its backward
    pass gathers per 2 x 2 quad of inputs).  The ONE place where that choice is made."""
    c, cstride, coff = geo[3], geo[9], geo[10]
    return not h16 and (k, s, p) == (3, 2, 1) and coff == 0 and cstride == c


def maxpool_fwd(x, out, arg, k, s, p, out_coff=0):
    """MaxPool2d(k, s, p) of `x` into channels [out_coff, ...) of `out`; `arg` uint8 [B, Hout, Wout, C]: window offset + "maximum > 0"."""
    h16 = _acts('maxpool_fwd', x=x, out=out)
    geo = _window('maxpool_fwd', x, 'x', out, 'out', k, s, p, out_coff, MAX_K)
    ptrs = _lib.hptr(x), _lib.hptr(out), _bytes('maxpool_fwd', 'arg', arg, (geo[0], geo[4], geo[5], geo[3]))
    if _is_3s2(h16, k, s, p, geo):
        _lib.call('spaa_maxpool3s2_fwd', *ptrs, *geo[:6])
    else:
        _lib.call('spaa_maxpool_fwd_f16' if h16 else 'spaa_maxpool_fwd', *ptrs, *geo)


def maxpool_bwd(g_out, arg, g_in, k, s, p, relu_gate, gout_coff=0, c=None):
    """Adjoint of maxpool_fwd: channels [gout_coff, ...) of `g_out` gathered into `g_in` [B, Hin, Win, C]; `relu_gate`: the pooled
    tensor is a ReLU output, windows whose maximum is not positive pass nothing.  `c`: the channel count the caller means (ConvPlan's
    unpool fallback pools its plan's `cin_p`); `g_in` must be exactly that wide."""
    h16 = _acts('maxpool_bwd', g_out=g_out, g_in=g_in)
    if c is not None and c != g_in.shape[3]:
        raise ValueError(f'maxpool_bwd: `g_in` is {g_in.shape[3]} channels wide, the caller pools {c}')
    geo = _window('maxpool_bwd', g_in, 'g_in', g_out, 'g_out', k, s, p, gout_coff, MAX_K)
    ptrs = _lib.hptr(g_out), _bytes('maxpool_bwd', 'arg', arg, (geo[0], geo[4], geo[5], geo[3])), int(bool(relu_gate)), _lib.hptr(g_in)
    if _is_3s2(h16, k, s, p, geo):
        _lib.call('spaa_maxpool3s2_bwd', *ptrs, *geo[:6])
    else:
        _lib.call('spaa_maxpool_bwd_f16' if h16 else 'spaa_maxpool_bwd', *ptrs, *geo)


def avgpool2d_fwd(x, out, k, s, p, out_coff=0):
    """avg_pool2d(k, s, p), count_include_pad=True, into channels [out_coff, ...) of `out`."""
    h16 = _acts('avgpool2d_fwd', x=x, out=out)
    geo = _window('avgpool2d_fwd', x, 'x', out, 'out', k, s, p, out_coff, AVG_K)
    _lib.call('spaa_avgpool2d_fwd_f16' if h16 else 'spaa_avgpool2d_fwd', _lib.hptr(x), _lib.hptr(out), *geo)


def avgpool2d_bwd(g_out, g_in, k, s, p, gout_coff=0):
    h16 = _acts('avgpool2d_bwd', g_out=g_out, g_in=g_in)
    geo = _window('avgpool2d_bwd', g_in, 'g_in', g_out, 'g_out', k, s, p, gout_coff, AVG_K)
    _lib.call('spaa_avgpool2d_bwd_f16' if h16 else 'spaa_avgpool2d_bwd', _lib.hptr(g_out), _lib.hptr(g_in), *geo)


def _features(fn, name, t, b, c):
    """Pointer of the global pool's features / their gradient: fp32 whatever the storage type, B x C values."""
    if t.dtype != torch.float32 or t.shape[0] != b or t.shape[-1] != c or t.numel() != b * c:
        raise ValueError(f'{fn}: `{name}` must be fp32 [{b}, ..., {c}] with {b * c} elements (got {t.dtype} {tuple(t.shape)})')
    _lib.check_dev(t)
    return _lib.ptr(t)


def global_avgpool_fwd(x, feat):
    """adaptive_avg_pool2d(1): `x` [B, H, W, C] -> `feat` fp32 [B, 1, 1, C]."""
    h16 = _acts('global_avgpool_fwd', x=x)
    b, h, w, c = x.shape
    _lib.call('spaa_avgpool_fwd_f16' if h16 else 'spaa_avgpool_fwd', _lib.hptr(x), _features('global_avgpool_fwd', 'feat', feat, b, c),
              b, h * w, c)


def global_avgpool_bwd(g_feat, act, g_in):
    """`g_feat` fp32 [B, 1, 1, C] / (H W) broadcast into `g_in` [B, H, W, C], through the ReLU gate of `act` (None: no gate)."""
    h16 = _acts('global_avgpool_bwd', g_in=g_in, act=act)
    b, h, w, c = g_in.shape
    if act is not None:
        _shaped('global_avgpool_bwd', 'act', act, g_in.shape, g_in.dtype)
    _lib.call('spaa_avgpool_bwd_f16' if h16 else 'spaa_avgpool_bwd', _features('global_avgpool_bwd', 'g_feat', g_feat, b, c),
              _lib.hptr(act), _lib.hptr(g_in), b, h * w, c)


def _adaptive(fn, full, full_name, pooled, pooled_name, gate=None):
    if _acts(fn, **{full_name: full, pooled_name: pooled, 'gate_in': gate}):
        raise ValueError(f'{fn}: fp32 only (got {full.dtype})')
    b, hin, win, c = full.shape
    _, hout, wout, cp = pooled.shape
    if c % 4 or cp != c:
        raise ValueError(f'{fn}: `{full_name}` and `{pooled_name}` need the same channel count, a multiple of 4 (got {c}, {cp})')
    if gate is not None:
        _shaped(fn, 'gate_in', gate, full.shape, full.dtype)
    return b, hin, win, c, hout, wout


def adaptive_avgpool_fwd(x, out):
    """adaptive_avg_pool2d((Hout, Wout)), fp32: the output size is `out`'s."""
    geo = _adaptive('adaptive_avgpool_fwd', x, 'x', out, 'out')
    _lib.call('spaa_adaptive_avgpool_fwd', _lib.hptr(x), _lib.hptr(out), *geo)


def adaptive_avgpool_bwd(g_out, gate_in, g_in):
    """Its adjoint, through the ReLU gate of the pool's input `gate_in` (None: no gate)."""
    geo = _adaptive('adaptive_avgpool_bwd', g_in, 'g_in', g_out, 'g_out', gate_in)
    _lib.call('spaa_adaptive_avgpool_bwd', _lib.hptr(g_out), _lib.hptr(gate_in), _lib.hptr(g_in), *geo)


def gate_mask(act, mask, c, coff=0):
    """ReLU-gate bytes (the `mask_out` format of a convolution launch) of channels [coff, coff + c) of `act` [B, H, W, cstride] into
    `mask` uint8 [B, H, W, cstride / 4]: for activations no convolution wrote (max-pool outputs)."""
    h16 = _acts('gate_mask', act=act)
    b, h, w, cstride = act.shape
    _channels('gate_mask', 'act', c, cstride, coff)
    _lib.call('spaa_gate_mask', _lib.hptr(act), int(h16), _bytes('gate_mask', 'mask', mask, (b, h, w, cstride // 4)), b * h * w, c, cstride, coff)
