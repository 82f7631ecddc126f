"""The camera's JPEG round trip on device tensors: `jpeg_roundtrip` (spaa_jpeg_fwd on [N,3,H,W] images) and
`quant_tables` (the two quantisation tables of a quality, as the kernel builds them)."""
import numpy as np
import torch

from . import _lib
from .models import to_nhwc4, to_nchw
from .attack_options import JPEG_SUBSAMPLINGS, jpeg_quality_range

# ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural (row-major) order
_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def quant_tables(quality):
    """(luminance, chrominance) int64 [8][8] at `quality` in 1..100, natural order, scaled as libjpeg scales them:
    clamp((base s + 50) // 100, 1, 255) with s = 5000 // Q below 50 and 200 - 2 Q from 50 on."""
    q, _ = jpeg_quality_range(quality, 'quant_tables')
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(base, dtype=np.int64).reshape(8, 8) * s + 50) // 100, 1, 255) for base in (_LUMA, _CHROMA))


def jpeg_roundtrip(im, quality, subsampling='4:2:0'):
    """decode(encode(im)) of the images `im` [N,3,H,W] (a float GPU tensor, nominally in [0, 1]) at `quality`: one integer in 1..100,
    or one per image; returns [N,3,H,W] on the 8-bit grid.  One call of spaa_jpeg_fwd: the batch goes through as two draws of
    ceil(N / 2) samples (the entry point's smallest J), the halves of one tensor."""
    if not isinstance(im, torch.Tensor) or im.ndim != 4 or im.shape[1] != 3:
        raise ValueError(f'jpeg_roundtrip: im must be a [N,3,H,W] tensor, got {tuple(getattr(im, "shape", ()))}')
    if not im.is_cuda:
        raise RuntimeError(f'spaa_amd.jpeg_roundtrip runs on the GPU only (no CPU fallback); got a tensor on {im.device}')
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"jpeg_roundtrip: subsampling must be one of {', '.join(map(repr, JPEG_SUBSAMPLINGS))}, got {subsampling!r}")
    n, _, H, W = im.shape
    if n < 1:
        raise ValueError('jpeg_roundtrip: no images')
    qs = [quality] * n if np.ndim(quality) == 0 else list(np.asarray(quality).tolist())
    if len(qs) != n:
        raise ValueError(f'jpeg_roundtrip: {len(qs)} qualities for {n} images')
    qs = [jpeg_quality_range(int(q) if float(q) == int(q) else q, 'jpeg_roundtrip')[0] for q in qs]
    code, h = JPEG_SUBSAMPLINGS[subsampling], (n + 1) // 2
    with _lib.on_device(im.device):
        y4 = torch.zeros(2 * h, H, W, 4, device=im.device)
        y4[:n] = to_nhwc4(im.detach().float().contiguous())
        rows = torch.zeros(h, 2, 4)
        rows[:, :, 0] = torch.tensor(qs + [qs[-1]] * (2 * h - n), dtype=torch.float32).view(2, h).t()   # (row[b][j]: image j h + b)
        rows = rows.to(im.device)
        out = torch.zeros_like(y4)
        gate = torch.zeros(2 * h, H * W, dtype=torch.uint8, device=im.device)
        floats = _lib.load().spaa_jpeg_ws_floats(code, 2, h, H, W)
        ws = torch.zeros(floats, device=im.device) if floats else None
        halves = lambda t: [t[:h], t[h:]]   # noqa: E731
        _lib.call('spaa_jpeg_fwd', _lib.ptr_array(halves(y4)), _lib.ptr(rows), 2, code, _lib.ptr_array(halves(out)),
                  _lib.ptr_array(halves(gate)), _lib.ptr(ws), h, H, W)
        return to_nchw(out[:n])
