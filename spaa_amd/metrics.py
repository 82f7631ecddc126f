"""Image-distance metrics of the reference's evaluation step on the GPU (HIP kernels, no CPU fallback).

Mirrors /root/reference/src/python/utils.py:420-491 — `calc_img_dists(x, y)` returns
(PSNR, RMSE, SSIM, mean-L2 * 255, mean-L_inf * 255, mean dE2000) as Python floats — and the single metrics
`psnr`, `rmse`, `ssim` (pytorch_ssim/__init__.py:98-107), `l2_norm`, `linf_norm`, `deltaE`
(perc_al/differential_color_functions.py:183-190).  x, y: [3,H,W] or [B,3,H,W] float tensors in [0,1] on any device
(moved to the GPU as the reference does).

Every metric is a ratio of sums that add over images (mse = sum d^2 / 3N, SSIM = sum map / 3N, L2 = sum ||d|| / N,
L_inf = sum max|d| / N, dE = sum dE / N over the N pixels of a group), so one launch (`spaa_img_stats`) returns the five
sums of each image pair over its crop rectangle, and any group of pairs is formed from them on the host in float64
(`dists_from_sums`).  `calc_img_dists` is the group "the whole batch"; the attack summary
(attack_summary.summarize_single_attacker) forms all groups of a setup from one `img_stats` call.
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib

TILE = 16            # spaa_img_stats: one block per 16 x 16 crop pixels
_INT32_MAX = 2 ** 31 - 1

# One image pair of img_stats: side x is the [3, xH, xW] image at element offset x_off of the flat x buffer, cropped to
# rows [xy0, xy0 + h) x columns [xx0, xx0 + w); side y likewise, or, when `rgb` is not None, the constant colour `rgb`.
Pair = namedtuple('Pair', 'x_off xH xW xy0 xx0 y_off yH yW yy0 yx0 h w rgb')


def _window(window_size=11, sigma=1.5):
    """pytorch_ssim/__init__.py:9-21: normalised 1-D Gaussian, outer product, float32."""
    g = torch.Tensor([math.exp(-(i - window_size // 2) ** 2 / float(2 * sigma ** 2)) for i in range(window_size)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().reshape(-1).contiguous()


def ssim_taps(window_size=11, sigma=1.5):
    """pytorch_ssim/__init__.py:9-12 (gaussian): the normalised 1-D Gaussian in float32, whose outer product `_window` is."""
    g = torch.Tensor([math.exp(-(i - window_size // 2) ** 2 / float(2 * sigma ** 2)) for i in range(window_size)])
    return g / g.sum()


def center_crop_origin(h, w, size):
    """img_proc.py:126-132 (center_crop): the crop's top-left corner (Python's round, as the reference)."""
    th, tw = size
    return int(round((h - th) / 2.)), int(round((w - tw) / 2.))


def stack_pairs(nx, x_hw, y_hw=None, crop=None, x_off=0, y_off=0, y_step=None, rgb=None):
    """Pairs of `nx` consecutive [3, *x_hw] images starting at x_off against y images starting at y_off (the next one y_step
    elements further on: 0 = one y image for all, the default = one per x image) or against the constant colour `rgb`;
    both sides centre-cropped to `crop` (h, w) as img_proc.center_crop does (None: the whole image, then y_hw == x_hw)."""
    xh, xw = x_hw
    yh, yw = (xh, xw) if y_hw is None else y_hw
    h, w = (xh, xw) if crop is None else crop
    xy0, xx0 = center_crop_origin(xh, xw, (h, w))
    if rgb is not None:
        yh, yw, yy0, yx0 = h, w, 0, 0
        rgb = tuple(float(c) for c in rgb)
    else:
        if crop is None and (yh, yw) != (xh, xw):
            raise ValueError(f'uncropped pairs need images of the same size, got {x_hw} and {y_hw}')
        yy0, yx0 = center_crop_origin(yh, yw, (h, w))
    ystep = 3 * yh * yw if y_step is None else y_step
    return [Pair(x_off + i * 3 * xh * xw, xh, xw, xy0, xx0, None if rgb is not None else y_off + i * ystep, yh, yw, yy0, yx0,
                 h, w, rgb) for i in range(nx)]


def _flat(t, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous().reshape(-1)


def _check_pairs(pairs, nx, ny):
    """ValueError for a crop outside its image, a side outside its buffer, or offsets / planes beyond the kernel's index width."""
    for k, p in enumerate(pairs):
        if p.h < 1 or p.w < 1:
            raise ValueError(f'pair {k}: empty crop {p.h}x{p.w}')
        sides = [('x', p.x_off, p.xH, p.xW, p.xy0, p.xx0, nx)]
        if p.rgb is None:
            sides.append(('y', p.y_off, p.yH, p.yW, p.yy0, p.yx0, ny))
        elif len(p.rgb) != 3:
            raise ValueError(f'pair {k}: a constant colour needs 3 components, got {p.rgb}')
        for side, off, hh, ww, y0, x0, n in sides:
            if y0 < 0 or x0 < 0 or y0 + p.h > hh or x0 + p.w > ww:
                raise ValueError(f'pair {k}: {side} crop {p.h}x{p.w} at ({y0}, {x0}) lies outside its {hh}x{ww} image')
            if 3 * hh * ww > _INT32_MAX:
                raise ValueError(f'pair {k}: a {hh}x{ww} {side} image exceeds the kernel\'s 32-bit plane index')
            if off < 0 or off + 3 * hh * ww > n:
                raise ValueError(f'pair {k}: {side} image at element offset {off} ({3 * hh * ww} elements) overruns its '
                                 f'buffer of {n} elements')


def img_stats(x, y, pairs):
    """One spaa_img_stats launch over `pairs` (a list of Pair): returns (sums float64 [P, 5], npix int64 [P]), the columns of
    `sums` being (sum d^2 over 3 channels, sum SSIM map over 3 channels, sum ||d||_2, sum max|d|, sum dE2000) over each pair's
    crop and npix = h * w.  x, y: tensors of any shape read as flat fp32 buffers (y may be None when every pair has a constant
    colour); they are moved to the GPU of x (or of y, or the current one).  Tile partials are added in fixed order in float64:
    repeated calls are bit-identical."""
    if not torch.cuda.is_available():
        raise RuntimeError('spaa_amd.metrics needs the GPU (no CPU fallback)')
    pairs = list(pairs)
    if not pairs:
        return np.zeros((0, 5)), np.zeros(0, dtype=np.int64)
    dev = x.device if x.is_cuda else (y.device if y is not None and y.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    with _lib.on_device(dev):
        xf = _flat(x, dev)
        yf = _flat(y, dev) if y is not None else None
        if yf is None and any(p.rgb is None for p in pairs):
            raise ValueError('img_stats: y is None but a pair reads it')
        _check_pairs(pairs, xf.numel(), 0 if yf is None else yf.numel())
        table = (_lib.ImgPair * len(pairs))()
        counts = np.array([-(-p.h // TILE) * -(-p.w // TILE) for p in pairs], dtype=np.int64)
        starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
        ntiles = int(counts.sum())
        if ntiles > _INT32_MAX:
            raise ValueError(f'img_stats: {ntiles} tiles exceed the kernel\'s 32-bit tile index')
        for k, p in enumerate(pairs):
            e = table[k]
            e.x_off, e.xH, e.xW, e.xy0, e.xx0 = p.x_off, p.xH, p.xW, p.xy0, p.xx0
            e.h, e.w, e.tile0 = p.h, p.w, int(starts[k])
            if p.rgb is None:
                e.y_off, e.yH, e.yW, e.yy0, e.yx0, e.y_const = p.y_off, p.yH, p.yW, p.yy0, p.yx0, 0
            else:
                e.y_const = 1
                e.y_rgb[:] = p.rgb
        pairs_d = torch.frombuffer(bytearray(table), dtype=torch.uint8).to(dev)
        tile_pair = torch.from_numpy(np.repeat(np.arange(len(pairs), dtype=np.int32), counts)).to(dev)
        partial = torch.empty(ntiles, 5, device=dev)
        win = _window().to(dev)
        _lib.call('spaa_img_stats', _lib.ptr(xf), _lib.ptr(yf), _lib.ptr(pairs_d), _lib.ptr(tile_pair), ntiles, _lib.ptr(win),
                  _lib.ptr(partial))
        part = partial.cpu().double().numpy()
    sums = np.add.reduceat(part, starts, axis=0)
    return sums, np.array([p.h * p.w for p in pairs], dtype=np.int64)


def dists_from_sums(sums, npix, idx=None):
    """calc_img_dists (utils.py:420-423) of the group of pairs `idx` (all when None) from img_stats' per-pair sums, in float64:
    (PSNR, RMSE, SSIM, mean L2 * 255, mean L_inf * 255, mean dE2000).  Host code only."""
    sums, npix = np.asarray(sums, dtype=np.float64), np.asarray(npix, dtype=np.float64)
    if idx is not None:
        sums, npix = sums[idx], npix[idx]
    sq, sm, l2, li, de = np.atleast_2d(sums).sum(0).tolist()
    n = float(np.sum(npix))
    if n <= 0:
        raise ValueError('dists_from_sums: empty group')
    mse = sq / (3 * n)
    return (10 * math.log10(1 / mse) if mse > 0 else math.inf, math.sqrt(mse * 3), sm / (3 * n), l2 / n * 255, li / n * 255,
            de / n)


def _sums(x, y):
    if not torch.cuda.is_available():
        raise RuntimeError('spaa_amd.metrics needs the GPU (no CPU fallback)')
    x, y = (t if t.ndim == 4 else t[None] for t in (x, y))
    if x.shape != y.shape or x.shape[1] != 3:
        raise ValueError(f'expected two [B,3,H,W] / [3,H,W] images of the same shape, got {tuple(x.shape)} {tuple(y.shape)}')
    return img_stats(x, y, stack_pairs(x.shape[0], tuple(x.shape[2:])))


def calc_img_dists(x, y):
    """utils.py:420-423."""
    return dists_from_sums(*_sums(x, y))


def psnr(x, y):
    return calc_img_dists(x, y)[0]


def rmse(x, y):
    return calc_img_dists(x, y)[1]


def ssim(x, y):
    return calc_img_dists(x, y)[2]


def l2_norm(x, y):
    return calc_img_dists(x, y)[3]


def linf_norm(x, y):
    return calc_img_dists(x, y)[4]


def deltaE(x, y):
    return calc_img_dists(x, y)[5]
