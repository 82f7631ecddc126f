"""The camera's lens blur on device tensors: `gaussian_blur` (spaa_blur_rows + spaa_blur_fwd on [N,3,H,W] images)."""
import numpy as np
import torch

from . import _lib
from .models import to_nhwc4, to_nchw
from .attack_options import blur_sigma_range


def gaussian_blur(im, sigma):
    """The images `im` [N,3,H,W] (a float GPU tensor) through the separable Gaussian of `sigma` camera pixels with replicated border:
    one number in 0..2.5, or one per image; returns [N,3,H,W].  sigma = 0 returns the image bit for bit.  One call of spaa_blur_rows
    and one of spaa_blur_fwd: the batch goes through as two draws of ceil(N / 2) samples (the entry point's smallest J), the halves of
    one tensor."""
    if not isinstance(im, torch.Tensor) or im.ndim != 4 or im.shape[1] != 3:
        raise ValueError(f'gaussian_blur: im must be a [N,3,H,W] tensor, got {tuple(getattr(im, "shape", ()))}')
    if not im.is_cuda:
        raise RuntimeError(f'spaa_amd.gaussian_blur runs on the GPU only (no CPU fallback); got a tensor on {im.device}')
    n, _, H, W = im.shape
    if n < 1:
        raise ValueError('gaussian_blur: no images')
    sg = [sigma] * n if np.ndim(sigma) == 0 else list(np.asarray(sigma).tolist())
    if len(sg) != n:
        raise ValueError(f'gaussian_blur: {len(sg)} sigmas for {n} images')
    sg = [blur_sigma_range(float(s), 'gaussian_blur')[0] for s in sg]
    h = (n + 1) // 2
    with _lib.on_device(im.device):
        y4 = torch.zeros(2 * h, H, W, 4, device=im.device)
        y4[:n] = to_nhwc4(im.detach().float().contiguous())
        # (row[b][j]: image j h + b)
        sigmas = torch.tensor(sg + [sg[-1]] * (2 * h - n), dtype=torch.float32).view(2, h).t().contiguous().to(im.device)
        rows = torch.zeros(h, 2, 12, device=im.device)
        out = torch.zeros_like(y4)
        halves = lambda t: [t[:h], t[h:]]   # noqa: E731
        _lib.call('spaa_blur_rows', _lib.ptr(sigmas), _lib.ptr(rows), 2 * h)
        _lib.call('spaa_blur_fwd', _lib.ptr_array(halves(y4)), _lib.ptr(rows), 2, _lib.ptr_array(halves(out)), h, H, W)
        return to_nchw(out[:n])
