"""Float64 restatement of the attention-weighted attack, for the attention tests: the class-activation map of a feature
map and its gradient (`cam`), its bilinear resampling onto the classifier crop (`resample`, `camera_map`), the weighting of a gradient
image (`apply`), the rounding bounds the kernels are held to (`bound_c`, `tol_map`, `tol_image`), and the feature map and gradient of
the oracle's own classifier bodies by autograd at the input of adaptive_avg_pool2d (`body_features`).  A helper, not a test module."""
import contextlib

import numpy as np
import torch

import spaa_oracle as so

U = 2.0 ** -24


def center_crop_origin(h, w, size):
    """img_proc.py:126-132."""
    return int(round((h - size[0]) / 2.)), int(round((w - size[1]) / 2.))


def cam(A, G, seed):
    """A, G [B, h, w, C], seed [B] -> dict of float64 arrays: alpha [B, C] = sign(seed) mean_ij G, pre [B, h, w] = sum_k alpha A,
    c = max(0, pre), cmax [B], m [B, h, w] = c / cmax where cmax > 0 else 1, and S [B, h, w] = sum_k |alpha A| (the scale of the
    rounding bounds)."""
    A, G, seed = np.asarray(A, dtype=np.float64), np.asarray(G, dtype=np.float64), np.asarray(seed, dtype=np.float64)
    alpha = np.sign(seed)[:, None] * G.mean(axis=(1, 2))
    pre = (alpha[:, None, None, :] * A).sum(axis=3)
    S = np.abs(alpha[:, None, None, :] * A).sum(axis=3)
    c = np.maximum(pre, 0.0)
    cmax = c.max(axis=(1, 2))
    m = np.where(cmax[:, None, None] > 0, c / np.where(cmax > 0, cmax, 1.0)[:, None, None], 1.0)
    return dict(alpha=alpha, pre=pre, c=c, cmax=cmax, m=m, S=S)


def _taps(out, n):
    """Half-pixel centres, edge clamped: source cells i0, i1 and the weight of i1 for each of `out` output cells on `n` input cells."""
    src = np.maximum((np.arange(out) + 0.5) * (n / out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, src - i0


def resample(m, size):
    """m [B, h, w] -> [B, ch, cw]: F.interpolate(mode='bilinear', align_corners=False), written out."""
    m = np.asarray(m, dtype=np.float64)
    y0, y1, fy = _taps(size[0], m.shape[1])
    x0, x1, fx = _taps(size[1], m.shape[2])
    top = m[:, y0][:, :, x0] * (1 - fx) + m[:, y0][:, :, x1] * fx
    bot = m[:, y1][:, :, x0] * (1 - fx) + m[:, y1][:, :, x1] * fx
    return top * (1 - fy)[None, :, None] + bot * fy[None, :, None]


def camera_map(m, cam_hw, crop_sz):
    """M [B, H, W]: `m` resampled onto the crop, placed at the crop origin of the camera frame; 0 outside."""
    H, W = cam_hw
    cy0, cx0 = center_crop_origin(H, W, crop_sz)
    M = np.zeros((np.asarray(m).shape[0], H, W))
    M[:, cy0:cy0 + crop_sz[0], cx0:cx0 + crop_sz[1]] = resample(m, crop_sz)
    return M


def apply(g_y, M, floor, crop_sz):
    """g_y [B, H, W, 4] with its three colour channels multiplied by floor + (1 - floor) M inside the crop; the rest as it is."""
    g = np.array(g_y, dtype=np.float64)
    H, W = g.shape[1:3]
    cy0, cx0 = center_crop_origin(H, W, crop_sz)
    wgt = np.ones((g.shape[0], H, W))
    sl = (slice(None), slice(cy0, cy0 + crop_sz[0]), slice(cx0, cx0 + crop_sz[1]))
    wgt[sl] = floor + (1 - floor) * np.asarray(M, dtype=np.float64)[sl]
    g[..., :3] *= wgt[..., None]
    return g, wgt


def bound_c(ref, C):
    """|c - c_ref| <= 2 (C + h w) 2^-24 S: the worst case of an fp32 sum of C products whose alpha is an fp32 mean of h w values."""
    hw = ref['S'].shape[1] * ref['S'].shape[2]
    return 2.0 * (C + hw) * U * ref['S']


def tol_map(ref, bc):
    """[B]: what M may differ by, from the bound `bc` [B, h, w] on c: twice its largest value over the reference maximum (numerator and
    denominator both carry it), plus 4 * 2^-24 for the interpolation and the division.  A sample with m = 1 has no tolerance but that."""
    worst = bc.reshape(bc.shape[0], -1).max(axis=1)
    return np.where(ref['cmax'] > 0, 2.0 * worst / np.where(ref['cmax'] > 0, ref['cmax'], 1.0), 0.0) + 4 * U


def tol_image(g_y, wgt, floor, tm):
    """[B, H, W, 1]: what a weighted colour value may differ by: |g| (1 - floor) tol_map + 4 * 2^-24 |g W|."""
    g = np.abs(np.asarray(g_y, dtype=np.float64)[..., :3])
    return g * (1 - floor) * tm[:, None, None, None] + 4 * U * g * wgt[..., None]


@contextlib.contextmanager
def _pool_input(store):
    """For the duration of a forward pass of an oracle body: the input of adaptive_avg_pool2d becomes a leaf that `store` keeps."""
    orig = so.F.adaptive_avg_pool2d

    def pool(x, size):
        leaf = x.detach().requires_grad_(True)
        store.append(leaf)
        return orig(leaf, size)

    so.F.adaptive_avg_pool2d = pool
    try:
        yield
    finally:
        so.F.adaptive_avg_pool2d = orig


def body_features(oracle_classifier, im, g_logits, crop_sz, dtype=torch.float64):
    """The oracle body's logits [B, ncls], the feature map A [B, h, w, C] that enters adaptive_avg_pool2d and G = d sum(g_logits *
    logits) / dA, in `dtype` on the CPU, as float64 arrays.  `im` [B, 3, H, W], `g_logits` [B, ncls]."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        c = oracle_classifier
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in c.sd.items()}
        clf = so.OracleClassifier(c.name, sd, sort_results=c.sort_results, input_sz=c.input_sz)
        store = []
        with _pool_input(store):
            logits = clf(im.to(dtype), crop_sz)[0]
        feat = store[-1]          # (the last call is the body's: F.interpolate(mode='area') of the preprocessing pools the same way)
        G, = torch.autograd.grad((torch.as_tensor(np.asarray(g_logits), dtype=dtype) * logits).sum(), feat)
    finally:
        torch.set_default_dtype(old)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).numpy().astype(np.float64)   # noqa: E731
    return logits.detach().numpy().astype(np.float64), nhwc(feat), nhwc(G)


def seeds(g_logits, target):
    return np.asarray(g_logits, dtype=np.float64)[np.arange(len(target)), np.asarray(target)]
