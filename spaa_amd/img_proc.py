"""Image helpers of the reference's img_proc.py that the training drivers need: `threshold_im` (the projector's direct-light mask
of a camera view, its convex region and its bounding-box corners) on HIP, and the small tensor helpers `expand_4d`, `center_crop`,
`resize`; `get_affine_transform` replaces cv.getAffineTransform.  OpenCV and scikit-image are not dependencies of this package.

`threshold_im` (img_proc.py:13-65, compensation=False) runs in libspaa_hip.so (csrc/direct_mask.hip):
  spaa_cb_direct_gray   clip to [0,1], grey byte image (and, from load_data, Nayar's separation in the same pass)
  spaa_mask_blur_hist   3 x 3 Gaussian (sigma 1.5) in integer arithmetic + 256-bin histogram
  spaa_otsu_mask_bbox   two-class Otsu threshold, mask, bounding box
The arithmetic rules are in DESIGN.md ("Direct-light mask arithmetic").  They restate the reference's call chain
(cv.cvtColor RGB2GRAY -> np.uint8(x * 255) -> cv.GaussianBlur(3 x 3, 1.5) -> skimage threshold_multiotsu(classes=2) -> np.digitize)
from the libraries' documented algorithms; neither library could be run against them.  Two points are NOT confirmed:
  * OpenCV's 8-bit GaussianBlur and its float cvtColor may round differently from the rules used here, by one grey level
    (io.torch_imread_mt carries the same caveat for its resize);
  * scikit-image is assumed to return the LAST value k of the lower class [vmin..k].  Here t is the first present value of the
    upper class and the mask is `smooth >= t`, i.e. exactly the upper class.  If the reference digitizes with k itself, pixels equal
    to k (one grey level at the class boundary) are foreground there and background here.
No CPU fallback: a non-GPU device raises."""
import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

BACKLIGHT = 0.9   # load_data's projector backlight strength b (train_network.py:75)


def _require_gpu(device):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError(f'spaa_amd.img_proc computes the direct-light mask on the GPU only (no CPU fallback); got device={dev}')
    return dev


def _corners(box, h, w):
    """img_proc.py:52-63: cv.boundingRect's (x, y, width, height) of the foreground as four corners, normalised to grid_sample's
    (-1, 1) coordinates."""
    x0, y0, x1, y1 = box
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    pts = [[x0, y0], [x0 + bw, y0], [x0 + bw, y0 + bh], [x0, y0 + bh]]
    return [[2 * (x / w) - 1, 2 * (y / h) - 1] for x, y in pts]


def direct_mask(cb, b=BACKLIGHT, *, device='cuda', want_images=False, timings=None):
    """The three launches on `cb` [N,3,H,W] float32 (N >= 2 checkerboard captures; N == 1: the direct image itself) or on a bool mask
    [H,W].  Returns dict(gray, smooth, hist, out, mask) of device tensors (+ direct / indirect [3,H,W] with `want_images`); out =
    int32 {t, xmin, ymin, xmax, ymax, count}.  `timings`: a list that receives (entry point, start event, end event)."""
    dev = _require_gpu(device)
    with _lib.on_device(dev):
        given_mask = cb.dtype == torch.bool
        if given_mask:
            if cb.ndim != 2:
                raise ValueError(f'a mask must be [H,W], got {tuple(cb.shape)}')
            h, w = cb.shape
        else:
            if cb.ndim != 4 or cb.shape[1] != 3:
                raise ValueError(f'expected [N,3,H,W] images, got {tuple(cb.shape)}')
            cb = cb.to(dev, torch.float32).contiguous()
            n, _, h, w = cb.shape
        if h < 2 or w < 2:
            raise ValueError(f'the image must be at least 2 x 2, got {h} x {w}')
        u8 = dict(dtype=torch.uint8, device=dev)
        res = dict(hist=torch.zeros(256, dtype=torch.int32, device=dev), out=torch.zeros(6, dtype=torch.int32, device=dev),
                   mask=torch.empty(h, w, **u8))
        p = _lib.ptr

        def launch(name, *args):
            if timings is None:
                return _lib.call(name, *args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.call(name, *args)
            e1.record()
            timings.append((name, e0, e1))

        if given_mask:
            # the mask as a two-valued byte image: any histogram with both values present puts t at 1
            res['smooth'] = cb.to(dev).to(torch.uint8).contiguous()
            res['hist'][:2] = 1
        else:
            res['gray'], res['smooth'] = torch.empty(h, w, **u8), torch.empty(h, w, **u8)
            if want_images:
                res['direct'] = torch.empty(3, h, w, device=dev)
                res['indirect'] = torch.empty(3, h, w, device=dev) if n > 1 else None
            launch('spaa_cb_direct_gray', p(cb), n, h, w, float(b), p(res['gray']), p(res.get('direct')), p(res.get('indirect')))
            launch('spaa_mask_blur_hist', p(res['gray']), h, w, p(res['smooth']), p(res['hist']))
        launch('spaa_otsu_mask_bbox', p(res['smooth']), p(res['hist']), h, w, p(res['mask']), p(res['out']))
        return res


def _convex_fill(mask):
    """The filled convex hull of the foreground pixels (cv.convexHull + cv.fillConvexPoly of img_proc.py:43-50), on the host: the
    hull of the pixel centres by Andrew's monotone chain, every pixel whose centre lies inside or on it."""
    h, w = mask.shape
    ys, xs = np.nonzero(mask)
    roi = np.zeros((h, w), dtype=bool)
    if len(xs) == 0:
        return roi
    # only each row's leftmost and rightmost foreground pixel can be a hull vertex
    rows = np.unique(ys)
    lo = np.full(h, w, dtype=np.int64)
    hi = np.full(h, -1, dtype=np.int64)
    np.minimum.at(lo, ys, xs)
    np.maximum.at(hi, ys, xs)
    pts = sorted({(int(lo[y]), int(y)) for y in rows} | {(int(hi[y]), int(y)) for y in rows})

    def half(points):
        out = []
        for q in points:
            while len(out) >= 2 and ((out[-1][0] - out[-2][0]) * (q[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (q[0] - out[-2][0])) <= 0:
                out.pop()
            out.append(q)
        return out

    hull = pts if len(pts) < 3 else half(pts)[:-1] + half(pts[::-1])[:-1]
    yy, xx = np.mgrid[0:h, 0:w]
    if len(hull) < 3:                                        # a point or a segment: the foreground's own extent along it
        (xa, ya), (xb, yb) = hull[0], hull[-1]
        on = (xb - xa) * (yy - ya) - (yb - ya) * (xx - xa) == 0
        return on & (xx >= min(xa, xb)) & (xx <= max(xa, xb)) & (yy >= min(ya, yb)) & (yy <= max(ya, yb))
    inside = np.ones((h, w), dtype=bool)
    for (xa, ya), (xb, yb) in zip(hull, hull[1:] + hull[:1]):   # counter-clockwise in (x, y): inside is on the left of every edge
        inside &= (xb - xa) * (yy - ya) - (yb - ya) * (xx - xa) >= 0
    return inside


def threshold_im(im_in, compensation=False, device='cuda'):
    """img_proc.py:13-65 with compensation=False (the only branch the reference uses): `im_in` an [H,W,3] float32 image (array or
    tensor; values outside [0,1] are clipped) or an [H,W] bool mask.  Returns (im_mask bool [H,W], im_roi bool [H,W], corners):
    the Otsu mask of the smoothed grey image, the filled convex hull of its foreground (host side) and the four corners of the
    foreground's bounding box in grid_sample coordinates.  ValueError when the image holds fewer than two distinct grey levels or
    the mask is empty.  See the module docstring for the two roundings of the reference's libraries that are not confirmed."""
    if compensation:
        raise NotImplementedError('threshold_im: only compensation=False (the SPAA direct-light mask) is implemented')
    dev = _require_gpu(device)
    x = im_in if isinstance(im_in, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im_in))
    if x.ndim == 3 and x.shape[-1] == 3:
        res = direct_mask(x.float().permute(2, 0, 1)[None], device=dev)
    elif x.ndim == 2 and x.dtype == torch.bool:
        res = direct_mask(x, device=dev)
    else:
        raise ValueError(f'threshold_im needs an [H,W,3] float image or an [H,W] bool mask, got {tuple(x.shape)} {x.dtype}')
    return _finish(res)


def _finish(res):
    out = res['out'].cpu().tolist()                           # (the one host sync)
    if out[0] < 0:
        raise ValueError('threshold_im: the smoothed image holds fewer than two distinct grey levels (no Otsu threshold)')
    if out[5] == 0:
        raise ValueError('threshold_im: the mask has no foreground pixel')
    im_mask = res['mask'].bool().cpu().numpy()
    h, w = im_mask.shape
    return im_mask, _convex_fill(im_mask), _corners(out[1:5], h, w)


def get_affine_transform(src, dst):
    """cv.getAffineTransform: the [2,3] matrix M with M [x, y, 1]^T = (x', y') for three point pairs, solved in float64."""
    src, dst = np.asarray(src, dtype=np.float64).reshape(3, 2), np.asarray(dst, dtype=np.float64).reshape(3, 2)
    a = np.concatenate([src, np.ones((3, 1))], axis=1)
    return np.linalg.solve(a, dst).T


# ------------------------------------------- tensor helpers (img_proc.py:110-132) -----------------------------------------------
def expand_4d(x):
    """A 1-D / 2-D / 3-D tensor as [B,C,H,W] (leading axes added)."""
    while x.ndim < 4:
        x = x[None]
    return x


def resize(x, size):
    """F.interpolate(mode='area') of a 2-D, 3-D or 4-D tensor to `size` = (h, w)."""
    if x.ndim not in (2, 3, 4):
        raise ValueError(f'resize: expected 2 to 4 dimensions, got {x.ndim}')
    lead = 4 - x.ndim
    return F.interpolate(expand_4d(x), size, mode='area')[(0,) * lead]


def center_crop(x, size):
    """The centred (th, tw) window of the last two axes."""
    th, tw = size
    i, j = int(round((x.shape[-2] - th) / 2.)), int(round((x.shape[-1] - tw) / 2.))
    return x[..., i:i + th, j:j + tw]
