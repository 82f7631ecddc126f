"""Float64 / integer restatements of the pose jitter, for the pose tests: the counter-based generator in Python
integers (`draw_word`, `draw_tables`), the source positions of a table row (`source`), the warp as torch's grid_sample in float64
(`warp_torch`, `forward`) with autograd's adjoint (`backward`), the adjoint kernel's 5 x 5 gather restated in numpy (`gather_adjoint`),
and one whole first iteration of the pose attack built from the oracle's PCNet, its classifier and the ensemble oracle's decision
(`first_iteration`).  A helper, not a test module."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import jitter_oracle as jo

M32 = 0xffffffff
FIRST = 0x85ebca6b                                  # the generator's first constant (the capture jitter's is 0x9e3779b9)
ROT, ZOOM, TX, TY, PX, PY = range(6)                # parameter indices of the generator
IDENTITY_ROW = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
LIMITS = (10.0, 0.15, 32.0, 0.1)                    # the largest rotate, zoom, shift, tilt of a PoseJitter
WINDOW = 2                                          # the adjoint kernel looks at the output pixels within 2 of round(H^-1 p)


def draw_word(seed, t, b, j, i):
    """The 32-bit word of (seed, iteration t, sample b, draw j, parameter index i)."""
    h = jo.mix32((seed & M32) ^ FIRST)
    for v in (t, b, j, i):
        h = jo.mix32(h ^ (v & M32))
    return h


def row_of(rotate, zoom, tx, ty, px, py, H, W):
    """The table row of an angle in degrees, a zoom s - 1, a translation and a tilt, for an H x W image."""
    a, s, R = rotate * np.pi / 180.0, 1.0 + zoom, max(H, W) / 2.0
    return np.array([s * np.cos(a), -s * np.sin(a), tx, s * np.sin(a), s * np.cos(a), ty, px / R, py / R])


def draw_tables(seed, t, B, J, rotate, zoom, shift, tilt, H, W, clean0):
    """table float64 [B][J][8] of iteration t.  The four ranges are taken as the float32 values the C entry point receives; the
    arithmetic is float64 (the kernel's differs by its fp32 roundings)."""
    rotate, zoom, shift, tilt = (float(np.float32(v)) for v in (rotate, zoom, shift, tilt))
    table = np.zeros((B, J, 8))
    for b in range(B):
        for j in range(J):
            if clean0 and j == 0:
                table[b, j] = IDENTITY_ROW
                continue
            s = [2.0 * jo.uniform(draw_word(seed, t, b, j, i)) - 1.0 for i in range(6)]
            table[b, j] = row_of(rotate * s[ROT], zoom * s[ZOOM], shift * s[TX], shift * s[TY], tilt * s[PX], tilt * s[PY], H, W)
    return table


def corner_rows(H, W, limits=LIMITS[:2] + (3.0,) + LIMITS[3:]):
    """The 16 sign corners of (rotate, zoom, tilt x, tilt y) at the limits, with a translation of `limits[2]` of alternating sign."""
    rot, zoom, shift, tilt = limits
    return np.stack([row_of(a * rot, z * zoom, a * z * shift, -a * shift, p * tilt, q * tilt, H, W)
                     for a, z, p, q in itertools.product((-1, 1), repeat=4)])


def random_rows(rng, n, H, W, limits=LIMITS):
    rot, zoom, shift, tilt = limits
    s = rng.uniform(-1, 1, (n, 6))
    return np.stack([row_of(rot * u[0], zoom * u[1], shift * u[2], shift * u[3], tilt * u[4], tilt * u[5], H, W) for u in s])


def source(row, H, W):
    """(xs, ys) float64 [H][W]: where output pixel (row, col) reads its source, in pixel indices."""
    h = [float(v) for v in row]
    u = np.arange(W)[None, :] + 0.5 - W / 2.0
    v = np.arange(H)[:, None] + 0.5 - H / 2.0
    w = h[6] * u + h[7] * v + 1.0
    return (h[0] * u + h[1] * v + h[2]) / w + (W / 2.0 - 0.5), (h[3] * u + h[4] * v + h[5]) / w + (H / 2.0 - 0.5)


def grid_of(rows, H, W):
    """grid_sample's grid [B][H][W][2] (float64, align_corners=False) of the table rows [B][8]."""
    g = np.zeros((len(rows), H, W, 2))
    for b, row in enumerate(rows):
        xs, ys = source(row, H, W)
        g[b, ..., 0] = (xs + 0.5) * 2.0 / W - 1.0
        g[b, ..., 1] = (ys + 0.5) * 2.0 / H - 1.0
    return torch.from_numpy(g)


def warp_torch(y, rows):
    """The warp of one draw for autograd: y [B,3,H,W] (double), rows [B][8] -> [B,3,H,W]."""
    B, _, H, W = y.shape
    return F.grid_sample(y, grid_of(rows, H, W).to(y.dtype), mode='bilinear', padding_mode='zeros', align_corners=False)


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)[..., :3].transpose(0, 3, 1, 2)))


def forward(y, table):
    """y [B][H][W][>= 3], table [B][J][8] -> out [J][B][H][W][4] float64, the pad channel 0."""
    yt = _nchw(y)
    B, _, H, W = yt.shape
    out = np.zeros((table.shape[1], B, H, W, 4))
    for j in range(table.shape[1]):
        out[j, ..., :3] = warp_torch(yt, table[:, j]).permute(0, 2, 3, 1).numpy()
    return out


def backward(g_out, table):
    """g_out [J][B][H][W][>= 3] -> g_y [J][B][H][W][4] float64: autograd's adjoint of the float64 warp, the pad channel 0."""
    J, B, H, W = np.asarray(g_out).shape[:4]
    out = np.zeros((J, B, H, W, 4))
    for j in range(J):
        y = torch.zeros(B, 3, H, W, dtype=torch.float64, requires_grad=True)
        g, = torch.autograd.grad((warp_torch(y, table[:, j]) * _nchw(g_out[j])).sum(), y)
        out[j, ..., :3] = g.permute(0, 2, 3, 1).numpy()
    return out


def bilinear(im, xs, ys):
    """The explicit form: im [H][W][C] sampled at (xs, ys) with taps outside the image contributing 0."""
    H, W = im.shape[:2]
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    fx, fy = xs - x0, ys - y0
    out = np.zeros(xs.shape + im.shape[2:])
    for dy, dx, w in ((0, 0, (1 - fy) * (1 - fx)), (0, 1, (1 - fy) * fx), (1, 0, fy * (1 - fx)), (1, 1, fy * fx)):
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        out += np.where(ok, w, 0.0)[..., None] * im[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
    return out


def inverse_centre(row, H, W):
    """(mc, mr) float64 [H][W]: H^-1 of every input pixel, in pixel indices of the output."""
    h = [float(v) for v in row]
    Hm = np.array([[h[0], h[1], h[2]], [h[3], h[4], h[5]], [h[6], h[7], 1.0]])
    inv = np.linalg.inv(Hm)
    us = np.arange(W)[None, :] + 0.5 - W / 2.0 + np.zeros((H, 1))
    vs = np.arange(H)[:, None] + 0.5 - H / 2.0 + np.zeros((1, W))
    m = np.einsum('ij,jhw->ihw', inv, np.stack([us, vs, np.ones_like(us)]))
    return m[0] / m[2] + (W / 2.0 - 0.5), m[1] / m[2] + (H / 2.0 - 0.5)


def gather_adjoint(g, row, window=WINDOW):
    """The adjoint kernel's gather restated: g [H][W][C] -> g_y [H][W][C].  Input pixel p = (r, q) sums, over the output pixels m
    within `window` of round(H^-1 p), g[m] times the forward weight of tap p at m (0 when p is none of m's four taps)."""
    H, W = g.shape[:2]
    xs, ys = source(row, H, W)
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    fx, fy = xs - x0, ys - y0
    mc, mr = inverse_centre(row, H, W)
    with np.errstate(invalid='ignore'):
        mc, mr = np.rint(mc), np.rint(mr)
    far = ~((mc >= -window) & (mc <= W - 1 + window) & (mr >= -window) & (mr <= H - 1 + window))
    mc, mr = np.where(far, -10 * window, mc).astype(np.int64), np.where(far, -10 * window, mr).astype(np.int64)
    r, q = np.mgrid[0:H, 0:W]
    out = np.zeros_like(g, dtype=np.float64)
    for di in range(-window, window + 1):
        for dk in range(-window, window + 1):
            mi, mk = mr + di, mc + dk
            ok = (mi >= 0) & (mi < H) & (mk >= 0) & (mk < W)
            mi, mk = np.clip(mi, 0, H - 1), np.clip(mk, 0, W - 1)
            dx, dy = q - x0[mi, mk], r - y0[mi, mk]
            ok &= (dx >= 0) & (dx <= 1) & (dy >= 0) & (dy <= 1)
            w = np.where(dx == 1, fx[mi, mk], 1 - fx[mi, mk]) * np.where(dy == 1, fy[mi, mk], 1 - fy[mi, mk])
            out += np.where(ok, w, 0.0)[..., None] * g[mi, mk]
    return out


def window_reach(row, H, W):
    """The largest |m - H^-1 p| per axis over the output pixels m and their taps p inside the image: below `WINDOW` + 0.5 the window
    around the rounded centre holds every contribution."""
    xs, ys = source(row, H, W)
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    mc, mr = inverse_centre(row, H, W)
    mi, mk = np.mgrid[0:H, 0:W]
    worst = 0.0
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        yy, xx = np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)
        d = np.maximum(np.abs(mc[yy, xx] - mk), np.abs(mr[yy, xx] - mi))
        if ok.any():
            worst = max(worst, float(d[ok].max()))
    return worst


def first_iteration(pcnet_sd, oracle_classifier, target, targeted, cam_scene, d_thr, setup_info, table, p_thresh=0.9, jit=None,
                    key=None, quantize=False):
    """The first iteration of the pose attack from the grey projector image, in float64 on the CPU, with the table [B][J][8] given
    (teacher-forced): y = PCNet(clamp(x), s); member j = the classifier behind draw j's warp (and, with `jit` / `key`, the capture
    jitter of jitter_oracle behind the warp), its logits and g_bj = d(-/+ logit_j[b, target_b]) / dy through the transform; then the
    ensemble oracle's decision (no focus) and combination.  Returns what ensemble_oracle.first_iteration returns."""
    import ensemble_oracle as eo
    import spaa_oracle as so
    B, J = len(target), table.shape[1]
    dtype = torch.float64
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        cast = lambda sd: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}   # noqa: E731
        c = oracle_classifier
        clf = so.OracleClassifier(c.name, cast(c.sd), sort_results=c.sort_results, input_sz=c.input_sz)
        scene = so.expand_4d(cam_scene.to(dtype)).expand(B, -1, -1, -1)
        x = torch.full((B, 3) + tuple(setup_info['prj_im_sz']), float(setup_info['prj_brightness']))
        with torch.no_grad():
            y = so.pcnet_forward(cast(pcnet_sd), x.clamp(0, 1), scene)
        y = y.detach().requires_grad_(True)
        sign = torch.tensor([-1.0 if t else 1.0 for t in targeted])
        idx = torch.arange(B)
        logits, gs = [], []
        for j in range(J):
            im = warp_torch(y, table[:, j])
            if jit is not None:
                im = jo.transform_torch(im, jit[:, j], key[:, j], quantize)
            raw = clf(im, setup_info['classifier_crop_sz'])[0]
            g, = torch.autograd.grad((sign * raw[idx, torch.as_tensor(list(target))]).sum(), y)
            logits.append(raw.detach().numpy().astype(np.float64))
            gs.append(g.permute(0, 2, 3, 1).reshape(B, -1, 3).numpy().astype(np.float64))
        caml2 = torch.norm(scene - y.detach(), dim=1).mean(1).mean(1).numpy().astype(np.float64)
    finally:
        torch.set_default_dtype(old)
    out = eo.decide_ens(logits, target, targeted, caml2, d_thr, p_thresh, False)
    top2 = [np.sort(lg, axis=1)[:, -2:] for lg in logits]
    out.update(cam=y.detach(), caml2=caml2, g=gs, g_adv=eo.combine(gs, out['ens_w']), logits=logits,
               gap=np.stack([t[:, 1] - t[:, 0] for t in top2], axis=1),
               p_margin=np.where(np.asarray(targeted, dtype=bool)[:, None], np.abs(out['p1'] - p_thresh), np.inf),
               d_margin=np.abs(caml2 * 255.0 - np.asarray(d_thr, dtype=np.float64)))
    return out


def eps_c(H, W):
    """The coordinate error of the kernels' fp32 evaluation order: at most 8 roundings at magnitude at most max(H, W)."""
    return 8 * 2.0 ** -24 * max(H, W)
