"""Float64 restatement of the WarpingNet kernels (csrc/warp.hip), for the warp tests: the sampling-grid build (`coarse_grid`,
`finish_grid`), bilinear grid_sample with align_corners=True and zero padding (`coords`, `sample`), its adjoint w.r.t. the image with
the clamp gate (`adjoint`), the prjl2 term and the squared norm that the fused adjoints fold in (`prjl2_and_sumsq`), the tap table and
its transposed (CSR) form (`taps`, `transposed`), the inputs the tests share (`affine_grid`, `dyadic_grid`, `image`, `masks`, `inputs`,
`CASES`, `grid_inputs`, `GRID_PARAMS`), the derived bars (`eps_c`, `bar_fwd`, `bar_bwd`, `eps_t`, `bar_grid`) and `MUTATIONS`: the same functions with one
deliberate mistake each, which tests/test_warp_cpu.py shows to move every result by more than its bar.  numpy on the CPU, written
from the operations' definitions (models.py:163-185 and pytorch_tps.py:54-106 of the reference; ATen's grid_sampler and linspace),
nothing from the kernels.  A helper, not a test module.

Layouts: images [B][H][W][>= 3] (the fourth lane is padding: never read here, written 0), grids [Hc][Wc][>= 2] (x, y in [-1, 1]),
masks [Hc][Wc].

The bars, with u = 2^-24 (the unit roundoff of fp32):

eps_c = 2 u max(Hp, Wp) max|g + 1| / 2.  A pixel coordinate is fl(fl(g + 1) * c), c = (W - 1) / 2 exact: two roundings, each at
most u relative, at magnitude at most (W - 1) |g + 1| / 2.  A contraction of the following `x - floor(x)` into an FMA drops the second
rounding and only lowers this.

bar_fwd = 2 eps_c D + 8 u V.  The bilinear interpolant with zero padding is continuous and piecewise bilinear; along either axis its
slope is at most D per pixel, D the largest difference of adjacent pixels of the (clamped) image with its zero border; both axes move
by at most eps_c.  At the exact coordinate the kernel's weights are products of two factors with at most one rounding each (1 - w),
the products v * w, the three additions and the mask multiply round once each: below 8 u times sum |v_i| w_i <= V = max |x|.

bar_bwd(s) = (2 eps_c + (n_s + 8) u) A_s.  Projector pixel s receives hat(x_c - s_x) hat(y_c - s_y) (g_c + g_xs s_c) m_c from every
camera pixel c; the hat is 1-Lipschitz and at most 1, so a weight moves by at most 2 eps_c, and only camera pixels whose exact
coordinate lies within 1 + eps_c of s on both axes can contribute in either evaluation: A_s sums their |g_c + g_xs s_c| m_c, n_s counts
them.  The roundings: g + g_xs s (2), the mask (1), the weight (3), the product (1) and the n_s - 1 additions.  Where the prjl2 term
applies, -scale (gray - x) / ||gray - x|| has a unit vector behind the scale: a subtraction, three products, two sums, a square root,
a division and two products, below 8 u scale.

eps_t and bar_grid: see `eps_t` and `bar_grid`."""
import functools

import numpy as np

U = 2.0 ** -24
SENTINEL = 0x7fffffff
TS = 16                                              # the tiled adjoint's projector tile


# ---------------------------------------------------------------------------------------------------------------- grid build
def linspace(start, end, steps, _bug=None):
    """torch.linspace as ATen computes it: from `start` in the lower half, from `end` in the upper half, so that
    linspace(-1, 1, n)[i] == -linspace(-1, 1, n)[n - 1 - i] exactly."""
    if steps == 1:
        return np.array([float(start)])
    i = np.arange(steps, dtype=np.float64)
    if _bug == 'linspace_not_symmetric':
        # (ATen's two evaluation orders differ by 1e-16 in float64, which no fp32 kernel can show; the mistake a test can see is a
        # linspace that is not symmetric about the midpoint at all: the end point left out)
        return start + (end - start) / steps * i
    step = (end - start) / (steps - 1)
    return np.where(i < steps // 2, start + step * i, end - step * (steps - 1 - i))


def tps_weights(theta, T, _bug=None):
    """(w [T][2], a [3][2]) of the reduced form: theta [T + 2][2] holds w_1 .. w_{T-1} and the three affine rows; w_0 = -sum(others)."""
    theta = np.asarray(theta, dtype=np.float64).reshape(T + 2, 2)
    free = theta[:T - 1]
    w0 = np.zeros((1, 2)) if _bug == 'tps_without_w0' else -free.sum(axis=0, keepdims=True)
    return np.concatenate([w0, free], axis=0), theta[T - 1:]


def tps_coords(theta, ctrl, T, out_size, _bug=None):
    """The TPS grid [Hout][Wout][2] in [-1, 1]: p + (1, p) a + sum_t U(|p - c_t|) w_t over [0, 1]^2, U = d^2 log(d + 1e-6)."""
    Hout, Wout = out_size
    ctrl = np.asarray(ctrl, dtype=np.float64).reshape(T, 2)
    w, a = tps_weights(theta, T, _bug)
    px = linspace(0.0, 1.0, Wout, _bug)[None, :] + np.zeros((Hout, 1))
    py = linspace(0.0, 1.0, Hout, _bug)[:, None] + np.zeros((1, Wout))
    d = np.sqrt((px[..., None] - ctrl[:, 0]) ** 2 + (py[..., None] - ctrl[:, 1]) ** 2)     # [Hout][Wout][T]
    u = d ** 2 * np.log(d + 1e-6)
    z = a[0] + px[..., None] * a[1] + py[..., None] * a[2] + u @ w
    return (np.stack([px, py], axis=-1) + z) * 2.0 - 1.0


def affine_field(aff, in_size, _bug=None):
    """F.affine_grid(aff, align_corners=True) [Hin][Win][2]."""
    Hin, Win = in_size
    A = np.asarray(aff, dtype=np.float64).reshape(2, 3)
    bx = linspace(-1.0, 1.0, Win, _bug)[None, :]
    by = linspace(-1.0, 1.0, Hin, _bug)[:, None]
    return np.stack([bx * A[0, 0] + by * A[0, 1] + A[0, 2], bx * A[1, 0] + by * A[1, 1] + A[1, 2]], axis=-1)


def coarse_grid(aff, theta, ctrl, T, in_size, out_size, _bug=None):
    """grid_sample(affine_grid(aff), tps_grid(theta, ctrl)) [Hout][Wout][2], not clamped: the analytic affine field sampled
    bilinearly with zero padding."""
    t = tps_coords(theta, ctrl, T, out_size, _bug)
    field = affine_field(aff, in_size, _bug)
    return _sample_channels(field[None], t)[0]


def finish_grid(coarse, refine=None, _bug=None):
    g = np.asarray(coarse, dtype=np.float64)[..., :2]
    if refine is not None:
        g = g + np.asarray(refine, dtype=np.float64)[..., :2]
    return g if _bug == 'grid_clamp_dropped' else np.clip(g, -1.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------- grid_sample
def coords(grid, Hp, Wp, _bug=None):
    """(xs, ys) float64 [Hc][Wc]: the pixel coordinates a grid addresses, align_corners=True."""
    g = np.asarray(grid, dtype=np.float64)
    if _bug == 'align_corners_false':
        return ((g[..., 0] + 1.0) * Wp - 1.0) / 2.0, ((g[..., 1] + 1.0) * Hp - 1.0) / 2.0
    return (g[..., 0] + 1.0) * (0.5 * (Wp - 1)), (g[..., 1] + 1.0) * (0.5 * (Hp - 1))


def _taps(xs, ys, _bug=None):
    """x0, y0 and the four (dy, dx, weight) in the order nw, ne, sw, se."""
    x0, y0 = np.floor(xs), np.floor(ys)
    fx, fy = xs - x0, ys - y0
    nw, ne, sw, se = (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy
    if _bug == 'ne_sw_swapped':
        ne, sw = sw, ne
    return x0.astype(np.int64), y0.astype(np.int64), ((0, 0, nw), (0, 1, ne), (1, 0, sw), (1, 1, se))


def _sample_channels(x, grid, _bug=None):
    """x [B][Hp][Wp][C] float64 at `grid` -> [B][Hc][Wc][C], zero padding."""
    B, Hp, Wp, _ = x.shape
    xs, ys = coords(grid, Hp, Wp, _bug)
    x0, y0, taps_ = _taps(xs, ys, _bug)
    out = np.zeros((B,) + xs.shape + (x.shape[-1],))
    for dy, dx, w in taps_:
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < Hp) & (xx >= 0) & (xx < Wp)
        if _bug == 'border_padding':
            ok = np.ones_like(ok)
        out += np.where(ok, w, 0.0)[None, ..., None] * x[:, np.clip(yy, 0, Hp - 1), np.clip(xx, 0, Wp - 1)]
    return out


def _mask_of(mask, _bug=None):
    m = np.asarray(mask, dtype=np.float64)
    if _bug == 'mask_wrong_pixel':
        m = np.roll(m.reshape(-1), -1).reshape(m.shape)          # mask[pix + 1]
    return m


def sample(x, grid, mask=None, clamp=False, _bug=None):
    """grid_sample(clamp(x, 0, 1) if clamp else x, grid, bilinear, zeros, align_corners=True) * mask -> [B][Hc][Wc][4], lane 3 = 0."""
    x = np.asarray(x, dtype=np.float64)[..., :3]
    if clamp:
        x = np.clip(x, 0.0, 1.0)
    out = np.zeros((x.shape[0],) + np.asarray(grid).shape[:2] + (4,))
    out[..., :3] = _sample_channels(x, grid, _bug)
    if mask is not None:
        out[..., :3] *= _mask_of(mask, _bug)[None, ..., None]
    return out


def effective_gradient(g, g_xs=None, s=None, mask=None, _bug=None):
    """(g + g_xs * s) * mask [B][Hc][Wc][3]: what the adjoint scatters."""
    ge = np.asarray(g, dtype=np.float64)[..., :3]
    if g_xs is not None:
        ge = ge + np.asarray(g_xs, dtype=np.float64)[..., :3] * np.asarray(s, dtype=np.float64)[..., :3]
    if mask is not None:
        ge = ge * _mask_of(mask, _bug)[None, ..., None]
    return ge


def adjoint(g, g_xs, s, x, grid, mask=None, clamp=False, _bug=None):
    """The adjoint of `sample` w.r.t. x at the cotangent g + g_xs * s (the second term: the gradient through x_warped * s):
    [B][Hp][Wp][4], lane 3 = 0.  With `clamp` the gradient passes where 0 <= x <= 1, equality included (ATen's clamp_backward)."""
    x = np.asarray(x, dtype=np.float64)[..., :3]
    B, Hp, Wp, _ = x.shape
    ge = effective_gradient(g, g_xs, s, mask, _bug).reshape(B, -1, 3)
    xs, ys = coords(grid, Hp, Wp, _bug)
    x0, y0, taps_ = _taps(xs, ys, _bug)
    acc = np.zeros((B, Hp * Wp, 3))
    for dy, dx, w in taps_:
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < Hp) & (xx >= 0) & (xx < Wp)
        if _bug == 'border_padding':
            ok = np.ones_like(ok)
        idx = (np.clip(yy, 0, Hp - 1) * Wp + np.clip(xx, 0, Wp - 1)).reshape(-1)
        np.add.at(acc, (slice(None), idx), ge * np.where(ok, w, 0.0).reshape(-1)[None, :, None])
    out = np.zeros((B, Hp, Wp, 4))
    out[..., :3] = acc.reshape(B, Hp, Wp, 3)
    if clamp:
        gate = (x > 0.0) & (x < 1.0) if _bug == 'gate_strict' else (x >= 0.0) & (x <= 1.0)
        out[..., :3] *= gate
    return out


def prjl2_and_sumsq(g_x, x, gray, scale, state):
    """spaa_grad_sumsq: g_x[b] += -scale_b (gray - x) / ||gray - x|| per pixel for the images with state[b][1] != 0 and scale_b != 0
    (zero where the norm is zero), then ss[b] = ||g_x[b]||^2.  `scale`: one number or one per image.  Returns (g_x, ss [B])."""
    out = np.array(g_x, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)[..., :3]
    B = out.shape[0]
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), (B,))
    state = None if state is None else np.asarray(state).reshape(B, -1)
    for b in range(B):
        if scale[b] != 0.0 and state is not None and state[b, 1] != 0:
            d = float(gray) - x[b]
            n = np.sqrt((d ** 2).sum(axis=-1, keepdims=True))
            out[b, ..., :3] += np.where(n != 0.0, -scale[b] * d / np.where(n != 0.0, n, 1.0), 0.0)
    return out, (out[..., :3] ** 2).reshape(B, -1).sum(axis=1)


# ---------------------------------------------------------------------------------------------------------------- tap tables
def taps(grid, Hp, Wp):
    """(src int32 [Hc*Wc][4], wgt float64 [Hc*Wc][4]) in the order nw, ne, sw, se: the projector pixel a tap reads and its weight;
    a tap outside the frame has src = 0x7fffffff and weight 0."""
    xs, ys = coords(grid, Hp, Wp)
    x0, y0, taps_ = _taps(xs, ys)
    src = np.full((xs.size, 4), SENTINEL, dtype=np.int64)
    wgt = np.zeros((xs.size, 4))
    for t, (dy, dx, w) in enumerate(taps_):
        yy, xx = (y0 + dy).reshape(-1), (x0 + dx).reshape(-1)
        ok = (yy >= 0) & (yy < Hp) & (xx >= 0) & (xx < Wp)
        src[ok, t] = (yy * Wp + xx)[ok]
        wgt[ok, t] = w.reshape(-1)[ok]
    return src.astype(np.int32), wgt


def transposed(src, wgt, mask, HWp):
    """The CSR form by projector pixel: (off int32 [HWp + 1], order int32 [4 Hc Wc], wm float32 [4 Hc Wc]): entries 4 campix + tap
    stably sorted by the pixel they read (the out-of-frame taps last, outside every list), weights times the camera pixel's mask."""
    flat = src.reshape(-1).astype(np.int64)
    order = np.argsort(flat, kind='stable')
    off = np.searchsorted(flat[order], np.arange(HWp + 1))
    wm = wgt if mask is None else wgt * np.asarray(mask, dtype=np.float64).reshape(-1, 1)
    return off.astype(np.int32), order.astype(np.int32), wm.reshape(-1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- shared inputs
# (camera size, projector size, grid kind, batch).  The forward-from-table kernel's workgroup counts 1, 10, 16, 20 and 30 (its XCD remap
# with fewer than 8, a multiple of 8 and other counts) are (5,7) B=1, (36,52) B=1, (64,64) B=1, (36,52) B=5 and (36,52) B=9; the batches
# 1, 3, 5, 6 and 9 leave 1, 3, 1, 2 and 1 images in the last group of four.
CASES = (((5, 7), (4, 6), 'b', 1), ((5, 7), (4, 6), 'd', 3),
         ((16, 17), (17, 33), 'a', 3), ((16, 17), (17, 33), 'c', 5), ((16, 17), (17, 33), 'b', 6),
         ((36, 52), (17, 33), 'a', 1), ((36, 52), (17, 33), 'c', 5), ((36, 52), (17, 33), 'd', 9),
         ((48, 40), (33, 33), 'a', 3), ((48, 40), (33, 33), 'b', 9),
         ((64, 64), (49, 33), 'c', 1), ((64, 64), (49, 33), 'b', 3), ((64, 64), (49, 33), 'd', 5))
SCALE = {'a': 0.9, 'b': 0.9, 'c': 1.3, 'd': 1.5}
GARBAGE = (float('nan'), 1e30)                       # what the lanes a kernel does not read hold
PLANTED = (0.0, -0.0, 1.0, float(np.nextafter(np.float32(0), np.float32(-1))), float(np.nextafter(np.float32(1), np.float32(2))))


def case_id(case):
    (hc, wc), (hp, wp), kind, b = case
    return f'{hc}x{wc}-{hp}x{wp}-{kind}-B{b}'


def affine_grid(cam, scale, clamp, rot=0.05, offset=(0.03, -0.02)):
    """float32 [Hc][Wc][4]: the camera frame rotated by `rot` rad, scaled and shifted, optionally clamped to [-1, 1]; lanes 2 and 3
    hold garbage (no kernel reads them)."""
    hc, wc = cam
    u, v = linspace(-1.0, 1.0, wc)[None, :], linspace(-1.0, 1.0, hc)[:, None]
    c, s = np.cos(rot), np.sin(rot)
    g = np.zeros((hc, wc, 4), dtype=np.float32)
    gx, gy = scale * (c * u - s * v) + offset[0], scale * (s * u + c * v) + offset[1]
    if clamp:
        gx, gy = np.clip(gx, -1.0, 1.0), np.clip(gy, -1.0, 1.0)
    g[..., 0], g[..., 1], g[..., 2], g[..., 3] = gx, gy, GARBAGE[0], GARBAGE[1]
    return g


def dyadic_grid(cam):
    """Grid (a): the 0.9 grid rounded to multiples of 2^-6.  On projector sizes 17 and 33, (W - 1) / 2 is 8 or 16, so every pixel
    coordinate, fraction and weight is exact in fp32.  The first pixels are planted: the four corners gx, gy = +-1, the centre, and
    integer pixel centres of both sizes."""
    g = affine_grid(cam, SCALE['a'], True)
    g[..., :2] = np.round(g[..., :2] * 64.0) / 64.0
    flat = g.reshape(-1, 4)
    for i, (gx, gy) in enumerate(((-1, -1), (1, 1), (-1, 1), (1, -1), (0, 0), (0.25, -0.5), (-0.875, 0.125), (1, 0.015625), (-0.5, -1))):
        flat[i, :2] = gx, gy
    return g


def make_grid(case):
    cam, _, kind, _ = case
    return dyadic_grid(cam) if kind == 'a' else affine_grid(cam, SCALE[kind], kind != 'd')


def image(B, Hp, Wp, seed, dyadic=False, plant=PLANTED):
    """float32 [B][Hp][Wp][4]: uniform in [-0.2, 1.2] (multiples of 2^-8 with `dyadic`), the values of `plant` in five middle columns
    of the middle row and, channel by channel, of the row above; garbage in lane 3."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.2, (B, Hp, Wp, 4)).astype(np.float32)
    if dyadic:
        x = (np.round(x * 256.0) / 256.0).astype(np.float32)
    r, c0 = Hp // 2, Wp // 2 - 2
    for k, v in enumerate(plant):
        x[:, r, c0 + k, :3] = v
        x[:, r - 1, c0 + k, k % 3] = v
    garbage(x)
    return x


def garbage(a):
    """Fills lane 3 of an NHWC4 array with what no kernel may read."""
    a[..., 3] = GARBAGE[0]
    a.reshape(-1, 4)[0, 3] = GARBAGE[1]
    return a


def masks(cam):
    """(rect, frac): a rectangle of ones whose 0 / 1 edge lies inside the projector's frame on every grid kind, and the same with quarters inside."""
    hc, wc = cam
    rect = np.zeros((hc, wc), dtype=np.float32)
    rect[hc // 4 + 1:hc - hc // 4, wc // 4 + 1:wc - wc // 4 - 1] = 1.0
    frac = rect * np.random.default_rng(hc * wc).choice(np.array([0.25, 0.5, 0.75, 1.0], dtype=np.float32), (hc, wc))
    return rect, frac.astype(np.float32)


DYADIC_PLANT = (0.0, -0.0, 1.0, 0.5, -0.125)         # (kind a: products and sums of the forward pass stay exact in fp32)
MASK_KINDS = ('none', 'rect', 'frac')


def inputs(case):
    """Everything the forward and adjoint tests of a case read, float32: grid [Hc][Wc][4], x [B][Hp][Wp][4] (dyadic for kind a),
    s in [0, 1], g and g_xs normal [B][Hc][Wc][4], the masks by MASK_KINDS name.  Lane 3 holds garbage everywhere."""
    (hc, wc), (hp, wp), kind, B = case
    rng = np.random.default_rng(hc * 1000 + wc + B)
    rect, frac = masks((hc, wc))
    return dict(grid=make_grid(case),
                x=image(B, hp, wp, hp * wp + B, dyadic=kind == 'a', plant=DYADIC_PLANT if kind == 'a' else PLANTED),
                s=garbage(rng.uniform(0, 1, (B, hc, wc, 4)).astype(np.float32)),
                g=garbage(rng.standard_normal((B, hc, wc, 4)).astype(np.float32)),
                g_xs=garbage(rng.standard_normal((B, hc, wc, 4)).astype(np.float32)),
                mask=dict(none=None, rect=rect, frac=frac))


def uniform_ctrl(n):
    """n x n control points on [0, 1]^2, x fastest."""
    l = linspace(0.0, 1.0, n)
    return np.stack([np.tile(l, n), np.repeat(l, n)], axis=1)


# (name, affine, theta scale): identity and zero theta; rotated and scaled with theta of the synthetic state dict's magnitude; scale 1.3
GRID_PARAMS = (('identity', (1, 0, 0, 0, 1, 0), 0.0), ('rot0.9', (0.9, 0.02, 0.05, -0.03, 0.9, 0.05), 1e-3),
               ('scale1.3', (1.3, 0.05, 0.02, -0.04, 1.3, -0.03), 1e-3))
GRID_SIZES = (((16, 17), (12, 21)), ((36, 52), (17, 33)))            # (out = camera, in = projector): in != out
GRID_T = (1, 2, 36)


def grid_inputs(name, T, out_size):
    """float32 (aff [6], theta [T + 2][2], ctrl [T][2], refine [Hout][Wout][4]) of a GRID_PARAMS row: theta as
    spaa_amd.synthetic.pcnet_state_dict draws it (scale * (1 + N(0, 0.25))), control points uniform (T = 36), the two ends of the
    diagonal (T = 2) or the centre (T = 1); the refine plane is small except a planted block that pushes values across +-1."""
    _, aff, tscale = next(p for p in GRID_PARAMS if p[0] == name)
    rng = np.random.default_rng(T + out_size[0])
    theta = (tscale * (1.0 + 0.5 * rng.standard_normal((T + 2, 2)))).astype(np.float32)
    ctrl = {1: np.array([[0.5, 0.5]]), 2: np.array([[0.0, 0.0], [1.0, 1.0]]), 36: uniform_ctrl(6)}[T].astype(np.float32)
    refine = np.zeros(out_size + (4,), dtype=np.float32)
    refine[..., :2] = 1e-3 * rng.standard_normal(out_size + (2,))
    refine[:3, :, 0] = -2.5
    refine[:, -3:, 1] = 2.5
    refine[-2:, :2, :2] = (2.5, -2.5)
    refine[..., 2], refine[..., 3] = GARBAGE
    return np.asarray(aff, dtype=np.float32), theta, ctrl, refine


# ---------------------------------------------------------------------------------------------------------------- bars
def eps_c(grid, Hp, Wp):
    g = np.asarray(grid, dtype=np.float64)[..., :2]
    return 2 * U * max(Hp, Wp) * np.abs(g + 1.0).max() / 2.0


def bar_fwd(x, grid, clamp):
    x = np.asarray(x, dtype=np.float64)[..., :3]
    if clamp:
        x = np.clip(x, 0.0, 1.0)
    Hp, Wp = x.shape[1:3]
    p = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    D = max(np.abs(np.diff(p, axis=1)).max(), np.abs(np.diff(p, axis=2)).max())
    return 2 * eps_c(grid, Hp, Wp) * D + 8 * U * np.abs(x).max()


def reach(g, g_xs, s, mask, grid, Hp, Wp):
    """(A [B][Hp][Wp][3], n [Hp][Wp]): per projector pixel s, the sum of |g_c + g_xs s_c| m_c and the count of the camera pixels
    whose float64 coordinate lies within 1 + eps_c of s on both axes."""
    ge = np.abs(effective_gradient(g, g_xs, s, mask))
    B = ge.shape[0]
    ge = ge.reshape(B, -1, 3)
    e = eps_c(grid, Hp, Wp)
    xs, ys = coords(grid, Hp, Wp)
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    A, n = np.zeros((B, Hp * Wp, 3)), np.zeros(Hp * Wp)
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            sx, sy = np.floor(xs) + dx, np.floor(ys) + dy
            ok = (np.abs(xs - sx) <= 1 + e) & (np.abs(ys - sy) <= 1 + e) & (sx >= 0) & (sx < Wp) & (sy >= 0) & (sy < Hp)
            idx = (sy * Wp + sx).astype(np.int64)[ok]
            np.add.at(A, (slice(None), idx), ge[:, ok])
            np.add.at(n, idx, 1.0)
    return A.reshape(B, Hp, Wp, 3), n.reshape(Hp, Wp)


def bar_bwd(g, g_xs, s, mask, grid, Hp, Wp):
    """[B][Hp][Wp][3]; 0 where no camera pixel can reach s: such a pixel's gradient is exactly 0."""
    A, n = reach(g, g_xs, s, mask, grid, Hp, Wp)
    return (2 * eps_c(grid, Hp, Wp) + (n[None, ..., None] + 8) * U) * A


def eps_t(theta, ctrl, T, out_size):
    """The error of a TPS coordinate in [-1, 1] units, [Hout][Wout], from the fp32 evaluation t = (p + z) 2 - 1,
    z = a_0 + p_x a_1 + p_y a_2 + sum_t U_t w_t, U_t = d_t^2 log(d_t + 1e-6):
      - p: linspace, two roundings at magnitude <= 1: 2 u.  It moves d_t by at most 2 sqrt(2) u, and U by |dU/dd| = |2 d log d + d| <=
        2.4 on d <= sqrt(2): below 8 u per unit of |w_t|: 8 u W1, W1 = sum_t |w_t|.
      - U_t: d is a square root of a sum of two squares (relative 2.5 u), d^2 one more product (relative 6 u together); the argument of
        the logarithm inherits 2.5 u relative plus a rounding, an absolute 3.5 u of the logarithm, i.e. 3.5 u d^2 of U; logf is good to
        4 ulp = 8 u relative; the product rounds once: |dU_t| <= 15 u |U_t| + 3.5 u d_t^2.
      - the sum: products U_t w_t round once, the T additions at most T u of the running magnitude; w_0 = -(w_1 + ...) carries
        (T - 1) u W1: together (T + 16) u S + 3.5 u Q + (T - 1) u |U_0| W1, S = sum |U_t| |w_t|, Q = sum d_t^2 |w_t|.
      - the affine part: two products and three additions at magnitude M = |a_0| + |a_1| + |a_2|, p's 2 u: 6 u M.
      - p + z, the doubling (exact) and the - 1: u (1 + |z|) + u |t|, and p's 2 u.
    All of it doubles with the final (p + z) 2."""
    Hout, Wout = out_size
    ctrl = np.asarray(ctrl, dtype=np.float64).reshape(T, 2)
    w, a = tps_weights(theta, T)
    px = linspace(0.0, 1.0, Wout)[None, :] + np.zeros((Hout, 1))
    py = linspace(0.0, 1.0, Hout)[:, None] + np.zeros((1, Wout))
    d = np.sqrt((px[..., None] - ctrl[:, 0]) ** 2 + (py[..., None] - ctrl[:, 1]) ** 2)
    u = np.abs(d ** 2 * np.log(d + 1e-6))
    t = np.abs(tps_coords(theta, ctrl, T, out_size))
    out = np.zeros((Hout, Wout))
    for k in range(2):
        aw = np.abs(w[:, k])
        W1, S, Q = aw.sum(), u @ aw, (d ** 2) @ aw
        M = np.abs(a[:, k]).sum()
        z = M + S
        e = (T + 16) * U * S + 3.5 * U * Q + (T - 1) * U * u[..., 0] * W1 + 8 * U * W1 + 6 * U * M + U * (1 + z) + 2 * U
        out = np.maximum(out, 2 * e + U * t[..., k])
    return out


def bar_grid(aff, theta, ctrl, T, in_size, out_size):
    """[Hout][Wout][2]: the bar of the coarse grid.  The sampled field is the bilinear interpolant of the affine field a(b) = A (b, 1)
    on the input lattice with zeros outside: inside the frame it reproduces a(.) and moves by |A_k0| + |A_k1| per unit of the two
    coordinates; within one input pixel of the frame's edge (and beyond) it fades to zero over one pixel, 2 / (W - 1) units: at most
    F_k (Win - 1) / 2 and F_k (Hin - 1) / 2 more per unit, F_k = |A_k0| + |A_k1| + |A_k2| >= max |field_k|.  The sampling coordinate is off by
    eps_t from the TPS evaluation plus, in pixels, the eps_c of the unnormalisation.  Roundings of the field's own evaluation (linspace
    2 u, two products, two additions: 6 u F_k) and of the four weights and sums (8 u F_k) are added."""
    Hin, Win = in_size
    A = np.abs(np.asarray(aff, dtype=np.float64).reshape(2, 3))
    t = tps_coords(theta, ctrl, T, out_size)
    et = eps_t(theta, ctrl, T, out_size)
    ec = 2 * U * max(Hin, Win) * np.abs(t + 1.0).max() / 2.0          # pixels
    xs, ys = coords(t, Hin, Win)
    m = 1.0 + ec
    fade = (xs < m) | (xs > Win - 1 - m) | (ys < m) | (ys > Hin - 1 - m)
    out = np.zeros(tuple(out_size) + (2,))
    for k in range(2):
        F = A[k].sum()
        Lx = A[k, 0] + np.where(fade, F * (Win - 1) / 2.0, 0.0)
        Ly = A[k, 1] + np.where(fade, F * (Hin - 1) / 2.0, 0.0)
        out[..., k] = Lx * (et + ec * 2.0 / (Win - 1)) + Ly * (et + ec * 2.0 / (Hin - 1)) + 14 * U * F
    return out


# ---------------------------------------------------------------------------------------------------------------- mutations
def _mutants(name, *fns):
    return {f.__name__: functools.partial(f, _bug=name) for f in fns}


# name -> {function name: the function with that mistake}
MUTATIONS = {
    'align_corners_false': _mutants('align_corners_false', sample, adjoint),
    'ne_sw_swapped': _mutants('ne_sw_swapped', sample, adjoint),
    'gate_strict': _mutants('gate_strict', adjoint),
    'mask_wrong_pixel': _mutants('mask_wrong_pixel', sample, adjoint),
    'border_padding': _mutants('border_padding', sample, adjoint),
    'tps_without_w0': _mutants('tps_without_w0', coarse_grid),
    'linspace_not_symmetric': _mutants('linspace_not_symmetric', coarse_grid),
    'grid_clamp_dropped': _mutants('grid_clamp_dropped', finish_grid),
}
