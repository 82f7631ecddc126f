"""Float64 restatement of the SSIM stealth term (csrc/ssim_ops.hip), for the SSIM tests: the per-sample SSIM of
pytorch_ssim._ssim(size_average=False) (`ssim`, `ssim_map`), the gradient of 1 - SSIM written out (`grad`, `grad_sum`), the window
statistics (`stats`), the inputs the tests share (`SIZES`, `KINDS`, `inputs`), the derived bars (`bars`) and `MUTATIONS`: the same
functions with one deliberate mistake each, which tests/test_ssim_cpu.py shows to move the results by more than their bars.  numpy on
the CPU, written from the definition (pytorch_ssim/__init__.py:9-66 of the reference), nothing from the kernels.  A helper, not a test
module.

Layouts: images [H][W][>= 3] float (one sample; the fourth lane is padding: never read here).  The window is the EXACT outer product
of the fp32-rounded 1-D taps (`taps`): "replicate-pad by 5, then filter" along an axis of length n is the n x n matrix F_n
(`filter_matrix`), F_n[p][q] = sum of w[k] over the k with clamp(p + k - 5) = q, a statistic is F_H X F_W^T and the adjoint of the
filter F_H^T M F_W.

The bars, with u = 2^-24 (the unit roundoff of fp32), are RUNNING ERROR BOUNDS: `bars` walks through the kernels' own sequence of
operations in float64 and carries, next to every value, a bound on what fp32 can have done to it so far:
  * a sum, product or quotient of (a, ea) and (b, eb): the first-order propagated error (ea + eb; |a| eb + |b| ea + ea eb;
    (ea + |a / b| eb) / (|b| - eb)) plus one rounding u |result|.  A contraction into an FMA drops a rounding and only lowers this.
  * a filter pass of 11 fused multiply-adds: a term passes through at most 11 roundings, so the pass adds ((1 + u)^11 - 1) F|x| to the
    filtered input error F e_x; rows then columns: gamma_f = (1 + 11 u)^2 - 1 on F|x|.  The squares and products y^2, y s, s^2 carry
    their one rounding into the filter.  With operand magnitudes up to 1 (images in [0, 1]) a plain second moment's bound is about
    1.3e-6, and the variance e11 - mu1^2 of a flat bright patch inherits it in full while its value is 0: against C2 = 9e-4 that is
    1.5e-3 relative in B2 and A2.  The kernels therefore accumulate the moments about a constant c per tile and channel (the scene's
    value at the tile's first pixel) and the walk follows them: y - c and scene - c (one rounding each), the shifted
    moments, the terms in 1 - Wt that make the shift exact for taps whose sum is not exactly 1, the means shifted back.  The
    operands of the moments are then differences from c, near 0 in a flat patch, and the bound shrinks with them; on texture the
    bound stays pixel by pixel what the magnitudes give.
  * the adjoint's passes: an edge pixel collects up to 6 x 11 taps per axis, so gamma_a = (1 + 66 u)^2 - 1 on F^T|m| (an upper bound
    for every pixel), then the three products and two sums of m_mu + 2 y m_11 + s m_12, the scale and the accumulation.
  * the value: a tile's sum passes through at most 6 + 6 + 3 additions per term (two pixels x three channels per thread, the wave's
    shuffle tree, the four waves), the sum over tiles is in double and rounded once.
Against the reference's own fp32 evaluation (the golden fixture) the same walk is used with the constants of ITS arithmetic
(`REF`): the 2-D window is fl(w_i w_j) (one rounding per weight) and conv2d adds 121 terms in an order that is not specified, at most
121 roundings per term: gamma_f = (1 + u)^123 - 1; its autograd pushes a cotangent back through the same 121-tap convolution and sums
up to 36 pad cells into a corner pixel: gamma_a = (1 + u)^(123 + 36) - 1; its mean adds 3 H W values, at most 3 H W roundings per
term.  Autograd evaluates the partial derivatives by the chain rule through the graph, not by the closed forms here: the same number
of operations of the same magnitudes within a factor 2, which `REF` carries as `slack`.
No pixel is excluded anywhere: every denominator is at least C1 C2 > 0."""
import math

import numpy as np
import torch

U = 2.0 ** -24
R, NT = 5, 11
C1, C2 = 0.01 ** 2, 0.03 ** 2
TILE_H, TILE_W = 16, 32                              # the kernels' output tile (SPAA_SSIM_TILE_H / _W of include/spaa_hip.h)

# 1 x 1: every tap on one pixel; 3 x 5: smaller than the radius, both edges feed one pixel; 11 x 11; just under / over one tile along
# each axis with the other axis below a tile; 2 x 3 tiles with ragged last tiles, so that halos cross tile borders
SIZES = ((1, 1), (3, 5), (11, 11), (TILE_H - 1, 9), (TILE_H + 1, 9), (7, TILE_W - 1), (7, TILE_W + 1), (TILE_H + 5, 2 * TILE_W + 6))
KINDS = ('flat', 'textured', 'equal', 'planted')


def taps():
    """The 11 taps as the reference's gaussian(11, 1.5) makes them: float64 exponentials, rounded to fp32, normalised in fp32."""
    g = torch.Tensor([math.exp(-(x - NT // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(NT)])
    return (g / g.sum()).numpy()


def filter_matrix(n, w, zero_pad=False):
    """F_n of the module docstring; zero_pad: the taps that fall beyond the border are dropped instead of clamped."""
    F = np.zeros((n, n))
    for p in range(n):
        for k in range(NT):
            q = p + k - R
            if 0 <= q < n:
                F[p, q] += float(w[k])
            elif not zero_pad:
                F[p, min(max(q, 0), n - 1)] += float(w[k])
    return F


def _rgb(a):
    return np.asarray(a, dtype=np.float64)[..., :3]


def _filt(Fh, Fw, x):
    return np.moveaxis(Fh @ np.moveaxis(x, 2, 0) @ Fw.T, 0, 2)             # [p][s][c] = sum_qr Fh[p][q] x[q][r][c] Fw[s][r]


def _adj(Fh, Fw, m):
    return np.moveaxis(Fh.T @ np.moveaxis(m, 2, 0) @ Fw, 0, 2)             # [q][s][c] = sum_pr Fh[p][q] m[p][r][c] Fw[r][s]


def stats(y, s, _bug=None):
    """(mu1, mu2, e11, e22, e12), each [H][W][3]."""
    y, s = _rgb(y), _rgb(s)
    w = taps()
    Fh, Fw = (filter_matrix(n, w, zero_pad=_bug == 'zero_padding') for n in y.shape[:2])
    mu1, mu2, e11, e22, e12 = (_filt(Fh, Fw, x) for x in (y, s, y * y, s * s, y * s))
    if _bug == 'scene_stats_for_y':
        mu1, e11 = mu2, e22
    if _bug == 'var_for_cov':
        e12 = e11
    return mu1, mu2, e11, e22, e12


def _algebra(mu1, mu2, e11, e22, e12, _bug=None):
    """S and its partials with respect to mu1, e11 and e12."""
    c1, c2 = (C2, C1) if _bug == 'c1_c2_swapped' else (C1, C2)
    A1, A2 = 2 * mu1 * mu2 + c1, 2 * (e12 - mu1 * mu2) + c2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + c1, (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + c2
    S = A1 * A2 / (B1 * B2)
    m_mu = 2 * mu2 * (A2 - A1) / (B1 * B2) - S * (2 * mu1 / B1 - 2 * mu1 / B2)
    return S, m_mu, -S / B2, 2 * A1 / (B1 * B2)


def ssim_map(y, s, _bug=None):
    return _algebra(*stats(y, s, _bug), _bug)[0]


def ssim(y, s, _bug=None):
    """SSIM_b: the mean of the map over 3 H W."""
    S = ssim_map(y, s, _bug)
    return S.sum() / (S.size // 3 if _bug == 'mean_over_hw' else S.size)


def grad_sum(y, s, _bug=None):
    """The gradient of 3 H W (1 - SSIM_b) at y, [H][W][3]: -(F^T m_mu + 2 y F^T m_11 + s F^T m_12)."""
    y, s = _rgb(y), _rgb(s)
    w = taps()
    _, m_mu, m_11, m_12 = _algebra(*stats(y, s, _bug), _bug)
    Fh, Fw = (filter_matrix(n, w, zero_pad=_bug in ('zero_padding', 'adjoint_without_pad_taps')) for n in y.shape[:2])
    two = 1.0 if _bug == 'missing_factor_2' else 2.0
    return -(_adj(Fh, Fw, m_mu) + two * y * _adj(Fh, Fw, m_11) + s * _adj(Fh, Fw, m_12))


def grad(y, s, _bug=None):
    """d (1 - SSIM_b) / d y."""
    g = grad_sum(y, s, _bug)
    return g / (g.size // 3 if _bug == 'mean_over_hw' else g.size)


# ---------------------------------------------------------------------------------------------------------------- bars
# the constants of an arithmetic: gamma_f on F|x| per filter, gamma_a on F^T|m| per adjoint, roundings per term of the mean, slack
KERNEL = dict(gamma_f=(1 + 11 * U) ** 2 - 1, gamma_a=(1 + 66 * U) ** 2 - 1, sum_roundings=lambda n: 15, slack=1.0, shift=True)
REF = dict(gamma_f=(1 + U) ** 123 - 1, gamma_a=(1 + U) ** (123 + 36) - 1, sum_roundings=lambda n: n, slack=2.0, shift=False)


class _V:
    """A float64 value and a bound on its fp32 evaluation's error."""

    def __init__(self, v, e=0.0):
        self.v, self.e = np.asarray(v, dtype=np.float64), np.asarray(e, dtype=np.float64) + np.zeros_like(v, dtype=np.float64)

    def _r(self):
        self.e = self.e + U * np.abs(self.v)
        return self

    def __add__(self, o):
        o = o if isinstance(o, _V) else _V(o, U * abs(o))     # (a constant: rounded to fp32 once)
        return _V(self.v + o.v, self.e + o.e)._r()

    def __sub__(self, o):
        return _V(self.v - o.v, self.e + o.e)._r()

    def __mul__(self, o):
        if not isinstance(o, _V):                             # (a power of two: exact)
            return _V(self.v * o, self.e * abs(o))
        return _V(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)._r()

    def __truediv__(self, o):
        lo = np.abs(o.v) - o.e
        assert (lo > 0).all(), 'a denominator whose bound reaches 0'
        q = self.v / o.v
        return _V(q, (self.e + np.abs(q) * o.e) / lo)._r()

    def __neg__(self):
        return _V(-self.v, self.e)


def _walk(y, s, c, arith):
    """The evaluation `arith` of S, the three maps and the unscaled gradient on one image pair, as _V; c [3]: the constants the
    moments are accumulated about (the kernels), or None (the reference: plain moments)."""
    w = taps()
    Fh, Fw = (filter_matrix(n, w) for n in y.shape[:2])
    gf, ga = arith['gamma_f'], arith['gamma_a']

    def filt(x):
        return _V(_filt(Fh, Fw, x.v), _filt(Fh, Fw, x.e) + gf * _filt(Fh, Fw, np.abs(x.v)))

    if c is None:
        Y, T = _V(y), _V(s)
        mu1, mu2, e11, e22, e12 = filt(Y), filt(T), filt(Y * Y), filt(T * T), filt(Y * T)
        m12s = mu1 * mu2
        var1, var2, cov = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - m12s
        A1, B1 = m12s * 2 + C1, (mu1 * mu1 + mu2 * mu2) + C1
    else:
        sw = float(np.sum(w.astype(np.float64)))
        Wt, omw, cc = _V(sw * sw, U * sw * sw), _V(1 - sw * sw, U * abs(1 - sw * sw)), _V(np.broadcast_to(c, y.shape))
        Y, T = _V(y) - cc, _V(s) - cc
        m1, m2, q11, q22, q12 = filt(Y), filt(T), filt(Y * Y), filt(T * T), filt(Y * T)
        k0 = cc * cc * Wt
        var1 = (q11 - m1 * m1) + omw * ((cc * 2) * m1 + k0)
        var2 = (q22 - m2 * m2) + omw * ((cc * 2) * m2 + k0)
        cov = (q12 - m1 * m2) + omw * (cc * (m1 + m2) + k0)
        mu1, mu2 = m1 + cc * Wt, m2 + cc * Wt
        A1, B1 = (mu1 * mu2) * 2 + C1, (mu1 * mu1 + mu2 * mu2) + C1
    A2, B2 = cov * 2 + C2, (var1 + var2) + C2
    D = B1 * B2
    S = (A1 * A2) / D
    m_mu = (mu2 * 2 * (A2 - A1)) / D - S * ((mu1 * 2) / B1 - (mu1 * 2) / B2)
    m_11 = -(S / B2)
    m_12 = (A1 * 2) / D
    return S, m_mu, m_11, m_12


def scene_stats(s, arith=KERNEL):
    """What spaa_ssim_scene_stats stores: (m2, q22, bar of m2, bar of q22), each [H][W][3]: the window mean and second moment of
    scene - c, c per tile and channel the scene's (fp32) value at the tile's first pixel, with the walk's bounds."""
    s = _rgb(s)
    H, W = s.shape[:2]
    w = taps()
    Fh, Fw = filter_matrix(H, w), filter_matrix(W, w)
    out = [np.zeros_like(s) for _ in range(4)]
    for y0 in range(0, H, TILE_H):
        for x0 in range(0, W, TILE_W):
            T = _V(s) - _V(np.broadcast_to(s[y0, x0], s.shape))
            res = []
            for x in (T, T * T):
                res += [_filt(Fh, Fw, x.v), _filt(Fh, Fw, x.e) + arith['gamma_f'] * _filt(Fh, Fw, np.abs(x.v))]
            for o, r in zip(out, (res[0], res[2], res[1], res[3])):
                o[y0:y0 + TILE_H, x0:x0 + TILE_W] = r[y0:y0 + TILE_H, x0:x0 + TILE_W]
    return out


def maps(y, s):
    """(S, m_mu, m_11, m_12) of the definition, each [H][W][3]."""
    return _algebra(*stats(y, s))


def bars(y, s, arith=KERNEL):
    """dict(S, m_mu, m_11, m_12, grad_sum: [H][W][3] bounds per value; value: the bound of SSIM_b) for the evaluation described by
    `arith` (KERNEL or REF) on this pair of images."""
    y, s = _rgb(y), _rgb(s)
    H, W = y.shape[:2]
    if arith['shift']:   # per tile: the moments about the scene's value at the tile's first pixel
        maps = [_V(np.zeros_like(y)) for _ in range(4)]
        for y0 in range(0, H, TILE_H):
            for x0 in range(0, W, TILE_W):
                for full, m in zip(_walk(y, s, s[y0, x0], arith), maps):
                    m.v[y0:y0 + TILE_H, x0:x0 + TILE_W] = full.v[y0:y0 + TILE_H, x0:x0 + TILE_W]
                    m.e[y0:y0 + TILE_H, x0:x0 + TILE_W] = full.e[y0:y0 + TILE_H, x0:x0 + TILE_W]
        S, m_mu, m_11, m_12 = maps
    else:
        S, m_mu, m_11, m_12 = _walk(y, s, None, arith)
    w = taps()
    Fh, Fw = filter_matrix(H, w), filter_matrix(W, w)
    ga = arith['gamma_a']

    def adj(m):
        return _V(_adj(Fh, Fw, m.v), _adj(Fh, Fw, m.e) + ga * _adj(Fh, Fw, np.abs(m.v)))

    g = (adj(m_mu) + _V(2 * y) * adj(m_11)) + _V(s) * adj(m_12)
    n = S.v.size
    val = (S.e.sum() + arith['sum_roundings'](n) * U * np.abs(S.v).sum()) / n + U * abs(S.v.sum() / n)
    k = arith['slack']
    return dict(S=k * S.e, m_mu=k * m_mu.e, m_11=k * m_11.e, m_12=k * m_12.e, grad_sum=k * g.e, value=k * val)


# ---------------------------------------------------------------------------------------------------------------- inputs
def inputs(kind, H, W, seed=0):
    """(y, scene) [H][W][4] float32 in [0, 1]: 'flat' a flat bright image against a flat bright scene (the cancellation case),
    'textured' smooth structure plus noise, 'equal' the image is the scene, 'planted' the textured pair with 0, -0.0 and 1 planted."""
    rng = np.random.default_rng(1000 * H + W + 7919 * seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    if kind == 'flat':
        y = np.full((H, W, 4), 0.9, np.float32)
        s = np.full((H, W, 4), 0.85, np.float32)
    else:
        base = 0.5 + 0.3 * np.sin(0.7 * xx + 0.3)[..., None] * np.cos(0.5 * yy[..., None] + np.arange(4))
        s = np.clip(base + 0.15 * (rng.random((H, W, 4)) - 0.5), 0, 1).astype(np.float32)
        y = np.clip(s + 0.2 * (rng.random((H, W, 4)) - 0.5), 0, 1).astype(np.float32)
        if kind == 'equal':
            y = s.copy()
        if kind == 'planted':
            for i, v in enumerate((0.0, -0.0, 1.0)):
                y[(i * 5) % H, (i * 3) % W, :3] = v
                s[(i * 7 + 1) % H, (i * 2 + 1) % W, :3] = v
    y[..., 3], s[..., 3] = 7.0, -3.0      # the pad lane: never read into a result
    return y, s


def _mutants(bug, *fns):
    return {f.__name__: (lambda *a, _f=f, **k: _f(*a, _bug=bug, **k)) for f in fns}


# name -> the functions whose results the mistake moves
MUTATIONS = {
    'zero_padding': _mutants('zero_padding', ssim, grad_sum),
    'adjoint_without_pad_taps': _mutants('adjoint_without_pad_taps', grad_sum),
    'var_for_cov': _mutants('var_for_cov', ssim, grad_sum),
    'c1_c2_swapped': _mutants('c1_c2_swapped', ssim, grad_sum),
    'missing_factor_2': _mutants('missing_factor_2', grad_sum),
    'mean_over_hw': _mutants('mean_over_hw', ssim, grad),
    'scene_stats_for_y': _mutants('scene_stats_for_y', ssim, grad_sum),
}
