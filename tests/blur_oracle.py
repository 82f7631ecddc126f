"""Float64 / integer restatement of the lens blur, for the blur tests: the draw word and the drawn sigmas in Python
integers (`draw_word`, `draw_sigmas`), the radius and the taps of a sigma (`radius`, `taps`, `row_of`, `rows_of`), the filter of one
axis as an explicit matrix (`axis_matrix`), the forward (`forward`), the transpose as the explicit transposed matrix (`backward`) and
as the fold formula of include/spaa_hip.h (`fold_formula`), the bars (`bar_sigma`, `bar_row`, `bar_forward`, `bar_backward`) and
MUTATIONS: one deliberate mistake each, switched on with `_bug`.  Independent of the host module.  A helper, not a test module.

Everything that starts from a sigma starts from the fp32 value the kernel wrote: `radius` evaluates ceil(3 sigma) in numpy float32, as
the kernel does, so that a float64 sigma one rounding away cannot pick another radius; the taps are then float64 functions of that fp32
value.

The bars, in units of the fp32 unit roundoff U = 2^-24:
  sigma    the kernel's fmaf(hi - lo, u, lo) rounds once; the restatement rounds the exact float64 sum to fp32, which can differ from it by
           double rounding only: one ulp of the larger end of the range, 2 U max(|lo|, |hi|).
  tap i    a_i = -(i i) / (2 sigma sigma) carries three roundings, which exp magnifies by |a_i|; expf is within EXPF_ULPS; the norm adds r
           terms, doubles, adds 1, and every tap is divided by it: relative (3 |a_i| + EXPF_ULPS + r + 3) U.  `tap_ulps` is the largest of
           these over the taps of a row, and what the image bars charge for taps that differ from the kernel's by that much.
  forward  one pass is a sum of 2 r + 1 products, r + 1 of them after an addition of two inputs: (2 r + 2) U of sum |w| |x| per pass, two
           passes, plus two passes of tap error: (2 (2 r + 2) + 2 tap_ulps) U (|A_H| |y| |A_W|^T).
  adjoint  an interior pixel is the forward's sum, (2 r + 2) U.  An edge pixel is sum_{m = 0 .. r} T_m g_m with the tail sums T_m = w_m + ..
           + w_r: T_m carries r - m additions, at most r U relative, and the r + 1 products and their additions r + 2 more: (2 r + 2) U
           again.  The bar charges (3 r + 3) U per pass, which also covers an edge sum taken literally as r + 1 values z_e of 2 r + 1
           products each (the form of the header's formula): (2 (3 r + 3) + 2 tap_ulps) U (|A_H|^T |g| |A_W|)."""
import numpy as np

M32 = 0xffffffff
U = 2.0 ** -24
RMAX = 8                 # SPAA_BLUR_RMAX
SIGMA_MAX = 2.5
ROW = 12                 # floats of a row: sigma, r, w_0 .. w_8, 0
FIRST = 0x2545f491       # the first constant of the blur's draw words
EXPF_ULPS = 2.0          # the device expf (documented within 1 ulp; twice that)

MUTATIONS = {
    'zeropad': 'zero padding instead of the replicated border',
    'nofold': 'the transpose without the fold: the taps that left the frame are lost',
    'fold_inner': 'the fold lands in pixel 1 / n - 2 instead of the edge pixel',
    'floor': 'r = floor(3 sigma) instead of ceil',
    'unnormalised': 'the taps are not divided by their sum',
    'norm_once': 'the norm counts the side taps once: w_0 + (w_1 + .. + w_r)',
    'jitter_constant': "the jitter's first constant 0x9e3779b9 in the draw word",
    'lowbits': 'u from the low 24 bits of the word instead of h >> 8',
    'clean0_ignored': 'clean0 is ignored: draw 0 is drawn like the others',
    'colclampW': 'the pass along the columns clamps its row index with W',
}
DRAW_MUTATIONS = ('jitter_constant', 'lowbits', 'clean0_ignored')
ROW_MUTATIONS = ('floor', 'unnormalised', 'norm_once')
FORWARD_MUTATIONS = ('zeropad', 'colclampW')
BACKWARD_MUTATIONS = ('nofold', 'fold_inner')


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw_word(seed, t, b, j, i, _bug=None):
    """The 32-bit word of (seed, iteration t, sample b, draw j, parameter index i) behind the blur's first constant."""
    h = mix32((seed & M32) ^ (0x9e3779b9 if _bug == 'jitter_constant' else FIRST))
    for v in (t, b, j, i):
        h = mix32(h ^ (v & M32))
    return h


def draw_sigmas(seed, t, B, J, lo, hi, clean0, _bug=None):
    """The sigmas [B][J] of iteration t as fp32 values (held in float64): fl32(lo + (hi - lo) u), hi - lo in fp32 as the kernel's
    argument of fmaf, the product exact in float64 (24 x 24 bits)."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    d = float(np.float32(hi32 - lo32))
    out = np.zeros((B, J))
    for b in range(B):
        for j in range(J):
            if clean0 and j == 0 and _bug != 'clean0_ignored':
                continue
            h = draw_word(seed, t, b, j, 0, _bug)
            u = ((h & 0xffffff) if _bug == 'lowbits' else (h >> 8)) / 16777216.0
            out[b, j] = float(np.float32(float(lo32) + d * u))
    return out


def bar_sigma(lo, hi):
    return 2.0 * U * max(abs(float(lo)), abs(float(hi)))


def radius(sigma, _bug=None):
    """r of the fp32 value `sigma`, evaluated in fp32 as the kernel evaluates it."""
    s = np.float32(sigma)
    if not s > 0:
        return 0
    x = np.float32(3.0) * s
    return int(min(RMAX, np.floor(x) if _bug == 'floor' else np.ceil(x)))


def taps(sigma, _bug=None):
    """(r, w float64 [RMAX + 1]) of the fp32 value `sigma`: the half kernel, entries beyond w_r are 0."""
    r = radius(sigma, _bug)
    s = float(np.float32(sigma))
    w = np.zeros(RMAX + 1)
    w[0] = 1.0
    for i in range(1, r + 1):
        w[i] = np.exp(-(i * i) / (2.0 * s * s)) if s * s > 0 else 0.0
    if _bug == 'unnormalised':
        return r, w
    return r, w / (w[0] + (1.0 if _bug == 'norm_once' else 2.0) * w[1:].sum())


def tap_ulps(sigma):
    """The largest relative error of a tap of the kernel's row of `sigma`, in units of U (the module docstring derives it)."""
    r, s = radius(sigma), float(np.float32(sigma))
    if r == 0:
        return 0.0
    a = min((r * r) / (2.0 * s * s), 104.0)   # (beyond exp(-104) the fp32 tap is 0 and carries no error)
    return 3.0 * a + EXPF_ULPS + r + 3.0


def row_of(sigma, _bug=None):
    r, w = taps(sigma, _bug)
    s = float(np.float32(sigma))
    return np.concatenate(([s if s > 0 else 0.0, float(r)], w, [0.0]))


def rows_of(sigmas, _bug=None):
    """[..., 12] rows of an array of fp32 sigmas."""
    sg = np.asarray(sigmas, dtype=np.float64)
    return np.stack([row_of(s, _bug) for s in sg.ravel()]).reshape(sg.shape + (ROW,))


def bar_row(sigma):
    """[12]: 0 for sigma (compared on its own), r and the pad (exact), the taps' relative bar times the taps."""
    r, w = taps(sigma)
    return np.concatenate(([0.0, 0.0], U * tap_ulps(sigma) * w, [0.0]))


def axis_matrix(n, r, w, _bug=None, clamp_n=None):
    """A [n][n] of one axis: out[m] = sum_k w_|k| in[clamp(m + k, 0, n - 1)], k = -r .. r.  `clamp_n`: the length the index is clamped
    with (the mutation 'colclampW': the other axis's; an index it lets beyond n - 1 reads what lies there, taken as row index mod n)."""
    A = np.zeros((n, n))
    for m in range(n):
        for k in range(-r, r + 1):
            q = m + k
            if _bug == 'zeropad':
                if 0 <= q < n:
                    A[m, q] += w[abs(k)]
                continue
            q = min(max(q, 0), (clamp_n or n) - 1) % n
            A[m, q] += w[abs(k)]
    return A


def forward(y, r, w, _bug=None):
    """y [H][W][C] float64 -> the separable filter with the half kernel w of radius r along both axes, border replicated."""
    y = np.asarray(y, dtype=np.float64)
    H, W = y.shape[:2]
    AW = axis_matrix(W, r, w, _bug)
    AH = axis_matrix(H, r, w, _bug, clamp_n=W if _bug == 'colclampW' else None)
    return np.einsum('im,mkc->ikc', AH, np.einsum('kn,mnc->mkc', AW, y))


def transpose_matrix(n, r, w, _bug=None):
    """A^T [n][n] of one axis, explicitly; the mutations: 'nofold' transposes the zero-padded filter, 'fold_inner' moves what the edge
    pixel collected beyond its own taps into its inner neighbour."""
    if _bug == 'nofold':
        return axis_matrix(n, r, w, 'zeropad').T
    T = axis_matrix(n, r, w).T
    if _bug == 'fold_inner' and n >= 3:
        plain = axis_matrix(n, r, w, 'zeropad').T
        for edge, inner in ((0, 1), (n - 1, n - 2)):
            extra = T[edge] - plain[edge]
            T[edge] -= extra
            T[inner] += extra
    return T


def backward(g, r, w, _bug=None):
    """g [H][W][C] float64 -> A^T g: the transposed matrices of both axes."""
    g = np.asarray(g, dtype=np.float64)
    H, W = g.shape[:2]
    TH, TW = transpose_matrix(H, r, w, _bug), transpose_matrix(W, r, w, _bug)
    return np.einsum('pm,mqc->pqc', TH, np.einsum('qn,mnc->mqc', TW, g))


def fold_formula(g, r, w):
    """One axis (the first) of the transpose by the header's formula: z_e = sum_k w_|k| g_{e-k} for e = -r .. n - 1 + r with g zero outside
    [0, n); g_in[p] = z_p inside, g_in[0] = sum_{e <= 0} z_e, g_in[n - 1] = sum_{e >= n - 1} z_e."""
    g = np.asarray(g, dtype=np.float64)
    n = g.shape[0]
    pad = np.zeros((n + 4 * r,) + g.shape[1:])
    pad[2 * r:2 * r + n] = g
    z = {e: sum(w[abs(k)] * pad[e - k + 2 * r] for k in range(-r, r + 1)) for e in range(-r, n + r)}
    out = np.zeros_like(g)
    for p in range(n):
        lo, hi = (-r if p == 0 else p), (n - 1 + r if p == n - 1 else p)
        out[p] = sum(z[e] for e in range(lo, hi + 1))
    return out


def bar_forward(y, r, w, ulps_taps):
    y = np.abs(np.asarray(y, dtype=np.float64))
    return U * (2.0 * (2 * r + 2) + 2.0 * ulps_taps) * forward(y, r, np.abs(w))


def bar_backward(g, r, w, ulps_taps):
    g = np.abs(np.asarray(g, dtype=np.float64))
    return U * (2.0 * (3 * r + 3) + 2.0 * ulps_taps) * backward(g, r, np.abs(w))


def float_image(rng, H, W):
    """A test image [H][W][3] float64 with structure at every scale and values on both sides of [0, 1] (the filter has no clamp), as fp32
    values."""
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.4 * np.sin(0.37 * xx + 0.11 * yy)[..., None] * np.array([1.0, -0.7, 0.4])
    return (base + 0.35 * rng.normal(size=(H, W, 3))).astype(np.float32).astype(np.float64)
