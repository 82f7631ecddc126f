"""Float64 restatement of the camera JPEG round trip, for the JPEG tests: the quantisation tables (`quant_tables`), the
round trip with everything it passes on the way (`forward`), its linearisation and adjoint in both gradient modes (`linearised`,
`adjoint`), the same chain in torch double for autograd (`forward_torch`), the integer rule of the quality draw (`draw_rows`), the
distances that decide what an fp32 kernel can be held to (`half_distance`, `safe_pixels`, `round_distance`), the derived fp32 bars
(`bar_adjoint`) and `MUTATIONS`: one deliberate mistake each, which tests/test_jpeg_cpu.py shows to be caught.  numpy on the CPU.  A
helper, not a test module.

Every linear step on a plane is a pair of explicit matrices (rows, columns): padding by edge replication, the 2 x 2 mean, the triangle
filter, the block DCT.  The adjoint applies their transposes, so that it is the transpose by construction; the autograd test and the
dot-product test then check the chain's order and the factor phi.

The bars, with u = 2^-24 (the unit roundoff of fp32):

forward.  An fp32 coefficient differs from the float64 one by at most E_c: the two 8-term passes with |D| row sums <= 2.83 give
2 * 8 u * 2.83^2 * M = 128 u M for samples |b - 128| <= M = 128, and the samples' own error (255 clamp, the 3-term colour sums, the
mean: <= 5 u 255 each) passes through D . D^T with an infinity norm <= 8: 40 u 255 < 80 u 128.  E_c = 256 u 128 = 2^-9 bounds both;
what is seen is several times smaller.  A coefficient whose c / T is nearer than that to a half-integer may round the other way, which
moves a whole block, so blocks are compared only where every c / T they depend on keeps HALF_MARGIN from the half-integers, and a
pixel whose pre-round value is within ROUND_MARGIN of a rounding boundary may come out one level off.  Both margins are the issue's.

adjoint.  A chain of linear maps A_n ... A_1 in fp32 errs by at most (sum of the maps' term counts) u |A_n| ... |A_1| |g|: `adjoint`
with absolute=True evaluates that product of absolute values, and N_OPS counts the terms: 1 (/ 255) + 3 (colour) + 8 (triangle, 4 per
axis) + 16 (DCT) + 1 (phi) + 16 (IDCT) + 1 (mean) + 3 (colour) + 2 (255, gate) + 13 for the rounding of the constants themselves = 64,
plus the cells summed into an edge pixel, at most (Hp - H + 1)(Wp - W + 1).  In 'soft' mode phi = 3 r^2 itself is computed from an
fp32 r: |d phi| <= 6 |r| d_s + 3 d_s^2 with d_s = E_c / T + 2 u |c / T| (the division and the subtraction), and the second term of the
bar is the absolute chain with d phi in the place of phi.  phi is continuous where the rounding flips, so no block is left out for
the adjoint's sake; the gates are given to the kernel."""
import numpy as np
import torch

import jitter_oracle as jo

U = 2.0 ** -24
E_C = 2.0 ** -9
HALF_MARGIN = 1e-3
ROUND_MARGIN = 1e-3
FIRST_CONSTANT = 0xc2b2ae35

# ITU-T T.81 Annex K, tables K.1 and K.2, natural (row-major) order
LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61,
                 12, 12, 14, 19, 26, 58, 60, 55,
                 14, 13, 16, 24, 40, 57, 69, 56,
                 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77,
                 24, 35, 55, 64, 81, 104, 113, 92,
                 49, 64, 78, 87, 103, 121, 120, 101,
                 72, 92, 95, 98, 112, 100, 103, 99]).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99,
                   18, 21, 26, 66, 99, 99, 99, 99,
                   24, 26, 56, 99, 99, 99, 99, 99,
                   47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32).reshape(8, 8)


def zigzag_positions():
    """The natural-order index of zig-zag position z, z = 0..63."""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order)


def quant_tables(Q, _bug=None):
    """(luminance, chrominance) int [8][8] at quality Q in 1..100, natural order, scaled as libjpeg scales them."""
    Q = int(Q)
    s = 5000 // Q if (Q < 50 and _bug != 'lowq') else 200 - 2 * Q
    out = []
    for base in ((CHROMA if _bug == 'chroma_on_y' else LUMA), CHROMA):
        t = np.clip((base * s + 50) // 100, 1, 255)
        if _bug == 'zigzag':   # the natural-order entries laid out along the zig-zag
            z = np.zeros(64, dtype=t.dtype)
            z[zigzag_positions()] = t.ravel()
            t = z.reshape(8, 8)
        out.append(t)
    return out[0], out[1]


def dct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    d = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    d[0] = np.sqrt(1.0 / 8.0)
    return d


D = dct_matrix()
TO_YCC = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]])   # (+128 on Cb, Cr)
TO_RGB = np.array([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]])                 # of (Y, Cb - 128, Cr - 128)


# ---------------------------------------------------------------------------------------------- the linear steps as matrices
def pad_matrix(n, npad, _bug=None):
    """[npad][n]: edge replication."""
    m = np.zeros((npad, n))
    m[np.arange(n), np.arange(n)] = 1
    if _bug != 'zeropad':
        m[n:, n - 1] = 1
    return m


def box_matrix(n):
    """[n / 2][n]: the mean of two neighbours."""
    m = np.zeros((n // 2, n))
    m[np.arange(n) // 2, np.arange(n)] = 0.5
    return m


def tri_matrix(n, _bug=None):
    """[2 n][n]: (3 near + far) / 4 with edge replication; libjpeg's "fancy" upsampling along one axis."""
    m = np.zeros((2 * n, n))
    i = np.arange(2 * n)
    near = i >> 1
    if _bug == 'replicate':
        m[i, near] = 1
        return m
    far = np.clip(near + np.where(i & 1, 1, -1), 0, n - 1)
    np.add.at(m, (i, near), 0.75)
    np.add.at(m, (i, far), 0.25)
    return m


def block_dct(n, d=D):
    """[n][n]: the 8-point matrix d on every 8 samples."""
    return np.kron(np.eye(n // 8), d)


def both(rows, x, cols):
    return rows @ x @ cols.T


def geometry(H, W, subsampling):
    if subsampling not in ('4:4:4', '4:2:0'):
        raise ValueError(subsampling)
    mcu = 16 if subsampling == '4:2:0' else 8
    return -(-H // mcu) * mcu, -(-W // mcu) * mcu, subsampling == '4:2:0'


def tiled(T, shape):
    return np.tile(T, (shape[0] // 8, shape[1] // 8)).astype(np.float64)


# ---------------------------------------------------------------------------------------------- the round trip
def forward(y, Q, subsampling='4:2:0', _bug=None):
    """y [H][W][>= 3] float64, Q in 0..100 -> dict: out [H][W][3] (levels / 255), v the pre-round values, in_gate / out_gate bool
    [H][W][3], gate uint8 [H][W] (in-gates bits 0-2, out-gates bits 4-6), ratios = c / T per plane (padded, chroma at its own
    resolution), tables.  Q = 0: the identity row."""
    y = np.asarray(y, dtype=np.float64)[..., :3]
    H, W, _ = y.shape
    if int(Q) == 0:
        ones = np.ones((H, W, 3), dtype=bool)
        return dict(out=y.copy(), v=y * 255.0, in_gate=ones, out_gate=ones, gate=np.full((H, W), 0x77, dtype=np.uint8), ratios=None)
    Hp, Wp, sub = geometry(H, W, subsampling)
    in_gate = (y >= 0) & (y <= 1)
    p = 255.0 * np.clip(y, 0, 1)
    to_ycc = TO_YCC[[0, 2, 1]] if _bug == 'swap' else TO_YCC
    planes = [p @ to_ycc[k] + (128.0 if k else 0.0) for k in range(3)]
    PH, PW = pad_matrix(H, Hp, _bug), pad_matrix(W, Wp, _bug)
    planes = [both(PH, pl, PW) for pl in planes]
    if sub:
        BH, BW = box_matrix(Hp), box_matrix(Wp)
        planes[1:] = [both(BH, pl, BW) for pl in planes[1:]]
    TL, TC = quant_tables(Q, _bug)
    ratios, dec = [], []
    for pl, T in zip(planes, (TL, TC, TC)):
        DH, DW = block_dct(pl.shape[0]), block_dct(pl.shape[1])
        c = both(DH, pl - (0.0 if _bug == 'noshift' else 128.0), DW)
        s = c / tiled(T, pl.shape)
        ratios.append(s)
        dec.append(both(DH.T, np.rint(s) * tiled(T, pl.shape), DW.T) + 128.0)
    if sub:
        UH, UW = tri_matrix(Hp // 2, _bug), tri_matrix(Wp // 2, _bug)
        dec[1:] = [both(UH, d, UW) for d in dec[1:]]
    ycc = np.stack([dec[0], dec[1] - 128.0, dec[2] - 128.0], axis=-1)[:H, :W]
    v = ycc @ TO_RGB.T
    out_gate = (v >= 0) & (v <= 255)
    out = np.rint(np.clip(v, 0, 255)) / 255.0
    bits = sum(in_gate[..., c].astype(np.uint8) << c for c in range(3)) + sum(out_gate[..., c].astype(np.uint8) << (4 + c) for c in range(3))
    return dict(out=out, v=v, in_gate=in_gate, out_gate=out_gate, gate=bits.astype(np.uint8), ratios=ratios, tables=(TL, TC))


def phi_of(ratios, gradient, _bug=None):
    """The factor that stands for d rint(s) / ds: 1 ('straight'), 3 r^2 with r = s - rint(s) ('soft': the derivative of k + r^3)."""
    if gradient not in ('soft', 'straight'):
        raise ValueError(gradient)
    if gradient == 'straight' or _bug == 'nophi':
        return [np.ones_like(s) for s in ratios]
    return [3.0 * (s - np.rint(s)) ** 2 for s in ratios]


def linearised(u, y, Q, subsampling='4:2:0', gradient='soft'):
    """The linearisation of the round trip at y applied to a direction u [H][W][3]: every linear step as it is, the gates, phi in the
    place of the coefficient rounding, the 8-bit step straight-through."""
    y = np.asarray(y, dtype=np.float64)[..., :3]
    if int(Q) == 0:
        return np.asarray(u, dtype=np.float64).copy()
    H, W, _ = y.shape
    Hp, Wp, sub = geometry(H, W, subsampling)
    fw = forward(y, Q, subsampling)
    dp = 255.0 * fw['in_gate'] * u
    planes = [both(pad_matrix(H, Hp), dp @ TO_YCC[k], pad_matrix(W, Wp)) for k in range(3)]
    if sub:
        planes[1:] = [both(box_matrix(Hp), pl, box_matrix(Wp)) for pl in planes[1:]]
    dec = []
    for pl, phi in zip(planes, phi_of(fw['ratios'], gradient)):
        DH, DW = block_dct(pl.shape[0]), block_dct(pl.shape[1])
        dec.append(both(DH.T, phi * both(DH, pl, DW), DW.T))
    if sub:
        dec[1:] = [both(tri_matrix(Hp // 2), d, tri_matrix(Wp // 2)) for d in dec[1:]]
    dv = np.stack(dec, axis=-1)[:H, :W] @ TO_RGB.T
    return fw['out_gate'] * dv / 255.0


def adjoint(g, y, Q, subsampling='4:2:0', gradient='soft', _bug=None, absolute=False, phi=None, gates=None):
    """g [H][W][>= 3] = d loss / d out -> d loss / dy [H][W][3]: the transposes in reverse order.  `absolute`: every matrix by its
    absolute values (for the bars); `phi`: given factors in the place of phi_of(); `gates`: (in_gate, out_gate) in the place of the
    forward's own."""
    y = np.asarray(y, dtype=np.float64)[..., :3]
    g = np.asarray(g, dtype=np.float64)[..., :3]
    if int(Q) == 0:
        return g.copy()
    mag = np.abs if absolute else (lambda m: m)
    H, W, _ = y.shape
    Hp, Wp, sub = geometry(H, W, subsampling)
    fw = forward(y, Q, subsampling)
    in_gate, out_gate = gates if gates is not None else (fw['in_gate'], fw['out_gate'])
    phi = phi if phi is not None else phi_of(fw['ratios'], gradient, _bug)
    gv = np.zeros((Hp, Wp, 3))
    gv[:H, :W] = out_gate * g / 255.0
    gd = [gv @ mag(TO_RGB)[:, k] for k in range(3)]
    if sub:
        UH, UW = tri_matrix(Hp // 2), tri_matrix(Wp // 2)
        gd[1:] = [both(UH.T, d, UW.T) for d in gd[1:]]
    gb = []
    for d, f in zip(gd, phi):
        DH, DW = block_dct(d.shape[0], mag(D)), block_dct(d.shape[1], mag(D))
        gb.append(both(DH.T, f * both(DH, d, DW), DW.T))
    if sub:
        BH, BW = box_matrix(Hp), box_matrix(Wp)
        gb[1:] = [both(BH.T, d, BW.T) for d in gb[1:]]
    if _bug == 'droppad':
        gb = [d[:H, :W] for d in gb]
    else:
        PH, PW = pad_matrix(H, Hp), pad_matrix(W, Wp)
        gb = [both(PH.T, d, PW.T) for d in gb]
    gp = np.stack(gb, axis=-1) @ mag(TO_YCC)
    return 255.0 * in_gate * gp


def bar_adjoint(g, y, Q, subsampling='4:2:0', gradient='soft', gates=None):
    """[H][W][3]: what an fp32 adjoint may differ by from adjoint() (see the module docstring)."""
    y = np.asarray(y, dtype=np.float64)[..., :3]
    if int(Q) == 0:
        return np.zeros_like(y)
    H, W, _ = y.shape
    Hp, Wp, _ = geometry(H, W, subsampling)
    fw = forward(y, Q, subsampling)
    phi = phi_of(fw['ratios'], gradient)
    n_ops = 64 + (Hp - H + 1) * (Wp - W + 1)
    bar = n_ops * U * adjoint(np.abs(g), y, Q, subsampling, absolute=True, phi=phi, gates=gates)
    if gradient == 'soft':
        TL, TC = fw['tables']
        dphi = []
        for s, T in zip(fw['ratios'], (TL, TC, TC)):
            d_s = E_C / tiled(T, s.shape) + 2 * U * np.abs(s)
            dphi.append(6 * np.abs(s - np.rint(s)) * d_s + 3 * d_s ** 2)
        bar = bar + adjoint(np.abs(g), y, Q, subsampling, absolute=True, phi=dphi, gates=gates)
    return bar


# ---------------------------------------------------------------------------------------------- what fp32 can be held to
def half_distance(ratios):
    """Per plane, per 8 x 8 block: the distance of the block's nearest c / T to a half-integer, [Hb][Wb]."""
    out = []
    for s in ratios:
        d = 0.5 - np.abs(s - np.rint(s))
        out.append(d.reshape(s.shape[0] // 8, 8, s.shape[1] // 8, 8).min(axis=(1, 3)))
    return out


def safe_pixels(fw, H, W, subsampling, margin=HALF_MARGIN):
    """bool [H][W]: the pixels that depend on no block with a c / T within `margin` of a half-integer: those of the block itself
    and, for the chroma blocks of 4:2:0, also the one pixel around its 16 x 16 pixels that the triangle filter carries it to."""
    if fw['ratios'] is None:
        return np.ones((H, W), dtype=bool)
    Hp, Wp, sub = geometry(H, W, subsampling)
    bad = np.zeros((Hp, Wp), dtype=bool)
    for k, d in enumerate(half_distance(fw['ratios'])):
        m = np.kron((d < margin).astype(np.float64), np.ones((8, 8)))
        if sub and k:
            m = both((tri_matrix(Hp // 2) > 0).astype(np.float64), m, (tri_matrix(Wp // 2) > 0).astype(np.float64))
        bad |= m > 0
    return ~bad[:H, :W]


def unsafe_block_fraction(fw, margin=HALF_MARGIN):
    """The share of the round trip's 8 x 8 blocks, over its three planes, whose nearest c / T is within `margin` of a half-integer."""
    if fw['ratios'] is None:
        return 0.0
    d = np.concatenate([h.ravel() for h in half_distance(fw['ratios'])])
    return float((d < margin).mean())


def round_distance(v):
    """Per pixel and channel: the distance of the clamped pre-round value to the nearest rounding boundary (a half-integer)."""
    c = np.clip(v, 0, 255)
    return np.abs(np.abs(c - np.floor(c)) - 0.5)


# ---------------------------------------------------------------------------------------------- torch, for autograd
def forward_torch(y, Q, subsampling='4:2:0', gradient='soft'):
    """The round trip of y [H][W][3] (a torch double tensor) with the coefficient rounding as k + r^3, k detached ('soft'), or
    s + (k - s).detach() ('straight'), and the 8-bit step straight-through.  The value of r^3 is taken off again (detached), so that
    the forward values, and with them the out-gates, are forward()'s: true rounding in both modes, the surrogate's derivative."""
    if int(Q) == 0:
        return y * 1.0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    H, W, _ = y.shape
    Hp, Wp, sub = geometry(H, W, subsampling)
    p = 255.0 * y.clamp(0, 1)
    planes = [p @ t(TO_YCC[k]) + (128.0 if k else 0.0) for k in range(3)]
    planes = [t(pad_matrix(H, Hp)) @ pl @ t(pad_matrix(W, Wp)).T for pl in planes]
    if sub:
        planes[1:] = [t(box_matrix(Hp)) @ pl @ t(box_matrix(Wp)).T for pl in planes[1:]]
    TL, TC = quant_tables(Q)
    dec = []
    for pl, T in zip(planes, (TL, TC, TC)):
        DH, DW, Tt = t(block_dct(pl.shape[0])), t(block_dct(pl.shape[1])), t(tiled(T, pl.shape))
        s = (DH @ (pl - 128.0) @ DW.T) / Tt
        k = torch.round(s).detach()
        r3 = (s - k) ** 3
        q = k + r3 - r3.detach() if gradient == 'soft' else s + (k - s).detach()
        dec.append(DH.T @ (q * Tt) @ DW + 128.0)
    if sub:
        dec[1:] = [t(tri_matrix(Hp // 2)) @ d @ t(tri_matrix(Wp // 2)).T for d in dec[1:]]
    v = torch.stack([dec[0], dec[1] - 128.0, dec[2] - 128.0], dim=-1)[:H, :W] @ t(TO_RGB).T
    c = v.clamp(0, 255)
    return (c + (torch.round(c) - c).detach()) / 255.0


# ---------------------------------------------------------------------------------------------- the draw
def draw_word(seed, t, b, j, i):
    """jitter_oracle.draw_word behind the JPEG stage's own first constant."""
    h = jo.mix32((seed & jo.M32) ^ FIRST_CONSTANT)
    for v in (t, b, j, i):
        h = jo.mix32(h ^ (v & jo.M32))
    return h


def draw_rows(seed, t, B, J, q_lo, q_hi, clean0):
    """row float32 [B][J][4] of iteration t: (Q, 0, 0, 0), Q = q_lo + (((h >> 8) n) >> 24), n = q_hi - q_lo + 1."""
    row = np.zeros((B, J, 4), dtype=np.float32)
    n = q_hi - q_lo + 1
    for b in range(B):
        for j in range(J):
            row[b, j, 0] = 0 if (clean0 and j == 0) else q_lo + (((draw_word(seed, t, b, j, 0) >> 8) * n) >> 24)
    return row


# ---------------------------------------------------------------------------------------------- inputs
def smooth_image(H, W):
    """A smooth, colourful image [H][W][3] in [0, 1]: slow sinusoids with a different phase and direction per channel, so that the
    chroma planes carry gradients of tens of levels per block."""
    i, k = np.mgrid[0:H, 0:W].astype(np.float64)
    r = 0.5 + 0.45 * np.sin(2 * np.pi * (i / H + 0.3 * k / W))
    g = 0.5 + 0.45 * np.sin(2 * np.pi * (k / W - 0.4 * i / H) + 2.0)
    b = 0.5 + 0.45 * np.cos(2 * np.pi * (0.7 * i / H + 0.8 * k / W) + 4.0)
    return np.stack([r, g, b], axis=-1)


def float_image(rng, H, W, planted=6, noise=4e-4, texture=0.03):
    """A float image [H][W][3] (not on the 8-bit grid, so that ties are not generic): a smooth part, faint noise everywhere (its
    coefficients stay well below one half even where T = 1, so that the smooth part decides which blocks sit near a tie), one
    textured 8 x 8 patch where the image has room for it (a block with a full spectrum), and `planted` values outside [0, 1] for the
    in-gates."""
    y = 0.3 + 0.4 * smooth_image(H, W) + rng.normal(0, noise, (H, W, 3))
    if H >= 32 and W >= 32:
        y[16:24, 16:24] += rng.normal(0, texture, (8, 8, 3))
    y = np.clip(y, 0.01, 0.99)
    for _ in range(planted):
        y[rng.integers(H), rng.integers(W), rng.integers(3)] = rng.choice([-0.2, 1.3, -0.01, 1.05])
    return y


# ---------------------------------------------------------------------------------------------- mutations
FORWARD_MUTATIONS = ('zigzag', 'chroma_on_y', 'lowq', 'noshift', 'swap', 'replicate', 'zeropad')
TABLE_MUTATIONS = ('zigzag', 'chroma_on_y', 'lowq')
ADJOINT_MUTATIONS = ('droppad', 'nophi')
MUTATIONS = {
    'zigzag': 'the table in zig-zag order instead of natural order',
    'chroma_on_y': 'the chroma table on Y',
    'lowq': 'the Q < 50 scaling branch wrong',
    'noshift': 'no level shift before the DCT',
    'swap': 'Cb and Cr swapped',
    'replicate': 'replicate instead of triangle upsampling',
    'zeropad': 'no edge replication in the padding',
    'droppad': "the padded cells' gradient dropped in the adjoint",
    'nophi': "phi missing in 'soft'",
}
