"""Float64 restatement of the fused shading tail and head (csrc/shading_tail.hip), for the tail tests: the
forward tail (`tail`), the backward head (`head`), the bounds on what the kernels' arithmetic can have done to them (`tail_bars`,
`head_bars`), the inputs and references the tests share (`SHAPES`, `CONTENTS`, `cases`, `inputs`, `reference_fwd`, `reference_bwd`)
and `MUTATIONS`: the same functions with one deliberate mistake each, which tests/test_shading_tail_cpu.py shows to move the results
by more than their bars.  numpy on the CPU, written from the layers' definitions, nothing from the kernels.  A helper, not a test
module.

Layouts (channel last): X6 [B][H2][W2][64], res1 / y / ypre / g [B][H][W][4] with H = 2 H2, W = 2 W2 (channel 3 is padding), mask7
[B][H][W][8] and mask6 [B][H2][W2][16] (bit e of byte c / 4 = channel c = 4 (c / 4) + e passes), gate_y [B][H][W] (bit e: 0 < ypre_e <=
1), state [B][4] int32, P6 [B][H2][W2][64].  Weights as the layers hold them: transConv2 `w2` [64 in][32 out][2][2], conv6 `w6`
[3 out][32 in][3][3].  The functions take the OPERAND VALUES the kernels are handed (`operands`): in fp32 storage the fp32 weights
(the packed planes sum to them exactly); in fp16 storage X6 as fp16, `w2` and the forward's `w6` rounded to fp16, and the adjoint's
conv6 weights in fp32 -- the head kernel rounds those to fp16 itself, which `head` restates (a rounding of an input: it has one result).

    pre7[2i+py][2j+px][c] = b2[c] + sum_k x6[i][j][k] w2[k][c][py][px]          x7 = relu(pre7)   (fp16 storage: rounded to fp16)
    pre[y][x][o] = b6[o] + res1[y][x][o] + sum_{ky,kx,c} w6[o][c][ky][kx] x7[y+ky-1][x+kx-1][c]       (zero outside the image)
    ypre = relu(pre), y = min(ypre, 1);  mask7 bit = x7 > 0;  gate_y bit = 0 < ypre <= 1
    cot = g[..., :3], or with `state`: (state[b][1] != 0 ? g_col : g) gated per channel by the byte / by 0 < ypre <= 1
    p7[y][x][c] = mask7 . sum_{ky,kx,o} w6[o][c][ky][kx] cot[y-ky+1][x-kx+1][o]                      (fp16 storage: rounded to fp16)
    p6[i][j][k] = mask6 . sum_{py,px,c} w2[k][c][py][px] p7[2i+py][2j+px][c]

THE BARS, with u = 2^-24 (fp32's unit roundoff) and h = 2^-11 (fp16's), follow the kernels' own sequence of operations; none is set
from what a kernel produced.

  * A sum of n addends t_i in fp32, in ANY order and grouping (the order inside an MFMA is not ours to assume): every addition rounds
    by at most u |its result| <= u sum |t_i| (to first order; the magnitudes below are taken with their own bars added, which covers
    the second), and an addend passes through at most one addition per addend: n u sum |t_i| for a chain that starts from 0.  One more
    addition (a bias) makes it (n + 1) u (sum |t_i| + |bias|).
  * bf16x6 product (fp32 storage; transConv2, both adjoints): a = a0 + a1 + a2 exactly, three bf16 planes of 8 significant bits:
    |a1| <= 2^-8 |a|, |a2| <= 2^-16 |a|, |a0| <= (1 + 2^-8) |a|.  Kept: w0 x0, w0 x1, w1 x0, w1 x1, w0 x2, w2 x0, each exact in fp32
    (8 + 8 bits).  Dropped: w1 x2, w2 x1, w2 x2 <= (2^-24 + 2^-24 + 2^-32) |w| |x| = DROP u |w| |x|, DROP = 2 + 2^-8.  The kept
    ones are 6 addends per term of magnitude <= (|w0| + |w1| + |w2|)(|x0| + |x1| + |x2|) <= SPLIT |w| |x| together, SPLIT =
    (1 + 2^-7 + 2^-16)^2.  A chain of n terms is 6 n addends:   (DROP + 6 n SPLIT) u sum |w| |x|,   n = 64 for transConv2 (+ 1: the
    bias), 27 for conv6's adjoint (one K = 32 step; its five zero slots add exactly), 128 for transConv2's adjoint.  For n = 64 that
    is 387 u = 2.3e-5 of sum |W| |x|.  The x6 family's MEASURED figure of tests/test_tuned_launches_gpu.py, 1.1e-6 of sum |W| |x|
    over K up to 4096, sits 20 times inside: roundings do not conspire, a worst-case bound assumes that they do.  The measured
    figure is not used here.
  * conv6 forward, fp32 storage: 288 fp32 FMAs per output (products not rounded separately), the two channel halves joined through
    LDS, then + b6: 289 additions in some order, THEN + res1 (the source adds it last and is compiled without reassociation).
    fp16 storage: fp16 x fp16 products are exact in fp32 (11 + 11 bits); three MFMA chains of 96 terms (one per tap column), their two
    joins and + b6: 99, then + res1.  With T = sum |w6| |x7| + |b6|:   n6 u T + the last addition's rounding, which is at most
    u |result| and at most |the other addend| (res1 is itself a candidate result): where X7 is zero and b6 is zero the sum IS res1.
  * first layer into second: sum |w6| bar(x7) forward, sum |w2| bar(p7) backward (27 terms, then 128).
  * fp16 storage: transConv2 is one chain of 64 exact products + bias: 65 u.  conv6's adjoint multiplies the fp16-rounded weights by
    the cotangent split into fp16 hi + lo: |g - hi - lo| <= max(2^-22 |g|, 2^-25) (lo is an fp16 subnormal below |g| = 2^-3), 54
    addends (two MFMAs of 27).  transConv2's adjoint: 128 u.  P6 is rounded to fp16 when stored: h (|p6| + its bar), at least 2^-25.
    X7 and P7 are ROUNDED TO fp16 IN LDS, and rounding is discontinuous: a value whose bar reaches a rounding boundary may land on
    either neighbour, one fp16 ulp (up to 2 h |value|) apart; a value whose bar reaches none rounds exactly as the float64 value does,
    with error 0.  So the bar of a rounded value is max(fl16(v + e) - fl16(v), fl16(v) - fl16(v - e)) for the unrounded bar e (rounding
    is monotone: the kernel's value lies between the two).  A flat "h |value| + e" for every element, the first thing one writes
    down, is at the same time too small at a boundary (by a factor of up to 2) and so wide elsewhere that dropping the rounding
    altogether stays inside it: `x7_rounding_dropped` would pass.
  * Gates.  A `mask7` bit is asserted where the interval [pre7 - bar, pre7 + bar] (rounded to fp16 in fp16 storage, as the kernel
    tests the rounded value) lies on one side of 0; `gate_y` bits and y's clamp where [pre - bar, pre + bar] holds neither 0 nor 1
    in its interior -- with bar = 0 (the planted image) that asserts the edges themselves.  `left_out` gives the share that is not
    asserted; the tests cap it at 1e-3 per case.  In `head` the masks and the clamp gate are inputs: nothing can flip."""
import functools

import numpy as np

U, H = 2.0 ** -24, 2.0 ** -11
DROP = 2.0 + 2.0 ** -8
SPLIT = (1.0 + 2.0 ** -7 + 2.0 ** -16) ** 2
C6, C7 = 64, 32
LEFT_OUT_CAP = 1e-3

# (B, H2, W2); B = None: the persistent walk, B from the device's compute units (`walk_batch`)
SHAPES = ((1, 1, 1), (2, 6, 14), (2, 7, 15), (1, 8, 16), (2, 9, 17), (3, 5, 23), (None, 9, 17))
STORAGES = ('f32', 'f16')
CONTENTS = ('random', 'edges')
CUS_MI355X = 256
PLANTED = (0.0, -0.0, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(1), np.float32(0))), -1e-30, 2.0)


def walk_batch(cus):
    """The smallest B with 4 B > 2 cus + 8: at 18 x 34 an image is four tiles of either kernel, the grids are cus and 2 cus."""
    return (2 * cus + 8) // 4 + 1


def fwd_tiles(B, H2, W2):
    return B * (-(-(2 * H2 + 1) // 14)) * (-(-(2 * W2 + 1) // 30))      # (the owned 14 x 30 interiors start at row / column -1)


def bwd_tiles(B, H2, W2):
    return B * (-(-H2 // 8)) * (-(-W2 // 16))


def fl16(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def _relu(a):
    return np.maximum(a, 0.0)


def unpack_bits(m, nch):
    """uint8 [..., nch / 4] -> bool [..., nch]."""
    m = np.asarray(m, dtype=np.uint8)
    return ((m[..., :, None] >> np.arange(4, dtype=np.uint8)) & 1).astype(bool).reshape(*m.shape[:-1], nch)


def pack_bits(b):
    """bool [..., C] -> uint8 [..., C / 4]."""
    b = np.asarray(b, dtype=np.uint8)
    q = b.reshape(*b.shape[:-1], b.shape[-1] // 4, 4)
    return (q * np.array([1, 2, 4, 8], dtype=np.uint8)).sum(-1).astype(np.uint8)


def pack_gate3(b):
    """bool [..., 3] -> one byte per pixel."""
    b = np.asarray(b, dtype=np.uint8)
    return (b[..., 0] | (b[..., 1] << 1) | (b[..., 2] << 2)).astype(np.uint8)


def operands(w2, b2, w6, b6, storage):
    """The operand values a kernel of `storage` is handed, float64: dict(w2, b2, w6 (the forward's), w6a (the adjoint's), b6)."""
    w2, b2, w6, b6 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (w2, b2, w6, b6))
    if storage == 'f16':
        return dict(w2=fl16(w2), b2=b2, w6=fl16(w6), w6a=w6, b6=b6)
    return dict(w2=w2, b2=b2, w6=w6, w6a=w6, b6=b6)


# ------------------------------------------------------------------------------------------------------------ the layers
def _tconv(x6, w2):
    """[B][H2][W2][64] -> [B][H][W][32]: out[2 i + py][2 j + px][c] = sum_k x6[i][j][k] w2[k][c][py][px]."""
    B, H2, W2, _ = x6.shape
    return np.einsum('bijk,kcpq->bipjqc', x6, w2, optimize=True).reshape(B, 2 * H2, 2 * W2, C7)


def _tconv_adj(p7, w2):
    """[B][H][W][32] -> [B][H2][W2][64]: out[i][j][k] = sum_{py,px,c} w2[k][c][py][px] p7[2 i + py][2 j + px][c]."""
    B, Hh, Ww, _ = p7.shape
    return np.einsum('bipjqc,kcpq->bijk', p7.reshape(B, Hh // 2, 2, Ww // 2, 2, C7), w2, optimize=True)


def _conv6(x7, w6, mirrored=False):
    """[B][H][W][32] -> [B][H][W][3]: out[y][x][o] = sum w6[o][c][ky][kx] x7[y + ky - 1][x + kx - 1][c], zero outside."""
    B, Hh, Ww, _ = x7.shape
    xp = np.pad(x7, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((B, Hh, Ww, 3))
    for ky in range(3):
        for kx in range(3):
            w = w6[:, :, 2 - ky, 2 - kx] if mirrored else w6[:, :, ky, kx]
            out += xp[:, ky:ky + Hh, kx:kx + Ww, :] @ w.T
    return out


def _conv6_adj(cot, w6, mirrored=True):
    """[B][H][W][3] -> [B][H][W][32]: out[y][x][c] = sum w6[o][c][ky][kx] cot[y - ky + 1][x - kx + 1][o], zero outside."""
    B, Hh, Ww, _ = cot.shape
    cp = np.pad(cot, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((B, Hh, Ww, C7))
    for ky in range(3):
        for kx in range(3):
            oy, ox = (2 - ky, 2 - kx) if mirrored else (ky, kx)
            out += cp[:, oy:oy + Hh, ox:ox + Ww, :] @ w6[:, :, ky, kx]
    return out


def _first_row_col_from(full, alt):
    out = full.copy()
    out[:, 0], out[:, :, 0] = alt[:, 0], alt[:, :, 0]
    return out


def _zero_first_row_col(a):
    z = a.copy()
    z[:, 0], z[:, :, 0] = 0.0, 0.0
    return z


def _gate3(ypre, bug=None):
    yp = np.asarray(ypre, dtype=np.float64)[..., :3]
    lo = yp >= 0 if bug == 'relu_ge' else yp > 0
    hi = yp < 1 if bug == 'clamp_lt' else yp <= 1
    return lo & hi


def _neighbour(bits):
    return bits.reshape(*bits.shape[:-1], -1, 2)[..., ::-1].reshape(bits.shape)      # channel c <- channel c ^ 1


# ------------------------------------------------------------------------------------------------------------ forward
def tail(x6, res1, ops, storage, _bug=None):
    """dict(pre7, x7, pre, ypre, y [.., 3 channels], mask7 [B][H][W][8] uint8, gate_y [B][H][W] uint8)."""
    x6, res1 = np.asarray(x6, dtype=np.float64), np.asarray(res1, dtype=np.float64)
    w2 = ops['w2'].transpose(0, 1, 3, 2) if _bug == 'parity_swapped' else ops['w2']
    pre7 = _tconv(x6, w2) + ops['b2']
    x7 = _relu(pre7)
    if storage == 'f16' and _bug != 'x7_rounding_dropped':
        x7 = fl16(x7)
    bits7 = (pre7 >= 0) if _bug == 'relu_ge' else (x7 > 0)
    if _bug == 'gate_neighbour_channel':
        bits7 = _neighbour(bits7)
    conv = _conv6(x7, ops['w6'], mirrored=_bug == 'tap_mirrored')
    if _bug == 'border_off_by_one':      # the first owned row and column miss the X7 row and column they sit on
        conv = _first_row_col_from(conv, _conv6(_zero_first_row_col(x7), ops['w6']))
    pre = conv + ops['b6'] + res1[..., :3]
    ypre = _relu(pre)
    return dict(pre7=pre7, x7=x7, pre=pre, ypre=ypre, y=np.minimum(ypre, 1.0), mask7=pack_bits(bits7), gate_y=pack_gate3(_gate3(ypre, _bug)))


def tail_bars(x6, res1, ops, storage):
    """The bounds along `tail`: dict(pre7, x7, pre [.., 3]: bounds per value (pre's holds for ypre and y: relu and min are
    1-Lipschitz); one7 / zero7 bool [B][H][W][32]: the mask7 bit is certainly 1 / 0; gate_sure bool [.., 3]: the gate_y bit and the
    clamp's side are certain; left_out: the share of mask7 bits and of gate bits that are not)."""
    x6, res1 = np.asarray(x6, dtype=np.float64), np.asarray(res1, dtype=np.float64)
    r = tail(x6, res1, ops, storage)
    s7 = _tconv(np.abs(x6), np.abs(ops['w2']))
    a7 = s7 + np.abs(ops['b2'])
    bar7 = U * 65 * a7 if storage == 'f16' else U * (DROP * s7 + (6 * C6 + 1) * SPLIT * a7)
    lo, hi = _relu(r['pre7'] - bar7), _relu(r['pre7'] + bar7)
    if storage == 'f16':
        lo, hi = fl16(lo), fl16(hi)
    barx7 = np.maximum(hi - r['x7'], r['x7'] - lo)
    assert (barx7 >= 0).all()
    one7, zero7 = lo > 0, hi <= 0
    w6a = np.abs(ops['w6'])
    p = _conv6(barx7, w6a)
    t = _conv6(np.abs(r['x7']) + barx7, w6a) + np.abs(ops['b6'])
    n6 = 99 if storage == 'f16' else 289
    before = p + n6 * U * t
    last = np.minimum(U * (np.abs(r['pre']) + before), t * (1 + n6 * U))
    bar = before + last
    plo, phi = r['pre'] - bar, r['pre'] + bar
    gate_sure = (phi <= 0) | ((plo > 0) & (phi <= 1)) | (plo > 1)
    left = dict(mask7=1.0 - float((one7 | zero7).mean()), gate=1.0 - float(gate_sure.mean()))
    return dict(pre7=bar7, x7=barx7, pre=bar, one7=one7, zero7=zero7, gate_sure=gate_sure, left_out=left)


# ------------------------------------------------------------------------------------------------------------ backward
def cotangent(g, state=None, g_col=None, gate=None, _bug=None):
    """[B][H][W][3]: g's first three channels, or with `state` the sample's choice gated by `gate` (uint8: the byte; float: ypre)."""
    g = np.asarray(g, dtype=np.float64)
    if state is None:
        return g[..., :3].copy()
    g_col = np.asarray(g_col, dtype=np.float64)
    if _bug == 'g_adv_g_col_swapped':
        g, g_col = g_col, g
    sel = np.asarray(state)[:, 0 if _bug == 'state_column_0' else 1] != 0
    cot = np.where(sel[:, None, None, None], g_col, g)[..., :3]
    gate = np.asarray(gate)
    if gate.dtype == np.uint8:
        ok = ((gate[..., None] >> np.arange(3, dtype=np.uint8)) & 1).astype(bool)
    else:
        ok = _gate3(gate, _bug)
    return np.where(ok, cot, 0.0)


def _head(cot, mask7, mask6, ops, storage, _bug=None):
    w6 = fl16(ops['w6a']) if storage == 'f16' else ops['w6a']
    w2 = ops['w2'].transpose(0, 1, 3, 2) if _bug == 'parity_swapped' else ops['w2']
    raw = _conv6_adj(cot, w6, mirrored=_bug != 'adjoint_not_mirrored')
    if _bug == 'border_off_by_one':
        raw = _first_row_col_from(raw, _conv6_adj(_zero_first_row_col(cot), w6))
    bits7 = unpack_bits(mask7, C7)
    if _bug == 'gate_neighbour_channel':
        bits7 = _neighbour(bits7)
    p7 = np.where(bits7, raw, 0.0)
    if storage == 'f16':
        p7 = fl16(p7)
    return cot, w6, p7, np.where(unpack_bits(mask6, C6), _tconv_adj(p7, w2), 0.0)


def head(g, mask7, mask6, ops, storage, state=None, g_col=None, gate=None, _bug=None):
    """P6 [B][H2][W2][64]."""
    return _head(cotangent(g, state, g_col, gate, _bug), mask7, mask6, ops, storage, _bug)[3]


def head_bars(g, mask7, mask6, ops, storage, state=None, g_col=None, gate=None):
    """The bound on `head`'s P6, per value (fp16 storage: of the fp16 number the kernel stores)."""
    cot, w6, p7, p6 = _head(cotangent(g, state, g_col, gate), mask7, mask6, ops, storage)
    s = _conv6_adj(np.abs(cot), np.abs(w6))
    b7, w2a = unpack_bits(mask7, C7), np.abs(ops['w2'])
    if storage == 'f16':
        resid = np.where(cot != 0, np.maximum(2.0 ** -22 * np.abs(cot), 2.0 ** -25), 0.0)
        e = np.where(b7, _conv6_adj(resid, np.abs(w6)) + 54 * U * s, 0.0)
        exact = np.where(b7, _conv6_adj(cot, w6), 0.0)
        bar7 = np.maximum(fl16(exact + e) - p7, p7 - fl16(exact - e))
        assert (bar7 >= 0).all()
        t = _tconv_adj(np.abs(p7) + bar7, w2a)
        raw = _tconv_adj(bar7, w2a) + 128 * U * t
        bar = raw + np.maximum(H * (np.abs(p6) + raw), 2.0 ** -25)
    else:
        bar7 = np.where(b7, U * (DROP + 6 * 27 * SPLIT) * s, 0.0)
        t = _tconv_adj(np.abs(p7) + bar7, w2a)
        bar = _tconv_adj(bar7, w2a) + U * (DROP + 6 * 128 * SPLIT) * t
    return np.where(unpack_bits(mask6, C6), bar, 0.0)


# ------------------------------------------------------------------------------------------------------------ inputs
def weights(seed=0):
    """transConv2's and conv6's weights and biases at their initialisation scale (uniform in +- 1 / sqrt(fan_in)), fp32."""
    rng = np.random.default_rng(4201 + seed)
    k2, k6 = 1 / np.sqrt(32 * 4), 1 / np.sqrt(32 * 9)
    return (rng.uniform(-k2, k2, (C6, C7, 2, 2)).astype(np.float32), rng.uniform(-k2, k2, C7).astype(np.float32),
            rng.uniform(-k6, k6, (3, C7, 3, 3)).astype(np.float32), rng.uniform(-k6, k6, 3).astype(np.float32))


def _plant(a, rng, zero_image=None):
    """PLANTED into the first three channels of `a` [B][H][W][4], over and over along the pixels of one image (or of all)."""
    B, Hh, Ww, _ = a.shape
    vals = np.array(PLANTED, dtype=np.float32)
    for b in range(B) if zero_image is None else (zero_image,):
        flat = a[b, ..., :3].reshape(-1)
        idx = rng.permutation(flat.size)[:max(len(vals), flat.size // 3)]
        flat[idx] = vals[np.arange(idx.size) % len(vals)]
        a[b, ..., :3] = flat.reshape(Hh, Ww, 3)


def inputs(content, storage, B, H2, W2):
    """The arrays of one case, as the kernels take them (fp32, X6 fp16 in fp16 storage, uint8 masks, int32 state): dict(w2, b2, w6, b6
    raw fp32 weights; x6, res1; g_adv, g_col, ypre_in, mask7_in, mask6_in, state for the head; zero_image: the all-zero image of
    'edges', or None)."""
    rng = np.random.default_rng(100003 * B + 1009 * H2 + 31 * W2 + (7 if storage == 'f16' else 0) + (3 if content == 'edges' else 0))
    Hh, Ww = 2 * H2, 2 * W2
    w2, b2, w6, b6 = weights()
    x6 = (np.abs(rng.standard_normal((B, H2, W2, C6))) * (rng.random((B, H2, W2, C6)) > 1 / 3)).astype(np.float32)
    res1 = rng.uniform(-0.2, 1.2, (B, Hh, Ww, 4)).astype(np.float32)
    g_adv, g_col = (rng.standard_normal((B, Hh, Ww, 4)).astype(np.float32) for _ in range(2))
    ypre_in = _relu(rng.uniform(-0.5, 1.5, (B, Hh, Ww, 4))).astype(np.float32)
    zero_image = None
    if content == 'edges':
        b2, b6 = np.zeros_like(b2), np.zeros_like(b6)
        zero_image = B - 1
        x6[zero_image] = 0
        _plant(res1, rng, zero_image)
        _plant(ypre_in, rng)
        ypre_in[..., :3] = _relu(ypre_in[..., :3])        # (a pre-clamp output: never below 0; -0.0 and -1e-30 become 0)
    if storage == 'f16':
        x6 = x6.astype(np.float16)
    for a in (res1, g_adv, g_col, ypre_in):                # the pad channel: never read into a result
        a[..., 3] = 7.0
        a[:, ::2, :, 3] = -3.0
    state = rng.integers(1, 1000, (B, 4)).astype(np.int32)      # nonzero junk in columns 0, 2, 3
    state[:, 1] = np.arange(B) * np.where(np.arange(B) % 2, 1, -1)      # 0, 1, -2, 3, ...: a different value per sample
    return dict(w2=w2, b2=b2, w6=w6, b6=b6, x6=x6, res1=res1, g_adv=g_adv, g_col=g_col, ypre_in=ypre_in,
                mask7_in=rng.integers(0, 16, (B, Hh, Ww, C7 // 4)).astype(np.uint8),
                mask6_in=rng.integers(0, 16, (B, H2, W2, C6 // 4)).astype(np.uint8), state=state, zero_image=zero_image)


def cases(cus=CUS_MI355X):
    """[(content, storage, B, H2, W2)]: every shape in both storages with both contents."""
    return [(c, s, B if B is not None else walk_batch(cus), h2, w2) for B, h2, w2 in SHAPES for s in STORAGES for c in CONTENTS]


@functools.lru_cache(maxsize=2)
def case_inputs(content, storage, B, H2, W2):
    """(inp, ops) of one case, computed once and not to be written to."""
    inp = inputs(content, storage, B, H2, W2)
    return inp, operands(inp['w2'], inp['b2'], inp['w6'], inp['b6'], storage)


@functools.lru_cache(maxsize=2)
def reference_fwd(content, storage, B, H2, W2):
    """(tail's results, tail_bars') of one case, computed once and not to be written to."""
    inp, ops = case_inputs(content, storage, B, H2, W2)
    return tail(inp['x6'], inp['res1'], ops, storage), tail_bars(inp['x6'], inp['res1'], ops, storage)


@functools.lru_cache(maxsize=2)
def reference_bwd(content, storage, B, H2, W2):
    """form ('plain', 'select', 'select_g') -> (P6, its bar) of one case, computed once and not to be written to."""
    inp, ops = case_inputs(content, storage, B, H2, W2)
    a = (inp['g_adv'], inp['mask7_in'], inp['mask6_in'], ops, storage)
    return {form: (head(*a, **kw), head_bars(*a, **kw)) for form, kw in head_forms(inp).items()}


def head_forms(inp):
    """form -> the keyword arguments of `head` / `head_bars`: the plain form on g_adv, the select form on ypre_in, the select form on
    the byte built from ypre_in."""
    sel = dict(state=inp['state'], g_col=inp['g_col'])
    return dict(plain={}, select=dict(sel, gate=inp['ypre_in']), select_g=dict(sel, gate=pack_gate3(_gate3(inp['ypre_in']))))


# ------------------------------------------------------------------------------------------------------------ mutations
# name -> (the functions it moves, the storages and the contents at which it must show)
MUTATIONS = {
    'parity_swapped': (('tail', 'head'), STORAGES, CONTENTS),
    'tap_mirrored': (('tail',), STORAGES, CONTENTS),
    'adjoint_not_mirrored': (('head',), STORAGES, CONTENTS),
    'border_off_by_one': (('tail', 'head'), STORAGES, CONTENTS),
    'gate_neighbour_channel': (('tail', 'head'), STORAGES, CONTENTS),
    'relu_ge': (('tail', 'head'), STORAGES, ('edges',)),
    'clamp_lt': (('tail', 'head'), STORAGES, ('edges',)),
    'state_column_0': (('head',), STORAGES, CONTENTS),
    'g_adv_g_col_swapped': (('head',), STORAGES, CONTENTS),
    'x7_rounding_dropped': (('tail',), ('f16',), CONTENTS),
}
