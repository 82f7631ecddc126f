"""Python-integer / float64 restatement of the Square Attack on the projector image, for the square tests: the draws, the
side schedule, the loss, the choice / accept / success / rest rules and the query counter, written from the specification and
independent of spaa_amd/square_attack.py.  `run` drives the algorithm over any `evaluate(image uint8 [Hp, Wp, 3]) -> logits`; every
rule that a one-character slip can get wrong has a named MUTATION that makes exactly that slip, so that the tests can show they would
notice it.  `loss_bar` is the error allowed to an fp32 evaluation of the loss.  A helper, not a test module."""
import math

import numpy as np

M32 = 0xffffffff
INIT, PROPOSE = 0x27d4eb2f, 0x165667b1
MUTATIONS = ('accept_le',        # accepted on loss <= best_loss
             'tie_high',         # ties between proposals go to the highest k
             'h_clamp_min',      # h clamped to min(Hp, Wp) instead of min(Hp, Wp) - 1
             'mod_short',        # positions modulo Hp - h, Wp - h
             'no_p_thresh',      # targeted success without the probability threshold
             'rest_counted',     # a resting sample's query counter goes on
             'sign_order',       # the three sign bits in the order B, G, R
             'margin_with_y')    # the untargeted margin's maximum includes j == y


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def word(first, seed, t, b, k, i):
    h = mix32((seed ^ first) & M32)
    h = mix32(h ^ t)
    h = mix32(h ^ b)
    h = mix32(h ^ k)
    return mix32(h ^ i)


def value(c0, eps8, bit):
    return max(0, min(255, c0 + eps8)) if bit else max(0, min(255, c0 - eps8))


def side(t, n_iters, p_init, Hp, Wp, mut=None):
    it = int(t / n_iters * 10000)
    if it <= 10:
        d = 1
    elif it <= 50:
        d = 2
    elif it <= 200:
        d = 4
    elif it <= 500:
        d = 8
    elif it <= 1000:
        d = 16
    elif it <= 2000:
        d = 32
    elif it <= 4000:
        d = 64
    elif it <= 6000:
        d = 128
    elif it <= 8000:
        d = 256
    else:
        d = 512
    p = p_init / d
    top = min(Hp, Wp) if mut == 'h_clamp_min' else min(Hp, Wp) - 1
    return max(1, min(top, int(round(math.sqrt(p * Hp * Wp)))))


def stripes(seed, b, c0, eps8, Hp, Wp):
    im = np.zeros((Hp, Wp, 3), dtype=np.uint8)
    for w in range(Wp):
        for ch in range(3):
            im[:, w, ch] = value(c0, eps8, word(INIT, seed, 0, b, w, ch) & 1)
    return im


def proposal(seed, t, b, k, h, c0, eps8, Hp, Wp, mut=None):
    """[r, c, h, R, G, B, 0, 0]"""
    short = 0 if mut == 'mod_short' else 1
    r = word(PROPOSE, seed, t, b, k, 0) % (Hp - h + short)
    c = word(PROPOSE, seed, t, b, k, 1) % (Wp - h + short)
    s = word(PROPOSE, seed, t, b, k, 2)
    bits = [(s >> 2) & 1, (s >> 1) & 1, s & 1] if mut == 'sign_order' else [s & 1, (s >> 1) & 1, (s >> 2) & 1]
    return [r, c, h] + [value(c0, eps8, bit) for bit in bits] + [0, 0]


def paint(im, p):
    out = im.copy()
    r, c, h = p[:3]
    out[r:r + h, c:c + h, 0], out[r:r + h, c:c + h, 1], out[r:r + h, c:c + h, 2] = p[3], p[4], p[5]
    return out


def score(logits, y, targeted, mut=None):
    """(loss, top-1, p1) in float64: top-1 the first maximum, p1 its softmax probability."""
    l = np.asarray(logits, dtype=np.float64)
    mx = float(l.max())
    top1 = int(np.flatnonzero(l == mx)[0]) if not np.isnan(mx) else 0
    se = float(np.exp(l - mx).sum())
    if targeted:
        loss = mx + math.log(se) - float(l[y])
    else:
        others = l if mut == 'margin_with_y' else np.concatenate((l[:y], l[y + 1:]))
        loss = float(l[y]) - float(others.max())
    return loss, top1, 1.0 / se


def decide(losses, best_loss, mut=None):
    """(k*, accepted) of one sample's K losses."""
    ks, lo = -1, math.inf
    for k, l in enumerate(losses):
        if l < lo or (mut == 'tie_high' and l == lo and ks >= 0):
            ks, lo = k, l
    if ks < 0:
        return 0, False
    return ks, (lo <= best_loss) if mut == 'accept_le' else (lo < best_loss)


def success(top1, p1, y, targeted, p_thresh, mut=None):
    if not targeted:
        return top1 != y
    return top1 == y and (mut == 'no_p_thresh' or p1 > p_thresh)


def run(evaluate, labels, flags, K, Hp, Wp, c0, eps8, n_iters, p_init, p_thresh, seed, b_off=0, iters=None, mut=None):
    """Iterations 0 .. iters (default n_iters) without an early stop; one record per iteration: t, h, prop [B][K][8], rows [B][K][3]
    (loss, top-1, p1), state [B][4] (accepted, k*, done, queries), best_loss [B], x_u8 [B][Hp][Wp][3] after the iteration."""
    B = len(labels)
    x = [stripes(seed, b_off + b, c0, eps8, Hp, Wp) for b in range(B)]
    best = [math.inf] * B
    state = [[0, 0, 0, 0] for _ in range(B)]
    rows = [[(0.0, 0, 0.0)] * K for _ in range(B)]
    out = []
    for t in range((n_iters if iters is None else iters) + 1):
        h = 0 if t == 0 else side(t, n_iters, p_init, Hp, Wp, mut)
        prop = [[[0] * 8 for _ in range(K)] for _ in range(B)]
        for b in range(B):
            state[b][0] = 0
            if state[b][2]:
                if mut == 'rest_counted':
                    state[b][3] += K
                continue
            if t == 0:
                rows[b] = [score(evaluate(x[b]), labels[b], flags[b], mut)] * K
                spent = 1
            else:
                prop[b] = [proposal(seed, t, b_off + b, k, h, c0, eps8, Hp, Wp, mut) for k in range(K)]
                rows[b] = [score(evaluate(paint(x[b], p)), labels[b], flags[b], mut) for p in prop[b]]
                spent = K
            ks, acc = decide([r[0] for r in rows[b]], best[b], mut)
            if acc:
                if t:
                    x[b] = paint(x[b], prop[b][ks])
                best[b] = rows[b][ks][0]
                state[b][2] = int(success(rows[b][ks][1], rows[b][ks][2], labels[b], flags[b], p_thresh, mut))
            state[b][0], state[b][1] = int(acc), ks
            state[b][3] += spent
        out.append(dict(t=t, h=h, prop=np.array(prop), rows=np.array(rows, dtype=np.float64), state=np.array(state),
                        best_loss=np.array(best), x_u8=np.stack(x)))
    return out


def note(line):
    """A figure a test measured: printed as an `accuracy:` line and, where the environment variable SPAA_ACCURACY_FILE names a file,
    appended to it (`SPAA_ACCURACY_FILE=profiles/square_accuracy.txt pytest -m gpu tests/test_square_ops_gpu.py tests/test_square_gpu.py`
    on a fresh file is how that file is made)."""
    import os
    print('accuracy: ' + line)
    path = os.environ.get('SPAA_ACCURACY_FILE')
    if path:
        with open(path, 'a') as fh:
            fh.write('accuracy: ' + line + '\n')


def loss_bar(logits):
    """What an fp32 evaluation of the loss may differ by from float64 on the same logits, u = 2^-24, n = ncls, M = max |l|, L = log n:
    the sum of n terms exp(l - max) in (0, 1], each within 3 u of exact (one rounding of the difference, whose effect |d| e^-d u stays
    below u / e, and 2 u for expf), added in any order with at most n roundings of partial sums that never exceed the sum: relative error
    of the sum <= (n + 3) u, which is the absolute error of its logarithm; logf adds 2 u |log sum| <= 2 u L; max + log sum and the
    subtraction of l[y] round values bounded by M + L and 2 M + L.  Total <= u (n + 3 + 2 L + (M + L) + (2 M + L)), rounded up to
    u (n + 8 + 8 (M + L)).  The untargeted margin is one rounding of a difference bounded by 2 M, inside the same bar."""
    l = np.asarray(logits, dtype=np.float64)
    return 2.0 ** -24 * (l.size + 8 + 8 * (float(np.abs(l).max()) + math.log(l.size)))
