"""The engineered inputs of the universal entry points' tests (csrc/universal_ops.hip), built on the CPU: test_universal_cpu.py shows
with the float64 oracle that the cases hold what they are meant to hold and that every mutation of tests/universal_oracle.py is seen on
them; test_universal_ops_gpu.py runs the kernels on them.  A helper, not a test module."""
import itertools

import numpy as np

import universal_oracle as uo

P_THRESH = 0.9
ADV_SCALE = 0.25
# (B, N) x ncls x HW (nblk 1, 13 and 257) x rate
DECIDE_CASES = list(itertools.product([(6, 3), (4, 2), (5, 5), (64, 64)], [10, 1000], [1, 3120, 65537], [1.0, 0.5]))
LOSS_WEIGHTS = [(0.1, 1.0, 1.0), (0.0, 1.0, 0.0), (0.1, 0.0, 1.0), (0.0, 1.0, 1.0)]


def _roles(N, need):
    """What a group is made to be: (fooled members, targeted, d_thr, best colour loss so far).  caml2 * 255 is near 7: a d_thr of 5 is
    exceeded, one of 9 is not; a best so far of 1e6 is beaten, one of 1e-3 is not."""
    between = need - 1 if need > 1 else 0
    return [(N, True, 5.0, 1e6),          # every member fooled, above d_thr: a new best
            (0, True, 5.0, 1e6),          # nobody fooled
            (need, False, 5.0, 1e-3),     # just enough fooled: the colour step, no new best
            (between, False, 5.0, 1e6),   # some fooled, not enough
            (N, False, 9.0, 1e6),         # every member fooled below d_thr: the adversarial step goes on
            (need, True, 9.0, 1e6),
            (N - 1, True, 5.0, 1e6),      # all but one: enough when need < N
            (1, False, 9.0, 1e-3)]


def decide_case(BN, ncls, HW, rate):
    """One case of spaa_decide_universal: U = B / N groups, group u in the role (u + the case's number) % 8, its fooled members at
    random places, its other members alternately failing outright and (targeted) winning without confidence.  Every sample has one clear
    top-1; with `ncls` = 1000 and HW = 3120 (and 10 and 1) sample 1 has two equal maxima instead, the one pair of the case that is not
    clear, and its target is neither."""
    B, N = BN
    number = DECIDE_CASES.index((BN, ncls, HW, rate))
    rng = np.random.default_rng(1000 + number)
    need = uo.need_of(N, rate)
    nblk = (HW + 255) // 256
    roles = _roles(N, need)
    logits = rng.standard_normal((B, ncls)).astype(np.float32)
    target = rng.integers(0, ncls, B)
    targeted, d_thr, col_best, weights = np.zeros(B, dtype=bool), np.zeros(B), np.zeros(B), np.zeros((B, 3))
    for u in range(B // N):
        k, tg, dt, cb = roles[(u + number) % len(roles)]
        rows = slice(u * N, (u + 1) * N)
        targeted[rows], d_thr[rows], col_best[rows], weights[rows] = tg, dt, cb, LOSS_WEIGHTS[(u + number) % len(LOSS_WEIGHTS)]
        fooled = np.zeros(N, dtype=bool)
        fooled[rng.permutation(N)[:k]] = True
        for i in range(N):
            b, t = u * N + i, target[u * N + i]
            rival = (t + 1) % ncls
            if tg and fooled[i]:
                logits[b, t] = 14.0
            elif tg and i % 2 == 0:
                logits[b, t], logits[b, rival] = 6.0, 5.0        # top-1 with p1 ~ 0.7 at 10 classes, ~ 0.2 at 1000: not confident
            elif tg or fooled[i]:
                logits[b, t], logits[b, rival] = -5.0, 8.0       # another class wins
            else:
                logits[b, t] = 14.0                              # untargeted: the true class stays
    tie = None
    if (ncls, HW) in ((1000, 3120), (10, 1)):
        first, second = (2, 900) if ncls == 1000 else (3, 7)     # (1000: lanes of different waves; 10: of one)
        target[1] = 5
        logits[1] = rng.standard_normal(ncls).astype(np.float32)
        logits[1, first] = logits[1, second] = 9.0
        tie = (1, first)
    # per-block sums of 256 pixels' |scene - y| ~ 256 * 7 / 255, dE ~ 256 * 3; the third column is not read
    partial = (rng.uniform(0.8, 1.2, (B, nblk, 3)) * np.array([256 * 7.0 / 255.0, 256 * 3.0, 1.0]) * HW / (256.0 * nblk)).astype(np.float32)
    params = np.concatenate([weights, d_thr[:, None]], axis=1).astype(np.float32)
    prjl2 = rng.uniform(0.01, 0.05, B).astype(np.float32)        # (one per sample: only member 0's may be read)
    return dict(B=B, N=N, need=need, ncls=ncls, HW=HW, nblk=nblk, target=target, targeted=targeted, logits=logits, partial=partial,
                params=params, prjl2=prjl2, col_best=col_best.astype(np.float32), tie=tie)


def decide_reference(c, focus, mutation=None):
    """The float64 decision of a case, with the margins of its inputs: gap [B] (top-2 logit gap), p_margin [B] = |p1 - P_THRESH| (inf
    for untargeted samples), d_margin [B] = |caml2 * 255 - d_thr| of the sample's group."""
    HW = c['HW']
    pt = c['partial'].astype(np.float64)
    ref = uo.decide_universal(c['logits'], c['target'], c['targeted'], pt[:, :, 0].sum(axis=1) / HW, pt[:, :, 1].sum(axis=1) / HW,
                              c['params'][:, :3], c['params'][:, 3], P_THRESH, focus, c['N'], c['need'], prjl2=c['prjl2'],
                              col_best=c['col_best'], mutation=mutation)
    top2 = np.sort(c['logits'].astype(np.float64), axis=1)[:, -2:]
    ref['gap'] = top2[:, 1] - top2[:, 0]
    ref['p_margin'] = np.where(c['targeted'], np.abs(ref['p1'] - P_THRESH), np.inf)
    ref['d_margin'] = np.abs(ref['caml2'] * 255.0 - c['params'][:, 3].astype(np.float64))
    return ref


def decide_differs(ref, other):
    """Whether two decisions differ by more than the tolerances of the comparison with the kernel: a flag, a count or a weight, or a
    value beyond rtol 1e-4."""
    flags = ('uni_state', 'uni_w', 'state_succ', 'best_adv', 'best', 'nfooled')
    values = ('p_min', 'tl_mean', 'caml2', 'camdE', 'col', 'prjl2', 'col_best_after')
    return (any(not np.array_equal(ref[k], other[k]) for k in flags) or
            any(not np.allclose(other[k], ref[k], rtol=1e-4, atol=1e-12) for k in values))


COMBINE_HW = [1, 255, 256, 257, 3120]
COMBINE_N = [2, 3, 8, 64]


def combine_case(N, HW, seed):
    """U = 3 groups in one launch: group 0 on the adversarial step with member 1 all zero and weights 1, group 1 on the colour step,
    group 2 on the adversarial step with member 0's weight 0 and the other weights unequal.  The members' magnitudes differ by decades;
    the inputs' pad channel holds garbage.  Returns g [B][HW][4], w [B], state [B][4]."""
    rng = np.random.default_rng(seed)
    B = 3 * N
    g = (rng.standard_normal((B, HW, 4)) * 10.0 ** rng.uniform(-6, -3, (B, 1, 1))).astype(np.float32)
    g[1, :, :3] = 0.0
    w = rng.uniform(0.5, 1.5, B).astype(np.float32)
    w[:N] = 1.0
    w[2 * N] = 0.0
    state = np.zeros((B, 4), dtype=np.int32)
    state[N:2 * N, 1] = 1
    state[:, 0] = np.arange(B) % 2          # (succ does not choose the rule)
    return g, w, state
