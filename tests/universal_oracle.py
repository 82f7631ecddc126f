"""Float64 restatements of the universal attack, for the universal tests: the decision over groups of N consecutive
samples (`decide_universal`), the combination of a group's gradient images at the projector (`combine_universal`) with the bar an fp32
implementation of it has to keep (`combine_bar`), and one whole first iteration built from the oracle's PCNet, its classifier and
autograd (`first_iteration`).  The member rows, the `focus` rule and the unit images are the ensemble's (tests/ensemble_oracle.py): a
member of a group is decided as a member of an ensemble is.  `MUTATIONS` names deliberate mistakes that both functions can be asked to
make, one at a time: the tests show that each of them is seen.  A helper, not a test module."""
import math

import numpy as np
import torch

import ensemble_oracle as eo
import multiview_oracle as mo
import spaa_oracle as so

MUTATIONS = ('need_is_n',            # `need` read as N: the rate is ignored
             'mean_over_need',       # the group's caml2 / camdE divided by `need` instead of N
             'prjl2_summed',         # prjl2 summed over the members instead of member 0's (x is shared)
             'focus_rests_fooled',   # focus keeps resting the fooled members of a group that is already fooled
             'unit_on_colour',       # unit images on the colour step
             'mean_on_adv',          # the plain mean on the adversarial step
             'boundary_off_by_one',  # group u taken as the samples uN+1 .. uN+N
             'order_reversed')       # member i weighted with member N-1-i's weight


def need_of(N, rate):
    """ceil(rate * N), a product that is an integer but for its rounding being that integer; 1 .. N."""
    return min(N, max(1, int(math.ceil(float(rate) * N - 1e-9))))


def _groups(a, N):
    a = np.asarray(a)
    return a.reshape((a.shape[0] // N, N) + a.shape[1:])


def _rows(a, N):
    """A per-group array [U][...] as one row per sample [U N][...]."""
    return np.repeat(np.asarray(a), N, axis=0)


def decide_universal(logits, target, targeted, caml2_b, camdE_b, weights, d_thr, p_thresh, focus, N, need, prjl2=None, col_best=None,
                     mutation=None):
    """The decision over groups: sample b = member b % N of group b // N.  `logits` [B][ncls]; target, targeted, d_thr per sample
    (targeted, d_thr and `weights` [B][3] = (prjl2_w, caml2_w, camdE_w) uniform within a group); caml2_b, camdE_b [B]: each sample's own
    stealth-loss means; prjl2 [B] or None; `col_best` [B]: the colour loss's best so far (None: `best` is not computed).  Returns a dict.
    Per sample: top1, p1, tl, succ, fooled, uni_state [B][2], uni_stats [B][4], uni_w.  The group's values, one ROW PER SAMPLE as the
    kernel writes them: state_succ, best_adv, best, nfooled (the four columns of `state`), p_min (stats 0), caml2, camdE, col, prjl2
    (stats 1..4), col_best_after (stats 5), tl_mean (stats 6), and nsucc, group_fooled, high_pert."""
    assert mutation is None or mutation in MUTATIONS
    lg = np.asarray(logits, dtype=np.float64)
    B = lg.shape[0]
    assert B % N == 0 and 1 <= need <= N
    if mutation == 'need_is_n':
        need = N
    top1, p1, tl, succ, fooled = eo.member_rows(lg, target, targeted, p_thresh)
    caml2_b, camdE_b = np.asarray(caml2_b, dtype=np.float64), np.asarray(camdE_b, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    d_thr = np.asarray(d_thr, dtype=np.float64)
    for per_sample in (np.asarray(targeted, dtype=bool), d_thr, w):
        g = _groups(per_sample, N)
        assert (g == g[:, :1]).all(), 'targeted, d_thr and the loss weights are uniform within a group'
    pl2_b = np.zeros(B) if prjl2 is None else np.where(w[:, 0] != 0, np.asarray(prjl2, dtype=np.float64), 0.0)

    def grouped(a):
        a = np.asarray(a)
        if mutation == 'boundary_off_by_one':
            a = np.roll(a, -1, axis=0)
        return _groups(a, N)

    succ_g, fooled_g = grouped(succ), grouped(fooled)
    nsucc, nfooled = succ_g.sum(axis=1), fooled_g.sum(axis=1)
    div = need if mutation == 'mean_over_need' else N
    caml2, camdE = grouped(caml2_b).sum(axis=1) / div, grouped(camdE_b).sum(axis=1) / div
    pl2 = _groups(pl2_b, N).sum(axis=1) if mutation == 'prjl2_summed' else _groups(pl2_b, N)[:, 0]
    wg = _groups(w, N)[:, 0]
    col = wg[:, 0] * pl2 + wg[:, 1] * caml2 + wg[:, 2] * camdE
    high_pert = caml2 * 255.0 > _groups(d_thr, N)[:, 0]
    group_succ, group_fooled = nsucc >= need, nfooled >= need
    best_adv = group_fooled & high_pert
    # the weights: the ensemble's rule per group (a fooled member rests unless all are), and nobody rests once the group is fooled
    fooled_own = _groups(fooled, N)
    uni_w = eo.focus_weights(fooled_own, focus)
    if focus and mutation != 'focus_rests_fooled':
        own_group_fooled = fooled_own.sum(axis=1) >= need
        uni_w = np.where(own_group_fooled[:, None], 1.0, np.where(fooled_own, 0.0, 1.0))
    out = dict(top1=top1, p1=p1, tl=tl, succ=succ, fooled=fooled,
               uni_state=np.stack([succ.astype(np.int64) | (fooled.astype(np.int64) << 1), top1], axis=1),
               uni_stats=np.stack([p1, tl, caml2_b, camdE_b], axis=1), uni_w=uni_w.reshape(B),
               state_succ=_rows(group_succ, N), group_fooled=_rows(group_fooled, N), high_pert=_rows(high_pert, N),
               best_adv=_rows(best_adv, N), nsucc=_rows(nsucc, N), nfooled=_rows(nfooled, N), p_min=_rows(grouped(p1).min(axis=1), N),
               tl_mean=_rows(grouped(tl).mean(axis=1), N), caml2=_rows(caml2, N), camdE=_rows(camdE, N), col=_rows(col, N),
               prjl2=_rows(pl2, N))
    if col_best is not None:
        cb = _groups(np.asarray(col_best, dtype=np.float64), N)[:, 0]
        best = best_adv & (col < cb)
        out['best'] = _rows(best, N)
        out['col_best_after'] = _rows(np.where(best, col, cb), N)
    return out


def combine_universal(g, w, col_step, N, mutation=None):
    """The B gradient images at the projector combined group by group: ([B][HW][4] float64 with the fourth channel 0 and a group's N
    rows equal, the sum of the terms' magnitudes [B][HW][3]).  A group whose first row has `col_step`: (sum_i g_i) / N; any other:
    sum_i w_i g_i / ||g_i||_2 (a member with zero norm contributes 0).  `g` [B][HW][3 or 4], `w` [B], `col_step` [B]."""
    assert mutation is None or mutation in MUTATIONS
    g = np.asarray(g, dtype=np.float64)[..., :3]
    w, col_step = np.asarray(w, dtype=np.float64), np.asarray(col_step, dtype=bool)
    B = g.shape[0]
    assert B % N == 0
    col_g = _groups(col_step, N)[:, 0]
    if mutation == 'boundary_off_by_one':
        g, w = np.roll(g, -1, axis=0), np.roll(w, -1, axis=0)
    if mutation == 'order_reversed':
        w = _groups(w, N)[:, ::-1].reshape(B)
    adv_terms = _groups(w[:, None, None] * eo.unit_images(g)[0], N)                  # [U][N][HW][3]
    col_terms = _groups(g, N)
    take_col = col_g
    if mutation == 'unit_on_colour':
        take_col = np.zeros_like(col_g)
    if mutation == 'mean_on_adv':
        take_col = np.ones_like(col_g)
    adv, col = np.zeros(adv_terms.shape[:1] + adv_terms.shape[2:]), np.zeros(adv_terms.shape[:1] + adv_terms.shape[2:])
    for i in range(N):                                                               # (in index order, as combine_views)
        adv += adv_terms[:, i]
        col += col_terms[:, i]
    pick = take_col[:, None, None]
    out = np.zeros((B,) + g.shape[1:2] + (4,))
    out[..., :3] = _rows(np.where(pick, col / N, adv), N)
    return out, _rows(np.where(pick, np.abs(col_terms).sum(axis=1) / N, np.abs(adv_terms).sum(axis=1)), N)


def combine_bar(N, HW):
    """What an fp32 combination that follows the stated order may be off by, relative to the sum of its terms' magnitudes, u = 2^-24
    the unit roundoff.  ||g_b||^2: a sum of positive terms, so its relative error is at most u times the depth of its additions -- a
    pixel's three products and two additions (3), six shuffle levels and the three additions of the four wave sums (9), the
    ceil(nblk / 256) partial sums a thread of the reducing workgroup adds, and that workgroup's own nine: (21 + ceil(nblk / 256)) u.  The
    square root halves it; the root and the division are allowed 3 u each (correctly rounded ones take half a u).  A term coef_i * g_i
    adds one rounding and the N - 1 additions in index order at most one each, every one of them bounded by u times the sum of the
    magnitudes.  The colour step (N - 1 additions, 1 / N and the product with it) stays below that."""
    nblk = (HW + 255) // 256
    per_thread = (nblk + 255) // 256
    coef = (21 + per_thread) / 2.0 + 3 + 3
    return (coef + 1 + (N - 1)) * 2.0 ** -24


def first_iteration(pcnet_sd, oracle_classifier, target, targeted, cam_scenes, d_thr, stealth_loss, setup_info, N, need, p_thresh=0.9,
                    focus=False, adv_lr=2, col_lr=1, dtype=torch.float64):
    """The first iteration from the grey projector image x, in `dtype` on the CPU: ONE PCNet and B scenes `cam_scenes` [B,3,H,W];
    y_b = PCNet(clamp(x), s_b), the classifier's logits on y_b and, as multiview_oracle.first_iteration does per view, the gradient
    images at the PROJECTOR  g_adv_b = d(-/+ logit[b, target_b] / B) / dx  and  g_col_b = d((caml2_w caml2_b + camdE_w camdE_b) / B) / dx
    (samples do not interact: row b of a batch gradient is sample b's own); the decision over groups of N, the combined gradient (with
    the prjl2 term's gradient added on the colour step) and the normalised step.  target / targeted / d_thr: one per sample;
    `stealth_loss`: one string or one per sample.  Returns decide_universal's dict plus cam [B,3,H,W], logits, g [B][HW][3] (per sample
    the gradient its group's step uses: g_col_b where best_adv, else g_adv_b), g_out [B][HW][4], x_next [B,3,Hp,Wp], and the margins
    the comparison with an fp32 implementation needs: gap [B] (top-2 logit gap), p_margin [B] = |p1 - p_thresh| (inf for untargeted
    samples, which do not read it), d_margin [B] = |caml2 * 255 - d_thr| of the sample's group."""
    B = len(target)
    losses = [stealth_loss] * B if isinstance(stealth_loss, str) else list(stealth_loss)
    weights = np.array([mo.loss_weights(s) for s in losses])
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        cast = lambda sd: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}   # noqa: E731
        c = oracle_classifier
        clf = so.OracleClassifier(c.name, cast(c.sd), sort_results=c.sort_results, input_sz=c.input_sz)
        wt = torch.tensor(weights)
        gray = torch.full((B, 3) + tuple(setup_info['prj_im_sz']), float(setup_info['prj_brightness']))
        x = gray.clone().requires_grad_(True)
        sign = torch.tensor([-1.0 if t else 1.0 for t in targeted])
        idx = torch.arange(B)
        flat = lambda g: g.permute(0, 2, 3, 1).reshape(B, -1, 3).numpy().astype(np.float64)           # noqa: E731
        scene = cam_scenes.to(dtype)
        assert scene.ndim == 4 and scene.shape[0] == B
        y = so.pcnet_forward(cast(pcnet_sd), x.clamp(0, 1), scene)
        raw = clf(y, setup_info['classifier_crop_sz'])[0]
        caml2 = torch.norm(scene - y, dim=1).mean(1).mean(1)
        camdE = so.ciede2000_diff(so.rgb2lab_diff(y), so.rgb2lab_diff(scene)).mean(1).mean(1)
        ga, = torch.autograd.grad((sign * raw[idx, torch.as_tensor(list(target))]).sum() / B, x, retain_graph=True)
        gc, = torch.autograd.grad((wt[:, 1] * caml2 + wt[:, 2] * camdE).sum() / B, x)
        prjl2 = torch.norm(gray - x, dim=1).mean(1).mean(1)
        g_pl2, = torch.autograd.grad((wt[:, 0] * prjl2).sum() / B, x)
        logits = raw.detach().numpy().astype(np.float64)
        ga, gc, g_pl2 = flat(ga), flat(gc), flat(g_pl2)
        caml2, camdE = caml2.detach().numpy().astype(np.float64), camdE.detach().numpy().astype(np.float64)
        prjl2 = prjl2.detach().numpy().astype(np.float64)
    finally:
        torch.set_default_dtype(old)
    out = decide_universal(logits, target, targeted, caml2, camdE, weights, d_thr, p_thresh, focus, N, need, prjl2=prjl2,
                           col_best=np.full(B, 1e6))
    col_step = out['best_adv']
    gs = np.where(col_step[:, None, None], gc, ga)
    g_out, _ = combine_universal(gs, out['uni_w'], col_step, N)
    g_out[..., :3] += np.where(col_step[:, None, None], g_pl2, 0.0)
    unit, _ = eo.unit_images(g_out)
    lr = np.where(col_step, float(col_lr), float(adv_lr))
    Hp, Wp = setup_info['prj_im_sz']
    step = torch.from_numpy((lr[:, None, None] * unit).reshape(B, Hp, Wp, 3)).permute(0, 3, 1, 2)
    top2 = np.sort(logits, axis=1)[:, -2:]
    out.update(cam=y.detach(), logits=logits, g=gs, g_out=g_out, x_next=gray.to(torch.float64) - step, gap=top2[:, 1] - top2[:, 0],
               p_margin=np.where(np.asarray(targeted, dtype=bool), np.abs(out['p1'] - p_thresh), np.inf),
               d_margin=np.abs(out['caml2'] * 255.0 - np.asarray(d_thr, dtype=np.float64)))
    return out
