"""Float64 restatements of the ensemble attack ("Ensemble attack"), for the ensemble tests: the decision over K members'
logits (`decide_ens`), the weighted sum of the members' unit gradient images (`combine`), and one whole first iteration built from the
oracle's PCNet, its classifiers and autograd (`first_iteration`).  A helper, not a test module."""
import numpy as np
import torch

import spaa_oracle as so


def member_rows(logits, target, targeted, p_thresh):
    """One member: logits [B][ncls] -> (top1 (first maximum), p1 = softmax top-1, target logit, succ, fooled), float64 / bool [B]."""
    lg = np.asarray(logits, dtype=np.float64)
    target, targeted = np.asarray(target), np.asarray(targeted, dtype=bool)
    top1 = lg.argmax(axis=1)                                    # (numpy: the first of equal maxima)
    p1 = 1.0 / np.exp(lg - lg.max(axis=1, keepdims=True)).sum(axis=1)
    tl = lg[np.arange(lg.shape[0]), target]
    succ = np.where(targeted, top1 == target, top1 != target)
    fooled = np.where(targeted, succ & (p1 > p_thresh), succ)
    return top1, p1, tl, succ, fooled


def focus_weights(fooled, focus):
    """Member weights a [B][K] from the fooled flags [B][K]: 1; with `focus`, 0 for a fooled member unless every member is fooled."""
    fooled = np.asarray(fooled, dtype=bool)
    if not focus:
        return np.ones(fooled.shape)
    return np.where(fooled & ~fooled.all(axis=1, keepdims=True), 0.0, 1.0)


def decide_ens(logits, target, targeted, caml2, d_thr, p_thresh, focus, col=None, col_best=None):
    """The ensemble decision.  `logits`: K arrays [B][ncls]; target, targeted, caml2, d_thr: per sample; `col` / `col_best`: the
    colour loss and its best so far (None: `best` is not computed).  Returns a dict: the member tables top1, p1, tl, succ, fooled
    [B][K], ens_state [B][K][2], ens_w [B][K], and per sample succ, best_adv, best, nfooled (the four columns of `state`),
    p_min (stats 0), tl_mean (stats 6)."""
    rows = [member_rows(lg, target, targeted, p_thresh) for lg in logits]
    top1, p1, tl, succ, fooled = (np.stack([r[i] for r in rows], axis=1) for i in range(5))
    high_pert = np.asarray(caml2, dtype=np.float64) * 255.0 > np.asarray(d_thr, dtype=np.float64)
    best_adv = fooled.all(axis=1) & high_pert
    out = dict(top1=top1, p1=p1, tl=tl, succ=succ, fooled=fooled, high_pert=high_pert,
               ens_state=np.stack([succ.astype(np.int64) | (fooled.astype(np.int64) << 1), top1], axis=2),
               ens_w=focus_weights(fooled, focus), state_succ=succ.all(axis=1), best_adv=best_adv, nfooled=fooled.sum(axis=1),
               p_min=p1.min(axis=1), tl_mean=tl.mean(axis=1))
    if col is not None:
        out['best'] = best_adv & (np.asarray(col, dtype=np.float64) < np.asarray(col_best, dtype=np.float64))
    return out


def unit_images(g):
    """g [B][HW][>=3] -> (g / ||g||_2 over the three colour channels of all pixels, 0 where the norm is 0) [B][HW][3], norms [B]."""
    g = np.asarray(g, dtype=np.float64)[..., :3]
    n = np.sqrt((g * g).sum(axis=(1, 2)))
    return np.where(n[:, None, None] > 0, g / np.where(n > 0, n, 1.0)[:, None, None], 0.0), n


def combine(gs, w):
    """sum_k w[b][k] * g_bk / ||g_bk||_2 -> [B][HW][4] float64 with the fourth channel 0.  `gs`: K arrays [B][HW][3 or 4]."""
    w = np.asarray(w, dtype=np.float64)
    units = [unit_images(g)[0] for g in gs]
    out = np.zeros(units[0].shape[:2] + (4,))
    for k, u in enumerate(units):
        out[..., :3] += w[:, k, None, None] * u
    return out


def first_iteration(pcnet_sd, oracle_classifiers, target, targeted, cam_scene, d_thr, setup_info, p_thresh=0.9, focus=False,
                    dtype=torch.float64):
    """The first iteration's forward pass and adversarial direction from the grey projector image, in `dtype` on the CPU:
    y = PCNet(clamp(x), s), the K members' logits and their gradient images g_bk = d(-/+ logit_k[b, target_b]) / dy, the decision and
    g_adv.  target / targeted / d_thr: one per sample.  Returns decide_ens's dict plus cam [B,3,H,W], caml2 [B], g [K][B][HW][3],
    g_adv [B][HW][4], and the margins the comparison with an fp32 implementation needs: gap [B][K] (top-2 logit gap),
    p_margin [B][K] = |p1 - p_thresh| (inf for untargeted samples, which do not read it), d_margin [B] = |caml2 * 255 - d_thr|."""
    B = len(target)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        cast = lambda sd: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}   # noqa: E731
        sd = cast(pcnet_sd)
        clfs = [so.OracleClassifier(c.name, cast(c.sd), sort_results=c.sort_results, input_sz=c.input_sz) for c in oracle_classifiers]
        scene = so.expand_4d(cam_scene.to(dtype)).expand(B, -1, -1, -1)
        x = torch.full((B, 3) + tuple(setup_info['prj_im_sz']), float(setup_info['prj_brightness']))
        with torch.no_grad():
            y = so.pcnet_forward(sd, x.clamp(0, 1), scene)
        y = y.detach().requires_grad_(True)
        sign = torch.tensor([-1.0 if t else 1.0 for t in targeted])
        idx = torch.arange(B)
        logits, gs = [], []
        for c in clfs:
            raw = c(y, setup_info['classifier_crop_sz'])[0]
            g, = torch.autograd.grad((sign * raw[idx, torch.as_tensor(list(target))]).sum(), y)
            logits.append(raw.detach().numpy().astype(np.float64))
            gs.append(g.permute(0, 2, 3, 1).reshape(B, -1, 3).numpy().astype(np.float64))
        caml2 = torch.norm(scene - y.detach(), dim=1).mean(1).mean(1).numpy().astype(np.float64)
    finally:
        torch.set_default_dtype(old)
    out = decide_ens(logits, target, targeted, caml2, d_thr, p_thresh, focus)
    top2 = [np.sort(lg, axis=1)[:, -2:] for lg in logits]
    out.update(cam=y.detach(), caml2=caml2, g=gs, g_adv=combine(gs, out['ens_w']), logits=logits,
               gap=np.stack([t[:, 1] - t[:, 0] for t in top2], axis=1),
               p_margin=np.where(np.asarray(targeted, dtype=bool)[:, None], np.abs(out['p1'] - p_thresh), np.inf),
               d_margin=np.abs(caml2 * 255.0 - np.asarray(d_thr, dtype=np.float64)))
    return out
