"""Float64 restatements of the multi-view attack ("Multi-view attack"), for the multi-view tests: the decision over V
views' logits and stealth losses (`decide_views`), the combination of the views' gradient images at the projector (`combine_views`),
and one whole first iteration built from the oracle's PCNet, its classifier and autograd (`first_iteration`).  The per-view rows, the
`focus` rule and the unit images are the ensemble's (tests/ensemble_oracle.py): a view is decided as a member is.  A helper, not a
test module."""
import numpy as np
import torch

import ensemble_oracle as eo
import spaa_oracle as so


def loss_weights(stealth_loss):
    """(prjl2_w, caml2_w, camdE_w) of a stealth-loss string, as oracle.spaa_oracle.spaa reads it."""
    return (0.1 if 'prjl2' in stealth_loss else 0.0, 1.0 if 'caml2' in stealth_loss else 0.0, 1.0 if 'camdE' in stealth_loss else 0.0)


def decide_views(logits, target, targeted, caml2_v, camdE_v, weights, d_thr, p_thresh, focus, prjl2=None, col_best=None):
    """The decision over views.  `logits`: V arrays [B][ncls]; caml2_v, camdE_v [B][V]: each view's stealth-loss means; `weights`
    [B][3] = (prjl2_w, caml2_w, camdE_w) per sample; target, targeted, d_thr per sample; prjl2 [B] or None; `col_best`: the colour
    loss's best so far (None: `best` is not computed).  Returns a dict: the view tables top1, p1, tl, succ, fooled [B][V], view_state
    [B][V][2], view_stats [B][V][4], view_w [B][V]; per sample state_succ, best_adv, best, nfooled (the four columns of `state`),
    p_min (stats 0), caml2, camdE, col, prjl2 (stats 1..4), col_best_after (stats 5), tl_mean (stats 6)."""
    V = len(logits)
    rows = [eo.member_rows(lg, target, targeted, p_thresh) for lg in logits]
    top1, p1, tl, succ, fooled = (np.stack([r[i] for r in rows], axis=1) for i in range(5))
    caml2_v, camdE_v = np.asarray(caml2_v, dtype=np.float64), np.asarray(camdE_v, dtype=np.float64)
    assert caml2_v.shape == camdE_v.shape == p1.shape
    caml2, camdE = caml2_v.sum(axis=1) / V, camdE_v.sum(axis=1) / V
    w = np.asarray(weights, dtype=np.float64)
    pl2 = np.zeros(len(caml2)) if prjl2 is None else np.where(w[:, 0] != 0, np.asarray(prjl2, dtype=np.float64), 0.0)
    col = w[:, 0] * pl2 + w[:, 1] * caml2 + w[:, 2] * camdE
    high_pert = caml2 * 255.0 > np.asarray(d_thr, dtype=np.float64)
    best_adv = fooled.all(axis=1) & high_pert
    out = dict(top1=top1, p1=p1, tl=tl, succ=succ, fooled=fooled, high_pert=high_pert,
               view_state=np.stack([succ.astype(np.int64) | (fooled.astype(np.int64) << 1), top1], axis=2),
               view_stats=np.stack([p1, tl, caml2_v, camdE_v], axis=2), view_w=eo.focus_weights(fooled, focus),
               state_succ=succ.all(axis=1), best_adv=best_adv, nfooled=fooled.sum(axis=1), p_min=p1.min(axis=1),
               tl_mean=tl.mean(axis=1), caml2=caml2, camdE=camdE, col=col, prjl2=pl2)
    if col_best is not None:
        col_best = np.asarray(col_best, dtype=np.float64)
        out['best'] = best_adv & (col < col_best)
        out['col_best_after'] = np.where(out['best'], col, col_best)
    return out


def combine_views(gs, w, col_step):
    """The V gradient images at the projector as one, [B][HW][4] float64 with the fourth channel 0: for a sample with `col_step` the
    mean over views (sum_v g_v) / V, for any other sum_v w[b][v] * g_bv / ||g_bv||_2 (a view with zero norm contributes 0).
    `gs`: V arrays [B][HW][3 or 4]."""
    w, col_step = np.asarray(w, dtype=np.float64), np.asarray(col_step, dtype=bool)
    gs = [np.asarray(g, dtype=np.float64)[..., :3] for g in gs]
    adv, col = np.zeros(gs[0].shape), np.zeros(gs[0].shape)
    for v, g in enumerate(gs):
        adv += w[:, v, None, None] * eo.unit_images(g)[0]
        col += g
    out = np.zeros(gs[0].shape[:2] + (4,))
    out[..., :3] = np.where(col_step[:, None, None], col / len(gs), adv)
    return out


def first_iteration(pcnet_sds, oracle_classifier, target, targeted, cam_scenes, d_thr, stealth_loss, setup_info, p_thresh=0.9,
                    focus=False, adv_lr=2, col_lr=1, dtype=torch.float64):
    """The first iteration from the grey projector image x, in `dtype` on the CPU: per view v  y_v = PCNet_v(clamp(x), s_v), the one
    classifier's logits on y_v, the gradient images at the PROJECTOR  g_adv_v = d(-/+ logit_v[b, target_b] / B) / dx  and
    g_col_v = d((caml2_w caml2_v + camdE_w camdE_v)_b / B) / dx; the decision, the combined gradient (with the prjl2 term's gradient
    added on the colour step) and the normalised step.  target / targeted / d_thr: one per sample; `stealth_loss`: one string or one
    per sample.  Returns decide_views's dict plus cams [V] of [B,3,H,W], g [V][B][HW][3] (per sample the gradient its step uses: g_col_v
    where best_adv, else g_adv_v), g_out [B][HW][4], x_next [B,3,Hp,Wp], and the margins the comparison with an fp32 implementation
    needs: gap [B][V] (top-2 logit gap), p_margin [B][V] = |p1 - p_thresh| (inf for untargeted samples, which do not read it),
    d_margin [B] = |caml2 * 255 - d_thr|."""
    B, V = len(target), len(pcnet_sds)
    losses = [stealth_loss] * B if isinstance(stealth_loss, str) else list(stealth_loss)
    weights = np.array([loss_weights(s) for s in losses])
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
        logits, cams, g_adv, g_col, caml2_v, camdE_v = [], [], [], [], [], []
        flat = lambda g: g.permute(0, 2, 3, 1).reshape(B, -1, 3).numpy().astype(np.float64)           # noqa: E731
        for sd, scene in zip(pcnet_sds, cam_scenes):
            scene = so.expand_4d(scene.to(dtype)).expand(B, -1, -1, -1)
            y = so.pcnet_forward(cast(sd), x.clamp(0, 1), scene)
            raw = clf(y, setup_info['classifier_crop_sz'])[0]
            caml2 = torch.norm(scene - y, dim=1).mean(1).mean(1)
            camdE = so.ciede2000_diff(so.rgb2lab_diff(y), so.rgb2lab_diff(scene)).mean(1).mean(1)
            ga, = torch.autograd.grad((sign * raw[idx, torch.as_tensor(list(target))]).sum() / B, x, retain_graph=True)
            gc, = torch.autograd.grad((wt[:, 1] * caml2 + wt[:, 2] * camdE).sum() / B, x)
            logits.append(raw.detach().numpy().astype(np.float64))
            cams.append(y.detach())
            g_adv.append(flat(ga))
            g_col.append(flat(gc))
            caml2_v.append(caml2.detach().numpy().astype(np.float64))
            camdE_v.append(camdE.detach().numpy().astype(np.float64))
        prjl2 = torch.norm(gray - x, dim=1).mean(1).mean(1)
        g_pl2, = torch.autograd.grad((wt[:, 0] * prjl2).sum() / B, x)
        g_pl2 = flat(g_pl2)
        prjl2 = prjl2.detach().numpy().astype(np.float64)
    finally:
        torch.set_default_dtype(old)
    caml2_v, camdE_v = np.stack(caml2_v, axis=1), np.stack(camdE_v, axis=1)
    out = decide_views(logits, target, targeted, caml2_v, camdE_v, weights, d_thr, p_thresh, focus, prjl2=prjl2,
                       col_best=np.full(B, 1e6))
    col_step = out['best_adv']
    gs = [np.where(col_step[:, None, None], gc, ga) for ga, gc in zip(g_adv, g_col)]
    g_out = combine_views(gs, out['view_w'], col_step)
    g_out[..., :3] += np.where(col_step[:, None, None], g_pl2, 0.0)
    unit, _ = eo.unit_images(g_out)
    lr = np.where(col_step, float(col_lr), float(adv_lr))
    Hp, Wp = setup_info['prj_im_sz']
    step = torch.from_numpy((lr[:, None, None] * unit).reshape(B, Hp, Wp, 3)).permute(0, 3, 1, 2)
    top2 = [np.sort(lg, axis=1)[:, -2:] for lg in logits]
    out.update(cams=cams, logits=logits, g=gs, g_out=g_out, x_next=gray.to(torch.float64) - step,
               gap=np.stack([t[:, 1] - t[:, 0] for t in top2], axis=1),
               p_margin=np.where(np.asarray(targeted, dtype=bool)[:, None], np.abs(out['p1'] - p_thresh), np.inf),
               d_margin=np.abs(out['caml2'] * 255.0 - np.asarray(d_thr, dtype=np.float64)))
    return out
