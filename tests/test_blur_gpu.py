"""GPU: the blur attack loop (BlurAttackState through spaa / spaa_sweep) on the 64 x 64 synthetic PCNet and the 56 x 56 ResNet-18 of
tests/test_jitter_gpu.py.  One first iteration against an oracle composition that is teacher-forced with the state's own camera image:
the sigma rows, the draw images, the per-draw logits and the decision from them, the pulled-back gradients and their combination.  Blur
in front of the jitter and behind the pose warp with the codec last, the later stages teacher-forced with the state's own blur images
through their own oracles; the eager / graph / repeat / sweep identities; gaussian_blur against spaa_blur_fwd; blur_survival.  Every
test prints its largest error over the bar as an `accuracy:` line (profiles/blur_accuracy.txt holds the lines of one run)."""
import numpy as np
import pytest
import torch

import blur_oracle as bo
import ensemble_oracle as eo
import jitter_oracle as jo
import pose_oracle as po
from test_gpu_parity import hip, make_pcnet  # noqa: F401  (hip: module fixture)
from test_jitter_gpu import (csd, clf, pcnet, case, DEV, SZ, SETUP, LOSS, P_THRESH, TARGETED, D_THR,  # noqa: F401  (fixtures)
                             UNTARGETED_OTHER)
from test_jpeg_gpu import _oracle_draws, _check_pullback, _logits
from test_pose_gpu import BWD_BAR

pytestmark = pytest.mark.gpu
CROP = SETUP['classifier_crop_sz']
F32 = np.float32


def _check_rows(rows, seed, t, B, J, lo, hi):
    """The state's rows against the rule: sigma within its bar of the integer rule's, r exactly and the taps within theirs of the
    oracle's row of the kernel's own sigma.  Returns (largest sigma error / bar, largest tap error / bar)."""
    rows = np.asarray(rows, dtype=np.float64)
    want = bo.draw_sigmas(seed, t, B, J, lo, hi, True)
    over_s = float(np.abs(rows[..., 0] - want).max() / bo.bar_sigma(lo, hi))
    over_t = 0.0
    for row in rows.reshape(-1, bo.ROW):
        ref, bar = bo.row_of(F32(row[0])), bo.bar_row(F32(row[0]))
        assert row[1] == ref[1] and row[11] == 0
        if ref[1] == 0:
            assert np.array_equal(row, ref)
            continue
        taps = slice(2, 3 + int(ref[1]))
        over_t = max(over_t, float((np.abs(row - ref)[taps] / bar[taps]).max()))
    assert (rows[:, 0, :3] == [0, 0, 1]).all()
    return over_s, over_t


def _oracle_blur(ims_in, rows, ims_gpu):
    """Per draw j the float64 blur of the J input batches `ims_in` [J][B][H][W][>= 3] with the taps of the state's own sigmas: (the
    oracle's images as fp32 [J][B][H][W][3], the largest |kernel - float64| / bar over every pixel)."""
    J, B = len(ims_in), ims_in[0].shape[0]
    out = np.zeros((J, B) + SZ + (3,), dtype=F32)
    worst = 0.0
    for j in range(J):
        for b in range(B):
            sigma = F32(rows[b, j, 0])
            r, w = bo.taps(sigma)
            x = ims_in[j][b][..., :3].astype(np.float64)
            got = ims_gpu[j][b, ..., :3]
            if r == 0:
                assert np.array_equal(got, ims_in[j][b][..., :3])
                out[j, b] = got
                continue
            want = bo.forward(x, r, w)
            worst = max(worst, float((np.abs(got - want) / bo.bar_forward(x, r, w, bo.tap_ulps(sigma))).max()))
            out[j, b] = want.astype(F32)
    return out, worst


def _blur_pullback(st, g_in, rows):
    """st.blur_grads against the float64 transpose of the gradient images `g_in` [J][B][H][W][4]: largest error over the bar."""
    worst = 0.0
    for j in range(st.K):
        got = st.blur_grads[j].cpu().numpy().astype(np.float64)
        assert (got[..., 3] == 0).all()
        for b in range(st.B):
            sigma = F32(rows[b, j, 0])
            r, w = bo.taps(sigma)
            g = g_in[j][b, ..., :3].astype(np.float64)
            if r == 0:
                assert np.array_equal(got[b, ..., :3], g)
                continue
            worst = max(worst, float((np.abs(got[b, ..., :3] - bo.backward(g, r, w)) / bo.bar_backward(g, r, w, bo.tap_ulps(sigma))).max()))
    return worst


def _check_combination(st, last):
    B = st.B
    own = eo.combine([g.reshape(B, -1, 4).cpu().numpy().astype(np.float64) for g in last], st.ens_w.cpu().numpy())
    g_adv = st.g_adv.reshape(B, -1, 4).cpu().numpy().astype(np.float64)
    err = np.abs(g_adv - own).max(axis=(1, 2)) / np.abs(own).max(axis=(1, 2))
    assert (err <= 2e-6).all() and (g_adv[..., 3] == 0).all(), err
    return float(err.max())


def test_first_iteration_against_the_oracle(hip, pcnet, clf, case):
    A = hip['attack']
    sd, scene, oc, targets = case
    J, B = 3, 4
    bl = A.CaptureBlur(sigma=(0.5, 2.0), draws=J, seed=11)
    st = A.BlurAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, bl)
    assert st.K == J and len({id(e) for e in st.clfs}) == J and [type(s).__name__ for s in st.stages] == ['BlurStage']
    st.forward_decide(TARGETED, D_THR, P_THRESH)
    st.backward_step(2, 1)
    rows = st.blur_rows.cpu().numpy()
    assert int(st.counter.item()) == 1
    over_s, over_t = _check_rows(rows, 11, 0, B, J, 0.5, 2.0)
    y = st._y.cpu().numpy()
    ims_gpu = [im.cpu().numpy() for im in st.blur_ims]
    ims, over_f = _oracle_blur([y] * J, rows, ims_gpu)
    assert np.array_equal(ims_gpu[0][..., :3], y[..., :3]) and all((im[..., 3] == 0).all() for im in ims_gpu)
    # per-draw logits: the product classifier on the oracle's images, and the decision from them
    logits = [_logits(clf, ims[j]) for j in range(J)]
    scene_b = scene.reshape(1, 3, *SZ).permute(0, 2, 3, 1).double().numpy()
    caml2 = np.sqrt(((scene_b - y[..., :3].astype(np.float64)) ** 2).sum(axis=-1)).mean(axis=(1, 2))
    ref = eo.decide_ens(logits, targets, TARGETED, caml2, D_THR, P_THRESH, False)
    top2 = [np.sort(lg, axis=1)[:, -2:] for lg in logits]
    gap = np.stack([t[:, 1] - t[:, 0] for t in top2], axis=1)
    p_margin = np.where(np.asarray(TARGETED)[:, None], np.abs(ref['p1'] - P_THRESH), np.inf)
    clear = (gap > 1e-3) & (p_margin > 1e-3)
    clear_d = np.abs(caml2 * 255.0 - np.asarray(D_THR)) > 1e-3
    assert (~clear).sum() <= 1 and clear_d.all(), 'the case itself is near a tie: choose other seeds'
    es, ef, ew = st.ens_state.cpu().numpy(), st.ens_stats.cpu().numpy().astype(np.float64), st.ens_w.cpu().numpy()
    state, stats = st.state.cpu().numpy(), st.stats.cpu().numpy().astype(np.float64)
    assert (es[clear] == ref['ens_state'][clear]).all(), (es, ref['ens_state'])
    row = clear.all(axis=1)
    assert (state[row, 0] == ref['state_succ'][row]).all() and (state[row, 3] == ref['nfooled'][row]).all()
    assert (state[row, 1] == ref['best_adv'][row]).all() and (ew == 1).all()
    print(f'sigmas {rows[..., 0].tolist()}; max |target logit - ref| {np.abs(ef[..., 1] - ref["tl"]).max():.3e} at max |ref| '
          f'{np.abs(ref["tl"]).max():.3f}')
    assert np.allclose(ef[..., 0][clear], ref['p1'][clear], rtol=1e-3) and np.allclose(ef[..., 1], ref['tl'], rtol=1e-3, atol=1e-3)
    assert np.allclose(stats[:, 1], caml2, rtol=1e-4)                          # the stealth loss is the CLEAN capture's
    # the adjoint's wiring: the pulled-back gradients are spaa_blur_bwd of the engines' own gradient images
    over_b = _blur_pullback(st, [e.g_y.cpu().numpy() for e in st.clfs], rows)
    comb = _check_combination(st, st.blur_grads)
    print(f'accuracy: BlurAttackState first iteration: largest |sigma - rule| / bar = {over_s:.3f}, |tap - float64| / bar = {over_t:.3f}, '
          f'|draw image - float64| / bar = {over_f:.3f}, |pulled-back gradient - float64| / bar = {over_b:.3f}; g_adv against the float64 '
          f'combination {comb:.2e} (bar 2e-6)')
    assert max(over_s, over_t, over_f, over_b) <= 1.0


def test_blur_in_front_of_jitter(hip, pcnet, clf, case):
    """Blur -> Jitter: the jitter reads the blur's images draw by draw (teacher-forced with them, through the jitter oracle), and the
    gradients go back the same way."""
    A = hip['attack']
    _, scene, _, targets = case
    B, J = 4, 3
    bl = A.CaptureBlur(sigma=(0.4, 2.5), draws=J, seed=4)
    jt = A.CaptureJitter(draws=J, seed=5, quantize=False)
    st = A.BlurAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, bl, jitter=jt)
    assert [type(s).__name__ for s in st.stages] == ['BlurStage', 'JitterStage']
    st.forward_decide(TARGETED, D_THR, P_THRESH)
    st.backward_step(2, 1)
    assert int(st.counter.item()) == 1 and int(st.jitter_counter.item()) == 1
    rows = st.blur_rows.cpu().numpy()
    over_s, over_t = _check_rows(rows, 4, 0, B, J, 0.4, 2.5)
    y = st._y.cpu().numpy()
    mid = [im.cpu().numpy() for im in st.blur_ims]
    _, over_f = _oracle_blur([y] * J, rows, mid)
    jit, key = st.jit.cpu().numpy().astype(np.float64), st.key.cpu().numpy().view(np.uint32)
    assert np.array_equal(key, jo.draw_tables(5, 0, B, J, jt.gain, jt.offset, jt.shift, jt.noise, True)[1])
    worst = 0.0
    for j in range(J):
        want = jo.forward(mid[j], jit[:, j:j + 1], key[:, j:j + 1], False)[0][0]
        worst = max(worst, float(np.abs(st.draw_ims[j].cpu().numpy() - want).max()))
    assert worst <= 2e-6, worst                                                 # (the jitter test's bar, its input given)
    g_eng = np.stack([e.g_y.cpu().numpy() for e in st.clfs])
    gates = np.stack([g.cpu().numpy().reshape(B, *SZ) for g in st.draw_gates])
    want = jo.backward(g_eng, jit, gates)
    got = np.stack([g.cpu().numpy() for g in st.draw_grads])
    err = np.abs(got - want).max() / np.abs(want).max()
    assert err <= 2e-6, err
    over_b = _blur_pullback(st, got, rows)
    comb = _check_combination(st, st.blur_grads)
    print(f'accuracy: Blur -> Jitter: largest |sigma - rule| / bar = {over_s:.3f}, |tap - float64| / bar = {over_t:.3f}, |blur image - '
          f'float64| / bar = {over_f:.3f}, |pulled-back gradient - float64| / bar = {over_b:.3f}; jitter behind it {worst:.2e} and its '
          f'adjoint {err:.2e} (bars 2e-6), combination {comb:.2e} (bar 2e-6)')
    assert max(over_s, over_t, over_f, over_b) <= 1.0


def test_blur_behind_pose_with_jpeg_last(hip, pcnet, clf, case):
    """Pose -> Blur -> Jpeg: the blur reads the warp's images, the codec the blur's (teacher-forced with them, through the JPEG oracle and
    its exemptions), and the gradients go back through the three adjoints."""
    A = hip['attack']
    _, scene, _, targets = case
    B, J = 4, 2
    bl = A.CaptureBlur(sigma=(0.5, 1.5), draws=J, seed=8)
    ps = A.PoseJitter(draws=J, seed=6)
    jg = A.JpegCapture(quality=(70, 90), draws=J, seed=4)
    st = A.BlurAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, bl, pose=ps, jpeg=jg)
    assert [type(s).__name__ for s in st.stages] == ['PoseStage', 'BlurStage', 'JpegStage']
    st.forward_decide(TARGETED, D_THR, P_THRESH)
    st.backward_step(2, 1)
    assert int(st.counter.item()) == 1 and int(st.blur_counter.item()) == 1 and int(st.jpeg_counter.item()) == 1
    rows = st.blur_rows.cpu().numpy()
    over_s, over_t = _check_rows(rows, 8, 0, B, J, 0.5, 1.5)
    warped = [im.cpu().numpy() for im in st.pose_ims]
    mid = [im.cpu().numpy() for im in st.blur_ims]
    _, over_f = _oracle_blur(warped, rows, mid)
    qrows = st.jpeg_rows.cpu().numpy()
    ims, fws, taken = _oracle_draws(mid, qrows, '4:2:0', [im.cpu().numpy() for im in st.jpeg_ims])
    tl = np.stack([_logits(clf, ims[j])[np.arange(B), targets] for j in range(J)], axis=1)
    ef = st.ens_stats.cpu().numpy().astype(np.float64)
    assert np.allclose(ef[..., 1], tl, rtol=1e-3, atol=1e-3)
    over_j = _check_pullback(st, mid, fws, '4:2:0', 'soft', [e.g_y.cpu().numpy() for e in st.clfs], qrows)
    g_jpeg = np.stack([g.cpu().numpy() for g in st.jpeg_grads])
    over_b = _blur_pullback(st, g_jpeg, rows)
    g_blur = np.stack([g.cpu().numpy() for g in st.blur_grads]).astype(np.float64)
    want = po.backward(g_blur, st.table.cpu().numpy().astype(np.float64))
    got = np.stack([g.cpu().numpy() for g in st.pose_grads]).astype(np.float64)
    err = np.abs(got - want).max() / np.abs(g_blur).max()
    assert err <= BWD_BAR, err
    comb = _check_combination(st, st.pose_grads)
    print(f'accuracy: Pose -> Blur -> Jpeg: largest |sigma - rule| / bar = {over_s:.3f}, |tap - float64| / bar = {over_t:.3f}, |blur image - '
          f'float64| / bar = {over_f:.3f}, |pulled-back gradient - float64| / bar = {over_b:.3f}; the codec behind it {over_j:.3f} of its bar '
          f'({taken:.2%} of its pixels taken from the kernel), the warp\'s adjoint {err:.2e} (bar {BWD_BAR:.2e}), combination {comb:.2e}')
    assert max(over_s, over_t, over_f, over_b, over_j) <= 1.0


def test_repeatability_and_sweep(hip, pcnet, clf, case, monkeypatch):
    """Eager and graph-replayed runs, and two runs with one seed, are bitwise equal (a replay that did not advance the counter would
    repeat the first sigmas and differ from the eager run); another seed draws other sigmas; the sweep returns per configuration what
    spaa() returns for it when each configuration is a chunk of its own; with transfer= and the 'camssim' term the attack runs."""
    A = hip['attack']
    _, scene, _, targets = case
    bl = A.CaptureBlur(draws=3, seed=2)
    args = (None, targets[:2], True, scene, 5, LOSS, DEV, SETUP)
    cam_g, prj_g = A.spaa(pcnet, clf, *args, iters=8, blur=bl)
    assert A.LAST_RUN == dict(iterations=8, graph=True)
    cam_2, prj_2 = A.spaa(pcnet, clf, *args, iters=8, blur=bl)
    assert torch.equal(cam_2, cam_g) and torch.equal(prj_2, prj_g)
    monkeypatch.setattr(A, 'GRAPH_MAX_PIXELS', 0)
    cam_e, prj_e = A.spaa(pcnet, clf, *args, iters=8, blur=bl)
    assert A.LAST_RUN == dict(iterations=8, graph=False) and torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    monkeypatch.undo()
    tables = []
    for seed in (2, 3):
        st = A.BlurAttackState(pcnet, clf, targets[:2], scene, LOSS, SETUP, DEV, A.CaptureBlur(draws=3, seed=seed))
        for _ in range(3):
            st.iteration(True, 5, 2, 1, P_THRESH)
        assert int(st.counter.item()) == 3
        tables.append(st.blur_rows.cpu().numpy())
        del st
    over_s, over_t = _check_rows(tables[0], 2, 2, 2, 3, 0.5, 2.0)               # the rows of iteration t = 2
    assert over_s <= 1.0 and over_t <= 1.0 and not np.array_equal(tables[0], tables[1])
    cfgs = [(LOSS, 5, True, targets[:2]), (LOSS, 9, False, targets[2:4])]
    res = A.spaa_sweep(pcnet, clf, None, scene, SETUP, DEV, cfgs, iters=6, max_batch=2, blur=bl)
    for (cam, prj), (loss, d_thr, targeted, tg) in zip(res, cfgs):
        want = A.spaa(pcnet, clf, None, tg, targeted, scene, d_thr, loss, DEV, SETUP, iters=6, blur=bl)
        assert torch.equal(cam, want[0]) and torch.equal(prj, want[1])
    one = A.spaa(pcnet, clf, *args, iters=6)
    same = A.spaa(pcnet, clf, *args, iters=6, blur=None)
    assert torch.equal(one[0], same[0]) and torch.equal(one[1], same[1])
    assert not torch.equal(one[1], A.spaa(pcnet, clf, *args, iters=6, blur=bl)[1])
    cam, prj = A.spaa(pcnet, clf, None, targets[:2], True, scene, 5, 'camdE_caml2_camssim', DEV, SETUP, iters=5, blur=bl,
                      transfer=A.Transfer(momentum=0.9, sigma=1.0))
    assert torch.isfinite(cam).all() and torch.isfinite(prj).all() and prj.min() >= 0 and prj.max() <= 1
    print(f'accuracy: BlurAttackState after three iterations: largest |sigma - rule of t = 2| / bar = {over_s:.3f}, |tap - float64| / bar = '
          f'{over_t:.3f}; eager, graph replay, repeat and sweep equal bit for bit (bar: exact)')


def test_gaussian_blur_equals_spaa_blur_fwd(hip):
    A, lib = hip['attack'], hip['lib']
    H, W, n = 20, 37, 3
    rng = np.random.default_rng(8)
    y = np.stack([bo.float_image(rng, H, W) for _ in range(n)]).astype(F32)
    im = torch.from_numpy(y).permute(0, 3, 1, 2).contiguous().to(DEV)
    worst = 0.0
    for sg in ([2.5, 0.0, 0.7], 1.2):
        got = A.gaussian_blur(im, sg)
        assert got.shape == im.shape and got.device == im.device
        y4 = torch.zeros(n, H, W, 4, device=DEV)
        y4[..., :3] = torch.from_numpy(y).to(DEV)
        sigmas = torch.tensor(sg if isinstance(sg, list) else [sg] * n, dtype=torch.float32, device=DEV)[:, None].expand(n, 2).contiguous()
        rows = torch.zeros(n, 2, 12, device=DEV)
        lib.call('spaa_blur_rows', lib.ptr(sigmas), lib.ptr(rows), 2 * n)
        outs = [torch.zeros_like(y4) for _ in range(2)]
        lib.call('spaa_blur_fwd', lib.ptr_array([y4, y4]), lib.ptr(rows), 2, lib.ptr_array(outs), n, H, W)
        assert torch.equal(got, outs[0][..., :3].permute(0, 3, 1, 2)) and torch.equal(outs[0], outs[1])
        for b in range(n):
            s = F32(sigmas[b, 0].item())
            r, w = bo.taps(s)
            if r:
                x = y[b].astype(np.float64)
                worst = max(worst, float((np.abs(got[b].permute(1, 2, 0).cpu().numpy() - bo.forward(x, r, w)) /
                                          bo.bar_forward(x, r, w, bo.tap_ulps(s))).max()))
    assert torch.equal(A.gaussian_blur(im, [2.5, 0.0, 0.7])[1], im[1])           # sigma = 0: the image bit for bit
    assert torch.equal(A.gaussian_blur(im[:1], 0.8), A.gaussian_blur(im, 0.8)[:1])       # (one image: the padded half is dropped)
    with pytest.raises(RuntimeError, match='GPU only'):
        A.gaussian_blur(im.cpu(), 1.0)
    with pytest.raises(ValueError):
        A.gaussian_blur(im, [1.0, 2.0])
    with pytest.raises(ValueError):
        A.gaussian_blur(im, 2.6)
    print(f'accuracy: gaussian_blur: equal to spaa_blur_fwd bit for bit (bar: exact), largest |image - float64| / bar = {worst:.3f}')
    assert worst <= 1.0


def test_blur_survival(hip, pcnet, clf, case):
    """Against the oracle's classification (the product classifier on the oracle's blurred images), sigma by sigma; the scene, which is
    not of class UNTARGETED_OTHER sharp, passes as an untargeted success at sigma = 0.5 too; and a uniform image is its own blur at
    every sigma (the taps sum to 1, the border is replicated), so its row of answers is the sharp image's answer."""
    A = hip['attack']
    _, scene, _, targets = case
    res = A.spaa_sweep(pcnet, clf, None, scene, SETUP, DEV, [(LOSS, 5, True, targets[:2])], iters=12, blur=A.CaptureBlur(draws=2, seed=1))
    flat = torch.full((1, 3, *SZ), 0.25, device=DEV)
    cams = torch.cat((res[0][0], scene.to(DEV).reshape(1, 3, *SZ), flat))       # two attacked captures, the plain scene, a uniform image
    flat_top1 = int(_logits(clf, flat.permute(0, 2, 3, 1).cpu().numpy())[0].argmax())
    tgt, tg = targets[:2] + [UNTARGETED_OTHER, flat_top1], [True, True, False, True]
    sigmas = (0.5, 1.5, 2.5)
    got = A.blur_survival(cams, clf, tgt, tg, CROP, sigmas=sigmas)
    assert got.shape == (3, 4) and got.dtype == bool and np.array_equal(got, A.blur_survival(cams, clf, tgt, tg, CROP, sigmas=sigmas))
    y = cams.permute(0, 2, 3, 1).cpu().numpy()
    want, gap = np.zeros((3, 4), dtype=bool), np.inf
    for s, sigma in enumerate(sigmas):
        r, w = bo.taps(F32(sigma))
        raw = _logits(clf, np.stack([bo.forward(y[b].astype(np.float64), r, w) for b in range(4)]).astype(F32))
        top2 = np.sort(raw, axis=1)[:, -2:]
        gap = min(gap, float((top2[:, 1] - top2[:, 0]).min()))
        want[s] = jo.survives(raw, tgt, tg)
    print(f'blur_survival: {got.astype(int).tolist()}, through the oracle {want.astype(int).tolist()}, smallest top-2 gap {gap:.3e}')
    assert gap > 1e-2, 'the planted case is near a tie: choose another seed'
    assert np.array_equal(got, want) and got[0, 2] and got[:, 3].all()
    assert A.blur_survival(cams[:1], clf, tgt[:1], True, CROP).shape == (5, 1)
