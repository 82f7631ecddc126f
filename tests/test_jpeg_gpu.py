"""GPU: the JPEG attack loop (JpegAttackState through spaa / spaa_sweep) on the 64 x 64 synthetic PCNet and the 56 x 56 ResNet-18 of
tests/test_jitter_gpu.py.  One first iteration against an oracle composition that is teacher-forced with the state's own camera image
(an fp32 y one rounding away from a float64 one may round a coefficient the other way, which is a different image, not an error): the
quality rows, the draw images on safe blocks, the per-draw logits and the decision from them, the pulled-back gradients and their
combination.  The Q = 100 / 4:4:4 / 'straight' twin of the plain attack, the codec behind jitter and behind pose + jitter, the eager /
graph / repeat / sweep identities, jpeg_roundtrip against spaa_jpeg_fwd, and jpeg_survival."""
import numpy as np
import pytest
import torch

import ensemble_oracle as eo
import jitter_oracle as jo
import jpeg_oracle as jp
import pose_oracle as po
from spaa_amd import synthetic as syn
from test_gpu_parity import hip, make_pcnet  # noqa: F401  (hip: module fixture)
from test_jitter_gpu import (csd, clf, pcnet, case, DEV, SZ, SETUP, LOSS, P_THRESH, TARGETED, D_THR,  # noqa: F401  (fixtures)
                             UNTARGETED_OTHER)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CROP = SETUP['classifier_crop_sz']


def _oracle_draws(ims_in, rows, sub, ims_gpu):
    """Per draw j the float64 round trip of the J input batches `ims_in` [J][B][H][W][>= 3] at the state's own qualities, with the
    kernel's value wherever the oracle cannot be held to (a block near a tie and the pixels that read it; a pixel within the rounding
    margin): (images fp32 [J][B][H][W][3], the forward dicts, the share of pixels taken from the kernel).  Asserts the rest equal.  (The
    10 % condition of tests/test_jpeg_ops_gpu.py is for its planted float images; a camera image is what it is, and behind the jitter's
    8-bit step exact ties are generic.  Here the share is printed, and must leave most of the image compared.)"""
    J, B = len(ims_in), ims_in[0].shape[0]
    out = np.zeros((J, B) + SZ + (3,), dtype=np.float32)
    fws, taken = [], 0
    for j in range(J):
        fws.append([])
        for b in range(B):
            fw = jp.forward(ims_in[j][b].astype(np.float64), int(rows[b, j, 0]), sub)
            fws[j].append(fw)
            got = ims_gpu[j][b, ..., :3]
            if fw['ratios'] is None:
                assert np.array_equal(got, ims_in[j][b][..., :3])
                out[j, b] = got
                continue
            hold = jp.safe_pixels(fw, *SZ, sub) & ~(jp.round_distance(fw['v']) < jp.ROUND_MARGIN).any(axis=-1)
            want = (np.rint(fw['out'] * 255.0).astype(np.float32) / np.float32(255.0))
            assert np.array_equal(got[hold], want[hold]), (j, b)
            out[j, b] = np.where(hold[..., None], want, got)
            taken += int((~hold).sum())
    share = taken / (J * B * SZ[0] * SZ[1])
    assert share < 0.5, 'the case is near too many ties for the comparison to say much: choose another seed'
    return out, fws, share


def _logits(clf, ims):
    """The product classifier's logits of fp32 images [B][H][W][3], as float64 numpy."""
    return clf(torch.from_numpy(ims).permute(0, 3, 1, 2).contiguous().to(DEV), CROP)[0].double().cpu().numpy()


def _bits(gate):
    g = gate.cpu().numpy().reshape(-1, *SZ)
    return (np.stack([(g >> c) & 1 for c in range(3)], axis=-1).astype(bool), np.stack([(g >> (4 + c)) & 1 for c in range(3)], axis=-1).astype(bool))


def _check_pullback(st, ims_in, fws, sub, gradient, g_eng, rows):
    """st.jpeg_grads against the float64 adjoint of the gradient images `g_eng` [J][B][H][W][4], with the kernel's own gate bytes."""
    worst = 0.0
    for j in range(st.K):
        in_g, out_g = _bits(st.jpeg_gates[j])
        got = st.jpeg_grads[j].cpu().numpy().astype(np.float64)
        assert (got[..., 3] == 0).all()
        for b in range(st.B):
            Q = int(rows[b, j, 0])
            y, g = ims_in[j][b].astype(np.float64), g_eng[j][b, ..., :3].astype(np.float64)
            want = jp.adjoint(g, y, Q, sub, gradient, gates=(in_g[b], out_g[b]))
            bar = jp.bar_adjoint(g, y, Q, sub, gradient, gates=(in_g[b], out_g[b])) + 1e-30
            if Q == 0:
                assert np.array_equal(got[b, ..., :3], g)
                continue
            worst = max(worst, float((np.abs(got[b, ..., :3] - want) / bar)[jp.safe_pixels(fws[j][b], *SZ, sub)].max()))
    return worst


@pytest.mark.parametrize('sub,gradient', [('4:2:0', 'soft'), ('4:4:4', 'straight')])
def test_first_iteration_against_the_oracle(hip, pcnet, clf, case, sub, gradient):
    A = hip['attack']
    sd, scene, oc, targets = case
    J, B = 3, 4
    jg = A.JpegCapture(quality=(60, 95), subsampling=sub, gradient=gradient, draws=J, seed=11)
    st = A.JpegAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, jg)
    assert st.K == J and len({id(e) for e in st.clfs}) == J and [type(s).__name__ for s in st.stages] == ['JpegStage']
    st.forward_decide(TARGETED, D_THR, P_THRESH)
    st.backward_step(2, 1)
    rows = st.jpeg_rows.cpu().numpy()
    assert int(st.counter.item()) == 1 and np.array_equal(rows, jp.draw_rows(11, 0, B, J, 60, 95, True))
    y = st._y.cpu().numpy()
    ims_gpu = [im.cpu().numpy() for im in st.jpeg_ims]
    ims, fws, taken = _oracle_draws([y] * J, rows, sub, ims_gpu)
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
    print(f'{sub} {gradient}: qualities {rows[..., 0].astype(int).tolist()}, {taken:.2%} of the pixels taken from the kernel; max |target '
          f'logit - ref| {np.abs(ef[..., 1] - ref["tl"]).max():.3e} at max |ref| {np.abs(ref["tl"]).max():.3f}')
    assert np.allclose(ef[..., 0][clear], ref['p1'][clear], rtol=1e-3) and np.allclose(ef[..., 1], ref['tl'], rtol=1e-3, atol=1e-3)
    assert np.allclose(stats[:, 1], caml2, rtol=1e-4)                          # the stealth loss is the CLEAN capture's
    # the adjoint's wiring: the pulled-back gradients are spaa_jpeg_bwd of the engines' own gradient images and the stage's gate bytes
    g_eng = [e.g_y.cpu().numpy() for e in st.clfs]
    worst = _check_pullback(st, [y] * J, fws, sub, gradient, g_eng, rows)
    print(f'accuracy: JpegStage pull-back {sub} {gradient}: largest |g - float64| / bar = {worst:.3f}')
    assert worst <= 1.0
    g_own = [g.reshape(B, -1, 4).cpu().numpy().astype(np.float64) for g in st.jpeg_grads]
    g_adv = st.g_adv.reshape(B, -1, 4).cpu().numpy().astype(np.float64)
    own = eo.combine(g_own, ew)
    err = np.abs(g_adv - own).max(axis=(1, 2)) / np.abs(own).max(axis=(1, 2))
    print(f'g_adv against the float64 combination of the pulled-back gradients, per sample {err.tolist()}')
    assert (err <= 2e-6).all() and (g_adv[..., 3] == 0).all()


def test_quality_100_twin_of_the_plain_attack(hip, pcnet, clf, case):
    """quality = (100, 100), 4:4:4, 'straight': every table entry is 1, so a draw is y behind coefficient rounding and the 8-bit step.
    It still runs J passes.  What the 8-bit step determines is asserted: draw 0 is the plain attack's capture bit for bit, and so are
    its logits; a compressed draw differs from y by at most 0.5 (2.83^2 worst-case gain of |D| x |D|) (1 + 1.772) + 0.5 = 11.6 levels
    (seen: about one); the 'straight' adjoint of such a draw is gate . M_ycc^T . M_rgb^T . gate, the identity up to the six-digit
    JFIF constants (|M_rgb M_ycc - 1| < 2e-6 per entry, three entries per row) and the fp32 chain, whose worst case is 65 terms at the
    gain 2.83^4 = 64 of four passes of |D|: 6e-6 + 65 . 64 u = 2.6e-4 of max |g|.  The direction: with u_0 the plain attack's unit gradient image and
    the J - 1 compressed draws orthogonal to it, the cosine of the combined direction to the plain one would be 1 / sqrt(J); that
    they agree with it means more."""
    A = hip['attack']
    _, scene, _, targets = case
    B, J = 4, 3
    jg = A.JpegCapture(quality=(100, 100), subsampling='4:4:4', gradient='straight', draws=J, seed=3)
    st = A.JpegAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, jg)
    st.forward_decide(TARGETED, D_THR, P_THRESH)
    st.backward_step(2, 1)
    plain = A.AttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV)
    plain.forward_decide(TARGETED, D_THR, P_THRESH)
    g_plain = plain._adv_gradient().clone()
    rows = st.jpeg_rows.cpu().numpy()
    assert int(st.counter.item()) == 1 and (rows[:, 0, 0] == 0).all() and (rows[:, 1:, 0] == 100).all() and len({id(e) for e in st.clfs}) == J
    assert torch.equal(st.jpeg_ims[0][..., :3], plain._y[..., :3]) and torch.equal(st.jpeg_grads[0][..., :3], st.clfs[0].g_y[..., :3])
    g0, gp = st.clfs[0].g_y.flatten(1).double(), g_plain.flatten(1).double()    # (the two decisions scale their seeds differently)
    assert ((g0 * gp).sum(1) / (g0.norm(dim=1) * gp.norm(dim=1)) >= 1 - 1e-9).all()
    for j in range(1, J):
        d = (st.jpeg_ims[j][..., :3] - plain._y[..., :3]).abs().max().item() * 255
        g, pulled, gate = st.clfs[j].g_y[..., :3], st.jpeg_grads[j][..., :3], st.jpeg_gates[j].reshape(B, *SZ)
        passing = torch.stack([((gate >> c) & (gate >> (4 + c)) & 1).bool() for c in range(3)], dim=-1)
        rel = ((pulled - g).abs() * passing).max().item() / g.abs().max().item()
        print(f'draw {j}: max |image - y| = {d:.2f} levels (bar 11.6), the adjoint against the identity where both gates pass {rel:.2e} (bar 2.6e-4)')
        assert 0 < d <= 11.6 and rel <= 2.6e-4 and not torch.equal(st.jpeg_ims[j], st.jpeg_ims[0])
    ga, gp = st.g_adv.flatten(1).double(), g_plain.flatten(1).double()
    cos = ((ga * gp).sum(1) / (ga.norm(dim=1) * gp.norm(dim=1))).cpu().numpy()
    print(f'cosine of the combined direction to the plain attack\'s, per sample: {cos.tolist()} (orthogonal draws would give {J ** -0.5:.3f})')
    assert (cos > J ** -0.5).all()


def test_jpeg_behind_jitter_and_behind_pose_and_jitter(hip, pcnet, clf, case):
    """Pose -> Jitter -> Jpeg: the codec reads the stage before it draw by draw, and the gradients go back the same way."""
    A = hip['attack']
    _, scene, _, targets = case
    B, J = 4, 2
    jg = A.JpegCapture(quality=(70, 90), draws=J, seed=4)
    jt = A.CaptureJitter(draws=J, seed=5)
    for pose in (None, A.PoseJitter(draws=J, seed=6)):
        st = A.JpegAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, jg, pose=pose, jitter=jt)
        names = [type(s).__name__ for s in st.stages]
        assert names == (['PoseStage'] if pose else []) + ['JitterStage', 'JpegStage']
        st.forward_decide(TARGETED, D_THR, P_THRESH)
        st.backward_step(2, 1)
        rows = st.jpeg_rows.cpu().numpy()
        assert np.array_equal(rows, jp.draw_rows(4, 0, B, J, 70, 90, True)) and int(st.jpeg_counter.item()) == 1 and int(st.counter.item()) == 1
        mid = [im.cpu().numpy() for im in st.draw_ims]                          # what the jitter stage made: the codec's inputs
        ims, fws, taken = _oracle_draws(mid, rows, '4:2:0', [im.cpu().numpy() for im in st.jpeg_ims])
        tl = np.stack([_logits(clf, ims[j])[np.arange(B), targets] for j in range(J)], axis=1)
        ef = st.ens_stats.cpu().numpy().astype(np.float64)
        print(f'{names}: {taken:.2%} of the pixels taken from the kernel, max |target logit - ref| {np.abs(ef[..., 1] - tl).max():.3e}')
        assert np.allclose(ef[..., 1], tl, rtol=1e-3, atol=1e-3)
        worst = _check_pullback(st, mid, fws, '4:2:0', 'soft', [e.g_y.cpu().numpy() for e in st.clfs], rows)
        print(f'accuracy: JpegStage pull-back behind {names[:-1]}: largest |g - float64| / bar = {worst:.3f}')
        assert worst <= 1.0
        # then the jitter's adjoint of the codec's, then the warp's of the jitter's
        jit = st.jit.cpu().numpy().astype(np.float64)
        gates = np.stack([g.cpu().numpy().reshape(B, *SZ) for g in st.draw_gates])
        g_jpeg = np.stack([g.cpu().numpy() for g in st.jpeg_grads])
        want = jo.backward(g_jpeg, jit, gates)
        got = np.stack([g.cpu().numpy() for g in st.draw_grads]).astype(np.float64)
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err <= 2e-6, err
        last = st.draw_grads
        if pose:
            table = st.table.cpu().numpy().astype(np.float64)
            want = po.backward(got, table)
            got = np.stack([g.cpu().numpy() for g in st.pose_grads]).astype(np.float64)
            err = np.abs(got - want).max() / np.abs(np.stack([g.cpu().numpy() for g in st.draw_grads])).max()
            assert err <= 2 * po.eps_c(*SZ) * 16 + 16 * U, err
            last = st.pose_grads
        own = eo.combine([g.reshape(B, -1, 4).cpu().numpy().astype(np.float64) for g in last], st.ens_w.cpu().numpy())
        g_adv = st.g_adv.reshape(B, -1, 4).cpu().numpy().astype(np.float64)
        assert (np.abs(g_adv - own).max(axis=(1, 2)) / np.abs(own).max(axis=(1, 2)) <= 2e-6).all()
        del st


def test_repeatability_and_sweep(hip, pcnet, clf, case, monkeypatch):
    """Eager and graph-replayed runs, and two runs with one seed, are bitwise equal; another seed draws other qualities; the sweep
    returns per configuration what spaa() returns for it when each configuration is a chunk of its own; with transfer= and the
    'camssim' term the attack runs."""
    A = hip['attack']
    _, scene, _, targets = case
    jg = A.JpegCapture(draws=3, seed=2)
    args = (None, targets[:2], True, scene, 5, LOSS, DEV, SETUP)
    cam_g, prj_g = A.spaa(pcnet, clf, *args, iters=8, jpeg=jg)
    assert A.LAST_RUN == dict(iterations=8, graph=True)
    cam_2, prj_2 = A.spaa(pcnet, clf, *args, iters=8, jpeg=jg)
    assert torch.equal(cam_2, cam_g) and torch.equal(prj_2, prj_g)
    monkeypatch.setattr(A, 'GRAPH_MAX_PIXELS', 0)
    cam_e, prj_e = A.spaa(pcnet, clf, *args, iters=8, jpeg=jg)
    assert A.LAST_RUN == dict(iterations=8, graph=False) and torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    monkeypatch.undo()
    tables = []
    for seed in (2, 3):
        st = A.JpegAttackState(pcnet, clf, targets[:2], scene, LOSS, SETUP, DEV, A.JpegCapture(draws=3, seed=seed))
        for _ in range(3):
            st.iteration(True, 5, 2, 1, P_THRESH)
        assert int(st.counter.item()) == 3
        tables.append(st.jpeg_rows.cpu().numpy())
        del st
    assert np.array_equal(tables[0], jp.draw_rows(2, 2, 2, 3, 60, 95, True)) and not np.array_equal(tables[0], tables[1])
    cfgs = [(LOSS, 5, True, targets[:2]), (LOSS, 9, False, targets[2:4])]
    res = A.spaa_sweep(pcnet, clf, None, scene, SETUP, DEV, cfgs, iters=6, max_batch=2, jpeg=jg)
    for (cam, prj), (loss, d_thr, targeted, tg) in zip(res, cfgs):
        want = A.spaa(pcnet, clf, None, tg, targeted, scene, d_thr, loss, DEV, SETUP, iters=6, jpeg=jg)
        assert torch.equal(cam, want[0]) and torch.equal(prj, want[1])
    one = A.spaa(pcnet, clf, *args, iters=6)
    same = A.spaa(pcnet, clf, *args, iters=6, jpeg=None)
    assert torch.equal(one[0], same[0]) and torch.equal(one[1], same[1])
    assert not torch.equal(one[1], A.spaa(pcnet, clf, *args, iters=6, jpeg=jg)[1])
    cam, prj = A.spaa(pcnet, clf, None, targets[:2], True, scene, 5, 'camdE_caml2_camssim', DEV, SETUP, iters=5, jpeg=jg,
                      transfer=A.Transfer(momentum=0.9, sigma=1.0))
    assert torch.isfinite(cam).all() and torch.isfinite(prj).all() and prj.min() >= 0 and prj.max() <= 1


def test_jpeg_roundtrip_equals_spaa_jpeg_fwd(hip):
    A, lib = hip['attack'], hip['lib']
    H, W, n = 20, 28, 3
    rng = np.random.default_rng(8)
    y = np.stack([jp.float_image(rng, H, W) for _ in range(n)]).astype(np.float32)
    im = torch.from_numpy(y).permute(0, 3, 1, 2).contiguous().to(DEV)
    for sub, code in (('4:2:0', 2), ('4:4:4', 0)):
        for qs in ([90, 35, 75], 60):
            got = A.jpeg_roundtrip(im, qs, sub)
            assert got.shape == im.shape and got.device == im.device
            y4 = torch.zeros(n, H, W, 4, device=DEV)
            y4[..., :3] = torch.from_numpy(y).to(DEV)
            rows = torch.zeros(n, 2, 4, device=DEV)
            rows[:, :, 0] = torch.tensor(qs if isinstance(qs, list) else [qs] * n, dtype=torch.float32, device=DEV)[:, None]
            outs = [torch.zeros_like(y4) for _ in range(2)]
            gates = [torch.zeros(n, H * W, dtype=torch.uint8, device=DEV) for _ in range(2)]
            floats = lib.load().spaa_jpeg_ws_floats(code, 2, n, H, W)
            ws = torch.zeros(floats, device=DEV) if floats else None
            lib.call('spaa_jpeg_fwd', lib.ptr_array([y4, y4]), lib.ptr(rows), 2, code, lib.ptr_array(outs), lib.ptr_array(gates),
                     lib.ptr(ws), n, H, W)
            assert torch.equal(got, outs[0][..., :3].permute(0, 3, 1, 2)) and torch.equal(outs[0], outs[1])
            assert torch.equal(torch.round(got * 255) / torch.full((), 255.0, device=DEV), got)
    assert torch.equal(A.jpeg_roundtrip(im[:1], 80), A.jpeg_roundtrip(im, 80)[:1])       # (one image: the padded half is dropped)
    with pytest.raises(RuntimeError, match='GPU only'):
        A.jpeg_roundtrip(im.cpu(), 75)
    with pytest.raises(ValueError):
        A.jpeg_roundtrip(im, [75, 80])
    with pytest.raises(ValueError):
        A.jpeg_roundtrip(im, 0)


def test_jpeg_survival(hip, pcnet, clf, case):
    """Against the oracle's classification (the product classifier on the oracle's round trips), quality by quality."""
    A = hip['attack']
    _, scene, _, targets = case
    res = A.spaa_sweep(pcnet, clf, None, scene, SETUP, DEV, [(LOSS, 5, True, targets[:2])], iters=12,
                       jpeg=A.JpegCapture(draws=2, seed=1))
    cams = torch.cat((res[0][0], scene.to(DEV).reshape(1, 3, *SZ)))             # two attacked captures and the plain scene
    tgt, tg = targets[:2] + [UNTARGETED_OTHER], [True, True, False]
    qualities = (95, 75, 30)
    for sub in ('4:2:0', '4:4:4'):
        got = A.jpeg_survival(cams, clf, tgt, tg, CROP, qualities=qualities, subsampling=sub)
        assert got.shape == (3, 3) and got.dtype == bool and np.array_equal(got, A.jpeg_survival(cams, clf, tgt, tg, CROP, qualities=qualities,
                                                                                                  subsampling=sub))
        y = cams.permute(0, 2, 3, 1).cpu().numpy()
        want, gap = np.zeros((3, 3), dtype=bool), np.inf
        for q, Q in enumerate(qualities):
            ims = np.stack([np.rint(jp.forward(y[b].astype(np.float64), Q, sub)['out'] * 255.0).astype(np.float32) / np.float32(255.0)
                            for b in range(3)])
            raw = _logits(clf, ims)
            top2 = np.sort(raw, axis=1)[:, -2:]
            gap = min(gap, float((top2[:, 1] - top2[:, 0]).min()))
            want[q] = jo.survives(raw, tgt, tg)
        print(f'jpeg_survival {sub}: {got.astype(int).tolist()}, through the oracle {want.astype(int).tolist()}, smallest top-2 gap {gap:.3e}')
        assert gap > 1e-2, 'the planted case is near a tie: choose another seed'
        assert np.array_equal(got, want) and got[:, 2].all()                    # (the scene is not class UNTARGETED_OTHER)
    assert A.jpeg_survival(cams[:1], clf, tgt[:1], True, CROP).shape == (5, 1)
