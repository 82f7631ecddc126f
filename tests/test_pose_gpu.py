"""GPU: the pose attack loop (PoseAttackState through spaa / spaa_sweep) on the 64 x 64 synthetic PCNet and the 56 x 56 ResNet-18 of
the jitter tests: one teacher-forced first iteration against the float64 oracle (tests/pose_oracle.py), the zero-range twin of the
plain attack, twelve traced iterations whose tables must be the stated function of (seed, t, b, j), the eager / graph / repeat / sweep
identities, pose together with capture jitter and with Transfer, and pose_survival."""
import numpy as np
import pytest
import torch

import ensemble_oracle as eo
import jitter_oracle as jo
import pose_oracle as po
import spaa_oracle as so
from spaa_amd import synthetic as syn
from test_gpu_parity import hip, make_pcnet  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SZ = (64, 64)
SETUP = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=SZ)
LOSS = 'camdE_caml2'
P_THRESH = 0.9
PCNET_SEED, SCENE_SEED = 0, 1
INPUT_SZ = (56, 56)
TARGETED = [True, True, False, False]
D_THR = [5.0, 5.0, 9.0, 5.0]
UNTARGETED_OTHER = 7               # an untargeted sample on a class the classifier does not give the scene: fooled from the start
ZERO = dict(rotate=0.0, zoom=0.0, shift=0.0, tilt=0.0)
U = 2.0 ** -24
BWD_BAR = 2 * po.eps_c(*SZ) * 16 + 16 * U     # the backward bar of test_pose_ops_gpu.py at 64 x 64, relative to max |g_out|


@pytest.fixture(scope='module')
def csd():
    return syn.resnet18_state_dict(2, logit_gain=20.0)


@pytest.fixture(scope='module')
def clf(hip, csd):
    return hip['clf'].Classifier('resnet18', DEV, state_dict=csd, input_sz=INPUT_SZ)


@pytest.fixture(scope='module')
def pcnet(hip):
    return make_pcnet(hip, syn.pcnet_state_dict(PCNET_SEED, cam_sz=SZ, mask='rect'), SZ)


@pytest.fixture(scope='module')
def case(csd):
    """CPU side: PCNet weights, scene, the oracle's classifier, the B = 4 targets (two targeted, then untargeted on the classifier's
    class of the scene and on UNTARGETED_OTHER)."""
    sd = syn.pcnet_state_dict(PCNET_SEED, cam_sz=SZ, mask='rect')
    scene = syn.scenes(SCENE_SEED, 1, SZ)
    oc = so.OracleClassifier('resnet18', csd, input_sz=INPUT_SZ)
    true_idx = int(oc(scene, SETUP['classifier_crop_sz'])[0][0].argmax())
    return sd, scene, oc, [204, 291, true_idx, UNTARGETED_OTHER]


def _close_tables(got, seed, t, B, J, ps, clean0=True):
    """The kernel's table against the restatement at the draw test's bar (relative 5e-7, absolute floor 1e-12)."""
    ref = po.draw_tables(seed, t, B, J, ps.rotate, ps.zoom, ps.shift, ps.tilt, *SZ, clean0)
    return bool((np.abs(got.astype(np.float64) - ref) <= 5e-7 * np.abs(ref) + 1e-12).all())


def test_first_iteration_against_the_oracle(hip, pcnet, clf, case):
    A = hip['attack']
    sd, scene, oc, targets = case
    J, B = 3, 4
    ps = A.PoseJitter(draws=J, seed=11)
    st = A.PoseAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, ps)
    assert st.K == J and len({id(e) for e in st.clfs}) == J and len(clf._engines[(B, SZ, (60, 60), 'f32')]) >= J
    st.forward_decide(TARGETED, D_THR, P_THRESH)
    st.backward_step(2, 1)
    table = st.table.cpu().numpy()
    assert int(st.counter.item()) == 1 and (table[:, 0] == np.array(po.IDENTITY_ROW, dtype=np.float32)).all()
    assert _close_tables(table, 11, 0, B, J, ps)
    # the three members: the float64 classifier behind the float64 warp with the state's OWN table (teacher-forced)
    ref = po.first_iteration(sd, oc, targets, TARGETED, scene, D_THR, SETUP, table.astype(np.float64), p_thresh=P_THRESH)
    clear = (ref['gap'] > 1e-3) & (ref['p_margin'] > 1e-3)
    clear_d = ref['d_margin'] > 1e-3
    print(f'oracle: top-2 gaps {ref["gap"].tolist()}, |p1 - p_thresh| {ref["p_margin"].tolist()}, |caml2 255 - d_thr| '
          f'{ref["d_margin"].tolist()}, fooled {ref["fooled"].astype(int).tolist()}, best_adv {ref["best_adv"].tolist()}')
    assert (~clear).sum() <= 1 and clear_d.all(), 'the case itself is near a tie: choose other seeds'
    es, ef, ew = st.ens_state.cpu().numpy(), st.ens_stats.cpu().numpy().astype(np.float64), st.ens_w.cpu().numpy()
    state, stats = st.state.cpu().numpy(), st.stats.cpu().numpy().astype(np.float64)
    assert (es[clear] == ref['ens_state'][clear]).all(), (es, ref['ens_state'])
    row = clear.all(axis=1)
    assert (state[row, 0] == ref['state_succ'][row]).all() and (state[row, 3] == ref['nfooled'][row]).all()
    assert (state[row & clear_d, 1] == ref['best_adv'][row & clear_d]).all()
    assert (ew == 1).all() and (ref['ens_w'] == 1).all()                       # (no focus: every draw pulls)
    print(f'max |p1 - ref| / ref {np.abs(ef[..., 0] / ref["p1"] - 1).max():.3e}, max |target logit - ref| '
          f'{np.abs(ef[..., 1] - ref["tl"]).max():.3e} at max |ref| {np.abs(ref["tl"]).max():.3f}')
    assert np.allclose(ef[..., 0][clear], ref['p1'][clear], rtol=1e-3) and np.allclose(ef[..., 1], ref['tl'], rtol=1e-3, atol=1e-3)
    assert np.allclose(stats[:, 1], ref['caml2'], rtol=1e-4)                   # the stealth loss is the UNWARPED capture's
    # the draws the members saw: the float64 warp of the state's own y
    y = st._y.cpu().numpy()
    D = max(np.abs(np.diff(np.pad(y[..., :3], ((0, 0), (1, 1), (1, 1), (0, 0))), axis=a)).max() for a in (1, 2))
    ims = np.stack([t.cpu().numpy() for t in st.pose_ims])
    err = np.abs(ims - po.forward(y, table.astype(np.float64))).max()
    print(f'draw images against the float64 warp: {err:.3e} (bar {2 * po.eps_c(*SZ) * D + 8 * U:.3e}, D = {D:.3f})')
    assert err <= 2 * po.eps_c(*SZ) * D + 8 * U and np.array_equal(ims[0, ..., :3], y[..., :3])
    # the pulled-back gradients: autograd's float64 adjoint of the engines' own gradient images
    g_eng = np.stack([e.g_y.cpu().numpy() for e in st.clfs])
    pulled = po.backward(g_eng, table.astype(np.float64)).reshape(J, B, -1, 4)
    g_own = [g.reshape(B, -1, 4).cpu().numpy().astype(np.float64) for g in st.pose_grads]
    gmax = np.abs(g_eng[..., :3]).reshape(J, B, -1).max(axis=2)
    err = max(np.abs(g_own[j][b] - pulled[j, b]).max() / gmax[j, b] for j in range(J) for b in range(B))
    print(f'pulled-back gradients against the float64 adjoint of the engines\' own: {err:.3e} of max |g| (bar {BWD_BAR:.3e})')
    assert err <= BWD_BAR
    # g_adv: the float64 combination of the pulled-back gradients the state itself produced
    g_adv = st.g_adv.reshape(B, -1, 4).cpu().numpy().astype(np.float64)
    own = eo.combine(g_own, ew)
    err = np.abs(g_adv - own).max(axis=(1, 2)) / np.abs(own).max(axis=(1, 2))
    print(f'g_adv against the float64 combination of the state\'s own pulled-back gradients, per sample {err.tolist()}')
    assert (err <= BWD_BAR).all() and (g_adv[..., 3] == 0).all()
    # against the oracle's direction: nothing beyond the members' own unit-vector errors and the new kernels' rounding
    e_bk = np.stack([np.sqrt(((eo.unit_images(g_own[k])[0] - eo.unit_images(ref['g'][k])[0]) ** 2).sum(axis=(1, 2)))
                     for k in range(J)], axis=1)
    l2 = np.sqrt(((g_adv - eo.combine(ref['g'], ew)) ** 2).sum(axis=(1, 2)))
    bound = (ew * e_bk).sum(axis=1) + 2e-6 * J
    print(f'unit-vector errors of the draws {e_bk.tolist()}, combined direction L2 error {l2.tolist()}, bound {bound.tolist()}')
    assert (l2 <= bound).all()


def test_zero_range_twin_of_the_plain_attack(hip, pcnet, clf, case):
    A = hip['attack']
    _, scene, _, targets = case
    B = 4
    st = A.PoseAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, A.PoseJitter(draws=2, **ZERO))
    st.iteration(TARGETED, D_THR, 2, 1, P_THRESH)
    plain = A.AttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV)
    plain.iteration(TARGETED, D_THR, 2, 1, P_THRESH)
    assert torch.equal(st.state[:, 0:3], plain.state[:, 0:3])
    dx = (st.x - plain.x).abs().max().item()
    print(f'zero-range twin: max |x - plain x| after one iteration = {dx:.3e}')
    assert dx <= 1e-5
    es = st.ens_state.cpu()
    assert torch.equal(es[:, 0], es[:, 1]) and torch.equal(st.ens_stats[:, 0], st.ens_stats[:, 1])
    assert torch.equal(st.pose_ims[0][..., :3], st._y[..., :3]) and torch.equal(st.pose_ims[1], st.pose_ims[0])
    assert (st.table.cpu().numpy() == np.array(po.IDENTITY_ROW, dtype=np.float32)).all()


def test_twelve_traced_iterations(hip, pcnet, clf, case):
    """In every iteration draw 0's row is the identity and the table the stated function of (seed, t, b, j), state and stats the
    ensemble's functions of the members' rows; the device counter reads 12 afterwards."""
    A = hip['attack']
    _, scene, _, targets = case
    J, B = 3, 4
    ps = A.PoseJitter(draws=J, seed=5)
    st = A.PoseAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, ps)
    targeted, d_thr, tgt = torch.tensor(TARGETED), torch.tensor(D_THR), torch.tensor(targets)
    best_before = torch.full((B,), 1e6)
    seen_col_step = seen_adv_step = False
    for i in range(12):
        st.iteration(TARGETED, D_THR, 2, 1, P_THRESH)
        entry = st.trace_entry()
        assert len(entry) == 4
        state, stats, es, ef = (t.cpu() for t in entry)
        table = st.table.cpu()
        assert torch.equal(table[:, 0], torch.tensor(po.IDENTITY_ROW).expand(B, 8)), i
        assert _close_tables(table.numpy(), 5, i, B, J, ps), i
        assert torch.equal(st.pose_ims[0][..., :3], st._y[..., :3]), i            # draw 0 is the unwarped capture
        assert state.shape == (B, 4) and stats.shape == (B, 8) and es.shape == (B, J, 2) and ef.shape == (B, J, 2)
        succ, fooled = (es[..., 0] & 1).bool(), (es[..., 0] & 2).bool()
        assert torch.equal(succ, torch.where(targeted[:, None], es[..., 1] == tgt[:, None], es[..., 1] != tgt[:, None])), i
        assert torch.equal(fooled, torch.where(targeted[:, None], succ & (ef[..., 0] > P_THRESH), succ)), i
        best_adv = fooled.all(dim=1) & (stats[:, 1] * 255.0 > d_thr)
        assert torch.equal(state[:, 0].bool(), succ.all(dim=1)) and torch.equal(state[:, 1].bool(), best_adv), i
        assert torch.equal(state[:, 3], fooled.sum(dim=1).int()), i
        assert torch.equal(stats[:, 0], ef[..., 0].min(dim=1).values), i
        best = best_adv & (stats[:, 3] < best_before)
        assert torch.equal(state[:, 2].bool(), best), i
        best_before = torch.where(best, stats[:, 3], best_before)
        seen_col_step |= bool(best_adv.any())
        seen_adv_step |= bool((~best_adv).any())
    assert seen_col_step and seen_adv_step                              # both steps were taken in this run
    assert int(st.counter.item()) == 12
    cam, prj = st.results()
    assert torch.isfinite(cam).all() and torch.isfinite(prj).all() and prj.min() >= 0 and prj.max() <= 1


def test_repeatability_and_sweep(hip, pcnet, clf, case, monkeypatch, capsys):
    """Eager and graph-replayed runs, and two runs with one seed, are bitwise equal; another seed gives other tables; the sweep returns
    per configuration what spaa() returns for it when each configuration is a chunk of its own."""
    A = hip['attack']
    _, scene, _, targets = case
    ps = A.PoseJitter(draws=3, seed=2)
    args = (None, targets[:2], True, scene, 5, LOSS, DEV, SETUP)
    cam_g, prj_g = A.spaa(pcnet, clf, *args, iters=8, pose=ps)
    assert A.LAST_RUN == dict(iterations=8, graph=True)
    cam_2, prj_2 = A.spaa(pcnet, clf, *args, iters=8, pose=ps)
    assert A.LAST_RUN == dict(iterations=8, graph=True) and torch.equal(cam_2, cam_g) and torch.equal(prj_2, prj_g)
    monkeypatch.setattr(A, 'GRAPH_MAX_PIXELS', 0)
    cam_e, prj_e = A.spaa(pcnet, clf, *args, iters=8, pose=ps)
    assert A.LAST_RUN == dict(iterations=8, graph=False) and torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    monkeypatch.undo()
    tables = []
    for seed in (2, 3):
        st = A.PoseAttackState(pcnet, clf, targets[:2], scene, LOSS, SETUP, DEV, A.PoseJitter(draws=3, seed=seed))
        st.forward_decide(True, 5, P_THRESH)
        tables.append(st.table.cpu().numpy())
        del st
    assert not np.array_equal(tables[0], tables[1]) and _close_tables(tables[0], 2, 0, 2, 3, ps)
    # two configurations of two samples, max_batch = 2: each is a chunk of its own, in spaa()'s batch order, with the same seed
    cfgs = [(LOSS, 5, True, targets[:2]), (LOSS, 9, False, targets[2:4])]
    res = A.spaa_sweep(pcnet, clf, None, scene, SETUP, DEV, cfgs, iters=6, max_batch=2, pose=ps)
    assert A.LAST_RUN == dict(iterations=6, graph=True)
    for (cam, prj), (loss, d_thr, targeted, tg) in zip(res, cfgs):
        want = A.spaa(pcnet, clf, None, tg, targeted, scene, d_thr, loss, DEV, SETUP, iters=6, pose=ps)
        assert torch.equal(cam, want[0]) and torch.equal(prj, want[1])
    # pose=None is the plain attack: the keyword changes nothing there
    one = A.spaa(pcnet, clf, *args, iters=6)
    same = A.spaa(pcnet, clf, *args, iters=6, pose=None)
    assert torch.equal(one[0], same[0]) and torch.equal(one[1], same[1])
    assert not torch.equal(one[1], A.spaa(pcnet, clf, *args, iters=6, pose=ps)[1])
    # the verbose line counts draws
    capsys.readouterr()
    A.spaa(pcnet, clf, *args, iters=2, pose=ps, verbose=True)
    assert 'of 3 draws fooled' in capsys.readouterr().out


def test_pose_with_jitter_and_with_transfer(hip, pcnet, clf, case):
    """pose + jitter: draw j is Jitter_j(Pose_j(y)) from the kernels' own tables, at the forward bar times the largest gain plus the
    jitter test's 2e-6 (D here is the largest step between adjacent pixels of y with its zero fill: the border is part of the sampled
    image), draw 0 is floor(y 255) / 255 with the 8-bit step; unequal draws raise.  pose + Transfer runs and accumulates momentum."""
    A = hip['attack']
    _, scene, _, targets = case
    J, B = 3, 4
    ps = A.PoseJitter(draws=J, seed=4)
    jt = A.CaptureJitter(draws=J, seed=4, quantize=False)
    st = A.PoseAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, ps, jitter=jt)
    st.iteration(TARGETED, D_THR, 2, 1, P_THRESH)
    assert int(st.counter.item()) == 1 and int(st.jitter_counter.item()) == 1
    table, jit = st.table.cpu().numpy().astype(np.float64), st.jit.cpu().numpy().astype(np.float64)
    key = st.key.cpu().numpy().view(np.uint32)
    assert np.array_equal(jit[:, 0], np.tile(jo.IDENTITY_ROW, (B, 1))) and np.array_equal(table[:, 0], np.tile(po.IDENTITY_ROW, (B, 1)))
    assert np.array_equal(key, jo.draw_tables(4, 0, B, J, jt.gain, jt.offset, jt.shift, jt.noise, True)[1])
    assert not np.allclose(table[:, 1:, 2], jit[:, 1:, 4])                     # (one seed, independent tables)
    y = st._y.cpu().numpy()
    D = max(np.abs(np.diff(np.pad(y[..., :3], ((0, 0), (1, 1), (1, 1), (0, 0))), axis=a)).max() for a in (1, 2))
    bar = jit[..., :3].max() * (2 * po.eps_c(*SZ) * D + 8 * U) + 2e-6
    warped = po.forward(y, table)
    worst = 0.0
    for j in range(J):
        want = jo.forward(warped[j], jit[:, j:j + 1], key[:, j:j + 1], False)[0][0]
        worst = max(worst, np.abs(st.draw_ims[j].cpu().numpy() - want).max())
    print(f'pose + jitter: max |draw - Jitter_j(Pose_j(y))| = {worst:.3e}, bar {bar:.3e} (D = {D:.3f})')
    assert worst <= bar
    assert all(torch.isfinite(g).all() for g in st.pose_grads) and any(g.any() for g in st.pose_grads[1:])
    # the adjoint chain: spaa_jitter_bwd of the engines' gradients, then the pose adjoint
    g_eng = np.stack([e.g_y.cpu().numpy() for e in st.clfs])
    gates = np.stack([g.cpu().numpy().reshape(B, *SZ) for g in st.draw_gates])
    mid = jo.backward(g_eng, jit, gates)
    pulled = po.backward(mid, table)
    err = max(np.abs(st.pose_grads[j][b].cpu().numpy() - pulled[j, b]).max() / np.abs(mid[j, b]).max() for j in range(J) for b in range(B))
    # (the jitter adjoint's 2e-6 passes through the pose adjoint, whose weights onto one pixel sum to less than 2 at these ranges)
    print(f'pose + jitter: pulled-back gradients against the float64 chain: {err:.3e} of max |g| (bar {BWD_BAR + 4e-6:.3e})')
    assert err <= BWD_BAR + 4e-6
    # with the camera's 8-bit step, draw 0 is the clean capture behind it
    st = A.PoseAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, ps, jitter=A.CaptureJitter(draws=J, seed=4))
    st.forward_decide(TARGETED, D_THR, P_THRESH)
    assert torch.equal(st.draw_ims[0][..., :3], (torch.floor(st._y * 255.0) / torch.full((), 255.0, device=DEV))[..., :3])
    with pytest.raises(ValueError, match='draws'):
        A.spaa(pcnet, clf, None, targets[:2], True, scene, 5, LOSS, DEV, SETUP, pose=ps, jitter=A.CaptureJitter(draws=2))
    cam, prj = A.spaa(pcnet, clf, None, targets[:2], True, scene, 5, LOSS, DEV, SETUP, iters=5, pose=ps, jitter=jt)
    assert A.LAST_RUN == dict(iterations=5, graph=True) and torch.isfinite(cam).all() and torch.isfinite(prj).all()
    # pose + Transfer: one iteration leaves momentum behind for the samples on the adversarial step
    st = A.PoseAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, ps, transfer=A.Transfer(0.9, 1.0))
    st.iteration(TARGETED, D_THR, 2, 1, P_THRESH)
    assert st.momentum.any() and torch.isfinite(st.momentum).all() and torch.isfinite(st.x).all()


def test_pose_survival(hip, pcnet, clf, case):
    A = hip['attack']
    lib = hip['lib']
    _, scene, _, targets = case
    crop = SETUP['classifier_crop_sz']
    ps = A.PoseJitter(draws=2, seed=1)
    res = A.spaa_sweep(pcnet, clf, None, scene, SETUP, DEV, [(LOSS, 5, True, targets[:2])], iters=12, pose=ps)
    cams = torch.cat((res[0][0], scene.to(DEV).reshape(1, 3, *SZ)))             # two attacked captures and the plain scene
    tgt, tg = targets[:2] + [UNTARGETED_OTHER], [True, True, False]
    succ = A.attack_transfer(cams, [clf], tgt, tg, crop)[:, 0]
    assert succ[2]                                                              # (the scene is not class UNTARGETED_OTHER)
    # the zero-range pose: every capture is the image itself
    zero = A.pose_survival(cams, clf, tgt, tg, crop, A.PoseJitter(draws=2, **ZERO), draws=6)
    assert zero.shape == (3,) and np.array_equal(zero, succ.astype(zero.dtype))
    # a real pose: in [0, 1], repeatable with one seed; with a jitter behind it too
    wide = A.PoseJitter(rotate=6.0, zoom=0.1, shift=4.0, tilt=0.05)
    draws = 8
    got = A.pose_survival(cams, clf, tgt, tg, crop, wide, draws=draws, seed=3)
    again = A.pose_survival(cams, clf, tgt, tg, crop, wide, draws=draws, seed=3)
    assert got.shape == (3,) and (got >= 0).all() and (got <= 1).all() and np.array_equal(got, again)
    both = A.pose_survival(cams, clf, tgt, tg, crop, wide, draws=4, seed=3, jitter=A.CaptureJitter())
    assert both.shape == (3,) and (both >= 0).all() and (both <= 1).all()
    # the planted case: the same fraction through the float64 warp from the kernel's own tables (rounds of four, clean0 = 0)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    table = torch.zeros(3, 4, 8, device=DEV)
    y = cams.permute(0, 2, 3, 1).cpu().numpy()
    hits, gap = np.zeros(3), np.inf
    for _ in range(draws // 4):
        lib.call('spaa_pose_draw', 3, lib.ptr(counter), wide.rotate, wide.zoom, wide.shift, wide.tilt, 0, lib.ptr(table), 3, 4, *SZ)
        assert (table[:, 0, 0] != 1).any()
        out = po.forward(y, table.cpu().numpy().astype(np.float64))
        for j in range(4):
            im = torch.from_numpy(out[j, ..., :3]).permute(0, 3, 1, 2).float().contiguous().to(DEV)
            raw = clf(im, crop)[0].double().cpu()
            top2 = raw.sort(dim=1).values[:, -2:]
            gap = min(gap, float((top2[:, 1] - top2[:, 0]).min()))
            hits += jo.survives(raw.numpy(), tgt, tg)
    print(f'pose_survival: {got.tolist()}, through the float64 warp {(hits / draws).tolist()}, smallest top-2 gap {gap:.3e}')
    assert gap > 1e-3, 'the planted case is near a tie: choose another seed'
    assert np.array_equal(got, (hits / draws).astype(got.dtype))
