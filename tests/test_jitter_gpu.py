"""GPU: the capture-jitter attack loop (JitterAttackState through spaa / spaa_sweep) on the 64 x 64 synthetic PCNet and the 56 x 56
ResNet-18 of the ensemble tests: one teacher-forced first iteration against the float64 oracle (tests/jitter_oracle.py), the
zero-range twin of the plain attack, twelve traced iterations whose sample tables must be the stated functions of the draw tables, the
eager / graph / repeat / sweep identities, and capture_survival."""
import numpy as np
import pytest
import torch

import ensemble_oracle as eo
import jitter_oracle as jo
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
ZERO = dict(gain=0.0, offset=0.0, shift=0.0, noise=0.0, quantize=False)


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


def _tables(st):
    return st.jit.cpu().numpy(), st.key.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('quantize', [False, True])
def test_first_iteration_against_the_oracle(hip, pcnet, clf, case, quantize):
    A = hip['attack']
    sd, scene, oc, targets = case
    J, B = 3, 4
    # (with the 8-bit step an fp32 image one rounding away from the float64 one can fall on the other side of a step at a few pixels:
    # measured, the target logits then still agree to 1.3e-5 at magnitude 56, as they do without the step, 2.1e-5)
    jt = A.CaptureJitter(draws=J, seed=11, quantize=quantize)
    st = A.JitterAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, jt)
    assert st.K == J and len({id(e) for e in st.clfs}) == J and len(clf._engines[(B, SZ, (60, 60), 'f32')]) >= J
    st.forward_decide(TARGETED, D_THR, P_THRESH)
    st.backward_step(2, 1)
    jit, key = _tables(st)
    assert int(st.counter.item()) == 1 and (jit[:, 0] == np.array(jo.IDENTITY_ROW, dtype=np.float32)).all()
    want_jit, want_key = jo.draw_tables(11, 0, B, J, jt.gain, jt.offset, jt.shift, jt.noise, True)
    assert np.array_equal(key, want_key) and np.abs(jit - want_jit).max() <= 3e-7
    # the three members: the float64 classifier behind the float64 transform with the state's OWN tables (teacher-forced)
    ref = jo.first_iteration(sd, oc, targets, TARGETED, scene, D_THR, SETUP, jit.astype(np.float64), key, jt.quantize, p_thresh=P_THRESH)
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
    assert (ew == 1).all()                                                     # (no focus: every draw pulls)
    print(f'quantize {quantize}: max |p1 - ref| / ref {np.abs(ef[..., 0] / ref["p1"] - 1).max():.3e}, max |target logit - ref| '
          f'{np.abs(ef[..., 1] - ref["tl"]).max():.3e} at max |ref| {np.abs(ref["tl"]).max():.3f}')
    assert np.allclose(ef[..., 0][clear], ref['p1'][clear], rtol=1e-3) and np.allclose(ef[..., 1], ref['tl'], rtol=1e-3, atol=1e-3)
    assert np.allclose(stats[:, 1], ref['caml2'], rtol=1e-4)                   # the stealth loss is the CLEAN capture's
    # wiring of the adjoint: the pulled-back gradients are spaa_jitter_bwd of the engines' own gradient images and gate bytes
    g_eng = np.stack([e.g_y.cpu().numpy() for e in st.clfs])
    gates = np.stack([g.cpu().numpy().reshape(B, *SZ) for g in st.draw_gates])
    pulled = jo.backward(g_eng, jit.astype(np.float64), gates).reshape(J, B, -1, 4)
    g_own = [g.reshape(B, -1, 4).cpu().numpy().astype(np.float64) for g in st.draw_grads]
    err = max(np.abs(g_own[j][b] - pulled[j, b]).max() / np.abs(pulled[j, b]).max() for j in range(J) for b in range(B))
    print(f'pulled-back gradients against the float64 adjoint of the engines\' own: {err:.3e}')
    assert err <= 2e-6
    # g_adv: the float64 combination of the pulled-back gradients the state itself produced
    g_adv = st.g_adv.reshape(B, -1, 4).cpu().numpy().astype(np.float64)
    own = eo.combine(g_own, ew)
    err = np.abs(g_adv - own).max(axis=(1, 2)) / np.abs(own).max(axis=(1, 2))
    print(f'g_adv against the float64 combination of the state\'s own pulled-back gradients, per sample {err.tolist()}')
    assert (err <= 2e-6).all() and (g_adv[..., 3] == 0).all()
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
    st = A.JitterAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, A.CaptureJitter(draws=2, **ZERO))
    st.iteration(TARGETED, D_THR, 2, 1, P_THRESH)
    plain = A.AttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV)
    plain.iteration(TARGETED, D_THR, 2, 1, P_THRESH)
    assert torch.equal(st.state[:, 0:3], plain.state[:, 0:3])
    dx = (st.x - plain.x).abs().max().item()
    print(f'zero-range twin: max |x - plain x| after one iteration = {dx:.3e}')
    assert dx <= 1e-5
    es = st.ens_state.cpu()
    assert torch.equal(es[:, 0], es[:, 1]) and torch.equal(st.ens_stats[:, 0], st.ens_stats[:, 1])
    assert torch.equal(st.draw_ims[0][..., :3], st._y[..., :3]) and torch.equal(st.draw_ims[1], st.draw_ims[0])


def test_twelve_traced_iterations(hip, pcnet, clf, case):
    """In every iteration state and stats are the stated functions of the draw tables, draw 0's table row is the identity row, the
    tables change; the device counter reads 12 afterwards."""
    A = hip['attack']
    _, scene, _, targets = case
    J, B = 3, 4
    st = A.JitterAttackState(pcnet, clf, targets, scene, [LOSS] * B, SETUP, DEV, A.CaptureJitter(draws=J, seed=5))
    targeted, d_thr, tgt = torch.tensor(TARGETED), torch.tensor(D_THR), torch.tensor(targets)
    best_before = torch.full((B,), 1e6)
    seen_col_step = seen_adv_step = False
    last_jit = None
    for i in range(12):
        st.iteration(TARGETED, D_THR, 2, 1, P_THRESH)
        entry = st.trace_entry()
        assert len(entry) == 4
        state, stats, es, ef = (t.cpu() for t in entry)
        jit = st.jit.cpu()
        assert torch.equal(jit[:, 0], torch.tensor(jo.IDENTITY_ROW).expand(B, 8)), i
        assert (jit[:, 1:, :3] != 1).all() and (last_jit is None or not torch.equal(jit, last_jit)), i
        last_jit = jit
        # draw 0 is the clean capture behind the camera's 8-bit step
        assert torch.equal(st.draw_ims[0][..., :3], (torch.floor(st._y * 255.0) / torch.full((), 255.0, device=DEV))[..., :3]), i
        assert state.shape == (B, 4) and stats.shape == (B, 8) and es.shape == (B, J, 2) and ef.shape == (B, J, 2)
        succ, fooled = (es[..., 0] & 1).bool(), (es[..., 0] & 2).bool()
        assert torch.equal(succ, torch.where(targeted[:, None], es[..., 1] == tgt[:, None], es[..., 1] != tgt[:, None])), i
        assert torch.equal(fooled, torch.where(targeted[:, None], succ & (ef[..., 0] > P_THRESH), succ)), i
        best_adv = fooled.all(dim=1) & (stats[:, 1] * 255.0 > d_thr)
        assert torch.equal(state[:, 0].bool(), succ.all(dim=1)) and torch.equal(state[:, 1].bool(), best_adv), i
        assert torch.equal(state[:, 3], fooled.sum(dim=1).int()), i
        assert torch.equal(stats[:, 0], ef[..., 0].min(dim=1).values), i
        tl = ef[..., 1].double()
        assert ((stats[:, 6].double() - tl.mean(dim=1)).abs() <= J * 2.0 ** -24 * tl.abs().sum(dim=1)).all(), i
        best = best_adv & (stats[:, 3] < best_before)
        assert torch.equal(state[:, 2].bool(), best), i
        assert torch.equal(stats[:, 5], torch.where(best, stats[:, 3], best_before)), i
        best_before = stats[:, 5].clone()
        seen_col_step |= bool(best_adv.any())
        seen_adv_step |= bool((~best_adv).any())
    assert seen_col_step and seen_adv_step                              # both steps were taken in this run
    assert int(st.counter.item()) == 12
    cam, prj = st.results()
    assert torch.isfinite(cam).all() and torch.isfinite(prj).all() and prj.min() >= 0 and prj.max() <= 1


def test_repeatability_and_sweep(hip, pcnet, clf, case, monkeypatch):
    """Eager and graph-replayed runs, and two runs with one seed, are bitwise equal; another seed gives other tables; the sweep returns
    per configuration what spaa() returns for it when each configuration is a chunk of its own."""
    A = hip['attack']
    _, scene, _, targets = case
    jt = A.CaptureJitter(draws=3, seed=2)
    args = (None, targets[:2], True, scene, 5, LOSS, DEV, SETUP)
    cam_g, prj_g = A.spaa(pcnet, clf, *args, iters=8, jitter=jt)
    assert A.LAST_RUN == dict(iterations=8, graph=True)
    cam_2, prj_2 = A.spaa(pcnet, clf, *args, iters=8, jitter=jt)
    assert A.LAST_RUN == dict(iterations=8, graph=True) and torch.equal(cam_2, cam_g) and torch.equal(prj_2, prj_g)
    monkeypatch.setattr(A, 'GRAPH_MAX_PIXELS', 0)
    cam_e, prj_e = A.spaa(pcnet, clf, *args, iters=8, jitter=jt)
    assert A.LAST_RUN == dict(iterations=8, graph=False) and torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    monkeypatch.undo()
    tables = []
    for seed in (2, 3):
        st = A.JitterAttackState(pcnet, clf, targets[:2], scene, LOSS, SETUP, DEV, A.CaptureJitter(draws=3, seed=seed))
        st.forward_decide(True, 5, P_THRESH)
        tables.append(_tables(st))
        del st
    assert not np.array_equal(tables[0][0], tables[1][0]) and not np.array_equal(tables[0][1], tables[1][1])
    assert np.array_equal(tables[0][1], jo.draw_tables(2, 0, 2, 3, jt.gain, jt.offset, jt.shift, jt.noise, True)[1])
    # two configurations of two samples, max_batch = 2: each is a chunk of its own, in spaa()'s batch order, with the same seed
    cfgs = [(LOSS, 5, True, targets[:2]), (LOSS, 9, False, targets[2:4])]
    res = A.spaa_sweep(pcnet, clf, None, scene, SETUP, DEV, cfgs, iters=6, max_batch=2, jitter=jt)
    assert A.LAST_RUN == dict(iterations=6, graph=True)
    for (cam, prj), (loss, d_thr, targeted, tg) in zip(res, cfgs):
        want = A.spaa(pcnet, clf, None, tg, targeted, scene, d_thr, loss, DEV, SETUP, iters=6, jitter=jt)
        assert torch.equal(cam, want[0]) and torch.equal(prj, want[1])
    # jitter=None is the plain attack: the keyword changes nothing there
    one = A.spaa(pcnet, clf, *args, iters=6)
    same = A.spaa(pcnet, clf, *args, iters=6, jitter=None)
    assert torch.equal(one[0], same[0]) and torch.equal(one[1], same[1])
    assert not torch.equal(one[1], A.spaa(pcnet, clf, *args, iters=6, jitter=jt)[1])


def test_capture_survival(hip, pcnet, clf, case):
    A = hip['attack']
    lib = hip['lib']
    _, scene, _, targets = case
    crop = SETUP['classifier_crop_sz']
    jt = A.CaptureJitter(draws=2, seed=1)
    res = A.spaa_sweep(pcnet, clf, None, scene, SETUP, DEV, [(LOSS, 5, True, targets[:2]), (LOSS, 5, False, targets[2:])], iters=12,
                       jitter=jt)
    cams = torch.cat((res[0][0], scene.to(DEV).reshape(1, 3, *SZ)))             # two attacked captures and the plain scene
    tgt, tg = targets[:2] + [UNTARGETED_OTHER], [True, True, False]
    succ = A.attack_transfer(cams, [clf], tgt, tg, crop)[:, 0]
    assert succ[2]                                                              # (the scene is not class UNTARGETED_OTHER)
    # the zero-range jitter: every capture is the image itself
    zero = A.capture_survival(cams, clf, tgt, tg, crop, A.CaptureJitter(draws=2, **ZERO), draws=6)
    assert zero.shape == (3,) and np.array_equal(zero, succ.astype(zero.dtype))
    assert A.capture_survival(cams[2:], clf, tgt[2:], False, crop, A.CaptureJitter(draws=2, **ZERO))[0] == 1.0
    # a real jitter: in [0, 1], repeatable with one seed
    wide = A.CaptureJitter(gain=0.3, offset=0.1, shift=2.0, noise=0.05, quantize=False)
    draws = 8
    got = A.capture_survival(cams, clf, tgt, tg, crop, wide, draws=draws, seed=3)
    again = A.capture_survival(cams, clf, tgt, tg, crop, wide, draws=draws, seed=3)
    assert got.shape == (3,) and (got >= 0).all() and (got <= 1).all() and np.array_equal(got, again)
    # the planted case: the same fraction through the oracle transform from the kernel's own tables (rounds of four, clean0 = 0)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    jit = torch.zeros(3, 4, 8, device=DEV)
    key = torch.zeros(3, 4, dtype=torch.int32, device=DEV)
    y = cams.permute(0, 2, 3, 1).cpu().numpy()
    hits, gap = np.zeros(3), np.inf
    for _ in range(draws // 4):
        lib.call('spaa_jitter_draw', 3, lib.ptr(counter), wide.gain, wide.offset, wide.shift, wide.noise, 0, lib.ptr(jit), lib.ptr(key),
                 3, 4)
        out, _, _ = jo.forward(y, jit.cpu().numpy().astype(np.float64), key.cpu().numpy().view(np.uint32), False)
        assert (jit[:, 0, :3] != 1).any()
        for j in range(4):
            im = torch.from_numpy(out[j, ..., :3]).permute(0, 3, 1, 2).float().contiguous().to(DEV)
            raw = clf(im, crop)[0].double().cpu()
            top2 = raw.sort(dim=1).values[:, -2:]
            gap = min(gap, float((top2[:, 1] - top2[:, 0]).min()))
            hits += jo.survives(raw.numpy(), tgt, tg)
    print(f'capture_survival: {got.tolist()}, through the oracle transform {(hits / draws).tolist()}, smallest top-2 gap {gap:.3e}')
    assert gap > 1e-3, 'the planted case is near a tie: choose another seed'
    assert np.array_equal(got, (hits / draws).astype(got.dtype))
