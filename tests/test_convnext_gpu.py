"""GPU: Classifier('convnext_tiny') against the float64 restatement of tests/convnext_oracle.py at that file's two geometries (a
narrow, shallow network of torchvision's key layout; the 'odd' geometry has odd maps at the first two downsamples and maps smaller than
the 7 x 7 window from the second stage on) and at torchvision's real widths and depths, and through the call sites the other bodies
serve.  The bars are those of tests/test_vit_gpu.py and tests/test_mobilenet_gpu.py: logits 1e-5 relative L-inf, input gradient at the
camera frame 1e-4 relative L2 per sample.  There are no gates to reconcile: LayerNorm and GELU are smooth, so the plain float64
gradient is the reference for every sample."""
import numpy as np
import pytest
import torch

import attention_oracle as ao
import convnext_oracle as co
import spaa_oracle as so
from spaa_amd import synthetic as syn
from spaa_amd.models import to_nchw
from test_gpu_parity import hip, make_pcnet, rel_inf, rel_l2  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSS = 'camdE_caml2'
P_THRESH = 0.9


@pytest.fixture(scope='module')
def clfs(hip):
    return {g: hip['clf'].Classifier('convnext_tiny', DEV, state_dict=co.state_dict(), input_sz=co.GEOMS[g][2]) for g in co.GEOMS}


def check_against_the_oracle(clf, sd, im, geom, what):
    """Logits and the camera-frame gradient of a random combination of them, HIP against float64; returns the body that ran."""
    (h, w), crop, insz = geom
    b = im.shape[0]
    r = torch.randn(b, co.NUM_CLASSES, generator=torch.Generator().manual_seed(1))
    im2 = im.clone().to(DEV).requires_grad_(True)
    raw2, p2, idx2 = clf(im2, crop)
    (raw2 * r.to(DEV)).sum().backward()
    im64 = im.double().requires_grad_(True)
    raw = co.forward(co.to64(sd), so.classifier_preprocess(im64, crop, insz))
    (raw * r.double()).sum().backward()
    e_logits = rel_inf(raw2, raw)
    grads = [rel_l2(im2.grad[i], im64.grad[i]) for i in range(b)]
    co.note(f'convnext_tiny {what}: logits rel Linf {e_logits:.2e} (bar 1e-5); input-gradient rel L2 per sample '
          f'{["%.2e" % g for g in grads]} (bar 1e-4)')
    assert float(im64.grad.abs().max()) > 0 and torch.isfinite(im2.grad).all()
    assert e_logits < 1e-5
    p = torch.softmax(raw.detach(), dim=1)
    assert (idx2[:, 0] == p.argmax(dim=1).numpy()).all() and np.allclose(p2[:, 0], p.max(dim=1).values.numpy(), atol=1e-5)
    assert all(e < 1e-4 for e in grads)
    return clf.engine(b, (h, w), crop).body


@pytest.mark.parametrize('geom', list(co.GEOMS))
def test_logits_and_input_gradient_against_the_oracle(hip, clfs, geom):
    clf = clfs[geom]
    assert clf.num_classes == co.NUM_CLASSES and clf.has_feature_map
    body = check_against_the_oracle(clf, co.state_dict(), co.images(geom), co.GEOMS[geom], geom)
    assert (body.P, body.dims, body.depths) == (4, co.DIMS, co.DEPTHS) and len(body.blocks) == sum(co.DEPTHS)
    assert tuple(body.feat.shape[1:3]) == ((2, 2) if geom == 'square' else (1, 1))
    dw = sum(2 * 49 * co.B * blk['d'].shape[1] * blk['d'].shape[2] * blk['d'].shape[3] for blk in body.blocks)
    assert body.flops_dw() == dw and body.flops_fwd() == sum(pl.flops(co.B, a, b) for pl, (a, b) in body.fwd_plans()) + dw
    body.refresh_masks()                                                       # (nothing to do, and it says so by doing nothing)
    assert not body.body_masks_switch


def test_real_widths_and_depths_against_the_oracle(hip):
    """torchvision's widths (96, 192, 384, 768) and depths (3, 3, 9, 3) at B = 2 on a 64 x 64 input: C = 768 and the 9-block stage."""
    sd = co.state_dict(full=True)
    geom = co.GEOMS['square']
    clf = hip['clf'].Classifier('convnext_tiny', DEV, state_dict=sd, input_sz=geom[2])
    body = check_against_the_oracle(clf, sd, co.images('square')[:2], geom, 'real widths')
    assert body.dims == (96, 192, 384, 768) and body.depths == (3, 3, 9, 3) and tuple(body.feat.shape) == (2, 2, 2, 768)


def test_grad_cam_against_the_oracle(hip, clfs):
    """Classifier.grad_cam against the float64 Grad-CAM of the oracle's last feature map, within the bound that the body's own feature
    and gradient errors give (the tolerance of tests/test_attention_gpu.py, as tests/test_mobilenet_gpu.py applies it)."""
    (h, w), crop, insz = co.GEOMS['square']
    clf, ims, classes = clfs['square'], co.images('square').to(DEV), [3, 7, 12]
    M = clf.grad_cam(ims, classes, crop)
    assert M.shape == (co.B, 1, h, w) and M.dtype == torch.float32 and M.is_cuda and M.min() >= 0 and M.max() <= 1
    eng = clf.engine(co.B, (h, w), crop)
    assert eng._cam is not None and eng._cam['valid']
    seed = np.zeros((co.B, co.NUM_CLASSES))
    seed[np.arange(co.B), classes] = 1.0
    rec = {}
    logits = co.forward(co.to64(co.state_dict()), so.classifier_preprocess(ims.cpu().double(), crop, insz).requires_grad_(True), record=rec)
    rec['feat'].retain_grad()
    (torch.from_numpy(seed) * logits).sum().backward()
    A_ref, G_ref = rec['feat'].detach().numpy(), rec['feat'].grad.numpy()
    sd_ = ao.seeds(seed, classes)
    ref = ao.cam(A_ref, G_ref, sd_)
    A, G, pooled = eng.body.attention_source()
    assert pooled and A is eng.body.feat and G is eng.body.g_pooled
    A = A.detach().cpu().double().numpy()
    G = np.broadcast_to(G.detach().cpu().double().numpy().reshape(co.B, 1, 1, -1) / (A.shape[1] * A.shape[2]), A.shape)
    C = A.shape[3]
    alpha = np.sign(sd_)[:, None] * G.mean(axis=(1, 2))
    e_A = np.abs(A - A_ref).reshape(co.B, -1).max(axis=1)
    e_al = np.abs(alpha - ref['alpha']).max(axis=1)
    bc = (np.abs(ref['alpha']).sum(axis=1) * e_A)[:, None, None] + e_al[:, None, None] * np.abs(A_ref).sum(axis=3) \
        + (C * e_al * e_A)[:, None, None] + ao.bound_c(ref, C)
    worst = bc.reshape(co.B, -1).max(axis=1)
    tm = ao.tol_map(ref, bc)
    Mref = ao.camera_map(ref['m'], (h, w), crop)
    errM = np.abs(M.detach().cpu().double().numpy()[:, 0] - Mref).reshape(co.B, -1).max(axis=1)
    co.note(f'convnext_tiny grad_cam: e_A {e_A.tolist()}, e_alpha {e_al.tolist()}, |M - M_ref| {errM.tolist()}, tolerance {tm.tolist()}')
    assert ((ref['cmax'] > 8 * worst) | (ref['pre'].reshape(co.B, -1).max(axis=1) < -worst)).all(), 'ill-conditioned case: choose other classes'
    assert (errM <= tm).all()
    assert torch.equal(clf.grad_cam(ims, classes, crop), M)
    assert torch.equal(clf.relevance(ims, classes, crop), M)                    # a convolutional body: relevance() is grad_cam()


SZ = (64, 64)
CROP = (60, 60)
SETUP = dict(classifier_crop_sz=CROP, prj_brightness=0.5, prj_im_sz=SZ)
TARGETS = [3, 7, 12]
INSZ = co.GEOMS['square'][2]


@pytest.fixture(scope='module')
def pcnet(hip):
    return make_pcnet(hip, syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect'), SZ)


@pytest.fixture(scope='module')
def clf(clfs):
    return clfs['square']


@pytest.fixture(scope='module')
def r18(hip):
    return hip['clf'].Classifier('resnet18', DEV, state_dict=syn.resnet18_state_dict(2, num_classes=co.NUM_CLASSES, logit_gain=20.0),
                                 input_sz=(56, 56))


def scene():
    return syn.scenes(1, 1, SZ)


def _args(targets=TARGETS):
    return (None, targets, True, scene(), 5, LOSS, DEV, SETUP)


def test_one_attack_iteration_against_the_oracle(hip, pcnet, clf):
    """One iteration of a plain spaa() of 3 targets from the initial (grey) state against the oracle's loop with the wrapped float64
    network: the decision table, and the updated projector image to 1e-4 relative L-inf on every sample whose decisions agree and whose
    PCNet gates agree with the oracle's (tests/gates.py: PCNet's ReLUs are the only gates on the path).  At least one sample must
    qualify, as tests/test_mobilenet_gpu.py demands."""
    import gates as G
    A = hip['attack']
    psd = syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect')
    sd64 = co.to64(co.state_dict())
    d_thr = 5.0
    st = A.AttackState(pcnet, clf, TARGETS, scene(), LOSS, SETUP, DEV)
    st.forward_decide(True, d_thr, P_THRESH)
    x0 = torch.full((co.B, 3, *SZ), 0.5)
    scene_b = scene().expand(co.B, -1, -1, -1)
    with torch.no_grad():
        xw = so.warp(psd, x0, SZ) * psd['mask']
        _, acts = so.shading_net(psd, xw, (scene_b, xw * scene_b), return_all=True)
    pflips, _ = G.count_flips(G.pcnet_pairs(st.eng, acts))
    state, stats = st.state.cpu().numpy(), st.stats.cpu().numpy()
    st.backward_step(2, 1)
    x1 = to_nchw(st.x).cpu()
    tr = []
    so.spaa(psd, co.classifier(sd64, INSZ), TARGETS, True, scene(), d_thr, LOSS, SETUP, iters=1, trace=tr)
    t = tr[0]
    err = torch.tensor([rel_inf(x1[b], torch.from_numpy(t['prj_adv'])[b]) for b in range(co.B)])
    co.note(f'convnext_tiny attack iteration: x rel Linf per sample {err.tolist()} (bar 1e-4); PCNet gate flips {pflips.tolist()}; '
          f'top-1 {state[:, 3].tolist()}, p1 {stats[:, 0].tolist()}')
    edge = (np.abs(t['p1'] - P_THRESH) < 1e-3) | (np.abs(t['caml2'] * 255 - d_thr) < 1e-2)
    assert ((state[:, 3] == t['top1']) | edge).all()
    assert ((state[:, 0] == t['succ']) | edge).all() and ((state[:, 1] == t['best_adv']) | edge).all()
    assert ((state[:, 2] == t['best']) | edge).all()
    assert np.allclose(stats[:, 0], t['p1'], atol=2e-4) and np.allclose(stats[:, 6], t['target_logit'], rtol=1e-4, atol=1e-4)
    assert np.allclose(stats[:, 1], t['caml2'], rtol=1e-4) and np.allclose(stats[:, 2], t['camdE'], rtol=1e-4)
    clean = torch.from_numpy(state[:, 1] == t['best_adv']) & (pflips == 0)
    assert clean.any(), 'vacuous: every sample has a PCNet gate within rounding of zero; choose another scene'
    assert (err[clean] < 1e-4).all()


def test_eager_graph_and_repeated_runs_agree(hip, pcnet, clf):
    """An iteration with this body captures and replays as a HIP graph, bitwise equal to the eager iteration."""
    A = hip['attack']
    cam_g, prj_g = A.spaa(pcnet, clf, *_args(), iters=5)
    assert A.LAST_RUN == dict(iterations=5, graph=True)
    cam_2, prj_2 = A.spaa(pcnet, clf, *_args(), iters=5)
    assert A.LAST_RUN == dict(iterations=5, graph=True) and torch.equal(cam_2, cam_g) and torch.equal(prj_2, prj_g)
    tr = []
    cam_e, prj_e = A.spaa(pcnet, clf, *_args(), iters=5, trace=tr)
    assert A.LAST_RUN == dict(iterations=5, graph=False) and len(tr) == 5
    assert torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    assert cam_g.shape == (co.B, 3, *SZ) and prj_g.shape == (co.B, 3, *SZ) and torch.isfinite(prj_g).all()
    assert all(torch.isfinite(stats).all() for _, stats in tr) and not torch.equal(tr[0][1], tr[4][1])      # the attack moves
    out = A.spaa_sweep(pcnet, clf, None, scene(), SETUP, DEV, [(LOSS, 5.0, True, TARGETS[:2]), ('caml2', 9.0, False, [5])], iters=2)
    assert len(out) == 2 and out[0][1].shape == (2, 3, *SZ) and out[1][1].shape == (1, 3, *SZ)


def consistent_with_classify(A, clf, cam, targets):
    """The loop's own decision (transfer_success) on the camera images `cam` agrees with clf.classify on them."""
    got = A.transfer_success(cam, clf, targets, True, CROP, P_THRESH)
    p = torch.softmax(clf(cam, CROP)[0], dim=1)
    want = (p.argmax(dim=1).cpu() == torch.tensor(targets)) & (p.max(dim=1).values.cpu() > P_THRESH)
    assert got.dtype == bool and got.tolist() == want.tolist()


def test_attention_weighted_attack(hip, pcnet, clf):
    A = hip['attack']
    cam, prj = A.spaa(pcnet, clf, *_args(), iters=2, attention=A.Attention(0.25))
    assert cam.shape == (co.B, 3, *SZ) and prj.shape == (co.B, 3, *SZ) and torch.isfinite(prj).all() and torch.isfinite(cam).all()
    consistent_with_classify(A, clf, cam, TARGETS)


def test_second_member_of_an_ensemble_with_resnet18(hip, pcnet, clf, r18):
    A = hip['attack']
    st = A.EnsembleAttackState(pcnet, [r18, clf], TARGETS, scene(), [LOSS] * 3, SETUP, DEV)
    st.iteration(True, 5.0, 2, 1, P_THRESH)
    state, stats, ens_state, ens_stats = st.trace_entry()
    assert state.shape == (co.B, 4) and stats.shape == (co.B, 8) and ens_state.shape == (co.B, 2, 2) and ens_stats.shape == (co.B, 2, 2)
    assert torch.isfinite(st.x).all() and torch.isfinite(st.g_adv).all() and st.g_adv.any()
    cam, prj = A.spaa(pcnet, [r18, clf], *_args(), iters=2)
    assert prj.shape == (co.B, 3, *SZ) and torch.isfinite(prj).all() and torch.isfinite(cam).all()
    consistent_with_classify(A, clf, cam, TARGETS)


def test_jitter_with_two_draws(hip, pcnet, clf):
    A = hip['attack']
    st = A.JitterAttackState(pcnet, clf, TARGETS, scene(), [LOSS] * 3, SETUP, DEV, A.CaptureJitter(draws=2, seed=3))
    st.iteration(True, 5.0, 2, 1, P_THRESH)
    assert torch.isfinite(st.x).all() and torch.isfinite(st.g_adv).all() and st.g_adv.any()
    cam, prj = A.spaa(pcnet, clf, *_args(), iters=2, jitter=A.CaptureJitter(draws=2, seed=1))
    assert prj.shape == (co.B, 3, *SZ) and torch.isfinite(prj).all() and torch.isfinite(cam).all()
    consistent_with_classify(A, clf, cam, TARGETS)


def test_transfer_success_with_convnext_held_out(hip, pcnet, clf, r18):
    """transfer_success is the loop's own decision for this body's own attack, and takes it as the held-out model of a ResNet-18 attack."""
    A = hip['attack']
    targets, targeted, d_thr = [3, 7, 12], [True, False, False], [5.0, 9.0, 5.0]
    st = A.AttackState(pcnet, clf, targets, scene(), [LOSS] * 3, SETUP, DEV)
    for _ in range(3):
        st.iteration(targeted, d_thr, 2, 1, P_THRESH)
    st.forward_decide(targeted, d_thr, P_THRESH)
    y = to_nchw(st._y).clone()
    state, stats = st.state.cpu(), st.stats.cpu()
    own = torch.where(torch.tensor(targeted), (state[:, 0] != 0) & (stats[:, 0] > P_THRESH), state[:, 0] != 0)
    got = A.transfer_success(y, clf, targets, targeted, CROP, P_THRESH)
    assert got.dtype == bool and got.shape == (3,) and got.tolist() == own.tolist()
    cam, _ = A.spaa(pcnet, r18, *_args(), iters=3)
    consistent_with_classify(A, clf, cam, TARGETS)


def test_f16_storage_is_refused_before_any_allocation(hip, clf):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(NotImplementedError, match='ConvNeXtBody'):
        clf.engine(co.B, SZ, CROP, storage='f16')
    assert torch.cuda.memory_allocated() == before                              # refused before anything is allocated
    assert all(k[3] != 'f16' or not v for k, v in clf._engines.items())         # ... and no half-built engine is kept
