"""GPU: Classifier('vit_b_16') against the float64 restatement of tests/vit_oracle.py at that file's three geometries (two small
widths with non-square patch grids, one with the real widths D = 768, M = 3072, dh = 64), and through the call sites the other bodies
serve.  The bars are those of tests/test_mobilenet_gpu.py: logits 1e-5 relative L-inf, input gradient at the camera frame 1e-4 relative
L2 per sample.  There are no gates to reconcile: GELU is smooth, so the gradient is a continuous function of the input and the plain
float64 gradient is the reference for every sample.  tests/test_vit_cpu.py shows that torch's own fp32 pass stays 5 to 50 times inside
these bars on the same inputs, and that the oracle's mutations are far outside them."""
import numpy as np
import pytest
import torch

import spaa_oracle as so
import vit_oracle as vo
from spaa_amd import synthetic as syn
from spaa_amd.models import to_nchw
from test_gpu_parity import hip, make_pcnet, rel_inf, rel_l2  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSS = 'camdE_caml2'
P_THRESH = 0.9
ATTACK_GEOM = 'wide'          # the network of the attack tests: two layers, a 4 x 6 patch grid


@pytest.fixture(scope='module')
def clfs(hip):
    return {g: hip['clf'].Classifier('vit_b_16', DEV, state_dict=vo.state_dict(g), input_sz=vo.GEOMS[g][2]) for g in vo.GEOMS}


@pytest.mark.parametrize('geom', list(vo.GEOMS))
def test_logits_and_input_gradient_against_the_oracle(hip, clfs, geom):
    (h, w), crop, insz, P, D, depth, M = vo.GEOMS[geom]
    clf = clfs[geom]
    assert clf.num_classes == vo.NUM_CLASSES
    im = vo.images(geom)
    r = torch.randn(vo.B, vo.NUM_CLASSES, generator=torch.Generator().manual_seed(1))
    im2 = im.clone().to(DEV).requires_grad_(True)
    raw2, p2, idx2 = clf(im2, crop)
    (raw2 * r.to(DEV)).sum().backward()
    body = clf.engine(vo.B, (h, w), crop).body
    assert (body.D, body.depth, body.M, body.P, body.T, body.dh) == (D, depth, M, P, (insz[0] // P) * (insz[1] // P) + 1, D // 12)
    assert body.flops_fwd() == sum(pl.flops(vo.B, a, b) for pl, (a, b) in body.fwd_plans()) + 4 * depth * vo.B * body.T ** 2 * D
    sd64 = vo.to64(vo.state_dict(geom))
    im64 = im.double().requires_grad_(True)
    raw = vo.forward(sd64, so.classifier_preprocess(im64, crop, insz))
    (raw * r.double()).sum().backward()
    e_logits = rel_inf(raw2, raw)
    grads = [rel_l2(im2.grad[b], im64.grad[b]) for b in range(vo.B)]
    print(f'{geom}: logits rel Linf {e_logits:.2e}; input-gradient rel L2 per sample {grads}')
    assert float(im64.grad.abs().max()) > 0 and torch.isfinite(im2.grad).all()
    assert e_logits < 1e-5
    p = torch.softmax(raw.detach(), dim=1)
    assert (idx2[:, 0] == p.argmax(dim=1).numpy()).all() and np.allclose(p2[:, 0], p.max(dim=1).values.numpy(), atol=1e-5)
    assert all(e < 1e-4 for e in grads)
    # the head's gradient buffer: every row but the class tokens' is still the zero it was allocated as
    assert not body.g_top[:, 1:].any() and body.g_top[:, 0].any()


PLAN_SHAPES = [(96, 288), (96, 96), (96, 384), (384, 96), (256, 96), (64, 96),                 # the small widths (patch rows: 4 P^2 = 256, 64)
               (768, 2304), (768, 768), (768, 3072), (3072, 768), (1024, 768)]                 # the real widths (patch rows: 1024)


@pytest.mark.parametrize('T', (5, 197))
@pytest.mark.parametrize('K,N', PLAN_SHAPES)
def test_token_map_plans_against_float64(hip, K, N, T):
    """The 1 x 1 plans on the token layout the body uses -- a map of height T and width 1 per sample -- forward with a residual add and
    input gradient, against float64 at the 1e-5 relative L-inf the logits are held to."""
    cp = hip['cp']
    gen = torch.Generator().manual_seed(K * 7 + N + T)
    b = 2
    wt = torch.randn(N, K, 1, 1, generator=gen) / K ** 0.5
    bias = torch.randn(N, generator=gen)
    x = torch.randn(b, T, 1, K, generator=gen)
    add = torch.randn(b, T, 1, N, generator=gen)
    out = torch.zeros(b, T, 1, N, device=DEV)
    cp.conv_fwd_plan(wt, bias, 1, 0, DEV, 'token').run(x.to(DEV), out, add=add.to(DEV))
    ref = torch.einsum('bhwc,oc->bhwo', x.double(), wt.double()[:, :, 0, 0]) + bias.double() + add.double()
    e = rel_inf(out, ref)
    g = torch.randn(b, T, 1, N, generator=gen)
    g_in = torch.zeros(b, T, 1, K, device=DEV)
    cp.conv_dgrad_plan(wt, 1, 0, DEV, 'token_dgrad').run(g.to(DEV), g_in)
    eg = rel_inf(g_in, torch.einsum('bhwo,oc->bhwc', g.double(), wt.double()[:, :, 0, 0]))
    print(f'1x1 {K} -> {N}, T = {T}: forward rel Linf {e:.2e}, input gradient {eg:.2e}')
    assert e < 1e-5 and eg < 1e-5


SZ = (64, 64)
CROP = (60, 60)
SETUP = dict(classifier_crop_sz=CROP, prj_brightness=0.5, prj_im_sz=SZ)
TARGETS = [3, 7, 12]
INSZ = vo.GEOMS[ATTACK_GEOM][2]


@pytest.fixture(scope='module')
def pcnet(hip):
    return make_pcnet(hip, syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect'), SZ)


@pytest.fixture(scope='module')
def clf(clfs):
    return clfs[ATTACK_GEOM]


def scene():
    return syn.scenes(1, 1, SZ)


def test_one_attack_iteration_against_the_oracle(hip, pcnet, clf):
    """One iteration of AttackState from the initial (grey) state against the oracle's spaa() with the wrapped float64 ViT: the decision
    table, and the updated projector image to 1e-4 relative L-inf on every sample whose PCNet gates agree with the oracle's
    (tests/gates.py: PCNet's ReLUs are the only gates on the path)."""
    import gates as G
    A = hip['attack']
    psd = syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect')
    sd64 = vo.to64(vo.state_dict(ATTACK_GEOM))
    d_thr = 5.0
    st = A.AttackState(pcnet, clf, TARGETS, scene(), LOSS, SETUP, DEV)
    st.forward_decide(True, d_thr, P_THRESH)
    x0 = torch.full((vo.B, 3, *SZ), 0.5)
    scene_b = scene().expand(vo.B, -1, -1, -1)
    with torch.no_grad():
        xw = so.warp(psd, x0, SZ) * psd['mask']
        _, acts = so.shading_net(psd, xw, (scene_b, xw * scene_b), return_all=True)
    pflips, _ = G.count_flips(G.pcnet_pairs(st.eng, acts))
    state, stats = st.state.cpu().numpy(), st.stats.cpu().numpy()
    st.backward_step(2, 1)
    x1 = to_nchw(st.x).cpu()
    tr = []
    so.spaa(psd, vo.classifier(sd64, INSZ), TARGETS, True, scene(), d_thr, LOSS, SETUP, iters=1, trace=tr)
    t = tr[0]
    err = torch.tensor([rel_inf(x1[b], torch.from_numpy(t['prj_adv'])[b]) for b in range(vo.B)])
    print(f'attack iteration: x rel Linf per sample {err.tolist()}; PCNet gate flips {pflips.tolist()}; top-1 {state[:, 3].tolist()}, '
          f'p1 {stats[:, 0].tolist()}')
    edge = (np.abs(t['p1'] - P_THRESH) < 1e-3) | (np.abs(t['caml2'] * 255 - d_thr) < 1e-2)
    assert ((state[:, 3] == t['top1']) | edge).all()
    assert ((state[:, 0] == t['succ']) | edge).all() and ((state[:, 1] == t['best_adv']) | edge).all()
    assert ((state[:, 2] == t['best']) | edge).all()
    assert np.allclose(stats[:, 0], t['p1'], atol=2e-4) and np.allclose(stats[:, 6], t['target_logit'], rtol=1e-4, atol=1e-4)
    assert np.allclose(stats[:, 1], t['caml2'], rtol=1e-4) and np.allclose(stats[:, 2], t['camdE'], rtol=1e-4)
    clean = torch.from_numpy(state[:, 1] == t['best_adv']) & (pflips == 0)
    assert clean.any(), 'vacuous: every sample has a PCNet gate within rounding of zero; choose another scene'
    assert (err[clean] < 1e-4).all()


def _args(targets=TARGETS):
    return (None, targets, True, scene(), 5, LOSS, DEV, SETUP)


def test_eager_graph_and_repeated_runs_agree(hip, pcnet, clf):
    A = hip['attack']
    cam_g, prj_g = A.spaa(pcnet, clf, *_args(), iters=5)
    assert A.LAST_RUN == dict(iterations=5, graph=True)
    cam_2, prj_2 = A.spaa(pcnet, clf, *_args(), iters=5)
    assert A.LAST_RUN == dict(iterations=5, graph=True) and torch.equal(cam_2, cam_g) and torch.equal(prj_2, prj_g)
    tr = []
    cam_e, prj_e = A.spaa(pcnet, clf, *_args(), iters=5, trace=tr)
    assert A.LAST_RUN == dict(iterations=5, graph=False) and len(tr) == 5
    assert torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    assert cam_g.shape == (vo.B, 3, *SZ) and prj_g.shape == (vo.B, 3, *SZ) and torch.isfinite(prj_g).all()
    assert all(torch.isfinite(stats).all() for _, stats in tr) and not torch.equal(tr[0][1], tr[4][1])      # the attack moves
    out = A.spaa_sweep(pcnet, clf, None, scene(), SETUP, DEV, [(LOSS, 5.0, True, TARGETS[:2]), ('caml2', 9.0, False, [5])], iters=2)
    assert len(out) == 2 and out[0][1].shape == (2, 3, *SZ) and out[1][1].shape == (1, 3, *SZ)


@pytest.fixture(scope='module')
def r18(hip):
    return hip['clf'].Classifier('resnet18', DEV, state_dict=syn.resnet18_state_dict(2, num_classes=vo.NUM_CLASSES, logit_gain=20.0),
                                 input_sz=(56, 56))


def test_ensemble_with_transfer(hip, pcnet, clf, r18):
    """One ensemble iteration of [vit_b_16, resnet18] with Transfer(0.9, 1.0): runs, documented shapes; and through spaa()."""
    A = hip['attack']
    st = A.EnsembleAttackState(pcnet, [clf, r18], TARGETS, scene(), [LOSS] * 3, SETUP, DEV, transfer=A.Transfer(0.9, 1.0))
    st.iteration(True, 5.0, 2, 1, P_THRESH)
    state, stats, ens_state, ens_stats = st.trace_entry()
    assert state.shape == (vo.B, 4) and stats.shape == (vo.B, 8) and ens_state.shape == (vo.B, 2, 2) and ens_stats.shape == (vo.B, 2, 2)
    assert st.momentum.shape == (vo.B, *SZ, 4) and st.momentum.any()
    assert torch.isfinite(st.x).all() and torch.isfinite(st.g_adv).all() and st.g_adv.any()
    cam, prj = st.results()
    assert cam.shape == (vo.B, 3, *SZ) and prj.shape == (vo.B, 3, *SZ)
    cam2, prj2 = A.spaa(pcnet, [clf, r18], *_args(), iters=2, transfer=A.Transfer(0.9, 1.0))
    assert prj2.shape == (vo.B, 3, *SZ) and torch.isfinite(prj2).all()


def test_transfer_success_with_the_vit_held_out(hip, pcnet, clf, r18):
    """transfer_success is the loop's own decision for the ViT's own attack, and takes the ViT as the held-out model of a ResNet-18 attack."""
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
    held = A.transfer_success(cam, clf, TARGETS, True, CROP, P_THRESH)
    raw = clf(cam, CROP)[0]
    p = torch.softmax(raw, dim=1)
    want = (p.argmax(dim=1).cpu() == torch.tensor(TARGETS)) & (p.max(dim=1).values.cpu() > P_THRESH)
    assert held.dtype == bool and held.tolist() == want.tolist()


def test_jitter_and_pose_iterations(hip, pcnet, clf):
    A = hip['attack']
    st = A.JitterAttackState(pcnet, clf, TARGETS, scene(), [LOSS] * 3, SETUP, DEV, A.CaptureJitter(draws=2, seed=3))
    st.iteration(True, 5.0, 2, 1, P_THRESH)
    assert torch.isfinite(st.x).all() and torch.isfinite(st.g_adv).all() and st.g_adv.any()
    sp = A.PoseAttackState(pcnet, clf, TARGETS, scene(), [LOSS] * 3, SETUP, DEV, A.PoseJitter(draws=2, seed=3))
    sp.iteration(True, 5.0, 2, 1, P_THRESH)
    assert torch.isfinite(sp.x).all() and torch.isfinite(sp.g_adv).all() and sp.g_adv.any()
    cam, prj = A.spaa(pcnet, clf, *_args(), iters=2, pose=A.PoseJitter(draws=2, seed=1), jitter=A.CaptureJitter(draws=2, seed=1))
    assert prj.shape == (vo.B, 3, *SZ) and torch.isfinite(prj).all()


def test_f16_storage_and_attention_are_refused_before_any_allocation(hip, pcnet, clf, r18):
    A = hip['attack']
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(NotImplementedError, match='ViTB16Body'):
        clf.engine(vo.B, SZ, CROP, storage='f16')
    assert all(k[3] != 'f16' or not v for k, v in clf._engines.items())               # no half-built engine is kept
    for c in (clf, [clf, r18], [r18, clf]):
        with pytest.raises(NotImplementedError, match='vit_b_16'):
            A.spaa(pcnet, c, *_args(), iters=2, attention=A.Attention(0.25))
    with pytest.raises(NotImplementedError, match='vit_b_16'):
        A.spaa_sweep(pcnet, clf, None, scene(), SETUP, DEV, [(LOSS, 5.0, True, TARGETS[:2])], iters=2, attention=A.Attention(0.25))
    with pytest.raises(NotImplementedError, match='no convolutional feature map'):
        clf.grad_cam(torch.rand(vo.B, 3, *SZ, device=DEV), TARGETS, CROP)
    assert torch.cuda.memory_allocated() == before
