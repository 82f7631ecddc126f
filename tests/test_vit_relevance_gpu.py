"""GPU: the ViT's relevance rollout through the public interface -- Classifier.relevance against the float64
whole-network map of tests/vit_relevance_oracle.py (autograd's gradient at each layer's probabilities, the matrix form of the rollout:
a different formulation from the kernels' recurrence) on the fixtures of tests/vit_oracle.py, ClassifierEngine.backward with
Attention(f, rollout=True) against the same pass's plain gradient image, and the attack entry points with a ViT, alone and next to a
ResNet-18.

The bar of the map: 1e-4 absolute on M in [0, 1], the project's bar for a ViT input gradient, which M is a function of.  torch's own
fp32 evaluation of the restatement is within 0.5 - 3.5e-6 of float64 on these fixtures and the nearest mutation 3.2e-2 away
(tests/test_vit_relevance_cpu.py).  Both errors are printed as `accuracy:` lines (profiles/vit_relevance_accuracy.txt)."""
import numpy as np
import pytest
import torch

import attention_oracle as ao
import spaa_oracle as so
import vit_oracle as vo
import vit_relevance_oracle as ro
from spaa_amd import synthetic as syn
from spaa_amd.models import to_nhwc4
from test_gpu_parity import hip, make_pcnet  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = vo.U
LOSS = 'camdE_caml2'
P_THRESH = 0.9
TARGETS = [3, 7, 12]
MAP_BAR = 1e-4
ATTACK_GEOM = 'wide'
SZ = (64, 64)
CROP = (60, 60)
SETUP = dict(classifier_crop_sz=CROP, prj_brightness=0.5, prj_im_sz=SZ)


@pytest.fixture(scope='module')
def clfs(hip):
    return {g: hip['clf'].Classifier('vit_b_16', DEV, state_dict=vo.state_dict(g), input_sz=vo.GEOMS[g][2]) for g in vo.GEOMS}


@pytest.fixture(scope='module')
def clf(clfs):
    return clfs[ATTACK_GEOM]


@pytest.fixture(scope='module')
def pcnet(hip):
    return make_pcnet(hip, syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect'), SZ)


@pytest.fixture(scope='module')
def r18(hip):
    return hip['clf'].Classifier('resnet18', DEV, state_dict=syn.resnet18_state_dict(2, num_classes=vo.NUM_CLASSES, logit_gain=20.0),
                                 input_sz=(56, 56))


def scene():
    return syn.scenes(1, 1, SZ)


def inside_of(h, w, crop):
    """[h, w] bool on the device: the classifier crop of the camera frame."""
    cy0, cx0 = ao.center_crop_origin(h, w, crop)
    m = torch.zeros(h, w, dtype=torch.bool, device=DEV)
    m[cy0:cy0 + crop[0], cx0:cx0 + crop[1]] = True
    return m


def _args(targets=TARGETS):
    return (None, targets, True, scene(), 5, LOSS, DEV, SETUP)


@pytest.mark.parametrize('geom', list(vo.GEOMS))
def test_relevance_against_the_float64_map(hip, clfs, geom):
    (h, w), crop, insz, P = vo.GEOMS[geom][:4]
    gh, gw = insz[0] // P, insz[1] // P
    im = vo.images(geom)
    M = clfs[geom].relevance(im.to(DEV), TARGETS, crop)
    M2 = clfs[geom].relevance(im.to(DEV), TARGETS, crop)
    assert M.shape == (vo.B, 1, h, w) and M.dtype == torch.float32 and M.is_cuda and torch.equal(M, M2)
    x64 = so.classifier_preprocess(im, crop, insz).double()
    m, cmax = ro.network_map(vo.to64(vo.state_dict(geom)), x64, TARGETS)
    assert (cmax > 0).all(), 'the fixture does not decide its maps: choose other targets'
    ref = ao.camera_map(m.reshape(vo.B, gh, gw).numpy(), (h, w), crop)
    m32 = ro.network_map(vo.state_dict(geom), x64.float(), TARGETS)[0].double()
    e_cpu = float(np.abs(ao.camera_map(m32.reshape(vo.B, gh, gw).numpy(), (h, w), crop) - ref).max())
    got = M[:, 0].cpu().double().numpy()
    err = float(np.abs(got - ref).max())
    print(f'accuracy: Classifier.relevance {geom}: |M - M_float64| = {err:.2e} on the device, {e_cpu:.2e} for torch fp32 on the CPU '
          f'(bar {MAP_BAR}); float64 cmax {cmax.tolist()}')
    assert got.min() >= 0 and got.max() <= 1 and np.isfinite(got).all()
    assert (got[:, ~inside_of(h, w, crop).cpu().numpy()] == 0).all()
    assert err <= MAP_BAR


def test_relevance_of_a_convolutional_body_is_grad_cam_and_grad_cam_still_refuses_the_vit(hip, clf, r18):
    im = torch.rand(vo.B, 3, *SZ, generator=torch.Generator().manual_seed(5)).to(DEV)
    assert torch.equal(r18.relevance(im, TARGETS, CROP), r18.grad_cam(im, TARGETS, CROP))
    with pytest.raises(NotImplementedError, match='no convolutional feature map'):
        clf.grad_cam(im, TARGETS, CROP)
    with pytest.raises(ValueError, match='relevance: class_idx'):
        clf.relevance(im, [0, 1, vo.NUM_CLASSES], CROP)
    with pytest.raises(ValueError, match='relevance: im must be'):
        clf.relevance(im[:, :2], TARGETS, CROP)


def test_engine_backward_weights_the_plain_gradient_image(hip, clf):
    """Inside the crop the weighted image is the same pass's plain image times f + (1 - f) M_out to 2 U relative (f = 0.25: 1 - f is
    exact, the weight is one fused multiply-add, the product one rounding); outside the crop and in the pad channel it is the plain
    image bit for bit; f = 1 is the plain image everywhere."""
    Att = hip['clf'].Attention
    (h, w), crop = vo.GEOMS[ATTACK_GEOM][:2]
    eng = clf.engine(vo.B, (h, w), crop)
    eng.forward(to_nhwc4(vo.images(ATTACK_GEOM).to(DEV)))
    target = torch.tensor(TARGETS, dtype=torch.int32, device=DEV)
    g = torch.zeros(vo.B, vo.NUM_CLASSES, device=DEV)
    g[torch.arange(vo.B), target.long()] = torch.tensor([-1.0 / 3.0, 1.0 / 3.0, -0.7], device=DEV)
    plain = eng.backward(g).clone()
    f = 0.25
    weighted = eng.backward(g, Att(f, rollout=True), target).clone()
    M = eng.attention_map()[:, 0]
    inside = inside_of(h, w, crop)
    assert torch.equal(eng.backward(g), plain)                                       # (the rollout leaves the pass itself alone)
    assert 0.5 < float(M.max()) <= 1.0 and float(M.min()) >= 0.0 and float(M[:, inside].min()) < 0.9
    want = plain[..., :3].double() * (f + (1 - f) * M.double()).unsqueeze(-1)
    err = (weighted[..., :3].double() - want).abs()
    rel = float((err[:, inside] / want[:, inside].abs().clamp_min(1e-300)).max())
    print(f'weighted against plain x (f + (1 - f) M): largest relative error {rel / U:.3f} U')
    assert (err[:, inside] <= 2 * U * want[:, inside].abs()).all() and plain[:, inside][..., :3].any()
    assert torch.equal(weighted[:, ~inside], plain[:, ~inside]) and torch.equal(weighted[..., 3], plain[..., 3])
    assert not torch.equal(weighted, plain)
    assert torch.equal(eng.backward(g, Att(1.0, rollout=True), target), plain)
    # the map of the engine's pass is the map Classifier.relevance gives for the same image and classes: the seed is divided out
    assert float((clf.relevance(vo.images(ATTACK_GEOM).to(DEV), TARGETS, crop)[:, 0] - M).abs().max()) <= MAP_BAR
    # without `rollout` the engine refuses as before
    with pytest.raises(NotImplementedError, match='no convolutional feature map'):
        eng.backward(g, Att(f), target)
    with pytest.raises(ValueError, match='target must be int32'):
        eng.backward(g, Att(f, rollout=True), target.long())


def test_attack_and_sweep_run_with_the_rollout(hip, pcnet, clf):
    A = hip['attack']
    att = A.Attention(0.25, rollout=True)
    cam, prj = A.spaa(pcnet, clf, *_args(), iters=3, attention=att)
    assert cam.shape == (vo.B, 3, *SZ) and prj.shape == (vo.B, 3, *SZ) and torch.isfinite(cam).all() and torch.isfinite(prj).all()
    out = A.spaa_sweep(pcnet, clf, None, scene(), SETUP, DEV, [(LOSS, 5.0, True, TARGETS[:2]), ('caml2', 9.0, False, [5])], iters=2,
                       attention=att)
    assert len(out) == 2 and out[0][1].shape == (2, 3, *SZ) and all(torch.isfinite(o[1]).all() for o in out)
    st = A.AttackState(pcnet, clf, TARGETS, scene(), [LOSS] * 3, SETUP, DEV, attention=att)
    for _ in range(3):
        st.iteration(True, 5.0, 2, 1, P_THRESH)
    maps = st.attention_maps()
    assert maps.shape == (vo.B, 1, *SZ) and float(maps.min()) >= 0 and float(maps.max()) <= 1 and maps.any()
    assert torch.isfinite(st.x).all() and torch.isfinite(st.clf.g_y).all() and st.clf.g_y.any()
    # the default Attention still refuses the ViT, at the entry points and in a state of its own
    with pytest.raises(NotImplementedError, match='vit_b_16'):
        A.spaa(pcnet, clf, *_args(), iters=2, attention=A.Attention(0.25))
    with pytest.raises(NotImplementedError, match='no convolutional feature map'):
        A.AttackState(pcnet, clf, TARGETS, scene(), [LOSS] * 3, SETUP, DEV, attention=A.Attention(0.25))
    for kw in (dict(jitter=A.CaptureJitter(draws=2, seed=1)), dict(pose=A.PoseJitter(draws=2, seed=1)), dict(storage='f16')):
        with pytest.raises(NotImplementedError):
            A.spaa(pcnet, clf, *_args(), iters=2, attention=att, **kw)


def test_mixed_ensemble_each_member_with_its_own_kind_of_map(hip, pcnet, clf, r18):
    A = hip['attack']
    att = A.Attention(0.25, rollout=True)
    st = A.EnsembleAttackState(pcnet, [clf, r18], TARGETS, scene(), [LOSS] * 3, SETUP, DEV, attention=att)
    st.iteration(True, 5.0, 2, 1, P_THRESH)
    maps = st.attention_maps()
    assert len(maps) == 2 and all(m.shape == (vo.B, 1, *SZ) and m.min() >= 0 and m.max() <= 1 for m in maps)
    assert not torch.equal(maps[0], maps[1])
    assert torch.isfinite(st.x).all() and torch.isfinite(st.g_adv).all() and st.g_adv.any()
    # the ResNet member's map is Grad-CAM's: a second engine of that classifier, on the same camera image and seeds, with the default
    # Attention
    eng = r18.engine(vo.B, SZ, CROP)
    assert eng is not st.clfs[1]
    eng.forward(st._y)
    eng.backward(st.ens_g_logits[1], A.Attention(0.25), st.target)
    assert torch.equal(eng.attention_map(), maps[1])
    cam, prj = A.spaa(pcnet, [clf, r18], *_args(), iters=2, attention=att)
    assert prj.shape == (vo.B, 3, *SZ) and torch.isfinite(prj).all()


def test_captured_iteration_replays_the_uncaptured_run(hip, pcnet, clf):
    A = hip['attack']
    att = A.Attention(0.25, rollout=True)
    cam_g, prj_g = A.spaa(pcnet, clf, *_args(), iters=5, attention=att)
    assert A.LAST_RUN == dict(iterations=5, graph=True)
    tr = []
    cam_e, prj_e = A.spaa(pcnet, clf, *_args(), iters=5, attention=att, trace=tr)
    assert A.LAST_RUN == dict(iterations=5, graph=False) and len(tr) == 5
    assert torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    plain = A.spaa(pcnet, clf, *_args(), iters=5)[1]
    assert not torch.equal(plain, prj_g)                                             # (the weights act)
