"""GPU: the attention-weighted attack (Attention through AttackState / EnsembleAttackState / MultiViewAttackState, spaa, spaa_sweep and
Classifier.grad_cam) on a 64 x 64 synthetic PCNet with a 60 x 60 classifier crop.

Bodies (test-sized): ResNet-18 at 56 x 56 and Inception-v3 at 107 x 107 have 2 x 2 feature maps, VGG-16 at 96 x 96 a 3 x 3 one, which
also takes the adaptive-pool route of its head.

  * wiring: after one teacher-forced forward_decide + backward_step the weighted gradient image equals the float64 definition
    (tests/attention_oracle.py) applied to the engine's OWN feature map, gradient and unweighted gradient image, within the kernel
    bound of tests/test_attention_ops_gpu.py;
  * parity: grad_cam() and attention_maps() against the oracle body's map, within a bound computed here from the body's own feature
    and gradient errors e_A, e_alpha: |c - c_ref| <= sum_k (|alpha_ref| e_A + e_alpha |A_ref|) + C e_alpha e_A + the kernel bound;
  * identities: floor = 1 is the plain attack bit for bit; eager, graph-replayed and repeated runs agree bit for bit;
  * twelve traced iterations of a mixed sweep; the argument errors.

The traced run uses the ResNet-18 body on purpose: on a 2 x 2 feature map every cell is a corner, the edge clamp of the resampling
reproduces the largest cell exactly, and "M is 1 somewhere" holds for every sample; on a larger map an interior maximum falls between
crop pixels and M only comes close to 1."""
import numpy as np
import pytest
import torch

import attention_oracle as ao
import spaa_oracle as so
from spaa_amd import synthetic as syn
from spaa_amd.models import to_nchw
from test_gpu_parity import hip, make_pcnet  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SZ = (64, 64)
CROP = (60, 60)
SETUP = dict(classifier_crop_sz=CROP, prj_brightness=0.5, prj_im_sz=SZ)
LOSS = 'camdE_caml2'
P_THRESH = 0.9
# name -> (state dict, input size, feature map)
BODIES = {'resnet18': (lambda: syn.resnet18_state_dict(2, logit_gain=20.0), (56, 56), (2, 2)),
          'vgg16': (lambda: syn.vgg16_state_dict(3, logit_gain=5.0, fc_width=256), (96, 96), (3, 3)),
          'inception_v3': (lambda: syn.inception_v3_state_dict(4, logit_gain=20.0), (107, 107), (2, 2))}
TARGETS = [204, 291, 7, 340]
TARGETED = [True, True, False, False]
D_THR = [5.0, 5.0, 9.0, 5.0]
_CSD = {}


def _csd(name):
    if name not in _CSD:
        _CSD[name] = BODIES[name][0]()
    return _CSD[name]


@pytest.fixture(scope='module')
def clfs(hip):
    return {n: hip['clf'].Classifier(n, DEV, state_dict=_csd(n), input_sz=BODIES[n][1]) for n in BODIES}


@pytest.fixture(scope='module')
def pcnet(hip):
    return make_pcnet(hip, syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect'), SZ)


@pytest.fixture(scope='module')
def pcnet2(hip):
    return make_pcnet(hip, syn.pcnet_state_dict(3, cam_sz=SZ, mask='rect', affine=(0.92, -0.04, -0.03, 0.05, 0.87, -0.04)), SZ)


def scene():
    return syn.scenes(1, 1, SZ)


def engine_inputs(eng, g_logits, target):
    """The engine's own feature map, gradient map and seeds as float64 arrays (a pooled gradient spread over the positions)."""
    A, G, pooled = eng.body.attention_source()
    A = A.detach().cpu().double().numpy()
    G = G.detach().cpu().double().numpy()
    if pooled:
        G = np.broadcast_to(G.reshape(A.shape[0], 1, 1, A.shape[3]) / (A.shape[1] * A.shape[2]), A.shape)
    seed = g_logits.detach().cpu().double().numpy()[np.arange(A.shape[0]), np.asarray(target)]
    return A, G, seed


def check_wiring(eng, g_logits, target, floor, what):
    """The engine's weighted g_y against the float64 definition on its own buffers; the unweighted image is the same backward pass run
    again without attention (the activations are still those of the forward pass)."""
    B = eng.B
    weighted = eng.g_y.detach().cpu().numpy().copy()
    M_gpu = eng.attention_map().cpu().double().numpy()[:, 0]
    plain = eng.backward(g_logits).detach().cpu().numpy().copy()
    A, G, seed = engine_inputs(eng, g_logits, target)
    assert A.shape[1:3] == BODIES[eng.name][2] and (seed != 0).all()
    ref = ao.cam(A, G, seed)
    bc = ao.bound_c(ref, A.shape[3])
    worst = bc.reshape(B, -1).max(axis=1)
    M = ao.camera_map(ref['m'], (eng.H, eng.W), CROP)
    tm = ao.tol_map(ref, bc)
    errM = np.abs(M_gpu - M).reshape(B, -1).max(axis=1)
    want, wgt = ao.apply(plain, M, floor, CROP)
    ti = ao.tol_image(plain, wgt, floor, tm)
    err = np.abs(weighted[..., :3].astype(np.float64) - want[..., :3])
    scale = np.abs(plain[..., :3]).reshape(B, -1).max(axis=1)
    print(f'{what}: c max / S there {(ref["cmax"] / np.maximum(ref["S"].reshape(B, -1).max(axis=1), 1e-300)).tolist()}, |M - M_def| '
          f'{errM.tolist()} (tolerance {tm.tolist()}), |g_y - def| / max|g| {(err.reshape(B, -1).max(axis=1) / scale).tolist()}, '
          f'largest tolerance / max|g| {(ti.reshape(B, -1).max(axis=1) / scale).tolist()}')
    # the case itself: every sample's map is decided beyond the kernel's rounding (a maximum clearly positive, or no positive cell)
    assert ((ref['cmax'] > 8 * worst) | (ref['pre'].reshape(B, -1).max(axis=1) < -worst)).all(), 'ill-conditioned case: choose other seeds'
    assert (errM <= tm).all() and (err <= ti).all()
    assert np.array_equal(weighted[..., 3], plain[..., 3])
    cy0, cx0 = ao.center_crop_origin(eng.H, eng.W, CROP)
    inside = np.zeros((eng.H, eng.W), dtype=bool)
    inside[cy0:cy0 + CROP[0], cx0:cx0 + CROP[1]] = True
    assert np.array_equal(weighted[:, ~inside], plain[:, ~inside]) and (M_gpu[:, ~inside] == 0).all()
    assert (scale > 0).all() and (np.abs(weighted[..., :3]).reshape(B, -1).max(axis=1) > 0).all()
    return ref


@pytest.mark.parametrize('name', list(BODIES))
def test_wiring_per_body(hip, pcnet, clfs, name):
    A = hip['attack']
    floor = 0.25
    st = A.AttackState(pcnet, clfs[name], TARGETS, scene(), [LOSS] * 4, SETUP, DEV, attention=A.Attention(floor))
    st.forward_decide(TARGETED, D_THR, P_THRESH)
    st.backward_step(2, 1)
    ref = check_wiring(st.clf, st.g_logits, TARGETS, floor, name)
    seed = ao.seeds(st.g_logits.cpu().numpy(), TARGETS)
    assert (np.sign(seed) == [-1, -1, 1, 1]).all()                            # targeted: negative seeds, untargeted: positive ones
    maps = st.attention_maps()
    assert maps.shape == (4, 1, *SZ) and maps.dtype == torch.float32 and maps.is_cuda
    assert (ref['cmax'] > 0).any()
    assert torch.isfinite(st.x).all()


def test_wiring_of_a_two_member_ensemble(hip, pcnet, clfs):
    A = hip['attack']
    names = ('resnet18', 'vgg16')
    st = A.EnsembleAttackState(pcnet, [clfs[n] for n in names], TARGETS, scene(), [LOSS] * 4, SETUP, DEV, attention=A.Attention(0.0))
    st.forward_decide(TARGETED, D_THR, P_THRESH)
    st.backward_step(2, 1)
    maps = st.attention_maps()
    assert isinstance(maps, list) and len(maps) == 2 and all(m.shape == (4, 1, *SZ) for m in maps)
    assert not torch.equal(maps[0], maps[1])                                   # each member its own map
    for k, n in enumerate(names):
        check_wiring(st.clfs[k], st.ens_g_logits[k], TARGETS, 0.0, f'member {n}')
    assert torch.isfinite(st.x).all() and torch.isfinite(st.g_adv).all()


def parity(name, eng, im, g_logits, target, M_gpu, what):
    """M_gpu against the oracle body's map of the image `im`, within the bound that the body's own errors give."""
    oc = so.OracleClassifier(name, _csd(name), input_sz=BODIES[name][1])
    g_logits = g_logits.detach().cpu().double().numpy()
    _, A_ref, G_ref = ao.body_features(oc, im.detach().cpu(), g_logits, CROP)
    seed = ao.seeds(g_logits, target)
    ref = ao.cam(A_ref, G_ref, seed)
    A, G, _ = engine_inputs(eng, torch.from_numpy(g_logits), target)
    B, C = A.shape[0], A.shape[3]
    assert A.shape == A_ref.shape
    alpha = np.sign(seed)[:, None] * G.mean(axis=(1, 2))
    e_A = np.abs(A - A_ref).reshape(B, -1).max(axis=1)
    e_al = np.abs(alpha - ref['alpha']).max(axis=1)
    bc = (np.abs(ref['alpha']).sum(axis=1) * e_A)[:, None, None] + e_al[:, None, None] * np.abs(A_ref).sum(axis=3) \
        + (C * e_al * e_A)[:, None, None] + ao.bound_c(ref, C)
    worst = bc.reshape(B, -1).max(axis=1)
    tm = ao.tol_map(ref, bc)
    M = ao.camera_map(ref['m'], SZ, CROP)
    errM = np.abs(M_gpu.detach().cpu().double().numpy()[:, 0] - M).reshape(B, -1).max(axis=1)
    print(f'{what}: e_A {e_A.tolist()} (max |A| {np.abs(A_ref).max():.3e}), e_alpha {e_al.tolist()} (max |alpha| '
          f'{np.abs(ref["alpha"]).max():.3e}), bound on c / c max (nan: no positive cell) {np.where(ref["cmax"] > 0, worst / np.maximum(ref["cmax"], 1e-300), np.nan).tolist()}, |M - M_ref| '
          f'{errM.tolist()}, tolerance {tm.tolist()}')
    assert ((ref['cmax'] > 8 * worst) | (ref['pre'].reshape(B, -1).max(axis=1) < -worst)).all(), 'ill-conditioned case: choose other seeds'
    assert (errM <= tm).all()
    return ref


@pytest.mark.parametrize('name', list(BODIES))
def test_grad_cam_against_the_oracle(hip, clfs, name):
    ims = syn.scenes(5, 3, SZ).to(DEV)
    classes = [204, 7, 340]
    M = clfs[name].grad_cam(ims, classes, CROP)
    assert M.shape == (3, 1, *SZ) and M.dtype == torch.float32 and M.is_cuda
    assert M.min() >= 0 and M.max() <= 1
    eng = clfs[name].engine(3, SZ, CROP)                                       # (the free engine grad_cam() ran on)
    assert eng._cam is not None and eng._cam['valid']
    seed = torch.zeros(3, eng.ncls)
    seed[torch.arange(3), torch.tensor(classes)] = 1.0
    parity(name, eng, ims, seed, classes, M, f'grad_cam {name}')
    assert torch.equal(clfs[name].grad_cam(ims, classes, CROP), M)             # two runs are identical
    # the head alone ran: the gradient at the input was not produced (the body's backward pass would need a forward pass with gates)
    assert not eng._grad_ready
    with pytest.raises(ValueError, match='class_idx'):
        clfs[name].grad_cam(ims, classes[:2], CROP)
    with pytest.raises(ValueError, match='class_idx'):
        clfs[name].grad_cam(ims, [1, 2, 1000], CROP)


def test_attention_maps_against_the_oracle(hip, pcnet, clfs):
    """attention_maps() of the first iteration: the oracle body's map of the camera image the engine saw, with the seeds the decision wrote."""
    A = hip['attack']
    st = A.AttackState(pcnet, clfs['vgg16'], TARGETS, scene(), [LOSS] * 4, SETUP, DEV, attention=A.Attention(0.25))
    st.forward_decide(TARGETED, D_THR, P_THRESH)
    y = to_nchw(st._y).clone()
    st.backward_step(2, 1)
    parity('vgg16', st.clf, y, st.g_logits, TARGETS, st.attention_maps(), 'attention_maps vgg16')


def _args(targets=TARGETS[:3]):
    return (None, targets, True, scene(), 5, LOSS, DEV, SETUP)


def test_floor_one_is_the_plain_attack(hip, pcnet, pcnet2, clfs):
    A = hip['attack']
    one = A.Attention(floor=1.0)
    r18, vgg = clfs['resnet18'], clfs['vgg16']
    plain = A.spaa(pcnet, r18, *_args(), iters=6)
    got = A.spaa(pcnet, r18, *_args(), iters=6, attention=one)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    plain = A.spaa(pcnet, [r18, vgg], *_args(), iters=5)
    got = A.spaa(pcnet, [r18, vgg], *_args(), iters=5, attention=one)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    sc2 = [scene(), syn.scenes(2, 1, SZ)]
    args = (None, TARGETS[:3], True, sc2, 5, LOSS, DEV, SETUP)
    plain = A.spaa([pcnet, pcnet2], r18, *args, iters=5)
    got = A.spaa([pcnet, pcnet2], r18, *args, iters=5, attention=one)
    assert all(torch.equal(a, b) for a, b in zip(got[0], plain[0])) and torch.equal(got[1], plain[1])
    # ... and a floor below one is another attack
    other = A.spaa(pcnet, r18, *_args(), iters=6, attention=A.Attention(0.0))
    assert not torch.equal(other[1], A.spaa(pcnet, r18, *_args(), iters=6)[1])


def test_eager_graph_and_repeated_runs_agree(hip, pcnet, clfs):
    A = hip['attack']
    at = A.Attention(0.0)
    for clf in (clfs['resnet18'], [clfs['resnet18'], clfs['vgg16']]):
        cam_g, prj_g = A.spaa(pcnet, clf, *_args(), iters=8, attention=at)
        assert A.LAST_RUN == dict(iterations=8, graph=True)
        cam_2, prj_2 = A.spaa(pcnet, clf, *_args(), iters=8, attention=at)
        assert A.LAST_RUN == dict(iterations=8, graph=True) and torch.equal(cam_2, cam_g) and torch.equal(prj_2, prj_g)
        tr = []
        cam_e, prj_e = A.spaa(pcnet, clf, *_args(), iters=8, attention=at, trace=tr)
        assert A.LAST_RUN == dict(iterations=8, graph=False) and len(tr) == 8
        assert torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)


def test_twelve_traced_iterations(hip, pcnet, clfs, monkeypatch):
    A = hip['attack']
    true_idx = int(clfs['resnet18'](scene().to(DEV), CROP)[0][0].argmax())
    cfgs = [(LOSS, 5.0, True, [204, 291]), (LOSS, 9.0, False, [true_idx]), ('caml2', 5.0, False, [7])]
    states = []
    make = A._attack_state

    def keep(*a, **kw):
        states.append(make(*a, **kw))
        return states[-1]

    monkeypatch.setattr(A, '_attack_state', keep)
    tr = []
    res = A.spaa_sweep(pcnet, clfs['resnet18'], None, scene(), SETUP, DEV, cfgs, iters=12, trace=tr, attention=A.Attention(0.25),
                       p_thresh=P_THRESH)
    assert A.LAST_RUN == dict(iterations=12, graph=False) and len(states) == 1 and len(tr) == 1 and len(tr[0]) == 12
    best_before = torch.full((4,), 1e6)
    for state, stats in tr[0]:
        state, stats = state.cpu(), stats.cpu()
        assert state.shape == (4, 4) and stats.shape == (4, 8) and torch.isfinite(stats).all()
        assert (stats[:, 5] <= best_before).all()                              # col_loss_best never rises
        best_before = stats[:, 5].clone()
    for (cam, prj), cfg in zip(res, cfgs):
        assert cam.shape == (len(cfg[3]), 3, *SZ) and prj.shape == (len(cfg[3]), 3, *SZ)
        assert torch.isfinite(cam).all() and torch.isfinite(prj).all() and prj.min() >= 0 and prj.max() <= 1
    st = states[0]
    assert torch.isfinite(st.x).all() and isinstance(st.attention, A.Attention)
    M = st.attention_maps().cpu()
    cy0, cx0 = ao.center_crop_origin(*SZ, CROP)
    inside = torch.zeros(SZ, dtype=torch.bool)
    inside[cy0:cy0 + CROP[0], cx0:cx0 + CROP[1]] = True
    assert M.shape == (4, 1, *SZ) and M.min() >= 0 and M.max() <= 1 and (M[:, 0][:, ~inside] == 0).all()
    assert (M.flatten(1).max(dim=1).values == 1).all()                         # 1 somewhere for every sample (2 x 2 feature map: see above)
    assert (M[:, 0][:, inside].flatten(1).min(dim=1).values < 1).any()         # and a real map, not the m = 1 fallback, somewhere


def test_argument_errors(hip, pcnet, clfs):
    A = hip['attack']
    r18 = clfs['resnet18']
    at = A.Attention(0.25)
    fresh = hip['clf'].Classifier('resnet18', DEV, state_dict=_csd('resnet18'), input_sz=(56, 56))

    def run(classifier, **kw):
        return A.spaa(pcnet, classifier, None, [1, 2], True, scene(), 5, LOSS, DEV, SETUP, iters=2, **kw)

    def sweep(classifier, **kw):
        return A.spaa_sweep(pcnet, classifier, None, scene(), SETUP, DEV, [(LOSS, 5, True, [1, 2])], iters=2, **kw)

    for call in (run, sweep):
        with pytest.raises(NotImplementedError, match='f16'):
            call(fresh, attention=at, storage='f16')
        with pytest.raises(NotImplementedError, match='attention together with capture jitter'):
            call(fresh, attention=at, jitter=A.CaptureJitter())
        with pytest.raises(TypeError):
            call(lambda im, cp: None, attention=at)
        with pytest.raises(TypeError, match='Attention'):
            call(fresh, attention=0.25)
    assert not fresh._engines                                                  # nothing was leased on the way
    with pytest.raises(ValueError):
        A.Attention(1.5)
    st = A.AttackState(pcnet, r18, [1, 2], scene(), LOSS, SETUP, DEV)
    with pytest.raises(RuntimeError, match='without attention'):
        st.attention_maps()
    st.forward_decide(True, 5, P_THRESH)
    with pytest.raises(ValueError, match='target'):
        st.clf.backward(st.g_logits, at)
    with pytest.raises(TypeError, match='Attention'):
        st.clf.backward(st.g_logits, 0.25, st.target)
    f16 = r18.engine(2, SZ, CROP, storage='f16')
    with pytest.raises(NotImplementedError, match='f16'):
        f16.attention_buffers()
    with pytest.raises(RuntimeError, match='no class-activation map'):
        r18.engine(1, SZ, CROP).attention_map()
