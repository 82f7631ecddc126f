"""GPU: Classifier('mobilenet_v2') against the float64 restatement of tests/mobilenet_oracle.py, and through the call sites the other
bodies serve, at the two geometries of tests/mobilenet_cases.py (whose inputs saturate every ReLU6 on both sides:
tests/test_mobilenet_cpu.py).

Gates.  The input gradient of a ReLU6 network is a discontinuous function of which units lie inside (0, 6): a unit within rounding of 0
or 6 may fall on the other side in fp32 than in float64, and that one bit changes the gradient in its whole receptive field
(tests/gates.py).  So the tests (1) count the gates on which the HIP pass and the oracle disagree and check that every such unit is
within the forward error of 0 or of 6 on both sides, and (2) run the float64 backward pass with the HIP pass's OWN gates -- read from
the body's gate bytes and pre-activation buffers -- and hold the gradient to 1e-4 on every sample.
NEAR: the logits are held to 1e-5 relative L-inf; a unit can only disagree if its value is within the forward error of a threshold, so
the bar for "within rounding" is 1e-5 of the layer's largest |pre-activation| (tests/gates.py's 1.3e-6 is three times what was measured
on a 20-layer ResNet-18; this network is 52 layers deep).  Measured on the fixtures here: no gate differs at either geometry."""
import numpy as np
import pytest
import torch

import attention_oracle as ao
import mobilenet_cases as mc
import mobilenet_oracle as mo
import spaa_oracle as so
from spaa_amd import synthetic as syn
from spaa_amd.models import to_nchw
from test_gpu_parity import hip, make_pcnet, rel_inf, rel_l2, outlier_fraction  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NEAR = 1e-5
LOSS = 'camdE_caml2'
P_THRESH = 0.9


@pytest.fixture(scope='module')
def sd64():
    return mo.to64(mc.state_dict())


@pytest.fixture(scope='module')
def clfs(hip):
    return {g: hip['clf'].Classifier('mobilenet_v2', DEV, state_dict=mc.state_dict(), input_sz=mc.GEOMS[g][2]) for g in mc.GEOMS}


def unpack(mask, c):
    sh = torch.tensor([0, 1, 2, 3], device=mask.device)
    return ((mask.unsqueeze(-1).int() >> sh) & 1).bool().view(*mask.shape[:-1], c)


def hip_gates(body):
    """The 35 gates of the body's last forward pass, in the order of mo.SITES, as boolean NCHW tensors on the CPU, and what the body
    keeps of each site's value (the pre-activation, or the clamped output of a depthwise layer / features.18)."""
    inside = lambda t: (t > 0) & (t < 6)     # noqa: E731
    gates, vals = [inside(body.s_pre)], [body.s_pre]
    for blk in body.blocks:
        if 'fe' in blk:
            gates.append(inside(blk['e_pre']))
            vals.append(blk['e_pre'])
        gates.append(unpack(blk['m_d'], blk['hid']))
        vals.append(blk['d'])
    gates.append(unpack(body.m_feat, body.feat.shape[3]))
    vals.append(body.feat)
    nchw = lambda t: t.detach().cpu().permute(0, 3, 1, 2).contiguous()   # noqa: E731
    return [nchw(g) for g in gates], [nchw(v).double() for v in vals]


def count_flips(body, rec, what):
    """Per-sample number of ReLU6 gates on which the HIP pass and the oracle (`rec`: its 35 pre-activations) disagree; every such unit
    is within NEAR x the layer's scale of 0 or of 6 on both sides.  Returns (flips [B], the HIP gates)."""
    gates, vals = hip_gates(body)
    assert len(gates) == len(rec) == 35
    flips = torch.zeros(rec[0].shape[0], dtype=torch.long)
    worst = 0.0
    for name, g, v, r in zip(mo.SITES, gates, vals, rec):
        assert g.shape == r.shape, (name, g.shape, r.shape)
        # the gate bytes a launch wrote are those of the values the body kept
        assert torch.equal(g, (v > 0) & (v < 6)), name
        mism = g != ((r > 0) & (r < 6))
        if mism.any():
            scale = float(r.abs().max())
            dist = lambda t: torch.minimum(t.abs(), (t - 6).abs())     # noqa: E731
            near = float(torch.maximum(dist(r), dist(v))[mism].max()) / scale     # (a clamped value is AT its threshold: distance 0)
            worst = max(worst, near)
            assert near < NEAR, (name, near)
        flips += mism.flatten(1).sum(dim=1)
    print(f'{what}: gates that differ from the oracle per sample {flips.tolist()}, farthest from its threshold {worst:.2e} of the layer scale')
    return flips, gates


@pytest.mark.parametrize('geom', list(mc.GEOMS))
def test_logits_and_input_gradient_against_the_oracle(hip, clfs, sd64, geom):
    (h, w), crop, insz = mc.GEOMS[geom]
    clf = clfs[geom]
    assert clf.num_classes == mc.NUM_CLASSES
    im = mc.images(geom)
    r = torch.randn(mc.B, mc.NUM_CLASSES, generator=torch.Generator().manual_seed(1))
    im2 = im.clone().to(DEV).requires_grad_(True)
    raw2, p2, idx2 = clf(im2, crop)
    (raw2 * r.to(DEV)).sum().backward()
    body = clf.engine(mc.B, (h, w), crop).body                          # (the free engine the call ran on)
    assert body.feat.shape[1:3] == (2, 2) and len(body.blocks) == 17
    # float64 oracle: plain, and with the HIP pass's gates
    im64 = im.double().requires_grad_(True)
    rec = []
    raw = mo.forward(sd64, so.classifier_preprocess(im64, crop, insz), record=rec)
    (raw * r.double()).sum().backward()
    e_logits = rel_inf(raw2, raw)
    print(f'{geom}: logits rel Linf {e_logits:.2e}')
    assert e_logits < 1e-5
    p = torch.softmax(raw.detach(), dim=1)
    assert (idx2[:, 0] == p.argmax(dim=1).numpy()).all() and np.allclose(p2[:, 0], p.max(dim=1).values.numpy(), atol=1e-5)
    assert p2.shape == (mc.B, mc.NUM_CLASSES) and idx2.shape == (mc.B, mc.NUM_CLASSES)
    flips, gates = count_flips(body, rec, geom)
    im64g = im.double().requires_grad_(True)
    (mo.forward(sd64, so.classifier_preprocess(im64g, crop, insz), gates=gates) * r.double()).sum().backward()
    forced = [rel_l2(im2.grad[b], im64g.grad[b]) for b in range(mc.B)]
    plain = [rel_l2(im2.grad[b], im64.grad[b]) for b in range(mc.B)]
    gl2, gout = rel_l2(im2.grad, im64.grad), outlier_fraction(im2.grad, im64.grad, 1e-3)
    print(f'{geom}: input-gradient rel L2 per sample with the HIP gates {forced}, against the oracle\'s own gates {plain}; whole batch '
          f'{gl2:.2e}, outliers {gout:.2e}')
    assert float(im64.grad.abs().max()) > 0 and torch.isfinite(im2.grad).all()
    assert all(e < 1e-4 for e in forced)
    for b in range(mc.B):
        if flips[b] == 0:
            assert plain[b] < 1e-4, (b, plain[b])
    assert gl2 < 1e-4 or (gl2 < 5e-3 and gout < 5e-3)


@pytest.mark.parametrize('cin,cout', [(16, 96), (96, 24), (24, 144), (144, 24), (32, 16), (96, 16)])
def test_narrow_1x1_plans_against_float64(hip, cin, cout):
    """The 1 x 1 plans at the narrow ends of MobileNetV2 (K or N of 16 and 24: smaller than anything the other bodies use), forward with
    a residual add and input-gradient under gate bytes, against float64, at the 1e-5 relative L-inf the logits are held to."""
    cp = hip['cp']
    gen = torch.Generator().manual_seed(cin * 1000 + cout)
    b, h, w = 3, 9, 12
    wt = torch.randn(cout, cin, 1, 1, generator=gen) / cin ** 0.5
    bias = torch.randn(cout, generator=gen)
    x = torch.randn(b, h, w, cin, generator=gen)
    add = torch.randn(b, h, w, cout, generator=gen)
    out = torch.zeros(b, h, w, cout, device=DEV)
    cp.conv_fwd_plan(wt, bias, 1, 0, DEV, 'narrow').run(x.to(DEV), out, add=add.to(DEV))
    ref = torch.einsum('bhwc,oc->bhwo', x.double(), wt.double()[:, :, 0, 0]) + bias.double() + add.double()
    e = rel_inf(out, ref)
    g = torch.randn(b, h, w, cout, generator=gen)
    bits = torch.rand(b, h, w, cin, generator=gen) > 0.5
    from spaa_amd import _lib
    mask = _lib.pack_gate_mask(bits.float()).to(DEV)
    g_in = torch.zeros(b, h, w, cin, device=DEV)
    cp.conv_dgrad_plan(wt, 1, 0, DEV, 'narrow_dgrad').run(g.to(DEV), g_in, gate_bits=mask)
    gref = torch.einsum('bhwo,oc->bhwc', g.double(), wt.double()[:, :, 0, 0]) * bits
    eg = rel_inf(g_in, gref)
    print(f'1x1 {cin} -> {cout}: forward rel Linf {e:.2e}, input gradient {eg:.2e}')
    assert e < 1e-5 and eg < 1e-5


def test_grad_cam_against_the_oracle(hip, clfs, sd64):
    """Classifier.grad_cam against the float64 Grad-CAM of the oracle's clamped features.18 map, within the bound that the body's own
    feature and gradient errors give (the tolerance of tests/test_attention_gpu.py: parity)."""
    (h, w), crop, insz = mc.GEOMS['square']
    clf, ims, classes = clfs['square'], mc.images('square').to(DEV), [3, 7, 12]
    M = clf.grad_cam(ims, classes, crop)
    assert M.shape == (mc.B, 1, h, w) and M.dtype == torch.float32 and M.is_cuda and M.min() >= 0 and M.max() <= 1
    eng = clf.engine(mc.B, (h, w), crop)
    assert eng._cam is not None and eng._cam['valid'] and not eng._grad_ready
    seed = np.zeros((mc.B, mc.NUM_CLASSES))
    seed[np.arange(mc.B), classes] = 1.0
    logits, feat = mo.feature(sd64, so.classifier_preprocess(ims.cpu().double(), crop, insz).requires_grad_(True))
    feat.retain_grad()
    (torch.from_numpy(seed) * logits).sum().backward()
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).numpy().astype(np.float64)     # noqa: E731
    A_ref, G_ref = nhwc(feat), nhwc(feat.grad)
    sd_ = ao.seeds(seed, classes)
    ref = ao.cam(A_ref, G_ref, sd_)
    A, G, pooled = eng.body.attention_source()
    assert pooled and A is eng.body.feat and float(A.max()) == 6.0 and float(A.min()) == 0.0       # the CLAMPED map
    A = A.detach().cpu().double().numpy()
    G = np.broadcast_to(G.detach().cpu().double().numpy().reshape(mc.B, 1, 1, -1) / (A.shape[1] * A.shape[2]), A.shape)
    C = A.shape[3]
    alpha = np.sign(sd_)[:, None] * G.mean(axis=(1, 2))
    e_A = np.abs(A - A_ref).reshape(mc.B, -1).max(axis=1)
    e_al = np.abs(alpha - ref['alpha']).max(axis=1)
    bc = (np.abs(ref['alpha']).sum(axis=1) * e_A)[:, None, None] + e_al[:, None, None] * np.abs(A_ref).sum(axis=3) \
        + (C * e_al * e_A)[:, None, None] + ao.bound_c(ref, C)
    worst = bc.reshape(mc.B, -1).max(axis=1)
    tm = ao.tol_map(ref, bc)
    Mref = ao.camera_map(ref['m'], (h, w), crop)
    errM = np.abs(M.detach().cpu().double().numpy()[:, 0] - Mref).reshape(mc.B, -1).max(axis=1)
    print(f'grad_cam: e_A {e_A.tolist()}, e_alpha {e_al.tolist()}, |M - M_ref| {errM.tolist()}, tolerance {tm.tolist()}')
    assert ((ref['cmax'] > 8 * worst) | (ref['pre'].reshape(mc.B, -1).max(axis=1) < -worst)).all(), 'ill-conditioned case: choose other classes'
    assert (errM <= tm).all()
    assert torch.equal(clf.grad_cam(ims, classes, crop), M)


SZ = (64, 64)
CROP = (60, 60)
SETUP = dict(classifier_crop_sz=CROP, prj_brightness=0.5, prj_im_sz=SZ)
TARGETS = [3, 7, 12]


@pytest.fixture(scope='module')
def pcnet(hip):
    return make_pcnet(hip, syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect'), SZ)


def scene():
    return syn.scenes(1, 1, SZ)


def test_one_attack_iteration_against_the_oracle(hip, pcnet, clfs, sd64):
    """One iteration of AttackState from the initial (grey) state against the oracle's spaa() with the wrapped float64 classifier: the
    decision table, and the updated projector image to 1e-4 relative L-inf -- against the oracle as it is on every sample whose gates
    all agree, and against the oracle run with the HIP pass's classifier gates on every sample whose PCNet gates agree."""
    import gates as G
    A, clf = hip['attack'], clfs['square']
    psd = syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect')
    insz = mc.GEOMS['square'][2]
    d_thr = 5.0
    st = A.AttackState(pcnet, clf, TARGETS, scene(), LOSS, SETUP, DEV)
    st.forward_decide(True, d_thr, P_THRESH)
    # the oracle's forward pass at the same state: PCNet activations (tests/gates.py) and the classifier's 35 pre-activations
    x0 = torch.full((mc.B, 3, *SZ), 0.5)
    scene_b = scene().expand(mc.B, -1, -1, -1)
    with torch.no_grad():
        xw = so.warp(psd, x0, SZ) * psd['mask']
        y, acts = so.shading_net(psd, xw, (scene_b, xw * scene_b), return_all=True)
        rec = []
        mo.forward(sd64, so.classifier_preprocess(y, CROP, insz).double(), record=rec)
    pflips, _ = G.count_flips(G.pcnet_pairs(st.eng, acts))
    cflips, gates = count_flips(st.clf.body, rec, 'attack iteration')
    state, stats = st.state.cpu().numpy(), st.stats.cpu().numpy()
    st.backward_step(2, 1)
    x1 = to_nchw(st.x).cpu()
    res = {}
    for mode, g in (('plain', None), ('hip_gates', gates)):
        tr = []

        def oclf(im, crop_sz, g=g):
            raw = mo.forward(sd64, so.classifier_preprocess(im, crop_sz, insz).double(), gates=g)
            p_sorted, idx = torch.softmax(raw, dim=1).detach().sort(descending=True)
            return raw, p_sorted.numpy(), idx.numpy()

        so.spaa(psd, oclf, TARGETS, True, scene(), d_thr, LOSS, SETUP, iters=1, trace=tr)
        res[mode] = (tr[0], torch.tensor([rel_inf(x1[b], torch.from_numpy(tr[0]['prj_adv'])[b]) for b in range(mc.B)]))
    t = res['plain'][0]
    # wrapped as the issue describes it, the oracle classifier gives the same table
    t2 = []
    so.spaa(psd, mo.classifier(sd64, insz), TARGETS, True, scene(), d_thr, LOSS, SETUP, iters=1, trace=t2)
    assert np.array_equal(t2[0]['prj_adv'], t['prj_adv']) and (t2[0]['top1'] == t['top1']).all()
    print(f'attack iteration: x rel Linf per sample {res["plain"][1].tolist()} (oracle gates), {res["hip_gates"][1].tolist()} (HIP classifier '
          f'gates); PCNet gate flips {pflips.tolist()}, classifier {cflips.tolist()}; top-1 {state[:, 3].tolist()}, p1 {stats[:, 0].tolist()}')
    # the decision table: equal unless the oracle itself sits on a knife edge (tests/test_gpu_parity.py)
    edge = (np.abs(t['p1'] - P_THRESH) < 1e-3) | (np.abs(t['caml2'] * 255 - d_thr) < 1e-2)
    assert ((state[:, 3] == t['top1']) | edge).all()
    assert ((state[:, 0] == t['succ']) | edge).all() and ((state[:, 1] == t['best_adv']) | edge).all()
    assert ((state[:, 2] == t['best']) | edge).all()
    assert np.allclose(stats[:, 0], t['p1'], atol=2e-4) and np.allclose(stats[:, 6], t['target_logit'], rtol=1e-4, atol=1e-4)
    assert np.allclose(stats[:, 1], t['caml2'], rtol=1e-4) and np.allclose(stats[:, 2], t['camdE'], rtol=1e-4)
    same = torch.from_numpy(state[:, 1] == t['best_adv'])
    clean_p = same & (pflips == 0)
    assert clean_p.any(), 'vacuous: every sample has a PCNet gate within rounding of zero; choose another scene'
    assert (res['hip_gates'][1][clean_p] < 1e-4).all()
    assert (res['plain'][1][clean_p & (cflips == 0)] < 1e-4).all()


def _args(targets=TARGETS):
    return (None, targets, True, scene(), 5, LOSS, DEV, SETUP)


def test_eager_graph_and_repeated_runs_agree(hip, pcnet, clfs):
    A, clf = hip['attack'], clfs['square']
    cam_g, prj_g = A.spaa(pcnet, clf, *_args(), iters=5)
    assert A.LAST_RUN == dict(iterations=5, graph=True)
    cam_2, prj_2 = A.spaa(pcnet, clf, *_args(), iters=5)
    assert A.LAST_RUN == dict(iterations=5, graph=True) and torch.equal(cam_2, cam_g) and torch.equal(prj_2, prj_g)
    tr = []
    cam_e, prj_e = A.spaa(pcnet, clf, *_args(), iters=5, trace=tr)
    assert A.LAST_RUN == dict(iterations=5, graph=False) and len(tr) == 5
    assert torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    assert cam_g.shape == (mc.B, 3, *SZ) and prj_g.shape == (mc.B, 3, *SZ) and torch.isfinite(prj_g).all()
    assert all(torch.isfinite(stats).all() for _, stats in tr) and not torch.equal(tr[0][1], tr[4][1])      # the attack moves
    # spaa_sweep takes the name as well
    out = A.spaa_sweep(pcnet, clf, None, scene(), SETUP, DEV, [(LOSS, 5.0, True, TARGETS[:2]), ('caml2', 9.0, False, [5])], iters=2)
    assert len(out) == 2 and out[0][1].shape == (2, 3, *SZ) and out[1][1].shape == (1, 3, *SZ)


def test_ensemble_with_attention_and_transfer(hip, pcnet, clfs):
    """One ensemble iteration of [mobilenet_v2, resnet18] with Attention(0.25) and Transfer(0.9, 1.0): runs, documented shapes."""
    A = hip['attack']
    r18 = hip['clf'].Classifier('resnet18', DEV, state_dict=syn.resnet18_state_dict(2, num_classes=mc.NUM_CLASSES, logit_gain=20.0),
                                input_sz=(56, 56))
    st = A.EnsembleAttackState(pcnet, [clfs['square'], r18], TARGETS, scene(), [LOSS] * 3, SETUP, DEV, attention=A.Attention(0.25),
                               transfer=A.Transfer(0.9, 1.0))
    st.iteration(True, 5.0, 2, 1, P_THRESH)
    state, stats, ens_state, ens_stats = st.trace_entry()
    assert state.shape == (mc.B, 4) and stats.shape == (mc.B, 8) and ens_state.shape == (mc.B, 2, 2) and ens_stats.shape == (mc.B, 2, 2)
    maps = st.attention_maps()
    assert len(maps) == 2 and all(m.shape == (mc.B, 1, *SZ) and m.min() >= 0 and m.max() <= 1 for m in maps)
    assert not torch.equal(maps[0], maps[1])
    assert st.momentum.shape == (mc.B, *SZ, 4) and st.momentum.any()
    assert torch.isfinite(st.x).all() and torch.isfinite(st.g_adv).all() and st.g_adv.any()
    cam, prj = st.results()
    assert cam.shape == (mc.B, 3, *SZ) and prj.shape == (mc.B, 3, *SZ)
    # ... and through spaa() as a member of the list
    cam2, prj2 = A.spaa(pcnet, [clfs['square'], r18], *_args(), iters=2, attention=A.Attention(0.25), transfer=A.Transfer(0.9, 1.0))
    assert prj2.shape == (mc.B, 3, *SZ) and torch.isfinite(prj2).all()


def test_transfer_success_is_the_loops_own_decision(hip, pcnet, clfs):
    A, clf = hip['attack'], clfs['square']
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


def test_f16_storage_is_refused(hip, clfs):
    before = torch.cuda.memory_allocated()
    with pytest.raises(NotImplementedError, match='MobileNetV2Body'):
        clfs['square'].engine(mc.B, SZ, CROP, storage='f16')
    assert torch.cuda.memory_allocated() == before                                  # refused before anything is allocated
    assert all(k[3] != 'f16' or not v for k, v in clfs['square']._engines.items())    # ... and no half-built engine is kept
