"""GPU: the transferable attack (Transfer through AttackState / EnsembleAttackState / MultiViewAttackState / JitterAttackState, spaa,
spaa_sweep and transfer_success) on the 64 x 64 synthetic PCNet with a 60 x 60 classifier crop of tests/test_attention_gpu.py.

  * twelve traced iterations: _shape_direction is wrapped to keep the gradient image that enters it; the float64 recurrence
    (tests/transfer_oracle.py) on these recorded gradients reproduces state.momentum and x after every iteration within the accumulated
    bounds derived there, and both kinds of step occur;
  * wiring: one iteration each of a two-member ensemble, two views and a jitter attack with two draws; spaa_sweep; transfer_success;
  * identities: eager, graph-replayed and repeated runs agree bit for bit;
  * transfer=None launches what the loop launched before: no new entry point, and the recorded names of an iteration are the recorded
    PCNet passes of tests/golden/pcnet_launch_sequences.json and the ResNet-18 passes of tests/golden/classifier_launch_sequences.json
    around the loop's own kernels, with spaa_step_and_track_n directly after the backward pass."""
import json
import os

import pytest
import torch

import transfer_oracle as to
from spaa_amd import synthetic as syn
from spaa_amd.models import to_nchw
from test_gpu_parity import hip, make_pcnet  # noqa: F401  (hip: module fixture)
import test_pcnet_routes_gpu as routes

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SZ = (64, 64)
CROP = (60, 60)
SETUP = dict(classifier_crop_sz=CROP, prj_brightness=0.5, prj_im_sz=SZ)
LOSS = 'camdE_caml2'
P_THRESH = 0.9
ADV_LR, COL_LR = 2, 1
# the addition chain behind ||d||^2 as spaa_step_and_track_n uses it: one entry of partial_ss (transfer_oracle.chain_ss = 13 with one
# 256-pixel chunk per block; the loop's own partial sums of a colour-step row are shorter: 3 + 9), then the step kernel's sum of the
# entries, at most ceil(npartial / 256) + 9 = 10 more
CHAIN_NORM = 13 + 10


@pytest.fixture(scope='module')
def r18(hip):
    return hip['clf'].Classifier('resnet18', DEV, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0), input_sz=(56, 56))


@pytest.fixture(scope='module')
def vgg(hip):
    return hip['clf'].Classifier('vgg16', DEV, state_dict=syn.vgg16_state_dict(3, logit_gain=5.0, fc_width=256), input_sz=(96, 96))


@pytest.fixture(scope='module')
def pcnet(hip):
    return make_pcnet(hip, syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect'), SZ)


@pytest.fixture(scope='module')
def pcnet2(hip):
    return make_pcnet(hip, syn.pcnet_state_dict(3, cam_sz=SZ, mask='rect', affine=(0.92, -0.04, -0.03, 0.05, 0.87, -0.04)), SZ)


def scene():
    return syn.scenes(1, 1, SZ)


def traced(st, iters, targeted, d_thr):
    """Runs `iters` iterations with _shape_direction wrapped; returns the recorded (gradient images, colour-step flags, npartial) and the
    momentum and x after every iteration, all on the CPU."""
    grads, cols, nps, ms, xs = [], [], [], [], []
    inner = st._shape_direction

    def keep(gx, partial_ss, npartial):
        grads.append(gx.clone())
        cols.append(st.state[:, 1] != 0)
        nps.append((int(npartial), tuple(partial_ss.shape)))
        return inner(gx, partial_ss, npartial)

    st._shape_direction = keep
    x0 = st.x.clone()
    for _ in range(iters):
        st.iteration(targeted, d_thr, ADV_LR, COL_LR, P_THRESH)
        ms.append(st.momentum.clone())
        xs.append(st.x.clone())
    torch.cuda.synchronize()
    del st._shape_direction
    assert len(grads) == iters and all(n == (nps[0][1][1], nps[0][1]) for n in nps)
    assert to.chain_ss(st.HWp, nps[0][0]) + 10 <= CHAIN_NORM
    cpu = lambda ts: [t.cpu() for t in ts]  # noqa: E731
    return x0.cpu(), cpu(grads), cpu(cols), cpu(ms), cpu(xs)


def check_against_recurrence(st, x0, grads, cols, ms, xs, what):
    tr = st.transfer
    w = to.taps64(tr)
    worst_m = worst_x = 0.0
    rec = to.recurrence([g.double() for g in grads], cols, x0.double(), w, float(tr.momentum), ADV_LR, COL_LR, CHAIN_NORM)
    for i, (m, x, E_m, E_x) in enumerate(rec):
        err_m = (ms[i].double() - m).abs()
        err_x = (xs[i].double() - x)[..., :3].abs()
        worst_m = max(worst_m, float((err_m / E_m.clamp_min(1e-300))[E_m > 0].max()) if (E_m > 0).any() else 0.0)
        worst_x = max(worst_x, float((err_x / E_x[..., :3]).max()))
        assert (err_m <= E_m).all(), f'{what}: momentum after iteration {i}'
        assert (err_x <= E_x[..., :3]).all(), f'{what}: x after iteration {i}'
        assert torch.equal(xs[i][..., 3], x0[..., 3])
    print(f'{what}: worst |m - m_64| / bound {worst_m:.3f}, worst |x - x_64| / bound {worst_x:.3f} over {len(grads)} iterations')


def test_twelve_traced_iterations(hip, pcnet, r18):
    """The case of the twelve-iteration tests of the attention and jitter attacks: two targeted samples at d_thr 5, the scene's own class
    untargeted at d_thr 9, one more untargeted sample with the caml2 loss."""
    A = hip['attack']
    true_idx = int(r18(scene().to(DEV), CROP)[0][0].argmax())
    targets, targeted, d_thr = [204, 291, true_idx, 7], [True, True, False, False], [5.0, 5.0, 9.0, 5.0]
    st = A.AttackState(pcnet, r18, targets, scene(), [LOSS, LOSS, LOSS, 'caml2'], SETUP, DEV, transfer=A.Transfer(0.9, 1.0))
    assert st.momentum.shape == (4, *SZ, 4) and st.momentum.dtype == torch.float32 and not st.momentum.any()
    x0, grads, cols, ms, xs = traced(st, 12, targeted, d_thr)
    kinds = torch.stack(cols)
    print(f'colour steps per iteration: {kinds.sum(dim=1).tolist()} of {kinds.shape[1]} samples')
    assert kinds.any() and (~kinds).any(), 'vacuous: the run did not take both kinds of step'
    check_against_recurrence(st, x0, grads, cols, ms, xs, 'AttackState')
    # a sample's momentum rests, bit for bit, while it is on the colour step
    for i in range(1, 12):
        for b in range(4):
            if cols[i][b]:
                assert torch.equal(ms[i][b], ms[i - 1][b])
    assert torch.isfinite(st.x).all()
    # the success rule on a classifier's own attack: transfer_success of the inferred capture is the decision of the loop
    st.forward_decide(targeted, d_thr, P_THRESH)
    y = to_nchw(st._y).clone()
    state, stats = st.state.cpu(), st.stats.cpu()
    own = torch.where(torch.tensor(targeted), (state[:, 0] != 0) & (stats[:, 0] > P_THRESH), state[:, 0] != 0)
    got = A.transfer_success(y, r18, targets, targeted, CROP, P_THRESH)
    assert got.dtype == bool and got.shape == (4,) and got.tolist() == own.tolist()
    assert A.transfer_success(y[:2], r18, targets[:2], True, CROP, p_thresh=2.0).tolist() == [False, False]   # (no p1 exceeds 1)
    with pytest.raises(ValueError, match='transfer_success'):
        A.transfer_success(y, r18, targets[:3], targeted, CROP)


def test_wiring_of_ensemble_views_and_jitter(hip, pcnet, pcnet2, r18, vgg):
    """One iteration each from the grey image: for a sample on the adversarial step m = t / |t|_1 of the recorded gradient, for one on
    the colour step (the untargeted sample may be there at once) m stays zero."""
    A = hip['attack']
    targets, targeted, d_thr = [204, 291, 7], [True, True, False], [5.0, 5.0, 9.0]
    tr = A.Transfer(1.0, 1.5)
    states = {
        'ensemble': A.EnsembleAttackState(pcnet, [r18, vgg], targets, scene(), [LOSS] * 3, SETUP, DEV, transfer=tr),
        'views': A.MultiViewAttackState([pcnet, pcnet2], r18, targets, [scene(), syn.scenes(2, 1, SZ)], [LOSS] * 3, SETUP, DEV, transfer=tr),
        'jitter': A.JitterAttackState(pcnet, r18, targets, scene(), [LOSS] * 3, SETUP, DEV, A.CaptureJitter(draws=2), transfer=tr),
    }
    for what, st in states.items():
        x0, grads, cols, ms, xs = traced(st, 1, targeted, d_thr)
        adv = ~cols[0]
        assert adv.any() and not ms[0][cols[0]].any()
        check_against_recurrence(st, x0, grads, cols, ms, xs, what)
        l1 = ms[0][..., :3].double().abs().sum(dim=(1, 2, 3))
        assert ((l1 - 1).abs() <= 64 * to.U)[adv].all()                                # |m|_1 = 1 after the first adversarial step


def test_sweep_takes_the_keyword(hip, pcnet, r18):
    A = hip['attack']
    cfgs = [(LOSS, 5.0, True, [204, 291]), ('caml2', 5.0, False, [7])]
    tr = []
    res = A.spaa_sweep(pcnet, r18, None, scene(), SETUP, DEV, cfgs, iters=3, trace=tr, transfer=A.Transfer(0.5, 1.0))
    tr_plain = []
    plain = A.spaa_sweep(pcnet, r18, None, scene(), SETUP, DEV, cfgs, iters=3, trace=tr_plain)
    assert len(tr) == 1 and len(tr[0]) == 3
    for (cam, prj), (cam_p, prj_p), cfg in zip(res, plain, cfgs):
        assert cam.shape == (len(cfg[3]), 3, *SZ) and torch.isfinite(cam).all() and torch.isfinite(prj).all()
        assert prj.min() >= 0 and prj.max() <= 1
    # another attack than the plain one: the same first iteration, other losses once the first steps have been taken
    assert torch.equal(tr[0][0][1], tr_plain[0][0][1]) and not torch.equal(tr[0][2][1], tr_plain[0][2][1])


def test_eager_graph_and_repeated_runs_agree(hip, pcnet, r18, vgg):
    A = hip['attack']
    tr = A.Transfer(0.9, 1.0)
    args = (None, [204, 291, 7], True, scene(), 5, LOSS, DEV, SETUP)
    for clf in (r18, [r18, vgg]):
        cam_g, prj_g = A.spaa(pcnet, clf, *args, iters=8, transfer=tr)
        assert A.LAST_RUN == dict(iterations=8, graph=True)
        cam_2, prj_2 = A.spaa(pcnet, clf, *args, iters=8, transfer=tr)
        assert A.LAST_RUN == dict(iterations=8, graph=True) and torch.equal(cam_2, cam_g) and torch.equal(prj_2, prj_g)
        trace = []
        cam_e, prj_e = A.spaa(pcnet, clf, *args, iters=8, transfer=tr, trace=trace)
        assert A.LAST_RUN == dict(iterations=8, graph=False) and len(trace) == 8
        assert torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    plain = A.spaa(pcnet, r18, *args, iters=8)
    assert not torch.equal(plain[1], A.spaa(pcnet, r18, *args, iters=8, transfer=tr)[1])


def _contains(seq, run):
    """The first index at which `run` occurs in `seq` as a contiguous run, or -1."""
    n = len(run)
    return next((i for i in range(len(seq) - n + 1) if seq[i:i + n] == run), -1)


def test_without_transfer_the_loop_launches_what_it_launched(hip, monkeypatch):
    """At the geometry of the PCNet launch fixture (camera 48 x 80, projector 64 x 64, batch 2, every fused route alive) with the
    ResNet-18 of the classifier launch fixture (input 64 x 64): an iteration with transfer=None is PCNet's recorded forward pass, the
    classifier's recorded passes and PCNet's recorded backward pass around the loop's own kernels, spaa_step_and_track_n follows the
    backward pass directly, and no entry point of the transferable step occurs.  With a Transfer the same sequence has the two new
    launches in that one place."""
    A, M, lib, cp = hip['attack'], hip['models'], hip['lib'], hip['cp']
    with open(routes.GOLDEN) as fh:
        want_pc = json.load(fh)['sequences']['f32-default-rough-select']
    with open(os.path.join(os.path.dirname(routes.GOLDEN), 'classifier_launch_sequences.json')) as fh:
        want_clf = json.load(fh)['sequences']['resnet18-f32-b2-64']
    monkeypatch.setattr(M, 'FUSE_SKIP2_MIN_PIXELS', 0)
    sd = syn.pcnet_state_dict(5, cam_sz=routes.CAM, mask='rect')
    pc = make_pcnet(hip, sd, routes.CAM)
    clf = hip['clf'].Classifier('resnet18', DEV, state_dict=syn.resnet18_state_dict(2), input_sz=(64, 64))
    setup = dict(classifier_crop_sz=(48, 48), prj_brightness=0.5, prj_im_sz=routes.PRJ)
    sc = syn.scenes(3, 1, routes.CAM)

    def record(transfer):
        st = A.AttackState(pc, clf, [1, 2], sc, LOSS, setup, DEV, transfer=transfer)
        st.iteration(True, 5, ADV_LR, COL_LR, P_THRESH)
        with routes.recording(lib, cp, seq := []):
            st.iteration(True, 5, ADV_LR, COL_LR, P_THRESH)
        torch.cuda.synchronize()
        return seq

    plain = record(None)
    assert not any(name.startswith('spaa_transfer') for name in plain)
    assert plain[:len(want_pc['forward'])] == want_pc['forward']
    tail = want_pc['backward'] + ['spaa_step_and_track_n']
    assert plain[-len(tail):] == tail
    # the classifier's passes between them (the fixture's recorder keeps a plan run as one entry and the fc layer as a plan)
    body = [n for n in plain[len(want_pc['forward']):-len(tail)]
            if n not in ('spaa_tapconv_f32', 'spaa_linear_small') and not n.startswith('plan:fc')]
    fwd = [r[0] for r in want_clf['forward'] if not r[0].startswith('plan:fc')]
    bwd = [r[0] for r in want_clf['backward'] if not r[0].startswith('plan:fc')]
    i, j = _contains(body, fwd), _contains(body, bwd)
    assert 0 <= i and i + len(fwd) <= j, (body, fwd, bwd)
    # what lies outside the bodies' passes is the loop's own: the crop / resize pair, the stealth loss and the decision
    rest = body[:i] + body[i + len(fwd):j] + body[j + len(bwd):]
    assert sorted(rest) == sorted(['spaa_preproc_fwd', 'spaa_stealth_loss_fwd_bwd', 'spaa_decide', 'spaa_preproc_bwd']), rest
    with_tr = record(A.Transfer(1.0, 1.0))
    assert with_tr == plain[:-1] + ['spaa_transfer_blur', 'spaa_transfer_momentum', 'spaa_step_and_track_n']
