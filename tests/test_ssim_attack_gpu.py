"""GPU: the SSIM stealth term in the attack loop ('camssim' through AttackState / EnsembleAttackState / MultiViewAttackState, spaa and
spaa_sweep) on the 64 x 64 synthetic PCNet with a 60 x 60 classifier crop and the random-init ResNet-18 of the other attack tests.

  * one forward_decide from the grey image, fp32 and fp16 storage: g_col of 'caml2_camssim' is g_col of 'caml2' plus gscale times the
    float64 gradient (tests/ssim_oracle.py) of state._y, gscale = gs_col / (B 3 Hc Wc), and state.ssim is the float64 SSIM, both
    within ssim_oracle.bars (derived there); the decision and stats are those of 'caml2';
  * spaa() with 'camdE_caml2_camssim': eager (with a trace) and as a replayed graph bit for bit, and another result than without;
  * spaa_sweep mixing 'caml2' and 'caml2_camssim': each configuration's samples bit for bit what spaa() gives them with that string
    for the whole batch (bitwise identities in this project hold at one batch size: the network launches choose their tiles by it);
  * two views and a two-member ensemble run and fill ssims / ssim; a jitter attack, a pose attack and an attention attack with a
    transferable step run with the term on the clean inference;
  * with 'caml2' alone the state has none of the new buffers."""
import numpy as np
import pytest
import torch

import ssim_oracle as so
from spaa_amd import synthetic as syn
from test_gpu_parity import hip, make_pcnet  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SZ = (64, 64)
CROP = (60, 60)
SETUP = dict(classifier_crop_sz=CROP, prj_brightness=0.5, prj_im_sz=SZ)
P_THRESH = 0.9
TARGETS = [204, 291]
NEW = ('ssim_w', 'ssim_maps', 'ssim_partials', 'ssim_scene_stats', 'ssim_tiles', '_ssim_taps')


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


def check_term(y, scene4, g_with, g_without, ssim, gscale, what):
    """Per sample: g_with - g_without against gscale grad_sum(y, scene) and ssim against the float64 SSIM, within the bars."""
    worst = 0.0
    for b in range(y.shape[0]):
        yn, sn = y[b].cpu().numpy(), scene4[b].cpu().numpy()
        bar = so.bars(yn, sn)
        gs = gscale * so.grad_sum(yn, sn)
        g0 = g_without[b, ..., :3].double().cpu().numpy()
        bound = gscale * bar['grad_sum'] + 2 * so.U * np.abs(gs) + so.U * np.abs(g0 + gs)
        err = np.abs(g_with[b, ..., :3].double().cpu().numpy() - (g0 + gs))
        assert np.abs(gs).max() > 10 * bound.max(), 'vacuous: the term is below its own bar'
        assert (err <= bound).all(), f'{what}, sample {b}: gradient at {(err / bound).max():.3f} of the bar'
        ev = abs(float(ssim[b]) - so.ssim(yn, sn))
        assert ev <= bar['value'], f'{what}, sample {b}: SSIM at {ev / bar["value"]:.3f} of the bar'
        worst = max(worst, (err / bound).max(), ev / bar['value'])
    print(f'[ssim] {what}: max error / bar = {worst:.4f}')


@pytest.mark.parametrize('storage', ['f32', 'f16'])
def test_forward_decide_adds_the_term(hip, pcnet, r18, storage):
    A = hip['attack']
    plain = A.AttackState(pcnet, r18, TARGETS, scene(), 'caml2', SETUP, DEV, storage=storage)
    assert plain.any_ssim is False and plain.ssim is None and not any(hasattr(plain, n) for n in NEW)
    st = A.AttackState(pcnet, r18, TARGETS, scene(), 'caml2_camssim', SETUP, DEV, storage=storage)
    assert st.any_ssim and st.ssim.shape == (2,) and st.ssim_w.tolist() == [1.0, 1.0] and st.ssim is st.ssims[0]
    assert st.loss_w == plain.loss_w
    for s in (plain, st):
        s.forward_decide(True, 5, P_THRESH)
    torch.cuda.synchronize()
    assert st._y.dtype == torch.float32 and st.g_col.dtype == torch.float32 and torch.equal(st._y, plain._y)
    assert torch.equal(st.state, plain.state) and torch.equal(st.stats, plain.stats)          # the decision does not see the term
    assert torch.equal(st.g_col[..., 3], plain.g_col[..., 3])
    gscale = st.gs_col / (st.B * 3 * st.HWc)
    assert (storage == 'f16') == (st.gs_col != 1.0)
    check_term(st._y, st.scene4, st.g_col, plain.g_col, st.ssim, gscale, f'forward_decide {storage}')


def test_eager_and_graph_agree_bit_for_bit(hip, pcnet, r18):
    A = hip['attack']
    # two targeted samples and an untargeted one whose d_thr of 0 puts it on the colour step as soon as its class is not the top one
    args = (None, TARGETS + [7], [True, True, False], scene(), [5.0, 5.0, 0.0], 'camdE_caml2_camssim', DEV, SETUP)
    cam_g, prj_g = A.spaa(pcnet, r18, *args, iters=8)
    assert A.LAST_RUN == dict(iterations=8, graph=True)
    trace = []
    cam_e, prj_e = A.spaa(pcnet, r18, *args, iters=8, trace=trace)
    assert A.LAST_RUN == dict(iterations=8, graph=False) and len(trace) == 8
    assert torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    assert torch.isfinite(prj_g).all() and torch.isfinite(cam_g).all()
    took_colour_step = any(bool(s[:, 1].any()) for s, _ in trace)
    plain = A.spaa(pcnet, r18, *args[:5], 'camdE_caml2', *args[6:], iters=8)
    assert took_colour_step == (not torch.equal(plain[1], prj_g)), 'the term acts on the colour step and only there'
    assert took_colour_step, 'vacuous: no sample reached the colour step'


def test_sweep_mixes_configurations_with_and_without_the_term(hip, pcnet, r18):
    A = hip['attack']
    # untargeted with d_thr 0: a sample whose class is not the top one is on the colour step, where the term acts, at once
    cfgs = [('caml2', 0.0, False, [7, 9]), ('caml2_camssim', 0.0, False, [7, 9])]
    res = A.spaa_sweep(pcnet, r18, None, scene(), SETUP, DEV, cfgs, iters=8)
    for i, (loss, d_thr, targeted, _) in enumerate(cfgs):
        cam, prj = A.spaa(pcnet, r18, None, [7, 9, 7, 9], targeted, scene(), d_thr, loss, DEV, SETUP, iters=8)
        assert torch.equal(res[i][0], cam[2 * i:2 * i + 2]) and torch.equal(res[i][1], prj[2 * i:2 * i + 2]), loss
    assert not torch.equal(res[0][1], res[1][1]), 'vacuous: the term changed nothing'
    # the mixed state skips the samples without the term: their rows stay as they were allocated
    st = A.AttackState(pcnet, r18, TARGETS + TARGETS, scene(), ['caml2'] * 2 + ['caml2_camssim'] * 2, SETUP, DEV)
    st.ssim.fill_(-7.0)
    st.forward_decide(True, 5.0, P_THRESH)
    torch.cuda.synchronize()
    assert st.ssim_w.tolist() == [0.0, 0.0, 1.0, 1.0] and st.ssim[:2].tolist() == [-7.0, -7.0]
    assert ((st.ssim[2:] > 0) & (st.ssim[2:] <= 1)).all() and not st.ssim_partials[0][:2].any()


def test_views_and_ensemble_fill_their_values(hip, pcnet, pcnet2, r18, vgg):
    A = hip['attack']
    loss = 'caml2_camssim'
    ens = A.EnsembleAttackState(pcnet, [r18, vgg], TARGETS, scene(), loss, SETUP, DEV)
    ens_plain = A.EnsembleAttackState(pcnet, [r18, vgg], TARGETS, scene(), 'caml2', SETUP, DEV)
    scenes = [scene(), syn.scenes(2, 1, SZ)]
    views = A.MultiViewAttackState([pcnet, pcnet2], r18, TARGETS, scenes, loss, SETUP, DEV)
    views_plain = A.MultiViewAttackState([pcnet, pcnet2], r18, TARGETS, scenes, 'caml2', SETUP, DEV)
    for st in (ens, ens_plain, views, views_plain):
        st.forward_decide(True, 5.0, P_THRESH)
    torch.cuda.synchronize()
    assert not ens_plain.any_ssim and not views_plain.any_ssim and views_plain.ssims is None
    gscale = 1.0 / (2 * 3 * 64 * 64)
    check_term(ens._y, ens.scene4, ens.g_col, ens_plain.g_col, ens.ssim, gscale, 'ensemble')
    assert len(views.ssims) == 2 and views.ssim is views.ssims[0] and len(views.ssim_scene_stats) == 2
    for v in range(2):
        check_term(views._ys[v], views.scene4s[v], views.g_cols[v], views_plain.g_cols[v], views.ssims[v], gscale, f'view {v}')
    assert not torch.equal(views.ssims[0], views.ssims[1])
    for st in (ens, views):
        st.backward_step(2, 1)
        st.iteration(True, 5.0, 2, 1, P_THRESH)
    torch.cuda.synchronize()
    assert torch.isfinite(ens.x).all() and torch.isfinite(views.x).all()
    jit = A.JitterAttackState(pcnet, r18, TARGETS, scene(), loss, SETUP, DEV, A.CaptureJitter(draws=2))
    jit.iteration(True, 5.0, 2, 1, P_THRESH)
    torch.cuda.synchronize()
    yn, sn = jit._y[0].cpu().numpy(), jit.scene4[0].cpu().numpy()          # the clean inference, as for the other stealth terms
    assert abs(float(jit.ssim[0]) - so.ssim(yn, sn)) <= so.bars(yn, sn)['value']
    # the pose attack, and attention with a transferable step: the term sits on the clean inference there as well
    others = (A.PoseAttackState(pcnet, r18, TARGETS, scene(), loss, SETUP, DEV, A.PoseJitter(draws=2)),
              A.AttackState(pcnet, r18, TARGETS, scene(), loss, SETUP, DEV, attention=A.Attention(0.25), transfer=A.Transfer(0.9, 1.0)))
    for st in others:
        for _ in range(2):
            st.iteration(True, 5.0, 2, 1, P_THRESH)
        torch.cuda.synchronize()
        for b in range(2):
            yn, sn = st._y[b].cpu().numpy(), st.scene4[b].cpu().numpy()
            assert abs(float(st.ssim[b]) - so.ssim(yn, sn)) <= so.bars(yn, sn)['value'], type(st).__name__
        assert torch.isfinite(st.x).all()
