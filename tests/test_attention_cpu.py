"""CPU: the attention-weighted attack's host side -- the three new entry points are declared and exported, Attention's value check,
the refusals of spaa() / spaa_sweep() and of the attack states (raised before anything touches a GPU), and the float64 restatement
(tests/attention_oracle.py) on its own: for the two global-average heads Grad-CAM by autograd is CAM (ReLU(fc.weight[t] . A),
normalised), the resampling is F.interpolate's, and the weighting leaves alone what it must."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_oracle as ao
import spaa_oracle as so
from spaa_amd import _lib, synthetic as syn
from spaa_amd import projector_based_attack as A
from spaa_amd.classifier import Attention, Classifier, ClassifierBody, ResNet18Body, VGG16Body
from spaa_amd.inception import InceptionV3Body
from spaa_amd.models import PCNet, WarpingNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_cam_alpha', 'spaa_cam_map', 'spaa_attention_apply')


def test_entry_points_are_declared_and_exported():
    import spaa_amd
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/spaa_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES
    assert 'attention_ops.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()
    assert spaa_amd.Attention is A.Attention is Attention
    for body in (ResNet18Body, VGG16Body, InceptionV3Body):
        assert body.attention_source is not ClassifierBody.attention_source


def test_attention_is_a_checked_immutable_value():
    a = Attention()
    assert a.floor == 0.0 and a == Attention(0.0) and hash(a) == hash(Attention(floor=0))
    with pytest.raises(AttributeError):
        a.floor = 0.5
    for bad in (-1e-6, 1.0001, float('nan'), float('inf'), '0.5', None, True):
        with pytest.raises(ValueError):
            Attention(bad)
    for ok in (0, 1, 0.25, 1.0):
        assert Attention(ok).floor == ok


@pytest.fixture(scope='module')
def parts():
    sd = syn.pcnet_state_dict(0, cam_sz=(64, 64))
    pcs = []
    for _ in range(2):
        pc = PCNet(sd['mask'], WarpingNet(out_size=(64, 64)))
        pc.load_state_dict(sd)
        pcs.append(pc)
    csd = syn.resnet18_state_dict(2)
    clfs = [Classifier('resnet18', 'cpu', state_dict=csd, input_sz=(56, 56)) for _ in range(2)]
    setup = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=(64, 64))
    return pcs, clfs, setup


def test_attention_refusals(parts):
    """From spaa() and spaa_sweep() with device='cuda' and no GPU in reach: nothing was leased or launched.  The order is that of the
    existing checks: the ensemble's and the views' own refusals come first, then the jitter's, then attention's."""
    pcs, clfs, setup = parts
    scene = syn.scenes(1, 1, (64, 64))
    at = Attention(0.25)

    def run(pcnet, classifier, sc=scene, **kw):
        return A.spaa(pcnet, classifier, None, [1, 2], True, sc, 5, 'caml2', 'cuda', setup, **kw)

    def sweep(pcnet, classifier, sc=scene, **kw):
        return A.spaa_sweep(pcnet, classifier, None, sc, setup, 'cuda', [('caml2', 5, True, [1, 2])], **kw)

    for call in (run, sweep):
        with pytest.raises(NotImplementedError, match='f16'):
            call(pcs[0], clfs[0], attention=at, storage='f16')
        with pytest.raises(NotImplementedError, match='attention together with capture jitter'):
            call(pcs[0], clfs[0], attention=at, jitter=A.CaptureJitter())
        with pytest.raises(TypeError):
            call(pcs[0], lambda im, cp: None, attention=at)
        for bad in (0.25, dict(floor=0.25), 'on', True):
            with pytest.raises(TypeError, match='Attention'):
                call(pcs[0], clfs[0], attention=bad)
        # the earlier checks keep their precedence
        with pytest.raises(NotImplementedError, match='ensemble'):
            call(pcs[0], [clfs[0], clfs[1]], attention=at, storage='f16')
        with pytest.raises(NotImplementedError, match='views'):
            call([pcs[0], pcs[1]], clfs[0], [scene, scene], attention=at, storage='f16')
        with pytest.raises(TypeError, match='CaptureJitter'):
            call(pcs[0], clfs[0], attention=at, jitter=dict(gain=0.1))
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)   # no engine was built on the way
    # the states themselves
    with pytest.raises(NotImplementedError, match='f16'):
        A.AttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', storage='f16', attention=at)
    with pytest.raises(TypeError, match='Attention'):
        A.AttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', attention=0.5)
    with pytest.raises(TypeError, match='Attention'):
        A.EnsembleAttackState(pcs[0], clfs, [1], scene, 'caml2', setup, 'cuda', attention=0.5)
    with pytest.raises(TypeError, match='Attention'):
        A.MultiViewAttackState(pcs, clfs[0], [1], [scene, scene], 'caml2', setup, 'cuda', attention=0.5)
    # attention=None is the plain call, which on a CPU device raises what the plain call raises; so does an attention attack
    for kw in (dict(attention=None), dict(attention=at)):
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa(pcs[0], clfs[0], None, [1], True, scene, 5, 'caml2', 'cpu', setup, **kw)
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa_sweep(pcs[0], clfs[0], None, scene, setup, 'cpu', [('caml2', 5, True, [1, 2])], **kw)
    with pytest.raises(RuntimeError, match='GPU only'):
        clfs[0].grad_cam(torch.zeros(1, 3, 64, 64), [1], (60, 60))
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)


@pytest.mark.parametrize('name,input_sz', [('resnet18', (96, 96)), ('inception_v3', (139, 139))])
def test_grad_cam_is_cam_for_a_global_average_head(name, input_sz):
    """logits = fc(mean_ij A): the gradient at A is fc.weight[t] / (h w) at every position, so the autograd Grad-CAM is
    ReLU(fc.weight[t] . A) up to the positive factor 1 / (h w), which the normalisation removes."""
    sd = {'resnet18': syn.resnet18_state_dict, 'inception_v3': syn.inception_v3_state_dict}[name](5, logit_gain=20.0)
    oc = so.OracleClassifier(name, sd, input_sz=input_sz)
    B, ncls = 3, sd['fc.weight'].shape[0]
    im = syn.scenes(3, B, (64, 64))
    target = [204, 291, 7]
    g_logits = np.zeros((B, ncls))
    g_logits[np.arange(B), target] = [-0.5, 0.25, 0.25]           # a targeted seed and two untargeted ones
    logits, Af, Gf = ao.body_features(oc, im, g_logits, (60, 60))
    h, w = Af.shape[1:3]
    assert h >= 2 and w >= 2 and Af.shape[3] == sd['fc.weight'].shape[1] and (Af >= 0).all()
    wt = sd['fc.weight'].double().numpy()[target]                 # [B, C]
    want_G = (ao.seeds(g_logits, target)[:, None] * wt / (h * w))[:, None, None, :]
    assert np.abs(Gf - want_G).max() <= 1e-12 * np.abs(want_G).max()
    ref = ao.cam(Af, Gf, ao.seeds(g_logits, target))
    cam = np.maximum((wt[:, None, None, :] * Af).sum(axis=3), 0.0)
    assert (cam.max(axis=(1, 2)) > 0).all()
    m = cam / cam.max(axis=(1, 2), keepdims=True)
    err = np.abs(ref['m'] - m).max()
    print(f'{name}: feature map {h} x {w} x {Af.shape[3]}, |Grad-CAM - CAM| = {err:.3e}')
    assert err <= 1e-12 and ref['m'].max() == 1.0 and ref['m'].min() >= 0.0
    # the logits are the oracle's own (the wrapped pool changed nothing)
    assert np.abs(logits - oc(im, (60, 60))[0].double().numpy()).max() <= 1e-4 * np.abs(logits).max()   # (that one in fp32)


@pytest.mark.parametrize('hw,size', [((2, 3), (20, 20)), ((7, 7), (60, 60)), ((1, 1), (5, 4)), ((8, 8), (6, 6)), ((5, 3), (3, 5)),
                                     ((3, 3), (3, 3))])
def test_resampling_is_interpolate(hw, size):
    rng = np.random.default_rng(hw[0] * 100 + size[0])
    m = rng.uniform(0, 1, (2,) + hw)
    want = F.interpolate(torch.from_numpy(m)[:, None], size=size, mode='bilinear', align_corners=False)[:, 0].numpy()
    got = ao.resample(m, size)
    assert got.shape == (2,) + size and np.abs(got - want).max() <= 1e-14
    assert got.min() >= m.min() - 1e-15 and got.max() <= m.max() + 1e-15


def test_definition_edge_cases():
    """m = 1 where no position is positive and where the seed is 0; the map sits at the crop origin; the weighting leaves the pad
    channel and the pixels outside the crop alone; floor = 1 is the identity."""
    rng = np.random.default_rng(0)
    A_ = rng.uniform(0.1, 1, (3, 2, 3, 8))
    G = rng.uniform(0.1, 1, (3, 2, 3, 8))
    ref = ao.cam(A_, G, [1.0, -1.0, 0.0])
    assert (ref['pre'][0] > 0).all() and ref['m'][0].max() == 1.0
    assert (ref['pre'][1] < 0).all() and (ref['m'][1] == 1).all() and ref['cmax'][1] == 0
    assert (ref['alpha'][2] == 0).all() and (ref['m'][2] == 1).all()
    M = ao.camera_map(ref['m'], (12, 16), (8, 10))
    assert ao.center_crop_origin(12, 16, (8, 10)) == (2, 3)
    inside = np.zeros((12, 16), dtype=bool)
    inside[2:10, 3:13] = True
    assert (M[:, ~inside] == 0).all() and (M[1:, inside] == 1).all() and M[0].max() <= 1.0
    g = rng.normal(size=(3, 12, 16, 4))
    out, wgt = ao.apply(g, M, 0.25, (8, 10))
    assert np.array_equal(out[..., 3], g[..., 3]) and np.array_equal(out[:, ~inside], g[:, ~inside])
    assert np.array_equal(out[1:], g[1:]) and np.allclose(out[0, inside, :3], g[0, inside, :3] * (0.25 + 0.75 * M[0, inside])[:, None])
    assert np.array_equal(ao.apply(g, M, 1.0, (8, 10))[0], g)
