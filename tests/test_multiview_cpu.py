"""CPU: the multi-view attack's host side -- the three new entry points are declared and exported, the float64 restatement
(tests/multiview_oracle.py) with two identical views is the oracle's own first iteration, the restated decision and combination on
hand-made tables, the argument errors of spaa() / spaa_sweep(), which are raised before anything touches a GPU, and plan_sweep, which
a list of views does not change."""
import os
import re

import numpy as np
import pytest
import torch

import multiview_oracle as mo
import spaa_oracle as so
from spaa_amd import _lib, synthetic as syn
from spaa_amd import projector_based_attack as A
from spaa_amd.classifier import Classifier
from spaa_amd.models import PCNet, WarpingNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_decide_views', 'spaa_views_combine', 'spaa_views_track')


def test_entry_points_are_declared_and_exported():
    import spaa_amd
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/spaa_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES
    assert re.search(r'#define\s+SPAA_VIEWS_MAX\s+4\b', hdr) and A.VIEWS_MAX == 4
    assert 'group_ops.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()
    assert spaa_amd.MultiViewAttackState is A.MultiViewAttackState and issubclass(A.MultiViewAttackState, A.AttackState)


@pytest.mark.parametrize('targeted', [True, False])
def test_two_identical_views_are_the_oracles_first_iteration(targeted):
    """V = 2 with the same PCNet and scene twice: first_iteration's view rows, decision and step against the first iteration of
    oracle.spaa_oracle.spaa on the same inputs, both in float32 (the mean of two equal losses is that loss, the sum of two equal
    unit images normalises to that image)."""
    sz = (64, 64)
    sd = syn.pcnet_state_dict(0, cam_sz=sz, mask='rect')
    oc = so.OracleClassifier('resnet18', syn.resnet18_state_dict(2, logit_gain=20.0), input_sz=(56, 56))
    scene = syn.scenes(1, 1, sz)
    setup = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=sz)
    true_idx = int(oc(scene, (60, 60))[2][0, 0])
    targets = [204, 291, true_idx] if targeted else [true_idx, 204]   # (untargeted on 204: a success from the start)
    d_thr = 0.0 if not targeted else 5.0                               # (0: every perturbation is above it, best_adv = fooled)
    B = len(targets)
    tr = []
    so.spaa(sd, oc, targets, targeted, scene, d_thr, 'camdE_caml2', setup, iters=1, trace=tr)
    t = tr[0]
    r = mo.first_iteration([sd, sd], oc, targets, [targeted] * B, [scene, scene], [d_thr] * B, 'camdE_caml2', setup,
                           dtype=torch.float32)
    assert r['top1'].shape == (B, 2) and r['view_stats'].shape == (B, 2, 4)
    for v in range(2):
        assert np.array_equal(r['top1'][:, v], t['top1']) and np.array_equal(r['succ'][:, v], t['succ'])
        assert np.allclose(r['p1'][:, v], t['p1'], rtol=1e-5) and np.allclose(r['tl'][:, v], t['target_logit'], rtol=1e-5, atol=1e-5)
        assert np.allclose(r['view_stats'][:, v, 2], t['caml2'], rtol=1e-5) and np.allclose(r['view_stats'][:, v, 3], t['camdE'], rtol=1e-5)
    assert np.array_equal(r['state_succ'], t['succ']) and np.array_equal(r['best_adv'], t['best_adv'])
    assert np.array_equal(r['best'], t['best']) and np.array_equal(r['nfooled'] == 2, r['fooled'][:, 0])
    assert np.allclose(r['p_min'], t['p1'], rtol=1e-5) and np.allclose(r['caml2'], t['caml2'], rtol=1e-5)
    assert np.allclose(r['camdE'], t['camdE'], rtol=1e-5) and np.allclose(r['col'], t['col_loss'], rtol=1e-5)
    if not targeted:
        assert t['succ'].tolist() == [False, True] and t['best_adv'].tolist() == [False, True]   # (both steps are compared)
    # the step: the same projector image (float32 gradients; a step moves a pixel by at most adv_lr / ||g|| |g|)
    assert r['x_next'].shape == t['prj_adv'].shape
    err = np.abs(r['x_next'].numpy() - t['prj_adv']).max()
    assert err <= 1e-5, err
    assert (r['g_out'][..., 3] == 0).all()


def test_decide_and_combine_restatements():
    """Hand-made tables: the view rows, the means over views, best_adv, the focus weights and both combination rules."""
    lg = np.full((2, 5), -3.0)
    hit, low, miss = lg.copy(), lg.copy(), lg.copy()
    hit[:, 2] = 9.0            # top-1 = 2 with p1 ~ 1
    low[:, 2] = -2.5           # top-1 = 2 with p1 ~ 0.29: below p_thresh
    miss[:, 4] = 9.0           # top-1 = 4
    w = [[0.1, 1.0, 1.0], [0.0, 1.0, 0.0]]
    # sample 0 targeted on class 2, sample 1 untargeted on class 2
    r = mo.decide_views([hit, low, miss], [2, 2], [True, False], [[0.1, 0.2, 0.3]] * 2, [[1.0, 2.0, 6.0]] * 2, w, [5.0, 60.0], 0.9,
                        True, prjl2=[0.5, 0.5], col_best=[1e6, 1e6])
    assert r['succ'].tolist() == [[True, True, False], [False, False, True]]
    assert r['fooled'].tolist() == [[True, False, False], [False, False, True]]
    assert r['view_w'].tolist() == [[0, 1, 1], [1, 1, 0]] and r['nfooled'].tolist() == [1, 1]
    assert r['view_state'][0].tolist() == [[3, 2], [1, 2], [0, 4]] and not r['best_adv'].any() and not r['state_succ'].any()
    assert np.allclose(r['caml2'], 0.2) and np.allclose(r['camdE'], 3.0) and r['prjl2'].tolist() == [0.5, 0.0]
    assert np.allclose(r['col'], [0.05 + 0.2 + 3.0, 0.2]) and r['view_stats'][1, 2].tolist()[2:] == [0.3, 6.0]
    assert r['high_pert'].tolist() == [True, False]                     # (0.2 * 255 = 51 against 5 and 60)
    r = mo.decide_views([hit, hit], [2, 4], [True, False], [[0.1, 0.3]] * 2, [[1.0, 1.0]] * 2, w, [5.0, 60.0], 0.9, True,
                        col_best=[1e6, 0.1])
    assert r['fooled'].all() and r['view_w'].tolist() == [[1, 1], [1, 1]]
    assert r['best_adv'].tolist() == [True, False] and r['best'].tolist() == [True, False]    # (sample 1: all fooled below d_thr)
    assert np.allclose(r['col_best_after'], [1.2, 0.1])
    r = mo.decide_views([hit, hit], [2, 4], [True, False], [[0.1, 0.3]] * 2, [[1.0, 1.0]] * 2, w, [5.0, 50.0], 0.9, True,
                        col_best=[1e6, 0.1])
    assert r['best_adv'].tolist() == [True, True] and r['best'].tolist() == [True, False]     # (col is not below its best)
    # the combination: sample 0 adversarial (unit images, weights), sample 1 colour (plain mean); a zero view contributes 0
    g0 = np.zeros((2, 4, 4))
    g0[:, 0, :3] = (3.0, 0.0, 4.0)
    g0[..., 3] = 7.0                       # (the pad channel is not part of the norm, and not passed on)
    g1 = np.zeros((2, 4, 3))
    g1[:, 1, 1] = (2.0, -8.0)
    out = mo.combine_views([g0, g1], [[1.0, 0.5], [1.0, 1.0]], [False, True])
    assert np.allclose(out[0, 0], (0.6, 0.0, 0.8, 0.0)) and np.allclose(out[0, 1], (0.0, 0.5, 0.0, 0.0))
    assert np.allclose(out[1, 0], (1.5, 0.0, 2.0, 0.0)) and np.allclose(out[1, 1], (0.0, -4.0, 0.0, 0.0))
    out = mo.combine_views([g0, np.zeros((2, 4, 3))], [[1.0, 1.0]] * 2, [False, False])
    assert np.allclose(out[0, 0], (0.6, 0.0, 0.8, 0.0)) and (out[:, 1:] == 0).all()


def _pcnet(sz):
    sd = syn.pcnet_state_dict(0, cam_sz=sz)
    pc = PCNet(sd['mask'], WarpingNet(out_size=sz))
    pc.load_state_dict(sd)
    return pc


@pytest.fixture(scope='module')
def parts():
    pcs = [_pcnet((64, 64)) for _ in range(5)]
    other = _pcnet((48, 64))
    csd = syn.resnet18_state_dict(2)
    clfs = [Classifier('resnet18', 'cpu', state_dict=csd, input_sz=(56, 56)) for _ in range(2)]
    setup = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=(64, 64))
    return pcs, other, clfs, setup


def test_multiview_argument_errors(parts):
    """Every error of the list forms that needs no device, from spaa() and spaa_sweep() with device='cuda' and no GPU in reach
    (nothing was allocated or launched); a sequence of one PCNet is the plain call."""
    pcs, other, clfs, setup = parts
    sc = syn.scenes(1, 1, (64, 64))
    sc_other = syn.scenes(1, 1, (48, 64))

    def run(pcnet, cam_scene, classifier=clfs[0], device='cuda', **kw):
        return A.spaa(pcnet, classifier, None, [1, 2], True, cam_scene, 5, 'caml2', device, setup, **kw)

    def sweep(pcnet, cam_scene, classifier=clfs[0], device='cuda', **kw):
        return A.spaa_sweep(pcnet, classifier, None, cam_scene, setup, device, [('caml2', 5, True, [1, 2])], **kw)

    for call in (run, sweep):
        with pytest.raises(TypeError, match='spaa_amd.PCNet'):
            call([pcs[0], object()], [sc, sc])
        with pytest.raises(TypeError, match='spaa_amd.PCNet'):
            call((pcs[0], torch.nn.Identity()), [sc, sc])
        with pytest.raises(ValueError, match='at most 4'):
            call(pcs, [sc] * 5)
        with pytest.raises(ValueError, match='twice'):
            call([pcs[0], pcs[1], pcs[0]], [sc] * 3)
        with pytest.raises(ValueError, match='one scene per view'):
            call([pcs[0], pcs[1]], [sc] * 3)
        with pytest.raises(ValueError, match='one scene per view'):
            call([pcs[0], pcs[1]], sc)
        with pytest.raises(ValueError, match='empty'):
            call([], [])
        with pytest.raises(NotImplementedError, match='ensemble'):
            call([pcs[0], pcs[1]], [sc, sc], classifier=[clfs[0], clfs[1]])
        with pytest.raises(TypeError, match='spaa_amd.Classifier'):
            call([pcs[0], pcs[1]], [sc, sc], classifier=lambda im, cp: None)
        with pytest.raises(NotImplementedError, match='f16'):
            call([pcs[0], pcs[1]], (sc, sc), storage='f16')
        with pytest.raises(ValueError, match='same camera size'):
            call([pcs[0], other], [sc, sc_other])
        # a sequence of one: the plain call (with the scene alone or in a sequence of one), which on a CPU device raises what it raises
        for seq, scenes in (([pcs[0]], sc), ((pcs[0],), [sc])):
            with pytest.raises(RuntimeError, match='GPU only'):
                call(seq, scenes, device='cpu')
        with pytest.raises(RuntimeError, match='GPU only'):
            call([pcs[0], pcs[1]], [sc, sc], device='cpu')
        with pytest.raises(RuntimeError, match='GPU only'):       # (a list of one classifier is that classifier)
            call([pcs[0], pcs[1]], [sc, sc], classifier=[clfs[0]], device='cpu')
    assert all(not p._engines for p in pcs + [other]) and all(not c._engines for c in clfs)   # no engine was built on the way
    with pytest.raises(ValueError, match='at least two'):
        A.MultiViewAttackState([pcs[0]], clfs[0], [1], [sc], 'caml2', setup, 'cuda')
    with pytest.raises(NotImplementedError):
        A.MultiViewAttackState(pcs[:2], clfs, [1], [sc, sc], 'caml2', setup, 'cuda')


def test_plan_sweep_is_unchanged():
    """The host side of the sweep does not know about views: the flattening and the chunks of a fixed configuration list."""
    cfgs = [('camdE_caml2', 5, True, [3, 4, 5]), ('caml2', 9.5, False, [7]), ('prjl2_caml2', 2, True, (8, 9))]
    samples, chunks = A.plan_sweep(cfgs, max_batch=4)
    assert samples == [(0, 'camdE_caml2', 5.0, True, 3), (0, 'camdE_caml2', 5.0, True, 4), (0, 'camdE_caml2', 5.0, True, 5),
                       (1, 'caml2', 9.5, False, 7), (2, 'prjl2_caml2', 2.0, True, 8), (2, 'prjl2_caml2', 2.0, True, 9)]
    assert chunks == [(0, 4), (4, 6)] and A.plan_sweep(cfgs)[1] == [(0, 6)]
    for bad in ([], [('caml2', 5, True, [])], [('l2', 5, True, [1])], [('caml2', 5, True)]):
        with pytest.raises(ValueError):
            A.plan_sweep(bad)
    with pytest.raises(ValueError):
        A.plan_sweep(cfgs, max_batch=0)
    # and its inverse, on per-chunk results in sample order
    res = [(torch.arange(4.0)[:, None], torch.arange(4.0)[:, None] + 10), (torch.arange(4.0, 6.0)[:, None], torch.arange(4.0, 6.0)[:, None] + 10)]
    out = A.split_sweep(samples, 3, res)
    assert [c[:, 0].tolist() for c, _ in out] == [[0, 1, 2], [3], [4, 5]] and [p[:, 0].tolist() for _, p in out] == [[10, 11, 12], [13], [14, 15]]
