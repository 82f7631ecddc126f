"""CPU: the ensemble attack's host side -- the three new entry points are declared and exported, the float64 restatement
(tests/ensemble_oracle.py) with one member is the oracle's own first-iteration decision, the `focus` rule, the driver's '+' names and
the argument errors of spaa() / spaa_sweep(), which are raised before anything touches a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import ensemble_oracle as eo
import spaa_oracle as so
from spaa_amd import _lib, io, synthetic as syn
from spaa_amd import projector_based_attack as A
from spaa_amd.attack_driver import ensemble_members
from spaa_amd.classifier import Classifier
from spaa_amd.models import PCNet, WarpingNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_decide_ens', 'spaa_ens_sumsq', 'spaa_ens_combine')


def test_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/spaa_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES
    assert re.search(r'#define\s+SPAA_ENS_MAX\s+4\b', hdr) and A.ENS_MAX == 4
    assert 'group_ops.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()


@pytest.mark.parametrize('targeted', [True, False])
def test_one_member_restatement_is_the_oracles_decision(targeted):
    """K = 1: first_iteration's decision (top-1, p1, target logit, succ; best_adv = fooled && high_pert) against the first iteration
    of oracle.spaa_oracle.spaa on the same inputs, both in float32."""
    sz = (64, 64)
    sd = syn.pcnet_state_dict(0, cam_sz=sz, mask='rect')
    oc = so.OracleClassifier('resnet18', syn.resnet18_state_dict(2, logit_gain=20.0), input_sz=(56, 56))
    scene = syn.scenes(1, 1, sz)
    setup = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=sz)
    true_idx = int(oc(scene, (60, 60))[2][0, 0])
    targets = [204, 291, true_idx] if targeted else [true_idx, 204]   # (untargeted on 204: a success from the start)
    d_thr = 0.0 if not targeted else 5.0                               # (0: every perturbation is above it, best_adv = fooled)
    tr = []
    so.spaa(sd, oc, targets, targeted, scene, d_thr, 'camdE_caml2', setup, iters=1, trace=tr)
    t = tr[0]
    r = eo.first_iteration(sd, [oc], targets, [targeted] * len(targets), scene, [d_thr] * len(targets), setup, dtype=torch.float32)
    assert r['top1'].shape == (len(targets), 1)
    assert np.array_equal(r['top1'][:, 0], t['top1']) and np.array_equal(r['state_succ'], t['succ'])
    assert np.array_equal(r['succ'][:, 0], t['succ']) and np.array_equal(r['best_adv'], t['best_adv'])
    assert np.array_equal(r['nfooled'] == 1, r['fooled'][:, 0])
    assert np.allclose(r['p1'][:, 0], t['p1'], rtol=1e-5) and np.allclose(r['p_min'], t['p1'], rtol=1e-5)
    assert np.allclose(r['tl'][:, 0], t['target_logit'], rtol=1e-5, atol=1e-5) and np.allclose(r['caml2'], t['caml2'], rtol=1e-5)
    if not targeted:
        assert t['succ'].tolist() == [False, True] and t['best_adv'].tolist() == [False, True]
    # one member: the combined direction is that member's unit gradient image
    u, n = eo.unit_images(r['g'][0])
    assert (n > 0).all() and np.array_equal(r['g_adv'][..., :3], u) and (r['g_adv'][..., 3] == 0).all()


def test_focus_rule():
    """The member weights on a hand-made table of the (fooled, all fooled) cases: a fooled member rests unless all are fooled."""
    fooled = np.array([[1, 1, 1],     # fooled, all fooled      -> 1
                       [1, 0, 1],     # fooled, not all         -> 0;  not fooled -> 1
                       [0, 0, 0],     # not fooled (none is)    -> 1
                       [0, 1, 0]], dtype=bool)
    assert eo.focus_weights(fooled, True).tolist() == [[1, 1, 1], [0, 1, 0], [1, 1, 1], [1, 0, 1]]
    assert eo.focus_weights(fooled, False).tolist() == [[1, 1, 1]] * 4
    # the same through decide_ens, from logits: sample 0 targeted on class 2, sample 1 untargeted on class 2
    lg = np.full((2, 5), -3.0)
    hit, low, miss = lg.copy(), lg.copy(), lg.copy()
    hit[:, 2] = 9.0            # top-1 = 2 with p1 ~ 1
    low[:, 2] = -2.5           # top-1 = 2 with p1 ~ 0.29: below p_thresh
    miss[:, 4] = 9.0           # top-1 = 4
    r = eo.decide_ens([hit, low, miss], [2, 2], [True, False], [0.1, 0.1], [5.0, 50.0], 0.9, True, col=[1.0, 1.0], col_best=[1e6, 1e6])
    assert r['succ'].tolist() == [[True, True, False], [False, False, True]]
    assert r['fooled'].tolist() == [[True, False, False], [False, False, True]]
    assert r['ens_w'].tolist() == [[0, 1, 1], [1, 1, 0]] and r['nfooled'].tolist() == [1, 1]
    assert r['ens_state'][0].tolist() == [[3, 2], [1, 2], [0, 4]] and not r['best_adv'].any() and not r['state_succ'].any()
    r = eo.decide_ens([hit, hit], [2, 4], [True, False], [0.1, 0.1], [5.0, 50.0], 0.9, True, col=[1.0, 1.0], col_best=[1e6, 0.5])
    assert r['fooled'].all() and r['ens_w'].tolist() == [[1, 1], [1, 1]]
    assert r['best_adv'].tolist() == [True, False] and r['best'].tolist() == [True, False]    # (sample 1: all fooled below d_thr)
    r = eo.decide_ens([hit, hit], [2, 4], [True, False], [0.1, 0.3], [5.0, 50.0], 0.9, True, col=[1.0, 1.0], col_best=[1e6, 0.5])
    assert r['best_adv'].tolist() == [True, True] and r['best'].tolist() == [True, False]     # (col is not below its best)
    # an exact tie: the first maximum wins
    tie = lg.copy()
    tie[:, 1] = tie[:, 3] = 4.0
    assert eo.member_rows(tie, [3, 3], [True, False], 0.9)[0].tolist() == [1, 1]


def test_combine_restatement():
    g0 = np.zeros((2, 4, 4))
    g0[0, 0, :3] = (3.0, 0.0, 4.0)
    g0[..., 3] = 7.0                       # (the pad channel is not part of the norm)
    g1 = np.zeros((2, 4, 3))
    g1[:, 1, 1] = (2.0, -8.0)
    out = eo.combine([g0, g1], [[1.0, 1.0], [1.0, 0.5]])
    assert np.allclose(out[0, 0], (0.6, 0.0, 0.8, 0.0)) and np.allclose(out[0, 1], (0.0, 1.0, 0.0, 0.0))
    assert np.allclose(out[1, 1], (0.0, -0.5, 0.0, 0.0)) and (out[1, 0] == 0).all()      # (member 0 of sample 1: zero norm)


def test_driver_names():
    assert ensemble_members('resnet18') == ['resnet18']
    assert ensemble_members('inception_v3+resnet18+vgg16') == ['inception_v3', 'resnet18', 'vgg16']
    with pytest.raises(ValueError):
        ensemble_members('resnet18+')
    assert A.get_attacker_cfg('SPAA', '.', ['s']).classifier_names == ['inception_v3', 'resnet18', 'vgg16']


def _write_labels(path, labels):
    with open(path, 'w') as fh:
        fh.write('{' + ',\n'.join(f"{k}: '{v}'" for k, v in labels.items()) + '}')


def _peak(cls):
    def clf(im, cp):
        raw = torch.zeros(im.reshape(-1, *im.shape[-3:]).shape[0], 40)
        raw[:, cls] = 3.0
        p = torch.softmax(raw, 1)
        return raw, p, p.argsort(1, descending=True)
    return clf


def test_driver_hands_the_members_to_the_sweep(tmp_path, monkeypatch, capsys):
    """A '+' name: the named members of `classifiers` in the written order as a list, the untargeted label from the first member,
    a warning when the members disagree on the scene, and the images under a folder of that name.  The sweep is a stand-in."""
    root = tmp_path / 'data'
    setup_path = root / 'setups' / 's'
    io.save_setup_info(str(setup_path), dict(classifier_crop_sz=(4, 4), prj_brightness=0.5, prj_im_sz=(8, 6), cam_im_sz=(7, 6)))
    io.save_imgs(torch.rand(2, 3, 9, 12, generator=torch.Generator().manual_seed(0)), str(setup_path / 'cam/raw/ref'))
    keys = list(range(1, 1 + 3 * 40, 3))
    _write_labels(root / 'imagenet1000_clsidx_to_labels.txt', {k: f'class{k}' for k in keys})
    _write_labels(root / 'imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in keys[:12]})
    calls, saves = [], []

    def sweep(model, classifier, labels, cam_scene, setup_info, device, configs, *, iters=50):
        calls.append((classifier, configs))
        return [(torch.zeros(len(t), 3, 6, 7), torch.zeros(len(t), 3, 6, 8)) for *_, t in configs]
    monkeypatch.setattr(A, 'spaa_sweep', sweep)
    monkeypatch.setattr(io, 'save_imgs', lambda im, path, idx=0: saves.append((tuple(im.shape), path)))
    a, b, c = _peak(17), _peak(5), _peak(17)
    cfg = A.get_attacker_cfg('SPAA', str(root), ['s'])
    cfg.device, cfg.stealth_losses, cfg.d_threshes = 'cpu', ['caml2'], [5]
    cfg.classifier_names = ['b+a', 'a', 'a+c']
    A.run_projector_based_attack(cfg, models={'s': torch.nn.Identity()}, classifiers=dict(a=a, b=b, c=c))
    assert [x[0] for x in calls][0] == [b, a] and calls[1][0] is a and calls[2][0] == [a, c]
    assert [cf[1][1][3] for cf in calls] == [[5], [17], [17]]          # the untargeted config's label: the first member's top-1
    out = capsys.readouterr().out
    assert out.count('disagree on the unattacked scene') == 1 and '[b+a]' in out
    cfg_str = A.to_attacker_cfg_str('SPAA')[0]
    assert [s[1] for s in saves] == [os.path.join(str(setup_path), kind, cfg_str, 'caml2', '5', name)
                                     for name in cfg.classifier_names for kind in ('cam/infer/adv', 'prj/adv')]
    assert all(s[0][0] == 11 for s in saves)
    # a missing member is reported as a missing classifier is
    with pytest.raises(ValueError, match=r"classifiers=.*\['d'\]"):
        A.run_projector_based_attack(_with(cfg, ['a+d']),
                                     models={'s': torch.nn.Identity()}, classifiers=dict(a=a))
    with pytest.raises(NotImplementedError):   # ensembles are SPAA's
        pc = A.get_attacker_cfg('PerC-AL+CompenNet++', str(root), ['s'])
        pc.device, pc.classifier_names = 'cpu', ['a+b']
        A.run_projector_based_attack(pc, models={'s': torch.nn.Identity()}, classifiers=dict(a=a, b=b))


def _with(cfg, names):
    cfg.classifier_names = names
    return cfg


@pytest.fixture(scope='module')
def parts():
    sd = syn.pcnet_state_dict(0, cam_sz=(64, 64))
    pc = PCNet(sd['mask'], WarpingNet(out_size=(64, 64)))
    pc.load_state_dict(sd)
    csd = syn.resnet18_state_dict(2)
    clfs = [Classifier('resnet18', 'cpu', state_dict=csd, input_sz=(56, 56)) for _ in range(5)]
    small = Classifier('resnet18', 'cpu', state_dict=syn.resnet18_state_dict(2, num_classes=10), input_sz=(56, 56))
    setup = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=(64, 64))
    return pc, clfs, small, setup


def test_ensemble_argument_errors(parts):
    """TypeError for a member that is no spaa_amd.Classifier, ValueError for more than four members, one object twice or differing
    class counts, NotImplementedError for fp16 storage -- from spaa() and spaa_sweep(), with no GPU in reach (nothing was launched);
    a sequence of one is the plain call."""
    pc, clfs, small, setup = parts
    scene = syn.scenes(1, 1, (64, 64))
    assert clfs[0].num_classes == 1000 and small.num_classes == 10

    def run(classifier, **kw):
        return A.spaa(pc, classifier, None, [1, 2], True, scene, 5, 'caml2', 'cuda', setup, **kw)

    def sweep(classifier, **kw):
        return A.spaa_sweep(pc, classifier, None, scene, setup, 'cuda', [('caml2', 5, True, [1, 2])], **kw)

    for call in (run, sweep):
        with pytest.raises(TypeError, match='spaa_amd.Classifier'):
            call([clfs[0], lambda im, cp: None])        # (no foreign-callable route for ensembles)
        with pytest.raises(TypeError):
            call((clfs[0], object()))
        with pytest.raises(ValueError, match='at most 4'):
            call(clfs)
        with pytest.raises(ValueError, match='twice'):
            call([clfs[0], clfs[1], clfs[0]])
        with pytest.raises(ValueError, match='number of classes'):
            call([clfs[0], small])
        with pytest.raises(NotImplementedError, match='f16'):
            call([clfs[0], clfs[1]], storage='f16')
        with pytest.raises(ValueError, match='empty'):
            call([])
    assert all(not c._engines for c in clfs + [small])      # no engine was built on the way to any of these errors
    with pytest.raises(ValueError):
        A.EnsembleAttackState(pc, [clfs[0]], [1], scene, 'caml2', setup, 'cuda')
    # a sequence of one: unwrapped to the plain call, which on a CPU device raises what the plain call raises
    for seq in ([clfs[0]], (clfs[0],)):
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa(pc, seq, None, [1], True, scene, 5, 'caml2', 'cpu', setup)
    with pytest.raises(RuntimeError, match='GPU only'):
        A.spaa(pc, [clfs[0], clfs[1]], None, [1], True, scene, 5, 'caml2', 'cpu', setup)
