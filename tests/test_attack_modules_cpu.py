"""CPU: the attack's modules -- projector_based_attack (the entry points, and the import surface), attack_options, attack_state,
attack_driver and attack_summary:
every public name stays reachable where it always was, importing the attack does not import pandas, AttackSetup reads a setup as the
drivers did, and the deep-learning driver's host logic (what it hands the attack, what it saves, in which order) with the attack
stubbed."""
import os
import subprocess
import sys

import pytest
import torch

from spaa_amd import io, img_proc, perc_al
from spaa_amd import projector_based_attack as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the module that defines it
FACADE = {
    'CLAMP_BITS': 'projector_based_attack', 'GRAPH_MAX_PIXELS': 'projector_based_attack', 'LAST_RUN': 'projector_based_attack',
    'LOSS_TERMS': 'projector_based_attack', 'loss_weights': 'projector_based_attack',
    'spaa': 'projector_based_attack', 'spaa_attack': 'projector_based_attack', '_attack_state': 'projector_based_attack',
    'AttackState': 'attack_state', 'EnsembleAttackState': 'attack_state', 'MultiViewAttackState': 'attack_state',
    'JitterAttackState': 'attack_state', 'PoseAttackState': 'attack_state',
    'CaptureJitter': 'attack_options', 'PoseJitter': 'attack_options', 'Transfer': 'attack_options', 'ENS_MAX': 'attack_options',
    'VIEWS_MAX': 'attack_options', 'JITTER_MAX': 'attack_options', 'TRANSFER_RMAX': 'attack_options', 'POSE_MAX_ROTATE': 'attack_options',
    '_attention_supported': 'attack_options', '_attention_checked': 'attack_options',
    'plan_sweep': 'projector_based_attack', 'split_sweep': 'projector_based_attack', 'spaa_sweep': 'projector_based_attack',
    'ATTACKERS': 'attack_driver', 'MODEL_TRAIN_CFG': 'attack_driver', 'get_attacker_cfg': 'attack_driver',
    'to_attacker_cfg_str': 'attack_driver',
    'run_projector_based_attack': 'attack_driver', 'project_capture_real_attack': 'attack_driver', 'attack_results': 'attack_summary',
    'SUMMARY_STEALTH_LOSSES': 'attack_summary', 'SUMMARY_D_THRESHES': 'attack_summary', 'SUMMARY_CLASSIFIERS': 'attack_summary',
    'SUMMARY_CHUNK': 'attack_summary', 'SUMMARY_COLUMNS': 'attack_summary', 'MONTAGE_CHUNK': 'attack_summary',
    'attack_success': 'attack_summary', 'write_stats': 'attack_summary', 'summarize_single_attacker': 'attack_summary',
    'summarize_all_attackers': 'attack_summary', '_sorted_classes': 'attack_summary'}


def test_facade():
    import importlib
    import spaa_amd
    for name, home in FACADE.items():
        assert hasattr(A, name), name
        assert getattr(importlib.import_module('spaa_amd.' + home), name) is getattr(A, name), name
    # every name of the package's lazy __getattr__ (the tuples of names in its code) resolves
    lazy = [n for c in spaa_amd.__getattr__.__code__.co_consts if isinstance(c, tuple) for n in c if isinstance(n, str)]
    assert 'spaa' in lazy and 'summarize_all_attackers' in lazy and len(lazy) > 50
    for name in lazy:
        assert getattr(spaa_amd, name) is not None, name
    for name in ('spaa', 'spaa_sweep', 'run_projector_based_attack', 'summarize_single_attacker', 'attack_results'):
        assert getattr(spaa_amd, name) is getattr(A, name)


def test_importing_the_attack_leaves_pandas_out():
    code = "import sys; import spaa_amd.projector_based_attack; sys.exit(1 if 'pandas' in sys.modules else 0)"
    assert subprocess.run([sys.executable, '-s', '-c', code], cwd=ROOT).returncode == 0


def _write_labels(path, labels):
    with open(path, 'w') as fh:
        fh.write('{' + ',\n'.join(f"{k}: '{v}'" for k, v in labels.items()) + '}')


KEYS_1000 = list(range(1, 1 + 3 * 40, 3))   # 40 entries keyed 1, 4, 7, ...
KEYS_10 = KEYS_1000[:12]                    # 12 entries: the first ten are the targets


@pytest.fixture()
def root(tmp_path):
    """data/setups/s: a 9 x 12 raw scene, cam_im_sz (w, h) = (7, 6), prj_im_sz (8, 6), crop (4, 4); the two label files."""
    root = tmp_path / 'data'
    setup_path = root / 'setups' / 's'
    io.save_setup_info(str(setup_path), dict(classifier_crop_sz=(4, 4), prj_brightness=0.5, prj_im_sz=(8, 6), cam_im_sz=(7, 6)))
    g = torch.Generator().manual_seed(0)
    io.save_imgs(torch.rand(2, 3, 9, 12, generator=g), str(setup_path / 'cam/raw/ref'))
    _write_labels(root / 'imagenet1000_clsidx_to_labels.txt', {k: f'class{k}, extra' for k in KEYS_1000})
    _write_labels(root / 'imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in KEYS_10})
    return root


def _cam_scene(root):
    raw = io.torch_imread(str(root / 'setups/s/cam/raw/ref/img_0002.png'))
    assert tuple(raw.shape) == (3, 9, 12)
    return img_proc.center_crop(raw, (6, 7))


def test_attack_setup(root):
    from spaa_amd.attack_driver import AttackSetup
    s = AttackSetup(str(root), 's')
    path = os.path.join(str(root), 'setups', 's')
    assert s.path == path and s.name == 's' and tuple(s.crop_sz) == (4, 4) and tuple(s.info['prj_im_sz']) == (8, 6)
    assert torch.equal(s.raw_scene(), io.torch_imread(os.path.join(path, 'cam/raw/ref/img_0002.png')))
    assert tuple(s.cam_scene().shape) == (3, 6, 7) and torch.equal(s.cam_scene(), _cam_scene(root))
    assert s.target_idx() == KEYS_1000[:10] and s.target_idx(3) == [1, 4, 7]
    assert list(s.imagenet_labels()) == KEYS_1000 and s.imagenet_labels()[7] == 'class7'
    folder = os.path.join('SPAA_x', 'camdE_caml2', '9', 'vgg16')
    assert s.folder('SPAA_x', 'camdE_caml2', 9, 'vgg16') == folder
    for accessor, kind in ((s.prj_adv, 'prj/adv'), (s.cam_infer_adv, 'cam/infer/adv'), (s.cam_raw_adv, 'cam/raw/adv'), (s.ret, 'ret')):
        assert accessor('SPAA_x', 'camdE_caml2', 9, 'vgg16') == os.path.join(path, kind, folder)
        assert accessor('SPAA_x') == os.path.join(path, kind, 'SPAA_x')


GRID = [('caml2', 5), ('caml2', 9), ('camdE_caml2', 5), ('camdE_caml2', 9)]


def _clf17(im, cp):
    """A classifier callable whose logits peak at class 17, whatever the image."""
    raw = torch.zeros(im.reshape(-1, *im.shape[-3:]).shape[0], 40)
    raw[:, 17] = 3.0
    p = torch.softmax(raw, 1)
    return raw, p, p.argsort(1, descending=True)


def _cfg(root, attacker):
    cfg = A.get_attacker_cfg(attacker, str(root), ['s'])
    cfg.device, cfg.classifier_names = 'cpu', ['c']
    cfg.stealth_losses, cfg.d_threshes = ['caml2', 'camdE_caml2'], [5, 9]
    return cfg


def _record_saves(monkeypatch):
    saves = []
    monkeypatch.setattr(io, 'save_imgs', lambda im, path, idx=0: saves.append((tuple(im.shape), path, idx)))
    return saves


def _expected_saves(root, cfg_str):
    path = os.path.join(str(root), 'setups', 's')
    return [((11, 3, h, w), os.path.join(path, kind, cfg_str, loss, str(d), 'c'), 0)
            for loss, d in GRID for kind, (h, w) in (('cam/infer/adv', (6, 7)), ('prj/adv', (6, 8)))]


def test_driver_host_logic_spaa(root, monkeypatch):
    """One spaa_sweep call per classifier with the centre-cropped scene and, per grid point, the targeted config on the ten targets
    then the untargeted one on the scene's top-1; per grid point the inferred images are saved first, then the projector images."""
    calls = []

    def sweep(model, classifier, labels, cam_scene, setup_info, device, configs, *, iters=50):
        calls.append(dict(model=model, classifier=classifier, labels=labels, cam_scene=cam_scene, device=device, configs=configs,
                          iters=iters, prj_im_sz=tuple(setup_info['prj_im_sz'])))
        return [(torch.zeros(len(t), 3, 6, 7), torch.zeros(len(t), 3, 6, 8)) for *_, t in configs]
    monkeypatch.setattr(A, 'spaa_sweep', sweep)
    saves = _record_saves(monkeypatch)
    model = torch.nn.Identity()
    cfg = _cfg(root, 'SPAA')
    assert A.run_projector_based_attack(cfg, models={'s': model}, classifiers={'c': _clf17}, iters=7) is cfg
    assert len(calls) == 1
    c = calls[0]
    assert c['model'] is model and c['classifier'] is _clf17 and c['iters'] == 7 and c['prj_im_sz'] == (8, 6)
    assert torch.device(c['device']) == torch.device('cpu') and list(c['labels']) == KEYS_1000
    assert torch.equal(c['cam_scene'], _cam_scene(root))
    ten = KEYS_1000[:10]
    assert [tuple(x) for x in c['configs']] == [x for loss, d in GRID for x in ((loss, d, True, ten), (loss, d, False, [17]))]
    assert saves == _expected_saves(root, A.to_attacker_cfg_str('SPAA')[0])


def test_driver_host_logic_perc_al(root, monkeypatch):
    """The PerC-AL+CompenNet++ branch: two perc_al_compennet_pp calls per grid point, the targeted one first; the same files."""
    calls = []

    def attack(model, classifier, labels, target_idx, targeted, cam_scene, d_thr, device, setup_info):
        calls.append((list(target_idx), targeted, d_thr, torch.equal(cam_scene, _cam_scene(root))))
        return torch.zeros(len(target_idx), 3, 6, 7), torch.zeros(len(target_idx), 3, 6, 8)
    monkeypatch.setattr(perc_al, 'perc_al_compennet_pp', attack)
    saves = _record_saves(monkeypatch)
    cfg = _cfg(root, 'PerC-AL+CompenNet++')
    A.run_projector_based_attack(cfg, models={'s': torch.nn.Identity()}, classifiers={'c': _clf17})
    ten = KEYS_1000[:10]
    assert calls == [x for _, d in GRID for x in ((ten, True, d, True), ([17], False, d, True))]
    assert saves == _expected_saves(root, A.to_attacker_cfg_str('PerC-AL+CompenNet++')[0])
