"""CPU: the attack driver's configuration (get_attacker_cfg / to_attacker_cfg_str, projector_based_attack.py:169-209), the host-side
flattening and chunking of a spaa_sweep, and its input validation (no GPU needed: every check runs before a launch)."""
import pytest
import torch

from spaa_amd import synthetic as syn
from spaa_amd import projector_based_attack as A


def test_attacker_cfg_values():
    cfg = A.get_attacker_cfg('SPAA', '/data', ['setup1'])
    assert cfg.attacker_name == 'SPAA' and cfg['attacker_name'] == 'SPAA'
    assert cfg.classifier_names == ['inception_v3', 'resnet18', 'vgg16']
    assert cfg.stealth_losses == ['caml2', 'camdE', 'camdE_caml2'] and cfg.d_threshes == [5, 7, 9, 11]
    assert cfg.data_root == '/data' and cfg.setup_list == ['setup1'] and cfg.device == 'cuda' and cfg.device_ids == [0]
    assert cfg.load_pretrained is False and cfg.plot_on is True
    p = A.get_attacker_cfg('PerC-AL+CompenNet++', '/d', ['s'], device_ids=[1], load_pretrained=True, plot_on=False)
    assert p.stealth_losses == ['camdE'] and p.d_threshes == [11] and p.device_ids == [1] and p.load_pretrained and not p.plot_on
    o = A.get_attacker_cfg('One-pixel_DE', '/d', ['s'])
    assert o.stealth_losses == ['-'] and o.d_threshes == ['-']


def test_attacker_cfg_strings():
    assert A.to_attacker_cfg_str('SPAA') == ('SPAA_PCNet_l1+ssim_500_24_2000', 'PCNet_l1+ssim_500_24_2000')
    assert A.to_attacker_cfg_str('PerC-AL+CompenNet++') == ('PerC-AL+CompenNet++_l1+ssim_500_24_2000',
                                                            'CompenNet++_l1+ssim_500_24_2000')
    assert A.to_attacker_cfg_str('One-pixel_DE') == ('One-pixel_DE', None)
    with pytest.raises(ValueError):
        A.to_attacker_cfg_str('FGSM')


def test_loss_weights():
    assert A.loss_weights('caml2') == (0.0, 1.0, 0.0)
    assert A.loss_weights('camdE') == (0.0, 0.0, 1.0)
    assert A.loss_weights('camdE_caml2') == (0.0, 1.0, 1.0)
    assert A.loss_weights('camdE_caml2_prjl2') == (0.1, 1.0, 1.0)


def _configs():
    # the reference's sweep of one classifier: stealth_losses x d_threshes x (10 targeted + 1 untargeted)
    tgt = [1, 7, 21, 207, 340, 745, 779, 846, 947, 950]
    return [c for loss in ('caml2', 'camdE', 'camdE_caml2') for d in (5, 7, 9, 11)
            for c in ((loss, d, True, tgt), (loss, d, False, [409]))]


@pytest.mark.parametrize('max_batch', [1, 7, 11, 16, 64, 132, 500])
def test_plan_sweep_flattens_and_chunks(max_batch):
    cfgs = _configs()
    samples, chunks = A.plan_sweep(cfgs, max_batch)
    assert len(samples) == 132
    # samples in config order, each config's targets in order, with that config's parameters
    want = [(i, c[0], float(c[1]), c[2], t) for i, c in enumerate(cfgs) for t in c[3]]
    assert samples == want
    # chunks tile [0, 132) in order, none larger than max_batch
    assert chunks[0][0] == 0 and chunks[-1][1] == 132
    assert all(a < b and b - a <= max_batch for a, b in chunks)
    assert all(chunks[k][1] == chunks[k + 1][0] for k in range(len(chunks) - 1))
    assert len(chunks) == -(-132 // max_batch)


def test_split_sweep_inverts_the_flattening():
    cfgs = [('caml2', 5, True, [3, 4, 5]), ('camdE', 9, False, [8]), ('camdE_caml2_prjl2', 40, True, [1, 2, 3, 4, 5, 6, 7])]
    for mb in (1, 2, 4, 11, 64):
        samples, chunks = A.plan_sweep(cfgs, mb)
        # fake per-chunk results: every sample's image carries its flat index
        res = [(torch.arange(a, b, dtype=torch.float32).view(-1, 1, 1, 1).expand(-1, 3, 2, 2),
                -torch.arange(a, b, dtype=torch.float32).view(-1, 1, 1, 1).expand(-1, 3, 4, 4)) for a, b in chunks]
        out = A.split_sweep(samples, len(cfgs), res)
        assert [o[0].shape[0] for o in out] == [3, 1, 7]
        assert [o[1].shape[0] for o in out] == [3, 1, 7]
        flat = torch.cat([o[0][:, 0, 0, 0] for o in out])
        assert torch.equal(flat, torch.arange(11, dtype=torch.float32))
        assert torch.equal(torch.cat([o[1][:, 0, 0, 0] for o in out]), -torch.arange(11, dtype=torch.float32))


def test_plan_sweep_validation_names_the_config():
    with pytest.raises(ValueError, match=r'configs\[1\].*empty'):
        A.plan_sweep([('caml2', 5, True, [1]), ('caml2', 5, True, [])])
    with pytest.raises(ValueError, match=r'configs\[0\].*unknown stealth loss'):
        A.plan_sweep([('caml2_l1', 5, True, [1])])
    with pytest.raises(ValueError, match=r'configs\[0\].*unknown stealth loss'):
        A.plan_sweep([('', 5, True, [1])])
    with pytest.raises(ValueError, match=r'configs\[2\]'):
        A.plan_sweep([('caml2', 5, True, [1]), ('camdE', 5, True, [1]), ('camdE', 5, True)])
    with pytest.raises(ValueError):
        A.plan_sweep([])
    with pytest.raises(ValueError):
        A.plan_sweep([('caml2', 5, True, [1])], max_batch=0)


def test_spaa_sweep_validation():
    from spaa_amd.models import PCNet, WarpingNet
    from spaa_amd.classifier import Classifier
    sd = syn.pcnet_state_dict(0, cam_sz=(64, 64))
    pc = PCNet(sd['mask'], WarpingNet(out_size=(64, 64)))
    pc.load_state_dict(sd)
    clf = Classifier('resnet18', 'cpu', state_dict=syn.resnet18_state_dict(2))
    setup = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=(64, 64))
    scene = syn.scenes(1, 1, (64, 64))
    ok = [('caml2', 5, True, [1, 2]), ('camdE', 7, False, [3])]
    with pytest.raises(ValueError, match=r'configs\[1\].*empty'):
        A.spaa_sweep(pc, clf, None, scene, setup, 'cuda', [ok[0], ('camdE', 7, False, [])])
    with pytest.raises(ValueError, match=r'configs\[0\].*unknown'):
        A.spaa_sweep(pc, clf, None, scene, setup, 'cuda', [('camdE_bogus', 7, False, [1])])
    with pytest.raises(TypeError):
        A.spaa_sweep(torch.nn.Identity(), clf, None, scene, setup, 'cuda', ok)
    with pytest.raises(TypeError):
        A.spaa_sweep(pc, lambda im, cp: None, None, scene, setup, 'cuda', ok)
    with pytest.raises(RuntimeError):   # no CPU fallback
        A.spaa_sweep(pc, clf, None, scene, setup, 'cpu', ok)
    with pytest.raises(ValueError, match='cam_scene'):
        A.spaa_sweep(pc, clf, None, syn.scenes(1, 1, (32, 64)), setup, 'cuda', ok)
    with pytest.raises(ValueError, match='cam_scene'):
        A.spaa_sweep(pc, clf, None, syn.scenes(1, 2, (64, 64)), setup, 'cuda', ok)


def test_driver_refuses_what_it_cannot_do(tmp_path):
    cfg = A.get_attacker_cfg('One-pixel_DE', str(tmp_path), ['s'])
    with pytest.raises(NotImplementedError, match='projector'):
        A.run_projector_based_attack(cfg)
    cfg = A.get_attacker_cfg('SPAA', str(tmp_path), ['s'])
    with pytest.raises(ValueError, match='models='):
        A.run_projector_based_attack(cfg, classifiers={})
    cfg.attacker_name = 'FGSM'
    with pytest.raises(ValueError):
        A.run_projector_based_attack(cfg)
