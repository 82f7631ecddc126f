"""GPU: Classifier('convnext_tiny') at the call sites that tests/test_convnext_gpu.py does not visit -- `pose=`, `jpeg=`, `transfer=`,
'camssim', multi-view, the three survival hooks, both One-pixel attackers and the attack driver's `classifiers={...}` dictionary.  One
call each on the narrow test network of tests/convnext_oracle.py, asserting shapes, finiteness and, where the call returns camera
images, that the loop's decision on them is the one `classify` gives: what these sites do is tested with the other bodies; here the
question is only whether they take this name."""
import os

import numpy as np
import pytest
import torch

import convnext_oracle as co
from spaa_amd import synthetic as syn
from test_gpu_parity import hip, make_pcnet  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSS = 'camdE_caml2'
P_THRESH = 0.9
SZ = (64, 64)
CROP = (60, 60)
SETUP = dict(classifier_crop_sz=CROP, prj_brightness=0.5, prj_im_sz=SZ)
TARGETS = [3, 7, 12]
B = len(TARGETS)


@pytest.fixture(scope='module')
def clf(hip):
    return hip['clf'].Classifier('convnext_tiny', DEV, state_dict=co.state_dict(), input_sz=co.GEOMS['square'][2])


@pytest.fixture(scope='module')
def clf1000(hip):
    """The narrow network with 1000 classes (the driver and the One-pixel attackers take ImageNet class ids), unsorted results."""
    sd = syn.convnext_tiny_state_dict(8, num_classes=1000, logit_gain=co.LOGIT_GAIN, dims=co.DIMS, depths=co.DEPTHS)
    return hip['clf'].Classifier('convnext_tiny', DEV, state_dict=sd, sort_results=False, input_sz=co.GEOMS['square'][2])


@pytest.fixture(scope='module')
def pcnet(hip):
    return make_pcnet(hip, syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect'), SZ)


def scene():
    return syn.scenes(1, 1, SZ)


def _args():
    return (None, TARGETS, True, scene(), 5, LOSS, DEV, SETUP)


def check(A, clf, cam, prj):
    assert cam.shape == (B, 3, *SZ) and prj.shape == (B, 3, *SZ) and torch.isfinite(prj).all() and torch.isfinite(cam).all()
    got = A.transfer_success(cam, clf, TARGETS, True, CROP, P_THRESH)
    p = torch.softmax(clf(cam, CROP)[0], dim=1)
    want = (p.argmax(dim=1).cpu() == torch.tensor(TARGETS)) & (p.max(dim=1).values.cpu() > P_THRESH)
    assert got.tolist() == want.tolist()


def test_pose_jpeg_transfer_and_camssim(hip, pcnet, clf):
    A = hip['attack']
    check(A, clf, *A.spaa(pcnet, clf, *_args(), iters=2, pose=A.PoseJitter(draws=2, seed=1)))
    check(A, clf, *A.spaa(pcnet, clf, *_args(), iters=2, jpeg=A.JpegCapture(draws=2, seed=2)))
    check(A, clf, *A.spaa(pcnet, clf, *_args(), iters=2, transfer=A.Transfer(0.9, 1.0)))
    check(A, clf, *A.spaa(pcnet, clf, None, TARGETS, True, scene(), 5, 'camdE_caml2_camssim', DEV, SETUP, iters=2))


def test_multi_view(hip, pcnet, clf):
    A = hip['attack']
    pcnet2 = make_pcnet(hip, syn.pcnet_state_dict(1, cam_sz=SZ, mask='rect'), SZ)
    st = A.MultiViewAttackState([pcnet, pcnet2], clf, TARGETS, [scene(), syn.scenes(2, 1, SZ)], [LOSS] * B, SETUP, DEV)
    st.iteration(True, 5.0, 2, 1, P_THRESH)
    assert torch.isfinite(st.x).all() and (st.x[..., :3] != 0.5).any() and tuple(st.state.shape) == (B, 4)
    assert torch.isfinite(st.stats).all()


def test_the_three_survival_hooks(hip, pcnet, clf):
    A = hip['attack']
    cams, _ = A.spaa(pcnet, clf, *_args(), iters=3)
    cap = A.capture_survival(cams, clf, TARGETS, True, CROP, A.CaptureJitter(draws=2), draws=4, seed=3)
    pose = A.pose_survival(cams, clf, TARGETS, True, CROP, A.PoseJitter(draws=2), draws=4, seed=3)
    for got in (cap, pose):
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == (B,) and ((got >= 0) & (got <= 1)).all()
    jp = A.jpeg_survival(cams, clf, TARGETS, True, CROP, qualities=(90, 50))
    assert jp.shape == (2, B) and jp.dtype == bool


def test_digital_one_pixel_attacker(hip, clf1000):
    from spaa_amd.one_pixel_attacker import DigitalOnePixelAttacker
    att = DigitalOnePixelAttacker({i: f'class{i}' for i in range(1000)}, CROP)
    np.random.seed(0)
    att(scene()[0], clf1000, target_idx=3, pixel_size=5, maxiter=1, popsize=10)
    assert att.last_result.nfev > 0 and np.isfinite(att.last_result.fun)


def _write_labels(path, labels):
    with open(path, 'w') as fh:
        fh.write('{' + ',\n'.join(f"{k}: '{v}'" for k, v in labels.items()) + '}')


def test_driver_dictionary_spaa_and_projector_one_pixel(hip, pcnet, clf1000, tmp_path):
    """run_projector_based_attack with classifiers={'convnext_tiny': ...}: SPAA (one loss, one d_thr, 3 iterations) and One-pixel_DE with
    the PCNet as the capture (the projector One-pixel attacker), on a 64 x 64 setup; the driver writes its 11 images for each."""
    A = hip['attack']
    from spaa_amd import io
    root = tmp_path / 'data'
    setup_path = root / 'setups' / 'synth'
    io.save_setup_info(str(setup_path), dict(classifier_crop_sz=CROP, prj_brightness=0.5, prj_im_sz=SZ, cam_im_sz=SZ))
    io.save_imgs(syn.scenes(1, 2, SZ), str(setup_path / 'cam/raw/ref'))
    _write_labels(root / 'imagenet1000_clsidx_to_labels.txt', {k: f'class{k}, extra' for k in range(1000)})
    _write_labels(root / 'imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in syn.IMAGENET10_TARGETS})
    names = [f'img_{i:04d}.png' for i in range(1, 12)]
    cfg = A.get_attacker_cfg('SPAA', str(root), ['synth'], device_ids=[0])
    cfg.classifier_names, cfg.stealth_losses, cfg.d_threshes = ['convnext_tiny'], ['camdE_caml2'], [5]
    A.run_projector_based_attack(cfg, models={'synth': pcnet}, classifiers={'convnext_tiny': clf1000}, iters=3)
    leaves = [dp for dp, dn, fn in os.walk(setup_path / 'prj/adv') if fn]
    assert len(leaves) == 1 and leaves[0].endswith('convnext_tiny') and sorted(os.listdir(leaves[0])) == names
    one = A.get_attacker_cfg('One-pixel_DE', str(root), ['synth'], device_ids=[0])
    one.classifier_names, one.maxiter = ['convnext_tiny'], 1
    A.run_projector_based_attack(one, models={'synth': pcnet}, classifiers={'convnext_tiny': clf1000}, capture='model')
    leaf = setup_path / 'prj/adv' / 'One-pixel_DE' / '-' / '-' / 'convnext_tiny'
    assert sorted(os.listdir(leaf)) == names
