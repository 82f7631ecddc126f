"""CPU: the test-side restatement of the PCNet ablation variants' training iteration (tests/pcnet_variant_oracle.py) and of
CompenNet++ without the grid-refine net (tests/compennet_train_oracle.py) against what the REFERENCE's own modules produced
(tests/golden/make_golden_pcnet_variants.py): losses, gradient norms, chosen gradients and updated parameters of two
iterations, within the tolerances of tests/test_oracle_golden.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pcnet_variant_oracle as pvo
from compennet_train_oracle import CompenNetTrainOracle, pp_inputs
from spaa_amd import synthetic as syn


def test_batch_sum_gate_bits_argument_checks():
    """spaa_batch_sum_gate_bits (include/spaa_hip.h) refuses bad arguments with an error code before any launch."""
    from spaa_amd import _lib
    lib = _lib.load()
    g, o = ctypes.c_void_p(16), ctypes.c_void_p(32)   # (never dereferenced: every call below fails its argument check)
    for args in ((None, o, 3, 7, 9, 20, 32), (g, None, 3, 7, 9, 20, 32), (g, o, 0, 7, 9, 20, 32), (g, o, 3, 0, 9, 20, 32),
                 (g, o, 3, 7, 9, 6, 32), (g, o, 3, 7, 9, 36, 32), (g, o, 3, 7, 9, 20, 30), (g, o, 3, 7, 9, 0, 32)):
        gp, op, b, h, w, c, cs = args
        assert lib.spaa_batch_sum_gate_bits(gp, None, None, op, b, h, w, c, cs, None) != 0, args


def checksum(sd):
    return np.array([float(sum(v.double().sum() for v in sd.values())), float(sum(v.double().abs().sum() for v in sd.values()))])


def _check_iteration(z, it, orc, lo, l2):
    assert abs(lo - float(z[f'loss{it}'])) < 1e-6 and abs(l2 - float(z[f'l2_{it}'])) < 1e-7, (it, lo, l2)
    names = [str(n) for n in z['names']]
    assert sorted(orc.grads) == names
    gn = np.array([float(orc.grads[k].double().norm()) for k in names])
    assert np.allclose(gn, z[f'gradnorm{it}'], rtol=1e-4)
    n = 0
    for key in z.files:
        if key.startswith(f'grad{it}.'):
            k = key[len(f'grad{it}.'):]
            assert np.abs(orc.grads[k].numpy() - z[key]).max() <= 1e-5 * max(np.abs(z[key]).max(), 1e-12), key
            assert np.abs(orc.p[k].detach().numpy() - z[f'param{it}.{k}']).max() <= 1e-5, key
            n += 1
    assert n >= 2


@pytest.mark.parametrize('variant', list(pvo.VARIANTS))
def test_variant_restatement_reproduces_reference(golden_dir, variant):
    z = np.load(os.path.join(golden_dir, pvo.fixture_name(variant) + '.npz'))
    use_mask, use_rough, with_refine, fix, seed = pvo.VARIANTS[variant]
    assert (bool(z['use_mask']), bool(z['use_rough']), bool(z['with_refine']), bool(z['fix_shading_net']), int(z['seed'])) == \
        (use_mask, use_rough, with_refine, fix, seed)
    sd = pvo.variant_sd(seed, use_mask, use_rough, with_refine)
    assert np.allclose(checksum(sd), z['wsum'], rtol=1e-9)
    # the reference's state_dict of the variant: 44 parameters + mask + ctrl_pts, minus what the variant drops
    assert int(z['n_state']) == len(sd) == 46 - (not use_mask) - 8 * (not with_refine)
    orc = pvo.PCNetVariantOracle(sd, syn.scenes(seed + 1, 1, pvo.CAM_SZ), int(z['bsz']), use_mask, use_rough, with_refine, fix)
    frozen0 = {k: v.detach().clone() for k, v in orc.p.items() if not v.requires_grad}
    assert sorted(frozen0) == sorted(str(n) for n in z['frozen'])
    for it, opt in enumerate(pvo.LOSSES):
        prj, cam = pvo.inputs(seed, it)
        lo, l2 = orc.step(prj, cam, opt)
        _check_iteration(z, it, orc, lo, l2)
    for k, v in frozen0.items():   # fix_shading_net: torch.optim.Adam skipped them (no moment, no weight decay)
        assert torch.equal(orc.p[k].detach(), v), k


def test_compennet_pp_wo_refine_restatement_reproduces_reference(golden_dir):
    z = np.load(os.path.join(golden_dir, 'compennet_pp_train_wo_refine.npz'))
    seed, bsz = int(z['seed']), int(z['bsz'])
    cam_sz, prj_sz = tuple(int(v) for v in z['cam_sz']), tuple(int(v) for v in z['prj_sz'])
    sd = {k: v for k, v in syn.compennet_pp_state_dict(seed, out_size=prj_sz).items() if 'grid_refine_net' not in k}
    assert np.allclose(checksum(sd), z['wsum'], rtol=1e-9)
    orc = CompenNetTrainOracle(sd, syn.scenes(seed + 1, 1, cam_sz), bsz, prj_sz, float(z['lr']), float(z['l2_reg']),
                               int(z['lr_drop_rate']), float(z['lr_drop_ratio']))
    for it, opt in enumerate(pvo.LOSSES):
        cam, prj = pp_inputs(seed, it, bsz, cam_sz, prj_sz)
        lo, l2 = orc.step(cam, prj, opt)
        _check_iteration(z, it, orc, lo, l2)
