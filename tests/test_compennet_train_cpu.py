"""CPU: the CompenNet++ training oracle (tests/compennet_train_oracle.py) against the reference fixture
tests/golden/compennet_train_48x64.npz (tests/golden/make_golden_compennet_train.py): losses, gradient norms, full gradients
and updated parameters of two CompenNet++ iterations (the second at the StepLR-dropped learning rate) and one bare-CompenNet
iteration."""
import os

import numpy as np
import torch

from compennet_train_oracle import CompenNetTrainOracle, compen_only, pp_inputs, cn_inputs
from spaa_amd import synthetic as syn

TOL = 1e-6


def _check(z, tag, it, orc, lo, l2, names):
    assert abs(lo - float(z[f'{tag}loss{it}'])) <= TOL and abs(l2 - float(z[f'{tag}l2_{it}'])) <= TOL, (tag, it, lo, l2)
    gn = np.array([float(orc.grads[k].double().norm()) for k in names])
    ref_gn = z[f'{tag}gradnorm{it}']
    assert np.all(np.abs(gn - ref_gn) <= TOL * np.maximum(1.0, ref_gn)), np.abs(gn - ref_gn).max()
    n = 0
    for key in z.files:
        if key.startswith(f'{tag}grad{it}.'):
            k = key[len(f'{tag}grad{it}.'):]
            ref = torch.from_numpy(z[key])
            assert float((orc.grads[k] - ref).abs().max()) <= TOL * max(1.0, float(ref.abs().max())), key
            assert float((orc.p[k].detach() - torch.from_numpy(z[f'{tag}param{it}.{k}'])).abs().max()) <= TOL, key
            n += 1
    assert n >= 5


def test_oracle_reproduces_reference_compennet_training(golden_dir):
    z = np.load(os.path.join(golden_dir, 'compennet_train_48x64.npz'))
    seed, bsz = int(z['seed']), int(z['bsz'])
    cam_sz, prj_sz = tuple(int(v) for v in z['cam_sz']), tuple(int(v) for v in z['prj_sz'])
    hyper = dict(lr=float(z['lr']), l2_reg=float(z['l2_reg']), lr_drop_rate=int(z['lr_drop_rate']), lr_drop_ratio=float(z['lr_drop_ratio']))
    sd = syn.compennet_pp_state_dict(seed, out_size=prj_sz)
    assert np.allclose(np.array([float(sum(v.double().sum() for v in sd.values())), float(sum(v.double().abs().sum() for v in sd.values()))]),
                       z['wsum'], rtol=1e-12)
    orc = CompenNetTrainOracle(sd, syn.scenes(seed + 1, 1, cam_sz), bsz, prj_sz, **hyper)
    names = [str(n) for n in z['names']]
    assert len(names) == len(orc.p)
    for it, loss in enumerate(str(v) for v in z['losses']):
        lr_before = orc.lr()
        lo, l2 = orc.step(*pp_inputs(seed, it, bsz, cam_sz, prj_sz), loss)
        _check(z, '', it, orc, lo, l2, names)
        assert lr_before == hyper['lr'] * hyper['lr_drop_ratio'] ** it
    s, x, y = cn_inputs(seed, bsz, prj_sz)
    orc = CompenNetTrainOracle(compen_only(sd), s, bsz, None, **hyper)
    lo, l2 = orc.step(x, y, 'l1+ssim')
    _check(z, 'cn_', 0, orc, lo, l2, [str(n) for n in z['cn_names']])


def test_init_checkpoint_name_is_the_reference_one():
    """With its defaults, init_compennet looks for (and writes) the file name the reference spells out (train_network.py:100)."""
    from spaa_amd import io
    from spaa_amd.train_network import _init_cfg
    assert io.opt_to_string(_init_cfg('/data', 'cuda', 'CompenNet')) == 'init_CompenNet_l1+ssim_500_48_500_0.001_0.2_800_0.0001'


def test_compennet_training_api_is_exported():
    import spaa_amd
    from spaa_amd import train_network
    for name in ('CompenNetTrainer', 'train_compennet_pp', 'init_compennet', 'evaluate_model'):
        assert getattr(spaa_amd, name) is getattr(train_network, name)
