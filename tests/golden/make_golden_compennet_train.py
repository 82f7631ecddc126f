"""Generates tests/golden/compennet_train_48x64.npz: two iterations of the REFERENCE's CompenNet++ training loop body
(train_network.py:180-192 with the scheduler step of :226) and one of a bare CompenNet (the init_compennet path,
:98-127), run on the unmodified reference modules (imported via oracle/ref_shims.py).  Runs only in the build container.

    python tests/golden/make_golden_compennet_train.py

train_network.py cannot be imported (visdom / Qt at import): `compute_loss` is exec'd from its source with the reference's
own pytorch_ssim.SSIM() as `ssim_fun`, as make_golden.py gen_train does.  The oracle (tests/compennet_train_oracle.py) runs
alongside; its largest difference is printed and stored (`oracle_maxdiff`).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (puts the repository root and oracle/ on sys.path)
from compennet_train_oracle import CompenNetTrainOracle, PP_KEYS, CN_KEYS, compen_only, pp_inputs, cn_inputs  # noqa: E402
from spaa_amd import synthetic as syn  # noqa: E402

NAME = 'compennet_train_48x64'
CAM_SZ, PRJ_SZ, BSZ, SEED = (48, 64), (64, 64), 4, 7
LR, L2_REG, DROP_RATE, DROP_RATIO = 1e-3, 1e-4, 1, 0.2       # lr_drop_rate 1: the second step runs at the dropped rate
LOSSES = ('l1+ssim', 'l1')


def run(model, x, s_b, y, opt, sched, loss_fn, loss):
    model.train()
    infer = model(x, s_b)
    lo, l2 = loss_fn(infer, y, loss)
    opt.zero_grad()
    lo.backward()
    grads = {k: v.grad.detach().clone() for k, v in model.named_parameters()}
    opt.step()
    sched.step()
    return float(lo.detach()), float(l2.detach()), grads


def main():
    ref = mg.ref_shims.load_reference()
    spec = importlib.util.spec_from_file_location('ref_pytorch_ssim', os.path.join(mg.ref_shims.REF_ROOT, 'pytorch_ssim', '__init__.py'))
    ref_ssim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_ssim)
    ns = mg._exec_defs(os.path.join(mg.ref_shims.REF_ROOT, 'train_network.py'), ('compute_loss',), dict(F=F, ssim_fun=ref_ssim.SSIM()))
    sd = syn.compennet_pp_state_dict(SEED, out_size=PRJ_SZ)
    holder = types.SimpleNamespace
    out, diff = {}, 0.0

    def record(tag, it, lo, l2, grads, params, keys):
        out[f'{tag}loss{it}'], out[f'{tag}l2_{it}'] = lo, l2
        out[f'{tag}gradnorm{it}'] = np.array([float(grads[k].double().norm()) for k in sorted(grads)])
        for k in keys:
            out[f'{tag}grad{it}.{k}'] = grads[k].numpy()
            out[f'{tag}param{it}.{k}'] = params[k].detach().numpy().copy()

    def compare(orc, lo, l2, grads, params, lo_o, l2_o):
        d = max(abs(lo - lo_o), abs(l2 - l2_o))
        for k, g in grads.items():
            d = max(d, float((orc.grads[k] - g).abs().max()) / max(1.0, float(g.abs().max())))
            d = max(d, float((orc.p[k].detach() - params[k].detach()).abs().max()))
        return d

    # ---- CompenNet++: camera CAM_SZ -> projector PRJ_SZ
    net = ref.models.CompenNetPlusplus(holder(module=ref.models.WarpingNet(out_size=PRJ_SZ)), holder(module=ref.models.CompenNet()))
    net.load_state_dict(sd)
    opt = torch.optim.Adam(filter(lambda p: p.requires_grad, net.parameters()), lr=LR, weight_decay=L2_REG)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=DROP_RATE, gamma=DROP_RATIO)
    scene = syn.scenes(SEED + 1, 1, CAM_SZ)
    orc = CompenNetTrainOracle(sd, scene, BSZ, PRJ_SZ, LR, L2_REG, DROP_RATE, DROP_RATIO)
    for it, loss in enumerate(LOSSES):
        cam, prj = pp_inputs(SEED, it, BSZ, CAM_SZ, PRJ_SZ)
        lo, l2, grads = run(net, cam, scene.expand(BSZ, -1, -1, -1), prj, opt, sched, ns['compute_loss'], loss)
        lo_o, l2_o = orc.step(cam, prj, loss)
        params = dict(net.named_parameters())
        diff = max(diff, compare(orc, lo, l2, grads, params, lo_o, l2_o))
        record('', it, lo, l2, grads, params, PP_KEYS)
    names = sorted(grads)
    # ---- bare CompenNet (init_compennet: no warp, target |prj - 0.3 s| -> prj)
    cn = ref.models.CompenNet()
    cn.load_state_dict(compen_only(sd))
    opt = torch.optim.Adam(filter(lambda p: p.requires_grad, cn.parameters()), lr=LR, weight_decay=L2_REG)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=DROP_RATE, gamma=DROP_RATIO)
    s, x, y = cn_inputs(SEED, BSZ, PRJ_SZ)
    orc = CompenNetTrainOracle(compen_only(sd), s, BSZ, None, LR, L2_REG, DROP_RATE, DROP_RATIO)
    lo, l2, grads = run(cn, x, s.expand(BSZ, -1, -1, -1), y, opt, sched, ns['compute_loss'], 'l1+ssim')
    lo_o, l2_o = orc.step(x, y, 'l1+ssim')
    params = dict(cn.named_parameters())
    diff = max(diff, compare(orc, lo, l2, grads, params, lo_o, l2_o))
    record('cn_', 0, lo, l2, grads, params, CN_KEYS)
    print(f'{NAME}: oracle maxdiff {diff:.3e}; losses {out["loss0"]:.6f} {out["loss1"]:.6f} (bare {out["cn_loss0"]:.6f})')
    mg.save(NAME, seed=SEED, cam_sz=CAM_SZ, prj_sz=PRJ_SZ, bsz=BSZ, lr=LR, l2_reg=L2_REG, lr_drop_rate=DROP_RATE,
            lr_drop_ratio=DROP_RATIO, losses=np.array(LOSSES), names=np.array(names), cn_names=np.array(sorted(grads)),
            wsum=mg.weights_checksum(sd), oracle_maxdiff=diff, **out)


if __name__ == '__main__':
    torch.manual_seed(0)
    main()
