"""Generates tests/golden/pcnet_train_<variant>.npz and compennet_pp_train_wo_refine.npz: two iterations ('l1+ssim', then 'l1')
of the REFERENCE's training loop body for the ablation models its drivers build by name (train_network.py:476-595 for PCNet,
:640-660 for CompenNet++): PCNet without the mask, without the rough input (ShadingNetSPAA(use_rough=False)), both, WarpingNet
without the grid-refine net ('w/o_refine'), a frozen ShadingNet (fix_shading_net=True), and CompenNet++ 'w/o_refine'.  The
unmodified reference modules are imported via oracle/ref_shims.py, with the optimisers / schedulers of train_network.py:247-265
(PCNet) resp. :147-150 (CompenNet++).  Runs only in the build container.

    python tests/golden/make_golden_pcnet_variants.py

The CompenNet++ fixture pins the CPU oracle only (tests/test_pcnet_variants_cpu.py): CompenNetTrainer keeps refusing
WarpingNet(with_refine=False), as tests/test_compennet_train_gpu.py::test_errors requires.

The test-side restatements (tests/pcnet_variant_oracle.py, tests/compennet_train_oracle.py) run alongside; their largest
difference is printed and stored (`oracle_maxdiff`).
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
import pcnet_variant_oracle as pvo  # noqa: E402
from compennet_train_oracle import CompenNetTrainOracle, pp_inputs  # noqa: E402
from spaa_amd import synthetic as syn  # noqa: E402

CN_NAME, CN_CAM_SZ, CN_PRJ_SZ, CN_BSZ, CN_SEED = 'compennet_pp_train_wo_refine', (48, 64), (64, 64), 3, 17
CN_KEYS = ('warping_net.affine_mat', 'warping_net.theta', 'compen_net.conv1_s.weight', 'compen_net.conv6.weight',
           'compen_net.skipConv1.0.weight', 'compen_net.transConv2.bias')


def reference_compute_loss(ref):
    spec = importlib.util.spec_from_file_location('ref_pytorch_ssim', os.path.join(mg.ref_shims.REF_ROOT, 'pytorch_ssim', '__init__.py'))
    ref_ssim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_ssim)
    ns = mg._exec_defs(os.path.join(mg.ref_shims.REF_ROOT, 'train_network.py'), ('compute_loss',), dict(F=F, ssim_fun=ref_ssim.SSIM()))
    return ns['compute_loss']


def gen_pcnet_variant(ref, compute_loss, variant):
    use_mask, use_rough, with_refine, fix, seed = pvo.VARIANTS[variant]
    name, sz, bsz = pvo.fixture_name(variant), pvo.CAM_SZ, pvo.BSZ
    sd = pvo.variant_sd(seed, use_mask, use_rough, with_refine)
    holder = types.SimpleNamespace
    full = syn.pcnet_state_dict(seed, cam_sz=sz, mask='rect')
    model = ref.models.PCNet(full['mask'], holder(module=ref.models.WarpingNet(out_size=tuple(sz), with_refine=with_refine)),
                             holder(module=ref.models.ShadingNetSPAA(use_rough=use_rough)), fix_shading_net=fix, use_mask=use_mask,
                             use_rough=use_rough)
    model.load_state_dict(sd)
    named = [('module.' + k, v) for k, v in model.named_parameters()]       # (the reference wraps the model in DataParallel)
    aff = [v for k, v in named if k in ['module.warping_net.affine_mat', 'module.warping_net.theta']]
    refine = [v for k, v in named if 'module.warping_net.grid_refine_net' in k]
    shading = [v for k, v in named if 'module.warping_net' not in k]
    opts = [torch.optim.Adam([{'params': aff}], lr=1e-2, weight_decay=0), torch.optim.Adam([{'params': refine}], lr=5e-3, weight_decay=0),
            torch.optim.Adam([{'params': shading}], lr=1e-3, weight_decay=1e-4)]
    scheds = [torch.optim.lr_scheduler.MultiStepLR(o, milestones=[m], gamma=0.2) for o, m in zip(opts, (100, 1200, 1800))]
    scene = syn.scenes(seed + 1, 1, sz)
    orc = pvo.PCNetVariantOracle(sd, scene, bsz, use_mask, use_rough, with_refine, fix)
    out, diff = {}, 0.0
    for it, loss_opt in enumerate(pvo.LOSSES):
        prj, cam = pvo.inputs(seed, it)
        model.train()
        infer = model(prj, scene.expand(bsz, -1, -1, -1))
        loss, l2 = compute_loss(infer, cam, loss_opt)
        for o in opts:
            o.zero_grad()
        loss.backward()
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
        for o in opts:
            o.step()
        for s in scheds:
            s.step()
        lo, l2o = orc.step(prj, cam, loss_opt)
        params = dict(model.named_parameters())
        assert sorted(grads) == sorted(orc.grads), name
        diff = max(diff, abs(lo - float(loss)), abs(l2o - float(l2)),
                   max(float((orc.grads[k] - g).abs().max()) / max(1.0, float(g.abs().max())) for k, g in grads.items()),
                   max(float((orc.p[k].detach() - v.detach()).abs().max()) for k, v in params.items()))
        out[f'loss{it}'], out[f'l2_{it}'] = float(loss), float(l2)
        for k in pvo.KEYS:
            if k in grads:
                out[f'grad{it}.{k}'] = grads[k].numpy()
                out[f'param{it}.{k}'] = params[k].detach().numpy().copy()
        out[f'gradnorm{it}'] = np.array([float(grads[k].double().norm()) for k in sorted(grads)])
    # the frozen parameters after both steps (bitwise as loaded: Adam never saw them)
    frozen = sorted(k for k, v in model.named_parameters() if not v.requires_grad)
    assert all(torch.equal(dict(model.named_parameters())[k].detach(), sd[k]) for k in frozen)
    print(f'  {name}: oracle maxdiff {diff:.3e}; losses {out["loss0"]:.6f} {out["loss1"]:.6f}; {len(grads)} trained tensors')
    mg.save(name, seed=seed, cam_sz=sz, prj_sz=pvo.PRJ_SZ, bsz=bsz, use_mask=use_mask, use_rough=use_rough, with_refine=with_refine,
            fix_shading_net=fix, n_state=len(model.state_dict()), names=np.array(sorted(grads)), frozen=np.array(frozen, dtype=str),
            wsum=mg.weights_checksum(sd), oracle_maxdiff=diff, **out)


def gen_compennet_wo_refine(ref, compute_loss):
    sd = {k: v for k, v in syn.compennet_pp_state_dict(CN_SEED, out_size=CN_PRJ_SZ).items() if 'grid_refine_net' not in k}
    holder = types.SimpleNamespace
    net = ref.models.CompenNetPlusplus(holder(module=ref.models.WarpingNet(out_size=CN_PRJ_SZ, with_refine=False)),
                                       holder(module=ref.models.CompenNet()))
    net.load_state_dict(sd)
    lr, l2_reg, drop_rate, drop_ratio = 1e-3, 1e-4, 800, 0.2
    opt = torch.optim.Adam(filter(lambda p: p.requires_grad, net.parameters()), lr=lr, weight_decay=l2_reg)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=drop_rate, gamma=drop_ratio)
    scene = syn.scenes(CN_SEED + 1, 1, CN_CAM_SZ)
    orc = CompenNetTrainOracle(sd, scene, CN_BSZ, CN_PRJ_SZ, lr, l2_reg, drop_rate, drop_ratio)
    out, diff = {}, 0.0
    for it, loss_opt in enumerate(pvo.LOSSES):
        cam, prj = pp_inputs(CN_SEED, it, CN_BSZ, CN_CAM_SZ, CN_PRJ_SZ)
        net.train()
        infer = net(cam, scene.expand(CN_BSZ, -1, -1, -1))
        loss, l2 = compute_loss(infer, prj, loss_opt)
        opt.zero_grad()
        loss.backward()
        grads = {k: v.grad.detach().clone() for k, v in net.named_parameters()}
        opt.step()
        sched.step()
        lo, l2o = orc.step(cam, prj, loss_opt)
        params = dict(net.named_parameters())
        diff = max(diff, abs(lo - float(loss)), abs(l2o - float(l2)),
                   max(float((orc.grads[k] - g).abs().max()) / max(1.0, float(g.abs().max())) for k, g in grads.items()),
                   max(float((orc.p[k].detach() - v.detach()).abs().max()) for k, v in params.items()))
        out[f'loss{it}'], out[f'l2_{it}'] = float(loss), float(l2)
        for k in CN_KEYS:
            out[f'grad{it}.{k}'] = grads[k].numpy()
            out[f'param{it}.{k}'] = params[k].detach().numpy().copy()
        out[f'gradnorm{it}'] = np.array([float(grads[k].double().norm()) for k in sorted(grads)])
    print(f'  {CN_NAME}: oracle maxdiff {diff:.3e}; losses {out["loss0"]:.6f} {out["loss1"]:.6f}')
    mg.save(CN_NAME, seed=CN_SEED, cam_sz=CN_CAM_SZ, prj_sz=CN_PRJ_SZ, bsz=CN_BSZ, lr=lr, l2_reg=l2_reg, lr_drop_rate=drop_rate,
            lr_drop_ratio=drop_ratio, names=np.array(sorted(grads)), wsum=mg.weights_checksum(sd), oracle_maxdiff=diff, **out)


def main():
    ref = mg.ref_shims.load_reference()
    compute_loss = reference_compute_loss(ref)
    for variant in pvo.VARIANTS:
        gen_pcnet_variant(ref, compute_loss, variant)
    gen_compennet_wo_refine(ref, compute_loss)


if __name__ == '__main__':
    torch.manual_seed(0)
    main()
