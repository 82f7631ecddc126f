"""GPU (-m gpu): training the PCNet ablation variants on HIP (spaa_amd/train_network.py PCNetTrainer for use_mask / use_rough /
with_refine / fix_shading_net; spaa_batch_sum_gate_bits in csrc/train_ops.hip)
against the CPU restatement (tests/pcnet_variant_oracle.py) and the reference fixtures (tests/golden/make_golden_pcnet_variants.py)."""
import math
import os

import numpy as np
import pytest
import torch

import pcnet_variant_oracle as pvo
import spaa_oracle as so
from spaa_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCENE_ONLY = ('conv1_s', 'conv2_s', 'conv3_s', 'conv4_s', 'skipConv1.0', 'skipConv1.2', 'skipConv1.4')


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    _lib.load()
    return _lib


def make_variant(variant, cam_sz=pvo.CAM_SZ):
    from spaa_amd.models import PCNet, WarpingNet
    use_mask, use_rough, with_refine, fix, seed = pvo.VARIANTS[variant]
    sd = pvo.variant_sd(seed, use_mask, use_rough, with_refine, cam_sz)
    pc = PCNet(sd.get('mask'), WarpingNet(out_size=cam_sz, with_refine=with_refine), fix_shading_net=fix, use_mask=use_mask,
               use_rough=use_rough)
    pc.load_state_dict(sd)
    return pc.to(DEV), sd


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3, 24])
@pytest.mark.parametrize('C,cs', [(32, 32), (20, 32), (256, 260), (4, 4)])
def test_batch_sum_gate_bits(lib, B, C, cs):
    """out = gate(sum_b g[b] + add) against the sequential fp32 sum over b (then add, then the gate), bitwise; gate bytes in the
    engine's format (bit e of byte q: channel 4 q + e passes); channels past C are not written."""
    H, W = 7, 9
    gen = torch.Generator().manual_seed(B * 1000 + C)
    g = torch.randn(B, H, W, cs, generator=gen)
    add = torch.randn(1, H, W, cs, generator=gen)
    bits = torch.randint(0, 16, (1, H, W, cs // 4), generator=gen, dtype=torch.uint8)
    chan = torch.arange(cs)
    passes = ((bits.long()[..., chan // 4] >> (chan % 4)) & 1).bool()
    gd, ad, bd = g.to(DEV), add.to(DEV), bits.to(DEV)
    from spaa_amd.models import C_ptr
    for with_add in (False, True):
        for with_gate in (False, True):
            want = g[0].clone()
            for b in range(1, B):
                want = want + g[b]                                   # fp32, b in order
            if with_add:
                want = want + add[0]
            if with_gate:
                want = torch.where(passes[0], want, torch.zeros_like(want))
            out = torch.full((1, H, W, cs), 7.0, device=DEV)
            lib.call('spaa_batch_sum_gate_bits', lib.ptr(gd), lib.ptr(ad) if with_add else None, C_ptr(bd) if with_gate else None,
                     lib.ptr(out), B, H, W, C, cs)
            got = out.cpu()[0]
            assert torch.equal(got[..., :C], want[..., :C]), (with_add, with_gate)
            assert bool((got[..., C:] == 7.0).all())


def _adam_check(tr, pc, p_before, adam_m, adam_v, it):
    """torch.optim.Adam semantics applied to the HIP gradients, for every parameter the trainer trains."""
    hp = dict(pc.named_parameters())
    for gname, grp in tr.groups.items():
        for name in grp['names']:
            lr, wd = grp['lr'], grp['wd']
            g = tr.grads[name].reshape(p_before[name].shape).cpu().double() + wd * p_before[name].double()
            adam_m[name] = 0.9 * adam_m.get(name, 0.0) + 0.1 * g
            adam_v[name] = 0.999 * adam_v.get(name, 0.0) + 0.001 * g * g
            t_ = it + 1
            want = p_before[name].double() - (lr / (1 - 0.9 ** t_)) * adam_m[name] / (adam_v[name].sqrt() / math.sqrt(1 - 0.999 ** t_) + 1e-8)
            got = hp[name].detach().cpu().double()
            assert float((got - want).abs().max()) < 1e-6 + 2e-3 * lr, (it, name, float((got - want).abs().max()))


@pytest.mark.parametrize('variant', list(pvo.VARIANTS))
def test_variant_training_steps(lib, golden_dir, variant):
    """Two steps of one PCNetTrainer against the CPU restatement (loss, l2, every gradient, the Adam update), the first step also
    against the reference's own modules (fixture); fix_shading_net: the ShadingNet's parameters bitwise unchanged."""
    from spaa_amd.train_network import PCNetTrainer
    use_mask, use_rough, with_refine, fix, seed = pvo.VARIANTS[variant]
    pc, sd = make_variant(variant)
    assert len(pc.state_dict()) == 46 - (not use_mask) - 8 * (not with_refine)
    scene = syn.scenes(seed + 1, 1, pvo.CAM_SZ)
    orc = pvo.PCNetVariantOracle(sd, scene, pvo.BSZ, use_mask, use_rough, with_refine, fix)
    tr = PCNetTrainer(pc, scene, pvo.BSZ, device=DEV)
    assert tr.collapse                                       # every variant takes the batch-1 scene-only layers by default
    z = np.load(os.path.join(golden_dir, pvo.fixture_name(variant) + '.npz'))
    shading0 = {n: v.detach().clone() for n, v in pc.named_parameters() if 'warping_net' not in n}
    adam_m, adam_v = {}, {}
    for it, opt in enumerate(pvo.LOSSES):
        p_before = {n: v.detach().cpu().clone() for n, v in pc.named_parameters()}
        prj, cam = pvo.inputs(seed, it)
        if it > 0:
            # the second step's gradients at the SAME parameters: Adam's first steps are ~lr * sign(g), so a gradient within rounding
            # of zero moves the two parameter sets apart by up to 2 lr (the update itself is checked by _adam_check)
            with torch.no_grad():
                for k, v in orc.p.items():
                    v.copy_(p_before[k])
        lo, l2o = orc.step(prj, cam, opt)
        lh, l2h = tr.step(prj, cam, opt)
        assert abs(lh - lo) < 2e-5 * max(1.0, abs(lo)) and abs(l2h - l2o) < 1e-6, (it, lh, lo)
        assert sorted(tr.grads) == sorted(orc.grads)
        worst = ('', 0.0)
        for name, g_ref in orc.grads.items():
            e = rel_l2(tr.grads[name].reshape(g_ref.shape), g_ref)
            worst = max(worst, (name, e), key=lambda t: t[1])
            assert e < 2e-3, (it, name, e)
        print(f'{variant} step {it} ({opt}): loss {lh:.6f} vs {lo:.6f}; worst gradient rel L2 {worst[1]:.2e} ({worst[0]})')
        _adam_check(tr, pc, p_before, adam_m, adam_v, it)
        if it == 0:   # the reference's own first step
            assert abs(lh - float(z['loss0'])) < 2e-5 and abs(l2h - float(z['l2_0'])) < 1e-6
            names = [str(n) for n in z['names']]
            gn = np.array([float(tr.grads[k].double().norm()) for k in names])
            assert np.allclose(gn, z['gradnorm0'], rtol=2e-3), np.abs(gn / z['gradnorm0'] - 1).max()
            for key in z.files:
                if key.startswith('grad0.'):
                    k = key[len('grad0.'):]
                    assert rel_l2(tr.grads[k].reshape(z[key].shape), torch.from_numpy(z[key])) < 2e-3, key
    if fix:
        for n, v in pc.named_parameters():
            if 'warping_net' not in n:
                assert torch.equal(v.detach(), shading0[n]), n
                assert n not in tr.grads
    assert tr.iters == 2


def _no_rough_step(collapse):
    from spaa_amd.train_network import PCNetTrainer
    use_mask, use_rough, with_refine, fix, seed = pvo.VARIANTS['no_rough']
    pc, _ = make_variant('no_rough')
    tr = PCNetTrainer(pc, syn.scenes(seed + 1, 1, pvo.CAM_SZ), pvo.BSZ, device=DEV, collapse=collapse)
    prj, cam = pvo.inputs(seed, 0)
    loss = tr.step(prj, cam, 'l1+ssim')
    return loss, {k: v.detach().clone() for k, v in tr.grads.items()}, {k: v.detach().clone() for k, v in pc.named_parameters()}


def test_no_rough_collapse_matches_batch_b_and_is_reproducible(lib):
    """The collapsed no_rough step (scene-only layers at batch 1, gradients from the batch sums) against the same step at batch B:
    every scene-only layer's gradient within 1e-5 relative; and the collapsed step run twice: bitwise the same."""
    l_on, g_on, p_on = _no_rough_step(True)
    l_off, g_off, _ = _no_rough_step(False)
    assert abs(l_on[0] - l_off[0]) < 1e-6 * max(1.0, abs(l_off[0]))
    worst = 0.0
    for k in g_off:
        if any(k.startswith('shading_net.' + m + '.') for m in SCENE_ONLY):
            e = rel_l2(g_on[k], g_off[k])
            worst = max(worst, e)
            assert e < 1e-5, (k, e)
    print(f'collapse on vs off: worst scene-only gradient rel L2 {worst:.2e}')
    l_again, g_again, p_again = _no_rough_step(True)
    assert l_again == l_on
    for k in g_on:
        assert torch.equal(g_on[k], g_again[k]), k
    for k in p_on:
        assert torch.equal(p_on[k], p_again[k]), k


@pytest.mark.parametrize('variant', ['no_mask', 'wo_refine', 'no_mask_no_rough'])
def test_variant_forward_and_input_gradient(lib, variant):
    """PCNet.forward and its gradient w.r.t. x (what train_pcnet validates with) for use_mask=False / with_refine=False against
    the oracle (a ones mask for use_mask=False; the oracle's grid skips the refine net when the state dict has none)."""
    use_mask, use_rough, with_refine, fix, seed = pvo.VARIANTS[variant]
    pc, sd = make_variant(variant)
    pc.eval()
    b = 2
    x = syn.scenes(seed + 50, b, pvo.PRJ_SZ)
    s = syn.scenes(seed + 1, 1, pvo.CAM_SZ).expand(b, -1, -1, -1)
    r = torch.randn(b, 3, *pvo.CAM_SZ, generator=torch.Generator().manual_seed(seed))
    sdo = dict(sd)
    if not use_mask:
        sdo['mask'] = torch.ones(1, 1, *pvo.CAM_SZ)
    xo = x.clone().requires_grad_(True)
    yo = so.pcnet_forward(sdo, xo, s, use_rough=use_rough)
    (yo * r).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    y = pc(xd, s.to(DEV))
    assert rel_l2(y, yo) < 1e-5 and float((y.detach().cpu() - yo.detach()).abs().max()) < 1e-4
    (y * r.to(DEV)).sum().backward()
    assert rel_l2(xd.grad, xo.grad) < 2e-3


def test_train_pcnet_no_mask_no_rough_end_to_end(lib):
    """train_pcnet on PCNet_no_mask_no_rough (the paper's ablation, reproduce_paper_results.py:64) for 3 iterations, validation
    metrics finite; evaluate_model on the trained model."""
    from spaa_amd.train_network import train_pcnet, evaluate_model
    import random
    random.seed(0)
    pc, _ = make_variant('no_mask_no_rough')
    assert pc.name == 'PCNet_no_mask_no_rough'
    n = 6
    scene = syn.scenes(1, 1, pvo.CAM_SZ)
    train = dict(cam_scene=scene, prj_train=syn.scenes(60, n, pvo.PRJ_SZ), cam_train=syn.scenes(61, n, pvo.CAM_SZ) * 0.8 + 0.05)
    valid = dict(cam_scene=scene, prj_valid=syn.scenes(62, 4, pvo.PRJ_SZ), cam_valid=syn.scenes(63, 4, pvo.CAM_SZ) * 0.8 + 0.05)
    cfg = dict(max_iters=3, batch_size=3, num_train=n, l2_reg=1e-4, lr_drop_ratio=0.2, device=DEV)
    p0 = {k: v.detach().clone() for k, v in pc.named_parameters()}
    model, psnr, rmse, ssim = train_pcnet(pc, train, valid, cfg)
    assert all(math.isfinite(float(v)) for v in (psnr, rmse, ssim)), (psnr, rmse, ssim)
    assert any(not torch.equal(p0[k], v.detach()) for k, v in model.named_parameters())
    psnr2, rmse2, ssim2, infer = evaluate_model(model, dict(valid, cam_scene=scene))
    assert infer.shape == valid['cam_valid'].shape and all(math.isfinite(float(v)) for v in (psnr2, rmse2, ssim2))
