"""GPU (-m gpu): CompenNet++ training on HIP (spaa_amd/train_network.py CompenNetTrainer, train_compennet_pp, init_compennet,
evaluate_model; csrc/compennet_train.hip) against torch autograd, the CPU oracle (tests/compennet_train_oracle.py) and the
reference fixture tests/golden/compennet_train_48x64.npz."""
import math
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spaa_oracle as so
from compennet_train_oracle import CompenNetTrainOracle, compen_only, pp_inputs, cn_inputs
from spaa_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def nhwc4(x):
    b, c, h, w = x.shape
    out = torch.zeros(b, h, w, 4, dtype=x.dtype)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out.contiguous()


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    _lib.load()
    return _lib


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3, 24])
@pytest.mark.parametrize('C,cs', [(32, 32), (20, 32), (256, 260)])
def test_batch_sum_gate(lib, B, C, cs):
    H, W = 7, 9
    gen = torch.Generator().manual_seed(B * 1000 + C)
    g = torch.randn(B, H, W, cs, generator=gen)
    act = torch.randn(1, H, W, cs, generator=gen)
    out = torch.full((1, H, W, cs), 7.0)
    gd, ad, od = g.to(DEV), act.to(DEV), out.to(DEV)
    lib.call('spaa_batch_sum_gate', lib.ptr(gd), lib.ptr(ad), lib.ptr(od), B, H, W, C, cs)
    want = (act[..., :C] > 0).double() * g[..., :C].double().sum(0, keepdim=True)
    got = od.cpu()
    assert float((got[..., :C].double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    assert torch.equal(got[..., C:], out[..., C:])                 # channels past C are not written
    od2 = torch.full_like(od, 7.0)
    lib.call('spaa_batch_sum_gate', lib.ptr(gd), lib.ptr(ad), lib.ptr(od2), B, H, W, C, cs)
    assert torch.equal(od2, od)                                    # fixed summation order: bitwise deterministic


def test_warp_bwd_grid2(lib):
    """Grid gradient of two sources of different batch (3 and 1), non-square source (12 x 20) != output (16 x 16), against torch
    autograd of F.grid_sample(align_corners=True) and against the sum of two spaa_warp_bwd_grid launches."""
    gen = torch.Generator().manual_seed(3)
    Hs, Ws, Ho, Wo, Ba, Bb = 12, 20, 16, 16, 3, 1
    xa, xb = torch.rand(Ba, 3, Hs, Ws, generator=gen), torch.rand(Bb, 3, Hs, Ws, generator=gen)
    ga, gb = torch.randn(Ba, 3, Ho, Wo, generator=gen), torch.randn(Bb, 3, Ho, Wo, generator=gen)
    grid = (torch.rand(1, Ho, Wo, 2, generator=gen) * 2.1 - 1.05).double().requires_grad_(True)
    loss = (ga.double() * F.grid_sample(xa.double(), grid.expand(Ba, -1, -1, -1), align_corners=True)).sum() + \
        (gb.double() * F.grid_sample(xb.double(), grid.expand(Bb, -1, -1, -1), align_corners=True)).sum()
    loss.backward()
    want = grid.grad[0]
    grid4 = torch.zeros(Ho, Wo, 4)
    grid4[..., :2] = grid.detach()[0].float()
    t = {k: v.to(DEV) for k, v in dict(ga=nhwc4(ga), xa=nhwc4(xa), gb=nhwc4(gb), xb=nhwc4(xb), grid=grid4).items()}
    out = torch.full((Ho, Wo, 4), 5.0, device=DEV)
    lib.call('spaa_warp_bwd_grid2', lib.ptr(t['ga']), lib.ptr(t['xa']), Ba, lib.ptr(t['gb']), lib.ptr(t['xb']), Bb, lib.ptr(t['grid']),
             lib.ptr(out), Hs, Ws, Ho, Wo)
    got = out.cpu()
    assert float((got[..., :2].double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert float(got[..., 2:].abs().max()) == 0.0
    oa, ob = torch.zeros(Ho, Wo, 4, device=DEV), torch.zeros(Ho, Wo, 4, device=DEV)
    lib.call('spaa_warp_bwd_grid', lib.ptr(t['ga']), lib.ptr(t['xa']), lib.ptr(t['grid']), None, lib.ptr(oa), Ba, Hs, Ws, Ho, Wo)
    lib.call('spaa_warp_bwd_grid', lib.ptr(t['gb']), lib.ptr(t['xb']), lib.ptr(t['grid']), None, lib.ptr(ob), Bb, Hs, Ws, Ho, Wo)
    assert float((out - (oa + ob)).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))


# ---------------------------------------------------------------------------------------------------------------
def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, 'compennet_train_48x64.npz'))
    hyper = dict(lr=float(z['lr']), l2_reg=float(z['l2_reg']), lr_drop_rate=int(z['lr_drop_rate']), lr_drop_ratio=float(z['lr_drop_ratio']))
    return (z, int(z['seed']), int(z['bsz']), tuple(int(v) for v in z['cam_sz']), tuple(int(v) for v in z['prj_sz']), hyper,
            [str(v) for v in z['losses']])


def _compare_step(it, tr, orc, z, tag, lo, l2, lh, l2h, p_before, model, hyper, adam):
    """Loss, every gradient (oracle and fixture), the Adam update at the step's StepLR rate; returns the worst gradient rel L2."""
    assert abs(lh - lo) < 2e-5 * max(1.0, abs(lo)) and abs(l2h - l2) < 1e-6, (it, lh, lo, l2h, l2)
    if it == 0:   # (the fixture's later iterations follow the reference's own parameters, see _run_two_steps)
        assert abs(lh - float(z[f'{tag}loss{it}'])) < 2e-5 * max(1.0, abs(lo)) and abs(l2h - float(z[f'{tag}l2_{it}'])) < 1e-6
    worst = ('', 0.0)
    for name, g_ref in orc.grads.items():
        e = rel_l2(tr.grads[name].reshape(g_ref.shape), g_ref)
        worst = max(worst, (name, e), key=lambda t: t[1])
        assert e < 2e-3, (it, name, e)
    for key in z.files:
        if it == 0 and key.startswith(f'{tag}grad{it}.'):
            k = key[len(f'{tag}grad{it}.'):]
            assert rel_l2(tr.grads[k].reshape(z[key].shape), torch.from_numpy(z[key])) < 2e-3, key
    lr = hyper['lr'] * hyper['lr_drop_ratio'] ** (it // hyper['lr_drop_rate'])
    hp = dict(model.named_parameters())
    for name in orc.p:
        g = tr.grads[name].reshape(p_before[name].shape).cpu().double() + hyper['l2_reg'] * p_before[name].double()
        m_, v_ = adam.get(name, (0.0, 0.0))
        m_, v_ = 0.9 * m_ + 0.1 * g, 0.999 * v_ + 0.001 * g * g
        adam[name] = (m_, v_)
        t_ = it + 1
        want = p_before[name].double() - (lr / (1 - 0.9 ** t_)) * m_ / (v_.sqrt() / math.sqrt(1 - 0.999 ** t_) + 1e-8)
        assert float((hp[name].detach().cpu().double() - want).abs().max()) < 1e-6 + 2e-3 * lr, (it, name)
    return worst


def _run_two_steps(model, tr, orc, z, tag, hyper, steps):
    """From the second step on the oracle starts from the HIP parameters: Adam's first update is +-lr wherever a gradient element
    is not zero, so an element within rounding of zero can take the opposite sign -- a 1e-3 step of a grid-refine weight initialised
    at 1e-4 scale -- and the two runs would no longer evaluate the same point.  The CPU test pins the oracle's trajectory to the
    reference's (tests/test_compennet_train_cpu.py); the Adam restatement below checks every HIP update."""
    adam, worst = {}, ('', 0.0)
    for it, (x, y, loss) in enumerate(steps):
        p_before = {n: v.detach().cpu().clone() for n, v in model.named_parameters()}
        if it > 0:
            with torch.no_grad():
                for n, v in p_before.items():
                    orc.p[n].copy_(v)
        lo, l2 = orc.step(x, y, loss)
        lr_used = tr.lr
        lh, l2h = tr.step(x, y, loss)
        assert lr_used == orc.opt.param_groups[0]['initial_lr'] * hyper['lr_drop_ratio'] ** it   # StepLR: the drop shows in step 2
        w = _compare_step(it, tr, orc, z, tag, lo, l2, lh, l2h, p_before, model, hyper, adam)
        worst = max(worst, w, key=lambda t: t[1])
        print(f'{tag or "pp"} step {it} ({loss}, lr {lr_used:g}): loss {lh:.6f} vs oracle {lo:.6f}; worst gradient rel L2 '
              f'{w[1]:.2e} ({w[0]})')
    assert tr.iters == len(steps)
    return worst


def test_compennet_pp_training_steps(golden_dir):
    from spaa_amd.models import CompenNetPlusplus, WarpingNet, CompenNet
    from spaa_amd.train_network import CompenNetTrainer
    z, seed, bsz, cam_sz, prj_sz, hyper, losses = _fixture(golden_dir)
    sd = syn.compennet_pp_state_dict(seed, out_size=prj_sz)
    model = CompenNetPlusplus(WarpingNet(out_size=prj_sz), CompenNet())
    model.load_state_dict(sd)
    model = model.to(DEV)
    scene = syn.scenes(seed + 1, 1, cam_sz)
    cam0 = pp_inputs(seed, 0, bsz, cam_sz, prj_sz)[0]
    with torch.no_grad():
        y_before = model(cam0.to(DEV), scene.to(DEV)).cpu()          # (fills the model's cached grid and packed weights)
    assert float((y_before - so.compennet_pp_forward(sd, cam0, scene.expand(bsz, -1, -1, -1), prj_sz)).abs().max()) < 1e-4
    orc = CompenNetTrainOracle(sd, scene, bsz, prj_sz, **hyper)
    tr = CompenNetTrainer(model, scene, bsz, device=DEV, **hyper)
    steps = [(*pp_inputs(seed, it, bsz, cam_sz, prj_sz), loss) for it, loss in enumerate(losses)]
    worst = _run_two_steps(model, tr, orc, z, '', hyper, steps)
    print(f'CompenNet++: largest gradient rel L2 over both steps {worst[1]:.2e} ({worst[0]})')
    # the model's own forward after training uses the trained parameters (no stale grid / packed weights)
    trained = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    cam = steps[1][0]
    with torch.no_grad():
        y = model(cam.to(DEV), scene.to(DEV)).cpu()
    want = so.compennet_pp_forward(trained, cam, scene.expand(bsz, -1, -1, -1), prj_sz)
    assert float((y - want).abs().max() / want.abs().max()) <= 1e-4
    assert float((y - y_before).abs().max()) > 1e-3


def test_bare_compennet_training_step(golden_dir):
    from spaa_amd.models import CompenNet
    from spaa_amd.train_network import CompenNetTrainer
    z, seed, bsz, cam_sz, prj_sz, hyper, _ = _fixture(golden_dir)
    sd = compen_only(syn.compennet_pp_state_dict(seed, out_size=prj_sz))
    cn = CompenNet()
    cn.load_state_dict(sd)
    cn = cn.to(DEV)
    s, x, y = cn_inputs(seed, bsz, prj_sz)
    with torch.no_grad():
        cn(x.to(DEV), s.to(DEV))
    orc = CompenNetTrainOracle(sd, s, bsz, None, **hyper)
    tr = CompenNetTrainer(cn, s, bsz, device=DEV, **hyper)
    x2, y2 = torch.flip(x, dims=[0]).contiguous(), torch.flip(y, dims=[0]).contiguous()
    worst = _run_two_steps(cn, tr, orc, z, 'cn_', hyper, [(x, y, 'l1+ssim'), (x2, y2, 'l1+ssim')])
    print(f'CompenNet: largest gradient rel L2 over both steps {worst[1]:.2e} ({worst[0]})')
    trained = {k: v.detach().cpu() for k, v in cn.state_dict().items()}
    with torch.no_grad():
        out = cn(x.to(DEV), s.to(DEV)).cpu()
    want = so.compennet_forward(trained, x, s.expand(bsz, -1, -1, -1), prefix='')
    assert float((out - want).abs().max() / want.abs().max()) <= 1e-4


# ---------------------------------------------------------------------------------------------------------------
def test_train_compennet_pp_end_to_end(tmp_path, monkeypatch):
    """A small synthetic setup (camera 48 x 64 -> projector 64 x 64, a learnable photometric target): the loss falls, the returned
    validation metrics are evaluate_model's, which are metrics.calc_img_dists of the same inference; the checkpoint is written."""
    from spaa_amd import metrics, io
    from spaa_amd import train_network as tn
    from spaa_amd.models import CompenNetPlusplus, WarpingNet, CompenNet
    cam_sz, prj_sz, n_train, n_valid = (48, 64), (64, 64), 16, 6
    model = CompenNetPlusplus(WarpingNet(out_size=prj_sz), CompenNet())
    model.load_state_dict(syn.compennet_pp_state_dict(11, out_size=prj_sz))
    model = model.to(DEV)
    scene = syn.scenes(12, 1, cam_sz)
    cam = syn.scenes(13, n_train + n_valid, cam_sz)
    prj = (0.6 * F.interpolate(cam, size=prj_sz, mode='bilinear', align_corners=True) + 0.2).contiguous()
    train = dict(cam_scene=scene, cam_train=cam[:n_train], prj_train=prj[:n_train])
    valid = dict(cam_scene=scene, cam_valid=cam[n_train:], prj_valid=prj[n_train:])
    cfg = dict(device=DEV, max_iters=100, batch_size=4, num_train=n_train, lr=1e-3, l2_reg=1e-4, lr_drop_rate=800, lr_drop_ratio=0.2,
               loss='l1+ssim', setup_name='synthetic', data_root=str(tmp_path / 'data'))
    seen = []
    step = tn.CompenNetTrainer.step

    def rec(self, *a, **k):
        r = step(self, *a, **k)
        seen.append(r[0])
        return r

    monkeypatch.setattr(tn.CompenNetTrainer, 'step', rec)
    random.seed(0)
    model, psnr, rmse, ssim = tn.train_compennet_pp(model, train, valid, cfg)
    assert len(seen) == 100 and all(math.isfinite(v) for v in seen)
    first, last = np.mean(seen[:5]), np.mean(seen[-5:])
    print(f'train_compennet_pp: loss {first:.4f} -> {last:.4f}; valid PSNR {psnr:.3f} RMSE {rmse:.4f} SSIM {ssim:.4f}')
    assert last < 0.3 * first
    e = tn.evaluate_model(model, valid)
    assert np.allclose((psnr, rmse, ssim), e[:3], rtol=1e-6, atol=0)
    p1, r1, s1, infer = tn.evaluate_model(model, valid, chunk_sz=1)
    d = metrics.calc_img_dists(infer, valid['prj_valid'])
    assert np.allclose((p1, r1, s1), d[:3], rtol=1e-6, atol=0)
    with torch.no_grad():
        assert float((infer - model(valid['cam_valid'].to(DEV), scene.to(DEV)).cpu()).abs().max()) <= 1e-6
    title = io.opt_to_string(dict(cfg, model_name='CompenNet++'))
    ck = tmp_path / 'checkpoint' / (title + '.pth')
    assert ck.exists()
    saved = torch.load(ck)
    for k, v in model.state_dict().items():
        assert torch.equal(saved[k].cpu(), v.cpu()), k


def test_init_compennet(tmp_path, monkeypatch):
    from spaa_amd import io
    from spaa_amd import train_network as tn
    from spaa_amd.models import CompenNet
    root = tmp_path / 'setup'
    io.save_imgs(syn.scenes(21, 1, (32, 32)), str(root / 'prj_share' / 'init'))
    io.save_imgs(syn.scenes(22, 6, (32, 32)), str(root / 'prj_share' / 'train'))
    torch.manual_seed(0)
    cn = CompenNet().to(DEV)
    w0 = {k: v.detach().clone() for k, v in cn.state_dict().items()}
    random.seed(1)
    cn1 = tn.init_compennet(cn, str(root), dict(device=DEV), max_iters=3, batch_size=4, num_train=6)
    ck = tmp_path / 'checkpoint' / 'init_CompenNet_l1+ssim_6_4_3_0.001_0.2_800_0.0001.pth'
    assert ck.exists()
    first = {k: v.detach().cpu().clone() for k, v in cn1.state_dict().items()}
    assert any(not torch.equal(first[k], w0[k].cpu()) for k in first)

    def no_training(*a, **k):
        raise AssertionError('init_compennet trained although its checkpoint exists')

    monkeypatch.setattr(tn, 'train_compennet_pp', no_training)
    torch.manual_seed(1)
    cn2 = tn.init_compennet(CompenNet().to(DEV), str(root), dict(device=DEV), max_iters=3, batch_size=4, num_train=6)
    for k, v in cn2.state_dict().items():
        assert torch.equal(v.cpu(), first[k]), k
    with torch.no_grad():   # (the loaded weights reach the forward pass)
        s = syn.scenes(21, 1, (32, 32)).to(DEV)
        x = syn.scenes(22, 2, (32, 32)).to(DEV)
        assert float((cn2(x, s) - cn1(x, s)).abs().max()) <= 1e-6


def test_errors():
    from spaa_amd.models import CompenNetPlusplus, WarpingNet, CompenNet
    from spaa_amd.train_network import CompenNetTrainer
    scene = syn.scenes(1, 1, (48, 64))
    model = CompenNetPlusplus(WarpingNet(out_size=(64, 64)), CompenNet()).to(DEV)
    tr = CompenNetTrainer(model, scene, 2, device=DEV)
    cam, prj = syn.scenes(2, 2, (48, 64)), syn.scenes(3, 2, (64, 64))
    for opt in ('l2', 'l1+l2', 'huber', 'l1+ssim+huber'):
        with pytest.raises(NotImplementedError):
            tr.step(cam, prj, opt)
    with pytest.raises(TypeError):
        tr.step(cam, prj, '')
    with pytest.raises(ValueError):
        tr.step(cam[:1], prj[:1])                    # batch differs from the trainer's
    assert tr.iters == 0
    with pytest.raises(NotImplementedError):
        CompenNetTrainer(CompenNetPlusplus(WarpingNet(out_size=(64, 64), with_refine=False), CompenNet()).to(DEV), scene, 2, device=DEV)
    with pytest.raises(ValueError):
        CompenNetTrainer(CompenNetPlusplus(WarpingNet(out_size=(62, 64)), CompenNet()).to(DEV), scene, 2, device=DEV)
    with pytest.raises(RuntimeError):
        CompenNetTrainer(CompenNetPlusplus(WarpingNet(out_size=(64, 64)), CompenNet()), scene, 2, device='cpu')
    with pytest.raises(ValueError):
        CompenNetTrainer(CompenNetPlusplus(WarpingNet(out_size=(64, 64)), CompenNet()), scene, 2, device=DEV)   # parameters on the host
    with pytest.raises(TypeError):
        CompenNetTrainer(torch.nn.Linear(2, 2).to(DEV), scene, 2, device=DEV)
