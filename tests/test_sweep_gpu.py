"""GPU: several attack configurations in one batch -- the _ps launches (per-sample loss weights, d_thr and targeted flag), a mixed
AttackState, spaa_sweep against the reference goldens, and the reference's attack driver (run_projector_based_attack)."""
import os

import numpy as np
import pytest
import torch

import spaa_oracle as so
from spaa_amd import synthetic as syn
from test_gpu_parity import hip, load, _setup_case  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SWEEP = ['spaa_64_untargeted', 'spaa_64_near', 'spaa_64_caml2_dthr', 'spaa_64_prjl2', 'spaa_64_imagenet10']


def _weights(loss):
    return [0.1 if 'prjl2' in loss else 0.0, 1.0 if 'caml2' in loss else 0.0, 1.0 if 'camdE' in loss else 0.0]


def _rand_case(B=12, HW=64 * 64, ncls=1000, seed=0):
    """Per-sample parameters covering {caml2}, {camdE}, {both}, {both + prjl2}, mixed targeted flags, d_thr either side of caml2."""
    g = torch.Generator().manual_seed(seed)
    losses = ['caml2', 'camdE', 'camdE_caml2', 'camdE_caml2_prjl2'] * (B // 4)
    targeted = [bool(b % 3 != 1) for b in range(B)]
    nblk = (HW + 255) // 256
    partial = torch.rand(B, nblk, 3, generator=g) * 256 * 0.05
    caml2 = partial[:, :, 0].sum(1) / HW
    d_thr = [float(caml2[b] * 255 * (0.8 if b % 2 else 1.2)) for b in range(B)]
    logits = torch.randn(B, ncls, generator=g) * 3
    target = torch.randint(0, ncls, (B,), generator=g, dtype=torch.int32)
    for b in range(0, B, 3):   # some samples whose top-1 is the target (targeted successes / untargeted failures)
        logits[b, int(target[b])] = 30.0
    stats = torch.zeros(B, 8)
    stats[:, 5] = torch.where(torch.arange(B) % 4 == 0, torch.tensor(1e6), torch.tensor(1e-3))
    prjl2 = torch.rand(B, generator=g)
    return dict(losses=losses, targeted=targeted, d_thr=d_thr, partial=partial.to(DEV), logits=logits.to(DEV),
                target=target.to(DEV), stats=stats.to(DEV), prjl2=prjl2.to(DEV), nblk=nblk, HW=HW, ncls=ncls)


def _table(losses, d_thr, targeted):
    params = torch.tensor([_weights(l) + [d] for l, d in zip(losses, d_thr)], dtype=torch.float32, device=DEV)
    flags = torch.tensor([int(t) for t in targeted], dtype=torch.int32, device=DEV)
    return params, flags


def test_ps_kernels_equal_scalar_launches(hip):
    """spaa_decide_ps / spaa_stealth_loss_fwd_bwd_ps / spaa_grad_sumsq_ps: per sample bitwise the scalar launch on that sample alone;
    with uniform parameters bitwise the scalar launch over the whole batch."""
    lib = hip['lib']
    p = lib.ptr
    c = _rand_case()
    B, HW, ncls, nblk = 12, c['HW'], c['ncls'], c['nblk']
    adv_scale, p_thresh = 1.0 / B, 0.9

    def decide_scalar(sl, loss, d_thr, targeted):
        w = _weights(loss)
        n = sl.stop - sl.start
        st, sts, gl = (torch.zeros(n, 4, dtype=torch.int32, device=DEV), c['stats'][sl].clone(),
                       torch.full((n, ncls), 7.0, device=DEV))
        lib.call('spaa_decide', p(c['logits'][sl].contiguous()), ncls, p(c['target'][sl].contiguous()), int(targeted),
                 p(c['partial'][sl].contiguous()), nblk, HW, p(c['prjl2'][sl].contiguous()) if w[0] else None, w[0], w[1], w[2],
                 float(d_thr), p_thresh, adv_scale, p(st), p(sts), p(gl), n)
        return st, sts, gl

    def decide_ps(losses, d_thr, targeted, with_prjl2=True):
        params, flags = _table(losses, d_thr, targeted)
        st, sts, gl = torch.zeros(B, 4, dtype=torch.int32, device=DEV), c['stats'].clone(), torch.full((B, ncls), 7.0, device=DEV)
        lib.call('spaa_decide_ps', p(c['logits']), ncls, p(c['target']), p(c['partial']), nblk, HW,
                 p(c['prjl2']) if with_prjl2 else None, p(params), p(flags), p_thresh, adv_scale, p(st), p(sts), p(gl), B)
        return st, sts, gl

    got = decide_ps(c['losses'], c['d_thr'], c['targeted'])
    assert got[0][:, 0].any() and not got[0][:, 0].all() and got[0][:, 1].any() and not got[0][:, 1].all()   # both sides exercised
    for b in range(B):
        ref = decide_scalar(slice(b, b + 1), c['losses'][b], c['d_thr'][b], c['targeted'][b])
        for r, g_, what in zip(ref, got, ('state', 'stats', 'g_logits')):
            assert torch.equal(g_[b:b + 1], r), (b, what)
    for loss in ('caml2', 'camdE_caml2_prjl2'):
        for tg in (True, False):
            ref = decide_scalar(slice(0, B), loss, 6.5, tg)
            got = decide_ps([loss] * B, [6.5] * B, [tg] * B, with_prjl2='prjl2' in loss)
            for r, g_ in zip(ref, got):
                assert torch.equal(g_, r), (loss, tg)

    # stealth loss: y == scene on some pixels (the zero-norm branch)
    torch.manual_seed(1)
    y = torch.rand(B, HW, 4, device=DEV)
    scene = torch.rand(B, HW, 4, device=DEV)
    y[..., 3] = scene[..., 3] = 0
    y[:, ::17] = scene[:, ::17]
    lab = torch.zeros_like(scene)
    lib.call('spaa_rgb2lab', p(scene), p(lab), B * HW)
    gscale = 1.0 / (B * HW)

    def stealth_scalar(sl, loss):
        w = _weights(loss)
        n = sl.stop - sl.start
        gy, part = torch.full((n, HW, 4), 3.0, device=DEV), torch.full((n, nblk, 3), 3.0, device=DEV)
        lib.call('spaa_stealth_loss_fwd_bwd', p(y[sl].contiguous()), p(scene[sl].contiguous()), p(lab[sl].contiguous()), w[1], w[2],
                 gscale, p(gy), None, p(part), n, HW)
        return gy, part

    def stealth_ps(losses):
        params, _ = _table(losses, [5.0] * B, [True] * B)
        gy, part = torch.full((B, HW, 4), 3.0, device=DEV), torch.full((B, nblk, 3), 3.0, device=DEV)
        lib.call('spaa_stealth_loss_fwd_bwd_ps', p(y), p(scene), p(lab), p(params), gscale, p(gy), None, p(part), B, HW)
        return gy, part

    got = stealth_ps(c['losses'])
    for b in range(B):
        ref = stealth_scalar(slice(b, b + 1), c['losses'][b])
        assert torch.equal(got[0][b:b + 1], ref[0]) and torch.equal(got[1][b:b + 1], ref[1]), b
    for loss in ('caml2', 'camdE', 'camdE_caml2'):
        ref, got = stealth_scalar(slice(0, B), loss), stealth_ps([loss] * B)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), loss

    # ||g||^2 with the prjl2 term of colour-step samples
    g0 = torch.randn(B, HW, 4, device=DEV)
    x = torch.rand(B, HW, 4, device=DEV)
    x[:, ::13, :3] = 0.5                                    # (zero-norm pixels)
    state = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    state[::2, 1] = 1
    state[7, 1] = 1                                         # (colour-step samples with and without the prjl2 term: 0, 7 / 11)
    scales = torch.tensor([_weights(l)[0] / (B * HW) for l in c['losses']], device=DEV)

    def sumsq_scalar(sl, scale):
        n = sl.stop - sl.start
        g, part = g0[sl].clone(), torch.full((n, nblk), 3.0, device=DEV)
        lib.call('spaa_grad_sumsq', p(g), p(x[sl].contiguous()), 0.5, float(scale), p(state[sl].contiguous()), p(part), n, HW)
        return g, part

    def sumsq_ps(sc):
        g, part = g0.clone(), torch.full((B, nblk), 3.0, device=DEV)
        lib.call('spaa_grad_sumsq_ps', p(g), p(x), 0.5, p(sc), p(state), p(part), B, HW)
        return g, part

    got = sumsq_ps(scales)
    assert not torch.equal(got[0], g0)                        # the prjl2 term was applied somewhere
    for b in range(B):
        ref = sumsq_scalar(slice(b, b + 1), float(scales[b]))
        assert torch.equal(got[0][b:b + 1], ref[0]) and torch.equal(got[1][b:b + 1], ref[1]), b
    for s in (0.0, float(scales[3])):
        ref, got = sumsq_scalar(slice(0, B), s), sumsq_ps(torch.full((B,), s, device=DEV))
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), s


def test_ps_warp_adjoint_sumsq_equals_scalar(hip):
    """spaa_warp_bwd_tiled_sumsq_ps against spaa_warp_bwd_tiled_sumsq on a 64 x 64 engine's tap tables (with and without the clamp
    bytes): per sample bitwise the scalar launch on that sample alone; uniform scales bitwise the scalar launch on the batch."""
    M, lib = hip['models'], hip['lib']
    p, cp = lib.ptr, M.C_ptr
    B, sz = 12, (64, 64)
    sd = syn.pcnet_state_dict(0, cam_sz=sz, mask='rect')
    pc = M.PCNet(sd['mask'], M.WarpingNet(out_size=sz))
    pc.load_state_dict(sd)
    eng = M.PCNetEngine(pc.to(DEV), B, sz)
    assert eng.tiled is not None
    lidx, w_e, tbox, cap = eng.tiled
    Hp, Wp = sz
    HWp, nt = Hp * Wp, eng.sumsq_tiles()
    torch.manual_seed(2)
    g_xw = torch.randn(B, sz[0], sz[1], 4, device=DEV)
    x = torch.rand(B, HWp, 4, device=DEV) * 1.4 - 0.2
    x[:, ::11, :3] = 0.5
    ok = (x[..., :3] >= 0) & (x[..., :3] <= 1)
    bits = (ok[..., 0].to(torch.uint8) | (ok[..., 1].to(torch.uint8) << 1) | (ok[..., 2].to(torch.uint8) << 2)).contiguous()
    state = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    state[::2, 1] = 1
    scales = torch.tensor([0.1 / (B * HWp) if b % 4 == 3 else 0.0 for b in range(B)], device=DEV)
    scales[1] = 0.37 / (B * HWp)

    def scalar(sl, scale, cb):
        n = sl.stop - sl.start
        gx, part = torch.full((n, HWp, 4), 3.0, device=DEV), torch.full((n, nt), 3.0, device=DEV)
        lib.call('spaa_warp_bwd_tiled_sumsq', p(g_xw[sl].contiguous()), p(x[sl].contiguous()), cp(eng.tap_off), cp(lidx), p(w_e),
                 cp(tbox), cap, p(gx), n, Hp, Wp, sz[0], sz[1], 1, 0.5, float(scale), p(state[sl].contiguous()), p(part),
                 p(cb[sl].contiguous()) if cb is not None else None)
        return gx, part

    def ps(sc, cb):
        gx, part = torch.full((B, HWp, 4), 3.0, device=DEV), torch.full((B, nt), 3.0, device=DEV)
        lib.call('spaa_warp_bwd_tiled_sumsq_ps', p(g_xw), p(x), cp(eng.tap_off), cp(lidx), p(w_e), cp(tbox), cap, p(gx), B, Hp, Wp,
                 sz[0], sz[1], 1, 0.5, p(sc), p(state), p(part), p(cb) if cb is not None else None)
        return gx, part

    for cb in (None, bits):
        got = ps(scales, cb)
        for b in range(B):
            ref = scalar(slice(b, b + 1), float(scales[b]), cb)
            assert torch.equal(got[0][b:b + 1], ref[0]) and torch.equal(got[1][b:b + 1], ref[1]), (b, cb is None)
        for s in (0.0, float(scales[1])):
            ref, got = scalar(slice(0, B), s, cb), ps(torch.full((B,), s, device=DEV), cb)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (s, cb is None)


def _sweep_case(hip, golden_dir):
    zs = [load(golden_dir, n) for n in SWEEP]
    for k in ('seed', 'scene_seed', 'mask', 'gain', 'sz', 'crop', 'input_sz'):
        assert all(np.array_equal(z[k], zs[0][k]) for z in zs), k
    sd, pc, clf, oclf, scene, setup = _setup_case(hip, zs[0])
    configs = [(str(z['stealth']), float(z['d_thr']), bool(z['targeted']), [int(t) for t in z['targets']]) for z in zs]
    return zs, pc, clf, scene, setup, configs


@pytest.mark.parametrize('max_batch', [64, 16])
def test_sweep_against_reference_goldens(hip, golden_dir, max_batch):
    """Five reference runs (35 samples: untargeted and targeted, three loss strings, d_thr 5 and 40) as ONE spaa_sweep -- one chunk of
    35, or chunks of 16 that split configs -- each config's slice held to test_spaa_fifty_iterations_statistics' bars against its own
    golden, and its iteration 0 to the golden's decisions and losses."""
    A = hip['attack']
    zs, pc, clf, scene, setup, configs = _sweep_case(hip, golden_dir)
    tr = []
    res = A.spaa_sweep(pc, clf, None, scene, setup, DEV, configs, max_batch=max_batch, trace=tr)
    assert len(tr) == -(-35 // max_batch) and len(res) == len(zs)
    st = np.concatenate([torch.stack([t[0] for t in chunk]).cpu().numpy() for chunk in tr], axis=1)    # [50, 35, 4]
    sts = np.concatenate([torch.stack([t[1] for t in chunk]).cpu().numpy() for chunk in tr], axis=1)   # [50, 35, 8]
    assert st.shape[:2] == (50, 35)
    a = 0
    for z, name, (cam, prj), cfg in zip(zs, SWEEP, res, configs):
        n = len(cfg[3])
        s, f = st[:, a:a + n], sts[:, a:a + n]
        a += n
        cam, prj = cam.cpu(), prj.cpu()
        assert cam.shape == (n, 3, 64, 64) and prj.shape == (n, 3, 64, 64)
        # iteration 0: decisions equal unless the reference sits on a knife edge; losses to 1e-4
        edge = (np.abs(z['p1'][0] - 0.9) < 1e-3) | (np.abs(z['caml2'][0] * 255 - cfg[1]) < 1e-2)
        assert ((s[0, :, 3] == z['top1'][0]) | edge).all(), (name, 'top1')
        assert ((s[0, :, 0] == z['succ'][0]) | edge).all() and ((s[0, :, 1] == z['best_adv'][0]) | edge).all(), (name, 'masks')
        assert np.allclose(f[0, :, 1], z['caml2'][0], rtol=1e-4) and np.allclose(f[0, :, 2], z['camdE'][0], rtol=1e-4), name
        # outcome after 50 iterations
        ever_hip, ever_ref = s[:, :, 2].any(axis=0), z['best'].any(axis=0)
        assert int((ever_hip != ever_ref).sum()) <= (1 if n >= 8 else 0), name
        if n >= 8:
            assert abs(int(s[-1, :, 0].sum()) - int(z['succ'][-1].sum())) <= 2, name
        sc = scene.expand(n, -1, -1, -1)
        ref_cam = torch.from_numpy(z['cam_infer_best'])

        def dist(c):
            l2 = torch.norm(c - sc, dim=1).mean().item()
            de = so.ciede2000_diff(so.rgb2lab_diff(c), so.rgb2lab_diff(sc.contiguous())).mean().item()
            return l2, de

        (l2h, deh), (l2r, der) = dist(cam), dist(ref_cam)
        print(f'{name} (max_batch {max_batch}): recorded best HIP {int(ever_hip.sum())} / reference {int(ever_ref.sum())} of {n}; '
              f'mean L2 {l2h:.5f} / {l2r:.5f}, mean dE {deh:.4f} / {der:.4f}')
        if l2r > 0:
            assert abs(l2h / l2r - 1) < 0.02 and abs(deh / der - 1) < 0.02, name
        else:
            assert l2h == 0.0 and torch.equal(prj, torch.from_numpy(z['prj_adv_best'])), name
        if name == 'spaa_64_imagenet10':   # Q7: nobody succeeds -> exactly the gray image and the scene
            assert (prj == 0.5).all() and torch.equal(cam, ref_cam)
        assert prj.min() >= 0 and prj.max() <= 1


@pytest.mark.parametrize('storage', ['f32', 'f16'])
def test_mixed_state_equals_separate_states(hip, golden_dir, storage):
    """One forward/decide on an AttackState holding the five configs against separate per-config AttackStates on the same x.
    (a) A per-config state of the same batch size (all 35 targets, that config's loss / targeted / d_thr): the network launches are the
    same, so the config's samples get bitwise its state and stats.  (b) fp32: a per-config state of the config's own size (other tile
    choices, other rounding): the same state except on knife edges, stats to 1e-5 of each column's scale.  (In fp16 storage a different
    batch size moves activations by fp16 ulps -- p1 by ~5e-4 --, so (b) is fp32 only.)"""
    A, M = hip['attack'], hip['models']
    zs, pc, clf, scene, setup, configs = _sweep_case(hip, golden_dir)
    losses = [c[0] for c in configs for _ in c[3]]
    d_thr = [c[1] for c in configs for _ in c[3]]
    targeted = [c[2] for c in configs for _ in c[3]]
    targets = [t for c in configs for t in c[3]]
    mixed = A.AttackState(pc, clf, targets, scene, losses, setup, DEV, storage=storage)
    torch.manual_seed(3)
    x = M.to_nhwc4((0.5 + 0.15 * torch.randn(len(targets), 3, 64, 64)).to(DEV))
    mixed.x.copy_(x)
    mixed.forward_decide(targeted, d_thr, 0.9)
    ms, mf = mixed.state.cpu().numpy(), mixed.stats.cpu().numpy()
    a = 0
    for loss, dt, tg, tgt in configs:
        n = len(tgt)
        same = A.AttackState(pc, clf, targets, scene, loss, setup, DEV, storage=storage)
        same.x.copy_(x)
        same.forward_decide(tg, dt, 0.9)
        assert np.array_equal(ms[a:a + n], same.state.cpu().numpy()[a:a + n]), (loss, dt, tg)
        assert np.array_equal(mf[a:a + n], same.stats.cpu().numpy()[a:a + n]), (loss, dt, tg)
        del same
        if storage == 'f32':
            sep = A.AttackState(pc, clf, tgt, scene, loss, setup, DEV, storage=storage)
            sep.x.copy_(x[a:a + n])
            sep.forward_decide(tg, dt, 0.9)
            ss, sf = sep.state.cpu().numpy(), sep.stats.cpu().numpy()
            edge = (np.abs(sf[:, 0] - 0.9) < 1e-3) | (np.abs(sf[:, 1] * 255 - dt) < 1e-2)
            assert ((ms[a:a + n] == ss).all(axis=1) | edge).all(), (loss, dt, tg)
            scale = np.abs(mf).max(axis=0, keepdims=True)
            assert (np.abs(mf[a:a + n] - sf) <= 1e-5 * scale).all(), (loss, dt, tg, np.abs(mf[a:a + n] - sf).max(axis=0))
            del sep
        a += n


def _write_labels(fn, labels):
    with open(fn, 'w') as fh:
        fh.write('{' + ',\n'.join(f"{k}: '{v}'" for k, v in labels.items()) + '}')


def test_run_projector_based_attack_spaa(hip, tmp_path):
    """The reference's driver on a 64 x 64 setup: its directory tree and file names, the PNGs equal to io.save_imgs of one spaa_sweep
    with the same arguments; One-pixel_DE and a missing model raise."""
    A = hip['attack']
    from spaa_amd import io
    from PIL import Image
    sz = (64, 64)
    sd = syn.pcnet_state_dict(0, cam_sz=sz, mask='rect')
    pc = hip['models'].PCNet(sd['mask'], hip['models'].WarpingNet(out_size=sz))
    pc.load_state_dict(sd)
    pc = pc.to(DEV)
    clf = hip['clf'].Classifier('resnet18', DEV, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0), input_sz=(56, 56))
    root = tmp_path / 'data'
    setup_path = root / 'setups' / 'synth'
    io.save_setup_info(str(setup_path), dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=sz, cam_im_sz=sz))
    io.save_imgs(syn.scenes(1, 2, sz), str(setup_path / 'cam/raw/ref'))           # img_0001, img_0002
    _write_labels(root / 'imagenet1000_clsidx_to_labels.txt', {k: f'class{k}, extra' for k in range(1000)})
    ten = [1, 7, 21, 207, 340, 745, 779, 846, 947, 950]
    _write_labels(root / 'imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in ten})
    cfg = A.get_attacker_cfg('SPAA', str(root), ['synth'], device_ids=[0])
    cfg.classifier_names, cfg.stealth_losses, cfg.d_threshes = ['resnet18'], ['caml2', 'camdE_caml2'], [5, 40]
    A.run_projector_based_attack(cfg, models={'synth': pc}, classifiers={'resnet18': clf})
    cfg_str = 'SPAA_PCNet_l1+ssim_500_24_2000'
    names = [f'img_{i:04d}.png' for i in range(1, 12)]
    leaves = {os.path.join(cfg_str, l, str(d), 'resnet18') for l in cfg.stealth_losses for d in cfg.d_threshes}
    for kind in ('prj/adv', 'cam/infer/adv'):
        base = setup_path / kind
        found = {os.path.relpath(dp, base) for dp, dn, fn in os.walk(base) if fn}
        assert found == leaves, (kind, found)
        for leaf in leaves:
            assert sorted(os.listdir(base / leaf)) == names
    assert sorted(os.listdir(setup_path / 'cam')) == ['infer', 'raw'] and sorted(os.listdir(setup_path / 'cam/raw')) == ['ref']
    # the same attacks through spaa_sweep, saved by io.save_imgs
    scene = io.torch_imread(str(setup_path / 'cam/raw/ref/img_0002.png'))
    true_idx = int(clf(scene.to(DEV), (60, 60))[0][0].argmax())
    configs = [c for l in cfg.stealth_losses for d in cfg.d_threshes for c in ((l, d, True, ten), (l, d, False, [true_idx]))]
    res = A.spaa_sweep(pc, clf, None, scene.to(DEV), io.load_setup_info(str(setup_path)), DEV, configs)
    k = 0
    for l in cfg.stealth_losses:
        for d in cfg.d_threshes:
            (ct, pt), (cu, pu) = res[k], res[k + 1]
            k += 2
            leaf = os.path.join(cfg_str, l, str(d), 'resnet18')
            for kind, ims in (('prj/adv', torch.cat((pt, pu))), ('cam/infer/adv', torch.cat((ct, cu)))):
                want = tmp_path / 'want' / kind / leaf
                io.save_imgs(ims, str(want))
                for nm in names:
                    a = np.asarray(Image.open(setup_path / kind / leaf / nm))
                    b = np.asarray(Image.open(want / nm))
                    assert np.array_equal(a, b), (kind, leaf, nm)
    with pytest.raises(NotImplementedError):
        A.run_projector_based_attack(A.get_attacker_cfg('One-pixel_DE', str(root), ['synth']))
    with pytest.raises(ValueError, match='models='):
        A.run_projector_based_attack(cfg, models={'other': pc}, classifiers={'resnet18': clf})
