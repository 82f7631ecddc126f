"""GPU: the direct-light mask kernels (csrc/direct_mask.hip) bit for bit against the numpy restatement of their rules
(tests/direct_mask_oracle.py), then the reference's drivers in front of the attack -- load_data, train_eval_pcnet,
train_eval_compennet_pp, run_projector_based_attack(train=True) -- on a synthetic setup rendered by a teacher PCNet."""
import faulthandler
import glob
import os

import numpy as np
import pandas as pd
import pytest
import torch

import direct_mask_oracle as dmo
from spaa_amd import synthetic as syn
from spaa_amd import io, img_proc
from spaa_amd import metrics as M
from spaa_amd import train_network as tn
from test_gpu_parity import hip  # noqa: F401  (hip: module fixture)
from test_sweep_gpu import _write_labels

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TIME_LIMIT = {'default': 120, 'test_train_eval_pcnet': 420, 'test_train_eval_compennet_pp': 420,
              'test_run_projector_based_attack_trains': 420}   # seconds per test


@pytest.fixture(autouse=True)
def time_limit(request):
    """Every test under its own time limit: a test still running after it (a hung launch does not return to Python) ends the
    process with a traceback instead of waiting."""
    faulthandler.dump_traceback_later(TIME_LIMIT.get(request.node.originalname, TIME_LIMIT['default']), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---------------------------------------------------------------------------------------------------------------------------------
def _poly_mask(h, w, pts):
    """Pixels inside the convex polygon `pts` (fractions of the image, counter-clockwise in (x, y))."""
    yy, xx = np.mgrid[0:h, 0:w]
    inside = np.ones((h, w), dtype=bool)
    p = [(x * (w - 1), y * (h - 1)) for x, y in pts]
    for (xa, ya), (xb, yb) in zip(p, p[1:] + p[:1]):
        inside &= (xb - xa) * (yy - ya) - (yb - ya) * (xx - xa) >= 0
    return inside


def _captures(kind, n, h, w, seed):
    """N synthetic captures [N,3,H,W] float32 of shifted checkerboards on a lit region, with the projector's backlight, a smooth
    surface colour, inter-reflection and sensor noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'quad':
        lit = _poly_mask(h, w, [(0.2, 0.15), (0.85, 0.25), (0.75, 0.9), (0.1, 0.7)])
        white, bp, noise = 0.5, 0.9, 0.01
    elif kind == 'blobs':
        r = min(h, w)
        lit = ((yy - 0.3 * h) ** 2 + (xx - 0.25 * w) ** 2 < (0.18 * r) ** 2) | ((yy - 0.7 * h) ** 2 + (xx - 0.75 * w) ** 2 < (0.15 * r) ** 2)
        white, bp, noise = 0.5, 0.9, 0.005
    elif kind == 'over':                                      # full-contrast boards: max - min up to 0.8, direct up to 8, clipped
        lit = _poly_mask(h, w, [(0.3, 0.2), (0.9, 0.3), (0.7, 0.8), (0.25, 0.75)])
        white, bp, noise = 0.9, 0.1, 0.01
    elif kind == 'border':                                    # the lit region runs into the left and the bottom edge
        lit = _poly_mask(h, w, [(-0.2, 0.4), (0.6, 0.5), (0.5, 1.3), (-0.3, 1.2)])
        white, bp, noise = 0.6, 0.9, 0.01
    else:
        raise ValueError(kind)
    albedo = syn.scenes(seed, 1, (h, w), box=5, lo=0.4, hi=1.0)[0].numpy()
    cell = max(2, min(h, w) // 12)
    cb = np.empty((n, 3, h, w), dtype=np.float32)
    for k in range(n):
        board = (((yy + k * cell // 2) // cell + (xx + k) // cell) % 2).astype(np.float32)
        light = lit * white * (bp + (1 - bp) * board)           # the projector's black level is bp of its white level
        cb[k] = albedo * (light + 0.03)[None] + rng.normal(0, noise, (3, h, w))
    return np.clip(cb, 0, 1).astype(np.float32)


@pytest.mark.parametrize('n', [2, 5])
@pytest.mark.parametrize('h,w', [(240, 320), (256, 256), (37, 53)])
@pytest.mark.parametrize('kind', ['quad', 'blobs', 'over', 'border'])
def test_kernels_equal_the_oracle(hip, kind, h, w, n):
    """Every stage bitwise: direct / indirect images, grey bytes, smoothed bytes, histogram, threshold, mask, box and count."""
    cb = _captures(kind, n, h, w, seed=h + n)
    direct, indirect = dmo.direct_indirect(cb, 0.9)
    want = dmo.threshold_im(direct)
    if kind == 'over':
        assert direct.max() > 1.5
    if kind == 'border':
        assert want['out'][1] == 0 and want['out'][4] == h - 1
    res = img_proc.direct_mask(torch.from_numpy(cb), 0.9, device=DEV, want_images=True)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert np.array_equal(got['direct'].view(np.uint32), direct.view(np.uint32))
    assert np.array_equal(got['indirect'].view(np.uint32), indirect.view(np.uint32))
    assert np.array_equal(got['gray'], want['gray'])
    assert np.array_equal(got['smooth'], want['smooth'])
    assert np.array_equal(got['hist'].astype(np.int64), want['hist'].astype(np.int64)) and got['hist'].sum() == h * w
    assert got['out'].tolist() == want['out'], (got['out'].tolist(), want['out'])
    assert np.array_equal(got['mask'].astype(bool), want['mask'])
    assert 0 < want['out'][5] < h * w
    # a second run (zeroed histogram, box re-initialised by the launch) gives the same
    again = img_proc.direct_mask(torch.from_numpy(cb), 0.9, device=DEV)
    assert again['out'].tolist() == want['out'] and torch.equal(again['hist'], res['hist'])


def test_threshold_im_image_mask_and_constant(hip):
    """threshold_im on an [H,W,3] image with values below 0 and above 1 (array and tensor), on a bool mask, and on a constant."""
    rng = np.random.default_rng(5)
    h, w = 45, 70
    im = rng.normal(0.05, 0.1, (h, w, 3)).astype(np.float32)
    im[10:30, 20:55] += rng.uniform(0.5, 1.6, (20, 35, 3)).astype(np.float32)
    assert im.min() < -0.05 and im.max() > 1.2
    want = dmo.threshold_im(np.ascontiguousarray(im.transpose(2, 0, 1)))
    for arg in (im, torch.from_numpy(im), torch.from_numpy(im).to(DEV)):
        mask, roi, corners = img_proc.threshold_im(arg, device=DEV)
        assert mask.dtype == np.bool_ and mask.shape == (h, w) and np.array_equal(mask, want['mask'])
        assert corners == want['corners']
        assert roi.dtype == np.bool_ and (roi | mask == roi).all()                  # the hull covers the foreground
    ys, xs = np.nonzero(want['mask'])
    assert not roi[:ys.min()].any() and not roi[:, xs.max() + 1:].any()             # ... and stays inside its box
    # an [H,W] bool mask goes straight to the box
    m = np.zeros((h, w), dtype=bool)
    m[5:9, 60:70] = True
    m[40, 3] = True
    mask, roi, corners = img_proc.threshold_im(torch.from_numpy(m), device=DEV)
    assert np.array_equal(mask, m) and corners == dmo.corners_of((3, 5, 69, 40), h, w)
    with pytest.raises(ValueError, match='fewer than two'):
        img_proc.threshold_im(np.full((16, 16, 3), 0.5, dtype=np.float32), device=DEV)
    with pytest.raises(ValueError, match='no foreground'):
        img_proc.threshold_im(torch.zeros(h, w, dtype=torch.bool), device=DEV)
    with pytest.raises(ValueError):
        img_proc.threshold_im(np.zeros((16, 16), dtype=np.float32), device=DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
SZ = (64, 64)               # camera and projector size of the synthetic setup
N_TRAIN, N_VALID, N_PRJ_TEST, N_CB = 8, 4, 6, 4


@pytest.fixture(scope='module')
def setup_root(hip, tmp_path_factory):
    """<root>/setups/synth rendered by a teacher PCNet (synthetic.pcnet_state_dict): cam/raw/{ref,train,test,cb}; <root>/prj_share/
    {train,test,init}; the label files the attack driver reads."""
    root = tmp_path_factory.mktemp('direct_mask') / 'data'
    setup_path = root / 'setups' / 'synth'
    sd = syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect')
    teacher = hip['models'].PCNet(sd['mask'], hip['models'].WarpingNet(out_size=SZ))
    teacher.load_state_dict(sd)
    teacher = teacher.to(DEV)
    scene = syn.scenes(1, 1, SZ)
    prj_train, prj_test = syn.scenes(20, N_TRAIN, SZ, box=4), syn.scenes(21, N_PRJ_TEST, SZ, box=4)
    yy, xx = np.mgrid[0:SZ[0], 0:SZ[1]]
    boards = torch.from_numpy(np.stack([(((yy + 2 * k) // 8 + (xx + 3 * k) // 8) % 2) for k in range(N_CB)]).astype(np.float32))
    prj_cb = boards[:, None].expand(-1, 3, -1, -1).contiguous()

    def render(prj):
        with torch.no_grad():
            return teacher(prj.to(DEV), scene.to(DEV).expand(prj.shape[0], -1, -1, -1)).clamp(0, 1).cpu()

    io.save_setup_info(str(setup_path), dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=SZ, cam_im_sz=SZ))
    io.save_imgs(torch.cat([render(torch.zeros(1, 3, *SZ)), scene]), str(setup_path / 'cam/raw/ref'))   # img_0002: the scene
    io.save_imgs(render(prj_train), str(setup_path / 'cam/raw/train'))
    io.save_imgs(render(prj_test[:N_VALID]), str(setup_path / 'cam/raw/test'))
    io.save_imgs(render(prj_cb), str(setup_path / 'cam/raw/cb'))
    io.save_imgs(prj_train, str(root / 'prj_share/train'))
    io.save_imgs(prj_test, str(root / 'prj_share/test'))
    io.save_imgs(syn.scenes(22, 1, SZ), str(root / 'prj_share/init'))
    _write_labels(root / 'imagenet1000_clsidx_to_labels.txt', {k: f'class{k}, extra' for k in range(1000)})
    _write_labels(root / 'imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in syn.IMAGENET10_TARGETS})
    return root


def _oracle_mask(root):
    cb = io.torch_imread_mt(str(root / 'setups/synth/cam/raw/cb')).numpy()
    return dmo.threshold_im(dmo.direct_indirect(cb, 0.9)[0])


def test_load_data(setup_root):
    """The reference's 8-tuple: shapes, dtypes, the scene = ref/img_0002, prj_valid cut to len(cam_valid), mask and corners equal to
    the oracle on the checkerboard PNGs."""
    cam_scene, cam_train, cam_valid, prj_train, prj_valid, im_mask, corners, info = tn.load_data(str(setup_root), 'synth', device=DEV)
    assert cam_scene.shape == (1, 3, *SZ) and cam_train.shape == (N_TRAIN, 3, *SZ) and cam_valid.shape == (N_VALID, 3, *SZ)
    assert prj_train.shape == (N_TRAIN, 3, *SZ) and prj_valid.shape == (N_VALID, 3, *SZ)
    assert all(t.dtype == torch.float32 and not t.is_cuda for t in (cam_scene, cam_train, cam_valid, prj_train, prj_valid))
    ref = io.torch_imread_mt(str(setup_root / 'setups/synth/cam/raw/ref'))
    assert torch.equal(cam_scene[0], ref[1])
    assert torch.equal(prj_valid, io.torch_imread_mt(str(setup_root / 'prj_share/test'))[:N_VALID])
    want = _oracle_mask(setup_root)
    assert im_mask.dtype == torch.bool and im_mask.shape == SZ and np.array_equal(im_mask.numpy(), want['mask'])
    assert corners == want['corners'] and len(corners) == 4 and all(-1 <= v <= 1 for pt in corners for v in pt)
    assert 0 < want['out'][5] < SZ[0] * SZ[1]
    assert info.prj_brightness == 0.5 and tuple(info['cam_im_sz']) == SZ
    # the mask is denser inside the teacher's lit rectangle (h/8 .. 7h/8, warped by its small affine) than over the whole view
    assert im_mask[16:48, 16:48].float().mean() > im_mask.float().mean()


def _small_cfg(root, model, **kw):
    cfg = tn.get_model_train_cfg([model], data_root=str(root), setup_list=['synth'], plot_on=False)
    cfg.update(dict(batch_size=4, num_train_list=[N_TRAIN], device=DEV), **kw)
    return cfg


def _check_outputs(root, cfg, ret, infer_dir):
    """What both drivers leave behind: the checkpoint, the log CSV and its columns, the inference PNGs."""
    name = cfg.model_name
    ckpt = root.parent / 'checkpoint' / (io.opt_to_string(cfg) + '.pth')
    assert ckpt.exists() and cfg.setup_name == 'synth' and cfg.num_train == N_TRAIN
    version = f'{name}_l1+ssim_{N_TRAIN}_4_{cfg.max_iters}'
    pngs = sorted(os.listdir(root / 'setups/synth' / infer_dir / version))
    assert pngs == [f'img_{i:04d}.png' for i in range(1, N_VALID + 1)]
    assert list(ret.columns) == tn.LOG_COLUMNS and len(ret) == 2
    assert list(ret.iloc[0, :6]) == ['synth', name, 'l1+ssim', N_TRAIN, 4, cfg.max_iters]
    assert ret.iloc[1, 0] == '[mean]_1_setups' and np.allclose(ret.iloc[1, 6:].astype(float), ret.iloc[0, 6:].astype(float))
    logs = sorted(glob.glob(str(root.parent / 'log' / '*.txt')))
    assert logs
    back = pd.read_csv(logs[-1])
    assert list(back.columns) == tn.LOG_COLUMNS and len(back) == 2
    assert np.allclose(back.iloc[0, 6:].astype(float), ret.iloc[0, 6:].astype(float), atol=5.1e-5)      # '%.4f'
    return ckpt


def _valid_data(root):
    cam_scene, _, cam_valid, _, prj_valid, *_ = tn.load_data(str(root), 'synth', device=DEV)
    return dict(cam_scene=cam_scene.to(DEV).expand(N_VALID, -1, -1, -1), cam_valid=cam_valid.to(DEV), prj_valid=prj_valid.to(DEV))


def _row(ret):
    return np.array(ret.iloc[0, 6:], dtype=np.float64)


def test_train_eval_pcnet(setup_root, monkeypatch):
    """train_eval_pcnet on the synthetic setup, 150 iterations at batch 4: files, log and row; the fresh model's affine; training
    lowers the validation RMSE; load_pretrained reproduces the row without training.

    Measured on an MI355X (validation RMSE, printed before the assertion): same-seed untrained model 0.7449, after training 0.0684.
    The returned row, the row recomputed from the returned model and the load_pretrained row agreed to every printed digit."""
    root = setup_root
    cfg0 = _small_cfg(root, 'PCNet', max_iters=150)
    pcnet, ret, cfg = tn.train_eval_pcnet(cfg0)
    assert pcnet.name == 'PCNet' and cfg.model_name == 'PCNet' and cfg.loss == 'l1+ssim' and 'model_list' not in cfg
    _check_outputs(root, cfg, ret, 'cam/infer/test')
    valid = _valid_data(root)
    infer = tn.evaluate_model(pcnet, valid)[-1]
    again = np.array(M.calc_img_dists(infer, valid['cam_valid']))
    print('row', _row(ret), 'recomputed', again)
    # (the same kernels on the same inputs; the tolerance covers fp32 sums whose order may change between two launches: a few ulp
    # of 6e-8)
    assert np.allclose(_row(ret), again, rtol=1e-6, atol=0)
    # a fresh model: seed 123, the affine solved from the first three mask corners (the output square's corners -> the box)
    want = _oracle_mask(root)
    fresh = tn._build_pcnet('PCNet', torch.from_numpy(want['mask']), want['corners'], SZ, DEV)
    aff = img_proc.get_affine_transform(want['corners'][0:3], [[-1, -1], [1, -1], [1, 1]])
    assert torch.equal(fresh.warping_net.affine_mat.detach().cpu().view(2, 3), torch.from_numpy(aff).float())
    assert not torch.equal(fresh.warping_net.affine_mat.detach().cpu().view(-1), torch.tensor([1., 0, 0, 0, 1, 0]))
    assert torch.equal(fresh.mask.cpu().bool().view(SZ), torch.from_numpy(want['mask']))
    fresh_infer = tn.evaluate_model(fresh, valid)[-1]
    rmse0, rmse1 = M.calc_img_dists(fresh_infer, valid['cam_valid'])[1], again[1]
    print(f'validation RMSE: untrained {rmse0:.4f}, trained {rmse1:.4f}')
    assert rmse1 < rmse0
    # load_pretrained: the checkpoint gives the same row; nothing is trained
    monkeypatch.setattr(tn, 'train_pcnet', lambda *a, **k: pytest.fail('train_pcnet called with load_pretrained'))
    cfg0.load_pretrained = True
    pc2, ret2, _ = tn.train_eval_pcnet(cfg0)
    print('row', _row(ret), 'pretrained', _row(ret2))
    assert np.allclose(_row(ret2), _row(ret), rtol=1e-6, atol=0)
    for (k, a), (_, b) in zip(pcnet.state_dict().items(), pc2.state_dict().items()):
        assert torch.equal(a, b), k


def test_train_eval_pcnet_variant_names(setup_root):
    """The ablation names build their variants and train (3 iterations each); the model column keeps the name as given while the
    folder and checkpoint names replace '/'."""
    cfg0 = _small_cfg(setup_root, 'PCNet', max_iters=3)
    cfg0.model_list = ['PCNet_no_mask_no_rough', 'PCNet_w/o_refine']
    pcnet, ret, cfg = tn.train_eval_pcnet(cfg0)
    assert list(ret['Model']) == cfg0.model_list * 2 and list(ret['Setup'][2:]) == ['[mean]_1_setups'] * 2
    assert pcnet.warping_net.grid_refine_net is None and pcnet.use_mask and pcnet.use_rough and cfg.model_name == 'PCNet_w_o_refine'
    assert (setup_root / 'setups/synth/cam/infer/test/PCNet_w_o_refine_l1+ssim_8_4_3').is_dir()
    assert (setup_root / 'setups/synth/cam/infer/test/PCNet_no_mask_no_rough_l1+ssim_8_4_3').is_dir()
    assert np.isfinite(np.array(ret.iloc[:, 6:], dtype=np.float64)).all()
    with pytest.raises(ValueError, match='unknown model'):
        cfg0.model_list = ['CompenNet++']
        tn.train_eval_pcnet(cfg0)


def test_train_eval_compennet_pp(setup_root, monkeypatch):
    """train_eval_compennet_pp at a small size (CompenNet initialised in 3 iterations, CompenNet++ trained for 5): the same file,
    log and row checks; load_pretrained reproduces the row without training."""
    root = setup_root
    cfg0 = _small_cfg(root, 'CompenNet++', max_iters=5, init_compennet=dict(max_iters=3, batch_size=4, num_train=6))
    with pytest.warns(UserWarning, match='no compensation images'):
        model, ret, cfg = tn.train_eval_compennet_pp(cfg0)
    assert model.name == 'CompenNet++' and cfg.model_name == 'CompenNet++'
    _check_outputs(root, cfg, ret, 'prj/infer/test')
    assert (root.parent / 'checkpoint' / 'init_CompenNet_l1+ssim_6_4_3_0.001_0.2_800_0.0001.pth').exists()
    valid = _valid_data(root)
    infer = tn.evaluate_model(model, valid)[-1]
    again = np.array(M.calc_img_dists(infer, valid['prj_valid']))
    print('row', _row(ret), 'recomputed', again)
    assert np.allclose(_row(ret), again, rtol=1e-6, atol=0)
    want = _oracle_mask(root)
    aff = img_proc.get_affine_transform(want['corners'][0:3], [[-1, -1], [1, -1], [1, 1]])
    fresh = tn._build_compennet_pp('CompenNet++', model.compen_net, want['corners'], SZ, DEV)
    assert torch.equal(fresh.warping_net.affine_mat.detach().cpu().view(2, 3), torch.from_numpy(aff).float())
    monkeypatch.setattr(tn, 'train_compennet_pp', lambda *a, **k: pytest.fail('train_compennet_pp called with load_pretrained'))
    cfg0.load_pretrained = True
    with pytest.warns(UserWarning, match='no compensation images'):
        _, ret2, _ = tn.train_eval_compennet_pp(cfg0)
    assert np.allclose(_row(ret2), _row(ret), rtol=1e-6, atol=0)
    # with desired images present, their compensations are written
    io.save_imgs(syn.scenes(30, 3, SZ), str(root / 'setups/synth/cam/desire/test'))
    tn.train_eval_compennet_pp(cfg0)
    assert len(os.listdir(root / 'setups/synth/prj/cmp/test/CompenNet++_l1+ssim_8_4_5')) == 3


def test_run_projector_based_attack_trains(hip, setup_root):
    """run_projector_based_attack(train=True) without `models`: trains the setup's PCNet through train_eval_pcnet (model_cfg laid over
    the defaults) and writes the attack folders; train=False still raises."""
    A = hip['attack']
    clf = hip['clf'].Classifier('resnet18', DEV, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0), input_sz=(56, 56))
    cfg = A.get_attacker_cfg('SPAA', str(setup_root), ['synth'], plot_on=False)
    cfg.classifier_names, cfg.stealth_losses, cfg.d_threshes = ['resnet18'], ['caml2'], [5, 11]
    with pytest.raises(ValueError, match='not trained here'):
        A.run_projector_based_attack(cfg, classifiers={'resnet18': clf})
    with pytest.raises(ValueError, match='not trained here'):
        A.run_projector_based_attack(cfg, classifiers={'resnet18': clf}, train=False, model_cfg=dict(max_iters=4))
    out = A.run_projector_based_attack(cfg, classifiers={'resnet18': clf}, iters=3, train=True,
                                       model_cfg=dict(max_iters=4, batch_size=4, num_train_list=[N_TRAIN]))
    assert out.model_cfg.max_iters == 4 and out.model_cfg.model_name == 'PCNet' and out.model_cfg.setup_name == 'synth'
    assert (setup_root.parent / 'checkpoint' / (io.opt_to_string(out.model_cfg) + '.pth')).exists()
    cfg_str = A.to_attacker_cfg_str('SPAA')[0]
    names = [f'img_{i:04d}.png' for i in range(1, 12)]
    for kind in ('prj/adv', 'cam/infer/adv'):
        for d_thr in (5, 11):
            leaf = setup_root / 'setups/synth' / kind / cfg_str / 'caml2' / str(d_thr) / 'resnet18'
            assert sorted(os.listdir(leaf)) == names
    assert (setup_root / 'setups/synth/cam/infer/test/PCNet_l1+ssim_8_4_4').is_dir()
