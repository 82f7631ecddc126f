"""GPU: the summary step -- spaa_img_stats (one launch over many cropped image pairs) against the float64 oracle, and the reference's
summary drivers (summarize_single_attacker / summarize_all_attackers) against a restatement of the reference's per-configuration
loop (projector_based_attack.py:417-614) on a synthetic setup."""
import itertools
import os
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

import spaa_oracle as so
from spaa_amd import synthetic as syn
from spaa_amd import io
from spaa_amd import metrics as M
from test_gpu_parity import hip  # noqa: F401  (hip: module fixture)
from test_sweep_gpu import _write_labels

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _framed(shape, y0, x0, h, w, seed):
    """A random image whose pixels just outside the crop rectangle alternate 0 / 1 (so a window that reads past the crop shows)."""
    g = torch.Generator().manual_seed(seed)
    im = torch.rand(3, *shape, generator=g)
    fill = (torch.arange(shape[0])[:, None] + torch.arange(shape[1])[None, :]) % 2
    out = torch.ones(shape, dtype=torch.bool)
    out[y0:y0 + h, x0:x0 + w] = False
    im[:, out] = fill[out].float()
    return im


def _crop(im, y0, x0, h, w):
    return im[..., y0:y0 + h, x0:x0 + w]


def test_img_stats_against_oracle(hip):
    """Ragged crops at arbitrary origins, a single 16 x 16 tile, 240 x 240 crops of differently sized images, a constant colour:
    per pair and per group against spaa_oracle.calc_img_dists of the explicitly cropped tensors; repeated calls bit-identical."""
    # (x shape, x origin, y shape or rgb, y origin, crop)
    cases = [((45, 60), (3, 4), (50, 58), (5, 2), (37, 53)),
             ((45, 60), (6, 1), (50, 58), (2, 5), (37, 53)),
             ((16, 16), (0, 0), (20, 20), (2, 2), (16, 16)),
             ((240, 320), (0, 40), (256, 256), (8, 8), (240, 240)),
             ((40, 50), (2, 1), (0.5, 0.3, 0.7), None, (33, 47))]
    xs, ys, pairs, want = [], [], [], []
    xoff = yoff = 0
    for k, (xsh, (xy0, xx0), ysh, yorg, (h, w)) in enumerate(cases):
        x = _framed(xsh, xy0, xx0, h, w, 2 * k)
        xc = _crop(x, xy0, xx0, h, w)
        if yorg is None:
            yc = torch.tensor(ysh).view(3, 1, 1).expand(3, h, w)
            pairs.append(M.Pair(xoff, *xsh, xy0, xx0, None, 0, 0, 0, 0, h, w, ysh))
        else:
            y = _framed(ysh, *yorg, h, w, 2 * k + 1)
            y[:, yorg[0]:yorg[0] + h, yorg[1]:yorg[1] + w] = (xc + 0.1 * torch.randn(3, h, w, generator=torch.Generator().manual_seed(k))).clamp(0, 1)
            yc = _crop(y, *yorg, h, w)
            pairs.append(M.Pair(xoff, *xsh, xy0, xx0, yoff, *ysh, *yorg, h, w, None))
            ys.append(y.reshape(-1))
            yoff += y.numel()
        xs.append(x.reshape(-1))
        xoff += x.numel()
        want.append((xc.contiguous(), yc.contiguous()))
    x, y = torch.cat(xs).to(DEV), torch.cat(ys).to(DEV)
    sums, npix = M.img_stats(x, y, pairs)
    assert sums.shape == (len(cases), 5) and npix.tolist() == [h * w for *_, (h, w) in cases]
    for k, (xc, yc) in enumerate(want):
        ref = np.array(so.calc_img_dists(xc, yc))
        got = np.array(M.dists_from_sums(sums, npix, [k]))
        assert np.abs(got / ref - 1).max() < 2e-5, (k, got, ref)
    ref = np.array(so.calc_img_dists(torch.stack([want[0][0], want[1][0]]), torch.stack([want[0][1], want[1][1]])))
    got = np.array(M.dists_from_sums(sums, npix, [0, 1]))
    assert np.abs(got / ref - 1).max() < 2e-5, (got, ref)
    again, _ = M.img_stats(x, y, pairs)
    assert np.array_equal(sums, again)
    # calc_img_dists is the group "the whole batch" of one img_stats call
    assert M.calc_img_dists(want[0][0], want[0][1]) == M.dists_from_sums(sums, npix, [0])

    bad = pairs[0]._replace(xy0=9)                                     # 9 + 37 > 45
    with pytest.raises(ValueError, match='outside'):
        M.img_stats(x, y, [bad])
    with pytest.raises(ValueError, match='overruns'):
        M.img_stats(x, y, [pairs[0]._replace(y_off=y.numel() - 10)])
    with pytest.raises(ValueError, match='32-bit'):
        M.img_stats(x, y, [pairs[0]._replace(xH=30000, xW=30000)])


def _cc(x, size):
    """img_proc.py:126-132 (center_crop)."""
    h, w = x.shape[-2:]
    th, tw = size
    i, j = int(round((h - th) / 2.)), int(round((w - tw) / 2.))
    return x[..., i:i + th, j:j + tw]


def _reference_rows(setup_path, setup_name, classifiers, cfg_str, model_cfg_str, target_idx):
    """projector_based_attack.py:448-541 restated: per configuration, the classifier on the scene / inferred / captured images and one
    calc_img_dists per group (only the skip differs: one configuration, not the classifier loop)."""
    from os.path import join
    setup_info = io.load_setup_info(setup_path)
    cp_sz = tuple(setup_info['classifier_crop_sz'])
    n = 10
    im_gray = setup_info['prj_brightness'] * torch.ones(1, 3, *setup_info['prj_im_sz']).to(DEV)
    cam_scene = io.torch_imread(join(setup_path, 'cam/raw/ref/img_0002.png')).to(DEV)
    im_infer = _cc(io.torch_imread_mt(join(setup_path, 'cam/infer/test', model_cfg_str)), cp_sz).to(DEV)
    im_gt = _cc(io.torch_imread_mt(join(setup_path, 'cam/raw/test')), cp_sz).to(DEV)
    valid_ret = M.calc_img_dists(im_infer, im_gt)
    rows = []
    for loss, d_thr, cname in itertools.product(['caml2', 'camdE', 'camdE_caml2', '-'], [5, 7, 9, 11, '-'],
                                                ['inception_v3', 'resnet18', 'vgg16']):
        folder = join(cfg_str, loss, str(d_thr), cname)
        paths = [join(setup_path, k, folder) for k in ('prj/adv', 'cam/raw/adv', 'cam/infer/adv')]
        if not all(os.path.exists(p) and os.listdir(p) for p in paths):
            continue
        prj_adv, cam_real, cam_infer = (io.torch_imread_mt(p).to(DEV) for p in paths)
        clf = classifiers[cname]
        ret = {k: clf(v, cp_sz) for k, v in (('scene', cam_scene), ('infer', cam_infer), ('real', cam_real))}
        t1_infer = np.count_nonzero(ret['infer'][2][:n, 0] == target_idx) / n
        t5_infer = np.count_nonzero([target_idx[i] in ret['infer'][2][i, :5] for i in range(n)]) / n
        t1_real = np.count_nonzero(ret['real'][2][:n, 0] == target_idx) / n
        t5_real = np.count_nonzero([target_idx[i] in ret['real'][2][i, :5] for i in range(n)]) / n
        true_idx = ret['scene'][2][0, 0]
        u_infer = np.count_nonzero(ret['infer'][2][n, 0] != true_idx)
        u_real = np.count_nonzero(ret['real'][2][n, 0] != true_idx)
        cs = _cc(cam_scene, cp_sz)
        groups = []
        for sel in (slice(0, n), slice(n, n + 1), slice(None)):
            groups += [M.calc_img_dists(prj_adv[sel], im_gray.expand_as(prj_adv[sel])),
                       M.calc_img_dists(_cc(cam_infer[sel], cp_sz), cs.expand_as(_cc(cam_infer[sel], cp_sz))),
                       M.calc_img_dists(_cc(cam_real[sel], cp_sz), cs.expand_as(_cc(cam_real[sel], cp_sz)))]
        rows.append([setup_name, cfg_str, loss, d_thr, cname, t1_infer, t5_infer, t1_real, t5_real, u_infer, u_real, *valid_ret,
                     *itertools.chain.from_iterable(groups)])
    return rows


def _assert_rows(table, rows):
    from spaa_amd.projector_based_attack import SUMMARY_COLUMNS
    assert list(table.columns) == SUMMARY_COLUMNS and len(table) == len(rows)
    for r, (_, got) in zip(rows, table.iterrows()):
        got = list(got)
        assert got[:5] == r[:5]
        assert got[5:11] == r[5:11], (r[:5], got[5:11], r[5:11])             # success rates: exactly
        g, w = np.array(got[11:], dtype=np.float64), np.array(r[11:], dtype=np.float64)
        assert np.allclose(g, w, rtol=1e-5, atol=0), (r[:5], g, w)   # (equal infinities agree: an inference can equal the scene)


def test_summarize_single_and_all_attackers(hip, tmp_path, capsys):
    """A 64 x 64 setup attacked by run_projector_based_attack (resnet18 and vgg16, two losses x two d_thr), captured images written
    as perturbed copies of the inferences: the summary equals the restated reference loop row for row; stats.txt parses; a removed
    configuration drops exactly its row; a missing classifier raises; summarize_all_attackers is the pandas pivot of the rows."""
    A = hip['attack']
    sz, raw_sz = (64, 64), (72, 80)
    sd = syn.pcnet_state_dict(0, cam_sz=sz, mask='rect')
    pc = hip['models'].PCNet(sd['mask'], hip['models'].WarpingNet(out_size=sz))
    pc.load_state_dict(sd)
    pc = pc.to(DEV)
    Clf = hip['clf'].Classifier
    classifiers = {'resnet18': Clf('resnet18', DEV, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0), input_sz=(56, 56)),
                   'vgg16': Clf('vgg16', DEV, state_dict=syn.vgg16_state_dict(3, logit_gain=5.0, fc_width=256), input_sz=(64, 64))}
    root = tmp_path / 'data'
    setup_path = root / 'setups' / 'synth'
    io.save_setup_info(str(setup_path), dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=sz, cam_im_sz=sz))
    io.save_imgs(syn.scenes(1, 2, raw_sz), str(setup_path / 'cam/raw/ref'))        # raw camera size: the summary crops it itself
    _write_labels(root / 'imagenet1000_clsidx_to_labels.txt', {k: f'class{k}, extra' for k in range(1000)})
    ten = [1, 7, 21, 207, 340, 745, 779, 846, 947, 950]
    _write_labels(root / 'imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in ten})
    cfg = A.get_attacker_cfg('SPAA', str(root), ['synth'])
    cfg.classifier_names, cfg.stealth_losses, cfg.d_threshes = ['resnet18', 'vgg16'], ['caml2', 'camdE_caml2'], [5, 11]
    A.run_projector_based_attack(cfg, models={'synth': pc}, classifiers=classifiers)
    cfg_str, model_cfg_str = A.to_attacker_cfg_str('SPAA')
    g = torch.Generator().manual_seed(7)
    for dp, _, fn in os.walk(setup_path / 'cam/infer/adv'):
        if fn:
            ims = io.torch_imread_mt(dp)
            io.save_imgs((ims + 0.06 * torch.randn(ims.shape, generator=g)).clamp(0, 1),
                         dp.replace(os.path.join('cam', 'infer', 'adv'), os.path.join('cam', 'raw', 'adv')))
    io.save_imgs(torch.rand(3, 3, *raw_sz, generator=g), str(setup_path / 'cam/raw/test'))
    io.save_imgs(torch.rand(3, 3, *sz, generator=g), str(setup_path / 'cam/infer/test' / model_cfg_str))

    table = A.summarize_single_attacker('SPAA', str(root), ['synth'], classifiers=classifiers)
    rows = _reference_rows(str(setup_path), 'synth', classifiers, cfg_str, model_cfg_str, ten)
    assert len(rows) == 8
    _assert_rows(table, rows)
    assert not np.allclose(table['T.infer_L2'], table['T.real_L2'])                  # the captured columns are their own
    assert all(isinstance(v, (int, np.integer)) for v in table['U.top-1_real'])
    stats = setup_path / 'ret' / cfg_str / 'stats.txt'
    back = pd.read_csv(stats, index_col=None, header=0, sep='\t')
    assert list(back.columns) == list(table.columns) and len(back) == 8
    assert np.allclose(back['All.real_dE'], table['All.real_dE'], atol=5e-5)
    assert 'results on [synth]' in capsys.readouterr().out

    # one configuration without captured images: exactly its row goes
    shutil.rmtree(setup_path / 'cam/raw/adv' / cfg_str / 'camdE_caml2' / '5' / 'vgg16')
    t2 = A.summarize_single_attacker('SPAA', str(root), ['synth'], classifiers=classifiers)
    keep = [k for k, r in enumerate(rows) if r[2:5] != ['camdE_caml2', 5, 'vgg16']]
    assert len(keep) == 7
    assert t2.reset_index(drop=True).equals(table.iloc[keep].reset_index(drop=True))
    with pytest.raises(ValueError, match='vgg16'):
        A.summarize_single_attacker('SPAA', str(root), ['synth'], classifiers={'resnet18': classifiers['resnet18']})

    # no validation inferences: NaN columns, the rest unchanged
    shutil.rmtree(setup_path / 'cam/infer/test')
    t3 = A.summarize_single_attacker('SPAA', str(root), ['synth'], classifiers=classifiers)
    valid = [c for c in t3.columns if c.startswith('Valid_')]
    assert t3[valid].isna().all().all()
    assert t3.drop(columns=valid).equals(t2.drop(columns=valid))

    allt, pivot = A.summarize_all_attackers(['SPAA'], str(root), ['synth'])
    want = pd.read_csv(setup_path / 'ret' / cfg_str / 'stats.txt', index_col=None, header=0, sep='\t')
    assert allt.equals(want) and len(allt) == 7
    ref = pd.pivot_table(want, values=['T.top-1_real', 'T.top-5_real', 'U.top-1_real', 'T.real_L2', 'T.real_Linf', 'T.real_dE',
                                       'T.real_SSIM', 'All.real_L2', 'All.real_Linf', 'All.real_dE', 'All.real_SSIM'],
                         index=['Attacker', 'd_thr', 'Stealth_loss', 'Classifier'], aggfunc='mean', sort=False)
    ref = ref.sort_index(level=[0, 1], ascending=[False, True])
    pd.testing.assert_frame_equal(pivot, ref)
    assert (root / 'setups' / 'stats_all.txt').exists() and (root / 'setups' / 'pivot_table_all.txt').exists()
    back = pd.read_csv(root / 'setups' / 'pivot_table_all.txt', sep='\t')
    assert len(back) == 7 and 'T.real_dE' in back.columns
