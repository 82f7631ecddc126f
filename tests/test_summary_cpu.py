"""CPU: the host side of the attack summary (projector_based_attack.py:417-614) -- grouping per-pair image sums into calc_img_dists
values (metrics.dists_from_sums), the success rates, the reference's column list and the stats.txt format."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

import spaa_oracle as so
from spaa_amd import metrics as M
from spaa_amd import projector_based_attack as A


def _sums_of(x, y):
    """Per-image sums recovered from the oracle's calc_img_dists of that image alone (the inverse of dists_from_sums)."""
    psnr, _, ssim, l2, linf, de = so.calc_img_dists(x, y)
    n = x.shape[-2] * x.shape[-1]
    mse = 10 ** (-psnr / 10)
    return [mse * 3 * n, ssim * 3 * n, l2 / 255 * n, linf / 255 * n, de * n], n


def _group(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    xs, ys = [], []
    for h, w in shapes:
        x = torch.rand(1, 3, h, w, generator=g)
        xs.append(x)
        ys.append((x + 0.08 * torch.randn(1, 3, h, w, generator=g)).clamp(0, 1))
    return xs, ys


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def test_dists_from_sums_equals_group_oracle():
    """T (10) / U (1) / All (11) groups of 40 x 50 images: the combined per-image sums equal the oracle on the whole group."""
    xs, ys = _group([(40, 50)] * 11, 0)
    per = [_sums_of(x, y) for x, y in zip(xs, ys)]
    sums, npix = np.array([p[0] for p in per]), np.array([p[1] for p in per])
    for sel in (slice(0, 10), slice(10, 11), slice(None)):
        want = so.calc_img_dists(torch.cat(xs[sel]), torch.cat(ys[sel]))
        got = M.dists_from_sums(sums, npix, np.arange(11)[sel])
        assert _rel(got, want) < 1e-6, (sel, got, want)
    assert M.dists_from_sums(sums, npix) == M.dists_from_sums(sums, npix, list(range(11)))


def test_dists_from_sums_unequal_sizes():
    """Images of different sizes weigh by their pixel counts: the group equals the oracle's per-pixel means over all of them."""
    shapes = [(40, 50), (17, 23), (64, 31)]
    xs, ys = _group(shapes, 1)
    per = [_sums_of(x, y) for x, y in zip(xs, ys)]
    sums, npix = np.array([p[0] for p in per]), np.array([p[1] for p in per])
    got = M.dists_from_sums(sums, npix)
    # the oracle on the pixels of all images at once: flatten each image to one row of a [1,3,1,N] "image" for the per-pixel
    # terms, and the pixel-weighted mean of the per-image SSIM values (SSIM windows do not cross images)
    fx = torch.cat([x.reshape(1, 3, 1, -1) for x in xs], -1)
    fy = torch.cat([y.reshape(1, 3, 1, -1) for y in ys], -1)
    d = fx - fy
    n = fx.shape[-1]
    mse = float((d.double() ** 2).mean())
    ssim = sum(so.calc_img_dists(x, y)[2] * x.shape[-2] * x.shape[-1] for x, y in zip(xs, ys)) / n
    de = so.calc_img_dists(fx, fy)[5]
    want = (10 * math.log10(1 / mse), math.sqrt(mse * 3), ssim, float(d.double().norm(dim=1).mean()) * 255,
            float(d.double().abs().amax(dim=1).mean()) * 255, de)
    assert _rel(got, want) < 1e-6, (got, want)


def test_dists_from_sums_edges():
    assert M.dists_from_sums([[0.0, 3.0, 0.0, 0.0, 0.0]], [1])[0] == math.inf   # identical images: PSNR inf, as the reference's
    with pytest.raises(ValueError):
        M.dists_from_sums(np.zeros((2, 5)), [4, 4], [])


def test_attack_success():
    target = [5, 6, 7, 8]
    scene = np.array([[3, 1, 2, 4, 0]])
    infer = np.array([[5, 0, 1, 2, 3],      # top-1 hit
                      [0, 1, 2, 3, 6],      # top-5 hit, not top-1
                      [7, 0, 1, 2, 3],      # wrong target in top-1, right one not in top-5
                      [0, 1, 2, 3, 4],      # miss
                      [3, 9, 9, 9, 9]])     # untargeted: still the scene's class -> failure
    real = np.array([[5, 0, 1, 2, 3], [6, 0, 1, 2, 3], [7, 0, 1, 2, 3], [1, 2, 3, 4, 8], [4, 3, 0, 0, 0]])
    infer[2, 0] = 9
    got = A.attack_success(infer, real, scene, target)
    assert got == (0.25, 0.5, 0.75, 1.0, 0, 1)
    assert all(isinstance(v, int) for v in got[4:])


REFERENCE_COLUMNS = [
    'Setup', 'Attacker', 'Stealth_loss', 'd_thr', 'Classifier', 'T.top-1_infer', 'T.top-5_infer', 'T.top-1_real', 'T.top-5_real',
    'U.top-1_infer', 'U.top-1_real', 'Valid_PSNR', 'Valid_RMSE', 'Valid_SSIM', 'Valid_L2', 'Valid_Linf', 'Valid_dE',
    'T.prj_PSNR', 'T.prj_RMSE', 'T.prj_SSIM', 'T.prj_L2', 'T.prj_Linf', 'T.prj_dE',
    'T.infer_PSNR', 'T.infer_RMSE', 'T.infer_SSIM', 'T.infer_L2', 'T.infer_Linf', 'T.infer_dE',
    'T.real_PSNR', 'T.real_RMSE', 'T.real_SSIM', 'T.real_L2', 'T.real_Linf', 'T.real_dE',
    'U.prj_PSNR', 'U.prj_RMSE', 'U.prj_SSIM', 'U.prj_L2', 'U.prj_Linf', 'U.prj_dE',
    'U.infer_PSNR', 'U.infer_RMSE', 'U.infer_SSIM', 'U.infer_L2', 'U.infer_Linf', 'U.infer_dE',
    'U.real_PSNR', 'U.real_RMSE', 'U.real_SSIM', 'U.real_L2', 'U.real_Linf', 'U.real_dE',
    'All.prj_PSNR', 'All.prj_RMSE', 'All.prj_SSIM', 'All.prj_L2', 'All.prj_Linf', 'All.prj_dE',
    'All.infer_PSNR', 'All.infer_RMSE', 'All.infer_SSIM', 'All.infer_L2', 'All.infer_Linf', 'All.infer_dE',
    'All.real_PSNR', 'All.real_RMSE', 'All.real_SSIM', 'All.real_L2', 'All.real_Linf', 'All.real_dE']


def test_columns_and_stats_file(tmp_path):
    assert A.SUMMARY_COLUMNS == REFERENCE_COLUMNS
    rng = np.random.default_rng(0)
    rows = [['synth', 'SPAA_PCNet_l1+ssim_500_24_2000', loss, d, 'resnet18', 0.3, 0.7, 0.2, 0.6, 1, 0] +
            list(rng.random(60) * 30) for loss, d in (('caml2', 5), ('camdE', 11))]
    table = pd.DataFrame(rows, columns=A.SUMMARY_COLUMNS)
    fn = tmp_path / 'stats.txt'
    A.write_stats(table, str(fn))
    back = pd.read_csv(fn, index_col=None, header=0, sep='\t')
    assert list(back.columns) == REFERENCE_COLUMNS
    assert back['d_thr'].tolist() == [5, 11] and back['U.top-1_infer'].tolist() == [1, 1]
    assert np.allclose(back[REFERENCE_COLUMNS[17:]].to_numpy(), table[REFERENCE_COLUMNS[17:]].to_numpy().astype(float), atol=5e-5)
    line = fn.read_text().splitlines()[1].split('\t')
    assert line[5] == '0.3000' and line[9] == '1' and all(len(v.split('.')[1]) == 4 for v in line[11:])
