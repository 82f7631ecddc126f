"""CPU: the direct-light mask step -- the three entry points of csrc/direct_mask.hip are exported and declared, the numpy oracle's
known answers (tests/direct_mask_oracle.py), the host helpers of spaa_amd.img_proc, get_model_train_cfg's defaults, and no CPU
fallback in load_data / threshold_im."""
import os
import re

import numpy as np
import pytest
import torch

import direct_mask_oracle as dmo
from spaa_amd import _lib, img_proc
from spaa_amd import train_network as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('spaa_cb_direct_gray', 'spaa_mask_blur_hist', 'spaa_otsu_mask_bbox')


def test_library_exports_the_direct_mask_symbols():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    for n in SYMBOLS:
        assert hasattr(lib, n), f'{n} not exported by libspaa_hip.so'
        assert re.search(r'int\s+' + n + r'\s*\(', hdr), f'{n} not declared in include/spaa_hip.h'
        assert n in _lib._SIGNATURES and n in _lib.EXPORTS


def test_oracle_blur_of_a_constant_is_that_constant():
    assert sum(dmo.WEIGHTS) == 256
    g = np.exp(-np.arange(-1, 2) ** 2 / (2 * 1.5 ** 2))
    assert tuple(np.round(256 * g / g.sum()).astype(int)) == dmo.WEIGHTS
    for v in (0, 1, 37, 128, 254, 255):
        assert (dmo.blur3(np.full((5, 7), v, dtype=np.uint8)) == v).all()
    # BORDER_REFLECT_101 and the single rounding on a hand-computed corner: rows (10 20 / 30 40), reflected 3 x 3 around (0, 0)
    im = np.array([[10, 20], [30, 40]], dtype=np.uint8)
    h = lambda r: 79 * r[1] + 98 * r[0] + 79 * r[1]
    v = 79 * h([30, 40]) + 98 * h([10, 20]) + 79 * h([30, 40])
    assert dmo.blur3(im)[0, 0] == (v + 32768) >> 16


def test_oracle_two_valued_image_thresholds_at_the_upper_value():
    for lo, hi in ((0, 255), (3, 4), (17, 200)):
        im = np.full((9, 11), lo, dtype=np.uint8)
        im[2:6, 3:9] = hi
        hist = dmo.histogram(im)
        assert hist.sum() == im.size and hist[lo] == im.size - 24 and hist[hi] == 24
        t = dmo.otsu_threshold(hist)
        assert t == hi
        mask, out = dmo.mask_bbox(im, t)
        assert (mask == (im == hi)).all() and out == [hi, 3, 2, 8, 5, 24]
    assert dmo.otsu_threshold(dmo.histogram(np.full((4, 4), 9, dtype=np.uint8))) == -1
    # three levels, the middle one nearer the top: the split falls below it
    hist = np.zeros(256, dtype=np.uint32)
    hist[[10, 180, 200]] = (100, 50, 50)
    assert dmo.otsu_threshold(hist) == 180
    hist[[10, 30, 200]] = (100, 50, 50)
    hist[180] = 0
    assert dmo.otsu_threshold(hist) == 200


def test_oracle_corners_of_a_known_rectangle():
    """Box x 4..11, y 2..5 of a 8 x 16 image: (x, y, w, h) = (4, 2, 8, 4); corners 2 x / w - 1, 2 y / h - 1 (img_proc.py:52-63)."""
    want = [[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]]
    assert dmo.corners_of((4, 2, 11, 5), 8, 16) == want
    assert img_proc._corners((4, 2, 11, 5), 8, 16) == want
    d = np.zeros((3, 8, 16), dtype=np.float32)
    d[:, 2:6, 4:12] = 1.0
    r = dmo.threshold_im(d)
    # the blur spreads the rectangle by one pixel at a level above the Otsu split or not: the box is the rectangle or one wider
    assert r['out'][1:5] in ([4, 2, 11, 5], [3, 1, 12, 6]) and r['gray'].max() == 255


def test_oracle_gray_and_separation_are_float32():
    cb = np.zeros((2, 3, 1, 2), dtype=np.float32)
    cb[0, :, 0, 0], cb[1, :, 0, 0] = 0.6, 0.55          # direct 0.5 up to rounding
    cb[0, :, 0, 1], cb[1, :, 0, 1] = 1.0, 0.0           # direct 10: clipped
    d, ind = dmo.direct_indirect(cb, 0.9)
    assert d.dtype == np.float32 and ind.dtype == np.float32
    assert d[0, 0, 0] == (np.float32(0.6) - np.float32(0.55)) / np.float32(0.09999999999999998)
    assert d[0, 0, 1] > 9.9
    g = dmo.gray_u8(d)
    assert g.dtype == np.uint8 and g[0, 1] == 255 and 126 <= g[0, 0] <= 128


def test_get_affine_transform_hand_solved():
    """x' = 2 x + 1, y' = 3 y + 2 through three points; and the identity-corner case of the WarpingNet initialisation."""
    m = img_proc.get_affine_transform([[0, 0], [1, 0], [1, 1]], [[1, 2], [3, 2], [3, 5]])
    assert m.shape == (2, 3) and m.dtype == np.float64
    assert np.allclose(m, [[2, 0, 1], [0, 3, 2]], rtol=0, atol=1e-15)
    # a shear: (0,0)->(0,0), (1,0)->(1,1), (0,1)->(0,1): x' = x, y' = x + y
    assert np.allclose(img_proc.get_affine_transform([[0, 0], [1, 0], [0, 1]], [[0, 0], [1, 1], [0, 1]]), [[1, 0, 0], [1, 1, 0]], atol=1e-15)
    corners = [[-0.5, -0.25], [0.5, -0.25], [0.5, 0.75], [-0.5, 0.75]]
    a = tn._affine_from_corners(corners)
    assert a.dtype == torch.float32 and torch.allclose(a, torch.tensor([2., 0., 0., 0., 2., -0.5]))
    with pytest.raises(np.linalg.LinAlgError):
        img_proc.get_affine_transform([[0, 0], [1, 1], [2, 2]], [[0, 0], [1, 0], [0, 1]])


def test_tensor_helpers():
    x = torch.arange(2 * 3 * 6 * 8, dtype=torch.float32).view(2, 3, 6, 8)
    assert img_proc.expand_4d(x[0, 0, 0]).shape == (1, 1, 1, 8) and img_proc.expand_4d(x) is x
    assert torch.equal(img_proc.center_crop(x, (4, 4)), x[..., 1:5, 2:6])
    assert torch.equal(img_proc.center_crop(x[0, 0] > 5, (2, 6)), (x[0, 0] > 5)[2:4, 1:7])
    for t in (x, x[0], x[0, 0]):
        r = img_proc.resize(t, (3, 4))
        assert r.shape == t.shape[:-2] + (3, 4)
        assert torch.allclose(r, torch.nn.functional.avg_pool2d(img_proc.expand_4d(t), 2).reshape(r.shape))


def test_convex_fill():
    m = np.zeros((8, 10), dtype=bool)
    m[2:5, 3:7] = True
    assert (img_proc._convex_fill(m) == m).all()                        # a rectangle is its own hull
    m[6, 1] = True
    roi = img_proc._convex_fill(m)
    assert (roi | m == roi).all() and roi[5, 2] and roi[5, 3] and not roi[5, 5] and not roi[6, 2]
    line = np.zeros((5, 5), dtype=bool)
    line[1, 1] = line[3, 3] = True
    assert img_proc._convex_fill(line).sum() == 3 and img_proc._convex_fill(line)[2, 2]
    assert not img_proc._convex_fill(np.zeros((4, 4), dtype=bool)).any()


def test_get_model_train_cfg_defaults():
    """train_network.py:444-473."""
    cfg = tn.get_model_train_cfg(['PCNet'], data_root='/d', setup_list=['a', 'b'])
    want = dict(data_root='/d', setup_list=['a', 'b'], device='cuda', device_ids=[0], load_pretrained=False, max_iters=2000,
                batch_size=24, lr=1e-3, lr_drop_ratio=0.2, lr_drop_rate=800, l2_reg=1e-4, train_plot_rate=50, valid_rate=200,
                plot_on=True, center_crop=False, model_list=['PCNet'], num_train_list=[500], loss_list=['l1+ssim'])
    assert dict(cfg) == want and cfg.max_iters == 2000 and cfg['batch_size'] == 24
    single = tn.get_model_train_cfg(['CompenNet++'], single=True, center_crop=True, load_pretrained=True, plot_on=False)
    assert single.model_name == 'CompenNet++' and single.num_train == 500 and single.loss == 'l1+ssim'
    assert 'model_list' not in single and single.center_crop and single.load_pretrained and not single.plot_on
    # the folder name the attack driver derives from the same defaults
    from spaa_amd.projector_based_attack import to_attacker_cfg_str
    assert to_attacker_cfg_str('SPAA')[1] == f'PCNet_{cfg.loss_list[0]}_{cfg.num_train_list[0]}_{cfg.batch_size}_{cfg.max_iters}'


def test_no_cpu_fallback(tmp_path):
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        img_proc.threshold_im(np.zeros((8, 8, 3), dtype=np.float32), device='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        img_proc.threshold_im(torch.zeros(8, 8, dtype=torch.bool), device='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        tn.load_data(str(tmp_path), 'nothing_here', device='cpu')
    with pytest.raises(NotImplementedError):
        img_proc.threshold_im(np.zeros((8, 8, 3), dtype=np.float32), compensation=True)
    with pytest.raises(NotImplementedError):
        tn.load_data(str(tmp_path), 'nothing_here', compensation=True)
