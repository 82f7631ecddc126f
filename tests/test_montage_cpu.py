"""CPU: the host side of the result montages (spaa_amd/montage.py: font, JET, layout_labels) and the real-capture step
project_capture_real_attack with a fake capture; the GPU entry points refuse CPU tensors (no fallback)."""
import os

import numpy as np
import pytest
import torch

from spaa_amd import io
from spaa_amd import montage as mt
from spaa_amd import projector_based_attack as A
from spaa_amd import synthetic as syn


def test_font_table():
    assert mt.FONT.shape == (95, mt.FONT_H) and mt.FONT.dtype == np.uint8 and 2 * mt.FONT_H <= mt.BAND
    assert (mt.FONT < (1 << mt.FONT_W)).all()                      # every glyph inside its cell
    assert not mt.FONT[0].any()                                    # space
    assert all(mt.FONT[g].any() for g in range(1, 95))
    assert len({mt.FONT[g].tobytes() for g in range(95)}) == 95     # pairwise distinct
    assert sorted(mt._GLYPHS) == [chr(c) for c in range(32, 127)]


def test_jet_table():
    j = mt.JET
    assert j.shape == (256, 3) and j.dtype == np.uint8
    assert tuple(j[0]) == (0, 0, 128) and tuple(j[255]) == (128, 0, 0)
    assert j[:, 1].max() == 255 and 96 <= int(np.argmax(j[:, 1])) <= 160 and j[0, 1] == 0 and j[255, 1] == 0
    for c in range(3):                                             # piecewise monotone: up, then down
        d = np.sign(np.diff(j[:, c].astype(int)))
        d = d[d != 0]
        assert (np.diff(d) != 0).sum() <= 1 and (len(d) == 0 or d[0] >= d[-1])


TEXTS = [('Cam-captured scene (3)', 'tabby (0.50)'), ('Model inferred adversarial projection', '\tL2=1.23'),
         ('Model inferred cam-captured projection', 'a class label that is far longer than any tile is wide, even the 256-pixel one (0.25)'
                                                    '\tL2=5.00'),
         ('Real cam-captured projection', 'y (0.75)\tL2=6.79'), ('Normalized difference, i.e., 4th-1st', '')]


@pytest.mark.parametrize('Wp', [16, 28, 70, 256])
def test_layout_labels_stays_inside_tiles(Wp):
    recs = mt.layout_labels(TEXTS, Wp)
    assert recs
    for x, y, g in recs:
        k = (x - 5) // (Wp + 5)
        assert 0 <= k < 5 and 5 + k * (Wp + 5) <= x and x + mt.FONT_W <= 5 + k * (Wp + 5) + Wp
        assert y in (0, mt.FONT_H) and y + mt.FONT_H <= mt.BAND and 0 <= g < 95


def test_layout_labels_alignment_and_truncation():
    Wp = 256
    recs = mt.layout_labels(TEXTS, Wp)
    x0, x1 = mt.tile_x(2, Wp), mt.tile_x(2, Wp) + Wp
    line2 = sorted((x, g) for x, y, g in recs if y == mt.FONT_H and x0 <= x < x1)
    s = ''.join(chr(g + 32) for _, g in line2)
    assert s.endswith('L2=5.00') and line2[-1][0] + mt.FONT_W == x1            # right-aligned to the tile's edge
    xr = x1 - 7 * mt.FONT_W
    left = [(x, g) for x, g in line2 if x < xr]
    assert left[0][0] == x0 and left[-1][0] + mt.FONT_W <= xr - mt.FONT_W      # truncated before the L2 string
    assert ''.join(chr(g + 32) for _, g in left) == TEXTS[2][1][:len(left)] and len(left) < len(TEXTS[2][1]) - 8
    # line 1 left-aligned at the tile's edge; a non-ASCII character is '?'
    recs = mt.layout_labels([('hé中\n', '')] + TEXTS[1:], 64)
    assert [(x, y, g) for x, y, g in recs if y == 0 and x < 5 + 64] == [(5, 0, ord('h') - 32)] + \
        [(5 + mt.FONT_W * i, 0, ord('?') - 32) for i in (1, 2, 3)]
    assert mt.layout_labels(mt.attack_texts(0, ('a', .5), ('b', .25), ('c', 1.0), (1, 2, 3.456)), 256)
    with pytest.raises(ValueError):
        mt.layout_labels(TEXTS[:4], 64)


def test_no_cpu_fallback():
    n, sz = 2, (16, 16)
    x = torch.rand(n, 3, *sz)
    texts = [TEXTS] * n
    with pytest.raises(RuntimeError, match='GPU only'):
        mt.attack_montages(x[0], x, x, x, (12, 12), texts)
    with pytest.raises(RuntimeError, match='GPU only'):
        mt.diff_range(x[0], x, (12, 12), sz)
    ret = {k: (None, np.ones((n, 5), dtype=np.float32), np.zeros((n, 5), dtype=np.int64)) for k in ('scene', 'infer', 'real')}
    with pytest.raises(RuntimeError, match='GPU only'):
        A.attack_results(ret, 0, {0: 'a'}, torch.full((1, 3, *sz), 0.5), x, x[0], x, x, sz, (12, 12))


def _setup(tmp_path, names=('a',)):
    root = tmp_path / 'data'
    for name in names:
        io.save_setup_info(str(root / 'setups' / name), dict(classifier_crop_sz=(20, 20), prj_brightness=0.5, prj_im_sz=(16, 12),
                                                              cam_im_sz=(24, 24)))
    return root


def test_project_capture_real_attack(tmp_path):
    root = _setup(tmp_path, ('a', 'b'))
    cfg = A.get_attacker_cfg('SPAA', str(root), ['a'])
    cfg.classifier_names, cfg.stealth_losses, cfg.d_threshes = ['resnet18', 'vgg16'], ['caml2'], [5, 11]
    cfg_str = A.to_attacker_cfg_str('SPAA')[0]
    g = torch.Generator().manual_seed(0)
    prj = {}
    for d_thr in (5, 11):
        for c in cfg.classifier_names:
            prj[d_thr, c] = torch.randint(0, 256, (3, 3, 12, 16), generator=g).float() / 255
            io.save_imgs(prj[d_thr, c], str(root / 'setups/a/prj/adv' / cfg_str / 'caml2' / str(d_thr) / c))
    seen = []

    def capture(setup_info):
        assert tuple(setup_info['cam_im_sz']) == (24, 24)

        def cap(im_prj):
            seen.append(im_prj.clone())
            assert im_prj.dtype == torch.uint8 and tuple(im_prj.shape) == (3, 12, 16)
            v = im_prj.float().mean() / 255
            return torch.stack([torch.full((24, 24), float(v)), torch.full((24, 24), 0.999), torch.linspace(0, 1, 24 * 24).view(24, 24)])
        return cap

    assert A.project_capture_real_attack(cfg, capture=capture) is cfg
    assert len(seen) == 12
    k = 0
    for d_thr in (5, 11):
        for c in cfg.classifier_names:
            src = root / 'setups/a/prj/adv' / cfg_str / 'caml2' / str(d_thr) / c
            dst = root / 'setups/a/cam/raw/adv' / cfg_str / 'caml2' / str(d_thr) / c
            assert sorted(os.listdir(dst)) == sorted(os.listdir(src)) == ['img_0001.png', 'img_0002.png', 'img_0003.png']
            got = io.torch_imread_mt(str(dst))
            for i in range(3):
                u8 = np.uint8(prj[d_thr, c][i].numpy() * 255)
                assert np.array_equal(seen[k].numpy(), u8)
                want = capture(io.load_setup_info(str(root / 'setups/a')))(torch.from_numpy(u8)).numpy()
                assert np.array_equal(np.uint8(got[i].numpy() * 255), np.floor(want * np.float32(255)).astype(np.uint8))
                k += 1
    assert len(seen) == 24 and got[0, 1, 0, 0] * 255 == 254          # 0.999 is written as floor(254.745)

    with pytest.raises(ValueError, match='exactly one setup'):
        A.project_capture_real_attack(A.get_attacker_cfg('SPAA', str(root), ['a', 'b']), capture=capture)
    with pytest.raises(ValueError, match='One-pixel_DE'):
        A.project_capture_real_attack(A.get_attacker_cfg('One-pixel_DE', str(root), ['a']), capture=capture)
    cfg.d_threshes = [5, 7]
    with pytest.raises(ValueError, match=os.path.join('caml2', '7', 'resnet18')):
        A.project_capture_real_attack(cfg, capture=capture)
    with pytest.raises(ValueError, match='capture must be'):
        A.project_capture_real_attack(cfg, capture=None)
    cfg.d_threshes = [5]
    with pytest.raises(ValueError, match='trained PCNet'):
        A.project_capture_real_attack(cfg, capture='model', models={})
