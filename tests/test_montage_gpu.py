"""GPU: the result montages (csrc/montage.hip through the C-ABI and through spaa_amd.montage.attack_montages) against the reference's
composition restated on the CPU (tests/montage_oracle.py).  Every step of the specification is one correctly rounded fp32 operation
and the result is bytes, so the comparison is exact: no tolerance anywhere in this file."""
import os

import numpy as np
import pytest
import torch

import montage_oracle as mo
from spaa_amd import io
from spaa_amd import metrics as M
from spaa_amd import montage as mt
from spaa_amd import synthetic as syn
from test_gpu_parity import hip  # noqa: F401  (hip: module fixture)
from test_sweep_gpu import _write_labels

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (Hc, Wc), cp_sz, (Hp, Wp), N: the smallest geometries that reach each branch
GEOMETRIES = {
    'up': ((24, 36), (22, 30), (28, 40), 11),          # up-sampling, non-integer ratio, non-square
    'down': ((40, 52), (36, 48), (20, 28), 11),        # down-sampling: windows of 1-2 and of 2-3
    'identity': ((24, 24), (20, 20), (20, 20), 1),     # identity resize, one item
    'wide': ((24, 80), (24, 72), (24, 70), 3),         # a tile wider than one 64-lane row; crop only in x
    'many': ((66, 66), (64, 64), (64, 64), 64),        # many items: per-item min / max must not leak
}
ALL95 = ''.join(chr(c) for c in range(32, 127))


def _u8_images(g, *shape):
    return torch.randint(0, 256, shape, generator=g).float() / 255


def _texts(n, wp):
    """Item 0 holds all 95 characters and a class label longer than any tile; the others the reference's strings."""
    out = [mt.attack_texts(t, (f'class{t}, extra', 0.125 * (t % 8)), (f'label{t}', 0.5), ('r', 1.0), (t + 0.5, 2.25, 31.0)) for t in range(n)]
    out[0] = [(ALL95[:24], ALL95[24:48] + ' (0.93)'), (ALL95[48:72], '\tL2=0.12'),
              (ALL95[72:], 'a class label that is much longer than the widest tile of these tests is (0.50)\tL2=9.87'),
              ('Real cam-captured projection é', 'x (1.00)\tL2=10.00'), ('Normalized difference, i.e., 4th-1st', '')]
    return out


_CASES = {}


def case(name):
    """Inputs, the helper's montages and its per-item (min, max), computed once per geometry."""
    if name not in _CASES:
        (hc, wc), cp, (hp, wp), n = GEOMETRIES[name]
        g = torch.Generator().manual_seed(sorted(GEOMETRIES).index(name))
        scene, prj = _u8_images(g, 3, hc, wc), _u8_images(g, n, 3, hp, wp)
        infer, real = _u8_images(g, n, 3, hc, wc), _u8_images(g, n, 3, hc, wc)
        if name == 'many':
            real[5] = scene                                    # a capture equal to the scene: the constant-difference branch
            real[6] = torch.floor((scene * 0.5 + 0.25) * 255) / 255   # a low-contrast item between full-range ones
        texts = _texts(n, wp)
        want = np.stack([mo.montage(scene, prj[i], infer[i], real[i], cp, texts[i]) for i in range(n)])
        rng = np.array([[float(v) for v in mo.diff(scene, real[i], cp, (hp, wp))[1:]] for i in range(n)], dtype=np.float32)
        _CASES[name] = dict(scene=scene, prj=prj, infer=infer, real=real, cp=cp, texts=texts, want=want, rng=rng, tile=(hp, wp), n=n)
    return _CASES[name]


def _show(got, want):
    bad = np.argwhere(got != want)
    return f'{len(bad)} bytes differ, first at (item, channel, y, x) = {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}'


@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_montage_bytes_equal_the_reference_composition(hip, name):
    c = case(name)
    got = mt.attack_montages(c['scene'].to(DEV), c['prj'].to(DEV), c['infer'].to(DEV), c['real'].to(DEV), c['cp'], c['texts'])
    hm, wm = mt.montage_size(*c['tile'])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (c['n'], 3, hm, wm) and got.is_cuda
    got = got.cpu().numpy()
    assert np.array_equal(got, c['want']), _show(got, c['want'])
    # the header band on its own, and everything outside the band's text and the tiles is background
    assert np.array_equal(got[:, :, :mt.BAND], c['want'][:, :, :mt.BAND]) and (got[0, :, :mt.BAND] == 0).any()
    outside = np.ones((hm, wm), dtype=bool)
    outside[:mt.BAND] = False
    for k in range(5):
        outside[mt.BAND + mt.PAD:mt.BAND + mt.PAD + c['tile'][0], mt.tile_x(k, c['tile'][1]):mt.tile_x(k, c['tile'][1]) + c['tile'][1]] = False
    assert (got[:, :, outside] == 255).all()
    assert set(np.unique(got[:, :, :mt.BAND])) <= {0, 255}


@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_diff_range_through_the_c_abi(hip, name):
    """spaa_montage_diff_range on its own: bit-equal to torch's min / max of the helper's difference image per item, and bitwise
    the same on a second call."""
    c = case(name)
    lib = hip['lib']
    scene, real = c['scene'].to(DEV).contiguous(), c['real'].to(DEV).contiguous()
    (hc, wc), (ch, cw), (hp, wp) = scene.shape[-2:], c['cp'], c['tile']
    y0, x0 = M.center_crop_origin(hc, wc, c['cp'])
    outs = []
    for _ in range(2):
        mm = torch.full((c['n'], 2), -7.0, device=DEV)            # (no initialisation needed: written in full)
        lib.call('spaa_montage_diff_range', lib.ptr(scene), hc, wc, y0, x0, lib.ptr(real), hc, wc, y0, x0, c['n'], ch, cw, hp, wp,
                 lib.ptr(mm))
        outs.append(mm.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    assert outs[0].tobytes() == c['rng'].tobytes(), (outs[0], c['rng'])
    assert mt.diff_range(scene, real, c['cp'], c['tile']).cpu().numpy().tobytes() == c['rng'].tobytes()
    # a crop that does not fit its image is refused by the entry point (no launch)
    with pytest.raises(RuntimeError, match='spaa_montage_diff_range'):
        lib.call('spaa_montage_diff_range', lib.ptr(scene), hc, wc, y0 + hc, x0, lib.ptr(real), hc, wc, y0, x0, c['n'], ch, cw, hp, wp,
                 lib.ptr(mm))


def test_constant_difference_item_and_no_leak(hip):
    """'many': item 5's capture equals the scene (mx == mn, where the reference divides by zero): its fifth tile is lut[0]
    everywhere; its neighbours keep their own ranges."""
    c = case('many')
    assert tuple(c['rng'][5]) == (0.0, 0.0) and c['rng'][6, 1] < 0.8 < c['rng'][4, 1]
    got = mt.attack_montages(c['scene'].to(DEV), c['prj'].to(DEV), c['infer'].to(DEV), c['real'].to(DEV), c['cp'], c['texts'])
    hp, wp = c['tile']
    tile = got[5, :, mt.BAND + mt.PAD:mt.BAND + mt.PAD + hp, mt.tile_x(4, wp):mt.tile_x(4, wp) + wp].cpu().numpy()
    assert (tile == mt.JET[0].reshape(3, 1, 1)).all()
    assert np.array_equal(got.cpu().numpy(), c['want'])


def test_colormap_argument_decodes_to_the_indices(hip):
    c = case('down')
    ramp = np.stack([np.arange(256), 255 - np.arange(256), np.arange(256) // 2], axis=1).astype(np.uint8)
    got = mt.attack_montages(c['scene'].to(DEV), c['prj'].to(DEV), c['infer'].to(DEV), c['real'].to(DEV), c['cp'], c['texts'],
                             colormap=ramp).cpu().numpy()
    hp, wp = c['tile']
    tile = got[:, :, mt.BAND + mt.PAD:mt.BAND + mt.PAD + hp, mt.tile_x(4, wp):mt.tile_x(4, wp) + wp]
    want = np.stack([mo.diff_index(c['scene'], c['real'][i], c['cp'], (hp, wp)) for i in range(c['n'])])
    assert np.array_equal(tile[:, 0], want) and np.array_equal(tile[:, 1], 255 - want) and np.array_equal(tile[:, 2], want // 2)
    assert len(np.unique(want)) > 100
    with pytest.raises(ValueError, match='colormap'):
        mt.attack_montages(c['scene'].to(DEV), c['prj'].to(DEV), c['infer'].to(DEV), c['real'].to(DEV), c['cp'], c['texts'],
                           colormap=ramp[:, :2])


def test_compose_through_the_c_abi_clips_glyphs(hip):
    """spaa_montage_compose called directly: glyphs that cross the montage's right and bottom edges are clipped, records that
    name no item or no glyph are skipped; no text at all (nrec = 0) leaves the tiles and the background."""
    c = case('identity')
    lib = hip['lib']
    t = {k: c[k].to(DEV).contiguous() for k in ('scene', 'prj', 'infer', 'real')}
    (hc, wc), (ch, cw), (hp, wp) = t['scene'].shape[-2:], c['cp'], c['tile']
    hm, wm = mt.montage_size(hp, wp)
    y0, x0 = M.center_crop_origin(hc, wc, c['cp'])
    mm = mt.diff_range(t['scene'], t['real'], c['cp'], c['tile'])
    lut, font = torch.from_numpy(mt.JET.copy()).to(DEV), torch.from_numpy(mt.FONT.copy()).to(DEV)
    blk = ord('#') - 32
    recs = [(0, wm - 3, 0, blk), (0, 40, hm - 4, blk), (0, -2, 3, blk), (1, 10, 0, blk), (-1, 10, 0, blk), (0, 10, 0, 95), (0, 10, 0, -1)]
    recs_d = torch.tensor(recs, dtype=torch.int32, device=DEV)

    def compose(nrec):
        out = torch.full((1, 3, hm, wm), 7, dtype=torch.uint8, device=DEV)
        lib.call('spaa_montage_compose', lib.ptr(t['scene']), hc, wc, y0, x0, lib.ptr(t['prj']), lib.ptr(t['infer']), hc, wc, y0, x0,
                 lib.ptr(t['real']), hc, wc, y0, x0, 1, ch, cw, hp, wp, lib.ptr(mm), lib.ptr(lut), lib.ptr(recs_d), nrec, lib.ptr(font),
                 mt.FONT_W, mt.FONT_H, lib.ptr(out))
        return out.cpu().numpy()[0]
    plain = mo.montage(c['scene'], c['prj'][0], c['infer'][0], c['real'][0], c['cp'], [('', '')] * 5)
    assert np.array_equal(compose(0), plain)
    want = plain.copy()
    for _, x, y, g in recs[:3]:
        for gy in range(mt.FONT_H):
            for gx in range(mt.FONT_W):
                if (mt.FONT[g, gy] >> gx) & 1 and 0 <= y + gy < hm and 0 <= x + gx < wm:
                    want[:, y + gy, x + gx] = 0
    assert np.array_equal(compose(len(recs)), want) and (want != plain).any()


def test_attack_results_is_one_montage_over_255(hip):
    c = case('up')
    A = hip['attack']
    n = c['n']
    d = {k: c[k].to(DEV) for k in ('scene', 'prj', 'infer', 'real')}
    labels = {k: f'class{k}, extra' for k in range(1000)}
    g = torch.Generator().manual_seed(3)
    ret = {}
    for key, rows in (('scene', 1), ('infer', n), ('real', n)):
        p = torch.softmax(4 * torch.randn(rows, 1000, generator=g), 1).sort(descending=True)
        ret[key] = (None, p[0].numpy(), p[1].numpy())
    gray = torch.full((1, 3, *c['tile']), 0.5, device=DEV)
    t = 4
    im = A.attack_results(ret, t, labels, gray, d['prj'], d['scene'][None], d['infer'], d['real'], c['tile'][::-1], c['cp'])
    assert im.dtype == torch.float32 and tuple(im.shape) == (3, *mt.montage_size(*c['tile']))
    l2 = (M.l2_norm(d['prj'][t], gray[0]), M.l2_norm(mo.cc(d['infer'][t], c['cp']), mo.cc(d['scene'], c['cp'])),
          M.l2_norm(mo.cc(d['real'][t], c['cp']), mo.cc(d['scene'], c['cp'])))
    texts = mt.attack_texts(t, *((labels[int(ret[k][2][r, 0])], float(ret[k][1][r, 0])) for k, r in (('scene', 0), ('infer', t), ('real', t))),
                            l2)
    assert texts[2][1] == f'{labels[int(ret["infer"][2][t, 0])]} ({ret["infer"][1][t, 0]:.2f})\tL2={l2[1]:.2f}'
    want = mt.attack_montages(d['scene'], d['prj'][t:t + 1], d['infer'][t:t + 1], d['real'][t:t + 1], c['cp'], [texts])[0].cpu()
    assert torch.equal(im.cpu(), want.float() / 255)
    # the tiles are those of the batch montage (the text differs)
    assert np.array_equal(want.numpy()[:, mt.BAND:], c['want'][t][:, mt.BAND:])


def test_summary_writes_the_montages(hip, tmp_path, monkeypatch):
    """A 64 x 64 setup (72 x 80 raw scene) attacked for two configurations, captured through project_capture_real_attack(capture='model'):
    montages=True writes 11 PNGs per configuration that equal attack_montages on the same images and labels, stats.txt is byte-identical
    to the montages=False run, which writes no PNG."""
    from PIL import Image
    A = hip['attack']
    attack_montages = mt.attack_montages
    sz, raw_sz, cp = (64, 64), (72, 80), (60, 60)
    sd = syn.pcnet_state_dict(0, cam_sz=sz, mask='rect')
    pc = hip['models'].PCNet(sd['mask'], hip['models'].WarpingNet(out_size=sz))
    pc.load_state_dict(sd)
    pc = pc.to(DEV)
    clf = hip['clf'].Classifier('resnet18', DEV, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0), input_sz=(56, 56))
    classifiers = {'resnet18': clf}
    root = tmp_path / 'data'
    setup_path = root / 'setups' / 'synth'
    io.save_setup_info(str(setup_path), dict(classifier_crop_sz=cp, prj_brightness=0.5, prj_im_sz=sz, cam_im_sz=sz))
    io.save_imgs(syn.scenes(1, 2, raw_sz), str(setup_path / 'cam/raw/ref'))
    _write_labels(root / 'imagenet1000_clsidx_to_labels.txt', {k: f'class{k}, extra' for k in range(1000)})
    labels = hip['clf'].load_imagenet_labels(str(root / 'imagenet1000_clsidx_to_labels.txt'))     # (the first name of each entry)
    _write_labels(root / 'imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in [1, 7, 21, 207, 340, 745, 779, 846, 947, 950]})
    cfg = A.get_attacker_cfg('SPAA', str(root), ['synth'])
    cfg.classifier_names, cfg.stealth_losses, cfg.d_threshes = ['resnet18'], ['caml2'], [5, 11]
    A.run_projector_based_attack(cfg, models={'synth': pc}, classifiers=classifiers, iters=3)
    A.project_capture_real_attack(cfg, capture='model', models={'synth': pc})
    cfg_str = A.to_attacker_cfg_str('SPAA')[0]
    folders = [os.path.join(cfg_str, 'caml2', str(d), 'resnet18') for d in (5, 11)]
    for f in folders:
        assert sorted(os.listdir(setup_path / 'cam/raw/adv' / f)) == sorted(os.listdir(setup_path / 'prj/adv' / f))
        assert len(os.listdir(setup_path / 'cam/raw/adv' / f)) == 11

    t0 = A.summarize_single_attacker('SPAA', str(root), ['synth'], classifiers=classifiers)
    stats = (setup_path / 'ret' / cfg_str / 'stats.txt').read_bytes()
    assert not [fn for _, _, fns in os.walk(setup_path / 'ret') for fn in fns if fn.endswith('.png')]
    calls = []
    monkeypatch.setattr(mt, 'attack_montages', lambda *a, **kw: calls.append(a[5]) or attack_montages(*a, **kw))
    t1 = A.summarize_single_attacker('SPAA', str(root), ['synth'], classifiers=classifiers, montages=True)
    monkeypatch.undo()
    assert len(calls) == 1 and len(calls[0]) == 22                          # every montage of the setup from one call
    assert (setup_path / 'ret' / cfg_str / 'stats.txt').read_bytes() == stats and t1.equals(t0) and len(t1) == 2

    scene = io.torch_imread(str(setup_path / 'cam/raw/ref/img_0002.png')).to(DEV)
    hm, wm = mt.montage_size(*sz)
    # the labels: one classifier call over the setup's images, composed as the summary composes it
    kinds = {kind: [io.torch_imread_mt(str(setup_path / kind / f)).to(DEV) for f in folders] for kind in ('prj/adv', 'cam/infer/adv', 'cam/raw/adv')}
    top = [None] * 5
    idx = A._sorted_classes(clf, [scene[None]] + kinds['cam/infer/adv'] + kinds['cam/raw/adv'], cp, top1=top)
    for j, f in enumerate(folders):
        names = sorted(os.listdir(setup_path / 'ret' / f))
        assert names == [f'img_{i:04d}.png' for i in range(1, 12)]
        got = np.stack([np.asarray(Image.open(setup_path / 'ret' / f / n)) for n in names])
        assert got.shape == (11, hm, wm, 3) and got.dtype == np.uint8
        prj, infer, real = (kinds[kind][j] for kind in ('prj/adv', 'cam/infer/adv', 'cam/raw/adv'))
        texts = []
        for t in range(11):
            l2 = (M.l2_norm(prj[t], torch.full_like(prj[t], 0.5)), M.l2_norm(mo.cc(infer[t], cp), mo.cc(scene, cp)),
                  M.l2_norm(mo.cc(real[t], cp), mo.cc(scene, cp)))
            texts.append(mt.attack_texts(t, (labels[int(idx[0][0, 0])], float(top[0][0])), (labels[int(idx[1 + j][t, 0])], float(top[1 + j][t])),
                                         (labels[int(idx[3 + j][t, 0])], float(top[3 + j][t])), l2))
        assert calls[0][11 * j:11 * (j + 1)] == texts
        want = mt.attack_montages(scene, prj, infer, real, cp, texts).permute(0, 2, 3, 1).cpu().numpy()
        assert np.array_equal(got, want), _show(got, want)
        assert (want[:, :mt.BAND] == 0).any()
