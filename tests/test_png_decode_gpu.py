"""GPU: the PNG decoder (csrc/png_decode.hip through spaa_amd.png.decode_png) against Pillow on files built in
tests/png_decode_cases.py -- every filter, every kind of deflate block, hand-made matches, a mixed batch, the malformed streams the
host build of the inflate core has already seen under sanitizers -- and the public readers with `device=`.  Pixels are exact."""
import faulthandler
import io as pyio
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_decode_cases as pc
from spaa_amd import io as sio
from spaa_amd import png
from spaa_amd import synthetic as syn
from spaa_amd import train_network as tn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FISH = os.path.join(ROOT, 'tests', 'golden', 'anemone_fish.png')


@pytest.fixture(autouse=True)
def time_limit():
    """A hung launch does not return to Python: the process ends with a traceback instead of waiting."""
    faulthandler.dump_traceback_later(60, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def pillow_rgb(data):
    with Image.open(pyio.BytesIO(data)) as im:
        return np.asarray(im.convert('RGB')).transpose(2, 0, 1)


def check_files(files, names):
    got = png.decode_png(files, DEV, names=names)
    assert len(got) == len(files)
    for g, f, n in zip(got, files, names):
        want = pillow_rgb(f)
        assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == want.shape, n
        assert np.array_equal(g.cpu().numpy(), want), n
    return got


def test_every_filter_size_and_channel_count():
    cases = pc.filter_cases()
    assert len(cases) == 4 * 3 * 6
    check_files([c.file() for c in cases], [c.name for c in cases])


def test_every_block_kind():
    cases = pc.zlib_cases() + pc.block_cases()
    names = [c.name for c in cases]
    for n in ('zlib_level1', 'zlib_level9', 'zlib_fixed', 'zlib_huffman_only', 'zlib_rle', 'zlib_sync_flush', 'zlib_full_flush',
              'zlib_level0_two_stored', 'dyn_run_crosses_tables', 'dyn_lengths_to_15', 'dyn_single_distance_code',
              'mixed_blocks_empty_stored'):
        assert n in names
    check_files([c.file() for c in cases], names)


def test_own_encoder_round_trip_and_the_fish():
    x = (syn.scenes(3, 2, (37, 53)) * 255).to(torch.uint8).to(DEV)
    files = png.encode_png(x) + [open(FISH, 'rb').read()]
    got = check_files(files, ['own0', 'own1', 'fish'])
    assert torch.equal(torch.stack(got[:2]), x)


def test_hand_made_fixed_huffman_matches():
    cases = pc.hand_cases()
    assert [c.name for c in cases][:3] == ['fixed_d32768_l258', 'fixed_d1_l258', 'fixed_d3_l10']
    assert all(c.shape == (105, 105, 3) and c.expect == 33180 for c in cases)
    check_files([c.file() for c in cases], [c.name for c in cases])


def test_batch_of_70_mixed_images_equals_each_alone():
    rng = np.random.default_rng(5)
    files = []
    for k in range(70):
        h, w, c = int(rng.integers(1, 40)), int(rng.integers(1, 50)), (1, 3, 4)[k % 3]
        img = pc.gradient_image(h, w, c, seed=k)
        raw = pc.filter_rows(img, rng.integers(0, 5, h))
        files.append(pc.make_png(w, h, c, pc.deflate(raw, (1, 6, 9)[k % 3])))
    names = [f'mixed{k}' for k in range(70)]
    batch = check_files(files, names)
    for k in range(0, 70, 7):                                      # (every image is also checked against Pillow above)
        assert torch.equal(png.decode_png([files[k]], DEV)[0], batch[k]), k
    assert torch.equal(png.decode_png(files[63:66], DEV)[1], batch[64])


def test_bad_streams_are_reported_and_do_not_disturb_the_good_ones():
    """Only streams the host program has handled cleanly (tests/test_png_decode_cpu.py runs pc.all_inflate_cases()): an error
    RETURN is checked, nothing here is meant to fault."""
    seen = {c.name for c in pc.all_inflate_cases()}
    good = [c for c in pc.filter_cases() if c.shape[:2] == (3, 5)] + pc.zlib_cases()[:2]
    bad = pc.malformed_cases()
    assert all(c.name in seen for c in good + bad)
    f5 = pc.filter5_case()                                         # a filter type that does not exist, in a stream that inflates
    assert f5.name in seen
    order, records, want = [], [], []
    for k, g in enumerate(good):
        order.append(g)
        records.append(g.record())
        want.append(0)
        if k < len(bad):
            order.append(bad[k])
            records.append(bad[k].record())
            want.append(bad[k].status)
    assert len(order) == len(good) + len(bad), 'more malformed streams than good ones to put them between'
    order.append(good[1])
    records.append(good[1].record(adler=zlib.adler32(good[1].raw) ^ 0x10000))
    want.append(png.ST_ADLER)
    order.append(f5)
    records.append(f5.record())
    want.append(pc.BAD_FILTER)
    images, status = png.decode_records(records, DEV)
    assert status.tolist() == want
    for case, im, st in zip(order, images, status):
        if st == 0:
            assert np.array_equal(im.cpu().numpy(), pillow_rgb(case.file())), case.name
    # decode_png names every bad file and its reason
    files = [good[0].file(), pc.make_png(39, 1, 1, pc.zwrap(bad[3].payload, b'')), good[1].file(),
             f5.file()]
    with pytest.raises(ValueError) as e:
        png.decode_png(files, DEV, names=['a.png', 'b.png', 'c.png', 'd.png'])
    msg = str(e.value)
    assert 'b.png' in msg and 'LEN and NLEN' in msg and 'd.png' in msg and 'filter type' in msg
    assert 'a.png' not in msg and 'c.png' not in msg
    wrong = bytearray(files[0])
    i = wrong.index(b'IEND') - 12
    wrong[i:i + 4] = bytes(4)                                       # the Adler-32 trailer; then the chunk's CRC is made right again
    j = wrong.index(b'IDAT')
    n = int.from_bytes(wrong[j - 4:j], 'big')
    wrong[j + 4 + n:j + 8 + n] = zlib.crc32(bytes(wrong[j:j + 4 + n])).to_bytes(4, 'big')
    with pytest.raises(ValueError, match='Adler-32'):
        png.decode_png([bytes(wrong)], DEV)
    # with the bad ones removed, the good ones are exact
    check_files([g.file() for g in good], [g.name for g in good])


@pytest.fixture(scope='module')
def image_dir(tmp_path_factory):
    """RGB, grey and RGBA files of 33 x 40, and one palette file (read through Pillow on either path)."""
    d = tmp_path_factory.mktemp('imread')
    for k, mode in enumerate(('RGB', 'L', 'RGBA', 'P', 'RGB', 'L')):
        Image.fromarray(pc.gradient_image(33, 40, 3, seed=k)).convert(mode).save(str(d / f'img_{k + 1:04d}.png'))
    return str(d)


@pytest.mark.parametrize('kw', [dict(), dict(index=[4, 0, 3]), dict(gray_scale=True), dict(normalize=True),
                                dict(index=[3, 1], gray_scale=True, normalize=True)], ids=str)
def test_torch_imread_mt_on_the_device_is_bit_equal(image_dir, kw):
    got = sio.torch_imread_mt(image_dir, device=DEV, **kw)
    want = sio.torch_imread_mt(image_dir, **kw)
    assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got.cpu(), want)


def test_torch_imread_mt_resized_is_within_one_grey_level(image_dir):
    got = sio.torch_imread_mt(image_dir, size=(20, 24), device=DEV)
    want = sio.torch_imread_mt(image_dir, size=(20, 24))
    assert got.shape == want.shape == (6, 3, 20, 24)
    levels = ((got.cpu() * 255).round() - (want * 255).round()).abs().max().item()      # both hold whole grey levels over 255
    print('resize: max difference', levels, 'grey levels')
    assert levels <= 1


def test_torch_imread_single_file_and_broken_file(image_dir, tmp_path):
    for k in (1, 2, 3, 4):
        path = os.path.join(image_dir, f'img_{k:04d}.png')
        got = sio.torch_imread(path, device=DEV)
        assert got.is_cuda and torch.equal(got.cpu(), sio.torch_imread(path))
    data = bytearray(open(os.path.join(image_dir, 'img_0001.png'), 'rb').read())
    data[data.index(b'IDAT') + 10] ^= 0x40                          # CRC no longer right: raised, never handed to Pillow
    (tmp_path / 'broken.png').write_bytes(bytes(data))
    with pytest.raises(ValueError, match='broken.png'):
        sio.torch_imread(str(tmp_path / 'broken.png'), device=DEV)


def test_load_data_with_gpu_decode_returns_the_same_eight(tmp_path):
    """A tiny setup written through Pillow (io.save_imgs of host tensors), like the one tests/test_direct_mask_gpu.py builds."""
    sz, root = (24, 32), tmp_path / 'data'
    setup = root / 'setups' / 'synth'
    sio.save_setup_info(str(setup), dict(classifier_crop_sz=(20, 20), prj_brightness=0.5, prj_im_sz=sz, cam_im_sz=sz[::-1]))
    sio.save_imgs(syn.scenes(1, 2, sz), str(setup / 'cam/raw/ref'))
    sio.save_imgs(syn.scenes(2, 5, sz), str(setup / 'cam/raw/train'))
    sio.save_imgs(syn.scenes(3, 3, sz), str(setup / 'cam/raw/test'))
    sio.save_imgs(syn.scenes(4, 5, sz), str(root / 'prj_share/train'))
    sio.save_imgs(syn.scenes(5, 4, sz), str(root / 'prj_share/test'))
    yy, xx = np.mgrid[0:sz[0], 0:sz[1]]
    lit = (abs(yy - sz[0] / 2) < sz[0] / 3) & (abs(xx - sz[1] / 2) < sz[1] / 3)
    cb = torch.stack([torch.from_numpy(lit * 0.5 * (0.9 + 0.1 * (((yy + 3 * k) // 4 + (xx + 5 * k) // 4) % 2)) + 0.03).float()
                      for k in range(4)])[:, None].expand(-1, 3, -1, -1)
    sio.save_imgs(cb.clamp(0, 1).contiguous(), str(setup / 'cam/raw/cb'))
    want = tn.load_data(str(root), 'synth', device=DEV, gpu_decode=False)
    got = tn.load_data(str(root), 'synth', device=DEV, gpu_decode=True)
    assert len(got) == len(want) == 8
    for g, w in zip(got[:6], want[:6]):
        assert g.device == w.device and g.dtype == w.dtype and torch.equal(g, w)
    assert got[6] == want[6] and dict(got[7]) == dict(want[7])
    assert want[5].any() and not want[5].all()
