"""GPU: the PNG encoder's device half (csrc/png.hip through spaa_amd.png) against its numpy restatement (tests/png_hip_oracle.py) and
zlib, then io.save_imgs end to end.  Everything is bytes and integer sums: every comparison is exact.  The one bound, the file
size against Pillow's, is the 3 % the scheme was specified with (a host prototype measured 0.3-0.8 %)."""
import io as pyio
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_hip_oracle as po
from png_ref import decode_png
from spaa_amd import io as sio
from spaa_amd import montage as mt
from spaa_amd import png
from spaa_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# H, W: one pixel; a tiny image; a 160-byte row; a row longer than one 256-thread pass (2100 bytes) with fewer rows than one
# workgroup takes; more than one workgroup of rows, a row of 514 bytes, 9 packer chunks
SHAPES = [(1, 1), (5, 7), (37, 53), (3, 700), (64, 171)]
N = 3
_CASES = {}


def case(shape):
    """N = 3 different uint8 images [N,3,H,W] and the oracle's streams, histograms, row sums, tables and packed bytes; made once."""
    if shape not in _CASES:
        h, w = shape
        rng = np.random.default_rng(h * 1000 + w)
        noise = rng.integers(0, 256, (3, h, w))
        smooth = (np.cumsum(rng.integers(-3, 4, (3, h, w)), axis=2) + np.cumsum(rng.integers(-2, 3, (3, h, 1)), axis=1) + 128) & 255
        mixed = noise.copy()
        mixed[:, 1::4] = mixed[:, 0::4][:, :mixed[:, 1::4].shape[1]]       # a row equal to the one above: Up
        mixed[:, 2::4] = 77                                                # a constant row: Sub
        if h > 3:
            mixed[:, 3] = 0                                                # zeros under a constant row
        imgs = np.stack([noise, smooth, mixed]).astype(np.uint8)
        parts = [po.filter_image(im.transpose(1, 2, 0)) for im in imgs]
        tabs = [png.deflate_tables(p[1]) for p in parts]
        packed = [po.pack_image(p[0], *t) for p, t in zip(parts, tabs)]
        _CASES[shape] = dict(imgs=imgs, streams=np.stack([p[0] for p in parts]), hist=np.stack([p[1] for p in parts]),
                             rows=np.stack([p[2] for p in parts]), tabs=tabs, packed=packed)
    return _CASES[shape]


def run_filter(x):
    streams, stats = png.filter_hist(x)
    n, _, h, w = x.shape
    stats = stats.cpu().numpy()
    return streams.cpu().numpy().reshape(n, h, 1 + 3 * w), stats[:n * 257].reshape(n, 257), stats[n * 257:].reshape(n, h, 2)


def check_filter(got, c):
    streams, hist, rows = got
    assert np.array_equal(streams[:, :, 0], c['streams'][:, :, 0]), 'filter types differ'
    assert np.array_equal(streams, c['streams'])
    assert np.array_equal(hist, c['hist'])
    assert np.array_equal(rows, c['rows'] % 65521)
    row_len = streams.shape[2]
    assert png.adler32_from_rows(rows, row_len).tolist() == [zlib.adler32(s.tobytes()) for s in c['streams']]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('source', ['uint8', 'float32'])
def test_filter_entry_matches_the_oracle(shape, source):
    c = case(shape)
    x = torch.from_numpy(c['imgs']).to(DEV)
    if source == 'float32':
        x = x.float() / 255                       # exactly k / 255: must come back as k
        assert np.array_equal(po.to_bytes(x.cpu().numpy()), c['imgs'])
    got = run_filter(x)
    check_filter(got, c)
    again = run_filter(x)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_filter_choice_covers_every_filter_and_a_tie():
    c = case((64, 171))
    kinds = c['streams'][:, :, 0]
    assert set(np.unique(kinds).tolist()) == {0, 1, 2, 3, 4}
    # row 0 of the smooth image: nothing above, so Paeth predicts the left byte and ties with Sub; the lower number wins
    costs = po.filter_costs(c['imgs'][1].transpose(1, 2, 0), 0)
    assert costs[1] == costs[4] == min(costs) and kinds[1, 0] == 1
    got = run_filter(torch.from_numpy(c['imgs']).to(DEV))
    assert got[0][1, 0, 0] == 1
    # an all-zero image: every filter costs 0 on every row, None wins
    z = run_filter(torch.zeros(1, 3, 5, 7, dtype=torch.uint8, device=DEV))
    assert not z[0].any() and z[1][0, 0] == 5 * 22 and z[1][0, 256] == 1 and z[1][0].sum() == 5 * 22 + 1


def test_float_conversion_truncates():
    k = np.arange(256, dtype=np.float32)
    exact = k / np.float32(255)
    below = np.nextafter(exact, np.float32(0))
    x = np.zeros((1, 3, 8, 64), dtype=np.float32)
    x[0, 0, :4] = exact.reshape(4, 64)
    x[0, 0, 4:] = below.reshape(4, 64)
    x[0, 1] = 1.0
    x[0, 2] = np.random.default_rng(5).random((8, 64), dtype=np.float32)
    want = po.to_bytes(x)
    assert np.array_equal(want[0, 0, :4].reshape(-1), np.arange(256)) and (want[0, 1] == 255).all()
    assert np.array_equal(want[0, 0, 4:].reshape(-1), np.maximum(np.arange(256) - 1, 0))      # one ulp below k / 255: k - 1
    stream, hist, rows = po.filter_image(want[0].transpose(1, 2, 0))
    got = run_filter(torch.from_numpy(x).to(DEV))
    assert np.array_equal(got[0][0], stream) and np.array_equal(got[1][0], hist) and np.array_equal(got[2][0], rows % 65521)


def run_pack(c, gaps=(0, 0, 0)):
    """-> (the ragged buffer's bytes, the offsets [N + 1]); image i is placed gaps[i] bytes after the end of image i - 1."""
    n = len(c['tabs'])
    nbytes = [len(p) for p in c['packed']]
    for p, (hist, t) in zip(nbytes, zip(c['hist'], c['tabs'])):
        assert p == (png.deflate_bits(hist, t[1], t[3]) + 7) // 8                 # the host's exact size
    offsets = np.concatenate(([0], np.cumsum(nbytes))) + np.concatenate((np.cumsum(gaps), [sum(gaps)]))
    streams = torch.from_numpy(c['streams'].reshape(n, -1)).to(DEV)
    out = png.pack(streams, np.stack([t[0] for t in c['tabs']]), np.stack([t[1] for t in c['tabs']]), [t[2] for t in c['tabs']],
                   [t[3] for t in c['tabs']], offsets[:-1], offsets[-1])
    return out.cpu().numpy().tobytes(), offsets


@pytest.mark.parametrize('shape', SHAPES)
def test_pack_entry_matches_the_oracle(shape):
    """N = 3 images with their own tables at ragged byte offsets: every image's bytes, last zero-padded byte included, are the
    oracle's, so no image's bits reach its neighbour's first or last byte."""
    c = case(shape)
    got, offsets = run_pack(c)
    assert len(got) == (offsets[-1] + 3) // 4 * 4 and not any(got[offsets[-1]:])
    for i, want in enumerate(c['packed']):
        assert got[offsets[i]:offsets[i + 1]] == want, f'image {i}'
    assert run_pack(c)[0] == got
    # the same images one, two and three bytes further on: every alignment of a stream's start within a word
    for gaps in ((1, 1, 1), (2, 1, 1), (3, 3, 3)):
        moved, at = run_pack(c, gaps)
        ends = [0] + [at[i] + len(p) for i, p in enumerate(c['packed'])]
        for i, want in enumerate(c['packed']):
            assert moved[at[i]:at[i] + len(want)] == want, (gaps, i)
            assert not any(moved[ends[i]:at[i]]), (gaps, i)
        assert not any(moved[ends[-1]:])
    for want, stream in zip(c['packed'], c['streams']):
        assert zlib.decompress(want, wbits=-15) == stream.tobytes()


def test_pack_boundaries_fall_inside_codes():
    """The cases above split codes across the packer's units: a run (16 symbols) and a chunk (4096 symbols) start in the middle of
    a 32-bit word, so the word is shared by two threads, or two workgroups."""
    for shape, chunks in (((37, 53), 2), ((64, 171), 9)):
        c = case(shape)
        s = c['streams'][0].size
        assert s // png.PACK_CHUNK + 1 == chunks
        for i in range(N):
            start = po.symbol_bit_starts(c['streams'][i], c['tabs'][i][1], c['tabs'][i][3])
            assert (start[png.PACK_CHUNK::png.PACK_CHUNK] % 32 != 0).all()
            assert (start[png.PACK_RUN::png.PACK_RUN] % 32 != 0).mean() > 0.5


def read_dir(path):
    names = sorted(os.listdir(path))
    return names, np.stack([decode_png(os.path.join(path, n)) for n in names]).transpose(0, 3, 1, 2)


@pytest.mark.parametrize('source', ['uint8', 'float32'])
def test_save_imgs_round_trip(tmp_path, source, monkeypatch):
    x = torch.from_numpy(case((37, 53))['imgs']).to(DEV)
    if source == 'float32':
        g = torch.Generator().manual_seed(3)
        x = torch.rand(3, 3, 37, 53, generator=g).to(DEV)
        x[0, :, 0, 0] = torch.tensor([0.999, 0.5, 1.0], device=DEV)
    want = x.cpu().numpy() if source == 'uint8' else np.uint8(x.cpu().numpy() * 255)
    sio.save_imgs(x, str(tmp_path / 'out'), idx=4)
    names, got = read_dir(tmp_path / 'out')
    assert names == ['img_0005.png', 'img_0006.png', 'img_0007.png']
    assert np.array_equal(got, want)
    assert torch.equal(sio.torch_imread_mt(str(tmp_path / 'out')), torch.from_numpy(want).float() / 255)
    # a non-contiguous view
    view = x[:, :, 1::2, ::3]
    assert not view.is_contiguous()
    sio.save_imgs(view, str(tmp_path / 'view'))
    assert np.array_equal(read_dir(tmp_path / 'view')[1], want[:, :, 1::2, ::3])
    # a CPU tensor still goes through Pillow
    monkeypatch.setattr(png, 'encode_png', lambda *a, **k: pytest.fail('encode_png called for a CPU tensor'))
    sio.save_imgs(x.cpu(), str(tmp_path / 'cpu'))
    bio = pyio.BytesIO()
    Image.fromarray(np.ascontiguousarray(want[0].transpose(1, 2, 0))).save(bio, format='PNG')
    assert (tmp_path / 'cpu' / 'img_0001.png').read_bytes() == bio.getvalue()
    assert np.array_equal(read_dir(tmp_path / 'cpu')[1], want)


def test_montages_round_trip(tmp_path):
    g = torch.Generator().manual_seed(11)
    scene, prj = torch.rand(3, 24, 36, generator=g), torch.rand(4, 3, 28, 40, generator=g)
    infer, real = torch.rand(4, 3, 24, 36, generator=g), torch.rand(4, 3, 24, 36, generator=g)
    texts = [mt.attack_texts(t, ('tabby, tabby cat', 0.87), ('hamster', 0.64), ('hamster', 0.51), (4.56, 7.89, 8.12)) for t in range(4)]
    ims = mt.attack_montages(scene.to(DEV), prj.to(DEV), infer.to(DEV), real.to(DEV), (22, 30), texts)
    assert ims.dtype == torch.uint8 and ims.is_cuda
    sio.save_imgs(ims, str(tmp_path / 'm'))
    names, got = read_dir(tmp_path / 'm')
    assert names == [f'img_{i:04d}.png' for i in range(1, 5)] and np.array_equal(got, ims.cpu().numpy())
    with Image.open(tmp_path / 'm' / 'img_0001.png') as im:
        assert np.array_equal(np.asarray(im).transpose(2, 0, 1), ims[0].cpu().numpy())


def test_file_size_against_pillow():
    """synthetic.scenes at 256 x 256, plain and with uniform noise in [-8, 8]: no file more than 3 % above Pillow's default one."""
    u8 = po.to_bytes(syn.scenes(2, 2, (256, 256)).numpy())
    rng = np.random.default_rng(0)
    noisy = np.clip(u8.astype(np.int32) + rng.integers(-8, 9, u8.shape), 0, 255).astype(np.uint8)
    imgs = np.concatenate([u8, noisy])
    files = png.encode_png(torch.from_numpy(imgs).to(DEV))
    for i, data in enumerate(files):
        bio = pyio.BytesIO()
        Image.fromarray(np.ascontiguousarray(imgs[i].transpose(1, 2, 0))).save(bio, format='PNG')
        ratio = len(data) / len(bio.getvalue())
        print(f'image {i}: {len(data)} bytes, Pillow {len(bio.getvalue())}, ratio {ratio:.4f}')
        with Image.open(pyio.BytesIO(data)) as im:
            assert np.array_equal(np.asarray(im).transpose(2, 0, 1), imgs[i])
        assert ratio <= 1.03
