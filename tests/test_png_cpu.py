"""CPU: the host half of the PNG encoder (spaa_amd/png.py) -- the length-limited Huffman code, the deflate block header and the
container -- fed by the numpy restatement of the device half (tests/png_hip_oracle.py); and io.save_imgs' unchanged Pillow path."""
import heapq
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
from spaa_amd import png
from spaa_amd import synthetic as syn


def plain_huffman(counts):
    """Unlimited Huffman code lengths with heapq (every leaf of a merged subtree moves one level down)."""
    heap = [(c, i, (i,)) for i, c in enumerate(counts) if c > 0]
    heapq.heapify(heap)
    lengths = [0] * len(counts)
    n = len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lengths[s] += 1
        heapq.heappush(heap, (a[0] + b[0], n, a[2] + b[2]))
        n += 1
    return lengths


def kraft_units(lengths, max_bits):
    return sum(1 << (max_bits - b) for b in lengths if b)


def check_code(counts, lengths, max_bits):
    assert len(lengths) == len(counts)
    assert all((b > 0) == (c > 0) for b, c in zip(lengths, counts))
    assert max(lengths) <= max_bits
    assert kraft_units(lengths, max_bits) == 1 << max_bits          # complete: the Kraft sum is exactly 1


def fib(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


HISTS = {
    'two': [0] * 256 + [1],
    'uniform': [7] * 257,
    'geometric': [max(1, 100000 >> (i // 4)) for i in range(256)] + [1],
    'sparse': [(i * 7919) % 13 == 0 and (i * 31) % 97 + 1 for i in range(256)] + [1],
    'random': np.random.default_rng(1).integers(0, 5000, 257).tolist(),
    'laplace': [int(60000 * 0.93 ** min(i, 256 - i)) for i in range(256)] + [1],
}
HISTS['two'][17] = 35
HISTS['sparse'] = [int(c) for c in HISTS['sparse']]


@pytest.mark.parametrize('name', sorted(HISTS))
def test_huffman_lengths_are_complete_and_optimal(name):
    counts = HISTS[name]
    got = png.huffman_lengths(counts, 15)
    check_code(counts, got, 15)
    want = plain_huffman(counts)
    if max(want) <= 15:
        assert sum(c * b for c, b in zip(counts, got)) == sum(c * b for c, b in zip(counts, want))


def test_huffman_lengths_limit_a_deep_tree():
    counts = fib(40) + [0, 0, 3]                       # the plain tree is 39 deep
    assert max(plain_huffman(counts)) > 15
    got = png.huffman_lengths(counts, 15)
    check_code(counts, got, 15)
    order = sorted((i for i, c in enumerate(counts) if c), key=lambda i: counts[i])
    assert all(got[a] >= got[b] for a, b in zip(order, order[1:]))   # a rarer symbol never has the shorter code
    # a 257-symbol histogram with a Fibonacci tail, as an image could produce
    counts = fib(30) + [1] * 227
    check_code(counts, png.huffman_lengths(counts, 15), 15)


def test_code_length_code_fits_7_bits():
    counts = fib(19)                                   # plain depth 18
    assert max(plain_huffman(counts)) > 7
    check_code(counts, png.huffman_lengths(counts, 7), 7)
    counts = [0, 1, 0, 0, 2, 3, 5, 8, 13, 21, 34, 55, 89, 0, 0, 0, 0, 0, 0]
    check_code(counts, png.huffman_lengths(counts, 7), 7)
    flat = png.huffman_lengths([250, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], 7)
    assert flat[:2] == [1, 1]
    want = plain_huffman([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3, 2, 3, 8])
    got = png.huffman_lengths([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3, 2, 3, 8], 7)
    assert max(want) <= 7 and sorted(got) == sorted(want)


def _images():
    rng = np.random.default_rng(0)
    return {
        '1x1': np.array([[[1, 2, 3]]], np.uint8),
        'flat5x7': np.zeros((5, 7, 3), np.uint8),
        'noise37x53': rng.integers(0, 256, (37, 53, 3), dtype=np.uint8),
        'scene96x128': po.to_bytes(syn.scenes(1, 1, (96, 128)).numpy())[0].transpose(1, 2, 0).copy(),
    }


IMAGES = _images()


def oracle_png(img):
    stream, hist, rows = po.filter_image(img)
    codes, lengths, header, hbits = png.deflate_tables(hist)
    body = po.pack_image(stream, codes, lengths, header, hbits)
    assert 8 * len(body) - 7 <= png.deflate_bits(hist, lengths, hbits) <= 8 * len(body)
    adler = png.adler32_from_rows(rows, stream.shape[1])
    assert int(adler) == zlib.adler32(stream.tobytes())
    return png.wrap_png(img.shape[1], img.shape[0], body, adler), stream, lengths


@pytest.mark.parametrize('name', sorted(IMAGES))
def test_oracle_stream_through_the_host_half_decodes(name, tmp_path):
    img = IMAGES[name]
    data, stream, lengths = oracle_png(img)
    path = tmp_path / 'a.png'
    path.write_bytes(data)
    assert np.array_equal(decode_png(str(path)), img)
    with Image.open(pyio.BytesIO(data)) as im:
        assert im.mode == 'RGB' and im.size == (img.shape[1], img.shape[0])
        assert np.array_equal(np.asarray(im), img)
    # the zlib stream holds exactly the scanlines, and the codes are at most 15 bits and complete
    i = data.index(b'IDAT')
    n = int.from_bytes(data[i - 4:i], 'big')
    assert zlib.decompress(data[i + 4:i + 4 + n]) == stream.tobytes()
    check_code([int(b > 0) for b in lengths], [int(b) for b in lengths], 15)
    if name == 'flat5x7':
        assert lengths[0] == 1 and lengths[256] == 1 and int((lengths > 0).sum()) == 2


def test_scene_file_is_about_pillows_size():
    """No LZ77: the row filters and the entropy code carry the compression of a camera-like image."""
    img = IMAGES['scene96x128']
    bio = pyio.BytesIO()
    Image.fromarray(img).save(bio, format='PNG')
    assert len(oracle_png(img)[0]) <= 1.03 * len(bio.getvalue())


def test_adler_rows_combine_with_and_without_reduction():
    rng = np.random.default_rng(3)
    stream = rng.integers(200, 256, (3, 9, 18001), dtype=np.uint8)       # rows whose weighted sum passes 2^32
    w = 18001 - np.arange(18001, dtype=np.int64)
    rows = np.stack([stream.sum(-1, dtype=np.int64), (stream.astype(np.int64) * w).sum(-1)], axis=-1)
    assert rows[..., 1].max() > 1 << 32
    want = [zlib.adler32(s.tobytes()) for s in stream]
    assert png.adler32_from_rows(rows, 18001).tolist() == want
    assert png.adler32_from_rows(rows % 65521, 18001).tolist() == want


def test_save_imgs_host_inputs_still_go_through_pillow(tmp_path, monkeypatch):
    monkeypatch.setattr(png, 'encode_png', lambda *a, **k: pytest.fail('encode_png called for a host image'))
    arr = IMAGES['noise37x53'][None]
    sio.save_imgs(arr, str(tmp_path / 'arr'), idx=2)
    x = torch.from_numpy(arr.transpose(0, 3, 1, 2).copy())
    sio.save_imgs(x, str(tmp_path / 'u8'))
    sio.save_imgs(x.float() / 255, str(tmp_path / 'f32'))
    bio = pyio.BytesIO()
    Image.fromarray(arr[0]).save(bio, format='PNG')
    assert os.listdir(tmp_path / 'arr') == ['img_0003.png']
    for p in ('arr/img_0003.png', 'u8/img_0001.png', 'f32/img_0001.png'):
        assert (tmp_path / p).read_bytes() == bio.getvalue(), p


def test_encode_png_has_no_cpu_fallback():
    with pytest.raises(RuntimeError):
        png.encode_png(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError):
        png.encode_png(np.zeros((1, 4, 4, 3), np.uint8))
