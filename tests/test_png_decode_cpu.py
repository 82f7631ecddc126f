"""CPU: the host half of the PNG decoder (spaa_amd/png.py: parse_png) and the inflate core the device runs
(spaa_amd/csrc/png_inflate_core.hpp), built for the host with AddressSanitizer and UBSan and run over every stream the GPU tests
decode -- well-formed and malformed -- before any of them reaches a GPU."""
import io as pyio
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import png_decode_cases as pc
from spaa_amd import _lib, png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FISH = os.path.join(ROOT, 'tests', 'golden', 'anemone_fish.png')


def pillow_png(arr, **kw):
    bio = pyio.BytesIO()
    Image.fromarray(arr).save(bio, format='PNG', **kw)
    return bio.getvalue()


def test_parse_png_concatenates_the_fish_idat_chunks():
    data = open(FISH, 'rb').read()
    assert data.count(b'IDAT') == 10
    rec = png.parse_png(data)
    with Image.open(FISH) as im:
        assert (rec.width, rec.height) == im.size and rec.channels == len(im.getbands())
    raw = zlib.decompress(rec.deflate, -15)
    assert len(raw) == rec.height * (1 + rec.width * rec.channels)
    assert zlib.adler32(raw) == rec.adler


def test_parse_png_takes_empty_and_one_byte_idat_chunks_and_skips_ancillary_ones():
    img = pc.gradient_image(5, 7, 3)
    raw = pc.filter_rows(img, [0, 1, 2, 3, 4])
    z = pc.deflate(raw, 6)
    cuts = [0, 0, 1, 2, 2, 3, len(z) - 1, len(z)]                  # zero-length and one-byte chunks, also first and last
    data = pc.make_png(7, 5, 3, z, cuts=cuts, extra=pc.chunk(b'tEXt', b'Comment\0hello') + pc.chunk(b'gAMA', struct.pack('>I', 45455)))
    assert data.count(b'IDAT') == len(cuts) + 1
    rec = png.parse_png(data)
    assert rec == png.PngRecord(7, 5, 3, z[2:-4], zlib.adler32(raw))
    with Image.open(pyio.BytesIO(data)) as im:                     # (the file is one Pillow reads, too)
        assert np.array_equal(np.asarray(im.convert('RGB')), img)


def test_parse_png_raises_on_a_broken_container():
    good = pc.make_png(7, 5, 3, pc.deflate(pc.filter_rows(pc.gradient_image(5, 7, 3), [0] * 5)))
    assert png.parse_png(good) is not None
    bad_crc = bytearray(good)
    bad_crc[good.index(b'IDAT') + 6] ^= 1
    cases = {
        'bad signature': b'\x89PNG\r\n\x1a\r' + good[8:],
        'bad CRC': bytes(bad_crc),
        'missing IHDR': good[:8] + good[8 + 25:],
        'missing IDAT': good[:good.index(b'IDAT') - 4] + pc.chunk(b'IEND', b''),
        'zero dimension': pc.make_png(0, 5, 3, pc.deflate(b'')),
        'zlib header': pc.make_png(7, 5, 3, b'\x78\x02' + good[good.index(b'IDAT') + 6:][:20]),
        'preset dictionary': pc.make_png(7, 5, 3, b'\x78\x20' + bytes(10)),
    }
    for name, data in cases.items():
        with pytest.raises(ValueError):
            png.parse_png(data)
            pytest.fail(name + ' was accepted')


def test_parse_png_declines_what_the_device_does_not_decode():
    rgb = pc.gradient_image(9, 11, 3)
    files = {}
    pal = pyio.BytesIO()
    Image.fromarray(rgb).convert('P').save(pal, format='PNG')
    files['palette'] = pal.getvalue()
    files['16-bit'] = pillow_png((rgb[..., 0].astype(np.uint16) * 257))
    files['1-bit'] = pillow_png(rgb[..., 0] > 128)
    # Pillow does not write interlaced files: the header of a well-formed file says so (parse_png decides on IHDR alone)
    files['interlaced'] = pc.make_png(11, 9, 3, pc.deflate(pc.filter_rows(rgb, [0] * 9)), interlace=1)
    for name, data in files.items():
        hdr = struct.unpack('>IIBBBBB', data[16:29])
        assert (hdr[2], hdr[3], hdr[6]) not in ((8, 0, 0), (8, 2, 0), (8, 6, 0)), name
        assert png.parse_png(data) is None, name
    for mode in ('L', 'RGB', 'RGBA'):
        rec = png.parse_png(pillow_png(np.asarray(Image.fromarray(rgb).convert(mode))))
        assert rec.channels == len(mode)


def test_decode_png_has_no_cpu_fallback():
    with pytest.raises(RuntimeError):
        png.decode_png([open(FISH, 'rb').read()], 'cpu')


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'a host C++ compiler is needed to build tests/host/png_inflate_host.cpp'
    exe = str(tmp_path_factory.mktemp('pih') / 'png_inflate_host')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall', '-Werror',
                    '-o', exe, os.path.join(ROOT, 'tests', 'host', 'png_inflate_host.cpp')], check=True)
    return exe


def test_inflate_core_is_clean_under_sanitizers_on_every_stream(host_program, tmp_path):
    """Every stream of the GPU tests: the expected bytes or the expected status, and no report from ASan or UBSan (a report ends the
    program with a non-zero status and text on stderr)."""
    cases = pc.all_inflate_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for wanted in ('truncated_mid_symbol', 'truncated_mid_stored', 'stored_len_nlen', 'block_type_3', 'oversubscribed_literals',
                   'incomplete_literals', 'repeat_16_first', 'repeat_past_tables', 'distance_past_start', 'output_one_longer',
                   'output_one_shorter', 'empty_payload'):
        assert wanted in names
    box = str(tmp_path / 'streams.pis')
    pc.write_container(box, cases)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([host_program, box], capture_output=True, text=True, env=env, timeout=120)
    lines = run.stdout.splitlines()
    assert run.returncode == 0 and run.stderr == '', (run.returncode, run.stderr[-2000:], [ln for ln in lines if not ln.endswith(' ok')])
    assert len(lines) == len(cases)
    for k, (c, ln) in enumerate(zip(cases, lines)):
        assert ln.startswith(f'{k} status={c.status} want={c.status} ') and ln.endswith(' ok'), (c.name, ln)


def test_new_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    for n in ('spaa_png_inflate', 'spaa_png_unfilter'):
        assert re.search(r'int\s+' + n + r'\s*\(', hdr), f'{n} not declared in include/spaa_hip.h'
        assert n in _lib._SIGNATURES and n in _lib.EXPORTS
        assert hasattr(_lib.load(), n)
    # the descriptor: five int64 and four int32, as the header lays them out
    import ctypes
    assert ctypes.sizeof(_lib.PngImg) == 56 and _lib.PngImg.ws_off.offset == 32
    for name, value in re.findall(r'#define (SPAA_PNG_[A-Z_0-9]+) (\d+)', hdr):
        assert getattr(pc, name[len('SPAA_PNG_'):]) == int(value), name
        if int(value):
            assert int(value) in png.STATUS_TEXT
    core = open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'png_inflate_core.hpp')).read()
    assert dict(re.findall(r'#define (SPAA_PNG_[A-Z_0-9]+) (\d+)', core)) == dict(re.findall(r'#define (SPAA_PNG_[A-Z_0-9]+) (\d+)', hdr))
