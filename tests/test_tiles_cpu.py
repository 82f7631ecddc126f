"""CPU: the tile table.  csrc/tiles.hpp (read through spaa_tapconv_tile_info) and spaa_amd/tiles.py hold the same rows; what convplan
and tools/autotune.py derive from them is what they spelled out before the table existed; and spaa_tapconv_check, which reads the
table's capability bits, decides as the literal range chains of spaa_tapconv_f32 did."""
import ctypes
import importlib.util
import itertools
import os

from spaa_amd import _lib, convplan as cp, tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1   # hipErrorInvalidValue


def R(a, b):
    return set(range(a, b + 1))


def test_c_table_and_python_table_are_the_same():
    lib = _lib.load()
    known = 0
    for tid in range(128):
        info = _lib.TileInfo()
        rc = lib.spaa_tapconv_tile_info(tid, ctypes.byref(info))
        t = tiles.BY_ID.get(tid)
        if t is None:
            assert rc != 0, f'tile {tid}: in csrc/tiles.hpp but not in spaa_amd/tiles.py'
            continue
        assert rc == 0, f'tile {tid}: in spaa_amd/tiles.py but not in csrc/tiles.hpp'
        known += 1
        assert (info.id, info.name.decode(), info.family, info.bm, info.bn) == (t.id, t.name, t.family, t.bm, t.bn), tid
        for bit in range(32):
            assert (info.caps >> bit) & 1 == (t.caps >> bit) & 1, f'tile {tid}: capability bit {bit}'
    assert known == len(tiles.TABLE) == len(tiles.BY_ID) == 67
    assert lib.spaa_tapconv_tile_info(-1, ctypes.byref(_lib.TileInfo())) != 0 and lib.spaa_tapconv_tile_info(1 << 20, ctypes.byref(_lib.TileInfo())) != 0
    assert 75 not in tiles.BY_ID      # (the small-linear route is Python's own launch)


def test_derived_names_and_sets_are_those_spelled_out_before():
    names = {1: '128x128', 2: '256x64', 3: '256x32', 4: '128x64a', 5: '128x32', 6: '64x64', 7: '64x128', 8: '128x64b',
             9: 'direct4', 10: 'direct32', 11: 'thin4', 12: 'x6_64x64', 13: 'x6_128x32', 14: 'x6_32x128',
             15: 'x6v2_128x64g3', 16: 'x6v2_128x64g2', 17: 'x6v2_128x128g1', 18: 'x6v2_64x64g3', 19: 'x6v2_64x128g2',
             20: 'x6v3_128x64g3', 21: 'x6v3_128x64g2', 22: 'x6v3_64x64g3', 23: 'x6v3_128x128g1', 24: 'x6v3_64x128g2',
             25: 'x6d_128x128', 26: 'x6d_256x128', 27: 'x6d_128x64', 28: 'thinpatch32', 29: 'thinpatch16',
             30: 'x6d_128x32', 31: 'x6d_64x64', 32: 'x6d_64x128', 33: 'x6d_256x64',
             34: 'x6d16_128x128', 35: 'x6d16_256x128', 36: 'x6d16_128x64', 37: 'x6d16_128x32', 38: 'smallcin',
             39: 'x6d16co_128x128', 40: 'x6d16co_128x64', 41: 'x6d16co_128x32',
             42: 'x6d16a3_128x64', 43: 'x6d16a3_128x32', 44: 'x6da3_128x64', 45: 'x6d16coa3_128x64', 46: 'x6d16coa3_128x32', 47: 'thinpatch16x2',
             48: 'x6d16p_128x128', 49: 'x6d16p_128x64', 50: 'x6d16a3p_128x64', 51: 'x6da3p_128x64', 52: 'x6d16p_256x128',
             53: 'x6d16p_128x32', 54: 'x6dp_128x128',
             60: 'h16_128x128', 61: 'h16_128x64', 62: 'h16_128x32', 63: 'h16_128x16', 64: 'h16_256x128', 65: 'h16_256x256', 68: 'h16p_16x32x128', 72: 'thinmf_12x32',
             73: 'wino_x6_8x32x64', 74: 'x6p_4x32', 76: 'c3conv_16x32',
             70: 'wino_x6_16x32x128', 71: 'wino_x6_16x32x64'}
    assert type(cp.TILE_NAMES) is dict and cp.TILE_NAMES == names
    assert cp.X6D_TILES == set(range(25, 28)) | set(range(30, 38)) | set(range(39, 47)) | set(range(48, 55))
    assert cp.X6D_PERSISTENT == set(range(48, 55))
    assert cp.H16_TILES == set(range(60, 66))
    assert cp.STORE4_TILES == set(range(15, 28)) | set(range(30, 47)) | set(range(48, 55)) | set(range(60, 66)) | {68, 70, 71, 73, 74, 76}
    assert cp.F16OUT_TILES == set(range(15, 25)) | {38, 76} | set(range(60, 66))
    assert cp.WINO_TILES == {70, 71, 73}
    assert cp.X6_TILES == set(range(12, 55)) | {72, 74, 76}
    assert cp.H16_SPLITK_BN == {60: 128, 61: 64, 62: 32, 63: 16}
    assert cp.GATE_MUL_TILES == {t for t in names if t >= 25}
    for name in ('X6D_TILES', 'X6D_PERSISTENT', 'H16_TILES', 'STORE4_TILES', 'F16OUT_TILES', 'WINO_TILES'):
        assert type(getattr(cp, name)) is set, name


def test_tune_values_split_into_tile_and_k_ranges():
    assert [cp.split_tune_value(v) for v in (0, 34, 134, 234, 436, 948, 70, 171, 871)] == [
        (0, 0), (34, 0), (34, 1), (34, 2), (36, 4), (48, 9), (70, 0), (71, 1), (71, 8)]
    assert all(cp.split_tune_value(v)[0] in cp.TILE_NAMES for v in cp.TUNE.values())


def test_autotune_candidates_are_the_list_spelled_out_before():
    spec = importlib.util.spec_from_file_location('autotune_under_test', os.path.join(ROOT, 'tools', 'autotune.py'))
    autotune = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(autotune)
    assert autotune.default_candidates() == (
        list(range(1, 55)) + [70, 71, 73, 170, 171, 270, 271, 470, 471, 870, 871]
        + [s * 100 + t for s in (2, 4, 8) for t in (25, 27, 31, 34, 35, 36, 42, 48, 50, 52)] + [900 + t for t in (48, 49, 50, 51, 52, 53, 54)])


# ---- spaa_tapconv_check against the rules spaa_tapconv_f32 spelled out as number ranges (restated here; NOT read from tiles.py)
KNOWN = {0} | R(1, 54) | R(60, 65) | {68, 70, 71, 72, 73, 74, 76}
# capability -> (does the case ask for it?, may tile t do it in this case?)
RULES = {
    'byte masks': (lambda c: c['mask'], lambda t, c: t in R(15, 27) | R(30, 46) | R(48, 54) | R(60, 65) | {68, 70, 71, 73, 74, 76}),
    'fp16 in': (lambda c: c['f16in'], lambda t, c: t in R(60, 65) | {68} or (t in (29, 72) and not c['f16out'])),
    'fp16 in required': (lambda c: not c['f16in'], lambda t, c: t not in R(60, 63)),
    'fp16 out': (lambda c: c['f16out'], lambda t, c: t in R(15, 24) | {38} | R(60, 65) | {68, 76}),
    'fp16 out with K ranges': (lambda c: c['f16out'] and c['ksplit'] != 0, lambda t, c: c['ksplit'] > 1 and t in R(60, 63) | {68}),
    'GATE_MUL': (lambda c: c['gmul'], lambda t, c: t >= 25),
    'nfold': (lambda c: c['nfold'] > 1, lambda t, c: t in R(25, 27) | R(30, 37) | R(39, 46) | R(48, 54) | R(60, 65) | {68}),
    'second source': (lambda c: c['cin2'] > 0, lambda t, c: t in (68, 70, 71, 72, 73, 74)),
    # (its channels are the last Cin2 of Cin: a second source as wide as Cin leaves no channel for `in`)
    'in2 out of Cin': (lambda c: c['cin2'] == 64, lambda t, c: not (t in (70, 71, 73) or (t == 68 and c['nfold'] <= 1))),
}


def _descriptor(keep):
    """Cin 64, Cout 32, one class of one tap, 8 x 8 pixels, non-null dummy pointers (nothing is launched, nothing dereferences them)."""
    buf = ctypes.create_string_buffer(64)
    keep.append(buf)
    ptr = ctypes.addressof(buf)
    d = _lib.TapConv()
    d.inp = d.out = d.weights = d.taps = ptr
    d.Hin = d.Win = d.Hout = d.Wout = d.Hm = d.Wm = 8
    d.B, d.Cin, d.in_cstride, d.Cout, d.out_cstride, d.s_in, d.s_out, d.nclass = 1, 64, 64, 32, 32, 1, 1, 1
    d.cls[0].ntaps, d.cls[0].K, d.cls[0].Kpad = 1, 64, 64
    return d, ptr


def test_check_decides_as_the_literal_ranges_did():
    lib = _lib.load()
    keep = []
    d, ptr = _descriptor(keep)
    assert lib.spaa_tapconv_check(ctypes.byref(d)) == 0
    seen = {name: set() for name in RULES}
    dims = dict(mask=(False, True), f16in=(False, True), f16out=(False, True), ksplit=(0, 2, -1), nfold=(0, 4), gmul=(False, True),
                cin2=(0, 32, 64))      # (cin2: second source off / on / on and as wide as Cin)
    n = 0
    for values in itertools.product(*dims.values()):
        c = dict(zip(dims, values))
        d.mask_out = ptr if c['mask'] else None
        d.io_dtype = (_lib.IO_IN_F16 if c['f16in'] else 0) | (_lib.IO_OUT_F16 if c['f16out'] else 0)
        d.ksplit, d.nfold = c['ksplit'], c['nfold']
        d.gate, d.gate_cstride, d.gate_mode = (ptr, 32, _lib.GATE_MUL) if c['gmul'] else (None, 0, _lib.GATE_NONE)
        d.in2, d.in2_cstride, d.Cin2 = (ptr, 64, c['cin2']) if c['cin2'] else (None, 0, 0)
        for tid in range(128):
            verdicts = {name: may(tid, c) for name, (asked, may) in RULES.items() if asked(c)}
            if tid in KNOWN and tid != 0:
                for name, ok in verdicts.items():
                    seen[name].add(ok)
            want = 0 if tid in KNOWN and all(verdicts.values()) else INVALID
            d.tile = tid
            assert lib.spaa_tapconv_check(ctypes.byref(d)) == want, (tid, c, verdicts)
            n += 1
    assert n == 128 * 2 * 2 * 2 * 3 * 2 * 2 * 3
    for name, outcomes in seen.items():
        assert outcomes == {True, False}, f'{name}: only {outcomes} exercised'


def test_check_keeps_the_shape_checks():
    """What does not depend on the tile: null pointers, channel alignment, class bookkeeping, 32-bit offset ranges."""
    lib = _lib.load()
    keep = []
    for field, value in (('inp', None), ('out', None), ('weights', None), ('taps', None), ('Cin', 62), ('in_coff', 4), ('Cout', 33),
                         ('nclass', 5), ('nclass', 0), ('B', 0), ('s_in', 0), ('Hin', 1 << 20)):
        d, ptr = _descriptor(keep)
        d.tile = 34
        assert lib.spaa_tapconv_check(ctypes.byref(d)) == 0
        setattr(d, field, value)
        assert lib.spaa_tapconv_check(ctypes.byref(d)) == INVALID, field
    d, ptr = _descriptor(keep)
    d.cls[0].Kpad = 48      # (not a multiple of the 32-deep K step)
    assert lib.spaa_tapconv_check(ctypes.byref(d)) == INVALID
    d, ptr = _descriptor(keep)
    d.tile, d.mask_out, d.out_cstride, d.out_coff = 34, ptr, 36, 2      # (byte masks need channel quads)
    assert lib.spaa_tapconv_check(ctypes.byref(d)) == INVALID
