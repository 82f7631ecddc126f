"""The tile table: every kernel id `spaa_tapconv_f32` dispatches, once on this side of the C ABI.

The same rows as csrc/tiles.hpp (tests/test_tiles_cpu.py compares the two through `spaa_tapconv_tile_info`): what an id is -- name,
kernel family, the GEMM tile where the id fixes one -- and what the kernel behind it can do.  `convplan` derives its tile sets from
here.  Adding a tile: a row here, the same row in csrc/tiles.hpp, a case in the family's `switch`.  Tile 75, the small-linear route
that `convplan.SmallLinearPlan` launches itself, is no tile of that dispatcher and has no row.
"""
import collections

# kernel families (include/spaa_hip.h: SPAA_FAM_*)
F32, DIRECT, THIN, X6, X6D, THINPATCH, SMALLCIN, H16, H16P, WINO, THINMF, X6P, C3 = range(13)
# capability bits (include/spaa_hip.h: SPAA_TILE_*)
MASKS, F16IN, F16IN_F32OUT, F16IN_REQ, F16OUT, F16OUT_KSPLIT, GATEMUL, NFOLD, IN2, IN2_CIN, PERSIST = (1 << i for i in range(11))

Tile = collections.namedtuple('Tile', 'id name family bm bn caps')

TABLE = (
    Tile(1, '128x128', F32, 128, 128, 0),
    Tile(2, '256x64', F32, 256, 64, 0),
    Tile(3, '256x32', F32, 256, 32, 0),
    Tile(4, '128x64a', F32, 128, 64, 0),
    Tile(5, '128x32', F32, 128, 32, 0),
    Tile(6, '64x64', F32, 64, 64, 0),
    Tile(7, '64x128', F32, 64, 128, 0),
    Tile(8, '128x64b', F32, 128, 64, 0),
    Tile(9, 'direct4', DIRECT, 0, 0, 0),
    Tile(10, 'direct32', DIRECT, 0, 0, 0),
    Tile(11, 'thin4', THIN, 0, 0, 0),
    Tile(12, 'x6_64x64', X6, 64, 64, 0),
    Tile(13, 'x6_128x32', X6, 128, 32, 0),
    Tile(14, 'x6_32x128', X6, 32, 128, 0),
    Tile(15, 'x6v2_128x64g3', X6, 128, 64, MASKS | F16OUT),
    Tile(16, 'x6v2_128x64g2', X6, 128, 64, MASKS | F16OUT),
    Tile(17, 'x6v2_128x128g1', X6, 128, 128, MASKS | F16OUT),
    Tile(18, 'x6v2_64x64g3', X6, 64, 64, MASKS | F16OUT),
    Tile(19, 'x6v2_64x128g2', X6, 64, 128, MASKS | F16OUT),
    Tile(20, 'x6v3_128x64g3', X6, 128, 64, MASKS | F16OUT),
    Tile(21, 'x6v3_128x64g2', X6, 128, 64, MASKS | F16OUT),
    Tile(22, 'x6v3_64x64g3', X6, 64, 64, MASKS | F16OUT),
    Tile(23, 'x6v3_128x128g1', X6, 128, 128, MASKS | F16OUT),
    Tile(24, 'x6v3_64x128g2', X6, 64, 128, MASKS | F16OUT),
    Tile(25, 'x6d_128x128', X6D, 128, 128, MASKS | GATEMUL | NFOLD),
    Tile(26, 'x6d_256x128', X6D, 256, 128, MASKS | GATEMUL | NFOLD),
    Tile(27, 'x6d_128x64', X6D, 128, 64, MASKS | GATEMUL | NFOLD),
    Tile(28, 'thinpatch32', THINPATCH, 0, 0, GATEMUL),
    Tile(29, 'thinpatch16', THINPATCH, 0, 0, F16IN | F16IN_F32OUT | GATEMUL),
    Tile(30, 'x6d_128x32', X6D, 128, 32, MASKS | GATEMUL | NFOLD),
    Tile(31, 'x6d_64x64', X6D, 64, 64, MASKS | GATEMUL | NFOLD),
    Tile(32, 'x6d_64x128', X6D, 64, 128, MASKS | GATEMUL | NFOLD),
    Tile(33, 'x6d_256x64', X6D, 256, 64, MASKS | GATEMUL | NFOLD),
    Tile(34, 'x6d16_128x128', X6D, 128, 128, MASKS | GATEMUL | NFOLD),
    Tile(35, 'x6d16_256x128', X6D, 256, 128, MASKS | GATEMUL | NFOLD),
    Tile(36, 'x6d16_128x64', X6D, 128, 64, MASKS | GATEMUL | NFOLD),
    Tile(37, 'x6d16_128x32', X6D, 128, 32, MASKS | GATEMUL | NFOLD),
    Tile(38, 'smallcin', SMALLCIN, 0, 0, MASKS | F16OUT | GATEMUL),
    Tile(39, 'x6d16co_128x128', X6D, 128, 128, MASKS | GATEMUL | NFOLD),
    Tile(40, 'x6d16co_128x64', X6D, 128, 64, MASKS | GATEMUL | NFOLD),
    Tile(41, 'x6d16co_128x32', X6D, 128, 32, MASKS | GATEMUL | NFOLD),
    Tile(42, 'x6d16a3_128x64', X6D, 128, 64, MASKS | GATEMUL | NFOLD),
    Tile(43, 'x6d16a3_128x32', X6D, 128, 32, MASKS | GATEMUL | NFOLD),
    Tile(44, 'x6da3_128x64', X6D, 128, 64, MASKS | GATEMUL | NFOLD),
    Tile(45, 'x6d16coa3_128x64', X6D, 128, 64, MASKS | GATEMUL | NFOLD),
    Tile(46, 'x6d16coa3_128x32', X6D, 128, 32, MASKS | GATEMUL | NFOLD),
    Tile(47, 'thinpatch16x2', THINPATCH, 0, 0, GATEMUL),
    Tile(48, 'x6d16p_128x128', X6D, 128, 128, MASKS | GATEMUL | NFOLD | PERSIST),
    Tile(49, 'x6d16p_128x64', X6D, 128, 64, MASKS | GATEMUL | NFOLD | PERSIST),
    Tile(50, 'x6d16a3p_128x64', X6D, 128, 64, MASKS | GATEMUL | NFOLD | PERSIST),
    Tile(51, 'x6da3p_128x64', X6D, 128, 64, MASKS | GATEMUL | NFOLD | PERSIST),
    Tile(52, 'x6d16p_256x128', X6D, 256, 128, MASKS | GATEMUL | NFOLD | PERSIST),
    Tile(53, 'x6d16p_128x32', X6D, 128, 32, MASKS | GATEMUL | NFOLD | PERSIST),
    Tile(54, 'x6dp_128x128', X6D, 128, 128, MASKS | GATEMUL | NFOLD | PERSIST),
    Tile(60, 'h16_128x128', H16, 128, 128, MASKS | F16IN | F16IN_REQ | F16OUT | F16OUT_KSPLIT | GATEMUL | NFOLD),
    Tile(61, 'h16_128x64', H16, 128, 64, MASKS | F16IN | F16IN_REQ | F16OUT | F16OUT_KSPLIT | GATEMUL | NFOLD),
    Tile(62, 'h16_128x32', H16, 128, 32, MASKS | F16IN | F16IN_REQ | F16OUT | F16OUT_KSPLIT | GATEMUL | NFOLD),
    Tile(63, 'h16_128x16', H16, 128, 16, MASKS | F16IN | F16IN_REQ | F16OUT | F16OUT_KSPLIT | GATEMUL | NFOLD),
    Tile(64, 'h16_256x128', H16, 256, 128, MASKS | F16IN | F16OUT | GATEMUL | NFOLD),
    Tile(65, 'h16_256x256', H16, 256, 256, MASKS | F16IN | F16OUT | GATEMUL | NFOLD),
    Tile(68, 'h16p_16x32x128', H16P, 0, 0, MASKS | F16IN | F16OUT | F16OUT_KSPLIT | GATEMUL | NFOLD | IN2 | IN2_CIN),
    Tile(70, 'wino_x6_16x32x128', WINO, 0, 0, MASKS | GATEMUL | IN2 | IN2_CIN),
    Tile(71, 'wino_x6_16x32x64', WINO, 0, 0, MASKS | GATEMUL | IN2 | IN2_CIN),
    Tile(72, 'thinmf_12x32', THINMF, 0, 0, F16IN | F16IN_F32OUT | GATEMUL | IN2),
    Tile(73, 'wino_x6_8x32x64', WINO, 0, 0, MASKS | GATEMUL | IN2 | IN2_CIN),
    Tile(74, 'x6p_4x32', X6P, 0, 0, MASKS | GATEMUL | IN2),
    Tile(76, 'c3conv_16x32', C3, 0, 0, MASKS | F16OUT | GATEMUL),
)
BY_ID = {t.id: t for t in TABLE}


def with_caps(caps):
    """The ids whose kernel has every capability bit of `caps`."""
    return {t.id for t in TABLE if t.caps & caps == caps}


def of_family(*families):
    """The ids of these kernel families."""
    return {t.id for t in TABLE if t.family in families}
