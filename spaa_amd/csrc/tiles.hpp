// tiles.hpp — the tile table: every kernel id spaa_tapconv_f32 dispatches, once.  What an id is (name, kernel family, the GEMM tile
// where the id fixes one) and what the kernel behind it can do (include/spaa_hip.h: SPAA_TILE_*).  spaa_tapconv_check reads the
// capability bits, the dispatcher the family; the template arguments of an id stay with its family's launcher.  Host-only.
// spaa_amd/tiles.py holds the same rows for the planner; tests/test_tiles_cpu.py compares the two through spaa_tapconv_tile_info.
// Adding a tile: a row here, the same row there, a case in the family's switch.
#pragma once
#include "../../include/spaa_hip.h"

namespace spaa_tiles {

struct entry_t {
    int id;
    const char* name;
    int family, bm, bn;
    unsigned caps;
};

enum : unsigned {
    MASKS = SPAA_TILE_BYTE_MASKS, F16IN = SPAA_TILE_F16_IN, F16IN_F32OUT = SPAA_TILE_F16_IN_F32_OUT, F16IN_REQ = SPAA_TILE_F16_IN_REQUIRED,
    F16OUT = SPAA_TILE_F16_OUT, F16OUT_KSPLIT = SPAA_TILE_F16_OUT_KSPLIT, GATEMUL = SPAA_TILE_GATE_MUL, NFOLD = SPAA_TILE_NFOLD,
    IN2 = SPAA_TILE_IN2, IN2_CIN = SPAA_TILE_IN2_OF_CIN, PERSIST = SPAA_TILE_PERSISTENT
};

// id, name, family, BM, BN, capabilities
inline constexpr entry_t TABLE[] = {
    {1, "128x128", SPAA_FAM_F32, 128, 128, 0},
    {2, "256x64", SPAA_FAM_F32, 256, 64, 0},
    {3, "256x32", SPAA_FAM_F32, 256, 32, 0},
    {4, "128x64a", SPAA_FAM_F32, 128, 64, 0},
    {5, "128x32", SPAA_FAM_F32, 128, 32, 0},
    {6, "64x64", SPAA_FAM_F32, 64, 64, 0},
    {7, "64x128", SPAA_FAM_F32, 64, 128, 0},
    {8, "128x64b", SPAA_FAM_F32, 128, 64, 0},
    {9, "direct4", SPAA_FAM_DIRECT, 0, 0, 0},
    {10, "direct32", SPAA_FAM_DIRECT, 0, 0, 0},
    {11, "thin4", SPAA_FAM_THIN, 0, 0, 0},
    {12, "x6_64x64", SPAA_FAM_X6, 64, 64, 0},
    {13, "x6_128x32", SPAA_FAM_X6, 128, 32, 0},
    {14, "x6_32x128", SPAA_FAM_X6, 32, 128, 0},
    {15, "x6v2_128x64g3", SPAA_FAM_X6, 128, 64, MASKS | F16OUT},
    {16, "x6v2_128x64g2", SPAA_FAM_X6, 128, 64, MASKS | F16OUT},
    {17, "x6v2_128x128g1", SPAA_FAM_X6, 128, 128, MASKS | F16OUT},
    {18, "x6v2_64x64g3", SPAA_FAM_X6, 64, 64, MASKS | F16OUT},
    {19, "x6v2_64x128g2", SPAA_FAM_X6, 64, 128, MASKS | F16OUT},
    {20, "x6v3_128x64g3", SPAA_FAM_X6, 128, 64, MASKS | F16OUT},
    {21, "x6v3_128x64g2", SPAA_FAM_X6, 128, 64, MASKS | F16OUT},
    {22, "x6v3_64x64g3", SPAA_FAM_X6, 64, 64, MASKS | F16OUT},
    {23, "x6v3_128x128g1", SPAA_FAM_X6, 128, 128, MASKS | F16OUT},
    {24, "x6v3_64x128g2", SPAA_FAM_X6, 64, 128, MASKS | F16OUT},
    {25, "x6d_128x128", SPAA_FAM_X6D, 128, 128, MASKS | GATEMUL | NFOLD},
    {26, "x6d_256x128", SPAA_FAM_X6D, 256, 128, MASKS | GATEMUL | NFOLD},
    {27, "x6d_128x64", SPAA_FAM_X6D, 128, 64, MASKS | GATEMUL | NFOLD},
    {28, "thinpatch32", SPAA_FAM_THINPATCH, 0, 0, GATEMUL},
    {29, "thinpatch16", SPAA_FAM_THINPATCH, 0, 0, F16IN | F16IN_F32OUT | GATEMUL},
    {30, "x6d_128x32", SPAA_FAM_X6D, 128, 32, MASKS | GATEMUL | NFOLD},
    {31, "x6d_64x64", SPAA_FAM_X6D, 64, 64, MASKS | GATEMUL | NFOLD},
    {32, "x6d_64x128", SPAA_FAM_X6D, 64, 128, MASKS | GATEMUL | NFOLD},
    {33, "x6d_256x64", SPAA_FAM_X6D, 256, 64, MASKS | GATEMUL | NFOLD},
    {34, "x6d16_128x128", SPAA_FAM_X6D, 128, 128, MASKS | GATEMUL | NFOLD},
    {35, "x6d16_256x128", SPAA_FAM_X6D, 256, 128, MASKS | GATEMUL | NFOLD},
    {36, "x6d16_128x64", SPAA_FAM_X6D, 128, 64, MASKS | GATEMUL | NFOLD},
    {37, "x6d16_128x32", SPAA_FAM_X6D, 128, 32, MASKS | GATEMUL | NFOLD},
    {38, "smallcin", SPAA_FAM_SMALLCIN, 0, 0, MASKS | F16OUT | GATEMUL},
    {39, "x6d16co_128x128", SPAA_FAM_X6D, 128, 128, MASKS | GATEMUL | NFOLD},
    {40, "x6d16co_128x64", SPAA_FAM_X6D, 128, 64, MASKS | GATEMUL | NFOLD},
    {41, "x6d16co_128x32", SPAA_FAM_X6D, 128, 32, MASKS | GATEMUL | NFOLD},
    {42, "x6d16a3_128x64", SPAA_FAM_X6D, 128, 64, MASKS | GATEMUL | NFOLD},
    {43, "x6d16a3_128x32", SPAA_FAM_X6D, 128, 32, MASKS | GATEMUL | NFOLD},
    {44, "x6da3_128x64", SPAA_FAM_X6D, 128, 64, MASKS | GATEMUL | NFOLD},
    {45, "x6d16coa3_128x64", SPAA_FAM_X6D, 128, 64, MASKS | GATEMUL | NFOLD},
    {46, "x6d16coa3_128x32", SPAA_FAM_X6D, 128, 32, MASKS | GATEMUL | NFOLD},
    {47, "thinpatch16x2", SPAA_FAM_THINPATCH, 0, 0, GATEMUL},
    {48, "x6d16p_128x128", SPAA_FAM_X6D, 128, 128, MASKS | GATEMUL | NFOLD | PERSIST},
    {49, "x6d16p_128x64", SPAA_FAM_X6D, 128, 64, MASKS | GATEMUL | NFOLD | PERSIST},
    {50, "x6d16a3p_128x64", SPAA_FAM_X6D, 128, 64, MASKS | GATEMUL | NFOLD | PERSIST},
    {51, "x6da3p_128x64", SPAA_FAM_X6D, 128, 64, MASKS | GATEMUL | NFOLD | PERSIST},
    {52, "x6d16p_256x128", SPAA_FAM_X6D, 256, 128, MASKS | GATEMUL | NFOLD | PERSIST},
    {53, "x6d16p_128x32", SPAA_FAM_X6D, 128, 32, MASKS | GATEMUL | NFOLD | PERSIST},
    {54, "x6dp_128x128", SPAA_FAM_X6D, 128, 128, MASKS | GATEMUL | NFOLD | PERSIST},
    {60, "h16_128x128", SPAA_FAM_H16, 128, 128, MASKS | F16IN | F16IN_REQ | F16OUT | F16OUT_KSPLIT | GATEMUL | NFOLD},
    {61, "h16_128x64", SPAA_FAM_H16, 128, 64, MASKS | F16IN | F16IN_REQ | F16OUT | F16OUT_KSPLIT | GATEMUL | NFOLD},
    {62, "h16_128x32", SPAA_FAM_H16, 128, 32, MASKS | F16IN | F16IN_REQ | F16OUT | F16OUT_KSPLIT | GATEMUL | NFOLD},
    {63, "h16_128x16", SPAA_FAM_H16, 128, 16, MASKS | F16IN | F16IN_REQ | F16OUT | F16OUT_KSPLIT | GATEMUL | NFOLD},
    {64, "h16_256x128", SPAA_FAM_H16, 256, 128, MASKS | F16IN | F16OUT | GATEMUL | NFOLD},
    {65, "h16_256x256", SPAA_FAM_H16, 256, 256, MASKS | F16IN | F16OUT | GATEMUL | NFOLD},
    {68, "h16p_16x32x128", SPAA_FAM_H16P, 0, 0, MASKS | F16IN | F16OUT | F16OUT_KSPLIT | GATEMUL | NFOLD | IN2 | IN2_CIN},
    {70, "wino_x6_16x32x128", SPAA_FAM_WINO, 0, 0, MASKS | GATEMUL | IN2 | IN2_CIN},
    {71, "wino_x6_16x32x64", SPAA_FAM_WINO, 0, 0, MASKS | GATEMUL | IN2 | IN2_CIN},
    {72, "thinmf_12x32", SPAA_FAM_THINMF, 0, 0, F16IN | F16IN_F32OUT | GATEMUL | IN2},
    {73, "wino_x6_8x32x64", SPAA_FAM_WINO, 0, 0, MASKS | GATEMUL | IN2 | IN2_CIN},
    {74, "x6p_4x32", SPAA_FAM_X6P, 0, 0, MASKS | GATEMUL | IN2},
    {76, "c3conv_16x32", SPAA_FAM_C3, 0, 0, MASKS | F16OUT | GATEMUL},
};

// the entry of `id`, or nullptr: no such tile (0 = "auto" is the dispatcher's heuristic, not a tile)
inline const entry_t* find(int id) {
    for (const entry_t& e : TABLE)
        if (e.id == id) return &e;
    return nullptr;
}

}  // namespace spaa_tiles
