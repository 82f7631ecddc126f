/*
 * spaa_hip.h — C-ABI of libspaa_hip.so: the MI355X (gfx950) kernels behind the SPAA attack loop.
 *
 * The reference (BingyaoHuang/SPAA) is pure Python over ATen; it has no FFI layer.  The drop-in boundary is
 * therefore the set of tensor operations its hot path dispatches (SURVEY.md §2.1 G0–G16, §8b).  Every entry point
 * takes raw device pointers, plain sizes and a hipStream_t, returns 0 on success or a hipError_t value, never
 * allocates, frees or synchronises (graph-capture safe), and names the reference call it replaces
 * (paths relative to /root/reference/src/python).
 *
 * Layout convention: activations are NHWC fp32 with an explicit channel stride (`cstride`, multiple of 4) and
 * channel offset (`coff`, multiple of 4); 3-channel images are stored NHWC with cstride 4 ("NHWC4", pad lane = 0).
 * The reference's NCHW tensors are converted at the Python boundary by spaa_nchw_to_nhwc4 / spaa_nhwc4_to_nchw.
 */
#ifndef SPAA_HIP_H
#define SPAA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* spaa_stream_t; /* hipStream_t */

#define SPAA_MAX_CLASSES 4
#define SPAA_MAX_TAPS 64
#define SPAA_SPLITK_HDR_FLOATS 4096 /* arrival counters at the head of a K-range workspace (SPAA_SPLITK_FIXUP) */

/* activation applied after bias + residual add */
enum { SPAA_ACT_NONE = 0, SPAA_ACT_RELU = 1, SPAA_ACT_RELU_CLAMP1 = 2, SPAA_ACT_LEAKY01 = 3 };
/* fp16-storage flags (spaa_tapconv_t.io_dtype) */
enum { SPAA_IO_IN_F16 = 1, SPAA_IO_OUT_F16 = 2 };
/* gate applied last (ReLU / clamp backward):  out = pass(gate) ? v : 0 */
enum { SPAA_GATE_NONE = 0, SPAA_GATE_POS = 1 /* gate > 0 */, SPAA_GATE_POS_LE1 = 2 /* 0 < gate <= 1 */,
       SPAA_GATE_MUL = 3 /* value * gate: the chain rule through `x * s` (models.py:342); SPAA_TILE_GATE_MUL tiles only */ };

typedef struct {
    int32_t oy0, ox0;  /* output offset of this parity class */
    int32_t ntaps;     /* taps of this class */
    int32_t tap_off;   /* first tap in `taps` */
    int32_t K;         /* ntaps * Cin */
    int32_t Kpad;      /* K rounded up to 32 */
    int64_t w_off;     /* float offset of this class's packed weights [Npad][Kpad] */
} spaa_tapclass_t;

/*
 * Per-tile FORM FLAGS of a launch: the bits of spaa_tapconv_t.reserved0 / reserved1 / reserved2.  Which kernel form a tile runs is
 * asked for here, by name; a name is the mask IN its word, and a field wider than one bit has a NAME_SHIFT next to it (value =
 * (word & NAME) >> NAME_SHIFT).  A name holds for the tiles stated: the same bit means something else, or nothing, elsewhere.
 * spaa_amd/_lib.py mirrors the names without the SPAA_ prefix (tests/test_cabi_cpu.py pins the two to each other).
 *
 * The product (spaa_amd/convplan.py with no switch set) sets SPAA_WINO_PAD, SPAA_C3_F16_OPERANDS, SPAA_H16P_CV with SPAA_H16P_CV_BN,
 * SPAA_H16P_LEAN_WIDE, SPAA_H16P_POOL, SPAA_H16P_UNPOOL and SPAA_X6P_STD, and the Winograd launcher sets SPAA_WINO_NO_CANVAS on its
 * own copy.  Everything else is a measurement (A/B run, timing ablation) or test switch, clear in a default launch.
 */
enum {
    /* ---- reserved0, every tile: measurement and test switches (spaa_amd/convplan.py DEBUG_*) ---- */
    SPAA_DBG_X6D_TAPMAJOR = 1 << 0,      /* x6d kernels: tap-major K order (A/B runs) */
    SPAA_DBG_PERSIST_CAP = 0xff << 8, SPAA_DBG_PERSIST_CAP_SHIFT = 8,   /* persistent x6d launches: > 0 = that many workgroups (tests: several tiles per workgroup on small layers) */
    SPAA_DBG_X6P_ABLATE = 0xff << 8, SPAA_DBG_X6P_ABLATE_SHIFT = 8,     /* the same bits in the -DSPAA_X6P_STAMP build of tile 74: timing-only ablation mask (wrong results) */
    SPAA_DBG_WINO_VAR = 3 << 16, SPAA_DBG_WINO_VAR_SHIFT = 16,          /* Winograd tiles: flips the bits of the launcher's kernel variant (A/B runs) */
    SPAA_DBG_WINO_ABLATE = 127 << 18, SPAA_DBG_WINO_ABLATE_SHIFT = 18,  /* Winograd tiles in a -DSPAA_WINO_ABLATE build: timing-only ablation mask (wrong results) */
    SPAA_DBG_H16_2STAGE = 1 << 25,       /* fp16 implicit-GEMM tiles: never the four-stage form (A/B runs) */
    SPAA_DBG_SMALLCIN_NOSLAB = 1 << 26,  /* smallcin tile: stride-2 layers with a residual store from the MFMA layout (A/B runs) */
    /* ---- reserved0, tile 72 only ---- */
    SPAA_DBG_THINMF = 7 << 27, SPAA_DBG_THINMF_SHIFT = 27,              /* -DSPAA_THINMF_ABLATE build: timing-only ablation mask (wrong results) */
    /* ---- reserved0, Winograd tiles (70 / 71 / 73) only ---- */
    SPAA_WINO_PAD = 3 << 27, SPAA_WINO_PAD_SHIFT = 27,   /* PRODUCT INPUT: the layer's zero padding as a code, 0 = pad 1 (same-size output), 1 = pad 0
                                                            (unpadded: output 2 smaller), 2 = pad 2 (that layer's input gradient: 2 larger) */
    SPAA_WINO_FORCE_CANVAS = 1 << 29,    /* tests: the canvas layout wherever it has fewer workgroup regions, whatever the cost model says */
    SPAA_WINO_NO_CANVAS = 1 << 30,       /* A/B runs: small images keep the image-aligned regions (no canvas, no K ranges); the launcher sets it on
                                            its own copy for two-source and unpadded layers */

    /* ---- reserved1 ---- */
    SPAA_C3_F16_OPERANDS = 1 << 0,       /* tile 76 (fp16-storage mode, fp16 output only): the image rounded to fp16 in registers, `w_split` = ONE plane of
                                            fp16 weights in the layout of ConvPlan.c3_pack(half=True), products on v_mfma_f32_16x16x32_f16 */
    SPAA_H16P_CV_BN = 3 << 0, SPAA_H16P_CV_BN_SHIFT = 0,   /* tile 68 with SPAA_H16P_CV: the N tile, 0 = the plan chooses, 1 = 64, 2 = 128 */
    SPAA_H16P_CV = 1 << 2,               /* tile 68: the canvas / K-range form (small images with long K: spaa_tapconv_h16p_plan below; `ksplit` > 1 with
                                            `splitk_ws` = that many K ranges) */
    SPAA_H16P_CV_FORCE = 1 << 3,         /* tile 68 with SPAA_H16P_CV (tests): canvases wherever they have fewer regions */
    SPAA_H16P_ONE_WG = 1 << 4,           /* tile 68 (A/B runs): 64-wide stride-1 layers as ONE workgroup per compute unit */
    SPAA_H16P_LEAN_WIDE = 1 << 5,        /* tile 68: 64-wide N tiles (two workgroups per compute unit) for a layer wider than 64 GEMM columns */
    SPAA_H16P_POOL = 1 << 6,             /* tile 68: the layer's ReLU and the 2 x 2 / stride-2 max-pool that follows it in the epilogue (stride 1, unfolded,
                                            image-aligned regions, act = ReLU, no residual / gates, even Hout / Wout): `out` is then the POOLED tensor
                                            [B, Hout / 2, Wout / 2, out_cstride] and `mask_out` the pool's arg-max bytes [B, Hout / 2, Wout / 2, Cout] in
                                            spaa_maxpool_fwd's format (or NULL) -- torchvision VGG-16's conv -> ReLU -> MaxPool2d(2, 2), classifier.py:21-24 */
    SPAA_H16P_UNPOOL = 1 << 7,           /* tile 68: the pool-adjoint PROLOGUE of that layer's input gradient (two-workgroup form only): `in` = the gradient
                                            w.r.t. the pool's output [B, Hin / 2, Win / 2, in_cstride] fp16, `in2` = the pool's arg-max bytes [B, Hin / 2,
                                            Win / 2, in2_cstride] -- spaa_maxpool_bwd with its ReLU gate applied while the patch is staged */
    SPAA_SPLITK_FIXUP = 1 << 8,          /* Winograd tiles and tile 68's K-range form, `ksplit` > 1 (off by default): `splitk_ws` BEGINS with
                                            SPAA_SPLITK_HDR_FLOATS floats of arrival counters (int32, all zero on first use; the kernels leave them zero), the
                                            K ranges' partial sums follow: the last-arriving workgroup of a (region, N tile) adds the K ranges in fixed order
                                            and applies the epilogue inside the kernel -- the same bits as the separate second pass, one launch less.  The
                                            workspace is then SPAA_SPLITK_HDR_FLOATS + K ranges x B x H x W x Npad floats.  Clear: the two-pass form on a
                                            workspace without header */

    /* ---- reserved2 ---- */
    SPAA_X6P_STD = 1 << 0                /* tile 74: the classes' tap lists have the canonical k3 / s2 order (csrc/tapconv_x6p.hip STD: the caller has
                                            compared them; the launcher re-checks what the descriptor shows: tap counts 1 / 2 / 2 / 4, window (0..1)^2) */
};

/*
 * Generic "tap-list" convolution as an implicit GEMM on fp32 MFMA (v_mfma_f32_32x32x2_f32):
 *   out[b, oy0 + s_out*y, ox0 + s_out*x, n] = gate( act( bias[n] + add[...] +
 *        sum_{t<ntaps, c<Cin} in[b, s_in*y + dy_t, s_in*x + dx_t, c] * W[n][t*Cin + c] ) )
 * for y < Hm, x < Wm, zero padding outside the input.  One primitive covers
 *   - nn.Conv2d forward, stride 1/2            (models.py:223-252 conv*, skipConv*; torchvision convs)
 *   - nn.ConvTranspose2d forward, stride 2     (models.py:237-238; = 4 output-parity classes)
 *   - aten::convolution_backward w.r.t. input  (autograd of the above, projector_based_attack.py:302,310)
 * by the choice of taps / weight packing (spaa_amd/convplan.py).
 */
typedef struct {
    const float* in;
    int32_t Hin, Win, Cin, in_cstride, in_coff;
    float* out;
    int32_t Hout, Wout, Cout, out_cstride, out_coff;
    int32_t B, Hm, Wm, s_in, s_out;
    const float* weights; /* packed, see spaa_tapclass_t.w_off; rows padded to a multiple of 128 */
    const uint16_t* w_split; /* optional: the same weights as three bf16 planes per class, [3][Npad][Kpad] with
                                w == h + m + l exactly (the bf16x6 families: fp32 emulated on the bf16 matrix cores); class c
                                starts at element 3 * cls[c].w_off */
    const uint16_t* w_half; /* SPAA_IO_IN_F16: the weights rounded to fp16, per class [Npad][Kpad64] (Kpad64 = K rounded up to 64,
                               zero padded); class c starts at element cls[c].w_off / Kpad * Kpad64 */
    const int32_t* taps;  /* device array of (dy, dx) pairs */
    const float* bias;    /* [Cout] or NULL */
    const float* add;     /* residual, indexed like `out`, or NULL */
    int32_t add_cstride, add_coff;
    const float* gate;    /* indexed like `out`, or NULL */
    int32_t gate_cstride, gate_coff, gate_mode;
    int32_t act;
    int32_t tile;         /* 0 = auto; else an explicit kernel / workgroup tile: an id of the tile table (csrc/tiles.hpp, read through
                             spaa_tapconv_tile_info below; chosen per layer shape by tools/autotune.py).  Which tiles serve byte masks, fp16
                             storage, K ranges, folded classes, a multiplicative gate or a second source is stated there, once, as the
                             SPAA_TILE_* capability bits -- the field comments below name the bit, not the ids. */
    float* aux_out;       /* optional second output (indexed like `out`):
                             act == SPAA_ACT_RELU_CLAMP1: the value BEFORE the clamp;
                             otherwise, with gate2: (gate2 > 0) ? out_value : 0  (a second ReLU-backward gate) */
    const float* gate2;
    int32_t gate2_cstride, gate2_coff;
    uint8_t* mask_out;         /* optional ReLU-gate mask of this launch's output: one BYTE per 4 consecutive channels, bit e =
                                  (out[n0 + e] > 0), at index (o * out_cstride + out_coff + n0) >> 2 (o = output pixel).  A
                                  dgrad launch then reads 2 bits per element instead of the 32-bit activation.  Needs Cout,
                                  out_cstride, out_coff % 4 == 0 and a SPAA_TILE_BYTE_MASKS tile */
    const uint8_t* gate_bits;  /* alternative to `gate` (meaning SPAA_GATE_POS): a mask written through `mask_out` by the
                                  launch that produced the activation; indexed with gate_cstride / gate_coff */
    const uint8_t* gate2_bits; /* likewise for `gate2` (gate2_cstride / gate2_coff) */
    int32_t tap_range[4]; /* (dy_min, dy_max, dx_min, dx_max) over the taps of all classes: patch-staged kernels */
    float* splitk_ws;     /* split-K workspace, ksplit * B*Hm*Wm * Npad floats (Npad = Cout rounded up to 128), or NULL */
    int32_t ksplit;       /* 0, 1: off.
                             > 1 (the families with a second pass, one class): K is cut into `ksplit` ranges computed by separate workgroups into
                             splitk_ws; a second kernel adds them in fixed order and applies the epilogue (layers with few
                             output pixels and long K, e.g. ResNet layer4: fills the chip).
                             -1 (SPAA_TILE_PERSISTENT tiles, one class): stream-K — the K-steps of all tiles are cut into equal
                             ranges per workgroup; splitk_ws must hold 2 * 768 * 128 * 128 floats; cut tiles are summed in
                             segment order by a second kernel. */
    int32_t nfold;        /* <= 1: off.  4 (SPAA_TILE_NFOLD tiles, one class, s_out == 2, Cout % 4 == 0): the four output-parity classes of
                             a kernel-2 stride-2 ConvTranspose2d share their single tap, so they are folded into the GEMM N
                             dimension: weight rows [nfold*Cout], row c*Cout + n -> output pixel (2y + c/2, 2x + c%2),
                             channel n.  The input is read once instead of once per class. */
    int32_t reserved0;    /* per-tile form flags (the enum above), word 0: the measurement / test switches SPAA_DBG_* of every tile, SPAA_DBG_THINMF
                             of tile 72, and of a Winograd launch SPAA_WINO_PAD (set by the product: the layer's zero padding), SPAA_WINO_FORCE_CANVAS
                             and SPAA_WINO_NO_CANVAS */
    int32_t io_dtype;     /* fp16-STORAGE mode (BASELINE.json configs[4]: "fp16 with fp32 dE2000"), bit flags:
                             SPAA_IO_IN_F16  (SPAA_TILE_F16_IN tiles: the fp16 implicit-GEMM tiles; tile 68: 3x3 / stride-1 layers with the input
                                             patch staged once in LDS; tile 72: thin outputs with the parity classes folded into N, fp32 out (with a
                                             4-channel pixel stride, offset 0 and Cout < 4 its 16-byte stores write ZERO into
                                             the pad channels Cout..3; every other tile leaves channels >= Cout untouched);
                                             tile 29 with an fp32 output of at most 4 channels: the image-side input
                                             gradients): `in` is fp16 NHWC (strides / offsets still in elements) and the
                                             weights come from `w_half`; fp32 accumulation on v_mfma_f32_16x16x32_f16;
                             SPAA_IO_OUT_F16 (SPAA_TILE_F16_OUT tiles: the fp16 kernels and the kernels that read fp32 IMAGES):
                                             `out`, `add`, `gate`, `aux_out`, `gate2` are fp16.
                             0 = everything fp32 (the default path; dtype "f32" in bench.py). */
    int32_t reserved1;    /* per-tile form flags, word 1: SPAA_C3_F16_OPERANDS (tile 76), the SPAA_H16P_* forms of tile 68 and SPAA_SPLITK_FIXUP
                             (tile 68 and the Winograd tiles).  The product sets all but SPAA_H16P_CV_FORCE, SPAA_H16P_ONE_WG and SPAA_SPLITK_FIXUP */
    int32_t nclass;
    spaa_tapclass_t cls[SPAA_MAX_CLASSES];
    /* optional SECOND SOURCE (NULL = none).
     * Tile 74: a 1 x 1 convolution of a tensor at OUTPUT resolution, added to the accumulators before bias / residual / activation
     * -- `transConv1(x) + skipConv2(x1)` (models.py:293,299) and its mirror image in the backward pass as ONE launch:
     * out[b, oy, ox, n] += sum_c in2[b, oy, ox, in2_coff + c] * W2[n][c] (weights `w2_split`, Cin2 = 32 or 64).
     * Tiles 70 / 71 (Winograd): the layer's LAST Cin2 input channels (Cin2 % 32 == 0, 0 < Cin2 < Cin) are read from `in2`
     * ([B, Hin, Win, in2_cstride]) instead of `in` -- conv(a, Wa) + conv(b, Wb) as one convolution over the concatenated channels,
     * `conv5(x4) + skipConv3(x2)` (models.py:294,298); `w2_split` unused (the weights are the layer's own, K = 16 x Cin).
     * Tile 68 (fp16 storage, FOLDED stride-2 transposed layer, nfold = 4, Cout % 16 == 0, fp16 output): the same 1 x 1 convolution
     * of an fp16 tensor at output resolution; `in2` is fp16 and `w2_split` ONE fp16 matrix [Cout][Cin2] (the weights rounded to fp16
     * like `w_half`). */
    const float* in2;         /* [B, Hout, Wout, in2_cstride] */
    int32_t in2_cstride, in2_coff, Cin2;   /* Cin2 = 32 or 64 */
    int32_t reserved2;        /* per-tile form flags, word 2: SPAA_X6P_STD (tile 74; set by the product) */
    const uint16_t* w2_split; /* W2 as three bf16 planes [3][Npad][Cin2] with w == h + m + l exactly */
} spaa_tapconv_t;

int spaa_tapconv_f32(const spaa_tapconv_t* desc, spaa_stream_t stream);

/* The tile table (csrc/tiles.hpp; mirrored by spaa_amd/tiles.py, tests/test_tiles_cpu.py pins the two to each other): what a tile id is
 * and what the kernel behind it can do.  Kernel family of a tile: */
enum { SPAA_FAM_F32 = 0 /* fp32 MFMA */, SPAA_FAM_DIRECT, SPAA_FAM_THIN, SPAA_FAM_X6, SPAA_FAM_X6D, SPAA_FAM_THINPATCH, SPAA_FAM_SMALLCIN,
       SPAA_FAM_H16, SPAA_FAM_H16P, SPAA_FAM_WINO, SPAA_FAM_THINMF, SPAA_FAM_X6P, SPAA_FAM_C3 };
/* capability bits of a tile: what the descriptor may ask of it (everything else is refused before any launch) */
enum { SPAA_TILE_BYTE_MASKS = 1,        /* `mask_out` / `gate_bits` / `gate2_bits`: the epilogues built on csrc/epilogue.hpp */
       SPAA_TILE_F16_IN = 2,            /* SPAA_IO_IN_F16 */
       SPAA_TILE_F16_IN_F32_OUT = 4,    /* ... but only together with an fp32 output */
       SPAA_TILE_F16_IN_REQUIRED = 8,   /* no fp32-input form */
       SPAA_TILE_F16_OUT = 16,          /* SPAA_IO_OUT_F16 */
       SPAA_TILE_F16_OUT_KSPLIT = 32,   /* ... together with `ksplit` > 1 (never with stream-K) */
       SPAA_TILE_GATE_MUL = 64,         /* SPAA_GATE_MUL */
       SPAA_TILE_NFOLD = 128,           /* `nfold` > 1 */
       SPAA_TILE_IN2 = 256,             /* a second source `in2` */
       SPAA_TILE_IN2_OF_CIN = 512,      /* ... whose Cin2 channels are the LAST of the Cin input channels (unfolded launches) */
       SPAA_TILE_PERSISTENT = 1024 };   /* persistent workgroups: stream-K (`ksplit` == -1) capable */
typedef struct {
    int32_t id;
    int32_t family;    /* SPAA_FAM_* */
    int32_t bm, bn;    /* the workgroup's GEMM tile where the id fixes one (fp32 MFMA, x6, x6d, h16 families), else 0 */
    uint32_t caps;     /* SPAA_TILE_* */
    const char* name;  /* static storage */
} spaa_tile_info_t;
/* Host-side queries: nothing is launched.  The table entry of `tile` (0 = ok, non-zero = no such tile; the small-linear route, reported
 * as 75 by spaa_amd/convplan.py, is no tile of this dispatcher). */
int spaa_tapconv_tile_info(int tile, spaa_tile_info_t* out);
/* Every host-side check spaa_tapconv_f32 makes before it dispatches: pointers, shapes, 32-bit offset ranges and what the tile's
 * capability bits allow.  0 or hipErrorInvalidValue (1); spaa_tapconv_f32 calls it first and returns its code. */
int spaa_tapconv_check(const spaa_tapconv_t* desc);
/* Weight and bias gradients of the layer `desc` describes in its FORWARD form (same geometry / taps / packing fields;
 * `in` = the layer's input activation; `out_cstride` / `out_coff` / Hout / Wout describe `gout`, the gradient w.r.t. the
 * layer's pre-activation [B,Hout,Wout,out_cstride]); fp32 only, nfold <= 1.
 *   dw_packed [sum_c Npad*Kpad_c]: dW in the layout of `weights` (spaa_tapclass_t.w_off), pad rows / columns zero
 *   dbias [Cout] or NULL:          sum over output pixels of gout
 *   workspace: nchunk * max(sum_c Npad*Kpad_c, Cout) floats; the pixel range is cut into `nchunk` parts that are summed in
 *   a fixed order (deterministic).  Replaces aten::convolution_backward(weight, bias) in `train_loss_batch.backward()`
 *   (train_network.py:316). */
int spaa_tapconv_wgrad(const spaa_tapconv_t* desc, const float* gout, float* dw_packed, float* dbias, float* workspace,
                       int nchunk, spaa_stream_t stream);
/* Launch plan of the Winograd F(2x2,3x3) form (tiles 70 / 71; `desc` as for spaa_tapconv_f32 with a 16-position weight matrix):
 * host-side query, nothing is launched.  plan[0..7] = { N tile (64 / 128), K ranges, canvas layout (0 / 1), images per canvas
 * (rows), (columns), workgroups, 32-channel blocks per K range, canvases }.  Small images (ResNet-18 layer3 / layer4 behind
 * classifier.py:26-28, 14 x 14 and 7 x 7) are laid out on virtual canvases so that the 16 x 32-pixel workgroup regions are full,
 * and few regions with long K are cut into K ranges summed in fixed order by a second kernel: a caller sizes `splitk_ws`
 * (plan[1] * B * H * W * Npad floats) from the plan and passes plan[1] back as `ksplit` (ksplit = 1: never split; 0 with a
 * workspace: the launcher's own choice, which this function reports). */
int spaa_tapconv_wino_plan(const spaa_tapconv_t* desc, int32_t* plan);
/* The same query for the canvas / K-range form of the patch-staged fp16 kernel (tile 68 with SPAA_H16P_CV in `reserved1`: 3 x 3 / stride-1 layers of
 * the fp16-storage classifiers on 14 x 14 and 7 x 7 maps -- ResNet-18 layer3 / layer4, VGG-16's last block; classifier.py:26-28,
 * perc_al/__init__.py:181-238): plan[0..7] as above.  `desc->ksplit` > 1 asks for that many K ranges, 1 for none, 0 leaves the choice to
 * the plan; SPAA_H16P_CV_BN likewise for the N tile.  The caller passes plan[1] back as `ksplit` (with `splitk_ws` of plan[1] * B * H *
 * W * Npad floats when > 1) and plan[0] as SPAA_H16P_CV_BN. */
int spaa_tapconv_h16p_plan(const spaa_tapconv_t* desc, int32_t* plan);
/* layout probes for language bindings: sizeof(spaa_tapconv_t) and the byte offset of field # `field`
 * (0 out, 1 weights, 2 taps, 3 gate2, 4 mask_out, 5 tap_range, 6 splitk_ws, 7 io_dtype, 8 nclass, 9 cls, 10 in2, 11 w2_split; else -1) */
int spaa_tapconv_sizeof(void);
int spaa_tapconv_offsetof(int field);

/* ---- layout conversion at the NCHW boundary ---------------------------------------------------------------- */
/* src [B,3,H,W] -> dst [B,H,W,4] (lane 3 = 0); optional clamp to [0,1] (projector_based_attack.py:265) */
int spaa_nchw_to_nhwc4(const float* src, float* dst, int B, int H, int W, int clamp01, spaa_stream_t stream);
/* dst [B,3,H,W]; optional final clamp to [0,1] (projector_based_attack.py:337) */
int spaa_nhwc4_to_nchw(const float* src, float* dst, int B, int H, int W, int clamp01, spaa_stream_t stream);

/* ---- WarpingNet (models.py:163-185, pytorch_tps.py:29-106) ----------------------------------------------- */
/* Coarse grid: F.affine_grid(affine_mat) sampled at tps_grid(theta, ctrl) (models.py:168-172), batch 1.
 * out: [Hout, Wout, 4] = (gx, gy, 0, 0) in normalised [-1,1] coordinates. theta: [T+2][2], ctrl: [T][2]. */
int spaa_warp_coarse_grid(const float* affine6, const float* theta, const float* ctrl, int T, int Hin, int Win,
                          int Hout, int Wout, float* out, spaa_stream_t stream);
/* fine = clamp(refine + coarse, -1, 1) (models.py:176); all [Hout, Wout, 4] */
int spaa_warp_finish_grid(const float* coarse, const float* refine, float* fine, int npix, spaa_stream_t stream);
/* F.grid_sample(clamp(x,0,1), fine_grid, bilinear, zeros, align_corners=True) * mask (models.py:184,340), and the
 * rough input [s, xw*s] (models.py:342).  x: [B,Hp,Wp,4]; grid: [Hc,Wc,4]; mask: [Hc,Wc]; s: [B,Hc,Wc,4];
 * xw: [B,Hc,Wc,4]; cat8: [B,Hc,Wc,8] = (s.rgb, xw*s .rgb, 0, 0) or NULL. */
int spaa_warp_fwd(const float* x, const float* grid, const float* mask, const float* s, float* xw, float* cat8,
                  int B, int Hp, int Wp, int Hc, int Wc, int clamp01, spaa_stream_t stream);
/* nn.Linear on a few rows (classifier.py:60: torchvision's `fc` = ATen addmm; its input gradient = mm with the weight):
 * out[m][n] = bias[n] + sum_k x[m][k] * w[n][k], fp32, M <= 256, K <= 4096, K % 4 == 0; x / w rows 16-byte aligned (ldx, ldw % 4 == 0),
 * bias may be NULL.  The input gradient is the same call with the transposed weight. */
int spaa_linear_small(const float* x, const float* w, const float* bias, float* out, int M, int K, int N, int ldx, int ldw, int ldo,
                      spaa_stream_t stream);
/* ShadingNetSPAA's two stride-2 entry layers with use_rough in one launch (models.py:284-285,295 of the reference):
 *   S1 = relu(conv1_s(cat[s, xw * s]) + bias_s),  X1 = relu(conv1(xw) + bias1 + S1)
 * xw, s: [B,H,W,4] fp32 (channel 3 = 0), H and W even; S1, X1: [B,H/2,W/2,32] fp32 (out_f16 = 0) or fp16 (1: the residual is
 * the rounded S1); mask_S1 / mask_X1: [B,H/2,W/2,8] ReLU gate bits of the stored values (1 byte per 4 channels) or NULL.
 * w_pair: [3][32][9][4] fp32 = conv1.weight, conv1_s.weight[:, 0:3], conv1_s.weight[:, 3:6] as [n][3 ky + kx][c], c = 3 zero. */
int spaa_conv1_pair_fwd(const float* xw, const float* s, const float* w_pair, const float* bias1, const float* bias_s,
                        void* S1, void* X1, uint8_t* mask_S1, uint8_t* mask_X1, int B, int H, int W, int out_f16,
                        spaa_stream_t stream);
/* fp16-storage mode, round 6: a FRACTIONAL-STRIDE 3 x 3 layer -- nn.ConvTranspose2d(Cin, Cout, 3, 2, 1, 1) forward (models.py:237,299
 * transConv1) or aten::convolution_backward(input) of nn.Conv2d(Cout, Cin, 3, 2, 1) (conv2, conv2_s: models.py:224,230 under autograd) --
 * written per INPUT pixel: exactly the nine real (output-parity class, tap) products, all weights resident in LDS, one persistent
 * workgroup per compute unit, no barrier after the prologue (csrc/fs2_h16.hip).  in: fp16 [B,Hi,Wi,in_cstride] (channels [0,Cin), Cin % 32
 * == 0); out: fp16 [B,2 Hi,2 Wi,Cout], Cout = 32 or 64.  w_img: the weights as the kernel's matrix operands, [Cin/32][9 pairs][Cout/16][64
 * lanes][8] fp16 (spaa_amd/models.py: pack_fs2 -- pair p = (operand in[y + r][x + q], class (cy, cx)) in the order (0,0) (0,1) (0,2) (0,3)
 * (1,1) (1,3) (2,2) (2,3) (3,3) of (2 r + q, 2 cy + cx); lane = (row n & 15, chunk g): element e = W[ky][kx][16 rb + (lane & 15)][32 ks +
 * 8 g + e] with ky = (cy == 0 ? 1 : r == 0 ? 2 : 0), kx likewise).  Optional second source at OUTPUT resolution (a 1 x 1 convolution added
 * before the epilogue: models.py:293,299 `+ skipConv2(x1)` and its mirror image in the backward pass): in2 fp16 [B,2 Hi,2 Wi,in2_cstride],
 * w2_img [Cin2/32][Cout/16][64][8].  Epilogue: + bias [Cout] (fp32, may be NULL), + add (fp16 [B,2 Hi,2 Wi,Cout], may be NULL), ReLU if
 * `relu`, gate_bits (byte masks of the output's shape: out = bit ? v : 0; may be NULL), fp16 store, mask_out = gate bytes of the stored
 * values (may be NULL).  LDS: (9 Cin/32 + Cin2/32) x Cout/16 KB <= 160 KB. */
int spaa_fs2_h16(const void* in, int in_cstride, int Cin, const void* w_img, const void* in2, int in2_cstride, int Cin2,
                 const void* w2_img, const float* bias, const void* add, const uint8_t* gate_bits, int relu, void* out,
                 uint8_t* mask_out, int Cout, int B, int Hi, int Wi, spaa_stream_t stream);

/* fp16-storage mode, round 6: the FORWARD form of a 3 x 3 / stride-2 / padding-1 convolution -- nn.Conv2d(Cin, Cout, 3, 2, 1) (models.py:224,230
 * conv2 / conv2_s) or aten::convolution_backward(input) of nn.ConvTranspose2d(Cout, Cin, 3, 2, 1, 1) (transConv1, models.py:237 under autograd)
 * -- as a persistent, barrier-free kernel with all weights resident in LDS (csrc/s2f_h16.hip).  in: fp16 [B,Hi,Wi,in_cstride] (Hi, Wi even,
 * channels [0,Cin), Cin % 32 == 0); out: fp16 [B,Hi/2,Wi/2,Cout], Cout = 64 or 128.  w_img: [Cin/32][9 taps 3 ky + kx][Cout/16][64 lanes][8]
 * fp16 (spaa_amd/models.py: pack_s2f; rows permuted as for spaa_fs2_h16).  Epilogue as spaa_fs2_h16: bias, add, ReLU, gate_bits, mask_out.
 * LDS: 9 Cin/32 x Cout/16 KB <= 160 KB; every tensor below 2 GiB (32-bit buffer offsets). */
int spaa_s2f_h16(const void* in, int in_cstride, int Cin, const void* w_img, const float* bias, const void* add, const uint8_t* gate_bits,
                 int relu, void* out, uint8_t* mask_out, int Cout, int B, int Hi, int Wi, spaa_stream_t stream);

/* fp32 mode, round 6: nn.Conv2d(Cin, 64, 3, 2, 1) forward (models.py:224,230 conv2 / conv2_s) on the same persistent weights-in-LDS form
 * with the bf16x6 arithmetic of the other fp32 kernels (exact fp32 operands split into three bf16 planes, six of the nine partial products,
 * fp32 accumulation; csrc/s2f_x6.hip).  in: fp32 [B,Hi,Wi,in_cstride] (Hi, Wi even, channels [0,Cin), Cin % 32 == 0); out: fp32
 * [B,Hi/2,Wi/2,64].  w_img: [Cin/32][9 taps 3 ky + kx][3 planes][4][64 lanes][8] bf16 (spaa_amd/models.py: pack_s2f_x6).  Epilogue: bias,
 * add (fp32, the output's shape), ReLU, gate_bits, mask_out (1 byte per 4 channels), any of them NULL.  LDS: 108 Cin/32 KB <= 160 KB (Cin =
 * 32); every tensor below 2 GiB. */
int spaa_s2f_x6(const float* in, int in_cstride, int Cin, const void* w_img, const float* bias, const float* add, const uint8_t* gate_bits,
                int relu, float* out, uint8_t* mask_out, int Cout, int B, int Hi, int Wi, spaa_stream_t stream);

/* the ADJOINT of the pair in fp16-storage mode (round 6): g_xw = conv1^T(g_x1) + scene * conv1_s^T(g_s1)[rough channels 3..5]
 * (models.py:284-285,295,342 under autograd: aten::convolution_backward(input) of both layers, the product with the surface image and the
 * sum), ONE launch instead of two thin-output launches with a round trip between them.  g_x1 / g_s1: fp16 [B,H/2,W/2,32] (already
 * ReLU-gated); scene, g_xw: fp32 [B,H,W,4]; w_image: the two layers' weights rounded to fp16 as the kernel's matrix operands,
 * [2 sources][4 operands (r, q)][64 lanes][8]: lane = (row 4 (2 cy + cx) + c, 8-channel chunk g), element e = weight[n = 8 g + e][c (+ 3
 * for the rough source)][ky][kx] with ky = (cy == 0 ? 1 : r == 0 ? 2 : 0), kx likewise, zero unless c < 3, r <= cy, q <= cx
 * (spaa_amd/models.py: pack_pair1_bwd); products on v_mfma_f32_16x16x32_f16, fp32 accumulation */
int spaa_conv1_pair_bwd_f16(const void* g_x1, const void* g_s1, const float* scene, const void* w_image, float* g_xw, int B, int H, int W,
                            spaa_stream_t stream);
/* Backward of the above w.r.t. x (grid_sampler_2d_backward + clamp mask): g_x must be zeroed by the caller
 * (spaa_zero); contributions are accumulated with float atomics.
 * g_xw: [B,Hc,Wc,4] gradient w.r.t. xw (conv1 path); g_xs: [B,Hc,Wc,4] gradient w.r.t. xw*s (channels 3..5 of
 * conv1_s's input) or NULL:  g_total = (g_xw + g_xs * s) * mask. */
int spaa_warp_bwd(const float* g_xw, const float* g_xs, const float* x, const float* grid, const float* mask,
                  const float* s, float* g_x, int B, int Hp, int Wp, int Hc, int Wc, int clamp01,
                  spaa_stream_t stream);

/* Deterministic form of the same backward: the grid is constant during an attack, so the scatter is transposed once.
 * spaa_warp_taps: per (camera pixel, tap) the projector pixel index (0x7fffffff = outside) and bilinear weight,
 * src/wgt: [Hc*Wc*4].  The host sorts the entries by source pixel (stable) into `order` (entry ids) and `off`
 * ([Hp*Wp+1] list boundaries); spaa_warp_bwd_gather then sums each projector pixel's list in fixed order (no atomics,
 * no zeroing, run-to-run reproducible). */
int spaa_warp_taps(const float* grid, int Hp, int Wp, int Hc, int Wc, int32_t* src, float* wgt, spaa_stream_t stream);
int spaa_warp_bwd_gather(const float* g_xw, const float* g_xs, const float* x, const float* mask, const float* s,
                         const int32_t* off, const int32_t* order, const float* wgt, float* g_x, int B, int Hp, int Wp,
                         int Hc, int Wc, int clamp01, spaa_stream_t stream);
/* The same gather (mask folded into the weights, no second gradient) with the camera-side operand staged through LDS: a
 * workgroup owns a 16 x 16 tile of projector pixels and 4 images and reads the bounding box of the camera pixels its tap
 * lists touch once per image.  lidx / w_e: per tap-list entry (in the order of `off`) the index inside the tile's box and
 * the weight; tbox: per tile (cy0, cx0, rows, columns) of its box, at most box_cap pixels (box_cap * 64 B <= 64 KiB).
 * Built once per attack by spaa_amd/models.py: tiled_taps.  Results are bitwise those of spaa_warp_bwd_gather. */
int spaa_warp_bwd_tiled(const float* g_xw, const float* x, const int32_t* off, const int32_t* lidx, const float* w_e,
                        const int32_t* tbox, int box_cap, float* g_x, int B, int Hp, int Wp, int Hc, int Wc, int clamp01,
                        spaa_stream_t stream);
/* ... with spaa_grad_sumsq folded into its epilogue (round 6: one launch and one pass over g_x less per iteration): g_x additionally takes
 * the prjl2 term's gradient for colour-step samples (prjl2_scale != 0: `state`, `gray` as spaa_grad_sumsq), and partial_ss
 * [B][ceil(Wp/16) * ceil(Hp/16)] receives the per-(image, 16 x 16 tile) sums of ||g_x||^2 in a fixed order -- consumed by
 * spaa_step_and_track_n with npartial = that tile count.  clamp_bits (may be NULL) [B][Hp*Wp]: the clamp gate's comparisons as written by
 * spaa_step_and_track_n for THIS x (bit c: channel c inside [0, 1]): the gate then reads 1 byte per pixel instead of x's 16 (x is still
 * read when prjl2_scale != 0); the caller answers for the bytes describing the x the forward pass read */
int spaa_warp_bwd_tiled_sumsq(const float* g_xw, const float* x, const int32_t* off, const int32_t* lidx, const float* w_e,
                              const int32_t* tbox, int box_cap, float* g_x, int B, int Hp, int Wp, int Hc, int Wc, int clamp01,
                              float gray, float prjl2_scale, const int32_t* state, float* partial_ss, const uint8_t* clamp_bits,
                              spaa_stream_t stream);
/* ... with one prjl2 scale per sample: prjl2_scale float [B] on the device (0: the sample has no prjl2 term; x is read only for
 * the samples whose scale is not 0).  Same kernel; per sample bitwise the scalar launch with that sample's scale. */
int spaa_warp_bwd_tiled_sumsq_ps(const float* g_xw, const float* x, const int32_t* off, const int32_t* lidx, const float* w_e,
                                 const int32_t* tbox, int box_cap, float* g_x, int B, int Hp, int Wp, int Hc, int Wc, int clamp01,
                                 float gray, const float* prjl2_scale, const int32_t* state, float* partial_ss,
                                 const uint8_t* clamp_bits, spaa_stream_t stream);
/* F.grid_sample forward (models.py:184,340) from the per-attack TAP TABLE of spaa_warp_taps instead of the grid: tap_src [Hc*Wc][4]
 * projector pixel of every bilinear tap (0x7fffffff: outside, weight 0), tap_wgt [Hc*Wc][4] its weight x mask -- the table the
 * deterministic backward pass is built from, so the pair is an exact adjoint.  A workgroup owns a 32 x 8 tile of camera pixels and four
 * images; xw [B,Hc,Wc,4].  (spaa_warp_fwd stays for the 8-channel concatenation output and for callers without a table.) */
int spaa_warp_fwd_taps(const float* x, const int32_t* tap_src, const float* tap_wgt, float* xw, int B, int Hp, int Wp, int Hc, int Wc,
                       int clamp01, spaa_stream_t stream);

/* ---- PCNet training step: WarpingNet parameter gradients and the optimiser (train_network.py:235-363) ------- */
/* d loss / d fine_grid summed over the batch: grid_sampler_2d_backward w.r.t. the GRID (models.py:184 under autograd).
 * g_xw: gradient w.r.t. the masked warped image [B,Hc,Wc,4]; x: the sampled image [B,Hp,Wp,4]; g_grid: [Hc,Wc,4] */
int spaa_warp_bwd_grid(const float* g_xw, const float* x, const float* grid, const float* mask, float* g_grid, int B, int Hp,
                       int Wp, int Hc, int Wc, spaa_stream_t stream);
/* backward of spaa_warp_finish_grid: g_sum = gradient w.r.t. (refine + coarse) (clamp gate), g_r6 (optional) = gradient
 * w.r.t. the refine net's last pre-activation (LeakyReLU 0.1) */
int spaa_warp_finish_grid_bwd(const float* g_fine, const float* coarse, const float* refine, float* g_sum, float* g_r6,
                              int npix, spaa_stream_t stream);
/* backward of spaa_warp_coarse_grid: g_params [6 + 2 (T+2)] = (d/d affine_mat [2,3] row-major, d/d theta [(T+2),2]);
 * partial: ceil(Hout*Wout/256) * (6 + 2 (T+2)) floats of scratch (block sums, added in order) */
int spaa_warp_coarse_grid_bwd(const float* g_coarse, const float* affine6, const float* theta, const float* ctrl, int T, int Hin,
                              int Win, int Hout, int Wout, float* partial, float* g_params, spaa_stream_t stream);
/* out = gate ? sum_b g[b] + add : 0 over the first C channels of NHWC fp32 tensors with channel stride `cstride`: g [B,H,W,cstride],
 * add / out [1,H,W,cstride] (add NULL: nothing added); gate_bits [1,H,W,cstride/4] one byte per 4 channels in the mask_out / gate_bits
 * format above (NULL: no gate); C % 4 == 0, cstride % 4 == 0, C <= cstride.  b runs 0 .. B-1 in order, then add, then the gate (no
 * atomics).  The gradient of a scene-only layer run once at batch 1 from the batch-B cotangents it feeds (PCNet training). */
int spaa_batch_sum_gate_bits(const float* g, const float* add, const uint8_t* gate_bits, float* out, int B, int H, int W, int C,
                             int cstride, spaa_stream_t stream);
/* ---- CompenNet++ training step (train_network.py:130-232), csrc/compennet_train.hip ----------------------------
 * out[0] = (act[0] > 0) * sum_b g[b] over the first C channels of NHWC tensors with channel stride `cstride`: g [B,H,W,cstride],
 * act / out [1,H,W,cstride] (act NULL: no gate); C % 4 == 0, cstride % 4 == 0, C <= cstride.  The sum runs b = 0 .. B-1 in
 * order (no atomics).  The gradient of the batch-1 surface branch from the backbone gradients it feeds (models.py:74-81). */
int spaa_batch_sum_gate(const float* g, const float* act, float* out, int B, int H, int W, int C, int cstride, spaa_stream_t stream);
/* grid gradient of TWO sources sampled through one grid (no mask), written (not accumulated): g_grid [Hc,Wc,4] =
 * d/d grid of source a (g_a [B_a,Hc,Wc,4] gradient w.r.t. the warped image, x_a [B_a,Hp,Wp,4]) plus source b (g_b [B_b,Hc,Wc,4],
 * x_b [B_b,Hp,Wp,4]); Hp x Wp is the source size, Hc x Wc the grid's (models.py:204-212: camera image and scene) */
int spaa_warp_bwd_grid2(const float* g_a, const float* x_a, int B_a, const float* g_b, const float* x_b, int B_b, const float* grid,
                        float* g_grid, int Hp, int Wp, int Hc, int Wc, spaa_stream_t stream);
/* ---- fused tail / head of ShadingNetSPAA (/root/reference/src/python/models.py:296-300) --------------------------
 * forward:   Ypre = relu(conv6(relu(transConv2(X6) + bias2)) + bias6 + res1),  Y = min(Ypre, 1); the activation between
 *            the two layers (X7, 32 channels at camera resolution) stays in LDS, only its ReLU gate bytes reach HBM.
 *   x6 [B,H2,W2,64] fp32; w2_split [3][128][64] bf16: the three planes (w == h + m + l) of W[n][k] =
 *   transConv2.weight[k][c][py][px], n = 32 (2 py + px) + c; bias2 [32]; w6 [3][9][32]: w6[o][3 ky + kx][c] =
 *   conv6.weight[o][c][ky][kx]; bias6 [3]; res1, y, ypre [B,2 H2,2 W2,4]; mask7 [B,2 H2,2 W2,8] gate bytes of X7
 *   (bit e of byte q = channel 4 q + e > 0, as `mask_out` of spaa_tapconv_t).
 * backward:  P6 = gate6 . transConv2^T( gate7 . conv6^T(gP) ): gp [B,2 H2,2 W2,4] (gradient w.r.t. Ypre, channel 3
 *   ignored); w6t [27][32]: w6t[3 t + o][c] = conv6.weight[o][c][2 - t / 3][2 - t % 3]; w2t_split [3][64][128] bf16 planes
 *   of W[n][k] = transConv2.weight[n][c][py][px], k = 32 (2 py + px) + c; mask7 as above, mask6 [B,H2,W2,16] gate bytes
 *   of X6; p6 [B,H2,W2,64]. */
int spaa_shading_tail_fwd(const float* x6, const uint16_t* w2_split, const float* bias2, const float* w6, const float* bias6,
                          const float* res1, float* y, float* ypre, uint8_t* mask7, int B, int H2, int W2, spaa_stream_t stream);
int spaa_shading_head_bwd(const float* gp, const float* w6t, const uint16_t* w2t_split, const uint8_t* mask7,
                          const uint8_t* mask6, float* p6, int B, int H2, int W2, spaa_stream_t stream);
/* the same two kernels in fp16-storage mode (BASELINE.json configs[4]): x6 resp. p6 are fp16 [B,H2,W2,64]; the transposed
 * convolution's weights are ROUNDED TO fp16 like every other layer's of this mode -- here `w2_split` is ONE fp16 matrix [128][64]
 * (rows n = 32 (2 py + px) + c) and `w2t_split` ONE fp16 matrix [64][128] (same index order as the bf16 planes above) -- and its
 * products run on v_mfma_f32_16x16x32_f16 with fp32 accumulation (backward: the conv6 gradient is rounded to fp16 as that MFMA's
 * operand, the rounding the separate launches apply when they store it).  Round 5: the forward kernel keeps X7 in LDS as fp16 (the value a
 * separate transConv2 launch of this mode would store) and takes conv6's weights rounded to fp16 as well: `w6` of
 * spaa_shading_tail_fwd_f16 points at [3][9][32] fp16 ([o][3 ky + kx][c]), its taps accumulate in fp32 (v_dot2_f32_f16).  Images, res1,
 * gp and conv6's transpose (`w6t`) stay fp32 */
/* (spaa_hip 0.6: the fp16 operands are typed `const void*` -- `w2_half` / `w2t_half` ONE fp16 matrix, `w6_half` fp16 [3][9][32] -- so that a
 * caller written against the bf16-plane / fp32 meaning these arguments had before round 5 no longer compiles against this header; round 6:
 * conv6 and its transpose run on v_mfma_f32_16x16x32_f16 as well (backward: conv6's weights `w6t` fp32 [27][32] are rounded to fp16 in the
 * kernel, the values the forward pass multiplies; the cotangent enters as hi + lo fp16 halves, exact to 2^-22)) */
int spaa_shading_tail_fwd_f16(const void* x6, const void* w2_half, const float* bias2, const void* w6_half, const float* bias6,
                              const float* res1, float* y, float* ypre, uint8_t* mask7, int B, int H2, int W2, spaa_stream_t stream);
int spaa_shading_head_bwd_f16(const float* gp, const float* w6t, const void* w2t_half, const uint8_t* mask7,
                              const uint8_t* mask6, void* p6, int B, int H2, int W2, spaa_stream_t stream);

/* the backward head with spaa_select_grad folded into its first phase (one launch and one [B,H,W,4] round trip less per iteration):
 * the cotangent of sample b is g_col (state[4 b + 1] != 0: the sample takes the colour step, projector_based_attack.py:310-315)
 * or g_adv (:302-307), gated by 0 < ypre <= 1 (backward of clamp(relu(.), max = 1), models.py:301); all three [B,2 H2,2 W2,4] */
int spaa_shading_head_bwd_select(const float* g_adv, const float* g_col, const int32_t* state, const float* ypre, const float* w6t,
                                 const uint16_t* w2t_split, const uint8_t* mask7, const uint8_t* mask6, float* p6, int B, int H2,
                                 int W2, spaa_stream_t stream);
int spaa_shading_head_bwd_select_f16(const float* g_adv, const float* g_col, const int32_t* state, const float* ypre, const float* w6t,
                                     const void* w2t_half, const uint8_t* mask7, const uint8_t* mask6, void* p6, int B, int H2,
                                     int W2, spaa_stream_t stream);

/* round 6: the same kernels with the clamp gate of the network output (models.py:301: backward of clamp(relu(.), max = 1) passes where
 * 0 < pre <= 1) as ONE byte per pixel -- gate_y [B,2 H2,2 W2], bit e = channel e passes -- instead of the 16-byte pre-clamp pixel: the tail
 * writes it (`ypre` may then be NULL: 63 MB less per batch-64 pass), the select head reads it instead of `ypre` (63 MB less) */
int spaa_shading_tail_fwd_g(const float* x6, const uint16_t* w2_split, const float* bias2, const float* w6, const float* bias6,
                            const float* res1, float* y, float* ypre, uint8_t* mask7, uint8_t* gate_y, int B, int H2, int W2,
                            spaa_stream_t stream);
int spaa_shading_tail_fwd_f16_g(const void* x6, const void* w2_half, const float* bias2, const void* w6_half, const float* bias6,
                                const float* res1, float* y, float* ypre, uint8_t* mask7, uint8_t* gate_y, int B, int H2, int W2,
                                spaa_stream_t stream);
int spaa_shading_head_bwd_select_g(const float* g_adv, const float* g_col, const int32_t* state, const uint8_t* gate_y, const float* w6t,
                                   const uint16_t* w2t_split, const uint8_t* mask7, const uint8_t* mask6, float* p6, int B, int H2,
                                   int W2, spaa_stream_t stream);
int spaa_shading_head_bwd_select_f16_g(const float* g_adv, const float* g_col, const int32_t* state, const uint8_t* gate_y,
                                       const float* w6t, const void* w2t_half, const uint8_t* mask7, const uint8_t* mask6, void* p6,
                                       int B, int H2, int W2, spaa_stream_t stream);

/* ReLU backward as a stand-alone op: out = (act > 0) ? g : 0, n floats (n % 4 == 0, 16-byte aligned) */
int spaa_relu_gate(const float* g, const float* act, float* out, int64_t n, spaa_stream_t stream);
/* torch.optim.Adam step on one flat parameter tensor (train_network.py:252-254: betas (0.9, 0.999), eps 1e-8, L2 weight
 * decay added to the gradient); `step` counts from 1 */
int spaa_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, double beta1,
                   double beta2, float eps, float weight_decay, int step, spaa_stream_t stream);

/* ---- stealthiness losses (projector_based_attack.py:275-287; perc_al/differential_color_functions.py) ----- */
/* rgb [B,H,W,4] -> lab [B,H,W,4]  (rgb2lab_diff :39-64) */
int spaa_rgb2lab(const float* rgb, float* lab, int npix, spaa_stream_t stream);
/* per-pixel CIEDE2000 map (ciede2000_diff :109-180) of two Lab images -> de [npix] */
int spaa_ciede2000(const float* lab1, const float* lab2, float* de, int npix, spaa_stream_t stream);
/* autograd of the two functions above (the reference differentiates them with torch.autograd — the `_diff` in
 * their names): g_rgb = J_lab(rgb)^T g_lab;  g_lab1 = g_de * d dE/d lab1, g_lab2 = g_de * d dE/d lab2 (either may
 * be NULL).  All images [npix][4]. */
int spaa_rgb2lab_bwd(const float* rgb, const float* g_lab, float* g_rgb, int npix, spaa_stream_t stream);
int spaa_ciede2000_bwd(const float* lab1, const float* lab2, const float* g_de, float* g_lab1, float* g_lab2, int npix,
                       spaa_stream_t stream);
/* PCNet training loss (train_network.py:367-392 compute_loss; pytorch_ssim/__init__.py:26-58), forward and gradient:
 *   loss = l1_w * mean|infer - target| + ssim_w * (1 - mean SSIM(infer, target))      (means over B*3*H*W)
 * infer, target, g_infer: NHWC4 [B,H,W,4]; window: the 11x11 Gaussian [121]; m_mu / m_11 / m_12: [B,H,W,4] scratch maps
 * (needed when ssim_w != 0); partial [B * ceil(H/16) * ceil(W/16)][3] = block sums of (SSIM map, |d|, d^2): the host
 * adds them in order (loss value and the MSE the reference logs).  g_infer = d loss / d infer. */
int spaa_train_loss_fwd_bwd(const float* infer, const float* target, const float* window, float l1_w, float ssim_w,
                            float* m_mu, float* m_11, float* m_12, float* partial, float* g_infer, int B, int H, int W,
                            spaa_stream_t stream);
/* Fused camera-side stealth loss + gradient (one launch replaces ~600 ATen ops):
 *   caml2_px = ||scene - y||_2 over rgb ; camdE_px = dE00(lab(y), scene_lab)
 *   g_y      = gscale * (caml2_w * d caml2_px/dy + camdE_w * d camdE_px/dy)      gscale = 1/(B*H*W)
 * y, scene, scene_lab, g_y: [B,HW,4]; de_map: optional [B,HW] per-pixel dE; partial: [B][nblk][3] block partial
 * sums (caml2, camdE, camdE^2) with nblk = ceil(HW/256), reduced in fixed order by spaa_decide / spaa_scale_by_map. */
int spaa_stealth_loss_fwd_bwd(const float* y, const float* scene, const float* scene_lab, float caml2_w,
                              float camdE_w, float gscale, float* g_y, float* de_map, float* partial, int B, int HW,
                              spaa_stream_t stream);
/* ... with per-sample weights: caml2_w = params[b][1], camdE_w = params[b][2] of the per-sample table (see spaa_decide_ps) */
int spaa_stealth_loss_fwd_bwd_ps(const float* y, const float* scene, const float* scene_lab, const float* params,
                                 float gscale, float* g_y, float* de_map, float* partial, int B, int HW, spaa_stream_t stream);

/* calc_img_dists (utils.py:420-491) of many image pairs in one launch: for every pair, the sums over its crop
 * rectangle of the per-pixel terms of PSNR/RMSE (d^2 over the 3 channels), SSIM (pytorch_ssim/__init__.py:26-58: the
 * 11x11 Gaussian `window` [121] as create_window builds it, C1 = 0.01^2, C2 = 0.03^2, per channel, replicate padding
 * clamped to the CROP rectangle, so no pixel outside it enters a window), mean L2 (:460-471, ||d||_2), mean L_inf
 * (:475-486, max|d|) and mean dE2000 (differential_color_functions.py:183-190).
 * x and y are read as NCHW fp32 planes: side s of a pair is the [3][s_H][s_W] image at element offset s_off of its base
 * pointer, cropped to rows [s_y0, s_y0 + h) x columns [s_x0, s_x0 + w).  y_const != 0: the y side is the constant colour
 * y_rgb (no memory read; `y` may then be NULL when no pair reads it).
 * Tiles are 16x16 crop pixels; pair p owns tiles [tile0, tile0 + ceil(h/16) * ceil(w/16)), row-major over its crop;
 * tile_pair[ntiles] maps a tile to its pair.  partial[ntiles][5] = the tile's (sum d^2, sum SSIM map, sum ||d||_2,
 * sum max|d|, sum dE): fixed slots, no atomics; the caller adds a pair's tiles in order.  The host checks every
 * rectangle against its image and every offset against its buffer (32-bit plane indices, 64-bit offsets). */
typedef struct {
    int64_t x_off, y_off;
    int32_t xH, xW, xy0, xx0;
    int32_t yH, yW, yy0, yx0;
    int32_t h, w, tile0, y_const;
    float y_rgb[3];
    int32_t reserved;
} spaa_img_pair_t;   /* 80 bytes */
int spaa_img_stats(const float* x, const float* y, const spaa_img_pair_t* pairs, const int32_t* tile_pair, int ntiles,
                   const float* window, float* partial, spaa_stream_t stream);

/* ---- classifier pre/post-processing (classifier.py:55-72, img_proc.py:117-132) --------------------------- */
/* center_crop + F.interpolate(mode='area') + Normalize, NHWC4 in -> NHWC4 out; mean3/std3 are HOST pointers */
int spaa_preproc_fwd(const float* y, float* out, int B, int H, int W, int cy0, int cx0, int ch, int cw, int oh,
                     int ow, const float* mean3, const float* std3, spaa_stream_t stream);
/* adjoint: g_out [B,oh,ow,4] -> g_y [B,H,W,4] (zero outside the crop) */
int spaa_preproc_bwd(const float* g_out, float* g_y, int B, int H, int W, int cy0, int cx0, int ch, int cw,
                     int oh, int ow, const float* std3, spaa_stream_t stream);
/* max_pool2d k3 s2 p1 forward (writes per element the argmax window offset 0..8 in bits 0-6 and, in bit 7, whether the
 * maximum is positive) and backward (gather; `relu_gate` != 0: the pooled tensor's producer is a ReLU, windows whose
 * maximum is not positive pass no gradient — read from bit 7, not from the activation), NHWC, C % 4 == 0 */
int spaa_maxpool3s2_fwd(const float* in, float* out, uint8_t* argmax, int B, int Hin, int Win, int C, int Hout,
                        int Wout, spaa_stream_t stream);
int spaa_maxpool3s2_bwd(const float* g_out, const uint8_t* argmax, int relu_gate, float* g_in, int B,
                        int Hin, int Win, int C, int Hout, int Wout, spaa_stream_t stream);
/* adaptive_avg_pool2d(1): [B,HW,C] -> [B,C]; backward broadcasts g/HW and applies the ReLU gate of `act` */
int spaa_avgpool_fwd(const float* in, float* out, int B, int HW, int C, spaa_stream_t stream);
int spaa_avgpool_bwd(const float* g_out, const float* act, float* g_in, int B, int HW, int C,
                     spaa_stream_t stream);

/* Generic NHWC pooling of the VGG-16 / Inception-v3 bodies (C % 4 == 0); `*_cstride/_coff` address a channel window
 * of a concatenated buffer; backward passes are deterministic gathers with an optional ReLU gate of the input.
 * Geometry, as torch's pooling: the input covers one padded window (Hin + 2p >= k, Win + 2p >= k), 2p <= k, and
 * Hout = floor((Hin + 2p - k) / s) + 1 (likewise Wout); anything else is refused.  Max pooling takes k <= 11: the arg-max byte
 * holds the window offset ky * k + kx in bits 0-6 (at most 120) and "maximum > 0" in bit 7.  avg_pool2d takes k <= 15.
 * NaN contract: the stand-alone pool propagates a NaN of its input ("NaN wins", like ATen's max_pool2d).  Every ReLU epilogue of this
 * library is fmaxf(v, 0), which maps a NaN pre-activation to 0 -- in the separate conv + ReLU launch exactly as in the fused
 * conv + ReLU + 2 x 2 pool epilogue (spaa_tapconv_h16p, bit 6) -- so the two forms of a conv -> ReLU -> pool chain agree on every input,
 * NaN included: a NaN produced by a convolution never reaches a pool.  The library's contract is FINITE VALUES ONLY (inputs in range and
 * finite weights give finite activations); torch's relu would propagate a NaN where these epilogues clear it. */
int spaa_maxpool_fwd(const float* in, float* out, uint8_t* argmax, int B, int Hin, int Win, int C, int Hout, int Wout,
                     int k, int s, int p, int out_cstride, int out_coff, spaa_stream_t stream);
int spaa_maxpool_bwd(const float* g_out, const uint8_t* argmax, int relu_gate, float* g_in, int B, int Hin,
                     int Win, int C, int Hout, int Wout, int k, int s, int p, int gout_cstride, int gout_coff,
                     spaa_stream_t stream);
/* fp16-storage variants (activations and their gradients fp16; argmax bytes as above) */
int spaa_maxpool_fwd_f16(const void* in, void* out, uint8_t* argmax, int B, int Hin, int Win, int C, int Hout, int Wout,
                         int k, int s, int p, int out_cstride, int out_coff, spaa_stream_t stream);
int spaa_maxpool_bwd_f16(const void* g_out, const uint8_t* argmax, int relu_gate, void* g_in, int B, int Hin, int Win,
                         int C, int Hout, int Wout, int k, int s, int p, int gout_cstride, int gout_coff,
                         spaa_stream_t stream);
/* global average pool, fp16 activation in -> fp32 features out; backward fp32 feature gradient -> fp16 gradient, with the
 * ReLU gate of `act` (fp16, may be NULL) */
int spaa_avgpool_fwd_f16(const void* in, float* out, int B, int HW, int C, spaa_stream_t stream);
int spaa_avgpool_bwd_f16(const float* g_out, const void* act, void* g_in, int B, int HW, int C, spaa_stream_t stream);
/* ReLU-gate bytes (format of spaa_tapconv_t.mask_out) of channels [coff, coff + C) of an activation [M pixels][cstride] (fp32, or
 * fp16 when f16 != 0) into mask [M][cstride / 4]: for activations that no convolution launch wrote -- the max-pool outputs that
 * gate their consumers in torchvision's Inception-v3 (/root/reference/src/python/classifier.py:29-33; autograd's threshold_backward
 * of the ReLU that produced the pooled values) */
int spaa_gate_mask(const void* act, int f16, uint8_t* mask, int64_t M, int C, int cstride, int coff, spaa_stream_t stream);
/* avg_pool2d(k, s, p), count_include_pad=True */
int spaa_avgpool2d_fwd(const float* in, float* out, int B, int Hin, int Win, int C, int Hout, int Wout, int k, int s,
                       int p, int out_cstride, int out_coff, spaa_stream_t stream);
int spaa_avgpool2d_bwd(const float* g_out, float* g_in, int B, int Hin, int Win, int C, int Hout, int Wout, int k,
                       int s, int p, int gout_cstride, int gout_coff, spaa_stream_t stream);
/* fp16-storage variants (fp32 accumulation, one rounding on the way out): Inception-v3's 3x3 / stride-1 branch pools */
int spaa_avgpool2d_fwd_f16(const void* in, void* out, int B, int Hin, int Win, int C, int Hout, int Wout, int k, int s,
                           int p, int out_cstride, int out_coff, spaa_stream_t stream);
int spaa_avgpool2d_bwd_f16(const void* g_out, void* g_in, int B, int Hin, int Win, int C, int Hout, int Wout, int k,
                           int s, int p, int gout_cstride, int gout_coff, spaa_stream_t stream);
/* adaptive_avg_pool2d((Hout, Wout)) */
int spaa_adaptive_avgpool_fwd(const float* in, float* out, int B, int Hin, int Win, int C, int Hout, int Wout,
                              spaa_stream_t stream);
int spaa_adaptive_avgpool_bwd(const float* g_out, const float* gate_in, float* g_in, int B, int Hin, int Win, int C,
                              int Hout, int Wout, spaa_stream_t stream);

/* ---- Depthwise 3 x 3 / ReLU6 layers of torchvision's MobileNetV2 (csrc/dwconv.hip; spaa_amd/mobilenet.py) --------------- */
/* NHWC fp32, C % 4 == 0, B Hin Win C < 2^29 elements (every tensor below 2 GiB).  ReLU6 is torch's hardtanh(0, 6): the value is
 * min(max(v, 0), 6), the gradient passes where 0 < v < 6, strictly on both sides.  Gate bytes have the format of
 * spaa_tapconv_t.mask_out (one byte per 4 consecutive channels, bit e = channel 4 q + e passes), so a convolution's input-gradient
 * launch takes them through `gate_bits` unchanged.  The clamp is fminf(fmaxf(v, 0), 6) like every ReLU epilogue of this library: a NaN
 * becomes 0 with its gate bit clear (FINITE VALUES ONLY, see the pooling section above).  Invalid arguments (a null pointer other
 * than the optional ones named below, C % 4 != 0, a stride other than 1 or 2, a size < 1 or over the limit) return
 * hipErrorInvalidValue with nothing launched and nothing written.
 *
 * spaa_dwconv3_fwd: depthwise 3 x 3, padding 1, stride 1 or 2: in [B, Hin, Win, C] -> out [B, Hout, Wout, C], Hout = (Hin - 1) / stride
 * + 1 (likewise Wout).  w [9][C] tap-major (tap = 3 ky + kx) with the BatchNorm folded in, bias [C].  in_relu6 != 0: `in` is a
 * pre-activation and is clamped to [0, 6] as it is loaded (the ReLU6 of the layer before, which that launch then does not apply).  The
 * accumulation order is fixed: acc = bias, then acc = fmaf(w, v, acc) over (ky, kx) in row-major order, taps outside the image skipped.
 * The output is always ReLU6'd; mask_out [B, Hout, Wout, C / 4] (may be NULL) receives bit = (0 < acc < 6).
 * spaa_dwconv3_bwd: its exact adjoint as a gather (no atomics; two runs are bitwise equal): g_in[y, x, c] = gate6(in_pre[y, x, c]) *
 * sum over the taps (ky, kx), row-major, that reach an output pixel, of w[ky, kx, c] g_out[oy, ox, c] (acc = 0, then fmaf).  in_pre
 * [B, Hin, Win, C]: the pre-activation the forward pass clamped on load (NULL: no gate).  g_out must arrive gated by the forward
 * pass's mask_out (the projection's input-gradient launch does that through gate_bits). */
int spaa_dwconv3_fwd(const float* in, int in_relu6, const float* w, const float* bias, float* out, uint8_t* mask_out, int B, int Hin,
                     int Win, int C, int stride, spaa_stream_t stream);
int spaa_dwconv3_bwd(const float* g_out, const float* w, const float* in_pre, float* g_in, int B, int Hin, int Win, int C, int stride,
                     spaa_stream_t stream);
/* In-place ReLU6 of act [M pixels][C], writing its gate bytes mask_out [M][C / 4] (may be NULL: a pass nobody differentiates):
 * MobileNetV2's features.18, whose clamped output is also the feature map Grad-CAM reads. */
int spaa_relu6_gate(float* act, uint8_t* mask_out, int64_t M, int C, spaa_stream_t stream);
/* adaptive_avg_pool2d(1) backward under a ReLU6 gate: g_in[b, p, c] = bit(mask[b, p, c / 4], c % 4) ? g_feat[b, c] / HW : 0
 * (spaa_avgpool_bwd gates on act > 0 only, which is wrong at 6). */
int spaa_global_avgpool_bwd_bits(const float* g_feat, const uint8_t* mask, float* g_in, int B, int HW, int C, spaa_stream_t stream);

/* ---- torchvision vit_b_16 (csrc/vit_ops.hip; spaa_amd/vit.py) ------------------------------------- */
/* fp32 throughout, exact-fp32 VALU arithmetic, no atomics and a fixed accumulation order (two runs are bitwise equal), no allocation
 * and no synchronisation.  Invalid arguments (a null pointer other than the optional `add`, a row length D or head width dh that is no
 * multiple of 4, dh > 64, T > 256, a size < 1, a tensor of 2^29 elements or more) return hipErrorInvalidValue with nothing launched and
 * nothing written.  Every pointer is 16-byte aligned and every row stride a multiple of 4 floats.
 *
 * spaa_vit_patchify: img [B, h, w, 4] -> patches [B n, 4 P P], n = (h / P)(w / P) tokens in row-major order of the patch grid, column
 * (ky P + kx) 4 + c (h % P == w % P == 0): a P x P / stride P convolution becomes a 1 x 1 plan over K = 4 P P whose weight the host
 * rearranges (zeros for c = 3).  spaa_vit_unpatchify: the adjoint, g_img[b, y, x] = g_patches[token, column]: one value per pixel.
 * spaa_vit_assemble: x [B, T, D], T = n + 1 >= 2: row 0 = class_token [D] + pos[0], row 1 + i = emb [B, n, D] row i + pos [T, D] row
 * 1 + i.  spaa_vit_assemble_bwd: g_emb[b, i] = g_x[b, 1 + i]. */
int spaa_vit_patchify(const float* img, float* patches, int B, int h, int w, int P, spaa_stream_t stream);
int spaa_vit_unpatchify(const float* g_patches, float* g_img, int B, int h, int w, int P, spaa_stream_t stream);
int spaa_vit_assemble(const float* emb, const float* class_token, const float* pos, float* x, int B, int T, int D, spaa_stream_t stream);
int spaa_vit_assemble_bwd(const float* g_x, float* g_emb, int B, int T, int D, spaa_stream_t stream);
/* LayerNorm over `rows` rows of D floats, row r of a tensor at r * its stride (stride >= D floats: the head normalises only the
 * class-token rows of [B, T, D] with stride T D).  Forward: mean first, then the biased variance as the mean of the centred squares;
 * y = (x - mean) rstd gamma + beta, rstd = 1 / sqrt(var + eps); mean [rows] and rstd [rows] are written for the adjoint.
 * Backward: gx = rstd (gh - mean(gh) - xh mean(gh xh)) (+ add where add != NULL: a residual gradient at no extra pass), gh = g gamma,
 * xh = (x - mean) rstd.  gx may be `g` or `add` itself (a lane reads what it writes before it writes). */
int spaa_layernorm_fwd(const float* x, int64_t x_stride, const float* gamma, const float* beta, float* y, int64_t y_stride, float* mean,
                       float* rstd, int rows, int D, float eps, spaa_stream_t stream);
int spaa_layernorm_bwd(const float* g, int64_t g_stride, const float* x, int64_t x_stride, const float* gamma, const float* mean,
                       const float* rstd, const float* add, int64_t add_stride, float* gx, int64_t gx_stride, int rows, int D,
                       spaa_stream_t stream);
/* Exact GELU x Phi(x) over n floats (n % 4 == 0), Phi(x) = erfc(-x / sqrt 2) / 2; the adjoint is g (Phi(pre) + pre phi(pre)) with the
 * PRE-activation the forward pass read (kept by the caller).  act may be pre, gx may be g (elementwise). */
int spaa_gelu_fwd(const float* pre, float* act, int64_t n, spaa_stream_t stream);
int spaa_gelu_bwd(const float* g, const float* pre, float* gx, int64_t n, spaa_stream_t stream);
/* Multi-head softmax attention.  qkv [B, T, 3 D], D = heads dh: columns [0, D) the queries, [D, 2 D) the keys, [2 D, 3 D) the values,
 * head h at columns h dh .. (h + 1) dh of each (torch.nn.MultiheadAttention's in_proj order).  ctx [B, T, D] (heads concatenated in
 * order) = softmax_j(q_i . k_j / sqrt(dh)) v_j with the row maximum subtracted; lse [B, heads, T] = max + log(sum) is kept instead of
 * the probabilities, which the adjoint recomputes as exp(s - lse).
 * spaa_attn_bwd: g_qkv [B, T, 3 D] from g_ctx [B, T, D] in two launches: a query-parallel pass writes delta [B, heads, T] (a workspace
 * of the caller's: delta_i = g_ctx_i . ctx_i) and g_q, a key-parallel pass g_k and g_v; every element of g_qkv is written. */
int spaa_attn_fwd(const float* qkv, float* ctx, float* lse, int B, int T, int heads, int dh, spaa_stream_t stream);
int spaa_attn_bwd(const float* qkv, const float* ctx, const float* lse, const float* g_ctx, float* g_qkv, float* delta, int B, int T,
                  int heads, int dh, spaa_stream_t stream);
/* Gradient-weighted attention rollout (Chefer, Gur and Wolf 2021): the class token's row rho [B, T] of
 * R = (I + A_L) ... (I + A_1), A_l = mean over the heads of max(0, P_h * dP_h / seed), pushed down one layer per call while the backward
 * pass visits that layer: P_h = exp(q k^T / sqrt(dh) - lse) and dP_h = g_ctx v^T are recomputed from what spaa_attn_bwd reads, and
 * seed = g_logits[b][target[b]] (read on the device; g_logits [B, ncls], target int32 [B]) turns the loop's cotangent into the class
 * logit's gradient.
 * spaa_attn_relevance: rho_out[j] = rho_in[j] + (1 / heads) sum_h sum_i rho_in[i] max(0, P_h[i][j] dP_h[i][j] / seed), the same
 * admissible shapes as the attention entry points.  rho_in == NULL stands for e_cls (the top layer; only query row 0 is read) and gives
 * bitwise what an explicit e_cls gives; rho_out may be rho_in.  head_ws [B, heads, T] is a workspace of the caller's, written whole.
 * Two launches; per head the queries are summed per lane in index order and then over the wave, the heads in index order, the mean
 * is one division.  A sample whose seed is 0 or whose target is no class in [0, ncls) keeps rho_out = rho_in.
 * spaa_relevance_map: c [B, T - 1] = max(0, rho[1:]) and cmax [B] = its maximum, both 0 for a sample without a seed: what spaa_cam_map
 * leaves for spaa_attention_apply, with fh x fw the patch grid.  T >= 2. */
int spaa_attn_relevance(const float* qkv, const float* lse, const float* g_ctx, const float* rho_in, const float* g_logits, int ncls,
                        const int32_t* target, float* head_ws, float* rho_out, int B, int T, int heads, int dh, spaa_stream_t stream);
int spaa_relevance_map(const float* rho, const float* g_logits, int ncls, const int32_t* target, float* c, float* cmax, int B, int T,
                       spaa_stream_t stream);

/* ---- Depthwise 7 x 7 layers of torchvision's ConvNeXt (csrc/convnext_ops.hip; spaa_amd/convnext.py) -------------- */
/* NHWC fp32, stride 1, zero padding 3 (the output has the size of the input), any H, W >= 1.  w [49][C] tap-major (tap = 7 ky + kx),
 * the convention of spaa_dwconv3_*.  Exact-fp32 VALU arithmetic in a fixed order, no atomics (two runs are bitwise equal), no
 * allocation and no synchronisation.  Invalid arguments (a null pointer other than `add`, C % 4 != 0, a size < 1, B H W C >= 2^29)
 * return hipErrorInvalidValue with nothing launched and nothing written.
 * spaa_dwconv7_fwd: out[y, x, c] = bias[c] + sum w[ky, kx, c] in[y - 3 + ky, x - 3 + kx, c]: acc = bias, then acc = fmaf(w, v, acc)
 * over (ky, kx) in row-major order; a tap outside the image contributes nothing (a column outside it is multiplied as a 0, which for
 * finite weights leaves acc as it is: FINITE VALUES ONLY).
 * spaa_dwconv7_bwd: its exact adjoint as a gather: g_in[y, x, c] = add[y, x, c] + sum over the taps (ky, kx), row-major, that reach an
 * output pixel, of w[ky, kx, c] g_out[y + 3 - ky, x + 3 - kx, c] (acc = 0, then fmaf; `add`, which may be NULL, is added last: the
 * residual gradient of a ConvNeXt block at no extra pass).  g_in may be `add` itself (a lane reads what it writes before it writes),
 * not g_out. */
int spaa_dwconv7_fwd(const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int C, spaa_stream_t stream);
int spaa_dwconv7_bwd(const float* g_out, const float* w, const float* add, float* g_in, int B, int H, int W, int C,
                     spaa_stream_t stream);
/* Measurement and test switch (host side, no stream, nothing launched): which of the kernel's two forms the two entry points above
 * launch from now on -- 0 the library's own choice by shape (the default), 1 strips of 4 columns and runs of at least 7 rows, 2 strips
 * of 2 columns and runs of at least 4 rows.  Both forms accumulate in the same order: their outputs are bitwise equal.  Returns the
 * value before the call; any other argument changes nothing. */
int spaa_dwconv7_form(int form);

/* ---- SPAA Algorithm 1 control on device (projector_based_attack.py:269-328) ------------------------------ */
/* Per-sample decision, one workgroup per sample: softmax top-1 / argmax of logits (classifier.py:64-68), loss
 * reduction, masks (:290-299), best bookkeeping (:318-320), and the seed of the adversarial backward pass
 * g_logits[b][c] = (c == target_b) ? -/+adv_scale : 0  (adv_scale = adv_w / B).
 * state (int32 [B][4]): 0 succ, 1 best_adv, 2 best, 3 top1.   stats (float [B][8]): 0 p1, 1 caml2, 2 camdE,
 * 3 col_loss, 4 prjl2, 5 col_loss_best (in/out, init 1e6), 6 target logit, 7 reserved.  prjl2 may be NULL. */
int spaa_decide(const float* logits, int ncls, const int32_t* target, int targeted, const float* partial, int nblk,
                int HW, const float* prjl2, float prjl2_w, float caml2_w, float camdE_w, float d_thr,
                float p_thresh, float adv_scale, int32_t* state, float* stats, float* g_logits, int B,
                spaa_stream_t stream);
/* Per-sample attack parameters (one batch = several attack configurations, spaa_sweep).  The _ps entry points launch the SAME
 * kernels as their scalar forms with the scalars read per sample from a device table:
 *   params float [B][4] = (prjl2_w, caml2_w, camdE_w, d_thr)      flags int32 [B]: bit 0 = targeted
 * p_thresh and adv_scale stay scalars.  prjl2 may be NULL; a sample with prjl2_w == 0 reads it as 0 (stats[b][4] = 0), as the
 * scalar launch does when its caller passes prjl2 = NULL.  With every sample's parameters equal to the scalars, the outputs are
 * bitwise those of the scalar launch; with mixed parameters, each sample's are bitwise those of the scalar launch on that sample. */
int spaa_decide_ps(const float* logits, int ncls, const int32_t* target, const float* partial, int nblk, int HW,
                   const float* prjl2, const float* params, const int32_t* flags, float p_thresh, float adv_scale,
                   int32_t* state, float* stats, float* g_logits, int B, spaa_stream_t stream);
/* Cotangent at the PCNet output: g = best_adv_b ? g_col : g_adv (one backward pass serves both of the reference's,
 * :302,310), then the backward of clamp(relu(pre), max=1) (models.py:301): pass where 0 < ypre <= 1 (ypre NULL: none).
 * all [B,npix,4] */
int spaa_select_grad(const float* g_adv, const float* g_col, const int32_t* state, const float* ypre, float* g,
                     int B, int npix, spaa_stream_t stream);
/* prjl2_b = mean_px ||gray - x||_2 (:275) */
int spaa_prjl2_fwd(const float* x, float gray, float* prjl2, int B, int HW, spaa_stream_t stream);
/* In place g += prjl2_scale * d prjl2_px/dx for colour-step samples (prjl2_scale = prjl2_w/(B*HW), 0 = off), and
 * block partials of ||g_b||^2 -> partial [B][ceil(HW/256)] */
int spaa_grad_sumsq(float* g, const float* x, float gray, float prjl2_scale, const int32_t* state, float* partial,
                    int B, int HW, spaa_stream_t stream);
/* ... with prjl2_scale float [B] on the device, one per sample (0: no prjl2 term) */
int spaa_grad_sumsq_ps(float* g, const float* x, float gray, const float* prjl2_scale, const int32_t* state, float* partial,
                       int B, int HW, spaa_stream_t stream);
/* x_b -= lr_b * g_b/||g_b||_2 with lr = best_adv ? col_lr : adv_lr (:307,315); then where succ: x_best_b = x_b
 * (post-step, Q4) and cam_best_b = cam_b (:323-328).   x, g, x_best: [B,HWp,4]; cam, cam_best: [B,HWc,4] */
int spaa_step_and_track(float* x, const float* g, const float* partial, const int32_t* state, float adv_lr,
                        float col_lr, float* x_best, const float* cam, float* cam_best, int B, int HWp, int HWc,
                        spaa_stream_t stream);
/* the same with the number of partial sums per sample stated (partial [B][npartial]: spaa_warp_bwd_tiled_sumsq's tile sums);
 * clamp_bits (may be NULL) [B][HWp]: receives, per pixel of the UPDATED x, bit c = (0 <= x_c <= 1) -- the clamp gate of the next
 * iteration's backward pass (models.py:337 `x.clamp(0, 1)` under autograd) */
int spaa_step_and_track_n(float* x, const float* g, const float* partial, int npartial, const int32_t* state, float adv_lr,
                          float col_lr, float* x_best, const float* cam, float* cam_best, int B, int HWp, int HWc,
                          uint8_t* clamp_bits, spaa_stream_t stream);

/* ---- ensemble SPAA: one projection against K classifiers on the same camera image, 2 <= K <= SPAA_ENS_MAX ----------------- */
#define SPAA_ENS_MAX 4
/* Member tensors are passed as HOST arrays of K device pointers (copied into the launch's arguments: no device pointer table).
 * Any other K is hipErrorInvalidValue and nothing is launched.
 *
 * The decision over K members' logits ([B][ncls] each), per-sample table form only (params, flags as spaa_decide_ps).  Member k of
 * sample b: top1, p1 and the target logit by the arithmetic of spaa_decide; succ = (top1 == target) if targeted else (top1 != target);
 * fooled = succ && p1 > p_thresh if targeted else succ.  Outputs:
 *   state [B][4]: 0 every member succ, 1 best_adv = every member fooled && caml2 * 255 > d_thr, 2 best, 3 number of fooled members
 *   stats [B][8]: 0 min over members of p1, 6 mean over members of the target logit, 1..5 as spaa_decide
 *   ens_state int32 [B][K][2] = (bit 0 succ | bit 1 fooled, top1)    ens_stats float [B][K][2] = (p1, target logit)
 *   ens_w float [B][K]: the member weights of spaa_ens_combine -- 1, or with focus != 0: 0 for a fooled member unless all are fooled
 *   g_logits: K seeds [B][ncls], (c == target_b) ? -1 (targeted) / +1 : 0 */
int spaa_decide_ens(const float* const* logits, int K, int ncls, const int32_t* target, const float* partial, int nblk, int HW,
                    const float* prjl2, const float* params, const int32_t* flags, float p_thresh, int focus, int32_t* state,
                    float* stats, int32_t* ens_state, float* ens_stats, float* ens_w, float* const* g_logits, int B,
                    spaa_stream_t stream);
/* 256-pixel block partials of the K gradient images' squared norms over the colour channels (g[k]: [B][HW][4], the pad channel is
 * ignored) -> partial [B][K][ceil(HW / 256)] */
int spaa_ens_sumsq(const float* const* g, int K, float* partial, int B, int HW, spaa_stream_t stream);
/* g_adv_b = sum over k in index order of ens_w[b][k] * g_bk / ||g_bk||_2 in fp32; a member with zero norm contributes 0; the pad
 * channel of g_adv [B][HW][4] is 0.  partial from spaa_ens_sumsq with nblk = ceil(HW / 256); run-to-run bitwise reproducible */
int spaa_ens_combine(const float* const* g, int K, const float* partial, int nblk, const float* ens_w, float* g_adv, int B, int HW,
                     spaa_stream_t stream);

/* ---- multi-view SPAA: one projection against V camera views of the same projector and scene, 2 <= V <= SPAA_VIEWS_MAX ------- */
#define SPAA_VIEWS_MAX 4
/* Per-view tensors are passed as HOST arrays of V device pointers, as the ensemble's member tensors.  Any other V is
 * hipErrorInvalidValue and nothing is launched.
 *
 * The decision over V views: view v has its own logits [B][ncls] (one classifier looking at camera image v) and its own stealth-loss
 * block partials [B][nblk][3] (spaa_stealth_loss_fwd_bwd_ps on camera image v).  Per-sample table form only (params, flags, adv_scale
 * as spaa_decide_ps).  View v of sample b: top1, p1, the target logit and the means caml2_v, camdE_v by the arithmetic of spaa_decide;
 * succ and fooled as in spaa_decide_ens.  Sample: caml2 = (sum over v in index order of caml2_v) / V, camdE likewise, col_loss =
 * prjl2_w prjl2 + caml2_w caml2 + camdE_w camdE.  Outputs:
 *   state [B][4]: 0 every view succ, 1 best_adv = every view fooled && caml2 * 255 > d_thr, 2 best, 3 number of fooled views
 *   stats [B][8]: 0 min over views of p1, 6 mean over views of the target logit, 1..5 as spaa_decide on the sample's values
 *   view_state int32 [B][V][2] = (bit 0 succ | bit 1 fooled, top1)    view_stats float [B][V][4] = (p1, target logit, caml2_v, camdE_v)
 *   view_w float [B][V]: the view weights of spaa_views_combine -- 1, or with focus != 0: 0 for a fooled view unless all are fooled
 *   g_logits: V seeds [B][ncls], (c == target_b) ? -adv_scale (targeted) / +adv_scale : 0
 * With V identical views (V a power of two) state[.][0..2], stats[.][1..5] and the seeds are bitwise those of spaa_decide_ps.
 * spaa_decide_ens is the same kernel with one loss table for all members: given that table V times (V a power of two) and
 * adv_scale = 1, state, stats, the weights, the seeds, view_state and view_stats[..][0..1] are bitwise spaa_decide_ens's. */
int spaa_decide_views(const float* const* logits, int V, int ncls, const int32_t* target, const float* const* partial, int nblk, int HW,
                      const float* prjl2, const float* params, const int32_t* flags, float p_thresh, float adv_scale, int focus,
                      int32_t* state, float* stats, int32_t* view_state, float* view_stats, float* view_w, float* const* g_logits,
                      int B, spaa_stream_t stream);
/* The V views' input gradients at the projector image, g[v]: [B][HW][4], as one: for a colour-step sample (state[b][1] != 0)
 * g_out_b = (sum over v in index order of g_bv) * (1 / V), the gradient of the mean of the views' stealth losses, not normalised (the
 * prjl2 term that spaa_grad_sumsq adds afterwards keeps its scale); for every other sample g_out_b = sum over v in index order of
 * view_w[b][v] * g_bv / ||g_bv||_2, a view with zero norm contributing 0.  The pad channel of g_out [B][HW][4] is 0.  partial
 * [B][V][nblk] from spaa_ens_sumsq with the same HW, nblk = ceil(HW / 256); run-to-run bitwise reproducible.  Where no sample is on
 * the colour step, g_out is bitwise spaa_ens_combine's (one kernel) */
int spaa_views_combine(const float* const* g, int V, const float* partial, int nblk, const float* view_w, const int32_t* state,
                       float* g_out, int B, int HW, spaa_stream_t stream);
/* cam_best[v]_b = cam[v]_b where state[b][0] != 0 (succ), for the views v = 1 .. V-1 in one launch: what spaa_step_and_track_n does
 * for the one camera image it is given (view 0's).  cam, cam_best: V pointers each to [B][HW][4]; entry 0 is not read */
int spaa_views_track(const float* const* cam, float* const* cam_best, int V, const int32_t* state, int B, int HW, spaa_stream_t stream);

/* ---- universal SPAA: one projection for a group of N scenes, 2 <= N <= SPAA_UNIVERSAL_MAX ------------------------------------- */
#define SPAA_UNIVERSAL_MAX 64
/* A batch of B samples is U = B / N groups; group u is the samples uN .. uN+N-1, whose N rows hold the same projector image and whose
 * parameters (params, flags) are uniform.  The members are rows of the ordinary [B][...] tensors: no pointer arrays.  Both entry points
 * return hipErrorInvalidValue and launch nothing on a null pointer (prjl2 alone may be NULL), N outside 2..SPAA_UNIVERSAL_MAX,
 * B % N != 0, B > 65535 or HW < 1; the decision also on need outside 1..N and nblk != ceil(HW / 256).
 *
 * The decision (logits, target, partial, nblk, HW, prjl2, params, flags, p_thresh, adv_scale as spaa_decide_ps).  Member b, by the
 * arithmetic of spaa_decide_ps on sample b alone (bitwise): top1, p1, the target logit, succ, fooled, its own means caml2_b, camdE_b and
 * its seed row g_logits[b].  Group: nsucc, nfooled; caml2 = (sum over members in index order of caml2_b) / N, camdE likewise; prjl2 is
 * member 0's; col_loss = prjl2_w prjl2 + caml2_w caml2 + camdE_w camdE.  Outputs, the group's words in EACH of its N rows:
 *   state [B][4]: 0 nsucc >= need, 1 best_adv = nfooled >= need && caml2 * 255 > d_thr, 2 best, 3 nfooled
 *   stats [B][8]: 0 min over members of p1, 6 mean over members of the target logit, 1..5 as spaa_decide on the group's values
 *   uni_state int32 [B][2] = (bit 0 succ | bit 1 fooled, top1)    uni_stats float [B][4] = (p1, target logit, caml2_b, camdE_b)
 *   uni_w float [B]: the member weights of spaa_universal_combine -- 1, or with focus != 0: 0 for a fooled member unless
 *   nfooled >= need
 * With need == N this is spaa_decide_views with members in the place of views. */
int spaa_decide_universal(const float* logits, int ncls, const int32_t* target, const float* partial, int nblk, int HW, const float* prjl2,
                          const float* params, const int32_t* flags, int N, int need, float p_thresh, float adv_scale, int focus,
                          int32_t* state, float* stats, int32_t* uni_state, float* uni_stats, float* uni_w, float* g_logits, int B,
                          spaa_stream_t stream);
/* The B per-sample gradient images at the projector, g [B][HW][4], combined group by group into g_out [B][HW][4] (another buffer), the
 * result in all N rows of the group, its pad channel 0: for a group on the colour step (state[uN][1] != 0) (sum over members in index
 * order of g_b) * (1 / N); for any other the sum over members in index order of coef_b g_b with coef_b = uni_w_b / ||g_b||_2, and 0
 * where the norm or the weight is 0.  Workspaces: partial float [B][ceil(HW / 256)] (block partials of ||g_b||^2) and coef float [B].
 * Run-to-run bitwise reproducible */
int spaa_universal_combine(const float* g, int N, const float* uni_w, const int32_t* state, float* partial, float* coef, float* g_out,
                           int B, int HW, spaa_stream_t stream);

/* ---- capture-robust SPAA: one projection against J randomly jittered captures of the camera image, 2 <= J <= SPAA_JITTER_MAX -- */
#define SPAA_JITTER_MAX 4
/* Per-draw tensors are passed as HOST arrays of J device pointers, as the ensemble's member tensors.  Any other J, or a null
 * pointer, is hipErrorInvalidValue and nothing is launched.  Images are [B][H*W][4] fp32.
 *
 * The parameter rows of iteration t = counter[0] (device memory; t + 1 is stored after every thread of the one workgroup has read
 * it, so a replayed graph advances the sequence without the host):
 *   jit [B][J][8] = (gain_r, gain_g, gain_b, offset, dx, dy, sigma, 0) with gain_c = 1 + gain (2u - 1), offset (2u - 1),
 *   dx, dy = shift (2u - 1) in camera pixels, sigma = noise;  key [B][J]: the draw's 32-bit noise key.
 * Each u = (h >> 8) 2^-24 with h a pure function of (seed, t, b, j, column) by 32-bit integer mixing ("Capture-robust
 * attack"; the key is column 7).  clean0 != 0: draw 0 of every sample is the identity row (1, 1, 1, 0, 0, 0, 0, 0). */
int spaa_jitter_draw(uint32_t seed, int32_t* counter, float gain, float offset, float shift, float noise, int clean0, float* jit,
                     uint32_t* key, int B, int J, spaa_stream_t stream);
/* out[j] = clamp(pre, 0, 1), pre_c = gain_c S(y)_c + offset + sigma n_c, then with quantize != 0 floorf(out 255.f) / 255.f (the
 * camera's 8-bit step); the pad channel of out is 0.  S: the bilinear translation by (dx, dy) with replicate border, per axis
 * out[m] = (1 - f) in[clamp(m + k)] + f in[clamp(m + k + 1)], k = floor(d), f = d - k.  n: standard normal by Box-Muller from two
 * uniforms of (key[b][j], pixel, c), none when sigma == 0.  gate[j] [B][H*W] bytes: bit c = (0 <= pre_c <= 1).  One launch. */
int spaa_jitter_fwd(const float* y, const float* jit, const uint32_t* key, int J, int quantize, float* const* out,
                    uint8_t* const* gate, int B, int H, int W, spaa_stream_t stream);
/* The adjoint: g_y[j] = S^T(gain_c gate_c g_out[j]) (the quantisation straight-through, no gradient of the noise) as a gather
 * without atomics: run-to-run bitwise reproducible.  The pad channel of g_y is 0.  One launch. */
int spaa_jitter_bwd(const float* const* g_out, const float* jit, const uint8_t* const* gate, int J, float* const* g_y, int B, int H,
                    int W, spaa_stream_t stream);
/* spaa_jitter_fwd with an input image of its own per draw: out[j] and gate[j] from y[j] (J device pointers in a host array), by the
 * same arithmetic; with J equal pointers the results are spaa_jitter_fwd's bit for bit.  One launch. */
int spaa_jitter_fwd_each(const float* const* y, const float* jit, const uint32_t* key, int J, int quantize, float* const* out,
                         uint8_t* const* gate, int B, int H, int W, spaa_stream_t stream);

/* ---- pose-robust SPAA: one projection against J randomly warped copies of the camera image, 2 <= J <= SPAA_JITTER_MAX
 * Conventions of the capture jitter above: host arrays of J device pointers, any other J / a null pointer / a size < 1 is
 * hipErrorInvalidValue with nothing launched, images [B][H*W][4] fp32, no allocation, no sync, no atomics.
 *
 * A table row h[b][j][0..7] is the homography [[h0, h1, h2], [h3, h4, h5], [h6, h7, 1]] in centred pixel coordinates: output pixel
 * (row, col) has u = col + 0.5 - W/2, v = row + 0.5 - H/2 and reads the source position, evaluated in fp32 in this order,
 *   w = fmaf(h6, u, fmaf(h7, v, 1)),  xs = fmaf(h0, u, fmaf(h1, v, h2)) / w + (W/2 - 0.5),  ys = fmaf(h3, u, fmaf(h4, v, h5)) / w + (H/2 - 0.5).
 *
 * spaa_pose_draw: the rows of iteration t = counter[0] (device memory; t + 1 is stored after every thread of the one workgroup has
 * read it): h = (s cos a, -s sin a, tx, s sin a, s cos a, ty, px / R, py / R), R = max(H, W) / 2, a = rotate (2u0 - 1) pi / 180,
 * s = 1 + zoom (2u1 - 1), tx, ty = shift (2u2 - 1), shift (2u3 - 1), px, py = tilt (2u4 - 1), tilt (2u5 - 1); the u_i are
 * spaa_jitter_draw's uniforms of (seed, t, b, j, i) with the first constant 0x85ebca6b in place of 0x9e3779b9.  clean0 != 0: draw 0
 * of every sample is the identity row (1, 0, 0, 0, 1, 0, 0, 0).  table: [B][J][8]. */
int spaa_pose_draw(uint32_t seed, int32_t* counter, float rotate, float zoom, float shift, float tilt, int clean0, float* table, int B,
                   int J, int H, int W, spaa_stream_t stream);
/* out[j] = the bilinear sample of y at (xs, ys), taps outside the image contributing 0 (torch's grid_sample, bilinear, zeros,
 * align_corners = False); the pad channel of out is 0.  The identity row copies the colour channels of y bit for bit.  One launch. */
int spaa_pose_fwd(const float* y, const float* table, int J, float* const* out, int B, int H, int W, spaa_stream_t stream);
/* The exact adjoint as a gather: input pixel p sums g_out[j][m] w_m(p) over the output pixels m within 2 of round(H^-1 p) (a 5 x 5
 * window, in row-major order), w_m(p) the forward's own weight of tap p at m recomputed by the identical fp32 expression.  The
 * window holds every contribution while the row stays within 10 degrees, zoom 0.15 and tilt 0.1 (what spaa_pose_draw is given by
 * PoseJitter); beyond them contributions are lost.  Run-to-run bitwise reproducible; the pad channel of g_y is 0.  One launch. */
int spaa_pose_bwd(const float* const* g_out, const float* table, int J, float* const* g_y, int B, int H, int W, spaa_stream_t stream);

/* ---- JPEG-robust SPAA: one projection against J codec round trips of the camera image, 2 <= J <= SPAA_JITTER_MAX ----
 * Conventions of the capture jitter above: host arrays of J device pointers, any other J / a null pointer / a size < 1 / another
 * subsampling code is hipErrorInvalidValue with nothing launched, images [B][H*W][4] fp32, no allocation, no sync, no atomics.
 *
 * A table row is (Q, 0, 0, 0), row [B][J][4]: Q in 1..100 is the codec's quality, Q = 0 the identity row.  The round trip of an image y
 * at quality Q: p = 255 clamp(y, 0, 1); JFIF full-range YCbCr; padding by edge replication to a multiple of the MCU (8 for 4:4:4, 16
 * for 4:2:0); 4:2:0: Cb, Cr become their 2 x 2 means; per 8 x 8 block c = D (b - 128) D^T with the orthonormal DCT-II matrix D,
 * k = rint(c / T), c^ = k T, b^ = D^T c^ D + 128, with T = clamp((base s + 50) / 100, 1, 255) in integers, s = 5000 / Q below 50 and
 * 200 - 2 Q from 50 on, base the ITU-T T.81 Annex K luminance table for Y and chrominance table for Cb, Cr in natural order; 4:2:0:
 * Cb, Cr back to full resolution over the padded planes by the separable triangle filter (3 near + far) / 4 with edge replication;
 * v = RGB by the JFIF inverse (1.402, 0.344136, 0.714136, 1.772); out = rint(clamp(v, 0, 255)) / 255 cropped to H x W, pad channel 0.
 * The planes are not rounded to 8 bits in between (libjpeg does).  The identity row: out = y bit for bit in the colour channels.
 * The gate byte of a pixel: bit c = (0 <= y_c <= 1), bit 4 + c = (0 <= v_c <= 255); 0x77 in an identity row. */
#define SPAA_JPEG_444 0
#define SPAA_JPEG_420 2
/* The rows of iteration t = counter[0] (device memory; t + 1 is stored after every thread of the one workgroup has read it):
 * Q = q_lo + (((h >> 8) (q_hi - q_lo + 1)) >> 24), h spaa_jitter_draw's word of (seed, t, b, j, 0) with the first constant 0xc2b2ae35
 * in place of 0x9e3779b9; 1 <= q_lo <= q_hi <= 100.  clean0 != 0: draw 0 of every sample is the identity row. */
int spaa_jpeg_draw(uint32_t seed, int32_t* counter, int q_lo, int q_hi, int clean0, float* row, int B, int J, spaa_stream_t stream);
/* The floats of workspace spaa_jpeg_fwd needs (host-side query): 0 for 4:4:4; J B Hp Wp 3/2 for 4:2:0, Hp and Wp the sides rounded up
 * to 16: the decoded planes between its two launches (Y [Hp][Wp], Cb and Cr [Hp/2][Wp/2] per draw and sample). */
int64_t spaa_jpeg_ws_floats(int subsampling, int J, int B, int H, int W);
/* out[j], gate[j] = the round trip of y[j] at the qualities row[b][j]; there is always one input pointer per draw (J equal pointers
 * where every draw starts from the same image: the results are then those of J distinct copies bit for bit).  4:4:4 is one launch
 * and reads no workspace (ws may be NULL); 4:2:0 is two with `ws` between them (the triangle filter reads across tile borders). */
int spaa_jpeg_fwd(const float* const* y, const float* row, int J, int subsampling, float* const* out, uint8_t* const* gate, float* ws,
                  int B, int H, int W, spaa_stream_t stream);
/* The adjoint: g_y[j] = the exact transpose of the chain's linear parts applied to g_out[j] -- the 8-bit step straight-through, both
 * gates, both colour matrices, the triangle filter, DCT and IDCT, the 1/4 spread of the 2 x 2 mean, the padding cells' gradients
 * summed into their edge pixel -- with the coefficient rounding replaced by the factor phi: 1 (soft == 0), or 3 r^2 with
 * r = c / T - rint(c / T) (soft != 0), c recomputed from y[j] (no residues are stored; soft == 0 does not read y).  The identity row
 * passes g_out through.  A gather without atomics: run-to-run bitwise reproducible.  The pad channel of g_y is 0.  One launch. */
int spaa_jpeg_bwd(const float* const* g_out, const float* const* y, const float* row, int J, int subsampling, int soft,
                  const uint8_t* const* gate, float* const* g_y, int B, int H, int W, spaa_stream_t stream);

/* ---- defocus-robust SPAA: one projection against J lens blurs of the camera image, 2 <= J <= SPAA_JITTER_MAX ----------
 * Conventions of the capture jitter above: host arrays of J device pointers, any other J / a null pointer / a size < 1 is
 * hipErrorInvalidValue with nothing launched, images [B][H*W][4] fp32, no allocation, no sync, no atomics, run-to-run bitwise
 * reproducible.
 *
 * A row is 12 floats (sigma, r, w_0 .. w_8, 0), row [B][J][12]: the half kernel of a symmetric filter of 2 r + 1 taps, entries beyond
 * w_r are 0.  The row of a sigma (camera pixels), in fp32: r = min(SPAA_BLUR_RMAX, (int)ceilf(3.0f * sigma)), w_0 = 1 (set, not
 * computed), w_i = expf(-(i i) / (2 sigma sigma)) for i = 1..r, all divided by w_0 + 2 (w_1 + .. + w_r) summed in index order.
 * sigma == 0 gives the identity row (0, 0, 1, 0, ...).  The sigmas of spaa_blur_rows lie in device memory, so the entry point cannot
 * refuse one: a sigma that is not > 0 (negative, NaN) gives the identity row, and a sigma above 2.5 gives r = SPAA_BLUR_RMAX with the
 * Gaussian truncated there (the 17 taps still normalised to sum 1); callers check the range on the host, as gaussian_blur() does.  The
 * image kernels read r and the taps of a row, never its sigma; an r outside 0..SPAA_BLUR_RMAX is taken as the nearer end. */
#define SPAA_BLUR_RMAX 8
/* The tile of one workgroup of spaa_blur_fwd / spaa_blur_bwd (columns x rows): what the tests place their shapes around. */
#define SPAA_BLUR_TILE_W 32
#define SPAA_BLUR_TILE_H 16
/* The rows of n sigmas from device memory: row [n][12] of sigma [n]; 1 <= n <= 2^24.  One launch. */
int spaa_blur_rows(const float* sigma, float* row, int n, spaa_stream_t stream);
/* The rows of iteration t = counter[0] (device memory; t + 1 is stored after every thread of the one workgroup has read it):
 * sigma = fmaf(hi - lo, u, lo), u = (h >> 8) 2^-24, h spaa_jitter_draw's word of (seed, t, b, j, 0) with the first constant 0x2545f491
 * in place of 0x9e3779b9; lo == hi gives exactly lo.  0 <= lo <= hi <= 2.5, both finite, else hipErrorInvalidValue.  clean0 != 0: draw
 * 0 of every sample is the identity row. */
int spaa_blur_draw(uint32_t seed, int32_t* counter, float lo, float hi, int clean0, float* row, int B, int J, spaa_stream_t stream);
/* out[j][b] = the separable filter of y[j][b] with the taps of row[b][j] along both axes, border replicated: per axis
 * out[m] = w_0 in[m] + sum_{i=1..r} w_i (in[clamp(m - i, 0, n - 1)] + in[clamp(m + i, 0, n - 1)]), i ascending, each colour channel on
 * its own in fp32, along the rows (W) first, then along the columns (H).  The pad channel of out is 0.  No clamp and no gate: the filter
 * is linear and its taps sum to 1.  The identity row copies the colour channels bit for bit.  There is always one input pointer per
 * draw (J equal pointers give the bits of J distinct copies).  One launch, both passes through LDS. */
int spaa_blur_fwd(const float* const* y, const float* row, int J, float* const* out, int B, int H, int W, spaa_stream_t stream);
/* The exact transpose as a gather.  Replicate padding is not self-adjoint: the taps that left the frame come back into the edge pixel.
 * Per axis, with g zero outside [0, n): z_e = sum_{k=-r..r} w_|k| g_{e-k} for e = -r .. n - 1 + r; g_in[p] = z_p for 0 < p < n - 1,
 * g_in[0] = sum_{e <= 0} z_e, g_in[n - 1] = sum_{e >= n - 1} z_e (n == 1: every z_e lands in the one pixel).  An edge pixel
 * evaluates its sum regrouped by input, sum_{m=0..r} T_m g_m with the tail sums T_m = w_m + .. + w_r (mirrored at n - 1; n == 1:
 * (2 T_0 - w_0) g_0): the same value to rounding at r + 1 products.  The identity row passes g_out through bit for bit.  Along the
 * columns first, then along the rows.  The pad channel of g_y is 0.  One launch. */
int spaa_blur_bwd(const float* const* g_out, const float* row, int J, float* const* g_y, int B, int H, int W, spaa_stream_t stream);

/* ---- attention-weighted attack: Grad-CAM of the classifier weights its gradient image ---------------------------
 * No atomics and fixed summation orders: bitwise repeatable.  One launch each, none syncs. */
/* alpha [B][C] = the spatial mean of a gradient map G [B][HW][cstride] (channels 0 .. C - 1 of each position), positions added in
 * index order, then one division by HW. */
int spaa_cam_alpha(const float* G, float* alpha, int B, int HW, int C, int cstride, spaa_stream_t stream);
/* Per sample b with t = target[b] and the seed s = g_logits[b][t] (0 where t is no class): c [B][HW] = max(0, sign(s) alpha_scale
 * sum_k alpha[b][k] A[b][p][k]) of the feature map A [B][HW][C] (contiguous, C % 4 == 0), cmax [B] = max_p c.  s == 0: c = 0 and
 * cmax = 0.  alpha_scale > 0: 1 for the channel means of spaa_cam_alpha, 1 / HW for the pooled gradient of a global-average head. */
int spaa_cam_map(const float* A, const float* alpha, float alpha_scale, const float* g_logits, int ncls, const int32_t* target, float* c,
                 float* cmax, int B, int HW, int C, spaa_stream_t stream);
/* M = (c / cmax) [fh][fw] resampled bilinearly onto the ch x cw crop at (cy0, cx0) of the H x W camera frame (half-pixel centres, edge
 * clamped: F.interpolate(mode='bilinear', align_corners=False)), at most 1; cmax <= 0: M = 1.  g_y [B][H][W][4] (may be NULL): the
 * three colour channels inside the crop are multiplied by floor + (1 - floor) M in place, the pad channel and the pixels outside the
 * crop are not written, and a sample with cmax <= 0 is not written at all.  M_out [B][H][W] (may be NULL): M, 0 outside the crop.
 * 0 <= floor <= 1; sides up to 16384. */
int spaa_attention_apply(const float* c, const float* cmax, float floor, float* g_y, float* M_out, int B, int H, int W, int cy0, int cx0,
                         int ch, int cw, int fh, int fw, spaa_stream_t stream);

/* ---- transferable attack: the adversarial step's direction is smoothed (TI-FGSM) and accumulated with momentum (MI-FGSM) at the
 * projector image ---------------------------------------------------------------------------------------------------
 * Images are [B][Hp][Wp][4] fp32, state is spaa_decide's [B][4].  A sample on the colour step (state[b][1] != 0) is skipped by both
 * launches: none of its rows of g, t, m, partial_l1 or partial_ss is read or written.  No atomics and fixed summation orders: bitwise
 * repeatable.  One launch each, none syncs. */
#define SPAA_TRANSFER_RMAX 7
/* tiles per image of the blur launch (16 x 32 pixel tiles, row-major); 0 for sizes that spaa_transfer_blur refuses */
int spaa_transfer_tiles(int Hp, int Wp);
/* t_b = K (*) g_b for every sample on the adversarial step: the separable filter with the 2 r + 1 taps `taps` (a HOST array, copied into
 * the launch's arguments) along both axes, zero beyond the image border (F.conv2d with padding = r), each colour channel on its own in
 * fp32 with fused multiply-adds, taps in index order, rows first.  The pad channel of g is not used and that of t is written 0.
 * partial_l1 [B][tiles] = each tile's sum over pixels and colour channels of |t|, tiles = spaa_transfer_tiles(Hp, Wp).  Both passes run
 * in one launch through LDS.  r == 0: t = taps[0] g.  Not in place.  r outside 0 .. SPAA_TRANSFER_RMAX, a non-positive size, B > 65535,
 * Hp Wp > 2^30 or a null pointer: hipErrorInvalidValue and nothing is launched. */
int spaa_transfer_blur(const float* g, const int32_t* state, const float* taps, int r, float* t, float* partial_l1, int B, int Hp, int Wp,
                       spaa_stream_t stream);
/* For every sample on the adversarial step: n1 = the sum of partial_l1[b][0 .. tiles - 1] in index order (accumulated in double, rounded
 * once to fp32); m_b = fma(mu, m_b, t_b / n1) per colour channel, or mu m_b when n1 == 0; the pad channel of m_b is written 0; g_b = m_b.
 * Block j of the sample handles the 256-pixel chunks j, j + npartial, ... and writes partial_ss[b][j] = its sum of m.r^2 + m.g^2 + m.b^2
 * (the fixed-order block sum); all npartial entries of the row are written, those without a chunk as 0: spaa_step_and_track_n with the
 * same npartial then steps by lr m_b / ||m_b||_2.  HW = Hp Wp.  0 <= mu <= 1; tiles, npartial >= 1; B <= 65535; HW <= 2^30; anything
 * else, or a null pointer: hipErrorInvalidValue and nothing is launched. */
int spaa_transfer_momentum(const float* t, const float* partial_l1, int tiles, float mu, const int32_t* state, float* m, float* g,
                           float* partial_ss, int npartial, int B, int HW, spaa_stream_t stream);

/* ---- SSIM stealth term of the attack loop, 'camssim'  --------------------------------------------------------------
 * SSIM_b(y, scene) as pytorch_ssim._ssim(size_average=False): the 11-tap Gaussian (sigma 1.5) along both axes after replicate padding
 * by 5, C1 = 0.01^2, C2 = 0.03^2, each colour channel on its own, the mean over the 3 H W values of the map S.  Images and maps are
 * [B][H][W][4] fp32; the pad channel is never read into a result and is written 0 in the maps.  `taps` is a HOST array of 11 floats,
 * copied into the launch's arguments.  w_ps [B] (device): per-sample weights; a sample with weight 0 is skipped by spaa_ssim_fwd,
 * spaa_ssim_bwd and spaa_ssim_value: none of its rows of the maps, partial, g_y or ssim is read or written.  fp32 with fused
 * multiply-adds, taps in index order, rows first; no atomics and fixed summation orders: bitwise repeatable.  One launch each, none
 * syncs.  A null pointer, a non-positive size, B > 65535 or H W > 2^30: hipErrorInvalidValue and nothing is launched. */
#define SPAA_SSIM_TILE_H 16
#define SPAA_SSIM_TILE_W 32
/* tiles per image (SPAA_SSIM_TILE_H x SPAA_SSIM_TILE_W pixels, row-major); 0 for sizes that the launches refuse */
int spaa_ssim_tiles(int H, int W);
/* the window statistics of the scene alone, for every sample (F: replicate-pad, rows, then columns): the window mean and second moment
 * of scene - c, c per tile and channel the scene's value at the tile's first pixel: mu2 = F (scene - c), e22 = F (scene - c)^2.
 * spaa_ssim_fwd accumulates its three statistics about the same constants and shifts the means back, so that the variances do not
 * cancel in fp32; S and the maps are those of the unshifted definition. */
int spaa_ssim_scene_stats(const float* scene, const float* taps, float* mu2, float* e22, int B, int H, int W, spaa_stream_t stream);
/* mu1 = F y, e11 = F y^2, e12 = F (y scene); per pixel and channel
 *   S = A1 A2 / (B1 B2), A1 = 2 mu1 mu2 + C1, A2 = 2 (e12 - mu1 mu2) + C2, B1 = mu1^2 + mu2^2 + C1, B2 = (e11 - mu1^2) + (e22 - mu2^2) + C2
 * and m_mu = dS/dmu1, m_11 = dS/de11, m_12 = dS/de12 (the algebra of spaa_train_loss_fwd_bwd); partial [B][tiles] = each tile's sum of
 * S over its pixels and colour channels (the fixed-order block sum), tiles = spaa_ssim_tiles(H, W). */
int spaa_ssim_fwd(const float* y, const float* scene, const float* mu2, const float* e22, const float* taps, const float* w_ps, float* m_mu,
                  float* m_11, float* m_12, float* partial, int B, int H, int W, spaa_stream_t stream);
/* g_y[q] += -gscale w_ps[b] (F^T m_mu + 2 y[q] F^T m_11 + scene[q] F^T m_12)[q] on the three colour channels: gscale w_ps[b] times the
 * gradient of 3 H W (1 - SSIM_b) at y.  F^T is the adjoint of F: an edge pixel also collects the taps of the pad cells that copy it. */
int spaa_ssim_bwd(const float* y, const float* scene, const float* m_mu, const float* m_11, const float* m_12, const float* taps,
                  const float* w_ps, float gscale, float* g_y, int B, int H, int W, spaa_stream_t stream);
/* ssim [B]: ssim[b] = (sum of partial[b][0 .. tiles - 1] in index order, in double) / (3 H W), rounded once to fp32;
 * tiles must be spaa_ssim_tiles(H, W) */
int spaa_ssim_value(const float* partial, const float* w_ps, int tiles, int H, int W, float* ssim, int B, spaa_stream_t stream);

/* ---- PerC_AL.adversary_projector (perc_al/__init__.py:133-256) ------------------------------------------ */
/* x = a + b (inputs + delta), NHWC4 */
int spaa_add_nhwc4(const float* a, const float* b, float* x, int npix, spaa_stream_t stream);
/* g_logits = mult * d CrossEntropy_sum / d logits = mult * (softmax - onehot)  (:186-187) */
int spaa_ce_grad(const float* logits, int ncls, const int32_t* label, float mult, float* g_logits, int B,
                 spaa_stream_t stream);
/* x_b += step * g_b/||g_b||_2 where (state[b][col] != 0) == want; partial from spaa_grad_sumsq  (:193-195,204-209) */
int spaa_masked_step(float* x, const float* g, const float* partial, const int32_t* state, int col, int want,
                     float step, int B, int HW, spaa_stream_t stream);
/* g_px *= dE_px / ||dE_b||_2 (gradient of color_dis = ||d_map||_2, :198-200), color_dis_b out; partial3 from
 * spaa_stealth_loss_fwd_bwd */
int spaa_scale_by_map(float* g, const float* de_map, const float* partial3, float* color_dis, int B, int HW,
                      spaa_stream_t stream);
/* delta = clamp(inputs+delta,0,1) - inputs; x_round = round((inputs+delta)*255)/255 (:211-212,15-18); partial
 * [B][nblk] = block sums of ||delta_px||_2 (:215) */
int spaa_perc_clamp_quant(const float* inputs, float* delta, float* x_round, float* partial, int B, int HW,
                          spaa_stream_t stream);
/* masks on the quantised image (:216-243). mode 0 targeted, 1 untargeted, 2 untargeted with Carlini margin.
 * state [B][4]: isadv, best_adv, best, top1; stats [B][8]: p1, caml2, margin, color_dis, -, bound_best(in/out) */
int spaa_perc_decide(const float* logits, int ncls, const int32_t* label, int mode, float confidence,
                     const float* partial, int nblk, int HW, const float* color_dis, float d_thr, float p_thresh,
                     int32_t* state, float* stats, int B, spaa_stream_t stream);
/* dst_b = src_b where state[b][0] != 0 (:244-245) */
int spaa_track_where(const float* src, float* dst, const int32_t* state, int B, int HW, spaa_stream_t stream);

/* One-pixel DE attacker (one_pixel_attacker/__init__.py:18-99).  base: the quantised image [H][W][4], u8 / 255.0f; cand: int32
 * [P][5*npix] (row, col, r, g, b per square, squares painted in order, the last one wins).  out [P][oh][ow][4] = bitwise
 * spaa_preproc_fwd of base with candidate p's squares (side 2*(pixel_size/2)+1) painted (perturb_image :18-44, classifier.py:59) */
int spaa_onepixel_preproc(const float* base, const int32_t* cand, int P, int npix, int pixel_size, float* out, int H, int W,
                          int cy0, int cx0, int ch, int cw, int oh, int ow, const float* mean3, const float* std3,
                          spaa_stream_t stream);
/* per row of logits [P][ncls]: p = softmax (classifier.py:64); energy = p[target], targeted 1 - p[target] (fp32, :91-95);
 * argmax = first index of the largest p (numpy.argmax, :68-72); pmax = that p */
int spaa_onepixel_score(const float* logits, int ncls, int target, int targeted, float* energy, int32_t* argmax, float* pmax,
                        int P, spaa_stream_t stream);
/* Projector variant (ProjectorOnePixelAttacker, :161-176) with a PCNet as the project-and-capture step.  base [Hp][Wp][4] and cand as
 * above (the squares are painted into the PROJECTOR image); tap_src / tap_wgt [Hc*Wc][4]: the engine's tap table (spaa_warp_taps,
 * weights x mask).  xw [P][Hc][Wc][4] = bitwise spaa_warp_fwd_taps of the P painted images: a tap reads the last square that covers
 * its projector pixel, else base; taps outside the image (0x7fffffff) read 0.  cat8 (may be NULL) [P][Hc][Wc][8] =
 * (s.rgb, xw.r*s.r, xw.g*s.g, xw.b*s.b, 0, 0) with scene s [Hc][Wc][4] shared by all candidates, as spaa_warp_fwd writes it */
int spaa_onepixel_warp(const float* base, const int32_t* cand, int P, int npix, int pixel_size, const int32_t* tap_src,
                       const float* tap_wgt, const float* scene, float* xw, float* cat8, int Hp, int Wp, int Hc, int Wc,
                       spaa_stream_t stream);
/* y [B][H][W][4] in [0, 1] (PCNet's output) -> the classifier input out [B][oh][ow][4]: bitwise spaa_preproc_fwd of
 * (float)(uint8)(y * 255) / 255 (quantize != 0: the camera's 8-bit step, capture() :153-159) or of y itself (quantize == 0) */
int spaa_capture_preproc(const float* y, float* out, int B, int H, int W, int cy0, int cx0, int ch, int cw, int oh, int ow,
                         const float* mean3, const float* std3, int quantize, spaa_stream_t stream);

/* ---- Square Attack on the projector image (Andriushchenko et al., ECCV 2020; spaa_amd/square_attack.py) ----------
 * Sample b's current projector image x_u8 [B][Hp][Wp]: one packed word per pixel, R | G << 8 | B << 16, top byte 0; its float value
 * is u8 / 255.0f (true division).  A perturbed value is clamp(c0 +/- eps8, 0, 255), c0 in 0..255, eps8 in 1..127.  Words come from
 * draw_rng.hpp's draw_word behind two first constants of their own; the sample index of a word is b_off + b.  1 <= K <= 8,
 * B <= 65535, Hp, Wp >= 2.  state int32 [B][4] = (accepted, k*, done, queries), best_loss float [B]: zeros and +inf before
 * iteration 0. */
/* the vertical stripes: column w, channel ch of sample b = c0 + eps8 where bit 0 of the word (seed, 0, b_off + b, w, ch) is set,
 * else c0 - eps8 */
int spaa_square_init(uint32_t seed, int b_off, int c0, int eps8, uint32_t* x_u8, int B, int Hp, int Wp, spaa_stream_t stream);
/* prop int32 [B][K][8] = (r, c, h, R, G, B, 0, 0): r = word(seed, t, b_off + b, k, 0) % (Hp - h + 1), c = word(.., 1) % (Wp - h + 1),
 * R / G / B = c0 +/- eps8 by bits 0 / 1 / 2 of word(.., 2).  0 <= h <= min(Hp, Wp) - 1.  A sample with state[b][2] != 0 (resting), and
 * every sample when h == 0 (iteration 0: the stripes themselves), gets rows of zeros, which paint nothing. */
int spaa_square_propose(uint32_t seed, int t, int b_off, int h, int c0, int eps8, const int32_t* state, int32_t* prop, int B, int K, int Hp,
                        int Wp, spaa_stream_t stream);
/* spaa_onepixel_warp with a per-sample base: xw [B*K][Hc][Wc][4], row b K + k = bitwise spaa_warp_fwd_taps of x_u8[b] / 255 with the
 * square [r, r + h) x [c, c + h) of prop[b][k] painted (R, G, B) / 255; taps outside the image (0x7fffffff) read 0; the proposal words are
 * compared, never used as addresses.  cat8 (may be NULL) [B*K][Hc][Wc][8] as spaa_onepixel_warp writes it, scene [Hc][Wc][4] shared. */
int spaa_square_warp(const uint32_t* x_u8, const int32_t* prop, int B, int K, const int32_t* tap_src, const float* tap_wgt,
                     const float* scene, float* xw, float* cat8, int Hp, int Wp, int Hc, int Wc, spaa_stream_t stream);
/* Two launches.  rows float [B*K][4] = (loss, top-1, p1, 0) of logits [B*K][ncls], ncls >= 2: top-1 the first maximum, p1 = 1 / sum
 * exp(l - max); loss = l[y] - max_{j != y} l[j] (targeted[b] == 0) or logsumexp(l) - l[y] (targeted[b] != 0), y = label[b]; a label
 * outside [0, ncls) gives NaN.  Then per sample: k* = the smallest loss of its first `count` rows (1 <= count <= K: K captures per
 * iteration, 1 for the stripes), ties to the lowest k, NaN never (k* = 0 when every loss is NaN); accepted iff that loss < best_loss[b]
 * (strict), which then takes it; done = the accepted row's top-1 != y, or, targeted, == y with p1 > p_thresh; queries += count.  A
 * sample with done != 0 keeps k*, done, queries and best_loss; its accepted word becomes 0. */
int spaa_square_score(const float* logits, int ncls, const int32_t* label, const int32_t* targeted, float p_thresh, int count, float* rows,
                      float* best_loss, int32_t* state, int B, int K, spaa_stream_t stream);
/* accepted samples (state[b][0] != 0): the square of prop[b][k*] into x_u8[b] and y[b K + k*] ([B*K][Hc][Wc][4]) into cam_best[b]
 * ([B][Hc][Wc][4]); a square that does not lie inside the image is not painted.  The others are left as they are. */
int spaa_square_commit(const int32_t* state, const int32_t* prop, const float* y, uint32_t* x_u8, float* cam_best, int B, int K, int Hp,
                       int Wp, int Hc, int Wc, spaa_stream_t stream);

/* ---- direct-light mask of a camera view (train_network.py:68-80 load_data, img_proc.py:13-65 threshold_im) ---- */
/* Nayar's separation of N >= 2 shifted-checkerboard captures cb [N][3][H][W] (planar fp32, projector backlight b in [0, 1)):
 * per pixel and channel l1 = max_n, l2 = min_n, direct = (l1 - l2) / (float)(1 - b), indirect = 2 (l2 - (float)b l1) /
 * (float)(1 - b b); then clip(direct, 0, 1), g = (0.299f R + 0.587f G) + 0.114f B, gray_u8 [H][W] = (uint8)(g 255f) truncated.
 * Each step is one correctly rounded fp32 operation in that order (numpy float32 gives the same bytes).  direct (before the clip)
 * and indirect: optional [3][H][W] outputs, may be NULL.  N == 1: cb is the direct image itself (no separation, no indirect).
 * H, W >= 2. */
int spaa_cb_direct_gray(const float* cb, int N, int H, int W, double b, uint8_t* gray_u8, float* direct, float* indirect,
                        spaa_stream_t stream);
/* smooth_u8 = the 3 x 3 Gaussian (sigma 1.5, BORDER_REFLECT_101) of gray_u8 in integer arithmetic: weights round(256 g) =
 * (79, 98, 79), rows then columns without intermediate rounding, (v + 32768) >> 16.  hist [256] uint32: the histogram of smooth_u8
 * is ADDED to it (zero it first: spaa_zero); integer atomics, exact in any order.  Not in place. */
int spaa_mask_blur_hist(const uint8_t* gray_u8, int H, int W, uint8_t* smooth_u8, uint32_t* hist, spaa_stream_t stream);
/* Two-class Otsu over the present value range [vmin, vmax] of hist: candidate k splits [vmin..k] | [k+1..vmax], between-class
 * variance w0 w1 (mu0 - mu1)^2 from exact integer sums in double, first maximum; t = the smallest present value above that k.
 * mask [H][W] bytes = smooth_u8 >= t; out6 int32 = {t, xmin, ymin, xmax, ymax, count} of the mask (integer atomics; written in
 * full, no initialisation needed).  Fewer than two distinct values: out6[0] = -1, the mask empty. */
int spaa_otsu_mask_bbox(const uint8_t* smooth_u8, const uint32_t* hist, int H, int W, uint8_t* mask, int32_t* out6,
                        spaa_stream_t stream);

/* ---- result montages of the summary step (projector_based_attack.py:362-414 attack_results, img_proc.py:174-197 resize,
 * torchvision make_grid(nrow=5, padding=5, pad_value=1), cv.applyColorMap) ---------------------------------------------------- */
/* rz(x) = the ch x cw window of x at (y0, x0) (img_proc.center_crop: the caller computes the origin), then
 * F.interpolate(mode='area') to Hp x Wp: output row o covers window rows floor(o ch / Hp) .. ceil((o + 1) ch / Hp) - 1, columns
 * likewise; the window's values are added from 0 in row-major order and the sum is divided by the window's height, then by its
 * width (two correctly rounded fp32 divisions, as ATen's adaptive average pooling).  cam_scene [3][Hs][Ws], cam_real
 * [N][3][Hr][Wr], planar fp32.  minmax [N][2] = min and max over the 3 Hp Wp values |rz(real_n) - rz(scene)|; written in full
 * (no initialisation needed), integer atomics on the bit patterns of the non-negative floats: bitwise the same on every run.
 * Two kernels whatever N.  N <= 65535, image sides <= 32768. */
int spaa_montage_diff_range(const float* cam_scene, int Hs, int Ws, int sy0, int sx0, const float* cam_real, int Hr, int Wr, int ry0,
                            int rx0, int N, int ch, int cw, int Hp, int Wp, float* minmax, spaa_stream_t stream);
/* out [N][3][Hm][Wm] bytes, Hm = 26 + Hp + 10, Wm = 5 (Wp + 5) + 5: background 255; tile k at (y = 31, x = 5 + k (Wp + 5)) =
 * rz(scene), prj_adv[n] ([N][3][Hp][Wp]), rz(cam_infer[n]), rz(cam_real[n]) as (uint8)floor(v 255f) for v in [0, 1], and the
 * difference tile lut[index], lut [256][3] bytes, index = (uint8)floor(m 255f), m = ((q_0 + q_1) + q_2) / 3f,
 * q_c = (|rz(real)_c - rz(scene)_c| - mn) / (mx - mn) with (mn, mx) = minmax[n] of spaa_montage_diff_range; mx == mn: index 0.
 * No operation is contracted or reassociated.  Then the text: glyph_recs [nrec][4] int32 = (item, x, y, glyph), font
 * [95][font_h] row bytes (bit x = column x, font_w <= 8), glyph = character code - 32; a set bit inside the montage becomes
 * (0, 0, 0), the rest of a glyph is clipped, a record that names no item or no glyph is skipped.  Two kernels whatever N. */
int spaa_montage_compose(const float* cam_scene, int Hs, int Ws, int sy0, int sx0, const float* prj_adv, const float* cam_infer, int Hi,
                         int Wi, int iy0, int ix0, const float* cam_real, int Hr, int Wr, int ry0, int rx0, int N, int ch, int cw, int Hp,
                         int Wp, const float* minmax, const uint8_t* lut, const int32_t* glyph_recs, int nrec, const uint8_t* font,
                         int font_w, int font_h, uint8_t* out, spaa_stream_t stream);

/* ---- PNG encoding of device-resident images (spaa_amd/png.py holds the host half: Huffman tables, chunk CRCs, files) ---------
 * images: N images [N][3][H][W], planar fp32 (is_f32 != 0) or planar bytes.  An fp32 value becomes the low 8 bits of
 * (int32)(x * 255f): one fp32 multiply, truncation toward zero, i.e. np.uint8(x * 255) for x in [0, 1]; NaN / inf unspecified.
 * streams [N][H][1 + 3 W]: the PNG scanlines, RGB interleaved, each row led by its filter type.  Filters 0..4 (None, Sub, Up,
 * Average, Paeth with tie order left, up, upper-left) are all computed from the UNFILTERED neighbours, bytes left of the row and
 * above row 0 counting as 0; a candidate byte v costs min(v, 256 - v) and the filter with the lowest row sum wins, ties to the
 * lowest number.  hist [N][257] uint32: the histogram of the image's stream bytes, bin 256 (end of block) = 1; written in full.
 * adler [N][H][2] uint32: per row (sum of its 1 + 3 W bytes, sum of byte j times (1 + 3 W - j)), both mod 65521.  Integer atomics
 * only: bitwise the same on every run.  N <= 65535, 3 W <= 30000.  Two kernels whatever N. */
int spaa_png_filter_hist(const void* images, int is_f32, int N, int H, int W, uint8_t* streams, uint32_t* hist, uint32_t* adler,
                         spaa_stream_t stream);
/* The deflate stream of every image as ONE dynamic-Huffman block of literals: the header bits, the code of every stream byte in
 * order, the code of symbol 256, the last byte zero-padded.  streams [N][stream_bytes]; tables [N][257] uint32 = code | length
 * << 16, the code bit-reversed (deflate packs Huffman codes from their most significant bit into a stream filled from the least
 * significant bit), length <= 15; hdr [N][64] uint32 little-endian header bits, hdr_bits [N] their count (<= 2048); offsets [N]
 * int64: the byte offset of image n's stream in out.  out [out_bytes]: ZEROED by the caller, 4-byte aligned, out_bytes a multiple
 * of 4 (bits are ORed in, so neighbouring images may share a word); nothing is written past out_bytes.  chunk_bits: scratch,
 * uint32 [N][stream_bytes / 4096 + 1].  Bit positions are 64-bit.  The bytes do not depend on the order of execution. */
int spaa_png_pack(const uint8_t* streams, int64_t stream_bytes, int N, const uint32_t* tables, const uint32_t* hdr,
                  const int32_t* hdr_bits, const int64_t* offsets, uint32_t* chunk_bits, uint8_t* out, int64_t out_bytes,
                  spaa_stream_t stream);

/* ---- PNG decoding to device-resident images (spaa_amd/png.py holds the host half: chunks, CRCs, the zlib header and trailer) ----
 * One descriptor per image; offsets are bytes into the buffers the entry points name. */
typedef struct {
    int64_t src_off;      /* the raw deflate payload (zlib header and Adler-32 trailer stripped): a multiple of 4 */
    int64_t src_len;
    int32_t H, W;
    int32_t channels;     /* 1 (grey), 3 (RGB) or 4 (RGBA) */
    int32_t reserved;
    int64_t ws_off;       /* the image's scanlines, H (1 + W channels) bytes, in the workspace: a multiple of 16 */
    int64_t out_off;      /* its planar output [3][H][W] */
    int64_t row0;         /* index of its first row in the Adler array */
} spaa_png_img_t;

/* status of one image: 0, or the first rule its stream broke */
#define SPAA_PNG_OK 0
#define SPAA_PNG_BAD_BLOCK_TYPE 1   /* reserved block type 3 */
#define SPAA_PNG_STORED_LEN 2       /* stored block: LEN is not the complement of NLEN */
#define SPAA_PNG_OVERSUBSCRIBED 3   /* code lengths that no prefix code has */
#define SPAA_PNG_INCOMPLETE 4       /* an incomplete code set other than one code of length 1, or no end-of-block code */
#define SPAA_PNG_BAD_REPEAT 5       /* repeat code with nothing to repeat, or running past HLIT + HDIST */
#define SPAA_PNG_BAD_SYMBOL 6       /* literal/length symbol 286 / 287, distance code 30 / 31, a bit pattern that is no code */
#define SPAA_PNG_DIST_TOO_FAR 7     /* distance beyond the output produced so far */
#define SPAA_PNG_OUTPUT_LONG 8      /* more output than H (1 + W channels) bytes */
#define SPAA_PNG_INPUT_END 9        /* the payload ended inside a block */
#define SPAA_PNG_OUTPUT_SHORT 10    /* the final block ended before H (1 + W channels) bytes */
#define SPAA_PNG_BAD_FILTER 11      /* a scanline's filter type above 4 */
#define SPAA_PNG_BAD_DESC 12        /* a descriptor that points outside the buffers, or a size out of range */

/* Inflates every image's payload into its scanline area: one wave per image, one launch.  Handles all of RFC 1951 (stored, fixed
 * and dynamic blocks, any number of them, distances to 32768).  Nothing outside [src_off, src_off + src_len) is read and nothing
 * outside the scanline area is written; the work per image is bounded by 8 src_len + H (1 + W channels).  status [N] int32 is
 * written for every image; a failed image leaves its scanlines unspecified and does not disturb the others.  payload 4-byte and
 * workspace 16-byte aligned. */
int spaa_png_inflate(const uint8_t* payload, int64_t payload_bytes, const spaa_png_img_t* imgs, int N, uint8_t* workspace,
                     int64_t workspace_bytes, int32_t* status, spaa_stream_t stream);
/* Scanlines -> planar bytes [3][H][W] per image (grey replicated, alpha dropped): filters 0..4 of the PNG specification, arithmetic
 * mod 256, Paeth ties left, up, upper-left, bytes left of a row and above row 0 counting as 0.  adler [adler_rows][2] uint32: per
 * row (sum of its 1 + W channels scanline bytes, sum of byte j times (1 + W channels - j)), both mod 65521, as the encoder's filter
 * entry writes them.  Images whose status is not 0 are skipped; a filter type above 4 sets SPAA_PNG_BAD_FILTER.  max_w: the widest
 * image of the batch, <= 16000.  One launch. */
int spaa_png_unfilter(const uint8_t* workspace, int64_t workspace_bytes, const spaa_png_img_t* imgs, int N, int max_w, uint8_t* out,
                      int64_t out_bytes, uint32_t* adler, int64_t adler_rows, int32_t* status, spaa_stream_t stream);

/* misc */
int spaa_zero(void* p, int64_t bytes, spaa_stream_t stream);
const char* spaa_version(void);

#ifdef __cplusplus
}
#endif
#endif
