// convnext_ops.hip — the depthwise 7 x 7 layers of torchvision's ConvNeXt body (spaa_amd/convnext.py), forward and input-gradient,
// NHWC fp32, stride 1, zero padding 3.  The layer moves 8 bytes and does 98 FLOPs per element (about 12 FLOP/B against a ridge of
// about 20): it stays near the memory roof only if every input element comes from beyond the CU about once, so the reuse across the
// 7 x 7 window has to happen in registers or LDS.
//
// The form kept: a ROLLING WINDOW OF ROWS IN REGISTERS, held as accumulators.  A thread owns a float4 of channels, a strip of S
// output columns and a run of R output rows.  It walks the R + 6 input rows of its run once; each row (S + 6 float4 in registers) is
// used for all seven ky at once, added into seven rows of S accumulators -- the output rows that the input row reaches.  When a row
// has received its last tap row it is stored and the accumulator rows move up by one.  An output row so receives ky = 0 .. 6 in this
// order and kx = 0 .. 6 within each: the row-major tap order of the specification.  Consecutive lanes take consecutive channel quads
// (a wave reads whole lines); the threads of a workgroup that share a channel group take neighbouring strips, so the 6 halo columns
// of a strip are its neighbours' own columns and come from the CU's vector cache.  The 49 weights of a quad are 196 registers --
// more than a thread can spare next to 7 x S accumulators --, so a workgroup stages the weights of its (at most 64) channel quads in
// LDS once, 49 KiB, and a thread reads each as one ds_read_b128 per S FMAs of a float4; lanes read consecutive quads: no bank
// conflict.  Every index into the register arrays is a compile-time constant after unrolling: no scratch.
//
// Two forms of that kernel, chosen by shape (dw7_form) and both always tested (spaa_dwconv7_form).  WIDE: S = 4 and runs of at least
// 7 rows -- 0.25 LDS reads per float4 FMA, 224 / 202 VGPRs (forward / backward), 2 waves per SIMD.  SHORT: S = 2 and runs of at least
// 4 rows -- 0.5 LDS reads per FMA and 10 input rows for 4 output rows, but four times the threads and 152 / 134 VGPRs, 3 waves per
// SIMD.  A work item is (sample, run of rows, strip) and a workgroup packs 256 / (quads per group) of them, so the small maps
// (14 x 14 x 384, 7 x 7 x 768) get their threads from channels and batch; R shrinks towards the form's minimum until the launch has
// TARGET_THREADS threads or the map is one run.  The two forms accumulate in the same order: their outputs are bitwise equal.
//
// The backward pass is the same kernel on the map mirrored in both axes: g_in[y, x] = add + sum w[ky, kx] g_out[y + 3 - ky,
// x + 3 - kx] is, in mirrored coordinates, the forward sum with the same (ky, kx) -- so the walk runs from the last row up and the
// taps keep their row-major order.  A gather, no atomics; acc starts at the bias (forward) or 0 (backward) and `add` is added last.
//
// A tap outside the image.  Rows outside the image are skipped.  Columns outside it are loaded as 0 and multiplied: fmaf(w, 0, acc)
// is acc for every finite w, so the value is that of the skipped tap (up to the sign of a zero sum); the library's contract is finite
// values.
//
// Measured on an MI355X (tools/time_convnext.py, profiles/convnext_time.jsonl; B = 64, buffers rotated past the last-level cache,
// median of 7 windows of 10 launches; at each shape WIDE, then SHORT, then the library's own choice), forward / backward with add /
// backward without, in us:
//                      WIDE                    SHORT                   as chosen
//   56 x 56 x  96    67.4 / 96.1 / 60.9      67.5 / 90.1 / 67.4      59.1 / 93.1 / 59.7  (WIDE)
//   28 x 28 x 192    36.6 / 52.1 / 36.5      44.0 / 55.9 / 41.6      36.5 / 52.3 / 36.4  (WIDE)
//   14 x 14 x 384    29.0 / 42.4 / 29.1      23.5 / 28.4 / 22.8      23.2 / 28.5 / 22.5  (SHORT)
//    7 x  7 x 768    21.6 / 34.9 / 21.4      16.9 / 22.4 / 16.3      16.8 / 22.1 / 16.1  (SHORT)
// WIDE is kept for the two large maps and SHORT for the two small ones, where WIDE cannot give every SIMD a wave (384 waves for 1024
// SIMDs at 7 x 7 x 768).  At 56 x 56 x 96 the two are a tie: WIDE's forward windows ran from 62.9 to 72.0 us when it was timed first
// after the buffers were made and 58.5 to 59.5 when timed last, SHORT is 6 % ahead with add and 10 % behind without.  As chosen:
// 2.6 / 2.1 / 1.7 / 1.15 TB/s of in + out forward, 0.33 / 0.26 / 0.21 / 0.14 of the 8 TB/s memory roof -- not at the roof on any
// shape (DESIGN.md 7p says what the counts suggest and what was not tried: a prefetch of the next row).
//
// The other candidate, a haloed pixel tile in LDS from which every thread reads its S + 6 inputs and 7 weights per tap row, was NOT
// built, so the rolling form was not measured against it: between those two the choice rests on a count ((S + 6 + 7) / (7 S) = 0.61
// float4 from LDS per float4 FMA there against 0.25 here, LDS bandwidth being the unit this form loads most), not on a measurement.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"

namespace {

constexpr int K = 7, PAD = 3, TAPS = K * K;
constexpr int MAX_CQ = 64;            // channel quads per workgroup (one wave wide): TAPS x MAX_CQ float4 = 49 KiB of LDS
constexpr int64_t TARGET_THREADS = 256 * 4 * 64 * 3;   // three waves per SIMD of 256 CUs
// The two forms of the one kernel: output columns per thread S and the shortest run of output rows per thread.
//   WIDE:  S = 4, runs of >= 7 rows (13 input rows for 7): 0.25 LDS reads per float4 FMA, 112 accumulator registers
//   SHORT: S = 2, runs of >= 4 rows (10 input rows for 4): 0.5 LDS reads per float4 FMA, 56 accumulator registers, four times the threads
constexpr int FORM_AUTO = 0, FORM_WIDE = 1, FORM_SHORT = 2;
constexpr int WIDE_S = 4, WIDE_MIN_ROWS = 7, SHORT_S = 2, SHORT_MIN_ROWS = 4;
// FORM_AUTO takes SHORT where WIDE at its shortest runs would launch fewer threads than one wave for every SIMD of 256 CUs (dw7_form).
// At B = 64 that is WIDE at 56 x 56 x 96 and 28 x 28 x 192 (172032 and 86016 threads) and SHORT at 14 x 14 x 384 and 7 x 7 x 768
// (49152 and 24576): the side of the line each shape was measured faster on, see the header.
constexpr int64_t SHORT_BELOW_THREADS = 256 * 4 * 64;
int g_form = FORM_AUTO;               // spaa_dwconv7_form

__device__ __forceinline__ float4 fma4(const float4 w, const float4 v, const float4 a) {
    return make_float4(fmaf(w.x, v.x, a.x), fmaf(w.y, v.y, a.y), fmaf(w.z, v.z, a.z), fmaf(w.w, v.w, a.w));
}

struct Geo {
    int B, H, W, C4;
    int cqb;          // channel quads per workgroup (<= MAX_CQ); blockIdx.y is the group
    int pb;           // work items per workgroup: 256 / cqb
    int nstrip, nrun, R;
    int64_t items;    // B x nrun x nstrip
};

// FLIP: the map is addressed mirrored in both axes (the backward pass).  `bias` [C4] or null (0); `add` [B, H, W, C4] or null, and it
// may be `out` itself (neither is __restrict__: a lane reads add[o] before it writes out[o], and no other lane touches o).
template <bool FLIP, int S>
__global__ __launch_bounds__(256) void dw7_kernel(const float4* __restrict__ in, const float4* __restrict__ w,
                                                  const float4* __restrict__ bias, const float4* add, float4* out, const Geo g) {
    constexpr int NC = S + K - 1;         // input columns per thread
    __shared__ float4 ws[TAPS * MAX_CQ];
    const int cq = (int)threadIdx.x % g.cqb, slot = (int)threadIdx.x / g.cqb;
    const int c0 = (int)blockIdx.y * g.cqb;
    for (int i = (int)threadIdx.x; i < TAPS * g.cqb; i += 256) {
        const int t = i / g.cqb, q = i % g.cqb;
        ws[t * MAX_CQ + q] = c0 + q < g.C4 ? w[(size_t)t * g.C4 + c0 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const int c = c0 + cq;
    const int64_t item = (int64_t)blockIdx.x * g.pb + slot;
    if (slot >= g.pb || c >= g.C4 || item >= g.items) return;
    const int sx = (int)(item % g.nstrip);
    const int64_t r = item / g.nstrip;
    const int run = (int)(r % g.nrun), b = (int)(r / g.nrun);
    // (u, v): column and row in the walk's frame; the tensor's are (W - 1 - u, H - 1 - v) where FLIP
    const int u0 = sx * S, v0 = run * g.R;
    const int nrows = min(g.R, g.H - v0);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 bs = zero;
    if (bias != nullptr) bs = bias[c];
    unsigned colok = 0;    // bit j: input column u0 - 3 + j lies in the image
#pragma unroll
    for (int j = 0; j < NC; ++j) colok |= ((unsigned)(u0 - PAD + j) < (unsigned)g.W ? 1u : 0u) << j;
    // input column j of the strip is `cstep` float4 after column j - 1 in memory (before it where FLIP).  Column 0 may lie outside the
    // image, so its offset `col0` from the row's first pixel stays an integer: `in` is indexed only where a column is loaded
    const int cstep = FLIP ? -g.C4 : g.C4;
    const int64_t col0 = (int64_t)(FLIP ? g.W - 1 - (u0 - PAD) : u0 - PAD) * g.C4;
    const int64_t img = (int64_t)b * g.H * g.W * g.C4 + c;
    const float4* const wq = ws + cq;
    float4 acc[K][S];      // acc[j]: the output row v - 3 + j while the walk is at input row v
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int i = 0; i < S; ++i) acc[j][i] = bs;
    for (int v = v0 - PAD; v < v0 + nrows + PAD; ++v) {
        if ((unsigned)v < (unsigned)g.H) {
            const int64_t row = img + (int64_t)(FLIP ? g.H - 1 - v : v) * g.W * g.C4 + col0;
            float4 x[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                x[j] = zero;
                if ((colok >> j) & 1u) x[j] = in[row + j * cstep];
            }
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                // tap row ky of the output row v + 3 - ky, which is acc[6 - ky]; only the rows of this thread's run are computed
                if ((unsigned)(v + PAD - ky - v0) >= (unsigned)nrows) continue;
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const float4 wk = wq[(ky * K + kx) * MAX_CQ];
#pragma unroll
                    for (int i = 0; i < S; ++i) acc[K - 1 - ky][i] = fma4(wk, x[i + kx], acc[K - 1 - ky][i]);
                }
            }
        }
        const int vo = v - PAD;    // the output row that has now received its last tap row
        if ((unsigned)(vo - v0) < (unsigned)nrows) {
            const size_t orow = ((size_t)b * g.H + (FLIP ? g.H - 1 - vo : vo)) * g.W;
#pragma unroll
            for (int i = 0; i < S; ++i) {
                const int u = u0 + i;
                if (u >= g.W) break;
                const size_t o = (orow + (FLIP ? g.W - 1 - u : u)) * g.C4 + c;
                float4 a = acc[0][i];
                if (add != nullptr) {
                    const float4 d = add[o];
                    a = make_float4(a.x + d.x, a.y + d.y, a.z + d.z, a.w + d.w);
                }
                out[o] = a;
            }
        }
#pragma unroll
        for (int j = 0; j < K - 1; ++j)
#pragma unroll
            for (int i = 0; i < S; ++i) acc[j][i] = acc[j + 1][i];
#pragma unroll
        for (int i = 0; i < S; ++i) acc[K - 1][i] = bs;
    }
}

// every tensor below 2^29 elements (2 GiB): element offsets and the item count fit an int / a grid
inline bool dw7_ok(int B, int H, int W, int C) {
    return B > 0 && H > 0 && W > 0 && C > 0 && !(C & 3) && (int64_t)B * H * W * C < ((int64_t)1 << 29);
}

inline Geo dw7_geo(int B, int H, int W, int C, int S, int min_rows) {
    Geo g{};
    g.B = B, g.H = H, g.W = W, g.C4 = C / 4;
    const int ngroup = (g.C4 + MAX_CQ - 1) / MAX_CQ;
    g.cqb = (g.C4 + ngroup - 1) / ngroup;          // 24, 48, 48 (two groups), 64 (three groups) at the four stage widths
    g.pb = 256 / g.cqb;
    g.nstrip = (W + S - 1) / S;
    // the longest run of rows that still gives TARGET_THREADS threads, at least min_rows
    const int64_t per_run = (int64_t)B * g.nstrip * g.C4;
    const int64_t want = (TARGET_THREADS + per_run - 1) / per_run;                       // runs per column of the map
    g.R = (int)(want >= H ? 1 : (H + want - 1) / want);
    if (g.R < min_rows) g.R = min_rows < H ? min_rows : H;
    g.nrun = (H + g.R - 1) / g.R;
    g.items = (int64_t)B * g.nrun * g.nstrip;
    return g;
}

// FORM_AUTO: SHORT where the WIDE form at its shortest runs cannot give the machine SHORT_BELOW_THREADS threads
inline int dw7_form(int B, int H, int W, int C) {
    if (g_form != FORM_AUTO) return g_form;
    const int64_t wide = (int64_t)B * ((H + WIDE_MIN_ROWS - 1) / WIDE_MIN_ROWS) * ((W + WIDE_S - 1) / WIDE_S) * (C / 4);
    return wide < SHORT_BELOW_THREADS ? FORM_SHORT : FORM_WIDE;
}

template <bool FLIP>
inline int dw7_launch(const float* in, const float* w, const float* bias, const float* add, float* out, int B, int H, int W, int C,
                      spaa_stream_t stream) {
    const bool wide = dw7_form(B, H, W, C) == FORM_WIDE;
    const Geo g = wide ? dw7_geo(B, H, W, C, WIDE_S, WIDE_MIN_ROWS) : dw7_geo(B, H, W, C, SHORT_S, SHORT_MIN_ROWS);
    const dim3 grid((unsigned)((g.items + g.pb - 1) / g.pb), (unsigned)((g.C4 + g.cqb - 1) / g.cqb));
    if (wide)
        hipLaunchKernelGGL((dw7_kernel<FLIP, WIDE_S>), grid, dim3(256), 0, (hipStream_t)stream, (const float4*)in, (const float4*)w,
                           (const float4*)bias, (const float4*)add, (float4*)out, g);
    else
        hipLaunchKernelGGL((dw7_kernel<FLIP, SHORT_S>), grid, dim3(256), 0, (hipStream_t)stream, (const float4*)in, (const float4*)w,
                           (const float4*)bias, (const float4*)add, (float4*)out, g);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int spaa_dwconv7_form(int form) {
    const int before = g_form;
    if (form == FORM_AUTO || form == FORM_WIDE || form == FORM_SHORT) g_form = form;
    return before;
}

int spaa_dwconv7_fwd(const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int C, spaa_stream_t stream) {
    if (!in || !w || !bias || !out || !dw7_ok(B, H, W, C)) return hipErrorInvalidValue;
    return dw7_launch<false>(in, w, bias, nullptr, out, B, H, W, C, stream);
}

int spaa_dwconv7_bwd(const float* g_out, const float* w, const float* add, float* g_in, int B, int H, int W, int C,
                     spaa_stream_t stream) {
    if (!g_out || !w || !g_in || !dw7_ok(B, H, W, C)) return hipErrorInvalidValue;
    return dw7_launch<true>(g_out, w, nullptr, add, g_in, B, H, W, C, stream);
}

}  // extern "C"
