// square_ops.hip — the device side of the Square Attack on the projector image (Andriushchenko, Croce, Flammarion, Hein: "Square Attack:
// a query-efficient black-box adversarial attack via random search", ECCV 2020; spaa_amd/square_attack.py): a random
// search in the L-infinity ball of radius eps8 around the grey projector image.  The state of sample b is its CURRENT projector image
// x_u8[b] (one packed 32-bit word per pixel: R | G << 8 | B << 16, the top byte 0; its float value is u8 / 255.0f by true division),
// best_loss[b] and the words state[b] = (accepted, k*, done, queries).  One iteration is
//   spaa_square_propose   K squares per sample from the counter-based generator of draw_rng.hpp
//   spaa_square_warp      spaa_onepixel_warp (onepixel.hip) with a per-sample base: the warped image of every candidate = the sample's
//                         current image with one square painted, straight from x_u8 and the tap table; no candidate's image exists
//   (PCNetEngine.forward_from_xw, spaa_capture_preproc, the classifier body: unchanged)
//   spaa_square_score     logits -> loss / top-1 / p1 per candidate, then per sample the choice, the acceptance and the success rule
//   spaa_square_commit    accepted samples: the chosen square into x_u8[b], the chosen capture into cam_best[b]
// and spaa_square_init writes the vertical stripes the search starts from.  All pixel arithmetic is in 8-bit integers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "../../include/spaa_hip.h"
#include "draw_rng.hpp"

namespace {

// first constants of the two tables (jitter, pose and JPEG have theirs): tests/square_oracle.py restates both in Python integers
constexpr uint32_t SQ_INIT = 0x27d4eb2fu, SQ_PROPOSE = 0x165667b1u;

// clamp(c0 +/- eps8, 0, 255): bit set = plus
__device__ __forceinline__ int sq_value(int c0, int eps8, uint32_t bit) {
    const int v = bit ? c0 + eps8 : c0 - eps8;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One thread per pixel: column w, channel ch of sample b takes bit 0 of the word (seed, 0, b_off + b, w, ch).
__global__ __launch_bounds__(256) void square_init_kernel(uint32_t seed, int b_off, int c0, int eps8, uint32_t* __restrict__ x, int B,
                                                          int Hp, int Wp) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * Hp * Wp) return;
    const int b = idx / (Hp * Wp);
    const int w = (idx - b * Hp * Wp) % Wp;
    uint32_t v = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        v |= (uint32_t)sq_value(c0, eps8, draw_word(SQ_INIT, seed, 0u, (uint32_t)(b_off + b), (uint32_t)w, (uint32_t)ch) & 1u) << (8 * ch);
    x[idx] = v;
}

// One thread per proposal (b, k): prop[b][k] = (r, c, h, R, G, B, 0, 0).  A resting sample (state[b][2] != 0) and every sample of an
// h == 0 call (iteration 0: the stripes themselves are the candidate) get a row of zeros, which paints nothing.
__global__ __launch_bounds__(256) void square_propose_kernel(uint32_t seed, uint32_t t, int b_off, int h, int c0, int eps8,
                                                             const int32_t* __restrict__ state, int32_t* __restrict__ prop, int B, int K,
                                                             int Hp, int Wp) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * K) return;
    const int b = idx / K, k = idx - b * K;
    int4 lo = make_int4(0, 0, 0, 0), hi = make_int4(0, 0, 0, 0);
    if (h > 0 && state[4 * b + 2] == 0) {
        const uint32_t bb = (uint32_t)(b_off + b);
        const uint32_t s = draw_word(SQ_PROPOSE, seed, t, bb, (uint32_t)k, 2u);
        lo.x = (int)(draw_word(SQ_PROPOSE, seed, t, bb, (uint32_t)k, 0u) % (uint32_t)(Hp - h + 1));
        lo.y = (int)(draw_word(SQ_PROPOSE, seed, t, bb, (uint32_t)k, 1u) % (uint32_t)(Wp - h + 1));
        lo.z = h;
        lo.w = sq_value(c0, eps8, s & 1u);
        hi.x = sq_value(c0, eps8, (s >> 1) & 1u);
        hi.y = sq_value(c0, eps8, (s >> 2) & 1u);
    }
    int4* o = (int4*)prop + 2 * (size_t)idx;
    o[0] = lo;
    o[1] = hi;
}

__device__ __forceinline__ float4 sq_rgb(int r, int g, int b) {
    return make_float4((float)(uint8_t)r / 255.0f, (float)(uint8_t)g / 255.0f, (float)(uint8_t)b / 255.0f, 0.f);
}

// onepixel_warp_kernel (onepixel.hip) with a per-sample base: the same 32 x 8 tile of camera pixels, the same XCD-contiguous walk, the same
// sum in the same order -- row b K + k is bitwise spaa_warp_fwd_taps of x_u8[b] / 255 with proposal (b, k) painted.  A workgroup owns one
// tile of ONE sample and writes its K rows from one set of four tap reads; the current image is 4 bytes per pixel (256 KB at 256 x 256,
// where the float image of the One-pixel kernel is 1 MB), so the B images of a batch stay in cache together.  A tap inside the square
// [r, r + h) x [c, c + h) reads the proposal's colour; h == 0 covers nothing.  The proposal words are uniform per workgroup and row
// (scalar loads) and are only compared, never used as addresses.  HBM traffic = the output: 16 B per camera pixel and row (48 B with cat8).
constexpr int SW_W = 32, SW_H = 8, SW_K = 8;
__global__ __launch_bounds__(256) void square_warp_kernel(const uint32_t* __restrict__ x, const int32_t* __restrict__ prop, int K,
                                                          const int4* __restrict__ src, const float4* __restrict__ wgt,
                                                          const float4* __restrict__ scene, float4* __restrict__ xw,
                                                          float4* __restrict__ cat8, int HWp, int Wp, int Hc, int Wc, int ntx, int ntile) {
    int t;
    {
        const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
        t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    }
    const int tile = t % ntile, b = t / ntile;
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int cy = ty * SW_H + (threadIdx.x >> 5), cx = tx * SW_W + (threadIdx.x & 31);
    if (cy >= Hc || cx >= Wc) return;
    const int pix = cy * Wc + cx;
    const int4 s = src[pix];
    const float4 w = wgt[pix];
    const int si[4] = {s.x, s.y, s.z, s.w};
    const float wi[4] = {w.x, w.y, w.z, w.w};
    const uint32_t* xb = x + (size_t)b * HWp;
    float4 bv[4];
    int py[4], px[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool in = si[q] != 0x7fffffff;
        const uint32_t u = in ? xb[si[q]] : 0u;
        bv[q] = sq_rgb((int)(u & 255u), (int)((u >> 8) & 255u), (int)((u >> 16) & 255u));
        py[q] = in ? si[q] / Wp : 0;
        px[q] = in ? si[q] - py[q] * Wp : 0;
    }
    float4 sv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cat8 != nullptr) sv = scene[pix];
    for (int k = 0; k < K; ++k) {
        const int32_t* c = prop + 8 * ((size_t)b * K + k);
        const long long r0 = c[0], c0 = c[1], h = c[2];
        const float4 col = sq_rgb(c[3], c[4], c[5]);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool hit = si[q] != 0x7fffffff && py[q] >= r0 && py[q] < r0 + h && px[q] >= c0 && px[q] < c0 + h;
            const float4 u = hit ? col : bv[q];
            a0 += u.x * wi[q];
            a1 += u.y * wi[q];
            a2 += u.z * wi[q];
        }
        const size_t o = ((size_t)b * K + k) * Hc * Wc + pix;
        xw[o] = make_float4(a0, a1, a2, 0.f);
        if (cat8 != nullptr) {
            cat8[2 * o] = make_float4(sv.x, sv.y, sv.z, a0 * sv.x);
            cat8[2 * o + 1] = make_float4(a1 * sv.y, a2 * sv.z, 0.f, 0.f);
        }
    }
}

// One wave per row b K + k of logits: rows[row] = (loss, top-1, p1, 0).  top-1 and p1 follow decide_top1's rule (decide_util.hpp: the first
// maximum, p1 = 1 / sum exp(l - max); that function is the 256-thread workgroup form of it, this one a wave's, with the sum in a wave's
// fixed order).  loss: untargeted l[y] - max_{j != y} l[j]; targeted logsumexp(l) - l[y] = (max + log sum) - l[y].  A label outside
// [0, ncls) gives NaN, and so does a NaN among the logits (the maxima skip a NaN, the sum does not: a row with a NaN anywhere has a NaN
// sum, as float64's max would make its loss NaN); the choice below never takes a NaN.
__global__ __launch_bounds__(256) void square_rows_kernel(const float* __restrict__ logits, int ncls, const int32_t* __restrict__ label,
                                                          const int32_t* __restrict__ targeted, float* __restrict__ rows, int K, int P) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= P) return;                         // (whole waves: no shuffle below is left without its partners)
    const float* lg = logits + (size_t)row * ncls;
    const int b = row / K;
    const int y = label[b];
    float mx = -INFINITY, mo = -INFINITY;         // the maximum, and the maximum over j != y
    int am = INT_MAX;
    for (int i = lane; i < ncls; i += 64) {
        const float v = lg[i];
        if (v > mx) {
            mx = v;
            am = i;
        }
        if (i != y) mo = fmaxf(mo, v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(mx, off, 64);
        const int oa = __shfl_xor(am, off, 64);
        if (ov > mx || (ov == mx && oa < am)) {
            mx = ov;
            am = oa;
        }
        mo = fmaxf(mo, __shfl_xor(mo, off, 64));
    }
    float se = 0.f;
    for (int i = lane; i < ncls; i += 64) se += expf(lg[i] - mx);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) se += __shfl_xor(se, off, 64);
    if (lane == 0) {
        float loss = NAN;
        if (y >= 0 && y < ncls && se == se) loss =targeted[b] ? (mx + logf(se)) - lg[y] : lg[y] - mo;
        ((float4*)rows)[row] = make_float4(loss, (float)am, 1.f / se, 0.f);
    }
}

// One thread per sample, the first `count` of its K rows in index order: count == K captures per iteration, 1 for the stripes, whose K rows
// are the same image (the networks do not promise the same bits at every batch position, so the other rows must not compete).  Choice: the
// smallest loss, ties to the lowest k (a strict < from +inf: a NaN is never taken).  Accepted iff that loss < best_loss[b] (strict).
// done = the accepted candidate succeeds: top-1 != label, or, targeted, top-1 == target and p1 > p_thresh (spaa()'s rule).  queries +=
// count while the sample is live.  A resting sample keeps k*, done, queries and best_loss; its `accepted` word is 0, so that the commit
// leaves it alone.
__global__ __launch_bounds__(256) void square_choose_kernel(const float* __restrict__ rows, const int32_t* __restrict__ label,
                                                            const int32_t* __restrict__ targeted, float p_thresh, int count,
                                                            float* __restrict__ best_loss, int32_t* __restrict__ state, int B, int K) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int32_t* s = state + 4 * b;
    if (s[2] != 0) {
        s[0] = 0;
        return;
    }
    const float4* r = (const float4*)rows + (size_t)b * K;
    float lo = INFINITY;
    int ks = -1;
    for (int k = 0; k < count; ++k) {
        const float l = r[k].x;
        if (l < lo) {
            lo = l;
            ks = k;
        }
    }
    const bool acc = ks >= 0 && lo < best_loss[b];
    if (acc) {
        const int top1 = (int)r[ks].y;
        best_loss[b] = lo;
        s[2] = targeted[b] ? (top1 == label[b] && r[ks].z > p_thresh) : (top1 != label[b]);
    }
    s[0] = acc;
    s[1] = ks < 0 ? 0 : ks;
    s[3] += count;
}

// Workgroups (x, b): those of a sample that was not accepted return at once.  Otherwise y[b K + k*] -> cam_best[b] (the byte-heavy part:
// 16 B per camera pixel read and written) and the h x h pixels of proposal k* into x_u8[b].  The proposal's position is used as an address
// here, so it is checked against the image again.
__global__ __launch_bounds__(256) void square_commit_kernel(const int32_t* __restrict__ state, const int32_t* __restrict__ prop,
                                                            const float4* __restrict__ y, uint32_t* __restrict__ x,
                                                            float4* __restrict__ cam_best, int K, int Hp, int Wp, int HWc) {
    const int b = blockIdx.y;
    const int ks = state[4 * b + 1];
    if (state[4 * b] == 0 || ks < 0 || ks >= K) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < HWc) cam_best[(size_t)b * HWc + i] = y[((size_t)b * K + ks) * HWc + i];
    const int32_t* c = prop + 8 * ((size_t)b * K + ks);
    const int r0 = c[0], c0 = c[1], h = c[2];
    if (h < 1 || h > Hp || h > Wp || r0 < 0 || c0 < 0 || r0 > Hp - h || c0 > Wp - h) return;
    const uint32_t v = (uint32_t)(uint8_t)c[3] | (uint32_t)(uint8_t)c[4] << 8 | (uint32_t)(uint8_t)c[5] << 16;
    for (int j = i; j < h * h; j += gridDim.x * blockDim.x) {
        const int dy = j / h, dx = j - dy * h;
        x[((size_t)b * Hp + (r0 + dy)) * Wp + (c0 + dx)] = v;
    }
}

// (element counts stay 255 below 2^31: a thread index rounded up to the workgroup never wraps in int)
constexpr int64_t SQ_MAX_ELEMS = (int64_t)INT_MAX - 255;
bool square_sizes_ok(int B, int K, int Hp, int Wp) {
    return B >= 1 && K >= 1 && K <= SW_K && Hp >= 2 && Wp >= 2 && (int64_t)B * Hp * Wp <= SQ_MAX_ELEMS && B <= 65535;
}

}  // namespace

extern "C" {

int spaa_square_init(uint32_t seed, int b_off, int c0, int eps8, uint32_t* x_u8, int B, int Hp, int Wp, spaa_stream_t stream) {
    if (!x_u8 || !square_sizes_ok(B, 1, Hp, Wp) || b_off < 0 || (int64_t)b_off + B > INT_MAX || c0 < 0 || c0 > 255 || eps8 < 1 || eps8 > 127)
        return hipErrorInvalidValue;
    const int n = B * Hp * Wp;
    hipLaunchKernelGGL(square_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, b_off, c0, eps8, x_u8,
                       B, Hp, Wp);
    return (int)hipGetLastError();
}

int spaa_square_propose(uint32_t seed, int t, int b_off, int h, int c0, int eps8, const int32_t* state, int32_t* prop, int B, int K, int Hp,
                        int Wp, spaa_stream_t stream) {
    if (!state || !prop || !square_sizes_ok(B, K, Hp, Wp) || t < 0 || b_off < 0 || (int64_t)b_off + B > INT_MAX || h < 0 || h > Hp - 1 ||
        h > Wp - 1 || c0 < 0 || c0 > 255 || eps8 < 1 || eps8 > 127)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(square_propose_kernel, dim3((unsigned)((B * K + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, (uint32_t)t,
                       b_off, h, c0, eps8, state, prop, B, K, Hp, Wp);
    return (int)hipGetLastError();
}

int spaa_square_warp(const uint32_t* x_u8, const int32_t* prop, int B, int K, const int32_t* tap_src, const float* tap_wgt,
                     const float* scene, float* xw, float* cat8, int Hp, int Wp, int Hc, int Wc, spaa_stream_t stream) {
    if (!x_u8 || !prop || !tap_src || !tap_wgt || !xw || (cat8 && !scene) || !square_sizes_ok(B, K, Hp, Wp) || Hc < 1 || Wc < 1)
        return hipErrorInvalidValue;
    if ((int64_t)B * K * Hc * Wc > SQ_MAX_ELEMS) return hipErrorInvalidValue;
    const int ntx = (Wc + SW_W - 1) / SW_W, nty = (Hc + SW_H - 1) / SW_H;
    const int64_t nwg = (int64_t)ntx * nty * B;
    if (nwg > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(square_warp_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, x_u8, prop, K, (const int4*)tap_src,
                       (const float4*)tap_wgt, (const float4*)scene, (float4*)xw, (float4*)cat8, Hp * Wp, Wp, Hc, Wc, ntx, ntx * nty);
    return (int)hipGetLastError();
}

int spaa_square_score(const float* logits, int ncls, const int32_t* label, const int32_t* targeted, float p_thresh, int count, float* rows,
                      float* best_loss, int32_t* state, int B, int K, spaa_stream_t stream) {
    if (!logits || !label || !targeted || !rows || !best_loss || !state || ncls < 2 || B < 1 || B > 65535 || K < 1 || K > SW_K || count < 1 ||
        count > K ||!(p_thresh >= 0.f && p_thresh <= 1.f))
        return hipErrorInvalidValue;
    const int P = B * K;
    hipLaunchKernelGGL(square_rows_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, ncls, label, targeted,
                       rows, K, P);
    hipLaunchKernelGGL(square_choose_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, label, targeted,
                       p_thresh, count, best_loss, state, B, K);
    return (int)hipGetLastError();
}

int spaa_square_commit(const int32_t* state, const int32_t* prop, const float* y, uint32_t* x_u8, float* cam_best, int B, int K, int Hp,
                       int Wp, int Hc, int Wc, spaa_stream_t stream) {
    if (!state || !prop || !y || !x_u8 || !cam_best || !square_sizes_ok(B, K, Hp, Wp) || Hc < 1 || Wc < 1 ||
        (int64_t)B * K * Hc * Wc > SQ_MAX_ELEMS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(square_commit_kernel, dim3((unsigned)((Hc * Wc + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, state,
                       prop, (const float4*)y, x_u8, (float4*)cam_best, K, Hp, Wp, Hc * Wc);
    return (int)hipGetLastError();
}

}  // extern "C"
