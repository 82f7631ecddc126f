// onepixel.hip — the per-candidate work of the One-pixel DE attacker (one_pixel_attacker/__init__.py:18-99 in the reference:
// DigitalOnePixelAttacker.perturb_and_predict / predict_fn), around the classifier body's forward pass:
//   spaa_onepixel_preproc   perturb_image (paint the candidate squares, :18-44) fused into the classifier's gather: center crop
//                           + area resize + Normalize (classifier.py:59), written straight into the body's input
//   spaa_onepixel_score     softmax (classifier.py:64) -> the DE energy p[target] / 1 - p[target] (:91-95) and numpy's
//                           argmax of p (:68-72), so only three numbers per candidate leave the device
// and of its projector variant (ProjectorOnePixelAttacker.step_and_predict, :161-176) with a PCNet as the project-and-capture step:
//   spaa_onepixel_warp      perturb_image fused into WarpingNet's sampling: the warped projector image of every candidate straight
//                           from the shared grey image and the per-attack tap table; no candidate's projector image exists
//   spaa_capture_preproc    the camera's 8-bit step (capture() returns uint8 / 255, :159) fused into the classifier's gather
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "../../include/spaa_hip.h"

namespace {

__device__ __forceinline__ int win_start(int i, int out, int in) {
    return (int)floorf((float)(i * in) / (float)out);
}
__device__ __forceinline__ int win_end(int i, int out, int in) {
    return (int)ceilf((float)((i + 1) * in) / (float)out);
}

// One thread per output pixel of one candidate.  The window sum runs in preproc_fwd_kernel's order (classifier_ops.hip) over
// the perturbed image: the result is bitwise spaa_preproc_fwd of that image.  A pixel inside candidate square k (centre
// (r_k, c_k), half-width d) reads (u8) rgb_k / 255 instead of the base image; the last square that covers it wins, as the
// reference paints them in list order.  Candidate values are only compared, never used as addresses.
__global__ __launch_bounds__(256) void onepixel_preproc_kernel(const float4* __restrict__ base, const int32_t* __restrict__ cand,
                                                               int P, int npix, int d, float4* __restrict__ out, int W, int cy0,
                                                               int cx0, int ch, int cw, int oh, int ow, float m0, float m1,
                                                               float m2, float s0, float s1, float s2) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * oh * ow) return;
    const int p = idx / (oh * ow);
    const int r = idx - p * oh * ow;
    const int oy = r / ow, ox = r - oy * ow;
    const int32_t* cp = cand + (size_t)p * 5 * npix;
    const int ys = win_start(oy, oh, ch), ye = win_end(oy, oh, ch);
    const int xs = win_start(ox, ow, cw), xe = win_end(ox, ow, cw);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int iy = ys; iy < ye; ++iy) {
        const int y = cy0 + iy;
        const float4* row = base + (size_t)y * W + cx0;
        for (int ix = xs; ix < xe; ++ix) {
            float4 v = row[ix];
            const int x = cx0 + ix;
            for (int k = 0; k < npix; ++k) {
                const int32_t* q = cp + 5 * k;
                if (llabs((long long)y - q[0]) <= d && llabs((long long)x - q[1]) <= d)
                    v = make_float4((float)(uint8_t)q[2] / 255.0f, (float)(uint8_t)q[3] / 255.0f, (float)(uint8_t)q[4] / 255.0f, 0.f);
            }
            a0 += v.x;
            a1 += v.y;
            a2 += v.z;
        }
    }
    const float cnt = (float)((ye - ys) * (xe - xs));
    out[idx] = make_float4((a0 / cnt - m0) / s0, (a1 / cnt - m1) / s1, (a2 / cnt - m2) / s2, 0.f);
}

// A camera pixel's four taps from the tap table, as warp_fwd_taps_kernel (warp.hip) reads them: the same 32 x 8 tile of camera pixels x
// FB images per workgroup, the same XCD-contiguous walk, the same sum in the same order -- the result is bitwise spaa_warp_fwd_taps of
// the host-painted images.  What differs is where a tap's colour comes from: the shared base image (one 16-byte load per tap for all FB
// candidates; the image is at most 1 MB and stays in cache) unless the tap's projector pixel lies in one of the candidate's squares.
// The candidate vectors are uniform per workgroup and image (scalar loads) and are only compared, never used as addresses.
// HBM traffic = the output: 16 B per camera pixel and candidate (48 B with cat8).
constexpr int OW_W = 32, OW_H = 8, OW_B = 4;
__global__ __launch_bounds__(256) void onepixel_warp_kernel(const float4* __restrict__ base, const int32_t* __restrict__ cand, int P,
                                                            int npix, int d, const int4* __restrict__ src,
                                                            const float4* __restrict__ wgt, const float4* __restrict__ scene,
                                                            float4* __restrict__ xw, float4* __restrict__ cat8, int Wp, int Hc,
                                                            int Wc, int ntx, int ntile) {
    int t;
    {
        const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
        t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    }
    const int tile = t % ntile, b0 = (t / ntile) * OW_B;
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int cy = ty * OW_H + (threadIdx.x >> 5), cx = tx * OW_W + (threadIdx.x & 31);
    if (cy >= Hc || cx >= Wc) return;
    const int pix = cy * Wc + cx;
    const int4 s = src[pix];
    const float4 w = wgt[pix];
    const int si[4] = {s.x, s.y, s.z, s.w};
    const float wi[4] = {w.x, w.y, w.z, w.w};
    float4 bv[4];
    int py[4], px[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool in = si[q] != 0x7fffffff;
        bv[q] = in ? base[si[q]] : make_float4(0.f, 0.f, 0.f, 0.f);
        py[q] = in ? si[q] / Wp : 0;
        px[q] = in ? si[q] - py[q] * Wp : 0;
    }
    float4 sv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cat8 != nullptr) sv = scene[pix];
#pragma unroll
    for (int k = 0; k < OW_B; ++k) {
        if (b0 + k >= P) break;
        const int32_t* cp = cand + (size_t)(b0 + k) * 5 * npix;
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = bv[q];
        for (int j = 0; j < npix; ++j) {
            const int32_t* c = cp + 5 * j;
            const long long r = c[0], cc = c[1];
            const float4 col = make_float4((float)(uint8_t)c[2] / 255.0f, (float)(uint8_t)c[3] / 255.0f, (float)(uint8_t)c[4] / 255.0f, 0.f);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (si[q] != 0x7fffffff && llabs((long long)py[q] - r) <= d && llabs((long long)px[q] - cc) <= d) v[q] = col;
        }
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 u = v[q];
            r0 += u.x * wi[q];
            r1 += u.y * wi[q];
            r2 += u.z * wi[q];
        }
        const size_t o = (size_t)(b0 + k) * Hc * Wc + pix;
        xw[o] = make_float4(r0, r1, r2, 0.f);
        if (cat8 != nullptr) {
            cat8[2 * o] = make_float4(sv.x, sv.y, sv.z, r0 * sv.x);
            cat8[2 * o + 1] = make_float4(r1 * sv.y, r2 * sv.z, 0.f, 0.f);
        }
    }
}

// preproc_fwd_kernel (classifier_ops.hip) with the camera's 8-bit step on every value it reads: Q: v -> (float)(uint8)(v * 255) / 255,
// torch's (y * 255).to(uint8).float() / 255 (truncation; y is PCNet's output, clamped to [0, 1]).  Same window rule and the same sums
// in the same order: bitwise spaa_preproc_fwd of the quantised (Q) or the given (!Q) image.
template <bool Q>
__global__ __launch_bounds__(256) void capture_preproc_kernel(const float4* __restrict__ y, float4* __restrict__ out, int B, int H,
                                                              int W, int cy0, int cx0, int ch, int cw, int oh, int ow, float m0,
                                                              float m1, float m2, float s0, float s1, float s2) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * oh * ow) return;
    const int b = idx / (oh * ow);
    const int r = idx - b * oh * ow;
    const int oy = r / ow, ox = r - oy * ow;
    const int ys = win_start(oy, oh, ch), ye = win_end(oy, oh, ch);
    const int xs = win_start(ox, ow, cw), xe = win_end(ox, ow, cw);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int iy = ys; iy < ye; ++iy) {
        const float4* row = y + ((size_t)b * H + (cy0 + iy)) * W + cx0;
        for (int ix = xs; ix < xe; ++ix) {
            float4 v = row[ix];
            if (Q) {
                v.x = (float)(uint8_t)(int)(v.x * 255.0f) / 255.0f;
                v.y = (float)(uint8_t)(int)(v.y * 255.0f) / 255.0f;
                v.z = (float)(uint8_t)(int)(v.z * 255.0f) / 255.0f;
            }
            a0 += v.x;
            a1 += v.y;
            a2 += v.z;
        }
    }
    const float cnt = (float)((ye - ys) * (xe - xs));
    out[idx] = make_float4((a0 / cnt - m0) / s0, (a1 / cnt - m1) / s1, (a2 / cnt - m2) / s2, 0.f);
}

// One wave per row of logits: max, fixed-order sum of exp(l - max), p_i = exp(l_i - max) / sum.  argmax = the first index of
// the largest p_i (numpy.argmax of the probabilities); energy = p[target] or, targeted, 1 - p[target], in fp32 as the
// reference's numpy float32 arithmetic gives it.
__global__ __launch_bounds__(256) void onepixel_score_kernel(const float* __restrict__ logits, int ncls, int target, int targeted,
                                                             float* __restrict__ energy, int32_t* __restrict__ argmax,
                                                             float* __restrict__ pmax, int P) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= P) return;                         // (whole waves: no shuffle below is left without its partners)
    const float* lg = logits + (size_t)row * ncls;
    float mx = -INFINITY;
    for (int i = lane; i < ncls; i += 64) mx = fmaxf(mx, lg[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    float se = 0.f;
    for (int i = lane; i < ncls; i += 64) se += expf(lg[i] - mx);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) se += __shfl_xor(se, off, 64);
    float best = -1.f;
    int bi = INT_MAX;
    for (int i = lane; i < ncls; i += 64) {
        const float pi = expf(lg[i] - mx) / se;
        if (pi > best) {
            best = pi;
            bi = i;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ob > best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
        }
    }
    if (lane == 0) {
        const float pt = expf(lg[target] - mx) / se;
        energy[row] = targeted ? 1.0f - pt : pt;
        argmax[row] = bi;
        pmax[row] = best;
    }
}

}  // namespace

extern "C" {

int spaa_onepixel_preproc(const float* base, const int32_t* cand, int P, int npix, int pixel_size, float* out, int H, int W,
                          int cy0, int cx0, int ch, int cw, int oh, int ow, const float* mean3, const float* std3,
                          spaa_stream_t stream) {
    if (!base || !cand || !out || !mean3 || !std3 || P < 1 || npix < 1 || pixel_size < 1 || H < 1 || W < 1 || cy0 < 0 ||
        cx0 < 0 || ch < 1 || cw < 1 || cy0 + ch > H || cx0 + cw > W || oh < 1 || ow < 1 || (int64_t)P * oh * ow > INT_MAX)
        return hipErrorInvalidValue;
    const int64_t n = (int64_t)P * oh * ow;
    hipLaunchKernelGGL(onepixel_preproc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)base, cand, P, npix, pixel_size / 2, (float4*)out, W, cy0, cx0, ch, cw, oh, ow, mean3[0],
                       mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    return (int)hipGetLastError();
}

int spaa_onepixel_score(const float* logits, int ncls, int target, int targeted, float* energy, int32_t* argmax, float* pmax,
                        int P, spaa_stream_t stream) {
    if (!logits || !energy || !argmax || !pmax || ncls < 1 || P < 1 || target < 0 || target >= ncls)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(onepixel_score_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, ncls,
                       target, targeted, energy, argmax, pmax, P);
    return (int)hipGetLastError();
}

int spaa_onepixel_warp(const float* base, const int32_t* cand, int P, int npix, int pixel_size, const int32_t* tap_src,
                       const float* tap_wgt, const float* scene, float* xw, float* cat8, int Hp, int Wp, int Hc, int Wc,
                       spaa_stream_t stream) {
    if (!base || !cand || !tap_src || !tap_wgt || !xw || (cat8 && !scene) || P < 1 || npix < 1 || pixel_size < 1 || Hp < 1 || Wp < 1 ||
        Hc < 1 || Wc < 1)
        return hipErrorInvalidValue;
    if ((int64_t)P * Hc * Wc >= ((int64_t)1 << 31) || (int64_t)Hp * Wp >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const int ntx = (Wc + OW_W - 1) / OW_W, nty = (Hc + OW_H - 1) / OW_H;
    const int64_t nwg = (int64_t)ntx * nty * ((P + OW_B - 1) / OW_B);
    if (nwg > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(onepixel_warp_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, (const float4*)base, cand, P, npix,
                       pixel_size / 2, (const int4*)tap_src, (const float4*)tap_wgt, (const float4*)scene, (float4*)xw, (float4*)cat8,
                       Wp, Hc, Wc, ntx, ntx * nty);
    return (int)hipGetLastError();
}

int spaa_capture_preproc(const float* y, float* out, int B, int H, int W, int cy0, int cx0, int ch, int cw, int oh, int ow,
                         const float* mean3, const float* std3, int quantize, spaa_stream_t stream) {
    if (!y || !out || !mean3 || !std3 || B < 1 || H < 1 || W < 1 || cy0 < 0 || cx0 < 0 || ch < 1 || cw < 1 || cy0 + ch > H ||
        cx0 + cw > W || oh < 1 || ow < 1 || (int64_t)B * oh * ow > INT_MAX || (int64_t)B * H * W > INT_MAX)
        return hipErrorInvalidValue;
    const int64_t n = (int64_t)B * oh * ow;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (quantize)
        hipLaunchKernelGGL(capture_preproc_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const float4*)y, (float4*)out, B, H,
                           W, cy0, cx0, ch, cw, oh, ow, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    else
        hipLaunchKernelGGL(capture_preproc_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const float4*)y, (float4*)out, B, H,
                           W, cy0, cx0, ch, cw, oh, ow, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    return (int)hipGetLastError();
}

}  // extern "C"
