// onepixel.hip — the per-candidate work of the One-pixel DE attacker (one_pixel_attacker/__init__.py:18-99 in the reference:
// DigitalOnePixelAttacker.perturb_and_predict / predict_fn), around the classifier body's forward pass:
//   spaa_onepixel_preproc   perturb_image (paint the candidate squares, :18-44) fused into the classifier's gather: center crop
//                           + area resize + Normalize (classifier.py:59), written straight into the body's input
//   spaa_onepixel_score     softmax (classifier.py:64) -> the DE energy p[target] / 1 - p[target] (:91-95) and numpy's
//                           argmax of p (:68-72), so only three numbers per candidate leave the device
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

}  // extern "C"
