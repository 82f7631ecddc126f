// attack_ops.hip — SPAA Algorithm 1's control logic and projected-gradient step, entirely on device.
//
// Replaces (projector_based_attack.py): adversarial loss :269-272, loss reductions :275-287, masks :290-299
// (the reference round-trips to the host three times per iteration: classifier.py:64, :291, :318), gradient
// normalisation and masked updates :302-315, best-so-far bookkeeping :318-328.
//
// Per sample b the reference consumes EITHER g_adv (if not best_adv) OR g_col (if best_adv), never both
// (:307,315), and samples do not interact (no BatchNorm in PCNet, classifier in eval mode).  So one backward pass
// with a per-sample-selected cotangent reproduces both of the reference's backward passes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "device_util.hpp"
#include "decide_util.hpp"

namespace {

// state: [B][4] = succ, best_adv, best, top1      stats: [B][8] = p1, caml2, camdE, col_loss, prjl2, col_loss_best,
// target logit, reserved
__global__ __launch_bounds__(256) void decide_kernel(const float* __restrict__ logits, int ncls,
                                                     const int32_t* __restrict__ target, int targeted,
                                                     const float* __restrict__ partial, int nblk, int HW,
                                                     const float* __restrict__ prjl2, float prjl2_w, float caml2_w,
                                                     float camdE_w, float d_thr, float p_thresh, float adv_scale,
                                                     int32_t* __restrict__ state, float* __restrict__ stats,
                                                     float* __restrict__ g_logits, const float* __restrict__ params,
                                                     const int32_t* __restrict__ flags) {
    __shared__ DecideLds lds;
    const int b = blockIdx.x;
    // spaa_decide_ps: this sample's (prjl2_w, caml2_w, camdE_w, d_thr) and targeted flag replace the scalars (uniform per workgroup)
    if (params != nullptr) {
        prjl2_w = params[4 * b];
        caml2_w = params[4 * b + 1];
        camdE_w = params[4 * b + 2];
        d_thr = params[4 * b + 3];
        targeted = flags[b] & 1;
    }
    const float* lg = logits + (size_t)b * ncls;
    // argmax (first maximum), softmax top-1 probability, the loss sums (fixed order), the success rules (:269-272, :290-299), the
    // seed row and the commit: decide_util.hpp, shared with the group form
    int am;
    float p1, a, d;
    decide_top1(lg, ncls, lds, am, p1);
    decide_loss_sums(partial + 3 * (size_t)b * nblk, nblk, lds, a, d);
    const DecideMember m = decide_member(lg, ncls, target[b], targeted, am, p1, p_thresh, adv_scale, g_logits + (size_t)b * ncls);
    if (threadIdx.x == 0) {
        // (per-sample mode: a sample without the prjl2 term reads 0, as the scalar launch whose caller passes prjl2 = NULL)
        const float pl2 = (prjl2 != nullptr && (params == nullptr || prjl2_w != 0.f)) ? prjl2[b] : 0.f;
        float* st = stats + 8 * (size_t)b;
        float col;
        const bool high_pert = decide_losses(a, d, HW, pl2, prjl2_w, caml2_w, camdE_w, d_thr, st, col);
        decide_commit(m.succ, m.fooled, high_pert, col, p1, m.tl, am, state + 4 * (size_t)b, st);
    }
}

// cotangent at the PCNet output: per-sample choice between the classifier path and the stealth-loss path, then the
// backward of clamp(relu(.), max=1) (models.py:301): pass where 0 < pre <= 1.
__global__ void select_grad_kernel(const float4* __restrict__ g_adv, const float4* __restrict__ g_col,
                                   const int32_t* __restrict__ state, const float4* __restrict__ ypre,
                                   float4* __restrict__ g, int B, int npix) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * npix) return;
    const int b = idx / npix;
    const bool best_adv = state[4 * b + 1] != 0;
    float4 v = best_adv ? g_col[idx] : g_adv[idx];
    if (ypre != nullptr) {
        const float4 y = ypre[idx];
        v.x = (y.x > 0.f && y.x <= 1.f) ? v.x : 0.f;
        v.y = (y.y > 0.f && y.y <= 1.f) ? v.y : 0.f;
        v.z = (y.z > 0.f && y.z <= 1.f) ? v.z : 0.f;
    }
    v.w = 0.f;
    g[idx] = v;
}

// prjl2_b = mean_px || gray - x ||_2   (:275); one workgroup per sample
__global__ __launch_bounds__(256) void prjl2_kernel(const float4* __restrict__ x, float gray,
                                                    float* __restrict__ prjl2, int HW) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    float a = 0.f;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const float4 v = x[(size_t)b * HW + i];
        const float d0 = gray - v.x, d1 = gray - v.y, d2 = gray - v.z;
        a += sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    }
    a = block_sum(a, red);
    if (threadIdx.x == 0) prjl2[b] = a / (float)HW;
}

// Adds the prjl2 gradient to g for samples taking the colour step, and writes block partials of ||g_b||^2.
// grid (nblk, B)
__global__ __launch_bounds__(256) void grad_sumsq_kernel(float4* __restrict__ g, const float4* __restrict__ x,
                                                         float gray, float prjl2_scale,
                                                         const int32_t* __restrict__ state,
                                                         float* __restrict__ partial, int HW,
                                                         const float* __restrict__ prjl2_scales) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    if (prjl2_scales != nullptr) prjl2_scale = prjl2_scales[b];   // spaa_grad_sumsq_ps: per sample (0 = no prjl2 term)
    const int pix = blockIdx.x * 256 + threadIdx.x;
    float ss = 0.f;
    if (pix < HW) {
        const size_t idx = (size_t)b * HW + pix;
        float4 v = g[idx];
        if (prjl2_scale != 0.f && state[4 * b + 1] != 0) {
            const float4 xv = x[idx];
            const float d0 = gray - xv.x, d1 = gray - xv.y, d2 = gray - xv.z;
            const float n = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
            if (n != 0.f) {  // d||gray - x|| / dx = -(gray - x)/n ; zero where the norm is zero (ATen norm_backward)
                const float k = -prjl2_scale / n;
                v.x += k * d0;
                v.y += k * d1;
                v.z += k * d2;
                g[idx] = v;
            }
        }
        ss = v.x * v.x + v.y * v.y + v.z * v.z;
    }
    ss = block_sum(ss, red);
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = ss;
}

// x_b -= lr_b * g_b / ||g_b||  with lr = col_lr if best_adv else adv_lr  (:307,315); then x_best_b = x_b where succ
// (read AFTER the update, Q4).   grid (nblk, B)
__global__ __launch_bounds__(256) void step_kernel(float4* __restrict__ x, const float4* __restrict__ g,
                                                   const float* __restrict__ partial, int nblk,
                                                   const int32_t* __restrict__ state, float adv_lr, float col_lr,
                                                   float4* __restrict__ x_best, int HW, uint8_t* __restrict__ clamp_bits) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    float a = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) a += partial[(size_t)b * nblk + i];
    a = block_sum(a, red);
    const float nrm = sqrtf(a);
    const float lr = (state[4 * b + 1] != 0) ? col_lr : adv_lr;
    const bool succ = state[4 * b] != 0;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    unsigned int bits = 0;
    if (pix < HW) {
        const size_t idx = (size_t)b * HW + pix;
        float4 xv = x[idx];
        const float4 gv = g[idx];
        xv.x -= lr * (gv.x / nrm);
        xv.y -= lr * (gv.y / nrm);
        xv.z -= lr * (gv.z / nrm);
        x[idx] = xv;
        if (succ) x_best[idx] = xv;
        bits = (xv.x >= 0.f && xv.x <= 1.f ? 1u : 0u) | (xv.y >= 0.f && xv.y <= 1.f ? 2u : 0u) | (xv.z >= 0.f && xv.z <= 1.f ? 4u : 0u);
    }
    // the clamp gate of the NEXT iteration's backward pass (x.clamp(0, 1), projector_based_attack.py:265 -> models.py:337): one byte per
    // pixel, bit c = channel c inside [0, 1] -- the grid_sample adjoint then reads 1 byte per pixel instead of x's 16.  Four lanes' bytes
    // leave as one 4-byte store where the image's rows allow it (HW % 4 == 0: every group of four pixels lies in one image, aligned).
    if (clamp_bits != nullptr) {
        if ((HW & 3) == 0) {
            unsigned int w = bits | (__shfl_down(bits, 1, 64) << 8);
            w |= __shfl_down(w, 2, 64) << 16;
            if ((threadIdx.x & 3) == 0 && pix < HW) *reinterpret_cast<unsigned int*>(clamp_bits + (size_t)b * HW + pix) = w;
        } else if (pix < HW) {
            clamp_bits[(size_t)b * HW + pix] = (uint8_t)bits;
        }
    }
}

// cam_infer_best_b = cam_infer_b where succ (:324,328)
__global__ void track_cam_kernel(const float4* __restrict__ cam, float4* __restrict__ cam_best,
                                 const int32_t* __restrict__ state, int B, int HW) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * HW) return;
    const int b = idx / HW;
    if (state[4 * b] != 0) cam_best[idx] = cam[idx];
}

}  // namespace

extern "C" {

static int launch_decide(const float* logits, int ncls, const int32_t* target, int targeted, const float* partial, int nblk,
                         int HW, const float* prjl2, float prjl2_w, float caml2_w, float camdE_w, float d_thr, float p_thresh,
                         float adv_scale, int32_t* state, float* stats, float* g_logits, int B, const float* params,
                         const int32_t* flags, spaa_stream_t stream) {
    if (!logits || !target || !partial || !state || !stats || !g_logits || B < 1 || ncls < 1 || nblk < 1 || HW < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(decide_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ncls, target, targeted,
                       partial, nblk, HW, prjl2, prjl2_w, caml2_w, camdE_w, d_thr, p_thresh, adv_scale, state, stats,
                       g_logits, params, flags);
    return (int)hipGetLastError();
}

int spaa_decide(const float* logits, int ncls, const int32_t* target, int targeted, const float* partial, int nblk,
                int HW, const float* prjl2, float prjl2_w, float caml2_w, float camdE_w, float d_thr, float p_thresh,
                float adv_scale, int32_t* state, float* stats, float* g_logits, int B, spaa_stream_t stream) {
    return launch_decide(logits, ncls, target, targeted, partial, nblk, HW, prjl2, prjl2_w, caml2_w, camdE_w, d_thr, p_thresh,
                         adv_scale, state, stats, g_logits, B, nullptr, nullptr, stream);
}

int spaa_decide_ps(const float* logits, int ncls, const int32_t* target, const float* partial, int nblk, int HW,
                   const float* prjl2, const float* params, const int32_t* flags, float p_thresh, float adv_scale,
                   int32_t* state, float* stats, float* g_logits, int B, spaa_stream_t stream) {
    if (!params || !flags) return hipErrorInvalidValue;
    return launch_decide(logits, ncls, target, 0, partial, nblk, HW, prjl2, 0.f, 0.f, 0.f, 0.f, p_thresh, adv_scale, state, stats,
                         g_logits, B, params, flags, stream);
}

int spaa_select_grad(const float* g_adv, const float* g_col, const int32_t* state, const float* ypre, float* g, int B,
                     int npix, spaa_stream_t stream) {
    if (!g_adv || !g_col || !state || !g || B < 1 || npix < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(select_grad_kernel, dim3((int)(((int64_t)B * npix + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const float4*)g_adv, (const float4*)g_col, state, (const float4*)ypre,
                       (float4*)g, B, npix);
    return (int)hipGetLastError();
}

int spaa_prjl2_fwd(const float* x, float gray, float* prjl2, int B, int HW, spaa_stream_t stream) {
    if (!x || !prjl2 || B < 1 || HW < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prjl2_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const float4*)x, gray, prjl2, HW);
    return (int)hipGetLastError();
}

static int launch_grad_sumsq(float* g, const float* x, float gray, float prjl2_scale, const float* prjl2_scales,
                             const int32_t* state, float* partial, int B, int HW, spaa_stream_t stream) {
    if (!g || !x || !state || !partial || B < 1 || HW < 1) return hipErrorInvalidValue;
    dim3 grid((HW + 255) / 256, B);
    hipLaunchKernelGGL(grad_sumsq_kernel, grid, dim3(256), 0, (hipStream_t)stream, (float4*)g, (const float4*)x, gray,
                       prjl2_scale, state, partial, HW, prjl2_scales);
    return (int)hipGetLastError();
}

int spaa_grad_sumsq(float* g, const float* x, float gray, float prjl2_scale, const int32_t* state, float* partial,
                    int B, int HW, spaa_stream_t stream) {
    return launch_grad_sumsq(g, x, gray, prjl2_scale, nullptr, state, partial, B, HW, stream);
}

int spaa_grad_sumsq_ps(float* g, const float* x, float gray, const float* prjl2_scale, const int32_t* state, float* partial,
                       int B, int HW, spaa_stream_t stream) {
    if (!prjl2_scale) return hipErrorInvalidValue;
    return launch_grad_sumsq(g, x, gray, 0.f, prjl2_scale, state, partial, B, HW, stream);
}

int spaa_step_and_track(float* x, const float* g, const float* partial, const int32_t* state, float adv_lr,
                        float col_lr, float* x_best, const float* cam, float* cam_best, int B, int HWp, int HWc,
                        spaa_stream_t stream) {
    return spaa_step_and_track_n(x, g, partial, (HWp + 255) / 256, state, adv_lr, col_lr, x_best, cam, cam_best, B, HWp, HWc, nullptr, stream);
}

int spaa_step_and_track_n(float* x, const float* g, const float* partial, int npartial, const int32_t* state, float adv_lr,
                          float col_lr, float* x_best, const float* cam, float* cam_best, int B, int HWp, int HWc,
                          uint8_t* clamp_bits, spaa_stream_t stream) {
    if (!x || !g || !partial || !state || !x_best || !cam || !cam_best || B < 1 || HWp < 1 || HWc < 1 || npartial < 1)
        return hipErrorInvalidValue;
    const int nblk = (HWp + 255) / 256;
    dim3 grid(nblk, B);
    hipLaunchKernelGGL(step_kernel, grid, dim3(256), 0, (hipStream_t)stream, (float4*)x, (const float4*)g, partial,
                       npartial, state, adv_lr, col_lr, (float4*)x_best, HWp, clamp_bits);
    hipLaunchKernelGGL(track_cam_kernel, dim3((int)(((int64_t)B * HWc + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const float4*)cam, (float4*)cam_best, state, B, HWc);
    return (int)hipGetLastError();
}

}  // extern "C"
