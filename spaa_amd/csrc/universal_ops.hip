// universal_ops.hip — universal SPAA: ONE projector image for a group of N scenes (2 <= N <= SPAA_UNIVERSAL_MAX).  A batch of B samples
// is U = B / N groups of N consecutive samples; every sample keeps its own scene, PCNet and classifier pass, and the N rows of a group
// hold the same projector image.  The decision over a group's members and the combination of their N gradient images at the projector
// (DESIGN.md 7q).  The rule is the multi-view attack's (group_ops.hip) with members in the place of views, but the members are rows of
// ordinary [B][...] tensors: strided addressing, no pointer tables, and no serial walk of the members' softmaxes in one workgroup.
//
// The group's four state words and stats[0..6] are written into EACH of its N rows, so that every per-sample kernel downstream
// (spaa_select_grad, spaa_grad_sumsq_ps, the transfer pair, spaa_step_and_track_n) reads the group's decision unchanged.  All
// reductions run in a fixed order: no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "device_util.hpp"
#include "decide_util.hpp"

namespace {

// One workgroup per SAMPLE: top1, p1, the target logit, succ, fooled, the sample's own stealth-loss means and the seed row, each by
// the one copy of that arithmetic in decide_util.hpp (so a member row is bitwise what spaa_decide_ps gives that sample).
// uni_state [B][2] = (succ | fooled << 1, top1); uni_stats [B][4] = (p1, target logit, caml2_b, camdE_b)
__global__ __launch_bounds__(256) void universal_member_kernel(const float* __restrict__ logits, int ncls, const int32_t* __restrict__ target,
                                                               const float* __restrict__ partial, int nblk, int HW,
                                                               const int32_t* __restrict__ flags, float p_thresh, float adv_scale,
                                                               int32_t* __restrict__ uni_state, float* __restrict__ uni_stats,
                                                               float* __restrict__ g_logits) {
    __shared__ DecideLds lds;
    const int b = blockIdx.x;
    const int targeted = flags[b] & 1;
    const float* lg = logits + (size_t)b * ncls;
    int am;
    float p1, a, d;
    decide_top1(lg, ncls, lds, am, p1);
    decide_loss_sums(partial + 3 * (size_t)b * nblk, nblk, lds, a, d);
    const DecideMember m = decide_member(lg, ncls, target[b], targeted, am, p1, p_thresh, adv_scale, g_logits + (size_t)b * ncls);
    if (threadIdx.x == 0) {
        float img[5], col;   // the means of this member's image: caml2 img[1], camdE img[2] (decide_losses with the weights off)
        decide_losses(a, d, HW, 0.f, 0.f, 0.f, 0.f, 0.f, img, col);
        uni_state[2 * (size_t)b] = (m.succ ? 1 : 0) | (m.fooled ? 2 : 0);
        uni_state[2 * (size_t)b + 1] = am;
        float* us = uni_stats + 4 * (size_t)b;
        us[0] = p1;
        us[1] = m.tl;
        us[2] = img[1];
        us[3] = img[2];
    }
}

// One workgroup (one wave) per GROUP u = samples uN .. uN+N-1, whose parameters are uniform: lane i fetches member i's row, lane 0
// walks the N rows in index order (nsucc, nfooled, min p1, the sums of the target logits and of the members' means) and commits the
// group with decide_losses / decide_commit -- group_succ = nsucc >= need and group_fooled = nfooled >= need in the place of "every
// member", prjl2 member 0's (x is shared), stats[5] the group's best colour loss so far (row uN's) -- and lane i writes the group's
// words to row uN + i and the member's weight: 1, or with `focus` 0 for a fooled member unless the group is fooled.
__global__ __launch_bounds__(64) void universal_group_kernel(const int32_t* __restrict__ uni_state, const float* __restrict__ uni_stats,
                                                             const float* __restrict__ prjl2, const float* __restrict__ params, int N,
                                                             int need, int focus, int32_t* __restrict__ state, float* __restrict__ stats,
                                                             float* __restrict__ uni_w) {
    __shared__ int32_t m_bits[SPAA_UNIVERSAL_MAX];
    __shared__ float m_stats[SPAA_UNIVERSAL_MAX][4];
    __shared__ int32_t s_out[4];
    __shared__ float st_out[8];
    __shared__ int s_group_fooled;
    const size_t b0 = (size_t)blockIdx.x * N;
    const int i = threadIdx.x;
    if (i < N) {
        m_bits[i] = uni_state[2 * (b0 + i)];
        const float4 r = reinterpret_cast<const float4*>(uni_stats)[b0 + i];
        m_stats[i][0] = r.x;
        m_stats[i][1] = r.y;
        m_stats[i][2] = r.z;
        m_stats[i][3] = r.w;
    }
    __syncthreads();
    if (i == 0) {
        const float prjl2_w = params[4 * b0], caml2_w = params[4 * b0 + 1], camdE_w = params[4 * b0 + 2], d_thr = params[4 * b0 + 3];
        int nsucc = 0, nfooled = 0;
        float p_min = INFINITY, tl_sum = 0.f, caml2_sum = 0.f, camdE_sum = 0.f;
        for (int k = 0; k < N; ++k) {
            nsucc += m_bits[k] & 1;
            nfooled += (m_bits[k] >> 1) & 1;
            p_min = fminf(p_min, m_stats[k][0]);
            tl_sum += m_stats[k][1];
            caml2_sum += m_stats[k][2];
            camdE_sum += m_stats[k][3];
        }
        const float pl2 = (prjl2 != nullptr && prjl2_w != 0.f) ? prjl2[b0] : 0.f;
        st_out[5] = stats[8 * b0 + 5];
        float col;
        // (the sums of the members' means over N, as the sum of an image's pixels over HW)
        const bool high_pert = decide_losses(caml2_sum, camdE_sum, N, pl2, prjl2_w, caml2_w, camdE_w, d_thr, st_out, col);
        const bool group_fooled = nfooled >= need;
        decide_commit(nsucc >= need, group_fooled, high_pert, col, p_min, tl_sum / (float)N, nfooled, s_out, st_out);
        s_group_fooled = group_fooled ? 1 : 0;
    }
    __syncthreads();
    if (i < N) {
        int32_t* s = state + 4 * (b0 + i);
        float* st = stats + 8 * (b0 + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = s_out[k];
#pragma unroll
        for (int k = 0; k < 7; ++k) st[k] = st_out[k];   // (stats[7] is reserved: not written)
        uni_w[b0 + i] = (focus && !s_group_fooled && ((m_bits[i] >> 1) & 1)) ? 0.f : 1.f;
    }
}

// block partials of ||g_b||^2 over the three colour channels (the pad channel is not read into the sum) for the samples of groups on
// the adversarial step; a colour-step group's coefficients are not read.  grid (nblk, B)
__global__ __launch_bounds__(256) void universal_sumsq_kernel(const float4* __restrict__ g, const int32_t* __restrict__ state,
                                                              float* __restrict__ partial, int HW) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    if (state[4 * (size_t)b + 1] != 0) return;   // (uniform per workgroup)
    const int pix = blockIdx.x * 256 + threadIdx.x;
    float ss = 0.f;
    if (pix < HW) {
        const float4 v = g[(size_t)b * HW + pix];
        ss = v.x * v.x + v.y * v.y + v.z * v.z;
    }
    ss = block_sum(ss, red);
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = ss;
}

// coef_b = uni_w_b / ||g_b||_2 from the sample's nblk partial sums in fixed order; 0 where the norm or the weight is 0 (and for a
// colour-step group, whose combination does not read it).  One workgroup per sample: the combine kernel's workgroups read N
// coefficients, not N x nblk partial sums.
__global__ __launch_bounds__(256) void universal_coef_kernel(const float* __restrict__ partial, int nblk, const float* __restrict__ uni_w,
                                                             const int32_t* __restrict__ state, float* __restrict__ coef) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    if (state[4 * (size_t)b + 1] != 0) {   // (uniform per workgroup)
        if (threadIdx.x == 0) coef[b] = 0.f;
        return;
    }
    float a = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) a += partial[(size_t)b * nblk + i];
    a = block_sum(a, red);
    if (threadIdx.x == 0) {
        const float w = uni_w[b];
        coef[b] = (a > 0.f && w != 0.f) ? w / sqrtf(a) : 0.f;
    }
}

// Group u on the colour step (state[uN][1] != 0): out = (sum_i g_i) * (1 / N); any other: out = sum_i coef_i g_i; members in index
// order, the pad channel 0, the result stored to all N rows of the group.  One pixel per lane with 16-byte loads and stores; the member
// loop runs eight loads ahead of their use.  grid (nblk, U)
constexpr int UNI_AHEAD = 8;

__global__ __launch_bounds__(256) void universal_combine_kernel(const float4* __restrict__ g, int N, const float* __restrict__ coef,
                                                                const int32_t* __restrict__ state, float4* __restrict__ g_out, int HW) {
    __shared__ float c[SPAA_UNIVERSAL_MAX];
    const size_t b0 = (size_t)blockIdx.y * N;
    const bool col_step = state[4 * b0 + 1] != 0;   // (uniform per workgroup)
    // the colour step's sum as the same loop with coefficients of 1
    if ((int)threadIdx.x < N) c[threadIdx.x] = col_step ? 1.f : coef[b0 + threadIdx.x];
    __syncthreads();
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const float4* src = g + b0 * HW + pix;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int i = 0;
    for (; i + UNI_AHEAD <= N; i += UNI_AHEAD) {
        float4 t[UNI_AHEAD];
#pragma unroll
        for (int k = 0; k < UNI_AHEAD; ++k) t[k] = src[(size_t)(i + k) * HW];
#pragma unroll
        for (int k = 0; k < UNI_AHEAD; ++k) {
            const float ck = c[i + k];
            acc.x += ck * t[k].x;
            acc.y += ck * t[k].y;
            acc.z += ck * t[k].z;
        }
    }
    for (; i < N; ++i) {
        const float4 t = src[(size_t)i * HW];
        const float ck = c[i];
        acc.x += ck * t.x;
        acc.y += ck * t.y;
        acc.z += ck * t.z;
    }
    if (col_step) {
        const float inv = 1.f / (float)N;
        acc.x *= inv;
        acc.y *= inv;
        acc.z *= inv;
    }
    float4* dst = g_out + b0 * HW + pix;
    for (i = 0; i < N; ++i) dst[(size_t)i * HW] = acc;
}

bool universal_shape_ok(int N, int B, int HW) {
    return N >= 2 && N <= SPAA_UNIVERSAL_MAX && B >= 1 && B <= 65535 && B % N == 0 && HW >= 1;
}

}  // namespace

extern "C" {

int spaa_decide_universal(const float* logits, int ncls, const int32_t* target, const float* partial, int nblk, int HW, const float* prjl2,
                          const float* params, const int32_t* flags, int N, int need, float p_thresh, float adv_scale, int focus,
                          int32_t* state, float* stats, int32_t* uni_state, float* uni_stats, float* uni_w, float* g_logits, int B,
                          spaa_stream_t stream) {
    if (!logits || !target || !partial || !params || !flags || !state || !stats || !uni_state || !uni_stats || !uni_w || !g_logits)
        return hipErrorInvalidValue;
    if (!universal_shape_ok(N, B, HW) || need < 1 || need > N || ncls < 1 || nblk != (HW + 255) / 256) return hipErrorInvalidValue;
    hipLaunchKernelGGL(universal_member_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ncls, target, partial, nblk, HW, flags,
                       p_thresh, adv_scale, uni_state, uni_stats, g_logits);
    hipLaunchKernelGGL(universal_group_kernel, dim3(B / N), dim3(64), 0, (hipStream_t)stream, uni_state, uni_stats, prjl2, params, N, need,
                       focus, state, stats, uni_w);
    return (int)hipGetLastError();
}

int spaa_universal_combine(const float* g, int N, const float* uni_w, const int32_t* state, float* partial, float* coef, float* g_out,
                           int B, int HW, spaa_stream_t stream) {
    if (!g || !uni_w || !state || !partial || !coef || !g_out || !universal_shape_ok(N, B, HW)) return hipErrorInvalidValue;
    const int nblk = (HW + 255) / 256;
    hipLaunchKernelGGL(universal_sumsq_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, (const float4*)g, state, partial, HW);
    hipLaunchKernelGGL(universal_coef_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, partial, nblk, uni_w, state, coef);
    hipLaunchKernelGGL(universal_combine_kernel, dim3(nblk, B / N), dim3(256), 0, (hipStream_t)stream, (const float4*)g, N, coef, state,
                       (float4*)g_out, HW);
    return (int)hipGetLastError();
}

}  // extern "C"
