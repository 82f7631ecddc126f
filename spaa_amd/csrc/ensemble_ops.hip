// ensemble_ops.hip — SPAA against K classifiers (2 <= K <= SPAA_ENS_MAX) that see the same camera image: the decision step over the
// K members' logits, and the adversarial cotangent  g_adv_b = sum_k a_bk g_bk / ||g_bk||_2  from the members' own gradient images.
//
// The member tensors arrive as HOST arrays of K device pointers (as mean3 / std3 of spaa_preproc_fwd are host pointers) and travel in a
// by-value kernel argument (ptr_table.hpp).
// The per-sample tables state [B][4] / stats [B][8] keep the meaning the rest of the loop reads ("Ensemble attack").
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "device_util.hpp"
#include "decide_util.hpp"
#include "ptr_table.hpp"

namespace {

using EnsIn = PtrTable<const float, SPAA_ENS_MAX>;
using EnsOut = PtrTable<float, SPAA_ENS_MAX>;

// One workgroup per sample.  Member k: top1, p1 and the target logit as decide_kernel computes them (decide_util.hpp);
// succ_k = (top1 == target) if targeted else (top1 != target); fooled_k = succ_k && p1 > p_thresh if targeted else succ_k.
// state = (AND succ_k, AND fooled_k && high_pert, best, number of fooled members); stats[0] = min p1, stats[6] = mean target logit.
__global__ __launch_bounds__(256) void decide_ens_kernel(const EnsIn logits, int K, int ncls, const int32_t* __restrict__ target,
                                                         const float* __restrict__ partial, int nblk, int HW,
                                                         const float* __restrict__ prjl2, const float* __restrict__ params,
                                                         const int32_t* __restrict__ flags, float p_thresh, int focus,
                                                         int32_t* __restrict__ state, float* __restrict__ stats,
                                                         int32_t* __restrict__ ens_state, float* __restrict__ ens_stats,
                                                         float* __restrict__ ens_w, const EnsOut g_logits) {
    __shared__ DecideLds lds;
    const int b = blockIdx.x;
    const float prjl2_w = params[4 * b], caml2_w = params[4 * b + 1], camdE_w = params[4 * b + 2], d_thr = params[4 * b + 3];
    const int targeted = flags[b] & 1;
    const int tgt = target[b];
    const float seed = targeted ? -1.f : 1.f;
    bool all_succ = true;
    int nfooled = 0;
    unsigned fooled_bits = 0;
    float p_min = INFINITY, tl_sum = 0.f;
    for (int k = 0; k < K; ++k) {
        const float* lg = ptr_of(logits, k) + (size_t)b * ncls;
        int am;
        float p1;
        decide_top1(lg, ncls, lds, am, p1);
        const bool succ = targeted ? (am == tgt) : (am != tgt);
        const bool fooled = targeted ? (succ && p1 > p_thresh) : succ;
        const float tl = lg[tgt];
        all_succ = all_succ && succ;
        nfooled += fooled ? 1 : 0;
        fooled_bits |= fooled ? (1u << k) : 0u;
        p_min = fminf(p_min, p1);
        tl_sum += tl;
        if (threadIdx.x == 0) {
            const size_t r = 2 * ((size_t)b * K + k);
            ens_state[r] = (succ ? 1 : 0) | (fooled ? 2 : 0);
            ens_state[r + 1] = am;
            ens_stats[r] = p1;
            ens_stats[r + 1] = tl;
        }
        // the seed of member k's backward pass: g_logits_k[b][c] = (c == target_b) ? -/+1 : 0
        float* gl = ptr_of(g_logits, k) + (size_t)b * ncls;
        for (int i = threadIdx.x; i < ncls; i += 256) gl[i] = (i == tgt) ? seed : 0.f;
    }
    float a, d;
    decide_loss_sums(partial + 3 * (size_t)b * nblk, nblk, lds, a, d);
    if (threadIdx.x == 0) {
        const float pl2 = (prjl2 != nullptr && prjl2_w != 0.f) ? prjl2[b] : 0.f;
        float* st = stats + 8 * (size_t)b;
        float col;
        const bool high_pert = decide_losses(a, d, HW, pl2, prjl2_w, caml2_w, camdE_w, d_thr, st, col);
        const bool all_fooled = nfooled == K;
        const bool best_adv = all_fooled && high_pert;
        const bool best = best_adv && (col < st[5]);
        if (best) st[5] = col;
        st[0] = p_min;
        st[6] = tl_sum / (float)K;
        int32_t* s = state + 4 * (size_t)b;
        s[0] = all_succ;
        s[1] = best_adv;
        s[2] = best;
        s[3] = nfooled;
        // member weights: with `focus`, a fooled member rests -- unless every member is fooled (the sample that succeeds below d_thr
        // keeps taking the adversarial step against all of them)
        for (int k = 0; k < K; ++k)
            ens_w[(size_t)b * K + k] = (focus && !all_fooled && ((fooled_bits >> k) & 1u)) ? 0.f : 1.f;
    }
}

// block partials of ||g_bk||^2 over the three colour channels (the pad channel is not read into the sum).  grid (nblk, K, B)
__global__ __launch_bounds__(256) void ens_sumsq_kernel(const EnsIn g, float* __restrict__ partial, int HW) {
    __shared__ float red[4];
    const int k = blockIdx.y, K = gridDim.y, b = blockIdx.z;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    float ss = 0.f;
    if (pix < HW) {
        const float4 v = reinterpret_cast<const float4*>(ptr_of(g, k))[(size_t)b * HW + pix];
        ss = v.x * v.x + v.y * v.y + v.z * v.z;
    }
    ss = block_sum(ss, red);
    if (threadIdx.x == 0) partial[((size_t)b * K + k) * gridDim.x + blockIdx.x] = ss;
}

// g_adv_b = sum_k a_bk g_bk / ||g_bk||_2, k in index order; a member with zero norm (or zero weight) contributes 0; pad channel 0.
// Every workgroup re-reduces its sample's K rows of partial sums in the same fixed order.  grid (nblk, B)
__global__ __launch_bounds__(256) void ens_combine_kernel(const EnsIn g, int K, const float* __restrict__ partial, int nblk,
                                                          const float* __restrict__ ens_w, float4* __restrict__ g_adv, int HW) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < K; ++k) {
        const float* pp = partial + ((size_t)b * K + k) * nblk;
        float a = 0.f;
        for (int i = threadIdx.x; i < nblk; i += 256) a += pp[i];
        a = block_sum(a, red);
        const float nrm = sqrtf(a);
        const float w = ens_w[(size_t)b * K + k];
        if (pix < HW && nrm > 0.f && w != 0.f) {
            const float4 v = reinterpret_cast<const float4*>(ptr_of(g, k))[(size_t)b * HW + pix];
            acc.x += w * (v.x / nrm);
            acc.y += w * (v.y / nrm);
            acc.z += w * (v.z / nrm);
        }
    }
    if (pix < HW) g_adv[(size_t)b * HW + pix] = acc;
}

}  // namespace

extern "C" {

int spaa_decide_ens(const float* const* logits, int K, int ncls, const int32_t* target, const float* partial, int nblk, int HW,
                    const float* prjl2, const float* params, const int32_t* flags, float p_thresh, int focus, int32_t* state,
                    float* stats, int32_t* ens_state, float* ens_stats, float* ens_w, float* const* g_logits, int B,
                    spaa_stream_t stream) {
    EnsIn in;
    EnsOut out;
    if (!gather(in, logits, K) || !gather(out, g_logits, K)) return hipErrorInvalidValue;
    if (!target || !partial || !params || !flags || !state || !stats || !ens_state || !ens_stats || !ens_w || B < 1 || ncls < 1 ||
        nblk < 1 || HW < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(decide_ens_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, in, K, ncls, target, partial, nblk, HW, prjl2,
                       params, flags, p_thresh, focus, state, stats, ens_state, ens_stats, ens_w, out);
    return (int)hipGetLastError();
}

int spaa_ens_sumsq(const float* const* g, int K, float* partial, int B, int HW, spaa_stream_t stream) {
    EnsIn in;
    if (!gather(in, g, K) || !partial || B < 1 || B > 65535 || HW < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ens_sumsq_kernel, dim3((HW + 255) / 256, K, B), dim3(256), 0, (hipStream_t)stream, in, partial, HW);
    return (int)hipGetLastError();
}

int spaa_ens_combine(const float* const* g, int K, const float* partial, int nblk, const float* ens_w, float* g_adv, int B, int HW,
                     spaa_stream_t stream) {
    EnsIn in;
    if (!gather(in, g, K) || !partial || !ens_w || !g_adv || B < 1 || B > 65535 || HW < 1 || nblk != (HW + 255) / 256)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ens_combine_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, in, K, partial, nblk, ens_w,
                       (float4*)g_adv, HW);
    return (int)hipGetLastError();
}

}  // extern "C"
