// multiview_ops.hip — SPAA against V camera views (2 <= V <= SPAA_VIEWS_MAX) of one projector and scene: the decision step over the V
// views' logits and stealth losses, the combination of the V input gradients at the projector image, and the best-image tracking of
// the views after the first.
//
// Per-view tensors arrive as HOST arrays of V device pointers and travel in a by-value kernel argument (ptr_table.hpp).  The per-sample tables state [B][4] / stats [B][8] keep the meaning the rest
// of the loop reads ("Multi-view attack").  All reductions run in a fixed order: no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "device_util.hpp"
#include "decide_util.hpp"
#include "ptr_table.hpp"

namespace {

using ViewsIn = PtrTable<const float, SPAA_VIEWS_MAX>;
using ViewsOut = PtrTable<float, SPAA_VIEWS_MAX>;

// One workgroup per sample.  View v: top1, p1, the target logit and the loss means as decide_kernel computes them (decide_util.hpp);
// succ_v = (top1 == target) if targeted else (top1 != target); fooled_v = succ_v && p1 > p_thresh if targeted else succ_v.
// The sample's caml2 / camdE are the means over the views (summed in index order); state = (AND succ_v, AND fooled_v && high_pert,
// best, number of fooled views); stats[0] = min p1, stats[6] = mean target logit.
__global__ __launch_bounds__(256) void decide_views_kernel(const ViewsIn logits, int V, int ncls, const int32_t* __restrict__ target,
                                                           const ViewsIn partial, int nblk, int HW, const float* __restrict__ prjl2,
                                                           const float* __restrict__ params, const int32_t* __restrict__ flags,
                                                           float p_thresh, float adv_scale, int focus, int32_t* __restrict__ state,
                                                           float* __restrict__ stats, int32_t* __restrict__ view_state,
                                                           float* __restrict__ view_stats, float* __restrict__ view_w,
                                                           const ViewsOut g_logits) {
    __shared__ DecideLds lds;
    const int b = blockIdx.x;
    const float prjl2_w = params[4 * b], caml2_w = params[4 * b + 1], camdE_w = params[4 * b + 2], d_thr = params[4 * b + 3];
    const int targeted = flags[b] & 1;
    const int tgt = target[b];
    const float seed = targeted ? -adv_scale : adv_scale;
    bool all_succ = true;
    int nfooled = 0;
    unsigned fooled_bits = 0;
    float p_min = INFINITY, tl_sum = 0.f, caml2_sum = 0.f, camdE_sum = 0.f;
    for (int v = 0; v < V; ++v) {
        const float* lg = ptr_of(logits, v) + (size_t)b * ncls;
        int am;
        float p1, a, d;
        decide_top1(lg, ncls, lds, am, p1);
        decide_loss_sums(ptr_of(partial, v) + 3 * (size_t)b * nblk, nblk, lds, a, d);
        // this view's means caml2_v, camdE_v (decide_losses with the weights off: tmp[1], tmp[2])
        float tmp[5], col_v;
        decide_losses(a, d, HW, 0.f, 0.f, 0.f, 0.f, 0.f, tmp, col_v);
        const bool succ = targeted ? (am == tgt) : (am != tgt);
        const bool fooled = targeted ? (succ && p1 > p_thresh) : succ;
        const float tl = lg[tgt];
        all_succ = all_succ && succ;
        nfooled += fooled ? 1 : 0;
        fooled_bits |= fooled ? (1u << v) : 0u;
        p_min = fminf(p_min, p1);
        tl_sum += tl;
        caml2_sum += tmp[1];
        camdE_sum += tmp[2];
        if (threadIdx.x == 0) {
            const size_t r = (size_t)b * V + v;
            view_state[2 * r] = (succ ? 1 : 0) | (fooled ? 2 : 0);
            view_state[2 * r + 1] = am;
            view_stats[4 * r] = p1;
            view_stats[4 * r + 1] = tl;
            view_stats[4 * r + 2] = tmp[1];
            view_stats[4 * r + 3] = tmp[2];
        }
        // the seed of view v's classifier backward pass, as decide_kernel writes it
        float* gl = ptr_of(g_logits, v) + (size_t)b * ncls;
        for (int i = threadIdx.x; i < ncls; i += 256) gl[i] = (i == tgt) ? seed : 0.f;
    }
    if (threadIdx.x == 0) {
        const float pl2 = (prjl2 != nullptr && prjl2_w != 0.f) ? prjl2[b] : 0.f;
        float* st = stats + 8 * (size_t)b;
        float col;
        // (the sums of the views' means over V, as the sum of a view's pixels over HW)
        const bool high_pert = decide_losses(caml2_sum, camdE_sum, V, pl2, prjl2_w, caml2_w, camdE_w, d_thr, st, col);
        const bool all_fooled = nfooled == V;
        const bool best_adv = all_fooled && high_pert;
        const bool best = best_adv && (col < st[5]);
        if (best) st[5] = col;
        st[0] = p_min;
        st[6] = tl_sum / (float)V;
        int32_t* s = state + 4 * (size_t)b;
        s[0] = all_succ;
        s[1] = best_adv;
        s[2] = best;
        s[3] = nfooled;
        // view weights: with `focus`, a fooled view rests -- unless every view is fooled (the sample that succeeds below d_thr keeps
        // taking the adversarial step against all of them)
        for (int v = 0; v < V; ++v)
            view_w[(size_t)b * V + v] = (focus && !all_fooled && ((fooled_bits >> v) & 1u)) ? 0.f : 1.f;
    }
}

// Colour-step sample: g_out = (sum_v g_v) * (1 / V).  Any other: g_out = sum_v w_bv g_bv / ||g_bv||_2, v in index order, a view with
// zero norm (or zero weight) contributing 0; every workgroup re-reduces its sample's V rows of partial sums in the same fixed order.
// 16-byte loads and stores, one pixel per lane; pad channel 0.  grid (nblk, B)
__global__ __launch_bounds__(256) void views_combine_kernel(const ViewsIn g, int V, const float* __restrict__ partial, int nblk,
                                                            const float* __restrict__ view_w, const int32_t* __restrict__ state,
                                                            float4* __restrict__ g_out, int HW) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const size_t idx = (size_t)b * HW + pix;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (state[4 * b + 1] != 0) {   // (uniform per workgroup)
        if (pix < HW) {
            for (int v = 0; v < V; ++v) {
                const float4 t = reinterpret_cast<const float4*>(ptr_of(g, v))[idx];
                acc.x += t.x;
                acc.y += t.y;
                acc.z += t.z;
            }
            const float inv = 1.f / (float)V;
            acc.x *= inv;
            acc.y *= inv;
            acc.z *= inv;
        }
    } else {
        for (int v = 0; v < V; ++v) {
            const float* pp = partial + ((size_t)b * V + v) * nblk;
            float a = 0.f;
            for (int i = threadIdx.x; i < nblk; i += 256) a += pp[i];
            a = block_sum(a, red);
            const float nrm = sqrtf(a);
            const float w = view_w[(size_t)b * V + v];
            if (pix < HW && nrm > 0.f && w != 0.f) {
                const float4 t = reinterpret_cast<const float4*>(ptr_of(g, v))[idx];
                acc.x += w * (t.x / nrm);
                acc.y += w * (t.y / nrm);
                acc.z += w * (t.z / nrm);
            }
        }
    }
    if (pix < HW) g_out[idx] = acc;
}

// cam_best_v = cam_v where succ, views 1 .. V-1.  grid (ceil(B HW / 256), V - 1)
__global__ __launch_bounds__(256) void views_track_kernel(const ViewsIn cam, const ViewsOut cam_best,
                                                          const int32_t* __restrict__ state, int B, int HW) {
    const int v = blockIdx.y + 1;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)B * HW) return;
    const int b = (int)(idx / HW);
    if (state[4 * b] != 0) reinterpret_cast<float4*>(ptr_of(cam_best, v))[idx] = reinterpret_cast<const float4*>(ptr_of(cam, v))[idx];
}

}  // namespace

extern "C" {

int spaa_decide_views(const float* const* logits, int V, int ncls, const int32_t* target, const float* const* partial, int nblk, int HW,
                      const float* prjl2, const float* params, const int32_t* flags, float p_thresh, float adv_scale, int focus,
                      int32_t* state, float* stats, int32_t* view_state, float* view_stats, float* view_w, float* const* g_logits,
                      int B, spaa_stream_t stream) {
    ViewsIn lg, pt;
    ViewsOut out;
    if (!gather(lg, logits, V) || !gather(pt, partial, V) || !gather(out, g_logits, V)) return hipErrorInvalidValue;
    if (!target || !params || !flags || !state || !stats || !view_state || !view_stats || !view_w || B < 1 || ncls < 1 || nblk < 1 ||
        HW < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(decide_views_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, lg, V, ncls, target, pt, nblk, HW, prjl2,
                       params, flags, p_thresh, adv_scale, focus, state, stats, view_state, view_stats, view_w, out);
    return (int)hipGetLastError();
}

int spaa_views_combine(const float* const* g, int V, const float* partial, int nblk, const float* view_w, const int32_t* state,
                       float* g_out, int B, int HW, spaa_stream_t stream) {
    ViewsIn in;
    if (!gather(in, g, V) || !partial || !view_w || !state || !g_out || B < 1 || B > 65535 || HW < 1 || nblk != (HW + 255) / 256)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(views_combine_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, in, V, partial, nblk, view_w, state,
                       (float4*)g_out, HW);
    return (int)hipGetLastError();
}

int spaa_views_track(const float* const* cam, float* const* cam_best, int V, const int32_t* state, int B, int HW, spaa_stream_t stream) {
    ViewsIn in;
    ViewsOut out;
    if (!gather(in, cam, V, 1) || !gather(out, cam_best, V, 1) || !state || B < 1 || HW < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(views_track_kernel, dim3((unsigned)(((int64_t)B * HW + 255) / 256), V - 1), dim3(256), 0, (hipStream_t)stream, in,
                       out, state, B, HW);
    return (int)hipGetLastError();
}

}  // extern "C"
