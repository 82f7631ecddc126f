// group_ops.hip — SPAA against a group of G classifier passes per sample (2 <= G <= 4): the K members of an ensemble that see the same
// camera image (and, through them, the J draws of the jitter and pose attacks), or one classifier on the V camera views of one projector
// and scene.  The decision step over the group's logits and stealth losses, the combination of the group's input gradients, and the
// best-image tracking of the views after the first.
//
// The per-member tensors arrive as HOST arrays of G device pointers and travel in a by-value kernel argument (ptr_table.hpp).  The
// per-sample tables state [B][4] / stats [B][8] keep the meaning the rest of the loop reads ("Ensemble attack" and
// "Multi-view attack").  All reductions run in a fixed order: no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "device_util.hpp"
#include "decide_util.hpp"
#include "ptr_table.hpp"

namespace {

using GroupIn = PtrTable<const float>;
using GroupOut = PtrTable<float>;

// One workgroup per sample.  Member g: top1, p1, the target logit, succ, fooled and the seed row as decide_kernel computes them
// (decide_util.hpp).  The group looks at `nimg` camera images, each with a loss table of its own: 1 (every member sees image 0: an
// ensemble, draws) or G (member g sees image g: views).  The sample's caml2 / camdE are the means over the images of the per-image
// means (summed in index order; one image: (a / HW) / 1.f, the per-image mean itself).
// state = (AND succ_g, AND fooled_g && high_pert, best, number of fooled members); stats[0] = min p1, stats[6] = mean target logit.
// grp_state [B][G][2] = (succ | fooled << 1, top1); grp_stats [B][G][row] = (p1, target logit) and, where row == 4, the means of
// member g's image.
__global__ __launch_bounds__(256) void decide_group_kernel(const GroupIn logits, int G, int ncls, const int32_t* __restrict__ target,
                                                           const GroupIn partial, int nimg, int nblk, int HW,
                                                           const float* __restrict__ prjl2, const float* __restrict__ params,
                                                           const int32_t* __restrict__ flags, float p_thresh, float seed_mag, int focus,
                                                           int32_t* __restrict__ state, float* __restrict__ stats,
                                                           int32_t* __restrict__ grp_state, float* __restrict__ grp_stats, int row,
                                                           float* __restrict__ grp_w, const GroupOut g_logits) {
    __shared__ DecideLds lds;
    const int b = blockIdx.x;
    const float prjl2_w = params[4 * b], caml2_w = params[4 * b + 1], camdE_w = params[4 * b + 2], d_thr = params[4 * b + 3];
    const int targeted = flags[b] & 1;
    const int tgt = target[b];
    bool all_succ = true;
    int nfooled = 0;
    unsigned fooled_bits = 0;
    float p_min = INFINITY, tl_sum = 0.f, caml2_sum = 0.f, camdE_sum = 0.f;
    float img[5];   // the means of member g's image: caml2 img[1], camdE img[2] (decide_losses with the weights off)
    for (int g = 0; g < G; ++g) {
        const float* lg = ptr_of(logits, g) + (size_t)b * ncls;
        int am;
        float p1;
        decide_top1(lg, ncls, lds, am, p1);
        if (g < nimg) {   // (uniform per workgroup)
            float a, d, col_g;
            decide_loss_sums(ptr_of(partial, g) + 3 * (size_t)b * nblk, nblk, lds, a, d);
            decide_losses(a, d, HW, 0.f, 0.f, 0.f, 0.f, 0.f, img, col_g);
            caml2_sum += img[1];
            camdE_sum += img[2];
        }
        const DecideMember m = decide_member(lg, ncls, tgt, targeted, am, p1, p_thresh, seed_mag, ptr_of(g_logits, g) + (size_t)b * ncls);
        all_succ = all_succ && m.succ;
        nfooled += m.fooled ? 1 : 0;
        fooled_bits |= m.fooled ? (1u << g) : 0u;
        p_min = fminf(p_min, p1);
        tl_sum += m.tl;
        if (threadIdx.x == 0) {
            const size_t r = (size_t)b * G + g;
            grp_state[2 * r] = (m.succ ? 1 : 0) | (m.fooled ? 2 : 0);
            grp_state[2 * r + 1] = am;
            grp_stats[row * r] = p1;
            grp_stats[row * r + 1] = m.tl;
            if (row == 4) {
                grp_stats[row * r + 2] = img[1];
                grp_stats[row * r + 3] = img[2];
            }
        }
    }
    if (threadIdx.x == 0) {
        const float pl2 = (prjl2 != nullptr && prjl2_w != 0.f) ? prjl2[b] : 0.f;
        float* st = stats + 8 * (size_t)b;
        float col;
        // (the sums of the images' means over nimg, as the sum of an image's pixels over HW)
        const bool high_pert = decide_losses(caml2_sum, camdE_sum, nimg, pl2, prjl2_w, caml2_w, camdE_w, d_thr, st, col);
        const bool all_fooled = nfooled == G;
        decide_commit(all_succ, all_fooled, high_pert, col, p_min, tl_sum / (float)G, nfooled, state + 4 * (size_t)b, st);
        // member weights: with `focus`, a fooled member rests -- unless every member is fooled (the sample that succeeds below d_thr
        // keeps taking the adversarial step against all of them)
        for (int g = 0; g < G; ++g)
            grp_w[(size_t)b * G + g] = (focus && !all_fooled && ((fooled_bits >> g) & 1u)) ? 0.f : 1.f;
    }
}

// block partials of ||g_bk||^2 over the three colour channels (the pad channel is not read into the sum).  grid (nblk, K, B)
__global__ __launch_bounds__(256) void ens_sumsq_kernel(const GroupIn g, float* __restrict__ partial, int HW) {
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

// A sample on the colour step (`state` given and state[b][1] != 0): g_out = (sum_g g_bg) * (1 / G).  Any other:
// g_out = sum_g w_bg g_bg / ||g_bg||_2, g in index order, a member with zero norm (or zero weight) contributing 0; every workgroup
// re-reduces its sample's G rows of partial sums in the same fixed order.  16-byte loads and stores, one pixel per lane; pad channel 0.
// grid (nblk, B)
__global__ __launch_bounds__(256) void combine_group_kernel(const GroupIn grad, int G, const float* __restrict__ partial, int nblk,
                                                            const float* __restrict__ grp_w, const int32_t* __restrict__ state,
                                                            float4* __restrict__ g_out, int HW) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const size_t idx = (size_t)b * HW + pix;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (state != nullptr && state[4 * b + 1] != 0) {   // (uniform per workgroup)
        if (pix < HW) {
            for (int g = 0; g < G; ++g) {
                const float4 t = reinterpret_cast<const float4*>(ptr_of(grad, g))[idx];
                acc.x += t.x;
                acc.y += t.y;
                acc.z += t.z;
            }
            const float inv = 1.f / (float)G;
            acc.x *= inv;
            acc.y *= inv;
            acc.z *= inv;
        }
    } else {
        for (int g = 0; g < G; ++g) {
            const float* pp = partial + ((size_t)b * G + g) * nblk;
            float a = 0.f;
            for (int i = threadIdx.x; i < nblk; i += 256) a += pp[i];
            a = block_sum(a, red);
            const float nrm = sqrtf(a);
            const float w = grp_w[(size_t)b * G + g];
            if (pix < HW && nrm > 0.f && w != 0.f) {
                const float4 t = reinterpret_cast<const float4*>(ptr_of(grad, g))[idx];
                acc.x += w * (t.x / nrm);
                acc.y += w * (t.y / nrm);
                acc.z += w * (t.z / nrm);
            }
        }
    }
    if (pix < HW) g_out[idx] = acc;
}

// cam_best_v = cam_v where succ, views 1 .. V-1.  grid (ceil(B HW / 256), V - 1)
__global__ __launch_bounds__(256) void views_track_kernel(const GroupIn cam, const GroupOut cam_best,
                                                          const int32_t* __restrict__ state, int B, int HW) {
    const int v = blockIdx.y + 1;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)B * HW) return;
    const int b = (int)(idx / HW);
    if (state[4 * b] != 0) reinterpret_cast<float4*>(ptr_of(cam_best, v))[idx] = reinterpret_cast<const float4*>(ptr_of(cam, v))[idx];
}

int launch_combine(const GroupIn& in, int G, const float* partial, int nblk, const float* grp_w, const int32_t* state, float* g_out, int B,
                   int HW, spaa_stream_t stream) {
    if (!partial || !grp_w || !g_out || B < 1 || B > 65535 || HW < 1 || nblk != (HW + 255) / 256) return hipErrorInvalidValue;
    hipLaunchKernelGGL(combine_group_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, in, G, partial, nblk, grp_w, state,
                       (float4*)g_out, HW);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int spaa_decide_ens(const float* const* logits, int K, int ncls, const int32_t* target, const float* partial, int nblk, int HW,
                    const float* prjl2, const float* params, const int32_t* flags, float p_thresh, int focus, int32_t* state,
                    float* stats, int32_t* ens_state, float* ens_stats, float* ens_w, float* const* g_logits, int B,
                    spaa_stream_t stream) {
    GroupIn in;
    GroupOut out;
    if (!gather(in, logits, K) || !gather(out, g_logits, K)) return hipErrorInvalidValue;
    if (!target || !partial || !params || !flags || !state || !stats || !ens_state || !ens_stats || !ens_w || B < 1 || ncls < 1 ||
        nblk < 1 || HW < 1)
        return hipErrorInvalidValue;
    // one loss table, member rows of 2 floats, seeds of -/+1
    const GroupIn pt = {{partial, nullptr, nullptr, nullptr}};
    hipLaunchKernelGGL(decide_group_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, in, K, ncls, target, pt, 1, nblk, HW, prjl2,
                       params, flags, p_thresh, 1.f, focus, state, stats, ens_state, ens_stats, 2, ens_w, out);
    return (int)hipGetLastError();
}

int spaa_ens_sumsq(const float* const* g, int K, float* partial, int B, int HW, spaa_stream_t stream) {
    GroupIn in;
    if (!gather(in, g, K) || !partial || B < 1 || B > 65535 || HW < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ens_sumsq_kernel, dim3((HW + 255) / 256, K, B), dim3(256), 0, (hipStream_t)stream, in, partial, HW);
    return (int)hipGetLastError();
}

int spaa_ens_combine(const float* const* g, int K, const float* partial, int nblk, const float* ens_w, float* g_adv, int B, int HW,
                     spaa_stream_t stream) {
    GroupIn in;
    if (!gather(in, g, K)) return hipErrorInvalidValue;
    return launch_combine(in, K, partial, nblk, ens_w, nullptr, g_adv, B, HW, stream);   // (no state: no sample takes the mean branch)
}

int spaa_decide_views(const float* const* logits, int V, int ncls, const int32_t* target, const float* const* partial, int nblk, int HW,
                      const float* prjl2, const float* params, const int32_t* flags, float p_thresh, float adv_scale, int focus,
                      int32_t* state, float* stats, int32_t* view_state, float* view_stats, float* view_w, float* const* g_logits,
                      int B, spaa_stream_t stream) {
    GroupIn lg, pt;
    GroupOut out;
    if (!gather(lg, logits, V) || !gather(pt, partial, V) || !gather(out, g_logits, V)) return hipErrorInvalidValue;
    if (!target || !params || !flags || !state || !stats || !view_state || !view_stats || !view_w || B < 1 || ncls < 1 || nblk < 1 ||
        HW < 1)
        return hipErrorInvalidValue;
    // a loss table per view, view rows of 4 floats, seeds of -/+adv_scale
    hipLaunchKernelGGL(decide_group_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, lg, V, ncls, target, pt, V, nblk, HW, prjl2,
                       params, flags, p_thresh, adv_scale, focus, state, stats, view_state, view_stats, 4, view_w, out);
    return (int)hipGetLastError();
}

int spaa_views_combine(const float* const* g, int V, const float* partial, int nblk, const float* view_w, const int32_t* state,
                       float* g_out, int B, int HW, spaa_stream_t stream) {
    GroupIn in;
    if (!gather(in, g, V) || !state) return hipErrorInvalidValue;
    return launch_combine(in, V, partial, nblk, view_w, state, g_out, B, HW, stream);
}

int spaa_views_track(const float* const* cam, float* const* cam_best, int V, const int32_t* state, int B, int HW, spaa_stream_t stream) {
    GroupIn in;
    GroupOut out;
    if (!gather(in, cam, V, 1) || !gather(out, cam_best, V, 1) || !state || B < 1 || HW < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(views_track_kernel, dim3((unsigned)(((int64_t)B * HW + 255) / 256), V - 1), dim3(256), 0, (hipStream_t)stream, in,
                       out, state, B, HW);
    return (int)hipGetLastError();
}

}  // extern "C"
