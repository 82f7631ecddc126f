// decide_util.hpp — the per-sample arithmetic and rules of SPAA's decision step, shared by decide_kernel (attack_ops.hip: one
// classifier) and decide_group_kernel (group_ops.hip: the members of an ensemble, the views or the draws of a sample): a classifier's
// first-maximum arg-max and softmax top-1 probability, the stealth-loss sums with the colour loss built from them, a member's succ /
// fooled rule and seed row, and the sample's best_adv / best rule with the state and stats words.  One copy, so that a member of an
// ensemble, or a view, gets bitwise what spaa_decide / spaa_decide_ps give that classifier and camera image alone.  Workgroups of 256
// threads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_util.hpp"

namespace {

// LDS scratch of the two functions below
struct DecideLds {
    float red[4];
    float s_max[4];
    int s_arg[4];
};

// argmax (first maximum) `am`, and the softmax top-1 probability p1 = 1 / sum exp(l - max) (classifier.py:64) of lg[0 .. ncls);
// both valid in every thread
__device__ __forceinline__ void decide_top1(const float* __restrict__ lg, int ncls, DecideLds& s, int& am, float& p1) {
    float mx = -INFINITY;
    am = 0x7fffffff;
    for (int i = threadIdx.x; i < ncls; i += 256) {
        const float v = lg[i];
        if (v > mx) {
            mx = v;
            am = i;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(mx, off, 64);
        const int oa = __shfl_down(am, off, 64);
        if (ov > mx || (ov == mx && oa < am)) {
            mx = ov;
            am = oa;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s.s_max[wave] = mx;
        s.s_arg[wave] = am;
    }
    __syncthreads();
    mx = s.s_max[0];
    am = s.s_arg[0];
    for (int w = 1; w < 4; ++w) {
        if (s.s_max[w] > mx || (s.s_max[w] == mx && s.s_arg[w] < am)) {
            mx = s.s_max[w];
            am = s.s_arg[w];
        }
    }
    float se = 0.f;
    for (int i = threadIdx.x; i < ncls; i += 256) se += expf(lg[i] - mx);
    se = block_sum(se, s.red);   // (its leading barrier also orders the reads of s_max / s_arg above before a next call's writes)
    p1 = 1.f / se;
}

// sums of the block partials (caml2, camdE, .) of one sample, in fixed order; valid in every thread
__device__ __forceinline__ void decide_loss_sums(const float* __restrict__ pp, int nblk, DecideLds& s, float& a, float& d) {
    a = 0.f;
    d = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) {
        a += pp[3 * i];
        d += pp[3 * i + 1];
    }
    a = block_sum(a, s.red);
    d = block_sum(d, s.red);
}

// stats[1..4] of one sample from the loss sums, and whether its perturbation is above d_thr (one thread).  `pl2`: the sample's prjl2
// (0 when the term is off).
__device__ __forceinline__ bool decide_losses(float a, float d, int HW, float pl2, float prjl2_w, float caml2_w, float camdE_w, float d_thr,
                                              float* __restrict__ st, float& col) {
    const float caml2 = a / (float)HW;
    const float camdE = d / (float)HW;
    col = prjl2_w * pl2;
    col += caml2_w * caml2;
    col += camdE_w * camdE;
    st[1] = caml2;
    st[2] = camdE;
    st[3] = col;
    st[4] = pl2;
    return caml2 * 255.f > d_thr;
}

// One classifier's outcome on one image (the plain form's, an ensemble member's, a view's, a draw's), valid in every thread
struct DecideMember {
    bool succ;     // top-1 is the target (targeted) / is not the true class (untargeted)
    bool fooled;   // succ, and for a targeted sample also confident: p1 > p_thresh
    float tl;      // the target logit
};

// The outcome from decide_top1's `am` and `p1`, and the seed row of this classifier's backward pass:
// d adv_loss / d logits, adv_loss = -/+ logit[target]:  gl[c] = (c == tgt) ? -seed_mag (targeted) / +seed_mag : 0   (all threads)
__device__ __forceinline__ DecideMember decide_member(const float* __restrict__ lg, int ncls, int tgt, int targeted, int am, float p1,
                                                      float p_thresh, float seed_mag, float* __restrict__ gl) {
    DecideMember m;
    m.succ = targeted ? (am == tgt) : (am != tgt);
    m.fooled = targeted ? (m.succ && p1 > p_thresh) : m.succ;
    m.tl = lg[tgt];
    const float seed = targeted ? -seed_mag : seed_mag;
    for (int i = threadIdx.x; i < ncls; i += 256) gl[i] = (i == tgt) ? seed : 0.f;
    return m;
}

// One thread's commit of the sample after decide_losses has filled st[1..4]: best_adv, best and the best colour loss so far (st[5]),
// the four state words s[0..3] and st[0], st[6].  all_succ / all_fooled: over the sample's classifiers (the plain form has one);
// p_stat, tl_stat: p1 and the target logit, or their min / mean over a group; state3: top-1 (plain) or the number fooled (group).
__device__ __forceinline__ void decide_commit(bool all_succ, bool all_fooled, bool high_pert, float col, float p_stat, float tl_stat,
                                              int state3, int32_t* __restrict__ s, float* __restrict__ st) {
    const bool best_adv = all_fooled && high_pert;
    const bool best = best_adv && (col < st[5]);
    if (best) st[5] = col;
    st[0] = p_stat;
    st[6] = tl_stat;
    s[0] = all_succ;
    s[1] = best_adv;
    s[2] = best;
    s[3] = state3;
}

}  // namespace
