// pose_ops.hip — camera-pose jitter for SPAA: J = 2..SPAA_JITTER_MAX copies of one camera image per iteration, each warped
// by a random homography (a few degrees of in-plane rotation, a few percent of zoom, some pixels of translation, a slight tilt), the
// homographies drawn on the device, and the exact adjoint of the warp.
//
//   spaa_pose_draw   the per-(sample, draw) homography rows of iteration t = counter[0]; stores t + 1
//   spaa_pose_fwd    out_j = bilinear(y, H_j m) with zero fill, for all J draws in one launch
//   spaa_pose_bwd    g_y_j = W_j^T g_out_j as a gather over a 5 x 5 window of output pixels (no atomics: bitwise repeatable)
//
// Conventions as in jitter_ops.hip: per-draw tensors are HOST arrays of J device pointers that travel in a by-value kernel argument;
// the generator is jitter's counter-based one with another first constant (tests/pose_oracle.py restates it in Python integers).
// The forward and the adjoint kernel evaluate the source position of an output pixel by ONE function (source_of), so the adjoint's
// weights are the forward's bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "ptr_table.hpp"
#include "draw_rng.hpp"

namespace {

template <typename T>
using Draws = PtrTable<T, SPAA_JITTER_MAX>;

// the word of (seed, t, b, j, parameter index i): jitter's chain behind another first constant, so that a pose table and a jitter
// table of one seed are independent
__device__ __forceinline__ uint32_t draw_word(uint32_t seed, uint32_t t, uint32_t b, uint32_t j, uint32_t i) {
    return draw_word(0x85ebca6bu, seed, t, b, j, i);
}

enum { POSE_ROT = 0, POSE_ZOOM = 1, POSE_TX = 2, POSE_TY = 3, POSE_PX = 4, POSE_PY = 5 };   // parameter indices of the generator

// One workgroup; rows = B * J; R = max(H, W) / 2
__global__ __launch_bounds__(256) void pose_draw_kernel(uint32_t seed, int32_t* __restrict__ counter, float rotate, float zoom,
                                                        float shift, float tilt, int clean0, float* __restrict__ table, int rows, int J,
                                                        float R) {
    const uint32_t t = (uint32_t)counter[0];
    for (int r = threadIdx.x; r < rows; r += 256) {
        const uint32_t b = (uint32_t)(r / J), j = (uint32_t)(r % J);
        float4 lo, hi;
        if (clean0 && j == 0) {
            lo = make_float4(1.f, 0.f, 0.f, 0.f);
            hi = make_float4(1.f, 0.f, 0.f, 0.f);
        } else {
            const float ang = rotate * signed_unit(draw_word(seed, t, b, j, POSE_ROT)) * 0.017453292519943295f;
            const float s = 1.f + zoom * signed_unit(draw_word(seed, t, b, j, POSE_ZOOM));
            const float sc = s * cosf(ang), ss = s * sinf(ang);
            lo = make_float4(sc, -ss, shift * signed_unit(draw_word(seed, t, b, j, POSE_TX)), ss);
            hi = make_float4(sc, shift * signed_unit(draw_word(seed, t, b, j, POSE_TY)),
                             tilt * signed_unit(draw_word(seed, t, b, j, POSE_PX)) / R,
                             tilt * signed_unit(draw_word(seed, t, b, j, POSE_PY)) / R);
        }
        reinterpret_cast<float4*>(table)[2 * (size_t)r] = lo;
        reinterpret_cast<float4*>(table)[2 * (size_t)r + 1] = hi;
    }
    __syncthreads();   // every thread has read t
    if (threadIdx.x == 0) counter[0] = (int32_t)(t + 1u);
}

// Where output pixel (row, col) of an H x W image reads its source under the row (lo, hi) = (h0 h1 h2 h3, h4 h5 h6 h7): the four taps
// (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) with weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy.  `any` is
// false when no tap can lie inside the image (a position off the frame, or not a number): x0, y0 are then not to be used.
struct Source {
    int x0, y0;
    float w00, w01, w10, w11;
    bool any;
};
__device__ __forceinline__ Source source_of(const float4 lo, const float4 hi, int row, int col, int H, int W) {
    const float cx = (float)W * 0.5f, cy = (float)H * 0.5f;
    const float u = (float)col + 0.5f - cx, v = (float)row + 0.5f - cy;
    const float w = fmaf(hi.z, u, fmaf(hi.w, v, 1.f));
    const float xs = fmaf(lo.x, u, fmaf(lo.y, v, lo.z)) / w + (cx - 0.5f);
    const float ys = fmaf(lo.w, u, fmaf(hi.x, v, hi.y)) / w + (cy - 0.5f);
    const float flx = floorf(xs), fly = floorf(ys);
    Source s;
    s.any = flx >= -1.f && flx <= (float)(W - 1) && fly >= -1.f && fly <= (float)(H - 1);   // (false for a NaN)
    s.x0 = s.any ? (int)flx : 0;
    s.y0 = s.any ? (int)fly : 0;
    const float fx = xs - flx, fy = ys - fly;
    const float gx = 1.f - fx, gy = 1.f - fy;
    s.w00 = __fmul_rn(gy, gx);
    s.w01 = __fmul_rn(gy, fx);
    s.w10 = __fmul_rn(fy, gx);
    s.w11 = __fmul_rn(fy, fx);
    return s;
}

__device__ __forceinline__ void add_tap(float4& acc, float w, const float4 v) {
    acc.x = fmaf(w, v.x, acc.x);
    acc.y = fmaf(w, v.y, acc.y);
    acc.z = fmaf(w, v.z, acc.z);
}

// grid (ceil(HW / 256), J, B); one output pixel of one draw per thread
__global__ __launch_bounds__(256) void pose_fwd_kernel(const float4* __restrict__ y, const float4* __restrict__ table,
                                                       const Draws<float> out, int H, int W) {
    const int j = blockIdx.y, J = gridDim.y, b = blockIdx.z;
    const int HW = H * W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const size_t row = (size_t)b * J + j;
    const int i = pix / W, k = pix - i * W;
    const Source s = source_of(table[2 * row], table[2 * row + 1], i, k, H, W);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s.any) {
        const float4* yb = y + (size_t)b * HW;
        const bool x0 = s.x0 >= 0, x1 = s.x0 + 1 < W, y0 = s.y0 >= 0, y1 = s.y0 + 1 < H;   // (x0 >= -1, y0 >= -1 by `any`)
        if (y0 && x0) add_tap(acc, s.w00, yb[s.y0 * W + s.x0]);
        if (y0 && x1) add_tap(acc, s.w01, yb[s.y0 * W + s.x0 + 1]);
        if (y1 && x0) add_tap(acc, s.w10, yb[(s.y0 + 1) * W + s.x0]);
        if (y1 && x1) add_tap(acc, s.w11, yb[(s.y0 + 1) * W + s.x0 + 1]);
    }
    reinterpret_cast<float4*>(ptr_of(out, j))[(size_t)b * HW + pix] = acc;
}

enum { POSE_WINDOW = 2 };   // the adjoint looks at the output pixels within 2 of round(H^-1 p): what the ranges of PoseJitter bound

// grid (ceil(HW / 256), J, B); one input pixel of one draw per thread.  Input pixel p = (r, q) collects g_out[m] w_m(p) over the
// output pixels m of the window around H^-1 p, in row-major order of m; w_m(p) is the forward's weight of tap p at m, 0 when p is
// none of m's taps.
__global__ __launch_bounds__(256) void pose_bwd_kernel(const Draws<const float> g_out, const float4* __restrict__ table,
                                                       const Draws<float> g_y, int H, int W) {
    const int j = blockIdx.y, J = gridDim.y, b = blockIdx.z;
    const int HW = H * W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const size_t row = (size_t)b * J + j;
    const float4 lo = table[2 * row], hi = table[2 * row + 1];
    const int r = pix / W, q = pix - r * W;
    // H^-1 p by the adjugate (its scale cancels in the division)
    const float cx = (float)W * 0.5f, cy = (float)H * 0.5f;
    const float us = (float)q + 0.5f - cx, vs = (float)r + 0.5f - cy;
    const float a = lo.x, bb = lo.y, c = lo.z, d = lo.w, e = hi.x, f = hi.y, g = hi.z, h = hi.w;
    const float mu = (e - f * h) * us + (c * h - bb) * vs + (bb * f - c * e);
    const float mv = (f * g - d) * us + (a - c * g) * vs + (c * d - a * f);
    const float mw = (d * h - e * g) * us + (bb * g - a * h) * vs + (a * e - bb * d);
    const float fc = rintf(mu / mw + (cx - 0.5f)), fr = rintf(mv / mw + (cy - 0.5f));
    // (a centre off the frame by more than the window, or not a number: an empty window)
    const bool near = fc >= -(float)POSE_WINDOW && fc <= (float)(W - 1 + POSE_WINDOW) && fr >= -(float)POSE_WINDOW &&
                      fr <= (float)(H - 1 + POSE_WINDOW);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (near) {
        const int mc = (int)fc, mr = (int)fr;
        const int c_lo = max(mc - POSE_WINDOW, 0), c_hi = min(mc + POSE_WINDOW, W - 1);
        const int r_lo = max(mr - POSE_WINDOW, 0), r_hi = min(mr + POSE_WINDOW, H - 1);
        const float4* gb = reinterpret_cast<const float4*>(ptr_of(g_out, j)) + (size_t)b * HW;
        for (int mi = r_lo; mi <= r_hi; ++mi) {
            for (int mk = c_lo; mk <= c_hi; ++mk) {
                const Source s = source_of(lo, hi, mi, mk, H, W);
                if (!s.any) continue;
                const int dx = q - s.x0, dy = r - s.y0;
                if (dx < 0 || dx > 1 || dy < 0 || dy > 1) continue;
                const float w = dy ? (dx ? s.w11 : s.w10) : (dx ? s.w01 : s.w00);
                add_tap(acc, w, gb[mi * W + mk]);
            }
        }
    }
    reinterpret_cast<float4*>(ptr_of(g_y, j))[(size_t)b * HW + pix] = acc;
}

}  // namespace

extern "C" {

int spaa_pose_draw(uint32_t seed, int32_t* counter, float rotate, float zoom, float shift, float tilt, int clean0, float* table, int B,
                   int J, int H, int W, spaa_stream_t stream) {
    if (!counter || !table || B < 1 || B > (1 << 24) || J < 2 || J > SPAA_JITTER_MAX || H < 1 || W < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pose_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, seed, counter, rotate, zoom, shift, tilt, clean0,
                       table, B * J, J, (float)(H > W ? H : W) * 0.5f);
    return (int)hipGetLastError();
}

int spaa_pose_fwd(const float* y, const float* table, int J, float* const* out, int B, int H, int W, spaa_stream_t stream) {
    Draws<float> o;
    dim3 grid;
    if (!gather(o, out, J) || !y || !table || !image_grid(B, J, H, W, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pose_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float4*)y, (const float4*)table, o, H, W);
    return (int)hipGetLastError();
}

int spaa_pose_bwd(const float* const* g_out, const float* table, int J, float* const* g_y, int B, int H, int W, spaa_stream_t stream) {
    Draws<const float> g;
    Draws<float> o;
    dim3 grid;
    if (!gather(g, g_out, J) || !gather(o, g_y, J) || !table || !image_grid(B, J, H, W, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pose_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, g, (const float4*)table, o, H, W);
    return (int)hipGetLastError();
}

}  // extern "C"
