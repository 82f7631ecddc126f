// jitter_ops.hip — capture jitter for SPAA ("Capture-robust attack"): J = 2..SPAA_JITTER_MAX randomly perturbed copies of one
// camera image per iteration (exposure / white balance, a sub-pixel shift, sensor noise, the 8-bit step), their parameters drawn on the
// device, and the exact adjoint of the transform.
//
//   spaa_jitter_draw   the per-(sample, draw) parameter rows and noise keys of iteration t = counter[0]; stores t + 1
//   spaa_jitter_fwd    out_j = Q(clamp(gain_c S_j(y) + offset + sigma n, 0, 1)) for all J draws in one launch, and the clamp gate
//   spaa_jitter_fwd_each  the same with an input image of its own per draw (behind the pose warp: DESIGN.md 7k)
//   spaa_jitter_bwd    g_y_j = S_j^T(gain_c gate_c g_out_j) as a gather (no atomics: bitwise repeatable)
//
// The per-draw tensors arrive as HOST arrays of J device pointers and travel in a by-value kernel argument, as the ensemble's members do
// (group_ops.hip).  The generator is counter-based: 32-bit integer mixing of (seed, t, b, j, parameter) / (key, pixel, channel), no
// state; tests/jitter_oracle.py restates it in Python integers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "ptr_table.hpp"
#include "draw_rng.hpp"

namespace {

template <typename T>
using Draws = PtrTable<T, SPAA_JITTER_MAX>;

// the word of (seed, t, b, j, parameter index i)
__device__ __forceinline__ uint32_t draw_word(uint32_t seed, uint32_t t, uint32_t b, uint32_t j, uint32_t i) {
    return draw_word(0x9e3779b9u, seed, t, b, j, i);
}

enum { JIT_GAIN = 0, JIT_OFFSET = 3, JIT_DX = 4, JIT_DY = 5, JIT_SIGMA = 6, JIT_KEY = 7 };   // parameter indices = columns of a row

// One workgroup; rows = B * J
__global__ __launch_bounds__(256) void jitter_draw_kernel(uint32_t seed, int32_t* __restrict__ counter, float gain, float offset,
                                                          float shift, float noise, int clean0, float* __restrict__ jit,
                                                          uint32_t* __restrict__ key, int rows, int J) {
    const uint32_t t = (uint32_t)counter[0];
    for (int r = threadIdx.x; r < rows; r += 256) {
        const uint32_t b = (uint32_t)(r / J), j = (uint32_t)(r % J);
        float4 lo, hi;
        if (clean0 && j == 0) {
            lo = make_float4(1.f, 1.f, 1.f, 0.f);
            hi = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            lo.x = 1.f + gain * signed_unit(draw_word(seed, t, b, j, JIT_GAIN));
            lo.y = 1.f + gain * signed_unit(draw_word(seed, t, b, j, JIT_GAIN + 1));
            lo.z = 1.f + gain * signed_unit(draw_word(seed, t, b, j, JIT_GAIN + 2));
            lo.w = offset * signed_unit(draw_word(seed, t, b, j, JIT_OFFSET));
            hi.x = shift * signed_unit(draw_word(seed, t, b, j, JIT_DX));
            hi.y = shift * signed_unit(draw_word(seed, t, b, j, JIT_DY));
            hi.z = noise;
            hi.w = 0.f;
        }
        reinterpret_cast<float4*>(jit)[2 * (size_t)r] = lo;
        reinterpret_cast<float4*>(jit)[2 * (size_t)r + 1] = hi;
        key[r] = draw_word(seed, t, b, j, JIT_KEY);
    }
    __syncthreads();   // every thread has read t
    if (threadIdx.x == 0) counter[0] = (int32_t)(t + 1u);
}

// one axis of S: the taps clamp(m + k), clamp(m + k + 1) with weights 1 - f, f
struct Axis {
    int k;
    float f;
};
__device__ __forceinline__ Axis axis_of(float d) {
    const float fl = floorf(d);
    return Axis{(int)fl, d - fl};
}
__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// a standard normal of (key, pixel, channel) by Box-Muller; u1 in (0, 1] so that the log is finite
__device__ __forceinline__ float normal_of(uint32_t a, uint32_t c) {
    const uint32_t h1 = mix32(a + 2u * c), h2 = mix32(a + 2u * c + 1u);
    const float u1 = (float)((h1 >> 8) + 1u) * 0x1p-24f, u2 = (float)(h2 >> 8) * 0x1p-24f;
    return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// one pixel of one draw per thread: draw j of sample b from the image batch y (grid (ceil(HW / 256), J, B))
__device__ __forceinline__ void jitter_fwd_pixel(const float4* __restrict__ y, const float4* __restrict__ jit,
                                                 const uint32_t* __restrict__ key, int quantize, const Draws<float>& out,
                                                 const Draws<uint8_t>& gate, int H, int W) {
    const int j = blockIdx.y, J = gridDim.y, b = blockIdx.z;
    const int HW = H * W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const size_t row = (size_t)b * J + j;
    const float4 lo = jit[2 * row], hi = jit[2 * row + 1];   // (gain rgb, offset), (dx, dy, sigma, 0)
    const Axis ax = axis_of(hi.x), ay = axis_of(hi.y);
    const int i = pix / W, k = pix - i * W;
    const int r0 = clampi(i + ay.k, H), r1 = clampi(i + ay.k + 1, H);
    const int c0 = clampi(k + ax.k, W), c1 = clampi(k + ax.k + 1, W);
    const float4* yb = y + (size_t)b * HW;
    const float4 v00 = yb[r0 * W + c0], v01 = yb[r0 * W + c1], v10 = yb[r1 * W + c0], v11 = yb[r1 * W + c1];
    const float gx = 1.f - ax.f, gy = 1.f - ay.f;
    // columns first, then rows
    float s[3] = {gy * (gx * v00.x + ax.f * v01.x) + ay.f * (gx * v10.x + ax.f * v11.x),
                  gy * (gx * v00.y + ax.f * v01.y) + ay.f * (gx * v10.y + ax.f * v11.y),
                  gy * (gx * v00.z + ax.f * v01.z) + ay.f * (gx * v10.z + ax.f * v11.z)};
    const float gain[3] = {lo.x, lo.y, lo.z};
    const float sigma = hi.z;
    const uint32_t a = mix32(key[row] ^ ((uint32_t)pix * 0x9e3779b1u));
    unsigned bits = 0;
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float pre = gain[c] * s[c] + lo.w;
        if (sigma != 0.f) pre += sigma * normal_of(a, (uint32_t)c);   // (uniform per workgroup)
        bits |= (pre >= 0.f && pre <= 1.f) ? (1u << c) : 0u;
        float v = fminf(fmaxf(pre, 0.f), 1.f);
        if (quantize) v = floorf(v * 255.f) / 255.f;
        o[c] = v;
    }
    reinterpret_cast<float4*>(ptr_of(out, j))[(size_t)b * HW + pix] = make_float4(o[0], o[1], o[2], 0.f);
    ptr_of(gate, j)[(size_t)b * HW + pix] = (uint8_t)bits;
}

// every draw from the one image batch y
__global__ __launch_bounds__(256) void jitter_fwd_kernel(const float4* __restrict__ y, const float4* __restrict__ jit,
                                                         const uint32_t* __restrict__ key, int quantize, const Draws<float> out,
                                                         const Draws<uint8_t> gate, int H, int W) {
    jitter_fwd_pixel(y, jit, key, quantize, out, gate, H, W);
}

// draw j from its own image batch y[j]
__global__ __launch_bounds__(256) void jitter_fwd_each_kernel(const Draws<const float> y, const float4* __restrict__ jit,
                                                              const uint32_t* __restrict__ key, int quantize, const Draws<float> out,
                                                              const Draws<uint8_t> gate, int H, int W) {
    jitter_fwd_pixel(reinterpret_cast<const float4*>(ptr_of(y, (int)blockIdx.y)), jit, key, quantize, out, gate, H, W);
}

// One axis of S^T as a gather: input index n receives from the output indices m in [lo, hi] those whose clamped taps land on n.
// Interior n: m = n - k - 1 (weight f) and m = n - k (weight 1 - f); the borders also collect every tap clamped onto them.
struct Span {
    int lo, hi;
};
__device__ __forceinline__ Span span_of(int n, int k, int N) {
    const int lo = n == 0 ? 0 : n - k - 1, hi = n == N - 1 ? N - 1 : n - k;
    return Span{lo < 0 ? 0 : lo, hi > N - 1 ? N - 1 : hi};
}
__device__ __forceinline__ float tap_weight(int m, int n, Axis a, int N) {
    return (clampi(m + a.k, N) == n ? 1.f - a.f : 0.f) + (clampi(m + a.k + 1, N) == n ? a.f : 0.f);
}

// grid (ceil(HW / 256), J, B); one input pixel of one draw per thread
__global__ __launch_bounds__(256) void jitter_bwd_kernel(const Draws<const float> g_out, const float4* __restrict__ jit,
                                                         const Draws<const uint8_t> gate, const Draws<float> g_y, int H, int W) {
    const int j = blockIdx.y, J = gridDim.y, b = blockIdx.z;
    const int HW = H * W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const size_t row = (size_t)b * J + j;
    const float4 lo = jit[2 * row], hi = jit[2 * row + 1];
    const Axis ax = axis_of(hi.x), ay = axis_of(hi.y);
    const int r = pix / W, q = pix - r * W;
    const Span sr = span_of(r, ay.k, H), sq = span_of(q, ax.k, W);
    const float4* gb = reinterpret_cast<const float4*>(ptr_of(g_out, j)) + (size_t)b * HW;
    const uint8_t* tb = ptr_of(gate, j) + (size_t)b * HW;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int mi = sr.lo; mi <= sr.hi; ++mi) {
        const float wr = tap_weight(mi, r, ay, H);
        float4 line = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int mk = sq.lo; mk <= sq.hi; ++mk) {
            const float wq = tap_weight(mk, q, ax, W);
            const float4 g = gb[mi * W + mk];
            const unsigned bits = tb[mi * W + mk];
            line.x += wq * ((bits & 1u) ? lo.x * g.x : 0.f);
            line.y += wq * ((bits & 2u) ? lo.y * g.y : 0.f);
            line.z += wq * ((bits & 4u) ? lo.z * g.z : 0.f);
        }
        acc.x += wr * line.x;
        acc.y += wr * line.y;
        acc.z += wr * line.z;
    }
    reinterpret_cast<float4*>(ptr_of(g_y, j))[(size_t)b * HW + pix] = acc;
}

}  // namespace

extern "C" {

int spaa_jitter_draw(uint32_t seed, int32_t* counter, float gain, float offset, float shift, float noise, int clean0, float* jit,
                     uint32_t* key, int B, int J, spaa_stream_t stream) {
    if (!counter || !jit || !key || B < 1 || B > (1 << 24) || J < 2 || J > SPAA_JITTER_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jitter_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, seed, counter, gain, offset, shift, noise,
                       clean0, jit, key, B * J, J);
    return (int)hipGetLastError();
}

int spaa_jitter_fwd(const float* y, const float* jit, const uint32_t* key, int J, int quantize, float* const* out,
                    uint8_t* const* gate, int B, int H, int W, spaa_stream_t stream) {
    Draws<float> o;
    Draws<uint8_t> gt;
    dim3 grid;
    if (!gather(o, out, J) || !gather(gt, gate, J) || !y || !jit || !key || !image_grid(B, J, H, W, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jitter_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float4*)y, (const float4*)jit, key, quantize,
                       o, gt, H, W);
    return (int)hipGetLastError();
}

int spaa_jitter_fwd_each(const float* const* y, const float* jit, const uint32_t* key, int J, int quantize, float* const* out,
                         uint8_t* const* gate, int B, int H, int W, spaa_stream_t stream) {
    Draws<const float> in;
    Draws<float> o;
    Draws<uint8_t> gt;
    dim3 grid;
    if (!gather(in, y, J) || !gather(o, out, J) || !gather(gt, gate, J) || !jit || !key || !image_grid(B, J, H, W, grid))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(jitter_fwd_each_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, (const float4*)jit, key, quantize, o, gt, H,
                       W);
    return (int)hipGetLastError();
}

int spaa_jitter_bwd(const float* const* g_out, const float* jit, const uint8_t* const* gate, int J, float* const* g_y, int B, int H,
                    int W, spaa_stream_t stream) {
    Draws<const float> g;
    Draws<const uint8_t> gt;
    Draws<float> o;
    dim3 grid;
    if (!gather(g, g_out, J) || !gather(gt, gate, J) || !gather(o, g_y, J) || !jit || !image_grid(B, J, H, W, grid))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(jitter_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, g, (const float4*)jit, gt, o, H, W);
    return (int)hipGetLastError();
}

}  // extern "C"
