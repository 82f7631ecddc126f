// blur_ops.hip — lens blur for SPAA: J = 2..SPAA_JITTER_MAX defocused copies of one camera image per iteration, each
// through a separable Gaussian of its own sigma with replicated border, the sigmas drawn on the device, and the exact transpose.
//
//   spaa_blur_rows   the tap rows of n given sigmas
//   spaa_blur_draw   the tap rows of iteration t = counter[0]; stores t + 1
//   spaa_blur_fwd    out_j = G_j(y_j), both passes of a 32 x 16 tile through LDS, one launch
//   spaa_blur_bwd    g_y_j = G_j^T(g_out_j) as a gather: the taps that left the frame fold back into the edge pixel, one launch
//
// A workgroup owns one tile of ONE (sample, draw): the radius and the taps are workgroup-uniform, so they are scalar loads and the tap
// loops have a uniform trip count.  The LDS tiles are channel-planar (as ssim_ops.hip's): lanes that are neighbours in x read
// neighbouring floats.  tests/blur_oracle.py restates all of it in Python integers and float64.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "ptr_table.hpp"
#include "draw_rng.hpp"

namespace {

template <typename T>
using Draws = PtrTable<T, SPAA_JITTER_MAX>;

constexpr int RMAX = SPAA_BLUR_RMAX, ROW = 12;                    // floats of a row: sigma, r, w_0 .. w_RMAX, 0
constexpr int TW = SPAA_BLUR_TILE_W, TH = SPAA_BLUR_TILE_H;       // the tile of a workgroup
constexpr int IW = TW + 2 * RMAX, IH = TH + 2 * RMAX;             // the tile with the widest halo
static_assert(ROW == RMAX + 4 && TW == 32 && TH == 16, "the row layout and the index arithmetic below");

// The row of one sigma: the ONE place where a radius and taps are made (spaa_blur_rows and spaa_blur_draw).
__device__ __forceinline__ void blur_row_of(float sigma, float* __restrict__ row) {
    float w[RMAX + 1];
    int r = 0;
    if (!(sigma > 0.f)) {
        sigma = 0.f;
    } else {
        r = (int)fminf(ceilf(3.0f * sigma), (float)RMAX);
    }
    w[0] = 1.f;   // (set, not computed: -0 / (2 sigma^2) is 0 / 0 for a tiny sigma)
    float side = 0.f;
#pragma unroll
    for (int i = 1; i <= RMAX; ++i) {
        w[i] = i <= r ? expf(-(float)(i * i) / (2.f * sigma * sigma)) : 0.f;
        side += w[i];
    }
    const float norm = w[0] + 2.f * side;
    float4* out = reinterpret_cast<float4*>(row);
    out[0] = make_float4(sigma, (float)r, w[0] / norm, w[1] / norm);
    out[1] = make_float4(w[2] / norm, w[3] / norm, w[4] / norm, w[5] / norm);
    out[2] = make_float4(w[6] / norm, w[7] / norm, w[8] / norm, 0.f);
}

__global__ __launch_bounds__(256) void blur_rows_kernel(const float* __restrict__ sigma, float* __restrict__ row, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) blur_row_of(sigma[i], row + (size_t)i * ROW);
}

// One workgroup; rows = B * J
__global__ __launch_bounds__(256) void blur_draw_kernel(uint32_t seed, int32_t* __restrict__ counter, float lo, float hi, int clean0,
                                                        float* __restrict__ row, int rows, int J) {
    const uint32_t t = (uint32_t)counter[0];
    for (int q = threadIdx.x; q < rows; q += 256) {
        const uint32_t b = (uint32_t)(q / J), j = (uint32_t)(q % J);
        float sigma = 0.f;
        if (!(clean0 && j == 0)) {
            const float u = (float)(draw_word(0x2545f491u, seed, t, b, j, 0u) >> 8) * 0x1p-24f;
            sigma = __fmaf_rn(hi - lo, u, lo);
        }
        blur_row_of(sigma, row + (size_t)q * ROW);
    }
    __syncthreads();   // every thread has read t
    if (threadIdx.x == 0) counter[0] = (int32_t)(t + 1u);
}

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// the radius and the taps of the workgroup's row (uniform: scalar loads)
struct Taps {
    int r;
    float w[RMAX + 1];
    float tail[RMAX + 1];   // tail[m] = w_m + .. + w_r, summed from the far end (the transpose's fold)
};
__device__ __forceinline__ Taps taps_of(const float* __restrict__ rw) {
    Taps t;
    const int r = (int)rw[1];
    t.r = r < 0 ? 0 : (r > RMAX ? RMAX : r);
#pragma unroll
    for (int i = 0; i <= RMAX; ++i) t.w[i] = i <= t.r ? rw[2 + i] : 0.f;
    t.tail[RMAX] = t.w[RMAX];
#pragma unroll
    for (int i = RMAX - 1; i >= 0; --i) t.tail[i] = t.w[i] + t.tail[i + 1];
    return t;
}

// w_0 c + sum_i w_i (line[-i] + line[+i]), i ascending: `line` points at the centre, `stride` floats between neighbours
__device__ __forceinline__ float filter_at(const float* line, int stride, const Taps& t) {
    float acc = t.w[0] * line[0];
#pragma unroll
    for (int i = 1; i <= RMAX; ++i) {
        if (i > t.r) break;   // (uniform)
        acc += t.w[i] * (line[-i * stride] + line[i * stride]);
    }
    return acc;
}

// grid (tiles, J, B); tile (ty0, tx0) of draw j of sample b
__global__ __launch_bounds__(256) void blur_fwd_kernel(const Draws<const float> y, const float* __restrict__ row, const Draws<float> out,
                                                       int H, int W, int tiles_x) {
    __shared__ float s_in[3][IH][IW];    // the tile with its halo, indices clamped into the image (= replicated border)
    __shared__ float s_mid[3][IH][TW];   // after the pass along the rows
    const int j = blockIdx.y, J = gridDim.y, b = blockIdx.z, tid = threadIdx.x;
    const int ty0 = ((int)blockIdx.x / tiles_x) * TH, tx0 = ((int)blockIdx.x % tiles_x) * TW;
    const Taps t = taps_of(row + ((size_t)b * J + j) * ROW);
    const int r = t.r, eh = TH + 2 * r, ew = TW + 2 * r;
    const size_t HW = (size_t)H * W;
    const float4* yb = reinterpret_cast<const float4*>(ptr_of(y, j)) + (size_t)b * HW;
    for (int idx = tid; idx < eh * ew; idx += 256) {
        const int ly = idx / ew, lx = idx - ly * ew;
        const float4 v = yb[clampi(ty0 - r + ly, H) * W + clampi(tx0 - r + lx, W)];
        s_in[0][ly][lx] = v.x;
        s_in[1][ly][lx] = v.y;
        s_in[2][ly][lx] = v.z;
    }
    __syncthreads();
    for (int idx = tid; idx < eh * TW; idx += 256) {
        const int ly = idx / TW, tx = idx % TW;
#pragma unroll
        for (int c = 0; c < 3; ++c) s_mid[c][ly][tx] = filter_at(&s_in[c][ly][tx + r], 1, t);
    }
    __syncthreads();
    float4* ob = reinterpret_cast<float4*>(ptr_of(out, j)) + (size_t)b * HW;
    for (int idx = tid; idx < TH * TW; idx += 256) {
        const int ty = idx / TW, tx = idx % TW;
        if (ty0 + ty >= H || tx0 + tx >= W) continue;
        float o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = filter_at(&s_mid[c][ty + r][tx], TW, t);
        ob[(ty0 + ty) * W + tx0 + tx] = make_float4(o[0], o[1], o[2], 0.f);
    }
}

// One axis of the transpose at index p of n.  `line` points at local index 0 of an LDS line, `stride` floats apart, that holds g at the
// indices base .. and 0 where those are outside [0, n); the line reaches r beyond the tile on both sides.  An interior p takes z_p.
// The edges take the fold: sum_{e = -r .. 0} z_e = sum_{m = 0 .. r} T_m g_m with the tail sums T_m = w_m + .. + w_r (each g_m counted once
// with everything it sent beyond the frame: the same sum as the header's, regrouped so that an edge pixel costs r + 1 products and
// not (r + 1)(2 r + 1)), mirrored at n - 1; n == 1 takes both folds less the z_0 they share.  Every index read lies within r of p.
__device__ __forceinline__ float transpose_at(const float* line, int stride, int base, int p, int n, const Taps& t) {
    const float* at = line + (p - base) * stride;
    if (p > 0 && p < n - 1) return filter_at(at, stride, t);
    if (n == 1) return (t.tail[0] + t.tail[0] - t.w[0]) * at[0];   // (the identity row: (1 + 1 - 1) g, bit for bit)
    const int step = p == 0 ? stride : -stride;
    float acc = t.tail[0] * at[0];
#pragma unroll
    for (int m = 1; m <= RMAX; ++m) {
        if (m > t.r) break;   // (uniform)
        acc += t.tail[m] * at[m * step];
    }
    return acc;
}

// grid (tiles, J, B); tile (ty0, tx0) of the input gradient of draw j of sample b
__global__ __launch_bounds__(256) void blur_bwd_kernel(const Draws<const float> g_out, const float* __restrict__ row,
                                                       const Draws<float> g_y, int H, int W, int tiles_x) {
    __shared__ float s_in[3][IH][IW];    // g_out over the tile with its halo, 0 outside the image
    __shared__ float s_mid[3][TH][IW];   // after the transpose along the columns: the tile's rows, every column of the halo
    const int j = blockIdx.y, J = gridDim.y, b = blockIdx.z, tid = threadIdx.x;
    const int ty0 = ((int)blockIdx.x / tiles_x) * TH, tx0 = ((int)blockIdx.x % tiles_x) * TW;
    const Taps t = taps_of(row + ((size_t)b * J + j) * ROW);
    const int r = t.r, eh = TH + 2 * r, ew = TW + 2 * r;
    const size_t HW = (size_t)H * W;
    const float4* gb = reinterpret_cast<const float4*>(ptr_of(g_out, j)) + (size_t)b * HW;
    for (int idx = tid; idx < eh * ew; idx += 256) {
        const int ly = idx / ew, lx = idx - ly * ew;
        const int gy = ty0 - r + ly, gx = tx0 - r + lx;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = gb[gy * W + gx];
        s_in[0][ly][lx] = v.x;
        s_in[1][ly][lx] = v.y;
        s_in[2][ly][lx] = v.z;
    }
    __syncthreads();
    for (int idx = tid; idx < TH * ew; idx += 256) {
        const int ty = idx / ew, lx = idx - ty * ew;
        const int p = ty0 + ty;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            s_mid[c][ty][lx] = p < H ? transpose_at(&s_in[c][0][lx], IW, ty0 - r, p, H, t) : 0.f;
    }
    __syncthreads();
    float4* ob = reinterpret_cast<float4*>(ptr_of(g_y, j)) + (size_t)b * HW;
    for (int idx = tid; idx < TH * TW; idx += 256) {
        const int ty = idx / TW, tx = idx % TW;
        const int p = tx0 + tx;
        if (ty0 + ty >= H || p >= W) continue;
        float o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = transpose_at(&s_mid[c][ty][0], 1, tx0 - r, p, W, t);
        ob[(ty0 + ty) * W + p] = make_float4(o[0], o[1], o[2], 0.f);
    }
}

// grid (tiles, J, B) of the image kernels
bool tile_grid(int B, int J, int H, int W, dim3& grid, int& tiles_x) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30) return false;
    tiles_x = (W + TW - 1) / TW;
    grid = dim3((unsigned)(tiles_x * ((H + TH - 1) / TH)), (unsigned)J, (unsigned)B);
    return true;
}

}  // namespace

extern "C" {

int spaa_blur_rows(const float* sigma, float* row, int n, spaa_stream_t stream) {
    if (!sigma || !row || n < 1 || n > (1 << 24)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blur_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sigma, row, n);
    return (int)hipGetLastError();
}

int spaa_blur_draw(uint32_t seed, int32_t* counter, float lo, float hi, int clean0, float* row, int B, int J, spaa_stream_t stream) {
    if (!counter || !row || B < 1 || B > (1 << 24) || J < 2 || J > SPAA_JITTER_MAX) return hipErrorInvalidValue;
    if (!(lo >= 0.f) || !(lo <= hi) || !(hi <= 2.5f)) return hipErrorInvalidValue;   // (a NaN fails every comparison)
    hipLaunchKernelGGL(blur_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, seed, counter, lo, hi, clean0, row, B * J, J);
    return (int)hipGetLastError();
}

int spaa_blur_fwd(const float* const* y, const float* row, int J, float* const* out, int B, int H, int W, spaa_stream_t stream) {
    Draws<const float> in;
    Draws<float> o;
    dim3 grid;
    int tiles_x;
    if (!gather(in, y, J) || !gather(o, out, J) || !row || !tile_grid(B, J, H, W, grid, tiles_x)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blur_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, row, o, H, W, tiles_x);
    return (int)hipGetLastError();
}

int spaa_blur_bwd(const float* const* g_out, const float* row, int J, float* const* g_y, int B, int H, int W, spaa_stream_t stream) {
    Draws<const float> g;
    Draws<float> o;
    dim3 grid;
    int tiles_x;
    if (!gather(g, g_out, J) || !gather(o, g_y, J) || !row || !tile_grid(B, J, H, W, grid, tiles_x)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blur_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, g, row, o, H, W, tiles_x);
    return (int)hipGetLastError();
}

}  // extern "C"
