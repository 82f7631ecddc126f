// transfer_ops.hip — the transferable adversarial step: the projector-side gradient image of a sample on the adversarial
// step is smoothed by a separable Gaussian (TI-FGSM) and accumulated, L1-normalised, into a momentum image (MI-FGSM).  Per sample b with
// state[b][1] == 0:
//   t   = K (*) g_b         taps w[-r..r] along both axes, zero beyond the image border, each colour channel on its own, pad channel 0
//   n1  = sum over pixels and the three colour channels of |t|
//   m_b = mu m_b + t / n1   (n1 == 0: m_b = mu m_b)
//   g_b = m_b,  partial_ss[b][:] = partial sums of ||m_b||^2: the unchanged spaa_step_and_track_n then steps by adv_lr m_b / ||m_b||_2
// A sample on the colour step (state[b][1] != 0) is not touched: its workgroups return at once.
// Two launches: spaa_transfer_blur (both passes of the filter through LDS, one trip through HBM) and spaa_transfer_momentum.  No atomics
// anywhere and every sum in a fixed order: a run is bitwise repeatable.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "device_util.hpp"

namespace {

constexpr int RMAX = SPAA_TRANSFER_RMAX;
// The output tile of one workgroup: 16 rows of 32 pixels, two pixels per thread.  LDS holds float4 pixels: the tile with its halo
// (at r = 7: 30 x 46 pixels, 22080 bytes) and the row pass's result for the tile's columns (30 x 32 pixels, 15360 bytes): 37.4 KB, four
// workgroups per CU.  Every LDS read is a ds_read_b128 whose 32-lane half-wave reads 32 neighbouring pixels of ONE row: the four 16-lane
// groups of that instruction then each cover the sixteen 16-byte slots of the 256-byte bank row exactly once, whatever the row pitch and
// the tap's offset -- no padding or swizzle is needed (a 16-wide tile would put two rows into one group and conflict for pitches that
// are no multiple of 16 pixels).
constexpr int TW = 32, TH = 16;
constexpr int IW = TW + 2 * RMAX, IH = TH + 2 * RMAX;

struct Taps {
    float w[2 * RMAX + 1];
};

// grid (tiles, B), tile index = row of tiles * tiles per row + column of tiles
__global__ __launch_bounds__(256) void transfer_blur_kernel(const float4* __restrict__ g, const int32_t* __restrict__ state, const Taps taps,
                                                            const int r, float4* __restrict__ t, float* __restrict__ partial_l1, const int Hp,
                                                            const int Wp, const int tiles_x) {
    __shared__ float4 in[IH * IW];
    __shared__ float4 mid[IH * TW];
    __shared__ float w[2 * RMAX + 1];
    __shared__ float red[4];
    const int b = blockIdx.y;
    if (state[4 * b + 1] != 0) return;   // (the whole workgroup: the colour step keeps its gradient image)
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const int n = 2 * r + 1, iw = TW + 2 * r, ih = TH + 2 * r;
    const float4* gb = g + (size_t)b * Hp * Wp;
#pragma unroll
    for (int k = 0; k < 2 * RMAX + 1; ++k)   // (constant indices: the taps stay in the kernel's argument registers)
        if (tid == k) w[k] = taps.w[k];
    // the tile and its halo; zeros beyond the image; the pad channel is dropped here
    for (int i = tid; i < ih * iw; i += 256) {
        const int ly = i / iw, lx = i - ly * iw;
        const int gy = y0 - r + ly, gx = x0 - r + lx;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)gy < (unsigned)Hp && (unsigned)gx < (unsigned)Wp) {
            v = gb[(size_t)gy * Wp + gx];
            v.w = 0.f;
        }
        in[ly * IW + lx] = v;
    }
    __syncthreads();
    // rows: mid[ly][lx] = sum_k w[k] in[ly][lx + k], for the tile's columns and every row of the halo
    for (int i = tid; i < ih * TW; i += 256) {
        const int ly = i / TW, lx = i - ly * TW;
        const float4* row = in + ly * IW + lx;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < n; ++k) {
            const float4 v = row[k];
            const float wk = w[k];
            a.x = fmaf(wk, v.x, a.x);
            a.y = fmaf(wk, v.y, a.y);
            a.z = fmaf(wk, v.z, a.z);
        }
        mid[i] = a;
    }
    __syncthreads();
    // columns: t[y][x] = sum_k w[k] mid[y + k][x]; thread -> column tid % 32, rows tid / 32 and tid / 32 + 8
    const int lx = tid & (TW - 1), x = x0 + lx;
    float l1 = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ly = (tid >> 5) + 8 * h, y = y0 + ly;
        if (y < Hp && x < Wp) {
            const float4* col = mid + ly * TW + lx;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < n; ++k) {
                const float4 v = col[k * TW];
                const float wk = w[k];
                a.x = fmaf(wk, v.x, a.x);
                a.y = fmaf(wk, v.y, a.y);
                a.z = fmaf(wk, v.z, a.z);
            }
            t[(size_t)b * Hp * Wp + (size_t)y * Wp + x] = a;
            l1 += fabsf(a.x) + fabsf(a.y) + fabsf(a.z);
        }
    }
    l1 = block_sum(l1, red);
    if (tid == 0) partial_l1[(size_t)b * gridDim.x + blockIdx.x] = l1;
}

// grid (npartial, B): block j of a sample handles the 256-pixel chunks j, j + npartial, ... and writes partial_ss[b][j]
__global__ __launch_bounds__(256) void transfer_momentum_kernel(const float4* __restrict__ t, const float* __restrict__ partial_l1,
                                                                const int tiles, const float mu, const int32_t* __restrict__ state,
                                                                float4* __restrict__ m, float4* __restrict__ g, float* __restrict__ partial_ss,
                                                                const int HW) {
    __shared__ float red[4];
    const int b = blockIdx.y, j = blockIdx.x, npartial = gridDim.x;
    if (state[4 * b + 1] != 0) return;
    const int nchunks = (HW + 255) / 256;
    if (j >= nchunks) {   // (more partial sums than chunks: the row is still written in full)
        if (threadIdx.x == 0) partial_ss[(size_t)b * npartial + j] = 0.f;
        return;
    }
    // n1: the tiles' sums in index order, the same in every thread of every block.  The running sum is a double: its one rounding to
    // fp32 keeps n1 within half an ulp of the sum of the partials, however many tiles the image has.
    double s = 0.0;
    for (int i = 0; i < tiles; ++i) s += (double)partial_l1[(size_t)b * tiles + i];
    const float n1 = (float)s;
    float ss = 0.f;
    for (int c = j; c < nchunks; c += npartial) {
        const int pix = c * 256 + threadIdx.x;
        if (pix < HW) {
            const size_t idx = (size_t)b * HW + pix;
            const float4 tv = t[idx];
            float4 mv = m[idx];
            if (n1 != 0.f) {
                mv.x = fmaf(mu, mv.x, tv.x / n1);
                mv.y = fmaf(mu, mv.y, tv.y / n1);
                mv.z = fmaf(mu, mv.z, tv.z / n1);
            } else {
                mv.x *= mu;
                mv.y *= mu;
                mv.z *= mu;
            }
            mv.w = 0.f;
            m[idx] = mv;
            g[idx] = mv;
            ss += mv.x * mv.x + mv.y * mv.y + mv.z * mv.z;
        }
    }
    ss = block_sum(ss, red);
    if (threadIdx.x == 0) partial_ss[(size_t)b * npartial + j] = ss;
}

}  // namespace

extern "C" {

int spaa_transfer_tiles(int Hp, int Wp) {
    if (Hp < 1 || Wp < 1 || (int64_t)Hp * Wp > (1 << 30)) return 0;
    return ((Hp + TH - 1) / TH) * ((Wp + TW - 1) / TW);
}

int spaa_transfer_blur(const float* g, const int32_t* state, const float* taps, int r, float* t, float* partial_l1, int B, int Hp, int Wp,
                       spaa_stream_t stream) {
    if (!g || !state || !taps || !t || !partial_l1 || r < 0 || r > RMAX || B < 1 || B > 65535 || Hp < 1 || Wp < 1 ||
        (int64_t)Hp * Wp > (1 << 30))
        return hipErrorInvalidValue;
    Taps tp = {};
    for (int k = 0; k < 2 * r + 1; ++k) tp.w[k] = taps[k];
    const int tiles_x = (Wp + TW - 1) / TW;
    hipLaunchKernelGGL(transfer_blur_kernel, dim3(spaa_transfer_tiles(Hp, Wp), B), dim3(256), 0, (hipStream_t)stream, (const float4*)g, state,
                       tp, r, (float4*)t, partial_l1, Hp, Wp, tiles_x);
    return (int)hipGetLastError();
}

int spaa_transfer_momentum(const float* t, const float* partial_l1, int tiles, float mu, const int32_t* state, float* m, float* g,
                           float* partial_ss, int npartial, int B, int HW, spaa_stream_t stream) {
    if (!t || !partial_l1 || !state || !m || !g || !partial_ss || tiles < 1 || npartial < 1 || B < 1 || B > 65535 || HW < 1 ||
        HW > (1 << 30) || !(mu >= 0.f && mu <= 1.f))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(transfer_momentum_kernel, dim3(npartial, B), dim3(256), 0, (hipStream_t)stream, (const float4*)t, partial_l1, tiles,
                       mu, state, (float4*)m, (float4*)g, partial_ss, HW);
    return (int)hipGetLastError();
}

}  // extern "C"
