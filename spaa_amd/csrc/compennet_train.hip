// compennet_train.hip — the two non-convolution pieces of the CompenNet++ training step (/root/reference/src/python/
// train_network.py:130-232) that the PCNet step has no use for:
//   spaa_batch_sum_gate   the surface branch runs once, at batch 1 (the scene is one image expanded to the batch, :139): its
//                         gradient is the batch sum of the backbone pre-activation gradients it feeds, gated by its ReLU
//   spaa_warp_bwd_grid2   CompenNet++ warps the camera image AND the scene with the same grid (models.py:204-212): the grid
//                         gradient of both sources in one launch, written once
// Both sum in a fixed order (no atomics): deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"

namespace {

// out[p][c] = (act[p][c] > 0) * sum_b g[b][p][c] for c < C; one thread per 4 channels of one pixel, b in order 0 .. B-1.
// g [B][npix][cstride], act / out [npix][cstride]; channels C .. cstride-1 of out are not written.
__global__ __launch_bounds__(256) void batch_sum_gate_kernel(const float4* __restrict__ g, const float4* __restrict__ act,
                                                             float4* __restrict__ out, int B, int64_t npix, int cq, int cs4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix * cq) return;
    const int64_t pix = i / cq;
    const int64_t o = pix * cs4 + (i - pix * cq);
    const int64_t img = npix * cs4;
    float4 s = g[o];
    for (int b = 1; b < B; ++b) {
        const float4 v = g[(int64_t)b * img + o];
        s.x += v.x;
        s.y += v.y;
        s.z += v.z;
        s.w += v.w;
    }
    if (act != nullptr) {
        const float4 a = act[o];
        s = make_float4(a.x > 0.f ? s.x : 0.f, a.y > 0.f ? s.y : 0.f, a.z > 0.f ? s.z : 0.f, a.w > 0.f ? s.w : 0.f);
    }
    out[o] = s;
}

// grid_sampler_2d_backward w.r.t. the grid (bilinear, zeros padding, align_corners=True) of one source, summed over its
// images in order: adds sum_b sum_c g_c * d v_c / d (x, y) to (gx, gy) (source-pixel units; the caller scales once)
__device__ __forceinline__ void grid_grad_source(const float4* __restrict__ g_w, const float4* __restrict__ x, int B, int Hp,
                                                 int Wp, int HWc, int pix, int x0, int y0, float w, float e, float n, float s,
                                                 float& gx, float& gy) {
    const bool vy0 = (unsigned)y0 < (unsigned)Hp, vy1 = (unsigned)(y0 + 1) < (unsigned)Hp;
    const bool vx0 = (unsigned)x0 < (unsigned)Wp, vx1 = (unsigned)(x0 + 1) < (unsigned)Wp;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = 0; b < B; ++b) {
        const float4* xb = x + (size_t)b * Hp * Wp;
        const float4 nw = (vy0 && vx0) ? xb[y0 * Wp + x0] : z, ne = (vy0 && vx1) ? xb[y0 * Wp + x0 + 1] : z;
        const float4 sw = (vy1 && vx0) ? xb[(y0 + 1) * Wp + x0] : z, se = (vy1 && vx1) ? xb[(y0 + 1) * Wp + x0 + 1] : z;
        const float4 g = g_w[(size_t)b * HWc + pix];
        // v = nw e s + ne w s + sw e n + se w n
        const float dvx0 = (ne.x - nw.x) * s + (se.x - sw.x) * n, dvy0 = (sw.x - nw.x) * e + (se.x - ne.x) * w;
        const float dvx1 = (ne.y - nw.y) * s + (se.y - sw.y) * n, dvy1 = (sw.y - nw.y) * e + (se.y - ne.y) * w;
        const float dvx2 = (ne.z - nw.z) * s + (se.z - sw.z) * n, dvy2 = (sw.z - nw.z) * e + (se.z - ne.z) * w;
        gx += g.x * dvx0 + g.y * dvx1 + g.z * dvx2;
        gy += g.x * dvy0 + g.y * dvy1 + g.z * dvy2;
    }
}

// g_grid[pix] = (d/dgx, d/dgy, 0, 0) of source a (B_a images) plus source b (B_b images), both sampled through `grid`
__global__ __launch_bounds__(256) void warp_bwd_grid2_kernel(const float4* __restrict__ g_a, const float4* __restrict__ x_a, int B_a,
                                                             const float4* __restrict__ g_b, const float4* __restrict__ x_b, int B_b,
                                                             const float4* __restrict__ grid, float4* __restrict__ g_grid, int Hp,
                                                             int Wp, int HWc) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= HWc) return;
    const float4 gr = grid[pix];
    const float xf = (gr.x + 1.f) * (0.5f * (float)(Wp - 1)), yf = (gr.y + 1.f) * (0.5f * (float)(Hp - 1));
    const float xw = floorf(xf), yn = floorf(yf);
    const float w = xf - xw, e = 1.f - w, n = yf - yn, s = 1.f - n;
    const int x0 = (int)xw, y0 = (int)yn;
    float gx = 0.f, gy = 0.f;
    grid_grad_source(g_a, x_a, B_a, Hp, Wp, HWc, pix, x0, y0, w, e, n, s, gx, gy);
    grid_grad_source(g_b, x_b, B_b, Hp, Wp, HWc, pix, x0, y0, w, e, n, s, gx, gy);
    g_grid[pix] = make_float4(gx * (0.5f * (float)(Wp - 1)), gy * (0.5f * (float)(Hp - 1)), 0.f, 0.f);
}

}  // namespace

extern "C" {

int spaa_batch_sum_gate(const float* g, const float* act, float* out, int B, int H, int W, int C, int cstride,
                        spaa_stream_t stream) {
    if (!g || !out || B < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || (cstride & 3) || C > cstride) return hipErrorInvalidValue;
    const int64_t npix = (int64_t)H * W, n = npix * (C / 4);
    hipLaunchKernelGGL(batch_sum_gate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)g,
                       (const float4*)act, (float4*)out, B, npix, C / 4, cstride / 4);
    return (int)hipGetLastError();
}

int spaa_warp_bwd_grid2(const float* g_a, const float* x_a, int B_a, const float* g_b, const float* x_b, int B_b, const float* grid,
                        float* g_grid, int Hp, int Wp, int Hc, int Wc, spaa_stream_t stream) {
    if (!g_a || !x_a || !g_b || !x_b || !grid || !g_grid || B_a < 1 || B_b < 1 || Hp < 1 || Wp < 1 || Hc < 1 || Wc < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(warp_bwd_grid2_kernel, dim3((Hc * Wc + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float4*)g_a,
                       (const float4*)x_a, B_a, (const float4*)g_b, (const float4*)x_b, B_b, (const float4*)grid, (float4*)g_grid, Hp,
                       Wp, Hc * Wc);
    return (int)hipGetLastError();
}

}  // extern "C"
