// ssim_ops.hip — the SSIM stealth term of the attack loop: per sample b with weight w_ps[b] != 0
//   loss_b += w_b (1 - SSIM_b(y_b, scene_b)),   SSIM_b = mean over the 3 H W values of the map S (pytorch_ssim._ssim, size_average=False)
//   S = A1 A2 / (B1 B2),  A1 = 2 mu1 mu2 + C1, A2 = 2 (e12 - mu1 mu2) + C2, B1 = mu1^2 + mu2^2 + C1, B2 = (e11 - mu1^2) + (e22 - mu2^2) + C2
// with the five window statistics mu1 = F y, e11 = F y^2, e12 = F (y scene), mu2 = F scene, e22 = F scene^2, and F = "replicate-pad by 5,
// then the 11 x 11 Gaussian", each colour channel on its own.  The window is the outer product of the 11 taps, so F runs as a row pass and
// a column pass (11 + 11 taps instead of 121), both through LDS.
//   spaa_ssim_scene_stats   mu2, e22: once per attack
//   spaa_ssim_fwd           mu1, e11, e12 -> S and its partials dS/dmu1, dS/de11, dS/de12 (three maps), tile sums of S
//   spaa_ssim_bwd           g_y[q] += -gscale w_b (F^T m_mu + 2 y[q] F^T m_11 + scene[q] F^T m_12)[q]
// F^T, the adjoint of "replicate-pad, then filter": along one axis of length n, (F^T m)[q] = sum over the padded positions q' that copy
// pixel q (q itself; -5 .. 0 for q = 0; n - 1 .. n + 4 for q = n - 1) of sum_k w[k] m[q' + 5 - k], m = 0 outside [0, n).  The clamp is
// per axis, so the adjoint is separable as the filter is.
// The variance e11 - mu1^2 cancels in fp32: in a flat bright patch both terms are near 1 and their rounding errors of about 1e-7 stand
// against C2 = 9e-4.  The moments are therefore accumulated about a constant c: per tile and channel the scene's value at the tile's first
// pixel.  With y~ = y - c, s~ = scene - c, the shifted statistics m1 = F y~, q11 = F y~^2, q12 = F (y~ s~), m2 = F s~, q22 = F s~^2 and
// Wt = (sum of the taps)^2, the sum of the window's weights (1 to about 1e-7, not exactly):
//   mu1 = m1 + c Wt,  e11 - mu1^2 = (q11 - m1^2) + (1 - Wt) (2 c m1 + c^2 Wt),  e12 - mu1 mu2 = (q12 - m1 m2) + (1 - Wt) (c (m1 + m2) + c^2 Wt)
// which is the same function of y exactly; in a flat patch the shifted moments are near 0 and nothing cancels.  The partials with respect
// to mu1, e11 and e12 keep their form, so the adjoint needs no shift.  spaa_ssim_scene_stats stores m2 and q22, about the same constants.
// LDS holds channel-planar fp32 tiles: a 32-lane half-wave reads 32 neighbouring floats of one row in both passes (ds_read_b32 banks are
// address / 4 mod 32 per half-wave), which is conflict-free whatever the pitch and the tap's offset.  No atomics and fixed summation
// orders: a run is bitwise repeatable.  A sample with weight 0 is skipped by spaa_ssim_fwd and spaa_ssim_bwd: its workgroups return at once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "device_util.hpp"

namespace {

constexpr int R = 5, NT = 2 * R + 1;
// The output tile of one workgroup: 16 rows of 32 pixels, two pixels per thread; with the halo 26 x 42.
constexpr int TW = SPAA_SSIM_TILE_W, TH = SPAA_SSIM_TILE_H;
constexpr int IW = TW + 2 * R, IH = TH + 2 * R;
constexpr int NIN = IH * IW, NMID = IH * TW;

struct Taps {
    float w[NT];
};

__device__ __forceinline__ float comp(const float4 v, const int c) { return c == 0 ? v.x : (c == 1 ? v.y : v.z); }

// (Every loop over the taps is unrolled: with constant indices the taps stay in the kernel's argument registers.)

// the tile of img - c with its halo, replicate-clamped to the image, into three planes p[channel * NIN + ...]
__device__ __forceinline__ void load_replicate(const float4* __restrict__ img, const float4 c, float* p, const int y0, const int x0,
                                               const int H, const int W) {
    for (int i = threadIdx.x; i < NIN; i += 256) {
        const int ly = i / IW, lx = i - ly * IW;
        const int gy = min(max(y0 - R + ly, 0), H - 1), gx = min(max(x0 - R + lx, 0), W - 1);
        const float4 v = img[(size_t)gy * W + gx];
        p[i] = v.x - c.x;
        p[NIN + i] = v.y - c.y;
        p[2 * NIN + i] = v.z - c.z;
    }
}

// grid (tiles, B): mu2 = F s~, e22 = F s~^2
__global__ __launch_bounds__(256) void ssim_scene_stats_kernel(const float4* __restrict__ scene, const Taps taps, float4* __restrict__ mu2,
                                                               float4* __restrict__ e22, const int H, const int W, const int tiles_x) {
    __shared__ float in[3 * NIN];
    __shared__ float mid[2 * 3 * NMID];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const size_t base = (size_t)b * H * W;
    load_replicate(scene + base, scene[base + (size_t)y0 * W + x0], in, y0, x0, H, W);
    __syncthreads();
    for (int i = tid; i < 3 * NMID; i += 256) {
        const int c = i / NMID, j = i - c * NMID;
        const int ly = j / TW, lx = j - ly * TW;
        const float* row = in + c * NIN + ly * IW + lx;
        float a = 0.f, q = 0.f;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const float v = row[k], wk = taps.w[k];
            a = fmaf(wk, v, a);
            q = fmaf(wk, v * v, q);
        }
        mid[i] = a;
        mid[3 * NMID + i] = q;
    }
    __syncthreads();
    const int lx = tid & (TW - 1), x = x0 + lx;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ly = (tid >> 5) + 8 * h, y = y0 + ly;
        if (y < H && x < W) {
            float a[3], q[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* col = mid + c * NMID + ly * TW + lx;
                a[c] = 0.f;
                q[c] = 0.f;
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    const float wk = taps.w[k];
                    a[c] = fmaf(wk, col[k * TW], a[c]);
                    q[c] = fmaf(wk, col[3 * NMID + k * TW], q[c]);
                }
            }
            const size_t o = base + (size_t)y * W + x;
            mu2[o] = make_float4(a[0], a[1], a[2], 0.f);
            e22[o] = make_float4(q[0], q[1], q[2], 0.f);
        }
    }
}

// grid (tiles, B)
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float4* __restrict__ yimg, const float4* __restrict__ scene,
                                                       const float4* __restrict__ mu2, const float4* __restrict__ e22, const Taps taps,
                                                       const float* __restrict__ w_ps, float4* __restrict__ Mmu, float4* __restrict__ M11,
                                                       float4* __restrict__ M12, float* __restrict__ partial, const float Wt,
                                                       const float omw, const int H, const int W, const int tiles_x) {
    __shared__ float in[6 * NIN];    // (y - c).rgb, (scene - c).rgb
    __shared__ float mid[3 * NMID];   // one channel's row-filtered y, y^2, y scene
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (w_ps[b] == 0.f) return;   // (the whole workgroup)
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const size_t base = (size_t)b * H * W;
    const float4 c4 = scene[base + (size_t)y0 * W + x0];
    load_replicate(yimg + base, c4, in, y0, x0, H, W);
    load_replicate(scene + base, c4, in + 3 * NIN, y0, x0, H, W);
    const int lx = tid & (TW - 1), x = x0 + lx;
    bool inside[2];
    float4 m2[2], q2[2];
    float mmu[2][3], m11[2][3], m12[2][3];
    float s_sum = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int y = y0 + (tid >> 5) + 8 * h;
        inside[h] = y < H && x < W;
        m2[h] = q2[h] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (inside[h]) {
            m2[h] = mu2[base + (size_t)y * W + x];
            q2[h] = e22[base + (size_t)y * W + x];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        __syncthreads();   // `in` is loaded (c == 0); the column pass of the channel before has read `mid`
        // rows: for the tile's columns and every row of the halo
        for (int i = tid; i < NMID; i += 256) {
            const int ly = i / TW, cx = i - ly * TW;
            const float* ry = in + c * NIN + ly * IW + cx;
            const float* rs = ry + 3 * NIN;
            float a = 0.f, q = 0.f, p = 0.f;
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const float v = ry[k], s = rs[k], wk = taps.w[k];
                a = fmaf(wk, v, a);
                q = fmaf(wk, v * v, q);
                p = fmaf(wk, v * s, p);
            }
            mid[i] = a;
            mid[NMID + i] = q;
            mid[2 * NMID + i] = p;
        }
        __syncthreads();
        // columns, then S and its partials: the algebra of train_loss_stats_kernel (color.hip)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ly = (tid >> 5) + 8 * h;
            const float* col = mid + ly * TW + lx;
            float m1 = 0.f, q11 = 0.f, q12 = 0.f;
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const float wk = taps.w[k];
                m1 = fmaf(wk, col[k * TW], m1);
                q11 = fmaf(wk, col[NMID + k * TW], q11);
                q12 = fmaf(wk, col[2 * NMID + k * TW], q12);
            }
            const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
            const float cc = comp(c4, c), mt2 = comp(m2[h], c), q22 = comp(q2[h], c);
            const float k0 = cc * cc * Wt;
            const float var1 = (q11 - m1 * m1) + omw * (2.f * cc * m1 + k0);
            const float var2 = (q22 - mt2 * mt2) + omw * (2.f * cc * mt2 + k0);
            const float cov = (q12 - m1 * mt2) + omw * (cc * (m1 + mt2) + k0);
            const float mu1 = m1 + cc * Wt, mu2c = mt2 + cc * Wt;
            const float A1 = 2.f * (mu1 * mu2c) + C1, A2 = 2.f * cov + C2;
            const float B1 = (mu1 * mu1 + mu2c * mu2c) + C1, B2 = (var1 + var2) + C2;
            const float S = (A1 * A2) / (B1 * B2);
            if (inside[h]) s_sum += S;
            mmu[h][c] = (2.f * mu2c * (A2 - A1)) / (B1 * B2) - S * (2.f * mu1 / B1 - 2.f * mu1 / B2);
            m11[h][c] = -S / B2;
            m12[h][c] = 2.f * A1 / (B1 * B2);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (inside[h]) {
            const size_t o = base + (size_t)(y0 + (tid >> 5) + 8 * h) * W + x;
            Mmu[o] = make_float4(mmu[h][0], mmu[h][1], mmu[h][2], 0.f);
            M11[o] = make_float4(m11[h][0], m11[h][1], m11[h][2], 0.f);
            M12[o] = make_float4(m12[h][0], m12[h][1], m12[h][2], 0.f);
        }
    s_sum = block_sum(s_sum, red);
    if (tid == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = s_sum;
}

// One axis of F^T at pixel q of an axis of length n: m points at the LDS value of position q, `stride` floats between neighbours; the
// values within R of q are in LDS, zero where they lie outside the image.  First the position q itself (tap k of output pixel
// q + R - k), then, for an edge pixel, the pad cells that copy it: -R .. -1 for q = 0, n .. n + R - 1 for q = n - 1.
__device__ __forceinline__ float adjoint_axis(const float* m, const int stride, const int q, const int n, const Taps& taps) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < NT; ++k) a = fmaf(taps.w[k], m[(R - k) * stride], a);
    if (q == 0) {
#pragma unroll
        for (int qp = -R; qp < 0; ++qp)
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const int p = qp + R - k;    // the output pixel whose tap k reads the pad cell qp
                if (p >= 0 && p < n) a = fmaf(taps.w[k], m[p * stride], a);
            }
    }
    if (q == n - 1) {
#pragma unroll
        for (int d = 1; d <= R; ++d)         // the pad cell n - 1 + d
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const int o = d + R - k;     // the output pixel q + o
                if (o <= 0 && q + o >= 0) a = fmaf(taps.w[k], m[o * stride], a);
            }
    }
    return a;
}

// grid (tiles, B)
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float4* __restrict__ yimg, const float4* __restrict__ scene,
                                                       const float4* __restrict__ Mmu, const float4* __restrict__ M11,
                                                       const float4* __restrict__ M12, const Taps taps, const float* __restrict__ w_ps,
                                                       const float gscale, float4* __restrict__ g, const int H, const int W,
                                                       const int tiles_x) {
    __shared__ float in[9 * NIN];     // m_mu.rgb, m_11.rgb, m_12.rgb, zero outside the image
    __shared__ float mid[3 * NMID];   // one channel's row pass of its three maps
    const int b = blockIdx.y, tid = threadIdx.x;
    const float wb = w_ps[b];
    if (wb == 0.f) return;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const size_t base = (size_t)b * H * W;
    for (int i = tid; i < NIN; i += 256) {
        const int ly = i / IW, cx = i - ly * IW;
        const int gy = y0 - R + ly, gx = x0 - R + cx;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a, e = a;
        if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
            const size_t o = base + (size_t)gy * W + gx;
            a = Mmu[o];
            c = M11[o];
            e = M12[o];
        }
        in[i] = a.x;
        in[NIN + i] = a.y;
        in[2 * NIN + i] = a.z;
        in[3 * NIN + i] = c.x;
        in[4 * NIN + i] = c.y;
        in[5 * NIN + i] = c.z;
        in[6 * NIN + i] = e.x;
        in[7 * NIN + i] = e.y;
        in[8 * NIN + i] = e.z;
    }
    const int lx = tid & (TW - 1), x = x0 + lx;
    float t[2][3][3] = {};   // [pixel of the thread][channel][map]
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        __syncthreads();   // `in` is loaded (c == 0); the column pass of the channel before has read `mid`
        // rows (columns of the tile past the image's right edge hold no pixel: zero, never read for a result)
        for (int i = tid; i < 3 * NMID; i += 256) {
            const int mp = i / NMID, j = i - mp * NMID;
            const int ly = j / TW, cx = j - ly * TW;
            const int qx = x0 + cx;
            mid[i] = qx < W ? adjoint_axis(in + (3 * mp + c) * NIN + ly * IW + cx + R, 1, qx, W, taps) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ly = (tid >> 5) + 8 * h, y = y0 + ly;
            if (y < H && x < W) {
#pragma unroll
                for (int mp = 0; mp < 3; ++mp) t[h][c][mp] = adjoint_axis(mid + mp * NMID + (ly + R) * TW + lx, TW, y, H, taps);
            }
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int y = y0 + (tid >> 5) + 8 * h;
        if (y < H && x < W) {
            const size_t o = base + (size_t)y * W + x;
            const float4 yv = yimg[o], sv = scene[o];
            float4 gv = g[o];
            const float s = -gscale * wb;
            gv.x = fmaf(s, t[h][0][0] + 2.f * yv.x * t[h][0][1] + sv.x * t[h][0][2], gv.x);
            gv.y = fmaf(s, t[h][1][0] + 2.f * yv.y * t[h][1][1] + sv.y * t[h][1][2], gv.y);
            gv.z = fmaf(s, t[h][2][0] + 2.f * yv.z * t[h][2][1] + sv.z * t[h][2][2], gv.z);
            g[o] = gv;
        }
    }
}

// one thread per sample: the tile sums in index order (accumulated in double, rounded once)
__global__ void ssim_value_kernel(const float* __restrict__ partial, const float* __restrict__ w_ps, const int tiles, const double inv_n,
                                  float* __restrict__ ssim, const int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || w_ps[b] == 0.f) return;
    double s = 0.0;
    for (int i = 0; i < tiles; ++i) s += (double)partial[(size_t)b * tiles + i];
    ssim[b] = (float)(s * inv_n);
}

bool bad_shape(int B, int H, int W) { return B < 1 || B > 65535 || H < 1 || W < 1 || (int64_t)H * W > (1 << 30); }

// Wt = (sum of the taps)^2 and 1 - Wt, in double, rounded once
void window_sum(const float* taps, float& Wt, float& omw) {
    double sw = 0.0;
    for (int k = 0; k < NT; ++k) sw += (double)taps[k];
    Wt = (float)(sw * sw);
    omw = (float)(1.0 - sw * sw);
}

Taps host_taps(const float* taps) {
    Taps tp;
    for (int k = 0; k < NT; ++k) tp.w[k] = taps[k];
    return tp;
}

}  // namespace

extern "C" {

int spaa_ssim_tiles(int H, int W) {
    if (H < 1 || W < 1 || (int64_t)H * W > (1 << 30)) return 0;
    return ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
}

int spaa_ssim_scene_stats(const float* scene, const float* taps, float* mu2, float* e22, int B, int H, int W, spaa_stream_t stream) {
    if (!scene || !taps || !mu2 || !e22 || bad_shape(B, H, W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ssim_scene_stats_kernel, dim3(spaa_ssim_tiles(H, W), B), dim3(256), 0, (hipStream_t)stream, (const float4*)scene,
                       host_taps(taps), (float4*)mu2, (float4*)e22, H, W, (W + TW - 1) / TW);
    return (int)hipGetLastError();
}

int spaa_ssim_fwd(const float* y, const float* scene, const float* mu2, const float* e22, const float* taps, const float* w_ps, float* m_mu,
                  float* m_11, float* m_12, float* partial, int B, int H, int W, spaa_stream_t stream) {
    if (!y || !scene || !mu2 || !e22 || !taps || !w_ps || !m_mu || !m_11 || !m_12 || !partial || bad_shape(B, H, W))
        return hipErrorInvalidValue;
    float Wt, omw;
    window_sum(taps, Wt, omw);
    hipLaunchKernelGGL(ssim_fwd_kernel, dim3(spaa_ssim_tiles(H, W), B), dim3(256), 0, (hipStream_t)stream, (const float4*)y,
                       (const float4*)scene, (const float4*)mu2, (const float4*)e22, host_taps(taps), w_ps, (float4*)m_mu, (float4*)m_11,
                       (float4*)m_12, partial, Wt, omw, H, W, (W + TW - 1) / TW);
    return (int)hipGetLastError();
}

int spaa_ssim_bwd(const float* y, const float* scene, const float* m_mu, const float* m_11, const float* m_12, const float* taps,
                  const float* w_ps, float gscale, float* g_y, int B, int H, int W, spaa_stream_t stream) {
    if (!y || !scene || !m_mu || !m_11 || !m_12 || !taps || !w_ps || !g_y || bad_shape(B, H, W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3(spaa_ssim_tiles(H, W), B), dim3(256), 0, (hipStream_t)stream, (const float4*)y,
                       (const float4*)scene, (const float4*)m_mu, (const float4*)m_11, (const float4*)m_12, host_taps(taps), w_ps, gscale,
                       (float4*)g_y, H, W, (W + TW - 1) / TW);
    return (int)hipGetLastError();
}

int spaa_ssim_value(const float* partial, const float* w_ps, int tiles, int H, int W, float* ssim, int B, spaa_stream_t stream) {
    if (!partial || !w_ps || !ssim || bad_shape(B, H, W) || tiles != spaa_ssim_tiles(H, W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ssim_value_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, partial, w_ps, tiles,
                       1.0 / (3.0 * (double)H * (double)W), ssim, B);
    return (int)hipGetLastError();
}

}  // extern "C"
