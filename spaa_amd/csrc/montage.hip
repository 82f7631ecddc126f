// montage.hip — the result montages of the summary step (attack_results of the reference's projector_based_attack.py:362-414 with
// resize of its img_proc.py:174-197, torchvision's make_grid and cv.applyColorMap), every montage of a setup as final 8-bit pixels:
//   spaa_montage_diff_range   per item, min and max of |rz(real_n) - rz(scene)| over the 3 Hp Wp values of the difference tile
//   spaa_montage_compose      background, the five tiles (scene, projection, inference, capture, colour-mapped difference), text
// rz = centre crop, then F.interpolate(mode='area').  Every value is a fixed sequence of correctly rounded fp32 operations that ends in
// an integer, and min / max do not depend on the order, so a torch / numpy restatement on the host (tests/montage_oracle.py)
// reproduces the bytes exactly.  A byte-bound gather / stream: one thread per output pixel, x fastest (the byte stores of a wave
// are 64 consecutive addresses of one plane), no LDS beyond the block's min / max.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"

// No contraction into FMAs and no reassociation in this file (also -ffp-contract=off from the Makefile).  `/` is IEEE division
// in HIP device code.
#pragma clang fp contract(off)

namespace {

constexpr int BAND = 26, PAD = 5;      // text band above the grid; make_grid's padding
constexpr int NGLYPH = 95;             // printable ASCII 32..126

// One image source: planes [3][H][W] per item, cropped at (y0, x0) to the common ch x cw window.
struct Src {
    const float* p;
    int H, W, y0, x0;
};

struct Geo {
    int ch, cw, Hp, Wp;
};

// adaptive_avg_pool2d's window of output index o: [floor(o n / N), ceil((o + 1) n / N))
__device__ __forceinline__ void window(int o, int n, int N, int& a, int& b) {
    a = (o * n) / N;
    b = ((o + 1) * n + N - 1) / N;
}

// F.interpolate(mode='area') of one crop pixel: the sum over the window in row-major order from 0, then / kh, then / kw
// (ATen's adaptive average pooling divides twice; one division by kh kw rounds differently, e.g. for 3 x 3 windows).
__device__ __forceinline__ float area_px(const float* __restrict__ plane, int W, int ya, int yb, int xa, int xb) {
    float s = 0.f;
    for (int y = ya; y < yb; ++y) {
        const float* r = plane + (size_t)y * W;
        for (int x = xa; x < xb; ++x) s = s + r[x];
    }
    return (s / (float)(yb - ya)) / (float)(xb - xa);
}

// rz(src item n) at tile pixel (ty, tx), the three channels
__device__ __forceinline__ void rz3(const Src& s, size_t n, const Geo& g, int ty, int tx, float v[3]) {
    int ya, yb, xa, xb;
    window(ty, g.ch, g.Hp, ya, yb);
    window(tx, g.cw, g.Wp, xa, xb);
    const float* base = s.p + n * 3 * (size_t)s.H * s.W;
    for (int c = 0; c < 3; ++c)
        v[c] = area_px(base + (size_t)c * s.H * s.W, s.W, s.y0 + ya, s.y0 + yb, s.x0 + xa, s.x0 + xb);
}

__device__ __forceinline__ uint8_t to_byte(float v) {          // ToPILImage / np.uint8(v * 255): truncation, v in [0, 1]
    const int q = (int)(v * 255.f);
    return (uint8_t)(q < 0 ? 0 : (q > 255 ? 255 : q));
}

__global__ void range_init_kernel(uint32_t* __restrict__ minmax, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) {
        minmax[2 * n] = 0x7f800000u;       // +inf
        minmax[2 * n + 1] = 0u;            // +0
    }
}

// Non-negative floats order as their bit patterns: integer atomics, exact in any order.
__global__ __launch_bounds__(256) void diff_range_kernel(Src scene, Src real, Geo g, uint32_t* __restrict__ minmax) {
    __shared__ float smn[4], smx[4];
    const int n = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float mn = __uint_as_float(0x7f800000u), mx = 0.f;
    if (i < g.Hp * g.Wp) {
        const int ty = i / g.Wp, tx = i - ty * g.Wp;
        float a[3], b[3];
        rz3(real, (size_t)n, g, ty, tx, a);
        rz3(scene, 0, g, ty, tx, b);
        for (int c = 0; c < 3; ++c) {
            const float d = fabsf(a[c] - b[c]);
            mn = fminf(mn, d);
            mx = fmaxf(mx, d);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        smn[wave] = mn;
        smx[wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            mn = fminf(mn, smn[w]);
            mx = fmaxf(mx, smx[w]);
        }
        if (mx >= mn) {                    // (a block with at least one pixel; NaN never enters through fminf / fmaxf)
            atomicMin(&minmax[2 * n], __float_as_uint(mn));
            atomicMax(&minmax[2 * n + 1], __float_as_uint(mx));
        }
    }
}

// out [N][3][Hm][Wm], Hm = BAND + Hp + 2 PAD, Wm = 5 (Wp + PAD) + PAD; block = 64 x 4 pixels of one item
__global__ __launch_bounds__(256) void compose_kernel(Src scene, const float* __restrict__ prj, Src infer, Src real, Geo g,
                                                      const float* __restrict__ minmax, const uint8_t* __restrict__ lut,
                                                      uint8_t* __restrict__ out, int Hm, int Wm) {
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const size_t n = blockIdx.z;
    if (X >= Wm || Y >= Hm) return;
    uint8_t px[3] = {255, 255, 255};
    const int ty = Y - (BAND + PAD), xr = X - PAD;
    if (ty >= 0 && ty < g.Hp && xr >= 0) {
        const int k = xr / (g.Wp + PAD), tx = xr - k * (g.Wp + PAD);
        if (k < 5 && tx < g.Wp) {
            float v[3];
            if (k == 1) {
                const float* p = prj + n * 3 * (size_t)g.Hp * g.Wp + (size_t)ty * g.Wp + tx;
                for (int c = 0; c < 3; ++c) px[c] = to_byte(p[(size_t)c * g.Hp * g.Wp]);
            } else if (k < 4) {
                if (k == 0) rz3(scene, 0, g, ty, tx, v);
                else if (k == 2) rz3(infer, n, g, ty, tx, v);
                else rz3(real, n, g, ty, tx, v);
                for (int c = 0; c < 3; ++c) px[c] = to_byte(v[c]);
            } else {
                float b[3];
                rz3(real, n, g, ty, tx, v);
                rz3(scene, 0, g, ty, tx, b);
                const float mn = minmax[2 * n], mx = minmax[2 * n + 1];
                int idx = 0;
                if (mx > mn) {             // mx == mn: a constant difference, index 0 (the reference divides by zero there)
                    const float den = mx - mn;
                    float q[3];
                    for (int c = 0; c < 3; ++c) q[c] = (fabsf(v[c] - b[c]) - mn) / den;
                    const float m = ((q[0] + q[1]) + q[2]) / 3.0f;
                    idx = (int)(m * 255.f);
                    idx = idx < 0 ? 0 : (idx > 255 ? 255 : idx);
                }
                for (int c = 0; c < 3; ++c) px[c] = lut[3 * idx + c];
            }
        }
    }
    uint8_t* o = out + n * 3 * (size_t)Hm * Wm + (size_t)Y * Wm + X;
    for (int c = 0; c < 3; ++c) o[(size_t)c * Hm * Wm] = px[c];
}

// recs [nrec][4] = (item, x, y, glyph); font [95][fh] row bytes, bit x = column x.  One thread per glyph cell pixel; a set bit
// inside the montage becomes (0, 0, 0).  Records that name no item or no glyph are skipped.
__global__ __launch_bounds__(256) void stamp_kernel(const int32_t* __restrict__ recs, int nrec, const uint8_t* __restrict__ font, int fw,
                                                    int fh, int N, int Hm, int Wm, uint8_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int cell = fw * fh;
    if (t >= (int64_t)nrec * cell) return;
    const int r = (int)(t / cell), q = (int)(t - (int64_t)r * cell);
    const int gy = q / fw, gx = q - gy * fw;
    const int item = recs[4 * r], x = recs[4 * r + 1], y = recs[4 * r + 2], glyph = recs[4 * r + 3];
    if (item < 0 || item >= N || glyph < 0 || glyph >= NGLYPH) return;
    if (!((font[glyph * fh + gy] >> gx) & 1)) return;
    const int64_t X = (int64_t)x + gx, Y = (int64_t)y + gy;
    if (X < 0 || X >= Wm || Y < 0 || Y >= Hm) return;
    uint8_t* o = out + (size_t)item * 3 * Hm * Wm + (size_t)Y * Wm + (size_t)X;
    for (int c = 0; c < 3; ++c) o[(size_t)c * Hm * Wm] = 0;
}

inline bool bad_src(const float* p, int H, int W, int y0, int x0, int ch, int cw) {
    return !p || H < 1 || W < 1 || H > 32768 || W > 32768 || y0 < 0 || x0 < 0 || y0 + ch > H || x0 + cw > W;
}

inline bool bad_geo(int N, int ch, int cw, int Hp, int Wp) {
    return N < 1 || N > 65535 || ch < 1 || cw < 1 || Hp < 1 || Wp < 1 || Hp > 32768 || Wp > 6000;
}

}  // namespace

extern "C" {

int spaa_montage_diff_range(const float* cam_scene, int Hs, int Ws, int sy0, int sx0, const float* cam_real, int Hr, int Wr, int ry0,
                            int rx0, int N, int ch, int cw, int Hp, int Wp, float* minmax, spaa_stream_t stream) {
    if (bad_geo(N, ch, cw, Hp, Wp) || bad_src(cam_scene, Hs, Ws, sy0, sx0, ch, cw) || bad_src(cam_real, Hr, Wr, ry0, rx0, ch, cw) ||
        !minmax)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(range_init_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, (uint32_t*)minmax, N);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const Src scene{cam_scene, Hs, Ws, sy0, sx0}, real{cam_real, Hr, Wr, ry0, rx0};
    hipLaunchKernelGGL(diff_range_kernel, dim3((Hp * Wp + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, scene, real,
                       Geo{ch, cw, Hp, Wp}, (uint32_t*)minmax);
    return (int)hipGetLastError();
}

int spaa_montage_compose(const float* cam_scene, int Hs, int Ws, int sy0, int sx0, const float* prj_adv, const float* cam_infer, int Hi,
                         int Wi, int iy0, int ix0, const float* cam_real, int Hr, int Wr, int ry0, int rx0, int N, int ch, int cw, int Hp,
                         int Wp, const float* minmax, const uint8_t* lut, const int32_t* glyph_recs, int nrec, const uint8_t* font,
                         int font_w, int font_h, uint8_t* out, spaa_stream_t stream) {
    if (bad_geo(N, ch, cw, Hp, Wp) || bad_src(cam_scene, Hs, Ws, sy0, sx0, ch, cw) || bad_src(cam_infer, Hi, Wi, iy0, ix0, ch, cw) ||
        bad_src(cam_real, Hr, Wr, ry0, rx0, ch, cw) || !prj_adv || !minmax || !lut || !out || nrec < 0 ||
        (nrec > 0 && (!glyph_recs || !font || font_w < 1 || font_w > 8 || font_h < 1 || font_h > 64)))
        return hipErrorInvalidValue;
    const int Hm = BAND + Hp + 2 * PAD, Wm = 5 * (Wp + PAD) + PAD;
    const Src scene{cam_scene, Hs, Ws, sy0, sx0}, infer{cam_infer, Hi, Wi, iy0, ix0}, real{cam_real, Hr, Wr, ry0, rx0};
    hipLaunchKernelGGL(compose_kernel, dim3((Wm + 63) / 64, (Hm + 3) / 4, N), dim3(256), 0, (hipStream_t)stream, scene, prj_adv, infer,
                       real, Geo{ch, cw, Hp, Wp}, minmax, lut, out, Hm, Wm);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || nrec == 0) return (int)e;
    const int64_t nthr = (int64_t)nrec * font_w * font_h;
    if ((nthr + 255) / 256 > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stamp_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, (hipStream_t)stream, glyph_recs, nrec, font,
                       font_w, font_h, N, Hm, Wm, out);
    return (int)hipGetLastError();
}

}  // extern "C"
