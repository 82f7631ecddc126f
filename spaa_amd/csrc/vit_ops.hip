// vit_ops.hip — what torchvision's vit_b_16 body (spaa_amd/vit.py) needs beside the 1 x 1 convolution plans: the patch / token
// bookkeeping, LayerNorm, exact (erf) GELU and softmax attention, each forward and adjoint, fp32.
//
// Everything here is exact-fp32 VALU arithmetic with a fixed accumulation order and no atomics: two runs are bitwise equal.  No entry
// point allocates or synchronises (an attack iteration with this body captures into one HIP graph).
//
// LayerNorm: a wave per row.  The row sits in registers (float4 number lane + 64 v of the row in slot v; D = 768 is three slots), the
// mean is a wave sum, the variance the wave sum of the CENTRED squares of those registers (biased, as torch), so a row of large mean and
// tiny variance loses nothing to cancellation.  Rows longer than 64 x 4 x LN_MAXV floats take the same steps with the row re-read from
// memory (L1 / L2: a row is a few KB).  Wave sums are xor butterflies: every lane ends with the same value, in the same order each run.
//
// Attention: one workgroup per (batch, head, block of 64 rows); the two [T, dh] matrices that every row of the block needs (K and V
// forward and in the query-parallel adjoint pass, Q and g_ctx in the key-parallel one) are staged in LDS once, rows padded by 4 floats:
// lane j reads row j as float4s, and with a row stride of dh + 4 floats (4 (mod 8) float4 banks for dh = 64, 16, 8...) the 16 lanes
// that one ds_read_b128 serves together fall on 16 different 16-byte bank groups.  A wave owns a row: its lanes run over the other
// index for the scores (at most ATT_SLOTS = 4 per lane: T <= 256) and over dh for the weighted sums, the weights broadcast from the
// lane that holds them by v_readlane.  The probabilities are never stored: the forward pass keeps lse = max + log(sum), both adjoint
// passes recompute p = exp(s - lse).
//
// Relevance rollout: one layer's step of the class token's row, in the form of the key-parallel adjoint pass without its
// weighted sums (Q and g_ctx staged, a wave owns key j, two dot products per query), then a small pass that adds the heads in index order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"

namespace {

constexpr int64_t MAX_ELEMS = (int64_t)1 << 29;   // every tensor below 2 GiB: element offsets fit an int
inline int nb(const int64_t n) { return (int)((n + 255) / 256); }
inline bool small(const int64_t n) { return n > 0 && n < MAX_ELEMS; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float sum4(const float4 a) { return (a.x + a.y) + (a.z + a.w); }
__device__ __forceinline__ float dot4(const float4 a, const float4 b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}
__device__ __forceinline__ float bcast(const float v, const int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// ---- patch / token bookkeeping ---------------------------------------------------------------------------------------------------
// img [B, h, w, 4] <-> patches [B n, 4 P P], n = (h / P)(w / P) tokens in row-major order, column (ky P + kx) 4 + c: one float4 per
// pixel either way (TO_PATCH: gather into the patch matrix; else the adjoint, which writes every pixel exactly once).
template <bool TO_PATCH>
__global__ __launch_bounds__(256) void patch_kernel(const float4* __restrict__ src, float4* __restrict__ dst, const int h, const int w,
                                                    const int P, const int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // pixel (b, y, x)
    if (idx >= total) return;
    const int x = (int)(idx % w);
    const int64_t r = idx / w;
    const int y = (int)(r % h);
    const int64_t b = r / h;
    const int gw = w / P, gh = h / P;
    const int64_t tok = (b * gh + y / P) * gw + x / P;
    const int64_t pidx = tok * ((int64_t)P * P) + (y % P) * P + (x % P);
    if (TO_PATCH) dst[pidx] = src[idx];
    else dst[idx] = src[pidx];
}

// x[b, 0] = cls + pos[0], x[b, 1 + i] = emb[b, i] + pos[1 + i] (rows of D floats, T = n + 1)
__global__ __launch_bounds__(256) void assemble_kernel(const float4* __restrict__ emb, const float4* __restrict__ cls,
                                                       const float4* __restrict__ pos, float4* __restrict__ x, const int T, const int D4,
                                                       const int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // (b, t, d4)
    if (idx >= total) return;
    const int d = (int)(idx % D4);
    const int64_t r = idx / D4;
    const int t = (int)(r % T);
    const int64_t b = r / T;
    const float4 v = t == 0 ? cls[d] : emb[(b * (T - 1) + (t - 1)) * D4 + d];
    x[idx] = add4(v, pos[(int64_t)t * D4 + d]);
}

__global__ __launch_bounds__(256) void assemble_bwd_kernel(const float4* __restrict__ g_x, float4* __restrict__ g_emb, const int T,
                                                           const int D4, const int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // (b, i, d4) of g_emb
    if (idx >= total) return;
    const int d = (int)(idx % D4);
    const int64_t r = idx / D4;
    const int i = (int)(r % (T - 1));
    const int64_t b = r / (T - 1);
    g_emb[idx] = g_x[(b * T + 1 + i) * D4 + d];
}

// ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
constexpr int LN_MAXV = 4;   // register slots of the in-register form: rows of up to 64 x 4 x 4 = 1024 floats

struct LnArgs {
    const float* x; int64_t x_stride;
    const float* gamma; const float* beta;
    float* y; int64_t y_stride;
    float* mean; float* rstd;
    const float* g; int64_t g_stride;        // backward: gradient of y
    const float* add; int64_t add_stride;    // backward: optional summand of gx
    int rows, D4;
    float eps;
};

// NV > 0: the row in NV register slots; NV == 0: re-read from memory
template <int NV>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const LnArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.rows) return;
    const float4* x = reinterpret_cast<const float4*>(a.x + (int64_t)row * a.x_stride);
    const float4* gm = reinterpret_cast<const float4*>(a.gamma);
    const float4* bt = reinterpret_cast<const float4*>(a.beta);
    float4* y = reinterpret_cast<float4*>(a.y + (int64_t)row * a.y_stride);
    const float invD = 1.f / (float)(a.D4 * 4);
    constexpr int NR = NV > 0 ? NV : 1;
    float4 v[NR];
    float s = 0.f;
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int d = lane + 64 * i;
            v[i] = d < a.D4 ? x[d] : make_float4(0.f, 0.f, 0.f, 0.f);
            s += sum4(v[i]);
        }
    } else {
        for (int d = lane; d < a.D4; d += 64) s += sum4(x[d]);
    }
    const float mu = wave_sum(s) * invD;
    float q = 0.f;
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (lane + 64 * i < a.D4) {
                const float4 c = make_float4(v[i].x - mu, v[i].y - mu, v[i].z - mu, v[i].w - mu);
                q += dot4(c, c, 0.f);
            }
        }
    } else {
        for (int d = lane; d < a.D4; d += 64) {
            const float4 t = x[d];
            const float4 c = make_float4(t.x - mu, t.y - mu, t.z - mu, t.w - mu);
            q += dot4(c, c, 0.f);
        }
    }
    const float rs = 1.f / sqrtf(wave_sum(q) * invD + a.eps);
    if (lane == 0) {
        a.mean[row] = mu;
        a.rstd[row] = rs;
    }
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int d = lane + 64 * i;
            if (d < a.D4) {
                const float4 w = gm[d], b = bt[d];
                y[d] = make_float4(fmaf((v[i].x - mu) * rs, w.x, b.x), fmaf((v[i].y - mu) * rs, w.y, b.y), fmaf((v[i].z - mu) * rs, w.z, b.z),
                                   fmaf((v[i].w - mu) * rs, w.w, b.w));
            }
        }
    } else {
        for (int d = lane; d < a.D4; d += 64) {
            const float4 t = x[d], w = gm[d], b = bt[d];
            y[d] = make_float4(fmaf((t.x - mu) * rs, w.x, b.x), fmaf((t.y - mu) * rs, w.y, b.y), fmaf((t.z - mu) * rs, w.z, b.z),
                               fmaf((t.w - mu) * rs, w.w, b.w));
        }
    }
}

// gx = rstd (gh - mean(gh) - xh mean(gh xh)) [+ add], gh = g gamma, xh = (x - mean) rstd; a.y is gx here
template <int NV>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const LnArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.rows) return;
    const float4* x = reinterpret_cast<const float4*>(a.x + (int64_t)row * a.x_stride);
    const float4* g = reinterpret_cast<const float4*>(a.g + (int64_t)row * a.g_stride);
    const float4* gm = reinterpret_cast<const float4*>(a.gamma);
    const float4* ad = a.add != nullptr ? reinterpret_cast<const float4*>(a.add + (int64_t)row * a.add_stride) : nullptr;
    float4* gx = reinterpret_cast<float4*>(a.y + (int64_t)row * a.y_stride);
    const float invD = 1.f / (float)(a.D4 * 4);
    const float mu = a.mean[row], rs = a.rstd[row];
    constexpr int NR = NV > 0 ? NV : 1;
    float4 gh[NR], xh[NR];
    float s1 = 0.f, s2 = 0.f;
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int d = lane + 64 * i;
            gh[i] = xh[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (d < a.D4) {
                const float4 t = x[d], gg = g[d], w = gm[d];
                gh[i] = make_float4(gg.x * w.x, gg.y * w.y, gg.z * w.z, gg.w * w.w);
                xh[i] = make_float4((t.x - mu) * rs, (t.y - mu) * rs, (t.z - mu) * rs, (t.w - mu) * rs);
            }
            s1 += sum4(gh[i]);
            s2 += dot4(gh[i], xh[i], 0.f);
        }
    } else {
        for (int d = lane; d < a.D4; d += 64) {
            const float4 t = x[d], gg = g[d], w = gm[d];
            const float4 h = make_float4(gg.x * w.x, gg.y * w.y, gg.z * w.z, gg.w * w.w);
            const float4 n = make_float4((t.x - mu) * rs, (t.y - mu) * rs, (t.z - mu) * rs, (t.w - mu) * rs);
            s1 += sum4(h);
            s2 += dot4(h, n, 0.f);
        }
    }
    const float m1 = wave_sum(s1) * invD, m2 = wave_sum(s2) * invD;
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int d = lane + 64 * i;
            if (d < a.D4) {
                float4 o = make_float4(rs * (gh[i].x - m1 - xh[i].x * m2), rs * (gh[i].y - m1 - xh[i].y * m2), rs * (gh[i].z - m1 - xh[i].z * m2),
                                       rs * (gh[i].w - m1 - xh[i].w * m2));
                if (ad != nullptr) o = add4(o, ad[d]);
                gx[d] = o;
            }
        }
    } else {
        for (int d = lane; d < a.D4; d += 64) {
            const float4 t = x[d], gg = g[d], w = gm[d];
            const float4 h = make_float4(gg.x * w.x, gg.y * w.y, gg.z * w.z, gg.w * w.w);
            const float4 n = make_float4((t.x - mu) * rs, (t.y - mu) * rs, (t.z - mu) * rs, (t.w - mu) * rs);
            float4 o = make_float4(rs * (h.x - m1 - n.x * m2), rs * (h.y - m1 - n.y * m2), rs * (h.z - m1 - n.z * m2), rs * (h.w - m1 - n.w * m2));
            if (ad != nullptr) o = add4(o, ad[d]);
            gx[d] = o;
        }
    }
}

inline bool ln_ok(const LnArgs& a, const int D) {
    if (a.rows < 1 || D < 4 || (D & 3)) return false;
    const int64_t strides[4] = {a.x_stride, a.y_stride, a.g_stride, a.add_stride};
    for (const int64_t s : strides)
        if (s < D || (s & 3) || !small((a.rows - 1) * s + D)) return false;
    return true;
}

#define LN_LAUNCH(kernel, a, stream)                                                                                         \
    do {                                                                                                                     \
        const dim3 grid(((a).rows + 3) / 4), block(256);                                                                     \
        const int nv = ((a).D4 + 63) / 64;                                                                                   \
        if (nv <= 1) hipLaunchKernelGGL((kernel<1>), grid, block, 0, (hipStream_t)(stream), a);                              \
        else if (nv == 2) hipLaunchKernelGGL((kernel<2>), grid, block, 0, (hipStream_t)(stream), a);                         \
        else if (nv == 3) hipLaunchKernelGGL((kernel<3>), grid, block, 0, (hipStream_t)(stream), a);                         \
        else if (nv <= LN_MAXV) hipLaunchKernelGGL((kernel<LN_MAXV>), grid, block, 0, (hipStream_t)(stream), a);             \
        else hipLaunchKernelGGL((kernel<0>), grid, block, 0, (hipStream_t)(stream), a);                                      \
    } while (0)

// ---- GELU (exact: x Phi(x)) ------------------------------------------------------------------------------------------------------
// Phi(x) = erfc(-x / sqrt 2) / 2: erfc keeps its relative accuracy in the lower tail, where 1 + erf(x / sqrt 2) cancels.
__device__ __forceinline__ float Phi(const float x) { return 0.5f * erfcf(-x * 0.70710678118654752f); }
__device__ __forceinline__ float phi(const float x) { return 0.39894228040143268f * expf(-0.5f * x * x); }
__device__ __forceinline__ float gelu(const float x) { return x * Phi(x); }
__device__ __forceinline__ float gelu_d(const float x) { return fmaf(x, phi(x), Phi(x)); }

__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float4* __restrict__ pre, float4* __restrict__ act, const int64_t n4) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n4) return;
    const float4 v = pre[idx];
    act[idx] = make_float4(gelu(v.x), gelu(v.y), gelu(v.z), gelu(v.w));
}

__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float4* __restrict__ g, const float4* __restrict__ pre, float4* __restrict__ gx,
                                                       const int64_t n4) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n4) return;
    const float4 v = pre[idx], gg = g[idx];
    gx[idx] = make_float4(gg.x * gelu_d(v.x), gg.y * gelu_d(v.y), gg.z * gelu_d(v.z), gg.w * gelu_d(v.w));
}

// ---- attention ---------------------------------------------------------------------------------------------------------------------
constexpr int ATT_SLOTS = 4;      // rows of the staged matrices per lane: T <= 256
constexpr int ATT_WAVES = 16;     // waves of a workgroup: four per SIMD, the one workgroup that fits a CU at T > 128
constexpr int ATT_ROWS = 64;      // rows of a workgroup's block (4 per wave)
constexpr int ATT_MAXDH = 64;
constexpr int ATT_PAD = 4;        // floats of padding per staged row

struct AttArgs {
    const float* qkv;     // [B, T, 3 D]: q | k | v, head h at columns h dh .. of each
    const float* ctx;     // [B, T, D]      (backward)
    const float* g_ctx;   // [B, T, D]      (backward)
    float* out;           // forward: ctx [B, T, D]; backward: g_qkv [B, T, 3 D]
    float* lse;           // [B, heads, T]: written forward, read backward
    float* delta;         // [B, heads, T]: written by the query-parallel pass, read by the key-parallel one
    int T, heads, dh, D;
    float scale;          // 1 / sqrt(dh)
};

// stage rows [0, T) x dh floats of a [.., T, ld] matrix (row pointer `src`, leading dimension ld) into LDS rows of dh + ATT_PAD floats
__device__ __forceinline__ void stage(float* __restrict__ dst, const float* __restrict__ src, const int64_t ld, const int T, const int dh) {
    const int c4n = dh >> 2, rs = dh + ATT_PAD;
    for (int i = threadIdx.x; i < T * c4n; i += ATT_WAVES * 64) {
        const int r = i / c4n, c = i - r * c4n;
        *reinterpret_cast<float4*>(dst + r * rs + 4 * c) = *reinterpret_cast<const float4*>(src + (int64_t)r * ld + 4 * c);
    }
}

// s[e] = a . A[lane + 64 e] and (TWO) t[e] = b . Bm[lane + 64 e] for the rows below T, zero above; a, b: per-wave LDS vectors
template <bool TWO>
__device__ __forceinline__ void row_dots(const float* __restrict__ A, const float* __restrict__ Bm, const float* __restrict__ a,
                                         const float* __restrict__ b, const int T, const int dh, const int lane, float (&s)[ATT_SLOTS],
                                         float (&t)[ATT_SLOTS]) {
    const int rs = dh + ATT_PAD;
#pragma unroll
    for (int e = 0; e < ATT_SLOTS; ++e) s[e] = t[e] = 0.f;
    // (unrolled so that the LDS reads of several steps are in flight together: a step's FMAs otherwise wait out its own reads' latency)
#pragma unroll(TWO ? 2 : 4)
    for (int c = 0; c < dh; c += 4) {
        const float4 av = *reinterpret_cast<const float4*>(a + c);
        float4 bv = av;
        if (TWO) bv = *reinterpret_cast<const float4*>(b + c);
#pragma unroll
        for (int e = 0; e < ATT_SLOTS; ++e) {
            const int r = lane + 64 * e;
            if (r < T) {
                s[e] = dot4(av, *reinterpret_cast<const float4*>(A + r * rs + c), s[e]);
                if (TWO) t[e] = dot4(bv, *reinterpret_cast<const float4*>(Bm + r * rs + c), t[e]);
            }
        }
    }
}

// sum over rows r < T of w[r] M[r][lane] (lane < dh), w[r] held by lane r % 64 in slot r / 64.  Four partial sums, row r of a slot's
// whole groups of four into sum r % 4 and the slot's last rows into sum 0, added as (0 + 1) + (2 + 3): a fixed order, four independent
// FMA chains, and the four LDS reads of a group (eight with the unrolling) in flight together.
__device__ __forceinline__ float weighted_rows(const float* __restrict__ M, const float (&w)[ATT_SLOTS], const int T, const int dh,
                                               const int lane) {
    const int rs = dh + ATT_PAD, col = lane < dh ? lane : 0;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int e = 0; e < ATT_SLOTS; ++e) {
        const int n = min(64, T - 64 * e);
        const float* __restrict__ base = M + 64 * e * rs + col;
        int l = 0;
#pragma unroll 2
        for (; l + 4 <= n; l += 4) {
            const float* __restrict__ r = base + l * rs;
            const float m0 = r[0], m1 = r[rs], m2 = r[2 * rs], m3 = r[3 * rs];
            a0 = fmaf(bcast(w[e], l), m0, a0);
            a1 = fmaf(bcast(w[e], l + 1), m1, a1);
            a2 = fmaf(bcast(w[e], l + 2), m2, a2);
            a3 = fmaf(bcast(w[e], l + 3), m3, a3);
        }
        for (; l < n; ++l) a0 = fmaf(bcast(w[e], l), base[l * rs], a0);
    }
    return (a0 + a1) + (a2 + a3);
}

template <int TCAP>
__global__ __launch_bounds__(ATT_WAVES * 64) void attn_fwd_kernel(const AttArgs a) {
    __shared__ __attribute__((aligned(16))) float Ks[TCAP * (ATT_MAXDH + ATT_PAD)];
    __shared__ __attribute__((aligned(16))) float Vs[TCAP * (ATT_MAXDH + ATT_PAD)];
    __shared__ __attribute__((aligned(16))) float qs[ATT_WAVES][ATT_MAXDH];
    const int bh = blockIdx.y, b = bh / a.heads, h = bh - b * a.heads;
    const int T = a.T, dh = a.dh, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t ld = 3 * (int64_t)a.D;
    const float* base = a.qkv + (int64_t)b * T * ld + h * dh;
    stage(Ks, base + a.D, ld, T, dh);
    stage(Vs, base + 2 * a.D, ld, T, dh);
    __syncthreads();
    const int i0 = blockIdx.x * ATT_ROWS, i1 = min(T, i0 + ATT_ROWS);
    for (int i = i0 + wave; i < i1; i += ATT_WAVES) {   // (wave-uniform: no workgroup barrier below)
        if (lane < dh) qs[wave][lane] = base[(int64_t)i * ld + lane];
        __builtin_amdgcn_wave_barrier();
        float s[ATT_SLOTS], unused[ATT_SLOTS];
        row_dots<false>(Ks, Ks, qs[wave], qs[wave], T, dh, lane, s, unused);
        float m = -INFINITY;
#pragma unroll
        for (int e = 0; e < ATT_SLOTS; ++e) {
            s[e] *= a.scale;
            if (lane + 64 * e < T) m = fmaxf(m, s[e]);
        }
        m = wave_max(m);
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < ATT_SLOTS; ++e) {
            s[e] = lane + 64 * e < T ? expf(s[e] - m) : 0.f;
            sum += s[e];
        }
        sum = wave_sum(sum);
        const float o = weighted_rows(Vs, s, T, dh, lane) / sum;
        if (lane < dh) a.out[((int64_t)b * T + i) * a.D + h * dh + lane] = o;
        if (lane == 0) a.lse[(int64_t)bh * T + i] = m + logf(sum);
        __builtin_amdgcn_wave_barrier();
    }
}

// KEYPAR == false: the wave's row is a query i; staged A = K, Bm = V; a = q_i, b = g_ctx_i.  Writes delta_i and g_q_i.
// KEYPAR == true:  the wave's row is a key j;   staged A = Q, Bm = g_ctx; a = k_j, b = v_j.  Writes g_k_j and g_v_j.
// Either way lane slot (r) holds p = exp(scale a . A[r] - lse[query]) and ds = p (b . Bm[r] - delta[query]).
template <int TCAP, bool KEYPAR>
__global__ __launch_bounds__(ATT_WAVES * 64) void attn_bwd_kernel(const AttArgs a) {
    __shared__ __attribute__((aligned(16))) float As[TCAP * (ATT_MAXDH + ATT_PAD)];
    __shared__ __attribute__((aligned(16))) float Bs[TCAP * (ATT_MAXDH + ATT_PAD)];
    __shared__ __attribute__((aligned(16))) float av[ATT_WAVES][ATT_MAXDH];
    __shared__ __attribute__((aligned(16))) float bv[ATT_WAVES][ATT_MAXDH];
    const int bh = blockIdx.y, b = bh / a.heads, h = bh - b * a.heads;
    const int T = a.T, dh = a.dh, D = a.D, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t ld = 3 * (int64_t)D;
    const float* base = a.qkv + (int64_t)b * T * ld + h * dh;
    const float* gc = a.g_ctx + (int64_t)b * T * D + h * dh;
    const float* cx = a.ctx + (int64_t)b * T * D + h * dh;
    float* go = a.out + (int64_t)b * T * ld + h * dh;
    const float* lse = a.lse + (int64_t)bh * T;
    float* delta = a.delta + (int64_t)bh * T;
    if (KEYPAR) {
        stage(As, base, ld, T, dh);
        stage(Bs, gc, D, T, dh);
    } else {
        stage(As, base + D, ld, T, dh);
        stage(Bs, base + 2 * D, ld, T, dh);
    }
    __syncthreads();
    const int i0 = blockIdx.x * ATT_ROWS, i1 = min(T, i0 + ATT_ROWS);
    for (int i = i0 + wave; i < i1; i += ATT_WAVES) {
        float l_row = 0.f, d_row = 0.f;
        if (KEYPAR) {
            if (lane < dh) {
                av[wave][lane] = base[(int64_t)i * ld + D + lane];
                bv[wave][lane] = base[(int64_t)i * ld + 2 * D + lane];
            }
        } else {
            float g = 0.f, c = 0.f;
            if (lane < dh) {
                av[wave][lane] = base[(int64_t)i * ld + lane];
                g = gc[(int64_t)i * D + lane];
                c = cx[(int64_t)i * D + lane];
                bv[wave][lane] = g;
            }
            d_row = wave_sum(g * c);
            l_row = lse[i];
            if (lane == 0) delta[i] = d_row;
        }
        __builtin_amdgcn_wave_barrier();
        float s[ATT_SLOTS], t[ATT_SLOTS];
        row_dots<true>(As, Bs, av[wave], bv[wave], T, dh, lane, s, t);
#pragma unroll
        for (int e = 0; e < ATT_SLOTS; ++e) {
            const int r = lane + 64 * e;
            float p = 0.f, ds = 0.f;
            if (r < T) {
                const float l = KEYPAR ? lse[r] : l_row, dl = KEYPAR ? delta[r] : d_row;
                p = expf(s[e] * a.scale - l);
                ds = p * (t[e] - dl);
            }
            s[e] = ds;
            t[e] = p;
        }
        const float g1 = weighted_rows(As, s, T, dh, lane) * a.scale;   // g_q (query-parallel) / g_k (key-parallel)
        if (KEYPAR) {
            const float g2 = weighted_rows(Bs, t, T, dh, lane);         // g_v
            if (lane < dh) {
                go[(int64_t)i * ld + D + lane] = g1;
                go[(int64_t)i * ld + 2 * D + lane] = g2;
            }
        } else if (lane < dh) {
            go[(int64_t)i * ld + lane] = g1;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

inline bool att_ok(int B, int T, int heads, int dh) {
    return B > 0 && T > 0 && T <= 64 * ATT_SLOTS && heads > 0 && dh >= 4 && !(dh & 3) && dh <= ATT_MAXDH &&
           small((int64_t)B * T * 3 * heads * dh) && (int64_t)B * heads < 65536;
}

// ---- relevance rollout ----------------------------------------------------------------------------------------------
// One layer's step of the class token's row of the gradient-weighted attention rollout, pushed down through the layer:
//   rho_out[j] = rho_in[j] + (1 / heads) sum_h sum_i rho_in[i] max(0, P_h[i][j] dP_h[i][j] / seed)
// with P_h[i][j] = exp(scale q_i . k_j - lse[h][i]) and dP_h[i][j] = g_ctx_i . v_j recomputed as in the key-parallel adjoint pass (Q
// and g_ctx staged, a wave owns key j), and seed = g_logits[b][target[b]] the cotangent the backward pass was seeded with.  Two
// launches: relevance_kernel writes the per-head sums w [B, heads, T], relevance_sum_kernel adds the heads in index order.
struct RelArgs {
    const float* qkv;       // [B, T, 3 D]
    const float* lse;       // [B, heads, T]
    const float* g_ctx;     // [B, T, D]
    const float* rho_in;    // [B, T], or NULL: e_cls (only query row 0 is staged and read)
    const float* g_logits;  // [B, ncls]
    const int32_t* target;  // [B]
    float* w;               // [B, heads, T]
    int T, heads, dh, D, ncls;
    float scale;
};

// the seed of sample b: 0 where the target is no class
__device__ __forceinline__ float seed_of(const float* __restrict__ g_logits, const int32_t* __restrict__ target, const int ncls, const int b) {
    const int t = target[b];
    return (unsigned)t < (unsigned)ncls ? g_logits[(int64_t)b * ncls + t] : 0.f;
}

// TCAP bounds the QUERY rows staged: T, or 1 where rho_in == NULL
template <int TCAP>
__global__ __launch_bounds__(ATT_WAVES * 64) void relevance_kernel(const RelArgs a) {
    __shared__ __attribute__((aligned(16))) float As[TCAP * (ATT_MAXDH + ATT_PAD)];
    __shared__ __attribute__((aligned(16))) float Bs[TCAP * (ATT_MAXDH + ATT_PAD)];
    __shared__ __attribute__((aligned(16))) float av[ATT_WAVES][ATT_MAXDH];
    __shared__ __attribute__((aligned(16))) float bv[ATT_WAVES][ATT_MAXDH];
    const int bh = blockIdx.y, b = bh / a.heads, h = bh - b * a.heads;
    const int T = a.T, dh = a.dh, D = a.D, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int Tq = a.rho_in != nullptr ? T : 1;
    const int64_t ld = 3 * (int64_t)D;
    const float* base = a.qkv + (int64_t)b * T * ld + h * dh;
    const float* gc = a.g_ctx + (int64_t)b * T * D + h * dh;
    const float* lse = a.lse + (int64_t)bh * T;
    float* w = a.w + (int64_t)bh * T;
    const int i0 = blockIdx.x * ATT_ROWS, i1 = min(T, i0 + ATT_ROWS);
    const float seed = seed_of(a.g_logits, a.target, a.ncls, b);
    if (seed == 0.f) {   // (workgroup-uniform) no class to explain: the step is the identity
        for (int i = i0 + threadIdx.x; i < i1; i += ATT_WAVES * 64) w[i] = 0.f;
        return;
    }
    const float inv = 1.f / seed;
    stage(As, base, ld, Tq, dh);
    stage(Bs, gc, D, Tq, dh);
    __syncthreads();
    float rho[ATT_SLOTS], l[ATT_SLOTS];
#pragma unroll
    for (int e = 0; e < ATT_SLOTS; ++e) {
        const int r = lane + 64 * e;
        rho[e] = r < Tq ? (a.rho_in != nullptr ? a.rho_in[(int64_t)b * T + r] : 1.f) : 0.f;
        l[e] = r < Tq ? lse[r] : 0.f;
    }
    for (int i = i0 + wave; i < i1; i += ATT_WAVES) {   // (wave-uniform: no workgroup barrier below)
        if (lane < dh) {
            av[wave][lane] = base[(int64_t)i * ld + D + lane];
            bv[wave][lane] = base[(int64_t)i * ld + 2 * D + lane];
        }
        __builtin_amdgcn_wave_barrier();
        float s[ATT_SLOTS], t[ATT_SLOTS];
        row_dots<true>(As, Bs, av[wave], bv[wave], Tq, dh, lane, s, t);
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < ATT_SLOTS; ++e) {
            if (lane + 64 * e < Tq) {
                const float x = expf(s[e] * a.scale - l[e]) * t[e] * inv;
                acc = fmaf(rho[e], x > 0.f ? x : 0.f, acc);
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) w[i] = acc;
        __builtin_amdgcn_wave_barrier();
    }
}

// rho_out[b][j] = rho_in[b][j] (NULL: e_cls) + (sum_h w[b][h][j]) / heads, the heads in index order
__global__ __launch_bounds__(256) void relevance_sum_kernel(const float* __restrict__ w, const float* rho_in, float* rho_out, const int T,
                                                            const int heads, const int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;   // (b, j)
    if (idx >= total) return;
    const int b = idx / T, j = idx - b * T;
    const float* wb = w + (int64_t)b * heads * T + j;
    float acc = 0.f;
    for (int h = 0; h < heads; ++h) acc += wb[(int64_t)h * T];
    const float r = rho_in != nullptr ? rho_in[idx] : (j == 0 ? 1.f : 0.f);
    rho_out[idx] = r + acc / (float)heads;
}

// c[b][i] = max(0, rho[b][1 + i]) and cmax[b] = max_i c[b][i] (both 0 where the seed is 0), as spaa_cam_map leaves them.  One
// workgroup of four waves per sample.
__global__ __launch_bounds__(256) void relevance_map_kernel(const float* __restrict__ rho, const float* __restrict__ g_logits, const int ncls,
                                                            const int32_t* __restrict__ target, float* __restrict__ c,
                                                            float* __restrict__ cmax, const int T) {
    __shared__ float red[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool live = seed_of(g_logits, target, ncls, b) != 0.f;
    float mx = 0.f;
    for (int i = threadIdx.x; i < T - 1; i += 256) {
        const float v = rho[(int64_t)b * T + 1 + i];
        const float cv = live && v > 0.f ? v : 0.f;
        c[(int64_t)b * (T - 1) + i] = cv;
        mx = fmaxf(mx, cv);
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) cmax[b] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

}  // namespace

extern "C" {

int spaa_vit_patchify(const float* img, float* patches, int B, int h, int w, int P, spaa_stream_t stream) {
    if (!img || !patches || B < 1 || h < 1 || w < 1 || P < 1 || h % P || w % P || !small((int64_t)B * h * w * 4)) return hipErrorInvalidValue;
    const int64_t total = (int64_t)B * h * w;
    hipLaunchKernelGGL((patch_kernel<true>), dim3(nb(total)), dim3(256), 0, (hipStream_t)stream, (const float4*)img, (float4*)patches, h, w, P,
                       total);
    return (int)hipGetLastError();
}

int spaa_vit_unpatchify(const float* g_patches, float* g_img, int B, int h, int w, int P, spaa_stream_t stream) {
    if (!g_patches || !g_img || B < 1 || h < 1 || w < 1 || P < 1 || h % P || w % P || !small((int64_t)B * h * w * 4)) return hipErrorInvalidValue;
    const int64_t total = (int64_t)B * h * w;
    hipLaunchKernelGGL((patch_kernel<false>), dim3(nb(total)), dim3(256), 0, (hipStream_t)stream, (const float4*)g_patches, (float4*)g_img, h,
                       w, P, total);
    return (int)hipGetLastError();
}

int spaa_vit_assemble(const float* emb, const float* class_token, const float* pos, float* x, int B, int T, int D, spaa_stream_t stream) {
    if (!emb || !class_token || !pos || !x || B < 1 || T < 2 || D < 4 || (D & 3) || !small((int64_t)B * T * D)) return hipErrorInvalidValue;
    const int64_t total = (int64_t)B * T * (D / 4);
    hipLaunchKernelGGL(assemble_kernel, dim3(nb(total)), dim3(256), 0, (hipStream_t)stream, (const float4*)emb, (const float4*)class_token,
                       (const float4*)pos, (float4*)x, T, D / 4, total);
    return (int)hipGetLastError();
}

int spaa_vit_assemble_bwd(const float* g_x, float* g_emb, int B, int T, int D, spaa_stream_t stream) {
    if (!g_x || !g_emb || B < 1 || T < 2 || D < 4 || (D & 3) || !small((int64_t)B * T * D)) return hipErrorInvalidValue;
    const int64_t total = (int64_t)B * (T - 1) * (D / 4);
    hipLaunchKernelGGL(assemble_bwd_kernel, dim3(nb(total)), dim3(256), 0, (hipStream_t)stream, (const float4*)g_x, (float4*)g_emb, T, D / 4,
                       total);
    return (int)hipGetLastError();
}

int spaa_layernorm_fwd(const float* x, int64_t x_stride, const float* gamma, const float* beta, float* y, int64_t y_stride, float* mean,
                       float* rstd, int rows, int D, float eps, spaa_stream_t stream) {
    if (!x || !gamma || !beta || !y || !mean || !rstd || !(eps >= 0.f)) return hipErrorInvalidValue;
    const LnArgs a{x, x_stride, gamma, beta, y, y_stride, mean, rstd, nullptr, x_stride, nullptr, x_stride, rows, D / 4, eps};
    if (!ln_ok(a, D)) return hipErrorInvalidValue;
    LN_LAUNCH(ln_fwd_kernel, a, stream);
    return (int)hipGetLastError();
}

int spaa_layernorm_bwd(const float* g, int64_t g_stride, const float* x, int64_t x_stride, const float* gamma, const float* mean,
                       const float* rstd, const float* add, int64_t add_stride, float* gx, int64_t gx_stride, int rows, int D,
                       spaa_stream_t stream) {
    if (!g || !x || !gamma || !mean || !rstd || !gx) return hipErrorInvalidValue;
    const LnArgs a{x, x_stride, gamma, nullptr, gx, gx_stride, const_cast<float*>(mean), const_cast<float*>(rstd), g, g_stride, add,
                   add ? add_stride : x_stride, rows, D / 4, 0.f};
    if (!ln_ok(a, D)) return hipErrorInvalidValue;
    LN_LAUNCH(ln_bwd_kernel, a, stream);
    return (int)hipGetLastError();
}

int spaa_gelu_fwd(const float* pre, float* act, int64_t n, spaa_stream_t stream) {
    if (!pre || !act || n < 4 || (n & 3) || n >= MAX_ELEMS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gelu_fwd_kernel, dim3(nb(n / 4)), dim3(256), 0, (hipStream_t)stream, (const float4*)pre, (float4*)act, n / 4);
    return (int)hipGetLastError();
}

int spaa_gelu_bwd(const float* g, const float* pre, float* gx, int64_t n, spaa_stream_t stream) {
    if (!g || !pre || !gx || n < 4 || (n & 3) || n >= MAX_ELEMS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3(nb(n / 4)), dim3(256), 0, (hipStream_t)stream, (const float4*)g, (const float4*)pre, (float4*)gx,
                       n / 4);
    return (int)hipGetLastError();
}

#define ATT_LAUNCH(kernel_of, a, B, stream)                                                                                      \
    do {                                                                                                                         \
        const dim3 grid(((a).T + ATT_ROWS - 1) / ATT_ROWS, (B) * (a).heads), block(ATT_WAVES * 64);                              \
        if ((a).T <= 64) hipLaunchKernelGGL((kernel_of(64)), grid, block, 0, (hipStream_t)(stream), a);                          \
        else if ((a).T <= 128) hipLaunchKernelGGL((kernel_of(128)), grid, block, 0, (hipStream_t)(stream), a);                   \
        else hipLaunchKernelGGL((kernel_of(256)), grid, block, 0, (hipStream_t)(stream), a);                                     \
    } while (0)
#define ATT_FWD(cap) attn_fwd_kernel<cap>
#define ATT_BWD_Q(cap) attn_bwd_kernel<cap, false>
#define ATT_BWD_K(cap) attn_bwd_kernel<cap, true>

int spaa_attn_fwd(const float* qkv, float* ctx, float* lse, int B, int T, int heads, int dh, spaa_stream_t stream) {
    if (!qkv || !ctx || !lse || !att_ok(B, T, heads, dh)) return hipErrorInvalidValue;
    const AttArgs a{qkv, nullptr, nullptr, ctx, lse, nullptr, T, heads, dh, heads * dh, 1.f / sqrtf((float)dh)};
    ATT_LAUNCH(ATT_FWD, a, B, stream);
    return (int)hipGetLastError();
}

int spaa_attn_bwd(const float* qkv, const float* ctx, const float* lse, const float* g_ctx, float* g_qkv, float* delta, int B, int T,
                  int heads, int dh, spaa_stream_t stream) {
    if (!qkv || !ctx || !lse || !g_ctx || !g_qkv || !delta || !att_ok(B, T, heads, dh)) return hipErrorInvalidValue;
    const AttArgs a{qkv, ctx, g_ctx, g_qkv, const_cast<float*>(lse), delta, T, heads, dh, heads * dh, 1.f / sqrtf((float)dh)};
    ATT_LAUNCH(ATT_BWD_Q, a, B, stream);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    ATT_LAUNCH(ATT_BWD_K, a, B, stream);
    return (int)hipGetLastError();
}

int spaa_attn_relevance(const float* qkv, const float* lse, const float* g_ctx, const float* rho_in, const float* g_logits, int ncls,
                        const int32_t* target, float* head_ws, float* rho_out, int B, int T, int heads, int dh, spaa_stream_t stream) {
    if (!qkv || !lse || !g_ctx || !g_logits || !target || !head_ws || !rho_out || ncls < 1 || !att_ok(B, T, heads, dh))
        return hipErrorInvalidValue;
    const RelArgs a{qkv, lse, g_ctx, rho_in, g_logits, target, head_ws, T, heads, dh, heads * dh, ncls, 1.f / sqrtf((float)dh)};
    const dim3 grid((T + ATT_ROWS - 1) / ATT_ROWS, B * heads), block(ATT_WAVES * 64);
    const int tq = rho_in ? T : 1;   // query rows staged
    if (tq <= 64) hipLaunchKernelGGL((relevance_kernel<64>), grid, block, 0, (hipStream_t)stream, a);
    else if (tq <= 128) hipLaunchKernelGGL((relevance_kernel<128>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((relevance_kernel<256>), grid, block, 0, (hipStream_t)stream, a);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(relevance_sum_kernel, dim3(nb((int64_t)B * T)), dim3(256), 0, (hipStream_t)stream, head_ws, rho_in, rho_out, T, heads,
                       B * T);
    return (int)hipGetLastError();
}

int spaa_relevance_map(const float* rho, const float* g_logits, int ncls, const int32_t* target, float* c, float* cmax, int B, int T,
                       spaa_stream_t stream) {
    if (!rho || !g_logits || !target || !c || !cmax || ncls < 1 || B < 1 || T < 2 || !small((int64_t)B * T)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(relevance_map_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, rho, g_logits, ncls, target, c, cmax, T);
    return (int)hipGetLastError();
}

}  // extern "C"
