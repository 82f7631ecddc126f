// dwconv.hip — the depthwise 3 x 3 / ReLU6 layers of torchvision's MobileNetV2 body (spaa_amd/mobilenet.py), forward and
// input-gradient, NHWC fp32.  Both passes are memory-bound (in + out + gate bytes against 9 FMAs per element): a thread owns a float4
// of channels and a short strip of pixels along W, consecutive lanes take consecutive channel quads and then consecutive strips (a
// wave reads whole cache lines), the nine weights and the bias of the quad are loaded once per thread, and the input columns that
// neighbouring pixels of the strip share are loaded once into registers.  Every index into the register arrays is a compile-time
// constant after unrolling: no LDS, no scratch.  The backward pass is a gather (each input pixel sums the outputs it fed), no atomics.
//
// ReLU6 (torch's hardtanh(0, 6)) lives here only: value min(max(v, 0), 6), gradient where 0 < v < 6, strictly on both sides.  Gate
// bytes have the format of spaa_tapconv_t.mask_out (one byte per 4 consecutive channels, bit e = channel 4 q + e passes), so that a
// convolution's input-gradient launch takes them through `gate_bits` unchanged.  As every ReLU epilogue of this library the clamp is
// fmaxf / fminf: a NaN becomes 0 and its gate bit is clear (the library's contract is finite values).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"

namespace {

__device__ __forceinline__ float clamp6(const float v) { return fminf(fmaxf(v, 0.f), 6.f); }
__device__ __forceinline__ float4 clamp6(const float4 v) { return make_float4(clamp6(v.x), clamp6(v.y), clamp6(v.z), clamp6(v.w)); }
__device__ __forceinline__ bool pass6(const float v) { return v > 0.f && v < 6.f; }
__device__ __forceinline__ unsigned bits6(const float4 v) {
    return (pass6(v.x) ? 1u : 0u) | (pass6(v.y) ? 2u : 0u) | (pass6(v.z) ? 4u : 0u) | (pass6(v.w) ? 8u : 0u);
}
__device__ __forceinline__ float4 fma4(const float4 w, const float4 v, const float4 a) {
    return make_float4(fmaf(w.x, v.x, a.x), fmaf(w.y, v.y, a.y), fmaf(w.z, v.z, a.z), fmaf(w.w, v.w, a.w));
}

struct Geo {
    int B, Hin, Win, C4, Hout, Wout, nstrip;
    int64_t total;   // threads: B x (rows) x nstrip x C4
    int pack4;       // gate bytes of four neighbouring lanes as one 32-bit store (C4 % 4 == 0 and a 4-byte aligned mask)
};

// One gate byte per lane is a 1-byte store per lane.  Where C4 % 4 == 0, lanes 4 k .. 4 k + 3 of a wave hold the channel quads
// c .. c + 3 of ONE pixel (c % 4 == lane % 4 == 0: the thread index is a multiple of C4 away from c, and all four are active or none:
// every bound is a multiple of C4), so lane 4 k collects the four bytes and stores them as one word.  Lanes of a group take the same
// branches; what a shuffle reads from lanes outside the group is not used.
__device__ __forceinline__ void store_gate(uint8_t* __restrict__ mask, const size_t o, const unsigned m, const int pack4) {
    if (pack4) {
        const unsigned w = m | ((unsigned)__shfl_down((int)m, 1) << 8) | ((unsigned)__shfl_down((int)m, 2) << 16) |
                           ((unsigned)__shfl_down((int)m, 3) << 24);
        if ((threadIdx.x & 3) == 0) *reinterpret_cast<uint32_t*>(mask + o) = w;
    } else {
        mask[o] = (uint8_t)m;
    }
}

// Forward: a thread writes S output pixels of one row; its NC = (S - 1) STRIDE + 3 input columns x 3 rows sit in registers.
// acc = bias, then fmaf(w, v, acc) over (ky, kx) in row-major order, taps outside the image skipped.
template <int STRIDE, int S>
__global__ __launch_bounds__(256) void dw3_fwd_kernel(const float4* __restrict__ in, const int in_relu6, const float4* __restrict__ w,
                                                      const float4* __restrict__ bias, float4* __restrict__ out,
                                                      uint8_t* __restrict__ mask, const Geo g) {
    constexpr int NC = (S - 1) * STRIDE + 3;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.total) return;
    const int c = (int)(idx % g.C4);
    int64_t r = idx / g.C4;
    const int sx = (int)(r % g.nstrip);
    r /= g.nstrip;
    const int oy = (int)(r % g.Hout);
    const int b = (int)(r / g.Hout);
    float4 wk[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wk[t] = w[(size_t)t * g.C4 + c];
    const float4 bs = bias[c];
    const int ox0 = sx * S, ix0 = ox0 * STRIDE - 1, iy0 = oy * STRIDE - 1;
    bool rowok[3], colok[NC];
    float4 v[3][NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) colok[j] = (unsigned)(ix0 + j) < (unsigned)g.Win;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        rowok[ky] = (unsigned)(iy0 + ky) < (unsigned)g.Hin;
        const float4* row = in + ((size_t)b * g.Hin + (rowok[ky] ? iy0 + ky : 0)) * g.Win * g.C4 + c;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rowok[ky] && colok[j]) {
                t = row[(size_t)(ix0 + j) * g.C4];
                if (in_relu6) t = clamp6(t);
            }
            v[ky][j] = t;
        }
    }
    const size_t orow = ((size_t)b * g.Hout + oy) * g.Wout;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        if (ox0 + i >= g.Wout) break;
        float4 acc = bs;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
                if (rowok[ky] && colok[i * STRIDE + kx]) acc = fma4(wk[ky * 3 + kx], v[ky][i * STRIDE + kx], acc);
        const size_t o = (orow + ox0 + i) * g.C4 + c;
        if (mask != nullptr) store_gate(mask, o, bits6(acc), g.pack4);
        out[o] = clamp6(acc);
    }
}

// Backward: a thread writes S input pixels of one row (S even, the strip starts at an even x).  Input pixel (y, x) was read by the
// output pixel (oy, ox) through tap (ky, kx) where oy STRIDE - 1 + ky = y and ox STRIDE - 1 + kx = x.
//   stride 1: ox = x + 1 - kx: the strip needs the output columns x0 - 1 .. x0 + S (S + 2 of them) and up to three rows;
//   stride 2: x + 1 - kx must be even: an even x takes kx = 1 only, an odd x takes kx = 0 and 2 -- the strip needs the S / 2 + 1
//             columns from x0 / 2 on, and an even row one output row (ky = 1), an odd row two (ky = 0, 2).
// acc = 0, then fmaf(w, g, acc) over the taps (ky, kx) in row-major order that reach an output pixel; then the ReLU6 gate of in_pre.
template <int STRIDE, int S>
__global__ __launch_bounds__(256) void dw3_bwd_kernel(const float4* __restrict__ g_out, const float4* __restrict__ w,
                                                      const float4* __restrict__ in_pre, float4* __restrict__ g_in, const Geo g) {
    static_assert(S % 2 == 0, "the strip starts at an even x");
    constexpr int NC = STRIDE == 1 ? S + 2 : S / 2 + 1;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.total) return;
    const int c = (int)(idx % g.C4);
    int64_t r = idx / g.C4;
    const int sx = (int)(r % g.nstrip);
    r /= g.nstrip;
    const int y = (int)(r % g.Hin);
    const int b = (int)(r / g.Hin);
    float4 wk[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wk[t] = w[(size_t)t * g.C4 + c];
    const int x0 = sx * S;
    const int obase = STRIDE == 1 ? x0 - 1 : x0 / 2;      // output column of register column 0
    bool rowok[3], colok[NC];
    float4 go[3][NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) colok[j] = (unsigned)(obase + j) < (unsigned)g.Wout;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int t = y + 1 - ky;
        const int oy = STRIDE == 1 ? t : t >> 1;
        rowok[ky] = t >= 0 && (STRIDE == 1 || !(t & 1)) && oy < g.Hout;
        const float4* row = g_out + ((size_t)b * g.Hout + (rowok[ky] ? oy : 0)) * g.Wout * g.C4 + c;
#pragma unroll
        for (int j = 0; j < NC; ++j)
            go[ky][j] = (rowok[ky] && colok[j]) ? row[(size_t)(obase + j) * g.C4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const size_t irow = ((size_t)b * g.Hin + y) * g.Win;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        if (x0 + i >= g.Win) break;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                // register column of the output pixel that read input pixel x0 + i through tap kx (x0 is even)
                const int num = i + 1 - kx;                      // x + 1 - kx - x0: -1 .. S, known after unrolling
                if (STRIDE == 2 && (num & 1)) continue;
                const int j = STRIDE == 1 ? num + 1 : num / 2;   // (stride 2: the even values are 0 .. S)
                if (rowok[ky] && colok[j]) acc = fma4(wk[ky * 3 + kx], go[ky][j], acc);
            }
        const size_t o = (irow + x0 + i) * g.C4 + c;
        if (in_pre != nullptr) {
            const float4 p = in_pre[o];
            acc = make_float4(pass6(p.x) ? acc.x : 0.f, pass6(p.y) ? acc.y : 0.f, pass6(p.z) ? acc.z : 0.f, pass6(p.w) ? acc.w : 0.f);
        }
        g_in[o] = acc;
    }
}

// in-place ReLU6 of [M][C] with its gate bytes (mask may be null)
__global__ __launch_bounds__(256) void relu6_gate_kernel(float4* __restrict__ act, uint8_t* __restrict__ mask, const int64_t n,
                                                         const int pack4) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const float4 v = act[idx];
    if (mask != nullptr) store_gate(mask, (size_t)idx, bits6(v), pack4);
    act[idx] = clamp6(v);
}

// g_in[b, p, c] = bit ? g_feat[b, c] / HW : 0
__global__ __launch_bounds__(256) void gap_bwd_bits_kernel(const float4* __restrict__ g_feat, const uint8_t* __restrict__ mask,
                                                           float4* __restrict__ g_in, const int HW, const int C4, const int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % C4);
    const int64_t b = idx / ((int64_t)HW * C4);
    const float4 g = g_feat[b * C4 + c];
    const unsigned m = mask[idx];
    const float d = (float)HW;
    g_in[idx] = make_float4((m & 1u) ? g.x / d : 0.f, (m & 2u) ? g.y / d : 0.f, (m & 4u) ? g.z / d : 0.f, (m & 8u) ? g.w / d : 0.f);
}

inline int nb(const int64_t n) { return (int)((n + 255) / 256); }
inline int pack4_ok(const int C, const uint8_t* mask) { return !(C & 15) && !((uintptr_t)mask & 3); }

// B x Hin x Win x C elements below 2^29 (every tensor below 2 GiB): the thread count and every block count fit an int
inline bool dw_ok(int B, int Hin, int Win, int C, int stride) {
    return B > 0 && Hin > 0 && Win > 0 && C > 0 && !(C & 3) && (stride == 1 || stride == 2) &&
           (int64_t)B * Hin * Win * C < ((int64_t)1 << 29);
}

constexpr int FWD_S1 = 4, FWD_S2 = 2, BWD_S = 4;   // strip lengths: 6 / 5 input columns forward, 6 / 3 output columns backward

}  // namespace

extern "C" {

int spaa_dwconv3_fwd(const float* in, int in_relu6, const float* w, const float* bias, float* out, uint8_t* mask_out, int B, int Hin,
                     int Win, int C, int stride, spaa_stream_t stream) {
    if (!in || !w || !bias || !out || !dw_ok(B, Hin, Win, C, stride)) return hipErrorInvalidValue;
    Geo g{B, Hin, Win, C / 4, (Hin - 1) / stride + 1, (Win - 1) / stride + 1, 0, 0, pack4_ok(C, mask_out)};
    const int S = stride == 1 ? FWD_S1 : FWD_S2;
    g.nstrip = (g.Wout + S - 1) / S;
    g.total = (int64_t)B * g.Hout * g.nstrip * g.C4;
    if (stride == 1)
        hipLaunchKernelGGL((dw3_fwd_kernel<1, FWD_S1>), dim3(nb(g.total)), dim3(256), 0, (hipStream_t)stream, (const float4*)in, in_relu6,
                           (const float4*)w, (const float4*)bias, (float4*)out, mask_out, g);
    else
        hipLaunchKernelGGL((dw3_fwd_kernel<2, FWD_S2>), dim3(nb(g.total)), dim3(256), 0, (hipStream_t)stream, (const float4*)in, in_relu6,
                           (const float4*)w, (const float4*)bias, (float4*)out, mask_out, g);
    return (int)hipGetLastError();
}

int spaa_dwconv3_bwd(const float* g_out, const float* w, const float* in_pre, float* g_in, int B, int Hin, int Win, int C, int stride,
                     spaa_stream_t stream) {
    if (!g_out || !w || !g_in || !dw_ok(B, Hin, Win, C, stride)) return hipErrorInvalidValue;
    Geo g{B, Hin, Win, C / 4, (Hin - 1) / stride + 1, (Win - 1) / stride + 1, 0, 0, 0};
    g.nstrip = (Win + BWD_S - 1) / BWD_S;
    g.total = (int64_t)B * Hin * g.nstrip * g.C4;
    if (stride == 1)
        hipLaunchKernelGGL((dw3_bwd_kernel<1, BWD_S>), dim3(nb(g.total)), dim3(256), 0, (hipStream_t)stream, (const float4*)g_out,
                           (const float4*)w, (const float4*)in_pre, (float4*)g_in, g);
    else
        hipLaunchKernelGGL((dw3_bwd_kernel<2, BWD_S>), dim3(nb(g.total)), dim3(256), 0, (hipStream_t)stream, (const float4*)g_out,
                           (const float4*)w, (const float4*)in_pre, (float4*)g_in, g);
    return (int)hipGetLastError();
}

int spaa_relu6_gate(float* act, uint8_t* mask_out, int64_t M, int C, spaa_stream_t stream) {
    if (!act || M < 1 || C < 4 || (C & 3) || M * (int64_t)C >= ((int64_t)1 << 29)) return hipErrorInvalidValue;
    const int64_t n = M * (C / 4);
    hipLaunchKernelGGL(relu6_gate_kernel, dim3(nb(n)), dim3(256), 0, (hipStream_t)stream, (float4*)act, mask_out, n,
                       pack4_ok(C, mask_out));
    return (int)hipGetLastError();
}

int spaa_global_avgpool_bwd_bits(const float* g_feat, const uint8_t* mask, float* g_in, int B, int HW, int C, spaa_stream_t stream) {
    if (!g_feat || !mask || !g_in || B < 1 || HW < 1 || C < 4 || (C & 3) || (int64_t)B * HW * C >= ((int64_t)1 << 29))
        return hipErrorInvalidValue;
    const int64_t n = (int64_t)B * HW * (C / 4);
    hipLaunchKernelGGL(gap_bwd_bits_kernel, dim3(nb(n)), dim3(256), 0, (hipStream_t)stream, (const float4*)g_feat, mask, (float4*)g_in, HW,
                       C / 4, n);
    return (int)hipGetLastError();
}

}  // extern "C"
