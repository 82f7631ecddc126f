// color.hip — differentiable sRGB -> CIELAB and the per-pixel CIEDE2000 map, plus the fused stealthiness loss.
//
// Replaces (perc_al/differential_color_functions.py): rgb2xyz :12-24, xyz_lab :27-36, rgb2lab_diff :39-64,
// hpf/dhpf/ahpf :73-106, ciede2000_diff :109-180 and their autograd, and the L2 stealth term
// projector_based_attack.py:279.  The reference's constants are reproduced as written (sRGB threshold 0.0405,
// 4-decimal RGB->XYZ matrix, white 95.0489/100/108.8840, f(0)=0, T's `aHP - 39`, the +1e-4 guards), not the
// textbook ones.
//
// One launch computes, per camera pixel, both loss terms and their analytic gradient w.r.t. the inferred camera
// image (hand-written reverse mode of the ~300-op ATen graph), i.e. ~600 elementwise ATen launches become one
// pass: read y, scene, scene_lab (48 B/px), write g_y (16 B/px).  Pixel sums are reduced per block in a fixed
// order (no atomics) so results are run-to-run reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "device_util.hpp"

namespace {

constexpr float kPi = 3.14159265358979323846f;
constexpr float kDeg = (float)(180.0 / 3.14159265358979323846);   // degrees(n) = n * (180/pi)
constexpr float kRad = (float)(3.14159265358979323846 / 180.0);   // radians(n) = n * (pi/180)
constexpr float kXn = 95.0489f, kYn = 100.f, kZn = 108.8840f;
constexpr float k25_7 = 6103515625.f;  // 25^7

// Round 5: the remaining libm sequences of the per-pixel colour map on the hardware transcendentals as well -- t^1.4 = exp2(1.4 log2 t)
// (v_log_f32 + v_exp_f32: 3 instructions for powf's ~60), the cube root likewise, v_sqrt_f32 (1 ulp) for sqrtf's 12-instruction
// correctly-rounded form, divisions by the colour constants as multiplications by their reciprocals: a few ulp on Lab (the fixtures of
// the reference are met at 1e-5 relative, dE at 2e-4 absolute, as before), the SAME functions in spaa_rgb2lab and inside the fused loss
// (identical pixels still give dE == 0 exactly).  SPAA_COLOR_LIBM: the libm forms, for A/B accuracy runs.
#ifdef SPAA_COLOR_LIBM
__device__ __forceinline__ float fpow14(float t) { return powf(t, 1.4f); }
__device__ __forceinline__ float fcbrt(float t) { return cbrtf(t); }
__device__ __forceinline__ float fsqrt(float t) { return sqrtf(t); }
__device__ __forceinline__ float fdivc(float x, float c) { return x / c; }
#else
__device__ __forceinline__ float fpow14(float t) { return __builtin_amdgcn_exp2f(1.4f * __builtin_amdgcn_logf(t)); }
__device__ __forceinline__ float fcbrt(float t) { return __builtin_amdgcn_exp2f((1.f / 3.f) * __builtin_amdgcn_logf(t)); }
__device__ __forceinline__ float fsqrt(float t) { return __builtin_amdgcn_sqrtf(t); }
__device__ __forceinline__ float fdivc(float x, float c) { return x * (1.f / c); }      // (c: a compile-time constant)
#endif

__device__ __forceinline__ float srgb_lin(float v, float& dv) {
    // rgb2xyz :16-20
    if (v > 0.0405f) {
        const float t = fdivc(v + 0.055f, 1.055f);
        const float p14 = fpow14(t);
        dv = 100.f * (2.4f / 1.055f) * p14;
        return 100.f * (p14 * t);  // t^2.4 = t^1.4 * t  (within an ulp of powf(t, 2.4f))
    }
    dv = 100.f / 12.92f;
    return 100.f * fdivc(v, 12.92f);
}

// forward-only variant: the SAME arithmetic as srgb_lin, so that Lab(scene) cached by spaa_rgb2lab and Lab(y)
// recomputed inside the fused loss kernel agree bit-for-bit on identical pixels (dE == 0 exactly, zero gradient).
__device__ __forceinline__ float srgb_lin_fwd(float v) {
    float d;
    return srgb_lin(v, d);
}

__device__ __forceinline__ float lab_f(float t, float& dt) {
    // xyz_lab :27-36 ; exactly-zero input maps to 0 with zero slope (Q3)
    if (t == 0.f) {
        dt = 0.f;
        return 0.f;
    }
    if (t > 0.008856f) {
        const float c = fcbrt(t);
        dt = (1.f / 3.f) / (c * c);
        return c;
    }
    dt = 7.787f;
    return 7.787f * t + (float)(16.0 / 116.0);
}

__device__ __forceinline__ void rgb_to_lab(float r, float g, float b, float& L, float& A, float& Bv) {
    float d;
    const float lr = srgb_lin_fwd(r), lg = srgb_lin_fwd(g), lb = srgb_lin_fwd(b);
    const float X = 0.4124f * lr + 0.3576f * lg + 0.1805f * lb;
    const float Y = 0.2126f * lr + 0.7152f * lg + 0.0722f * lb;
    const float Z = 0.0193f * lr + 0.1192f * lg + 0.9504f * lb;
    const float fx = lab_f(fdivc(X, kXn), d), fy = lab_f(fdivc(Y, kYn), d), fz = lab_f(fdivc(Z, kZn), d);
    L = 116.f * fy - 16.f;
    A = 500.f * (fx - fy);
    Bv = 200.f * (fy - fz);
}

__device__ __forceinline__ float pow7(float x) {
    const float x2 = x * x, x4 = x2 * x2;
    return x4 * x2 * x;
}

// hue angle of hpf_diff :73-81 (x = b, y = a'), in degrees in [0, 360)
__device__ __forceinline__ float hue_deg(float x, float y) {
    if (x == 0.f && y == 0.f) return 0.f;
    const float t = atan2f(x, y) * kDeg;
    return t >= 0.f ? t : 360.f + t;
}

// Trigonometry of the dE2000 weighting terms on the hardware transcendentals (v_sin_f32 / v_cos_f32 / v_exp_f32: one 8-cycle
// instruction each instead of libm's ~40-instruction sequences; 14 of them per pixel and pass).  Arguments are bounded
// (|angle| <= 4 x 360 + 63 degrees), the results enter dE through weights of at most 0.32 (T), 30 (dRO, Gaussian) and the
// half hue difference: absolute errors of ~1e-6 in sin / cos move dE by < 1e-5 of its value (gated by the known-answer and
// gradient tests against the reference's fixtures).  SPAA_COLOR_LIBM: the libm forms, for A/B accuracy runs.
#ifdef SPAA_COLOR_LIBM
__device__ __forceinline__ float fsin(float x) { return sinf(x); }
__device__ __forceinline__ float fcos(float x) { return cosf(x); }
__device__ __forceinline__ float fexp(float x) { return expf(x); }
#else
__device__ __forceinline__ float fsin(float x) { return __sinf(x); }
__device__ __forceinline__ float fcos(float x) { return __cosf(x); }
__device__ __forceinline__ float fexp(float x) { return __expf(x); }
#endif

// x / y through v_rcp_f32 (1 ulp) instead of the IEEE-exact ten-instruction sequence: 64 divisions per pixel in the dE2000 map
// and its reverse mode.  Every divisor is non-zero where it is used (guards below); results move by ~1e-7 relative.
#ifdef SPAA_COLOR_LIBM
__device__ __forceinline__ float fdiv(float x, float y) { return x / y; }
#else
__device__ __forceinline__ float fdiv(float x, float y) { return x * __builtin_amdgcn_rcpf(y); }
#endif

struct DE {
    float de;
    float gL, gA, gB;  // d de / d (L1, A1, B1)
};

// CIEDE2000 of (L1,A1,B1) vs (L2,A2,B2) as the reference computes it, with the gradient w.r.t. the first colour.
template <bool GRAD>
__device__ __forceinline__ DE ciede2000(float L1, float A1, float B1, float L2, float A2, float B2) {
    DE out;
    const bool m01 = (A1 == 0.f) && (B1 == 0.f);
    const bool m02 = (A2 == 0.f) && (B2 == 0.f);
    if (m01) B1 += 0.0001f;
    if (m02) B2 += 0.0001f;
    const float C1 = fsqrt(A1 * A1 + B1 * B1);
    const float C2 = fsqrt(A2 * A2 + B2 * B2);
    const float aC = ((C1 + C2) * 0.5f);
    const float aC7 = pow7(aC);
    const float fG = fdiv(aC7, (aC7 + k25_7));
    const float sfG = sqrtf(fG);   // (fG = aC^7 / (aC^7 + 25^7) is DENORMAL for near-grey pairs: v_sqrt_f32 would flush it to 0)
    const float G = 0.5f * (1.f - sfG);
    const float a1P = (1.f + G) * A1;
    const float a2P = (1.f + G) * A2;
    const float c1P = fsqrt(a1P * a1P + B1 * B1);
    const float c2P = fsqrt(a2P * a2P + B2 * B2);
    const float h1P = m01 ? 0.f : hue_deg(B1, a1P);
    const float h2P = m02 ? 0.f : hue_deg(B2, a2P);
    const float dLP = L2 - L1;
    const float dCP = c2P - c1P;
    const bool mc0 = (C1 * C2) == 0.f;
    const float dh = h2P - h1P;
    float dhP = 0.f;
    if (!mc0) dhP = (fabsf(dh) <= 180.f) ? dh : (dh > 180.f ? dh - 360.f : dh + 360.f);
    const float sq = fsqrt(c1P * c2P);
    const float half = ((dhP * kRad) * 0.5f);
    const float sn = fsin(half), cs = fcos(half);
    const float m_no = (m01 || m02) ? 0.f : 1.f;
    const float dHP = 2.f * sq * sn * m_no;
    const float aL = ((L1 + L2) * 0.5f);
    const float aCP = ((c1P + c2P) * 0.5f);
    const float hs = h1P + h2P;
    float aHP = 0.f;
    if (!mc0) {
        const float r = (fabsf(dh) <= 180.f) ? hs : ((fabsf(hs) < 360.f) ? hs + 360.f : hs - 360.f);
        aHP = r * 0.5f;
    }
    const float t1 = (aHP - 39.f) * kRad, t2 = (2.f * aHP) * kRad, t3 = (3.f * aHP + 6.f) * kRad,
                t4 = (4.f * aHP - 63.f) * kRad;
    const float T = 1.f - 0.17f * fcos(t1) + 0.24f * fcos(t2) + 0.32f * fcos(t3) - 0.2f * fcos(t4);
    const float e = ((aHP - 275.f) * (1.f / 25.f));
    const float dRO = 30.f * fexp(-1.f * (e * e));
    const float aCP7 = pow7(aCP);
    const float fR = fdiv(aCP7, (aCP7 + k25_7));
    const float rC = sqrtf(fR);    // (likewise)
    const float q = (aL - 50.f) * (aL - 50.f);
    const float sq20 = fsqrt(20.f + q);
    const float sL = 1.f + fdiv((0.015f * q), sq20);
    const float sC = 1.f + 0.045f * aCP;
    const float sH = 1.f + 0.015f * aCP * T;
    const float ang = (2.f * dRO) * kRad;
    const float sa = fsin(ang);
    const float rT = -2.f * rC * sa;
    const float u = fdiv(dLP, sL), v = fdiv(dCP, sC), w = fdiv(dHP, sH);
    const float rs = u * u + (v * v) * m_no + (w * w) * m_no + rT * v * w * m_no;
    const bool m0 = rs <= 0.f;
    out.de = m0 ? 0.f : fsqrt(rs);
    out.gL = out.gA = out.gB = 0.f;
    if (!GRAD || m0) return out;

    // ---- reverse mode -----------------------------------------------------------------------------------
    const float rs_b = fdiv(0.5f, out.de);
    const float u_b = rs_b * 2.f * u;
    const float v_b = rs_b * m_no * (2.f * v + rT * w);
    const float w_b = rs_b * m_no * (2.f * w + rT * v);
    const float rT_b = rs_b * m_no * v * w;
    const float dLP_b = fdiv(u_b, sL);
    const float sL_b = -u_b * fdiv(dLP, (sL * sL));
    const float dCP_b = fdiv(v_b, sC);
    const float sC_b = -v_b * fdiv(dCP, (sC * sC));
    const float dHP_b = fdiv(w_b, sH);
    const float sH_b = -w_b * fdiv(dHP, (sH * sH));
    const float rC_b = rT_b * (-2.f * sa);
    const float dRO_b = rT_b * (-2.f * rC * fcos(ang)) * (2.f * kRad);
    float aCP_b = sH_b * 0.015f * T + sC_b * 0.045f;
    const float T_b = sH_b * 0.015f * aCP;
    const float q_b = sL_b * 0.015f * (fdiv(1.f, sq20) - 0.5f * fdiv(q, (sq20 * sq20 * sq20)));
    const float aL_b = q_b * 2.f * (aL - 50.f);
    {
        const float den = aCP7 + k25_7;
        const float aCP6 = fdiv(aCP7, aCP);
        // d sqrt(f) / d f = 0.5 / sqrt(f) with f = aCP^7 / (aCP^7 + 25^7) underflowed to 0 (aCP below ~1e-5): 0.5 / 0 would
        // give inf (or NaN against aCP6 == 0); the true derivative there is ~3.5 aCP^2.5 / 25^3.5 < 1e-16, taken as 0
        const float r_rC = rC > 0.f ? fdiv(0.5f, rC) : 0.f;
        aCP_b += rC_b * r_rC * (fdiv(k25_7, (den * den))) * 7.f * aCP6;
    }
    float aHP_b = dRO_b * dRO * (-2.f * (e * (1.f / 25.f)));
    aHP_b += T_b * kRad * (0.17f * fsin(t1) - 0.48f * fsin(t2) - 0.96f * fsin(t3) + 0.8f * fsin(t4));
    const float dHPm_b = dHP_b * m_no;
    const float sq_b = dHPm_b * 2.f * sn;
    const float dhP_b = dHPm_b * 2.f * sq * cs * (kRad * 0.5f);
    float c1P_b = 0.f, c2P_b = 0.f;
    if (sq_b != 0.f) {
        c1P_b = sq_b * (fdiv(0.5f, sq)) * c2P;
        c2P_b = sq_b * (fdiv(0.5f, sq)) * c1P;
    }
    c1P_b += aCP_b * 0.5f - dCP_b;
    c2P_b += aCP_b * 0.5f + dCP_b;
    float L1_b = aL_b * 0.5f - dLP_b;
    float h1P_b = 0.f, h2P_b = 0.f;
    if (!mc0) {
        h1P_b = aHP_b * 0.5f - dhP_b;
        h2P_b = aHP_b * 0.5f + dhP_b;
    }
    float a1P_b = 0.f, a2P_b = 0.f, B1_b = 0.f;
    if (!m01 && !(B1 == 0.f && a1P == 0.f)) {
        const float den = B1 * B1 + a1P * a1P;
        B1_b += h1P_b * kDeg * (fdiv(a1P, den));
        a1P_b += h1P_b * kDeg * (-fdiv(B1, den));
    }
    if (!m02 && !(B2 == 0.f && a2P == 0.f)) {
        const float den = B2 * B2 + a2P * a2P;
        a2P_b += h2P_b * kDeg * (-fdiv(B2, den));
    }
    a1P_b += c1P_b * (fdiv(a1P, c1P));
    B1_b += c1P_b * (fdiv(B1, c1P));
    a2P_b += c2P_b * (fdiv(a2P, c2P));
    float A1_b = a1P_b * (1.f + G);
    const float G_b = a1P_b * A1 + a2P_b * A2;
    float aC_b = 0.f;
    if (G_b != 0.f) {
        const float den = aC7 + k25_7;
        const float aC6 = fdiv(aC7, aC);
        const float r_sfG = sfG > 0.f ? -fdiv(0.25f, sfG) : 0.f;   // (likewise: fG underflowed for aC below ~1e-5)
        aC_b = G_b * r_sfG * (fdiv(k25_7, (den * den))) * 7.f * aC6;
    }
    const float C1_b = aC_b * 0.5f;
    A1_b += C1_b * (fdiv(A1, C1));
    B1_b += C1_b * (fdiv(B1, C1));
    out.gL = L1_b;
    out.gA = A1_b;
    out.gB = B1_b;
    return out;
}

__global__ void rgb2lab_kernel(const float4* __restrict__ rgb, float4* __restrict__ lab, int npix) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix) return;
    const float4 v = rgb[idx];
    float L, A, B;
    rgb_to_lab(v.x, v.y, v.z, L, A, B);
    lab[idx] = make_float4(L, A, B, 0.f);
}

__global__ void ciede2000_kernel(const float4* __restrict__ lab1, const float4* __restrict__ lab2,
                                 float* __restrict__ de, int npix) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix) return;
    const float4 a = lab1[idx], b = lab2[idx];
    // identical colours: the reference's res_square is exactly 0 -> dE = 0 (:174-178); do not leave it to how the compiler
    // contracts the two (textually different) chroma expressions
    de[idx] = (a.x == b.x && a.y == b.y && a.z == b.z) ? 0.f : ciede2000<false>(a.x, a.y, a.z, b.x, b.y, b.z).de;
}

// autograd of rgb2lab_diff (:39-64): g_rgb = J^T g_lab, per pixel
__global__ void rgb2lab_bwd_kernel(const float4* __restrict__ rgb, const float4* __restrict__ g_lab,
                                   float4* __restrict__ g_rgb, int npix) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix) return;
    const float4 v = rgb[idx], gl = g_lab[idx];
    float dr, dg, db;
    const float lr = srgb_lin(v.x, dr), lg = srgb_lin(v.y, dg), lb = srgb_lin(v.z, db);
    const float X = 0.4124f * lr + 0.3576f * lg + 0.1805f * lb;
    const float Y = 0.2126f * lr + 0.7152f * lg + 0.0722f * lb;
    const float Z = 0.0193f * lr + 0.1192f * lg + 0.9504f * lb;
    float dfx, dfy, dfz;
    lab_f(fdivc(X, kXn), dfx);
    lab_f(fdivc(Y, kYn), dfy);
    lab_f(fdivc(Z, kZn), dfz);
    const float fy_b = 116.f * gl.x - 500.f * gl.y + 200.f * gl.z;
    const float fx_b = 500.f * gl.y;
    const float fz_b = -200.f * gl.z;
    const float X_b = fdivc(fx_b * dfx, kXn), Y_b = fdivc(fy_b * dfy, kYn), Z_b = fdivc(fz_b * dfz, kZn);
    g_rgb[idx] = make_float4((0.4124f * X_b + 0.2126f * Y_b + 0.0193f * Z_b) * dr,
                             (0.3576f * X_b + 0.7152f * Y_b + 0.1192f * Z_b) * dg,
                             (0.1805f * X_b + 0.0722f * Y_b + 0.9504f * Z_b) * db, 0.f);
}

// autograd of ciede2000_diff (:109-180): g_lab1 = g_de * d dE/d lab1 and (optionally) g_lab2 = g_de * d dE/d lab2.
// The map is symmetric in its two colours (dLP, dCP, dHP change sign together; aL, aCP, aHP, T, rT do not change), so
// the second gradient is the first-colour adjoint of the swapped pair.
__global__ void ciede2000_bwd_kernel(const float4* __restrict__ lab1, const float4* __restrict__ lab2,
                                     const float* __restrict__ g_de, float4* __restrict__ g_lab1,
                                     float4* __restrict__ g_lab2, int npix) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix) return;
    const float4 a = lab1[idx], b = lab2[idx];
    float g = g_de[idx];
    // identical colours: dE = 0 through the reference's `res_square <= 0` mask, whose gradient is exactly zero (the map is
    // |x|-like there: any rounding asymmetry between the two chroma expressions would otherwise give an O(1) gradient)
    if (a.x == b.x && a.y == b.y && a.z == b.z) g = 0.f;
    if (g_lab1 != nullptr) {
        const DE d = ciede2000<true>(a.x, a.y, a.z, b.x, b.y, b.z);
        g_lab1[idx] = make_float4(g * d.gL, g * d.gA, g * d.gB, 0.f);
    }
    if (g_lab2 != nullptr) {
        const DE d = ciede2000<true>(b.x, b.y, b.z, a.x, a.y, a.z);
        g_lab2[idx] = make_float4(g * d.gL, g * d.gA, g * d.gB, 0.f);
    }
}

// d dE(lab(rgb), lab2) / d rgb, and dE
__device__ __forceinline__ float de_rgb_grad(float r, float g, float b, float L2, float A2, float B2, float& gr,
                                             float& gg, float& gb) {
    float dr, dg, db;
    const float lr = srgb_lin(r, dr), lg = srgb_lin(g, dg), lb = srgb_lin(b, db);
    const float X = 0.4124f * lr + 0.3576f * lg + 0.1805f * lb;
    const float Y = 0.2126f * lr + 0.7152f * lg + 0.0722f * lb;
    const float Z = 0.0193f * lr + 0.1192f * lg + 0.9504f * lb;
    float dfx, dfy, dfz;
    const float fx = lab_f(fdivc(X, kXn), dfx), fy = lab_f(fdivc(Y, kYn), dfy), fz = lab_f(fdivc(Z, kZn), dfz);
    const float L = 116.f * fy - 16.f, A = 500.f * (fx - fy), Bv = 200.f * (fy - fz);
    const DE d = ciede2000<true>(L, A, Bv, L2, A2, B2);
    const float fy_b = 116.f * d.gL - 500.f * d.gA + 200.f * d.gB;
    const float fx_b = 500.f * d.gA;
    const float fz_b = -200.f * d.gB;
    const float X_b = fdivc(fx_b * dfx, kXn), Y_b = fdivc(fy_b * dfy, kYn), Z_b = fdivc(fz_b * dfz, kZn);
    gr = (0.4124f * X_b + 0.2126f * Y_b + 0.0193f * Z_b) * dr;
    gg = (0.3576f * X_b + 0.7152f * Y_b + 0.1192f * Z_b) * dg;
    gb = (0.1805f * X_b + 0.0722f * Y_b + 0.9504f * Z_b) * db;
    return d.de;
}

// grid: (nblk, B); block 256 px
__global__ __launch_bounds__(256) void stealth_loss_kernel(const float4* __restrict__ y,
                                                           const float4* __restrict__ scene,
                                                           const float4* __restrict__ scene_lab, float caml2_w,
                                                           float camdE_w, float gscale, float4* __restrict__ g_y,
                                                           float* __restrict__ de_map, float* __restrict__ partial,
                                                           int HW, const float* __restrict__ params) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    if (params != nullptr) {   // spaa_stealth_loss_fwd_bwd_ps: this sample's weights (params[b] = prjl2_w, caml2_w, camdE_w, d_thr)
        caml2_w = params[4 * b + 1];
        camdE_w = params[4 * b + 2];
    }
    const int pix = blockIdx.x * 256 + threadIdx.x;
    float l2 = 0.f, de = 0.f;
    if (pix < HW) {
        const size_t idx = (size_t)b * HW + pix;
        const float4 yv = y[idx];
        const float4 sv = scene[idx];
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
        // caml2 = || scene - y ||_2 over channels (projector_based_attack.py:279); norm backward is 0 at 0
        const float d0 = sv.x - yv.x, d1 = sv.y - yv.y, d2 = sv.z - yv.z;
        l2 = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
        if (caml2_w != 0.f && l2 != 0.f) {
            const float k = -caml2_w / l2;
            g0 = k * d0;
            g1 = k * d1;
            g2 = k * d2;
        }
        if (l2 == 0.f) {
            // identical pixels: the reference's two Lab values are bitwise equal, so res_square == 0 -> dE = 0 with
            // zero gradient (differential_color_functions.py:174-178); do not depend on Lab(scene) having been
            // rounded identically by another kernel.
            de = 0.f;
        } else if (camdE_w != 0.f) {
            const float4 lv = scene_lab[idx];
            float r0, r1, r2;
            de = de_rgb_grad(yv.x, yv.y, yv.z, lv.x, lv.y, lv.z, r0, r1, r2);
            g0 += camdE_w * r0;
            g1 += camdE_w * r1;
            g2 += camdE_w * r2;
        } else {
            const float4 lv = scene_lab[idx];
            float L, A, Bv;
            rgb_to_lab(yv.x, yv.y, yv.z, L, A, Bv);
            de = ciede2000<false>(L, A, Bv, lv.x, lv.y, lv.z).de;
        }
        g_y[idx] = make_float4(g0 * gscale, g1 * gscale, g2 * gscale, 0.f);
        if (de_map != nullptr) de_map[idx] = de;
    }
    const float s_l2 = block_sum(l2, red);
    const float s_de = block_sum(de, red);
    const float s_de2 = block_sum(de * de, red);
    if (threadIdx.x == 0) {
        float* p = partial + 3 * ((size_t)b * gridDim.x + blockIdx.x);
        p[0] = s_l2;
        p[1] = s_de;
        p[2] = s_de2;
    }
}

// gradient of  sum_px w_px * dE(lab1, lab(rgb2))  w.r.t. rgb2 is not needed by SPAA; PerC-AL uses
// dE(inputs_LAB, lab(x)) with the *second* argument variable (perc_al/__init__.py:197): provided by the
// symmetric kernel below (argument order swapped inside ciede2000 is NOT equivalent, so it has its own adjoint).

// ---------------------------------------------------------------------------------------------------------------
// calc_img_dists (utils.py:420-491) of a table of image pairs, one block per 16x16 tile of a pair's crop rectangle (the tile list of
// all pairs is flattened: tile_pair[tile] -> pair).  x and y are NCHW fp32 planes read in place (no crop copy, no NHWC4 conversion);
// the y side may be a constant colour.  Per tile, in the same pass over the halo: the SSIM map (pytorch_ssim/__init__.py:26-58:
// the 11x11 Gaussian window passed in as the reference builds it, replicate padding CLAMPED TO THE CROP, the reference's
// cc(...) then _ssim) and the per-pixel terms of MSE / mean-L2 / mean-L_inf / mean dE2000.
// partial[tile][5] = (sum d^2 over 3 channels, sum SSIM over 3 channels, sum ||d||_2, sum max|d|, sum dE): fixed slots, no
// atomics; the host adds a pair's tiles in order.
constexpr int SS_T = 16, SS_R = 5, SS_P = SS_T + 2 * SS_R;
static_assert(sizeof(spaa_img_pair_t) == 80, "spaa_img_pair_t: the layout _lib.ImgPair restates");
__global__ __launch_bounds__(256) void img_stats_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        const spaa_img_pair_t* __restrict__ pairs,
                                                        const int32_t* __restrict__ tile_pair,
                                                        const float* __restrict__ window, float* __restrict__ partial) {
    __shared__ float4 sx[SS_P * SS_P], sy[SS_P * SS_P];
    __shared__ float sw[121];
    __shared__ float red[4];
    const int tile = blockIdx.x;
    const spaa_img_pair_t P = pairs[tile_pair[tile]];
    const int ntx = (P.w + SS_T - 1) / SS_T, lt = tile - P.tile0;
    const int ty = lt / ntx, y0 = ty * SS_T, x0 = (lt - ty * ntx) * SS_T;
    const float* xb = x + P.x_off;
    const int xplane = P.xH * P.xW;
    for (int i = threadIdx.x; i < SS_P * SS_P; i += 256) {
        const int py = i / SS_P, px = i - py * SS_P;
        const int cy = min(max(y0 + py - SS_R, 0), P.h - 1), cx = min(max(x0 + px - SS_R, 0), P.w - 1);  // replicate, inside the crop
        const int xi = (P.xy0 + cy) * P.xW + P.xx0 + cx;
        sx[i] = make_float4(xb[xi], xb[xi + xplane], xb[xi + 2 * xplane], 0.f);
        if (P.y_const) {
            sy[i] = make_float4(P.y_rgb[0], P.y_rgb[1], P.y_rgb[2], 0.f);
        } else {
            const float* yb = y + P.y_off;
            const int yplane = P.yH * P.yW, yi = (P.yy0 + cy) * P.yW + P.yx0 + cx;
            sy[i] = make_float4(yb[yi], yb[yi + yplane], yb[yi + 2 * yplane], 0.f);
        }
    }
    if (threadIdx.x < 121) sw[threadIdx.x] = window[threadIdx.x];
    __syncthreads();
    const int ly = threadIdx.x / SS_T, lx = threadIdx.x - ly * SS_T;
    float mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0}, s11[3] = {0, 0, 0}, s22[3] = {0, 0, 0}, s12[3] = {0, 0, 0};
    for (int ky = 0; ky < 11; ++ky)
        for (int kx = 0; kx < 11; ++kx) {
            const float w = sw[ky * 11 + kx];
            const float4 a = sx[(ly + ky) * SS_P + lx + kx], c = sy[(ly + ky) * SS_P + lx + kx];
            const float av[3] = {a.x, a.y, a.z}, cv[3] = {c.x, c.y, c.z};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                mu1[ch] = fmaf(w, av[ch], mu1[ch]);
                mu2[ch] = fmaf(w, cv[ch], mu2[ch]);
                s11[ch] = fmaf(w, av[ch] * av[ch], s11[ch]);
                s22[ch] = fmaf(w, cv[ch] * cv[ch], s22[ch]);
                s12[ch] = fmaf(w, av[ch] * cv[ch], s12[ch]);
            }
        }
    float v = 0.f, sq = 0.f, l2 = 0.f, li = 0.f, de = 0.f;
    if (y0 + ly < P.h && x0 + lx < P.w) {
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float m11 = mu1[ch] * mu1[ch], m22 = mu2[ch] * mu2[ch], m12 = mu1[ch] * mu2[ch];
            v += ((2.f * m12 + C1) * (2.f * (s12[ch] - m12) + C2)) /
                 ((m11 + m22 + C1) * ((s11[ch] - m11) + (s22[ch] - m22) + C2));
        }
        const float4 a = sx[(ly + SS_R) * SS_P + lx + SS_R], b = sy[(ly + SS_R) * SS_P + lx + SS_R];
        const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
        sq = dx * dx + dy * dy + dz * dz;
        l2 = sqrtf(sq);
        li = fmaxf(fabsf(dx), fmaxf(fabsf(dy), fabsf(dz)));
        float L1, A1, B1, L2, A2, B2;
        rgb_to_lab(a.x, a.y, a.z, L1, A1, B1);
        rgb_to_lab(b.x, b.y, b.z, L2, A2, B2);
        de = ciede2000<false>(L1, A1, B1, L2, A2, B2).de;
    }
    const float s0 = block_sum(sq, red), s1 = block_sum(v, red), s2 = block_sum(l2, red), s3 = block_sum(li, red),
                s4 = block_sum(de, red);
    if (threadIdx.x == 0) {
        float* o = partial + (size_t)tile * 5;
        o[0] = s0;
        o[1] = s1;
        o[2] = s2;
        o[3] = s3;
        o[4] = s4;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Training loss of PCNet (train_network.py:367-392 compute_loss): l1 [+ (1 - SSIM)], with its gradient w.r.t. the inferred
// image, and the MSE the reference logs.  SSIM as pytorch_ssim/__init__.py:26-58 (11x11 Gaussian, replicate padding).
//   S = A1 A2 / (B1 B2),  A1 = 2 mu1 mu2 + C1, A2 = 2 (e12 - mu1 mu2) + C2, B1 = mu1^2 + mu2^2 + C1, B2 = e11 - mu1^2 + e22 - mu2^2 + C2
// pass 1 (per output pixel p): S and its partials w.r.t. the three window statistics that depend on y:
//   Mmu = dS/dmu1, M11 = dS/de11, M12 = dS/de12        (mu1 = sum w y, e11 = sum w y^2, e12 = sum w y t)
// pass 2 (per image pixel q): g[q] = sign(y-t)/N - (1/N) sum_{q' -> q} sum_p w(p - q') [Mmu(p) + 2 y[q] M11(p) + t[q] M12(p)]
//   where q' runs over the replicate-padded positions that read pixel q (q itself, plus the pad cells beside an edge pixel).
__global__ __launch_bounds__(256) void train_loss_stats_kernel(const float4* __restrict__ x, const float4* __restrict__ y,
                                                               const float* __restrict__ window, float4* __restrict__ Mmu,
                                                               float4* __restrict__ M11, float4* __restrict__ M12,
                                                               float* __restrict__ partial, int H, int W, int use_ssim) {
    __shared__ float4 sx[SS_P * SS_P], sy[SS_P * SS_P];
    __shared__ float sw[121];
    __shared__ float red[4];
    const int b = blockIdx.z, y0 = blockIdx.y * SS_T, x0 = blockIdx.x * SS_T;
    const size_t base = (size_t)b * H * W;
    for (int i = threadIdx.x; i < SS_P * SS_P; i += 256) {
        const int py = i / SS_P, px = i - py * SS_P;
        const int iy = min(max(y0 + py - SS_R, 0), H - 1), ix = min(max(x0 + px - SS_R, 0), W - 1);  // replicate
        sx[i] = x[base + (size_t)iy * W + ix];
        sy[i] = y[base + (size_t)iy * W + ix];
    }
    if (threadIdx.x < 121) sw[threadIdx.x] = window[threadIdx.x];
    __syncthreads();
    const int ly = threadIdx.x / SS_T, lx = threadIdx.x - ly * SS_T;
    const bool inside = y0 + ly < H && x0 + lx < W;
    float s_sum = 0.f, l1 = 0.f, l2 = 0.f;
    float mmu[3] = {0, 0, 0}, m11[3] = {0, 0, 0}, m12[3] = {0, 0, 0};
    if (inside) {
        const float4 a0 = sx[(ly + SS_R) * SS_P + lx + SS_R], c0 = sy[(ly + SS_R) * SS_P + lx + SS_R];
        const float d[3] = {a0.x - c0.x, a0.y - c0.y, a0.z - c0.z};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            l1 += fabsf(d[ch]);
            l2 += d[ch] * d[ch];
        }
    }
    if (use_ssim) {
        float mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0}, e11[3] = {0, 0, 0}, e22[3] = {0, 0, 0}, e12[3] = {0, 0, 0};
        for (int ky = 0; ky < 11; ++ky)
            for (int kx = 0; kx < 11; ++kx) {
                const float w = sw[ky * 11 + kx];
                const float4 a = sx[(ly + ky) * SS_P + lx + kx], c = sy[(ly + ky) * SS_P + lx + kx];
                const float av[3] = {a.x, a.y, a.z}, cv[3] = {c.x, c.y, c.z};
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    mu1[ch] = fmaf(w, av[ch], mu1[ch]);
                    mu2[ch] = fmaf(w, cv[ch], mu2[ch]);
                    e11[ch] = fmaf(w, av[ch] * av[ch], e11[ch]);
                    e22[ch] = fmaf(w, cv[ch] * cv[ch], e22[ch]);
                    e12[ch] = fmaf(w, av[ch] * cv[ch], e12[ch]);
                }
            }
        if (inside) {
            const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float m11s = mu1[ch] * mu1[ch], m22s = mu2[ch] * mu2[ch], m12s = mu1[ch] * mu2[ch];
                const float A1 = 2.f * m12s + C1, A2 = 2.f * (e12[ch] - m12s) + C2;
                const float B1 = m11s + m22s + C1, B2 = (e11[ch] - m11s) + (e22[ch] - m22s) + C2;
                const float S = (A1 * A2) / (B1 * B2);
                s_sum += S;
                mmu[ch] = (2.f * mu2[ch] * (A2 - A1)) / (B1 * B2) - S * (2.f * mu1[ch] / B1 - 2.f * mu1[ch] / B2);
                m11[ch] = -S / B2;
                m12[ch] = 2.f * A1 / (B1 * B2);
            }
        }
        if (inside) {
            const size_t o = base + (size_t)(y0 + ly) * W + x0 + lx;
            Mmu[o] = make_float4(mmu[0], mmu[1], mmu[2], 0.f);
            M11[o] = make_float4(m11[0], m11[1], m11[2], 0.f);
            M12[o] = make_float4(m12[0], m12[1], m12[2], 0.f);
        }
    }
    const float r0 = block_sum(s_sum, red), r1 = block_sum(l1, red), r2 = block_sum(l2, red);
    if (threadIdx.x == 0) {
        float* pp = partial + 3 * (((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
        pp[0] = r0;
        pp[1] = r1;
        pp[2] = r2;
    }
}

__global__ __launch_bounds__(256) void train_loss_grad_kernel(const float4* __restrict__ x, const float4* __restrict__ y,
                                                              const float* __restrict__ window, const float4* __restrict__ Mmu,
                                                              const float4* __restrict__ M11, const float4* __restrict__ M12,
                                                              float4* __restrict__ g, int B, int H, int W, float l1_w,
                                                              float ssim_w, float inv_n) {
    __shared__ float sw[121];
    if (threadIdx.x < 121) sw[threadIdx.x] = window[threadIdx.x];
    __syncthreads();
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * H * W) return;
    const int b = idx / (H * W);
    const int r = idx - b * H * W;
    const int qy = r / W, qx = r - qy * W;
    const float4 xv = x[idx], yv = y[idx];
    const float xa[3] = {xv.x, xv.y, xv.z}, ya[3] = {yv.x, yv.y, yv.z};
    float gout[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float d = xa[ch] - ya[ch];
        gout[ch] = l1_w * inv_n * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
    }
    if (ssim_w != 0.f) {
        // padded positions (q'y, q'x) whose replicate-clamped source is this pixel
        const int ylo = qy == 0 ? -SS_R : qy, yhi = qy == H - 1 ? H - 1 + SS_R : qy;
        const int xlo = qx == 0 ? -SS_R : qx, xhi = qx == W - 1 ? W - 1 + SS_R : qx;
        float acc[3] = {0, 0, 0};
        const size_t base = (size_t)b * H * W;
        for (int py = ylo; py <= yhi; ++py)
            for (int px = xlo; px <= xhi; ++px)
                // output pixels p whose 11x11 window covers the padded position: p = q' - k + R, k = 0..10
                for (int ky = 0; ky < 11; ++ky) {
                    const int oy = py - ky + SS_R;
                    if ((unsigned)oy >= (unsigned)H) continue;
                    for (int kx = 0; kx < 11; ++kx) {
                        const int ox = px - kx + SS_R;
                        if ((unsigned)ox >= (unsigned)W) continue;
                        const float w = sw[ky * 11 + kx];
                        const size_t o = base + (size_t)oy * W + ox;
                        const float4 a = Mmu[o], c = M11[o], e = M12[o];
                        acc[0] += w * (a.x + 2.f * xa[0] * c.x + ya[0] * e.x);
                        acc[1] += w * (a.y + 2.f * xa[1] * c.y + ya[1] * e.y);
                        acc[2] += w * (a.z + 2.f * xa[2] * c.z + ya[2] * e.z);
                    }
                }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) gout[ch] -= ssim_w * inv_n * acc[ch];
    }
    g[idx] = make_float4(gout[0], gout[1], gout[2], 0.f);
}

}  // namespace

extern "C" {

int spaa_train_loss_fwd_bwd(const float* infer, const float* target, const float* window, float l1_w, float ssim_w,
                            float* m_mu, float* m_11, float* m_12, float* partial, float* g_infer, int B, int H, int W,
                            spaa_stream_t stream) {
    if (!infer || !target || !window || !partial || !g_infer || B < 1 || H < 1 || W < 1 || B > 65535) return hipErrorInvalidValue;
    if (ssim_w != 0.f && (!m_mu || !m_11 || !m_12)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(train_loss_stats_kernel, dim3((W + SS_T - 1) / SS_T, (H + SS_T - 1) / SS_T, B), dim3(256), 0,
                       (hipStream_t)stream, (const float4*)infer, (const float4*)target, window, (float4*)m_mu, (float4*)m_11,
                       (float4*)m_12, partial, H, W, ssim_w != 0.f ? 1 : 0);
    const float inv_n = 1.f / (3.f * (float)B * (float)H * (float)W);
    hipLaunchKernelGGL(train_loss_grad_kernel, dim3((B * H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)infer, (const float4*)target, window, (const float4*)m_mu, (const float4*)m_11,
                       (const float4*)m_12, (float4*)g_infer, B, H, W, l1_w, ssim_w, inv_n);
    return (int)hipGetLastError();
}

int spaa_img_stats(const float* x, const float* y, const spaa_img_pair_t* pairs, const int32_t* tile_pair, int ntiles,
                   const float* window, float* partial, spaa_stream_t stream) {
    if (!x || !pairs || !tile_pair || !window || !partial || ntiles < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(img_stats_kernel, dim3(ntiles), dim3(256), 0, (hipStream_t)stream, x, y, pairs, tile_pair, window, partial);
    return (int)hipGetLastError();
}

int spaa_rgb2lab(const float* rgb, float* lab, int npix, spaa_stream_t stream) {
    if (!rgb || !lab || npix < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rgb2lab_kernel, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)rgb, (float4*)lab, npix);
    return (int)hipGetLastError();
}

int spaa_ciede2000(const float* lab1, const float* lab2, float* de, int npix, spaa_stream_t stream) {
    if (!lab1 || !lab2 || !de || npix < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ciede2000_kernel, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)lab1, (const float4*)lab2, de, npix);
    return (int)hipGetLastError();
}

int spaa_rgb2lab_bwd(const float* rgb, const float* g_lab, float* g_rgb, int npix, spaa_stream_t stream) {
    if (!rgb || !g_lab || !g_rgb || npix < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rgb2lab_bwd_kernel, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)rgb, (const float4*)g_lab, (float4*)g_rgb, npix);
    return (int)hipGetLastError();
}

int spaa_ciede2000_bwd(const float* lab1, const float* lab2, const float* g_de, float* g_lab1, float* g_lab2, int npix,
                       spaa_stream_t stream) {
    if (!lab1 || !lab2 || !g_de || (!g_lab1 && !g_lab2) || npix < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ciede2000_bwd_kernel, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)lab1, (const float4*)lab2, g_de, (float4*)g_lab1, (float4*)g_lab2, npix);
    return (int)hipGetLastError();
}

static int launch_stealth_loss(const float* y, const float* scene, const float* scene_lab, float caml2_w, float camdE_w,
                               const float* params, float gscale, float* g_y, float* de_map, float* partial, int B, int HW,
                               spaa_stream_t stream) {
    if (!y || !scene || !scene_lab || !g_y || !partial || B < 1 || HW < 1) return hipErrorInvalidValue;
    dim3 grid((HW + 255) / 256, B);
    hipLaunchKernelGGL(stealth_loss_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float4*)y,
                       (const float4*)scene, (const float4*)scene_lab, caml2_w, camdE_w, gscale, (float4*)g_y,
                       de_map, partial, HW, params);
    return (int)hipGetLastError();
}

int spaa_stealth_loss_fwd_bwd(const float* y, const float* scene, const float* scene_lab, float caml2_w,
                              float camdE_w, float gscale, float* g_y, float* de_map, float* partial, int B, int HW,
                              spaa_stream_t stream) {
    return launch_stealth_loss(y, scene, scene_lab, caml2_w, camdE_w, nullptr, gscale, g_y, de_map, partial, B, HW, stream);
}

int spaa_stealth_loss_fwd_bwd_ps(const float* y, const float* scene, const float* scene_lab, const float* params,
                                 float gscale, float* g_y, float* de_map, float* partial, int B, int HW, spaa_stream_t stream) {
    if (!params) return hipErrorInvalidValue;
    return launch_stealth_loss(y, scene, scene_lab, 0.f, 0.f, params, gscale, g_y, de_map, partial, B, HW, stream);
}

}  // extern "C"
