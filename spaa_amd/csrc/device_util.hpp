// device_util.hpp — device-side primitives shared by the kernels (launch_util.hpp holds the host-side helpers): vector types,
// the exact fp32 -> three-bf16 split and the six-product MFMA sum of the bf16x6 arithmetic, wave-uniform buffer descriptors,
// the LDS-DMA piece and the fixed-order block sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// ---- bf16x6: every fp32 operand x == h + m + l exactly (three bf16), a product = six bf16 MFMAs with fp32 accumulation

// two fp32 -> two bf16 (round to nearest even) packed in one word; lo_f / hi_f give them back as fp32
__device__ __forceinline__ unsigned int cvt2(float a, float b) {
    f2 v = {a, b};
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float lo_f(unsigned int p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float hi_f(unsigned int p) { return __builtin_bit_cast(float, p & 0xffff0000u); }

// 8 fp32 -> three bf16x8 with x == h + m + l exactly
__device__ __forceinline__ void split8(const float (&x)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
    u4 hh, mm, ll;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned int ph = cvt2(x[2 * i], x[2 * i + 1]);
        const float r0 = x[2 * i] - lo_f(ph), r1 = x[2 * i + 1] - hi_f(ph);
        const unsigned int pm = cvt2(r0, r1);
        const float s0 = r0 - lo_f(pm), s1 = r1 - hi_f(pm);
        hh[i] = ph;
        mm[i] = pm;
        ll[i] = cvt2(s0, s1);
    }
    h = __builtin_bit_cast(bf16x8, hh);
    m = __builtin_bit_cast(bf16x8, mm);
    l = __builtin_bit_cast(bf16x8, ll);
}
__device__ __forceinline__ void split8(const f4 a, const f4 b, bf16x8& h, bf16x8& m, bf16x8& l) {
    const float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    split8(x, h, m, l);
}
__device__ __forceinline__ void split8(const u32x4 a, const u32x4 b, bf16x8& h, bf16x8& m, bf16x8& l) {   // fp32 bits
    const float x[8] = {__uint_as_float(a[0]), __uint_as_float(a[1]), __uint_as_float(a[2]), __uint_as_float(a[3]),
                        __uint_as_float(b[0]), __uint_as_float(b[1]), __uint_as_float(b[2]), __uint_as_float(b[3])};
    split8(x, h, m, l);
}

// Six of the nine partial products of (w0 + w1 + w2) . (p0 + p1 + p2) on v_mfma_f32_16x16x32_bf16 (the three dropped ones are below
// 2^-24 relative).  The small terms come first: they are summed among themselves before w0 . p0 joins the fp32 accumulator, so fewer
// of their low bits are rounded away.  Every bf16x6 kernel uses this order, and the parity tests pin the fp32 results it gives.
__device__ __forceinline__ f32x4 mfma6(const bf16x8 w0, const bf16x8 w1, const bf16x8 w2, const bf16x8 p0, const bf16x8 p1, const bf16x8 p2,
                                       f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2, p0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, p2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, p1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, p0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, p1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, p0, acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ f32x4 mfma6(const bf16x8 (&w)[3], const bf16x8 (&p)[3], f32x4 acc) {
    return mfma6(w[0], w[1], w[2], p[0], p[1], p[2], acc);
}

// ---- buffer descriptors and LDS-DMA

// the descriptor's flags word (dword 3) for raw 32-bit buffer access on gfx950
constexpr int BUF_RSRC_FLAGS = 0x00020000;

// wave-uniform descriptor of `bytes` bytes at `ptr`: the address halves and the size through readfirstlane, so that the
// descriptor sits in SGPRs.  (readfirstlane returns a SIGNED int: the halves are kept in uint32_t, or a low word with bit 31 set
// would sign-extend into the high word of the base address.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wave_rsrc(const void* ptr, const int bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(ptr);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)a), hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, __builtin_amdgcn_readfirstlane(bytes),
                                             BUF_RSRC_FLAGS);
}
// the same for a tensor that may be absent: a NULL tensor has no records (loads give zero, stores are dropped)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_or_empty(const void* ptr, const int64_t bytes) {
    return wave_rsrc(ptr, ptr != nullptr ? (int)bytes : 0);
}

// One LDS-DMA piece: 64 lanes x 16 bytes, global (buffer, per-lane byte offset `voff` + uniform `soff`) -> LDS at the
// wave-uniform address `dst` + 16 * lane.  An out-of-range offset writes zeros.  (A __device__ helper: the builtin has no
// host-side meaning and would silently drop the kernel's host stub if it sat in the kernel template itself.)
__device__ __forceinline__ void dma16(const __amdgpu_buffer_rsrc_t rsrc, unsigned char* dst, int voff, int soff = 0) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)dst, 16, voff, soff, 0, 0);
}

// ---- reductions

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// fixed-order block reduction (256 threads: wave shuffle, then the four wave partials through LDS `red[4]`); result valid in every thread
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

}  // namespace
