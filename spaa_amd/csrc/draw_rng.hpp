// draw_rng.hpp — the counter-based generator of the draw kernels (jitter_ops.hip, pose_ops.hip): 32-bit integer mixing, no state;
// tests/jitter_oracle.py and tests/pose_oracle.py restate it in Python integers.  And the launch grid of their per-draw image kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// the word of (seed, t, b, j, parameter index i) behind the first constant `first`: tables of one seed drawn behind different
// constants are independent
__device__ __forceinline__ uint32_t draw_word(uint32_t first, uint32_t seed, uint32_t t, uint32_t b, uint32_t j, uint32_t i) {
    uint32_t h = mix32(seed ^ first);
    h = mix32(h ^ t);
    h = mix32(h ^ b);
    h = mix32(h ^ j);
    return mix32(h ^ i);
}

// 2 u - 1 with u = (h >> 8) 2^-24: exact in fp32
__device__ __forceinline__ float signed_unit(uint32_t h) { return (float)((int32_t)(h >> 8) * 2 - (1 << 24)) * 0x1p-24f; }

// grid (ceil(HW / 256), J, B) of a kernel that handles one pixel of one draw per thread
inline bool image_grid(int B, int J, int H, int W, dim3& grid) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30) return false;
    grid = dim3((unsigned)((H * W + 255) / 256), (unsigned)J, (unsigned)B);
    return true;
}

}  // namespace
