// jpeg_ops.hip — camera JPEG for SPAA: J = 2..SPAA_JITTER_MAX codec round trips of the camera image per iteration, each
// at a quality of its own drawn on the device, and the adjoint of the round trip with the coefficient rounding replaced by a factor.
//
//   spaa_jpeg_draw   the per-(sample, draw) quality rows of iteration t = counter[0]; stores t + 1
//   spaa_jpeg_fwd    out_j = decode(encode(y_j, Q_bj)): clamp, JFIF YCbCr, edge-replicated padding to the MCU, 2 x 2 chroma means
//                    (4:2:0), 8 x 8 DCT, the quantisation table of Q built in the workgroup, rounding, IDCT, triangle chroma upsampling
//                    (4:2:0), RGB, the 8-bit step; and the gate byte
//   spaa_jpeg_bwd    g_y_j = the transpose of that chain's linear parts applied to g_out_j, the coefficient rounding as the factor phi
//                    (1, or 3 r^2 from the forward coefficients recomputed from y_j); a gather, no atomics: bitwise repeatable
//
// Conventions as in jitter_ops.hip: per-draw tensors are HOST arrays of J device pointers that travel in a by-value kernel argument;
// the generator is jitter's counter-based one with another first constant (tests/jpeg_oracle.py restates it in Python integers).
//
// A workgroup of 256 threads owns a 32 x 32 pixel tile (a multiple of both MCUs, so padding cells, chroma means and every 8 x 8 block
// of the tile are its own) as planes in LDS with a row stride of 33 floats (17 for the 16 x 16 chroma planes of 4:2:0): a thread runs
// one 8-point transform along a row or a column of a block, and with that stride the 32 lanes of a half wave touch 32 different banks
// in both directions.  4:4:4 is one launch.  4:2:0 forward is two: the triangle filter reads decoded chroma of the neighbouring tiles,
// so the first launch leaves the decoded planes (level-shifted Y at full, Cb and Cr at half resolution, padded sizes) in a planar
// workspace and the second one filters, converts and rounds per pixel.  The adjoint's halo is on its INPUT side (one pixel of g_out
// and gate around the tile), so it stays one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "ptr_table.hpp"
#include "draw_rng.hpp"

namespace {

template <typename T>
using Draws = PtrTable<T, SPAA_JITTER_MAX>;

constexpr int TILE = 32, LD = TILE + 1, CT = TILE / 2, CLD = CT + 1;

// ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural (row-major) order
__constant__ uint8_t BASE_TABLE[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68, 109, 103,  77,  24, 35, 55, 64, 81, 104, 113,  92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// entry i of table `which` at quality Q in 1..100, scaled as libjpeg scales it
__device__ __forceinline__ float quant_entry(int which, int i, int Q) {
    const int s = Q < 50 ? 5000 / Q : 200 - 2 * Q;
    const int t = ((int)BASE_TABLE[which][i] * s + 50) / 100;
    return (float)(t < 1 ? 1 : (t > 255 ? 255 : t));
}

// the quality of a table row: 0 is the identity row, anything else is brought into 1..100
__device__ __forceinline__ int quality_of(const float4 r) {
    const int q = (int)r.x;
    return q <= 0 ? 0 : (q > 100 ? 100 : q);
}

// the word of (seed, t, b, j, parameter index i): jitter's chain behind a first constant of its own
__device__ __forceinline__ uint32_t draw_word(uint32_t seed, uint32_t t, uint32_t b, uint32_t j, uint32_t i) {
    return draw_word(0xc2b2ae35u, seed, t, b, j, i);
}

// One workgroup; rows = B * J; n = q_hi - q_lo + 1
__global__ __launch_bounds__(256) void jpeg_draw_kernel(uint32_t seed, int32_t* __restrict__ counter, int q_lo, uint32_t n, int clean0,
                                                        float4* __restrict__ row, int rows, int J) {
    const uint32_t t = (uint32_t)counter[0];
    for (int r = threadIdx.x; r < rows; r += 256) {
        const uint32_t b = (uint32_t)(r / J), j = (uint32_t)(r % J);
        const int q = (clean0 && j == 0) ? 0 : q_lo + (int)(((draw_word(seed, t, b, j, 0) >> 8) * n) >> 24);
        row[r] = make_float4((float)q, 0.f, 0.f, 0.f);
    }
    __syncthreads();   // every thread has read t
    if (threadIdx.x == 0) counter[0] = (int32_t)(t + 1u);
}

// D[u][x] = a(u) cos((2x + 1) u pi / 16), a(0) = sqrt(1/8), a(u) = 1/2: the orthonormal DCT-II matrix.  Called with unrolled indices
// only, so every value is an immediate.
__device__ __forceinline__ float dct_coef(int u, int x) {
    constexpr float HALF_COS[9] = {0.5f,          0.4903926402f, 0.4619397663f, 0.4157348062f, 0.3535533906f,
                                   0.2777851165f, 0.1913417162f, 0.0975451610f, 0.f};   // cos(k pi / 16) / 2
    if (u == 0) return 0.3535533906f;
    const int k = ((2 * x + 1) * u) & 31;
    int m = k > 16 ? 32 - k : k;
    float s = 1.f;
    if (m > 8) {
        m = 16 - m;
        s = -1.f;
    }
    return s * HALF_COS[m];
}

// o[u] = sum_x D[u][x] v[x]
__device__ __forceinline__ void dct8(const float (&v)[8], float (&o)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float a = 0.f;
#pragma unroll
        for (int x = 0; x < 8; ++x) a = fmaf(dct_coef(u, x), v[x], a);
        o[u] = a;
    }
}

// o[x] = sum_u D[u][x] c[u]
__device__ __forceinline__ void idct8(const float (&c)[8], float (&o)[8]) {
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        float a = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) a = fmaf(dct_coef(u, x), c[u], a);
        o[x] = a;
    }
}

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }
__device__ __forceinline__ int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The 8 x 8 blocks of a tile.  SUB = 0 (4:4:4): 16 blocks in each of the three 32 x 32 planes.  SUB = 1 (4:2:0): the 16 blocks of the
// Y plane, then 4 in each 16 x 16 chroma plane.  `on`: the block lies inside the padded image.
struct Block {
    int plane, row, col, ld, table;
    bool on;
};
template <int SUB>
__device__ __forceinline__ Block block_of(int blk, int r0, int c0, int Hp, int Wp) {
    Block k;
    if (!SUB || blk < 16) {
        k.plane = blk >> 4;
        k.row = ((blk >> 2) & 3) * 8;
        k.col = (blk & 3) * 8;
        k.ld = LD;
        k.on = r0 + k.row < Hp && c0 + k.col < Wp;
    } else {
        const int cb = blk - 16;
        k.plane = 1 + (cb >> 2);
        k.row = ((cb >> 1) & 1) * 8;
        k.col = (cb & 1) * 8;
        k.ld = CLD;
        k.on = r0 / 2 + k.row < Hp / 2 && c0 / 2 + k.col < Wp / 2;
    }
    k.table = k.plane ? 1 : 0;
    return k;
}
template <int SUB>
constexpr int lines_of() { return (SUB ? 24 : 48) * 8; }

// the planes of a tile in LDS: full[3] at 32 x 32 (4:2:0 uses full[0] for Y and full[1..2] before the means), half[2] at 16 x 16
template <int SUB>
struct Planes {
    float full[3][TILE][LD];
    float half[SUB ? 2 : 1][CT][CLD];
    __device__ __forceinline__ float* at(const Block& k) {
        return (SUB && k.ld == CLD) ? &half[k.plane - 1][k.row][k.col] : &full[k.plane][k.row][k.col];
    }
};

// level-shifted JFIF YCbCr of p = 255 clamp(y, 0, 1), and the in-gate bits 0-2
__device__ __forceinline__ unsigned encode_pixel(const float4 v, float& Y, float& Cb, float& Cr) {
    const unsigned bits = ((v.x >= 0.f && v.x <= 1.f) ? 1u : 0u) | ((v.y >= 0.f && v.y <= 1.f) ? 2u : 0u) |
                          ((v.z >= 0.f && v.z <= 1.f) ? 4u : 0u);
    const float R = 255.f * fminf(fmaxf(v.x, 0.f), 1.f), G = 255.f * fminf(fmaxf(v.y, 0.f), 1.f), B = 255.f * fminf(fmaxf(v.z, 0.f), 1.f);
    Y = 0.299f * R + 0.587f * G + 0.114f * B - 128.f;
    Cb = -0.168736f * R - 0.331264f * G + 0.5f * B;
    Cr = 0.5f * R - 0.418688f * G - 0.081312f * B;
    return bits;
}

// RGB of the decoded level-shifted planes, rounded to 8 bits; adds the out-gate bits 4-6 to `bits`
__device__ __forceinline__ float4 decode_pixel(float Ys, float Cb, float Cr, unsigned& bits) {
    const float Y = Ys + 128.f;
    const float v[3] = {Y + 1.402f * Cr, Y - 0.344136f * Cb - 0.714136f * Cr, Y + 1.772f * Cb};
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        bits |= (v[c] >= 0.f && v[c] <= 255.f) ? (16u << c) : 0u;
        o[c] = rintf(fminf(fmaxf(v[c], 0.f), 255.f)) / 255.f;
    }
    return make_float4(o[0], o[1], o[2], 0.f);
}

// The tile's pixels of y as level-shifted planes (rows and columns beyond the image repeat its last one: the encoder's padding), and
// for 4:2:0 the 2 x 2 means of Cb and Cr.  Thread t holds pixels t + 256 q, q = 0..3: row (t >> 5) + 8 q, column t & 31.  Ends with
// a barrier.
template <int SUB>
__device__ __forceinline__ void load_planes(Planes<SUB>& P, const float4* __restrict__ yb, int r0, int c0, int H, int W,
                                            unsigned (&inbits)[4]) {
    const int lc = threadIdx.x & 31;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int lr = (threadIdx.x >> 5) + 8 * q;
        const int gi = min(r0 + lr, H - 1), gk = min(c0 + lc, W - 1);
        float Y, Cb, Cr;
        inbits[q] = encode_pixel(yb[(size_t)gi * W + gk], Y, Cb, Cr);
        P.full[0][lr][lc] = Y;
        P.full[1][lr][lc] = Cb;
        P.full[2][lr][lc] = Cr;
    }
    __syncthreads();
    if (SUB) {
        const int cr = threadIdx.x >> 4, cc = threadIdx.x & 15;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const float (*f)[LD] = P.full[1 + pl];
            P.half[pl][cr][cc] = 0.25f * ((f[2 * cr][2 * cc] + f[2 * cr][2 * cc + 1]) + (f[2 * cr + 1][2 * cc] + f[2 * cr + 1][2 * cc + 1]));
        }
        __syncthreads();
    }
}

// the row pass of the forward DCT over every block of the planes, in place; no barrier
template <int SUB>
__device__ __forceinline__ void dct_rows(Planes<SUB>& P, int r0, int c0, int Hp, int Wp) {
    for (int t = threadIdx.x; t < lines_of<SUB>(); t += 256) {
        const Block k = block_of<SUB>(t >> 3, r0, c0, Hp, Wp);
        if (!k.on) continue;
        float* p = P.at(k) + (t & 7) * k.ld;
        float v[8], o[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) v[x] = p[x];
        dct8(v, o);
#pragma unroll
        for (int x = 0; x < 8; ++x) p[x] = o[x];
    }
}

// the row pass of the inverse DCT, in place; no barrier
template <int SUB>
__device__ __forceinline__ void idct_rows(Planes<SUB>& P, int r0, int c0, int Hp, int Wp) {
    for (int t = threadIdx.x; t < lines_of<SUB>(); t += 256) {
        const Block k = block_of<SUB>(t >> 3, r0, c0, Hp, Wp);
        if (!k.on) continue;
        float* p = P.at(k) + (t & 7) * k.ld;
        float v[8], o[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) v[x] = p[x];
        idct8(v, o);
#pragma unroll
        for (int x = 0; x < 8; ++x) p[x] = o[x];
    }
}

struct Tile {
    int r0, c0, Hp, Wp;
};
template <int SUB>
__device__ __forceinline__ Tile tile_of(int H, int W, int tiles_x) {
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    constexpr int MCU = SUB ? 16 : 8;
    return Tile{ty * TILE, tx * TILE, round_up(H, MCU), round_up(W, MCU)};
}

// grid (tiles, J, B).  SUB = 0 writes out and gate; SUB = 1 writes the in-gate bits and the decoded planes of draw j, sample b to
// ws + (j B + b) Hp Wp 3/2: Y [Hp][Wp], Cb [Hp/2][Wp/2], Cr [Hp/2][Wp/2].  The identity row copies y in both.
template <int SUB>
__global__ __launch_bounds__(256) void jpeg_fwd_kernel(const Draws<const float> y, const float4* __restrict__ row, const Draws<float> out,
                                                       const Draws<uint8_t> gate, float* __restrict__ ws, int H, int W, int tiles_x) {
    __shared__ Planes<SUB> P;
    __shared__ float T[2][64];
    const int j = blockIdx.y, J = gridDim.y, b = blockIdx.z, B = gridDim.z;
    const Tile tl = tile_of<SUB>(H, W, tiles_x);
    const int r0 = tl.r0, c0 = tl.c0, Hp = tl.Hp, Wp = tl.Wp;
    const size_t HW = (size_t)H * W;
    const int Q = quality_of(row[(size_t)b * J + j]);
    const float4* yb = reinterpret_cast<const float4*>(ptr_of(y, j)) + (size_t)b * HW;
    float4* ob = reinterpret_cast<float4*>(ptr_of(out, j)) + (size_t)b * HW;
    uint8_t* gb = ptr_of(gate, j) + (size_t)b * HW;
    const int lc = threadIdx.x & 31;
    if (Q == 0) {   // (uniform per workgroup)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gi = r0 + (threadIdx.x >> 5) + 8 * q, gk = c0 + lc;
            if (gi < H && gk < W) {
                const float4 v = yb[(size_t)gi * W + gk];
                ob[(size_t)gi * W + gk] = make_float4(v.x, v.y, v.z, 0.f);
                gb[(size_t)gi * W + gk] = 0x77;
            }
        }
        return;
    }
    if (threadIdx.x < 128) T[threadIdx.x >> 6][threadIdx.x & 63] = quant_entry(threadIdx.x >> 6, threadIdx.x & 63, Q);
    unsigned inbits[4];
    load_planes<SUB>(P, yb, r0, c0, H, W, inbits);
    dct_rows<SUB>(P, r0, c0, Hp, Wp);
    __syncthreads();
    // columns: the second DCT pass gives the coefficients of column u; round them and run the first inverse pass on the spot
    for (int t = threadIdx.x; t < lines_of<SUB>(); t += 256) {
        const Block k = block_of<SUB>(t >> 3, r0, c0, Hp, Wp);
        if (!k.on) continue;
        const int u = t & 7;
        float* p = P.at(k) + u;
        float v[8], c[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[i * k.ld];
        dct8(v, c);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float tq = T[k.table][i * 8 + u];
            c[i] = rintf(c[i] / tq) * tq;
        }
        idct8(c, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i * k.ld] = v[i];
    }
    __syncthreads();
    idct_rows<SUB>(P, r0, c0, Hp, Wp);
    __syncthreads();
    if (!SUB) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int lr = (threadIdx.x >> 5) + 8 * q;
            const int gi = r0 + lr, gk = c0 + lc;
            if (gi < H && gk < W) {
                unsigned bits = inbits[q];
                ob[(size_t)gi * W + gk] = decode_pixel(P.full[0][lr][lc], P.full[1][lr][lc], P.full[2][lr][lc], bits);
                gb[(size_t)gi * W + gk] = (uint8_t)bits;
            }
        }
    } else {
        const int Hc = Hp / 2, Wc = Wp / 2;
        float* wy = ws + ((size_t)j * B + b) * ((size_t)Hp * Wp / 2 * 3);
        float* wc = wy + (size_t)Hp * Wp;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int lr = (threadIdx.x >> 5) + 8 * q;
            const int gi = r0 + lr, gk = c0 + lc;
            if (gi < Hp && gk < Wp) wy[(size_t)gi * Wp + gk] = P.full[0][lr][lc];
            if (gi < H && gk < W) gb[(size_t)gi * W + gk] = (uint8_t)inbits[q];
        }
        const int cr = threadIdx.x >> 4, cc = threadIdx.x & 15;
        const int ci = r0 / 2 + cr, ck = c0 / 2 + cc;
        if (ci < Hc && ck < Wc) {
            wc[(size_t)ci * Wc + ck] = P.half[0][cr][cc];
            wc[(size_t)Hc * Wc + (size_t)ci * Wc + ck] = P.half[1][cr][cc];
        }
    }
}

// one axis of the triangle filter over n samples: full-resolution index i reads (3 c[near] + c[far]) / 4, far clamped to the plane
struct Tri {
    int near, far;
};
__device__ __forceinline__ Tri tri_of(int i, int n) {
    const int near = i >> 1;
    return Tri{near, clampi(near + ((i & 1) ? 1 : -1), n)};
}

// 4:2:0, second launch: grid (ceil(HW / 256), J, B), one pixel per thread
__global__ __launch_bounds__(256) void jpeg_up_kernel(const float4* __restrict__ row, const float* __restrict__ ws, const Draws<float> out,
                                                      const Draws<uint8_t> gate, int H, int W) {
    const int j = blockIdx.y, J = gridDim.y, b = blockIdx.z, B = gridDim.z;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    if (quality_of(row[(size_t)b * J + j]) == 0) return;   // the first launch has copied y
    const int Hp = round_up(H, 16), Wp = round_up(W, 16), Hc = Hp / 2, Wc = Wp / 2;
    const float* wy = ws + ((size_t)j * B + b) * ((size_t)Hp * Wp / 2 * 3);
    const float* wc = wy + (size_t)Hp * Wp;
    const int i = pix / W, k = pix - i * W;
    const Tri ti = tri_of(i, Hc), tk = tri_of(k, Wc);
    float ch[2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        const float* c = wc + (size_t)pl * Hc * Wc;
        const float a = 0.75f * c[(size_t)ti.near * Wc + tk.near] + 0.25f * c[(size_t)ti.near * Wc + tk.far];
        const float f = 0.75f * c[(size_t)ti.far * Wc + tk.near] + 0.25f * c[(size_t)ti.far * Wc + tk.far];
        ch[pl] = 0.75f * a + 0.25f * f;
    }
    const size_t at = (size_t)b * H * W + pix;
    unsigned bits = ptr_of(gate, j)[at] & 7u;
    reinterpret_cast<float4*>(ptr_of(out, j))[at] = decode_pixel(wy[(size_t)i * Wp + k], ch[0], ch[1], bits);
    ptr_of(gate, j)[at] = (uint8_t)bits;
}

// the weight with which full-resolution index i of the triangle filter reads chroma index ci
__device__ __forceinline__ float tri_weight(int i, int ci, int n) {
    const Tri t = tri_of(i, n);
    return (t.near == ci ? 0.75f : 0.f) + (t.far == ci ? 0.25f : 0.f);
}

// grid (tiles, J, B)
template <int SUB>
__global__ __launch_bounds__(256) void jpeg_bwd_kernel(const Draws<const float> g_out, const Draws<const float> y,
                                                       const float4* __restrict__ row, int soft, const Draws<const uint8_t> gate,
                                                       const Draws<float> g_y, int H, int W, int tiles_x) {
    constexpr int HALO = SUB, HT = TILE + 2 * HALO;
    __shared__ Planes<SUB> F;   // the forward planes (soft only)
    __shared__ Planes<SUB> G;   // the gradient planes
    __shared__ float GH[SUB ? 2 : 1][SUB ? HT : 1][SUB ? HT + 1 : 1];   // 4:2:0: d/d(upsampled Cb, Cr) with one pixel around the tile
    __shared__ float T[2][64];
    const int j = blockIdx.y, J = gridDim.y, b = blockIdx.z;
    const Tile tl = tile_of<SUB>(H, W, tiles_x);
    const int r0 = tl.r0, c0 = tl.c0, Hp = tl.Hp, Wp = tl.Wp;
    const size_t HW = (size_t)H * W;
    const int Q = quality_of(row[(size_t)b * J + j]);
    const float4* gob = reinterpret_cast<const float4*>(ptr_of(g_out, j)) + (size_t)b * HW;
    const uint8_t* gb = ptr_of(gate, j) + (size_t)b * HW;
    float4* gyb = reinterpret_cast<float4*>(ptr_of(g_y, j)) + (size_t)b * HW;
    const int lc = threadIdx.x & 31;
    if (Q == 0) {   // (uniform per workgroup)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gi = r0 + (threadIdx.x >> 5) + 8 * q, gk = c0 + lc;
            if (gi < H && gk < W) {
                const float4 g = gob[(size_t)gi * W + gk];
                gyb[(size_t)gi * W + gk] = make_float4(g.x, g.y, g.z, 0.f);
            }
        }
        return;
    }
    // the transposes of the 8-bit step (straight-through), the out-gate and the YCbCr -> RGB matrix; zero beyond the image (the crop)
    for (int idx = threadIdx.x; idx < HT * HT; idx += 256) {
        const int hr = idx / HT, hc = idx - hr * HT;
        const int gi = r0 - HALO + hr, gk = c0 - HALO + hc;
        float gR = 0.f, gG = 0.f, gB = 0.f;
        if (gi >= 0 && gi < H && gk >= 0 && gk < W) {
            const float4 g = gob[(size_t)gi * W + gk];
            const unsigned bits = gb[(size_t)gi * W + gk];
            gR = (bits & 16u) ? g.x * (1.f / 255.f) : 0.f;
            gG = (bits & 32u) ? g.y * (1.f / 255.f) : 0.f;
            gB = (bits & 64u) ? g.z * (1.f / 255.f) : 0.f;
        }
        const float gCb = -0.344136f * gG + 1.772f * gB, gCr = 1.402f * gR - 0.714136f * gG;
        if (!SUB) {
            G.full[0][hr][hc] = gR + gG + gB;
            G.full[1][hr][hc] = gCb;
            G.full[2][hr][hc] = gCr;
        } else {
            if (hr >= HALO && hr < HALO + TILE && hc >= HALO && hc < HALO + TILE) G.full[0][hr - HALO][hc - HALO] = gR + gG + gB;
            GH[0][hr][hc] = gCb;
            GH[1][hr][hc] = gCr;
        }
    }
    __syncthreads();
    if (SUB) {   // the transpose of the triangle filter as a gather: chroma pixel (ci, ck) from the 4 x 4 pixels that read it
        const int Hc = Hp / 2, Wc = Wp / 2;
        const int cr = threadIdx.x >> 4, cc = threadIdx.x & 15;
        const int ci = r0 / 2 + cr, ck = c0 / 2 + cc;
        float acc[2] = {0.f, 0.f};
        for (int di = -1; di <= 2; ++di) {
            const int i = 2 * ci + di;
            if (i < 0 || i >= Hp) continue;
            const float wi = tri_weight(i, ci, Hc);
            float line[2] = {0.f, 0.f};
            for (int dk = -1; dk <= 2; ++dk) {
                const int k = 2 * ck + dk;
                if (k < 0 || k >= Wp) continue;
                const float wk = tri_weight(k, ck, Wc);
                line[0] += wk * GH[0][2 * cr + di + HALO][2 * cc + dk + HALO];
                line[1] += wk * GH[1][2 * cr + di + HALO][2 * cc + dk + HALO];
            }
            acc[0] += wi * line[0];
            acc[1] += wi * line[1];
        }
        G.half[0][cr][cc] = acc[0];
        G.half[1][cr][cc] = acc[1];
    }
    unsigned inbits[4];
    if (soft) {   // (uniform) the forward coefficients again, for phi
        if (threadIdx.x < 128) T[threadIdx.x >> 6][threadIdx.x & 63] = quant_entry(threadIdx.x >> 6, threadIdx.x & 63, Q);
        load_planes<SUB>(F, reinterpret_cast<const float4*>(ptr_of(y, j)) + (size_t)b * HW, r0, c0, H, W, inbits);
        dct_rows<SUB>(F, r0, c0, Hp, Wp);
    } else {
        __syncthreads();
    }
    // the transpose of the inverse DCT is the forward DCT: rows, then columns
    dct_rows<SUB>(G, r0, c0, Hp, Wp);
    __syncthreads();
    for (int t = threadIdx.x; t < lines_of<SUB>(); t += 256) {
        const Block k = block_of<SUB>(t >> 3, r0, c0, Hp, Wp);
        if (!k.on) continue;
        const int u = t & 7;
        float v[8], gc[8];
        float* p = G.at(k) + u;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[i * k.ld];
        dct8(v, gc);
        if (soft) {
            const float* f = F.at(k) + u;
            float c[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = f[i * k.ld];
            dct8(v, c);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float s = c[i] / T[k.table][i * 8 + u];
                const float r = s - rintf(s);
                gc[i] *= 3.f * r * r;
            }
        }
        idct8(gc, v);   // the transpose of the forward DCT's column pass
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i * k.ld] = v[i];
    }
    __syncthreads();
    idct_rows<SUB>(G, r0, c0, Hp, Wp);
    __syncthreads();
    // the transposes of the 2 x 2 mean, of the padding (the last row / column collects its copies), of the RGB -> YCbCr matrix and of
    // 255 clamp
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int gi = r0 + (threadIdx.x >> 5) + 8 * q, gk = c0 + lc;
        if (gi >= H || gk >= W) continue;
        const int i1 = gi == H - 1 ? Hp - 1 : gi, k1 = gk == W - 1 ? Wp - 1 : gk;
        float sY = 0.f, sCb = 0.f, sCr = 0.f;
        for (int i = gi; i <= i1; ++i)
            for (int k = gk; k <= k1; ++k) {
                sY += G.full[0][i - r0][k - c0];
                if (!SUB) {
                    sCb += G.full[1][i - r0][k - c0];
                    sCr += G.full[2][i - r0][k - c0];
                } else {
                    sCb += 0.25f * G.half[0][(i - r0) >> 1][(k - c0) >> 1];
                    sCr += 0.25f * G.half[1][(i - r0) >> 1][(k - c0) >> 1];
                }
            }
        const unsigned bits = gb[(size_t)gi * W + gk];
        const float gR = 0.299f * sY - 0.168736f * sCb + 0.5f * sCr;
        const float gG = 0.587f * sY - 0.331264f * sCb - 0.418688f * sCr;
        const float gB = 0.114f * sY + 0.5f * sCb - 0.081312f * sCr;
        gyb[(size_t)gi * W + gk] = make_float4((bits & 1u) ? 255.f * gR : 0.f, (bits & 2u) ? 255.f * gG : 0.f, (bits & 4u) ? 255.f * gB : 0.f, 0.f);
    }
}

// grid (tiles, J, B) of the tile kernels
inline bool tile_grid(int B, int J, int H, int W, dim3& grid, int& tiles_x) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30) return false;
    tiles_x = (W + TILE - 1) / TILE;
    grid = dim3((unsigned)(((H + TILE - 1) / TILE) * tiles_x), (unsigned)J, (unsigned)B);
    return true;
}

inline bool subsampling_ok(int s) { return s == SPAA_JPEG_444 || s == SPAA_JPEG_420; }

}  // namespace

extern "C" {

int64_t spaa_jpeg_ws_floats(int subsampling, int J, int B, int H, int W) {
    if (subsampling != SPAA_JPEG_420 || J < 1 || B < 1 || H < 1 || W < 1) return 0;
    return (int64_t)J * B * ((int64_t)((H + 15) / 16 * 16) * ((W + 15) / 16 * 16) / 2 * 3);
}

int spaa_jpeg_draw(uint32_t seed, int32_t* counter, int q_lo, int q_hi, int clean0, float* row, int B, int J, spaa_stream_t stream) {
    if (!counter || !row || B < 1 || B > (1 << 24) || J < 2 || J > SPAA_JITTER_MAX || q_lo < 1 || q_hi > 100 || q_lo > q_hi)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, seed, counter, q_lo, (uint32_t)(q_hi - q_lo + 1),
                       clean0, (float4*)row, B * J, J);
    return (int)hipGetLastError();
}

int spaa_jpeg_fwd(const float* const* y, const float* row, int J, int subsampling, float* const* out, uint8_t* const* gate, float* ws,
                  int B, int H, int W, spaa_stream_t stream) {
    Draws<const float> in;
    Draws<float> o;
    Draws<uint8_t> gt;
    dim3 grid, pixels;
    int tiles_x;
    if (!gather(in, y, J) || !gather(o, out, J) || !gather(gt, gate, J) || !row || !subsampling_ok(subsampling) ||
        (subsampling == SPAA_JPEG_420 && !ws) || !tile_grid(B, J, H, W, grid, tiles_x) || !image_grid(B, J, H, W, pixels))
        return hipErrorInvalidValue;
    if (subsampling == SPAA_JPEG_444) {
        hipLaunchKernelGGL(jpeg_fwd_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, in, (const float4*)row, o, gt, ws, H, W, tiles_x);
    } else {
        hipLaunchKernelGGL(jpeg_fwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, in, (const float4*)row, o, gt, ws, H, W, tiles_x);
        hipLaunchKernelGGL(jpeg_up_kernel, pixels, dim3(256), 0, (hipStream_t)stream, (const float4*)row, (const float*)ws, o, gt, H, W);
    }
    return (int)hipGetLastError();
}

int spaa_jpeg_bwd(const float* const* g_out, const float* const* y, const float* row, int J, int subsampling, int soft,
                  const uint8_t* const* gate, float* const* g_y, int B, int H, int W, spaa_stream_t stream) {
    Draws<const float> g, in;
    Draws<const uint8_t> gt;
    Draws<float> o;
    dim3 grid;
    int tiles_x;
    if (!gather(g, g_out, J) || !gather(in, y, J) || !gather(gt, gate, J) || !gather(o, g_y, J) || !row || !subsampling_ok(subsampling) ||
        !tile_grid(B, J, H, W, grid, tiles_x))
        return hipErrorInvalidValue;
    if (subsampling == SPAA_JPEG_444)
        hipLaunchKernelGGL(jpeg_bwd_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, g, in, (const float4*)row, soft, gt, o, H, W, tiles_x);
    else
        hipLaunchKernelGGL(jpeg_bwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, g, in, (const float4*)row, soft, gt, o, H, W, tiles_x);
    return (int)hipGetLastError();
}

}  // extern "C"
