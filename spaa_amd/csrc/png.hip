// png.hip — the device half of the PNG encoder behind io.save_imgs (spaa_amd/png.py holds the host half):
//   spaa_png_filter_hist   images -> PNG scanline streams (per-row choice among the five filters), their byte histograms and the
//                          per-row Adler-32 partial sums
//   spaa_png_pack          scanline streams + per-image Huffman tables and block header -> the complete deflate streams, ragged
// The deflate stream is one dynamic-Huffman block of literals only (no LZ77 matching): after the row filters the entropy code
// carries almost all of the compression for camera-like images, and every step is data-parallel.  All five filters are computed from
// the unfiltered neighbours, so rows are independent.  Everything is integer arithmetic; the only atomics are integer adds and ORs,
// which commute: the bytes are the same on every run, and a numpy restatement (tests/png_hip_oracle.py) reproduces them exactly.
// Byte-bound streams, written plainly: 256-thread workgroups, rows and symbol chunks staged in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"

namespace {

constexpr int ROWS_PER_WG = 8;           // rows one workgroup filters before it flushes its LDS histogram
constexpr int MAX_ROW_BYTES = 30000;     // 3 W: two rows of the image are staged in LDS
constexpr int RUN = 16;                  // packer: consecutive symbols per thread
constexpr int CHUNK = 256 * RUN;         // packer: symbols per workgroup
constexpr int HDR_WORDS = 64;            // block header: at most 2048 bits per image
constexpr uint32_t ADLER_MOD = 65521u;

// np.uint8(x * 255) for x in [0, 1]: one fp32 multiply, truncation toward zero, the low 8 bits
__device__ __forceinline__ uint8_t to_byte(float v) { return (uint8_t)(int32_t)(v * 255.0f); }

template <typename T>
__device__ __forceinline__ T wave_sum_u(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// PNG predictors from the unfiltered left (a), up (b), upper-left (c) bytes
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int predict(int k, int a, int b, int c) {
    switch (k) {
        case 0: return 0;
        case 1: return a;
        case 2: return b;
        case 3: return (a + b) >> 1;
        default: return paeth(a, b, c);
    }
}

__device__ __forceinline__ uint32_t cost_of(int x, int pred) {
    const int v = (x - pred) & 255;
    return (uint32_t)(v < 128 ? v : 256 - v);
}

// hist [N][257]: zero, bin 256 (end of block) = 1
__global__ void hist_init_kernel(uint32_t* __restrict__ hist, int total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) hist[i] = (i % 257 == 256) ? 1u : 0u;
}

// grid (ceil(H / ROWS_PER_WG), N); dynamic LDS: two rows of RBP = 3 W rounded up to 16 bytes
template <bool F32>
__global__ __launch_bounds__(256) void filter_hist_kernel(const void* __restrict__ src, int H, int W, uint8_t* __restrict__ streams,
                                                          uint32_t* __restrict__ hist, uint32_t* __restrict__ adler) {
    extern __shared__ __align__(16) uint8_t rows[];
    __shared__ uint32_t bins[256];
    __shared__ uint32_t red32[5][4];
    __shared__ unsigned long long red64[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = blockIdx.y;
    const int RB = 3 * W, L = RB + 1, RBP = (RB + 15) & ~15;
    const int y0 = blockIdx.x * ROWS_PER_WG, y1 = min(H, y0 + ROWS_PER_WG);
    const size_t plane = (size_t)H * W, img = n * 3 * plane;
    uint8_t* prev = rows;
    uint8_t* cur = rows + RBP;

    auto load_row = [&](int y, uint8_t* dst) {          // planar source row -> RGB-interleaved bytes; the row above row 0 is zero
        if (y < 0) {
            for (int i = tid; i < RB; i += 256) dst[i] = 0;
            return;
        }
        for (int x = tid; x < W; x += 256)
            for (int c = 0; c < 3; ++c) {
                const size_t idx = img + c * plane + (size_t)y * W + x;
                dst[3 * x + c] = F32 ? to_byte(((const float*)src)[idx]) : ((const uint8_t*)src)[idx];
            }
    };

    bins[tid] = 0;
    load_row(y0 - 1, prev);
    for (int y = y0; y < y1; ++y) {
        load_row(y, cur);
        __syncthreads();
        // pass 1: the cost sum(min(v, 256 - v)) of each filter over the row
        uint32_t cost[5] = {0, 0, 0, 0, 0};
        for (int i = tid; i < RB; i += 256) {
            const int x = cur[i], b = prev[i];
            const int a = i >= 3 ? cur[i - 3] : 0, c = i >= 3 ? prev[i - 3] : 0;
            for (int k = 0; k < 5; ++k) cost[k] += cost_of(x, predict(k, a, b, c));
        }
        for (int k = 0; k < 5; ++k) {
            const uint32_t s = wave_sum_u(cost[k]);
            if (lane == 0) red32[k][wave] = s;
        }
        __syncthreads();
        int best = 0;
        uint32_t best_cost = 0;
        for (int k = 0; k < 5; ++k) {                   // lowest cost, ties to the lowest filter number
            const uint32_t s = red32[k][0] + red32[k][1] + red32[k][2] + red32[k][3];
            if (k == 0 || s < best_cost) {
                best = k;
                best_cost = s;
            }
        }
        // pass 2: the winning filter's bytes, their histogram and Adler sums (byte j of the row weighs L - j)
        uint8_t* out = streams + (n * H + y) * (size_t)L;
        unsigned long long s1 = 0, s2 = 0;
        if (tid == 0) {
            out[0] = (uint8_t)best;
            atomicAdd(&bins[best], 1u);
            s1 = (unsigned long long)best;
            s2 = (unsigned long long)best * L;
        }
        for (int base = 0; base < RB; base += 256) {
            const int i = base + tid;
            int v = -1;
            if (i < RB) {
                const int x = cur[i], b = prev[i];
                const int a = i >= 3 ? cur[i - 3] : 0, c = i >= 3 ? prev[i - 3] : 0;
                v = (x - predict(best, a, b, c)) & 255;
                out[1 + i] = (uint8_t)v;
                s1 += (unsigned long long)v;
                s2 += (unsigned long long)v * (unsigned long long)(RB - i);
            }
            // zeros dominate a well-predicted row: one LDS add per wave for them
            const unsigned long long zeros = __ballot(v == 0);
            if (v > 0) atomicAdd(&bins[v], 1u);
            if (lane == 0 && zeros) atomicAdd(&bins[0], (uint32_t)__popcll(zeros));
        }
        s1 = wave_sum_u(s1);
        s2 = wave_sum_u(s2);
        if (lane == 0) {
            red64[0][wave] = s1;
            red64[1][wave] = s2;
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t* ad = adler + (n * H + y) * 2;
            ad[0] = (uint32_t)((red64[0][0] + red64[0][1] + red64[0][2] + red64[0][3]) % ADLER_MOD);
            ad[1] = (uint32_t)((red64[1][0] + red64[1][1] + red64[1][2] + red64[1][3]) % ADLER_MOD);
        }
        uint8_t* t = prev;
        prev = cur;
        cur = t;
    }
    __syncthreads();
    const uint32_t cnt = bins[tid];
    if (cnt) atomicAdd(&hist[n * 257 + tid], cnt);
}

// Symbol s of an image: stream byte s for s < S, the end-of-block symbol 256 for s == S.
// table entry = code (bit-reversed, low 16 bits) | length << 16

// grid (nchunk, N): bits of the chunk's codes
__global__ __launch_bounds__(256) void chunk_bits_kernel(const uint8_t* __restrict__ streams, int64_t S,
                                                         const uint32_t* __restrict__ tables, int nchunk,
                                                         uint32_t* __restrict__ chunk_bits) {
    __shared__ uint32_t len[257];
    __shared__ uint32_t red[4];
    const int tid = threadIdx.x;
    const size_t n = blockIdx.y;
    for (int i = tid; i < 257; i += 256) len[i] = (tables[n * 257 + i] >> 16) & 15u;
    __syncthreads();
    const uint8_t* src = streams + n * (size_t)S;
    const int64_t s0 = (int64_t)blockIdx.x * CHUNK;
    uint32_t bits = 0;
    for (int k = 0; k < RUN; ++k) {
        const int64_t s = s0 + k * 256 + tid;
        if (s <= S) bits += len[s < S ? src[s] : 256];
    }
    bits = wave_sum_u(bits);
    if ((tid & 63) == 0) red[tid >> 6] = bits;
    __syncthreads();
    if (tid == 0) chunk_bits[n * nchunk + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ void or_word(uint32_t* __restrict__ out, uint64_t w, uint64_t out_words, uint32_t v) {
    if (v != 0 && w < out_words) atomicOr(out + w, v);
}

// grid (nchunk, N).  out: 32-bit words, zeroed by the caller.  A word that lies wholly inside one thread's run is stored plainly; a
// word shared with a neighbouring run, the header or the next image is ORed in.
__global__ __launch_bounds__(256) void pack_kernel(const uint8_t* __restrict__ streams, int64_t S, const uint32_t* __restrict__ tables,
                                                   const uint32_t* __restrict__ hdr, const int32_t* __restrict__ hdr_bits,
                                                   const int64_t* __restrict__ offsets, const uint32_t* __restrict__ chunk_bits,
                                                   int nchunk, uint32_t* __restrict__ out, uint64_t out_words) {
    __shared__ uint32_t tab[257];
    __shared__ __align__(16) uint8_t sym[CHUNK];
    __shared__ unsigned long long red[4];
    __shared__ uint32_t wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = blockIdx.y;
    const int c = blockIdx.x;
    for (int i = tid; i < 257; i += 256) tab[i] = tables[n * 257 + i];
    const uint8_t* src = streams + n * (size_t)S;
    const int64_t s0 = (int64_t)c * CHUNK;
    const int nsym = (int)min((int64_t)CHUNK, S + 1 - s0);          // >= 1: the last chunk holds at least the end of block
    for (int k = 0; k < RUN; ++k) {
        const int idx = k * 256 + tid;
        sym[idx] = s0 + idx < S ? src[s0 + idx] : 0;
    }
    // where this chunk starts: the image's offset, its header, the chunks before this one
    unsigned long long pre = 0;
    for (int j = tid; j < c; j += 256) pre += chunk_bits[n * nchunk + j];
    pre = wave_sum_u(pre);
    if (lane == 0) red[wave] = pre;
    __syncthreads();
    const int hb = min(max(hdr_bits[n], 0), 32 * HDR_WORDS);
    const uint64_t img_bit = 8ull * (uint64_t)offsets[n];
    const uint64_t start = img_bit + (uint64_t)hb + red[0] + red[1] + red[2] + red[3];

    if (c == 0 && tid < HDR_WORDS) {                               // the header: byte-aligned, not word-aligned
        const int valid = min(max(hb - 32 * tid, 0), 32);
        if (valid > 0) {
            uint32_t v = hdr[n * HDR_WORDS + tid];
            if (valid < 32) v &= (1u << valid) - 1u;
            const uint64_t p = img_bit + 32ull * tid;
            const int sh = (int)(p & 31);
            or_word(out, p >> 5, out_words, v << sh);
            if (sh) or_word(out, (p >> 5) + 1, out_words, v >> (32 - sh));
        }
    }

    // this thread's run: its bit length, then its start from the block's exclusive scan
    const int r0 = tid * RUN;
    uint32_t mine = 0;
    for (int k = 0; k < RUN; ++k) {
        const int idx = r0 + k;
        if (idx < nsym) mine += (tab[s0 + idx == S ? 256 : sym[idx]] >> 16) & 15u;
    }
    uint32_t inc = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t before = inc - mine;
    for (int w = 0; w < wave; ++w) before += wtot[w];

    const uint64_t p = start + before;
    uint64_t w = p >> 5;
    uint32_t nb = (uint32_t)(p & 31);
    uint64_t acc = 0;
    bool shared_word = nb != 0;                                    // the run's first word also holds the previous run's last bits
    for (int k = 0; k < RUN; ++k) {
        const int idx = r0 + k;
        if (idx >= nsym) break;
        const uint32_t e = tab[s0 + idx == S ? 256 : sym[idx]];
        const uint32_t len = (e >> 16) & 15u;
        acc |= (uint64_t)(e & ((1u << len) - 1u)) << nb;           // nb <= 31, len <= 15
        nb += len;
        if (nb >= 32) {
            if (shared_word) or_word(out, w, out_words, (uint32_t)acc);
            else if (w < out_words) out[w] = (uint32_t)acc;
            shared_word = false;
            acc >>= 32;
            nb -= 32;
            ++w;
        }
    }
    or_word(out, w, out_words, (uint32_t)acc);                     // the run's last, partial word
}

}  // namespace

extern "C" {

int spaa_png_filter_hist(const void* images, int is_f32, int N, int H, int W, uint8_t* streams, uint32_t* hist, uint32_t* adler,
                         spaa_stream_t stream) {
    if (!images || !streams || !hist || !adler || N < 1 || N > 65535 || H < 1 || W < 1 || 3 * (int64_t)W > MAX_ROW_BYTES ||
        H > (1 << 24))
        return hipErrorInvalidValue;
    const int total = N * 257;
    hipLaunchKernelGGL(hist_init_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, hist, total);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const dim3 grid((H + ROWS_PER_WG - 1) / ROWS_PER_WG, N);
    const size_t lds = 2 * (size_t)((3 * W + 15) & ~15);
    if (is_f32)
        hipLaunchKernelGGL(filter_hist_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, images, H, W, streams, hist, adler);
    else
        hipLaunchKernelGGL(filter_hist_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, images, H, W, streams, hist, adler);
    return (int)hipGetLastError();
}

int spaa_png_pack(const uint8_t* streams, int64_t stream_bytes, int N, const uint32_t* tables, const uint32_t* hdr,
                  const int32_t* hdr_bits, const int64_t* offsets, uint32_t* chunk_bits, uint8_t* out, int64_t out_bytes,
                  spaa_stream_t stream) {
    if (!streams || !tables || !hdr || !hdr_bits || !offsets || !chunk_bits || !out || N < 1 || N > 65535 || stream_bytes < 1 ||
        out_bytes < 4 || (out_bytes & 3) || ((uintptr_t)out & 3))
        return hipErrorInvalidValue;
    const int64_t nchunk = stream_bytes / CHUNK + 1;                // symbols 0 .. stream_bytes (the end of block is the last)
    if (nchunk > 0x7fffffff / 65535) return hipErrorInvalidValue;  // (chunk_bits is indexed n * nchunk + c)
    const dim3 grid((unsigned)nchunk, N);
    hipLaunchKernelGGL(chunk_bits_kernel, grid, dim3(256), 0, (hipStream_t)stream, streams, stream_bytes, tables, (int)nchunk,
                       chunk_bits);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pack_kernel, grid, dim3(256), 0, (hipStream_t)stream, streams, stream_bytes, tables, hdr, hdr_bits, offsets,
                       chunk_bits, (int)nchunk, (uint32_t*)out, (uint64_t)(out_bytes / 4));
    return (int)hipGetLastError();
}

}  // extern "C"
