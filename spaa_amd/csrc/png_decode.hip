// png_decode.hip — the device half of the PNG decoder behind io.torch_imread_mt(..., device=) (spaa_amd/png.py holds the host half:
// container parsing, CRCs, the zlib header and trailer):
//   spaa_png_inflate    raw deflate payloads -> PNG scanline streams; ONE WAVE PER IMAGE, the inflate of png_inflate_core.hpp
//   spaa_png_unfilter   scanline streams -> planar bytes [3][H][W] and the per-row Adler-32 partial sums of the scanlines
// Inflate is serial in its symbols, so the parallelism is across images (a batch of files) and, inside an image, in the table
// construction and the match copies.  Each wave is its own workgroup and owns ~38 KiB of LDS (four per CU): a 32 KiB ring of the
// newest output -- every match reads its history there, never from global memory -- a 2 KiB window of the input and the tables.
// The ring is flushed to global memory in 8 KiB pieces of coalesced dwords; each output byte is stored to global memory once and is
// not read again by this kernel.
// Unfilter runs one wave per image as a skewed wavefront: lane r owns row r of a 64-row band and works one pixel behind lane r - 1,
// whose result reaches it through a lane shuffle; the last row of a band waits in LDS for the next band.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "png_inflate_core.hpp"

namespace {

constexpr uint32_t RING = 32768, PIECE = 8192, WINDOW = 2048;
constexpr uint32_t ADLER_MOD = 65521u;
constexpr int MAX_W = 16000;             // unfilter: one packed pixel (4 bytes) per column of the band's last row in LDS

struct WavePolicy {
    const uint8_t* src;                  // the payload (4-byte aligned)
    uint32_t src_len;
    uint8_t* dst;                        // the image's scanline area (16-byte aligned)
    uint8_t* ring;                       // LDS [RING]
    uint8_t* window;                     // LDS [WINDOW]
    uint32_t win_base, win_end;          // the window holds input bytes [win_base, win_end)
    uint32_t flushed;                    // output bytes already in global memory: a multiple of PIECE
    int ln;

    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int lanes() const { return 64; }
    __device__ __forceinline__ void sync() { __syncthreads(); }

    __device__ __forceinline__ uint8_t in(uint32_t pos) {
        if (pos - win_base >= win_end - win_base) {                // (uniform; also true for pos < win_base: unsigned)
            __syncthreads();
            win_base = pos & ~3u;
            const uint32_t n = min(WINDOW, src_len - win_base);
            win_end = win_base + n;
            for (uint32_t i = 4 * ln; i < n; i += 256) {
                if (i + 4 <= n) {
                    *(uint32_t*)(window + i) = *(const uint32_t*)(src + win_base + i);
                } else {
                    for (uint32_t k = i; k < n; ++k) window[k] = src[win_base + k];
                }
            }
            __syncthreads();
        }
        return window[pos - win_base];
    }

    __device__ __forceinline__ uint8_t& hist(uint32_t p) { return ring[p & (RING - 1)]; }

    __device__ __forceinline__ void stored(uint32_t out, uint32_t pos, uint32_t n) {
        __syncthreads();
        for (uint32_t i = ln; i < n; i += 64) ring[(out + i) & (RING - 1)] = src[pos + i];
        __syncthreads();
    }

    // ring bytes [flushed, upto) -> global; flushed is a multiple of 4 and the ring does not wrap inside a dword
    __device__ __forceinline__ void flush(uint32_t upto) {
        __syncthreads();
        const uint32_t n = upto - flushed;
        for (uint32_t i = 4 * ln; i < n; i += 256) {
            const uint32_t p = flushed + i;
            if (i + 4 <= n) {
                *(uint32_t*)(dst + p) = *(const uint32_t*)(ring + (p & (RING - 1)));
            } else {
                for (uint32_t k = p; k < upto; ++k) dst[k] = ring[k & (RING - 1)];
            }
        }
        __syncthreads();
        flushed = upto;
    }

    // at most PIECE - 1 + STORED_PIECE bytes are ever unflushed, so a ring slot is rewritten only after its byte has left
    __device__ __forceinline__ void produced(uint32_t out) {
        if (out - flushed >= PIECE) flush(out & ~(PIECE - 1));
    }
};

// a descriptor's areas lie inside the buffers the caller named, so that a wrong descriptor is a status and not a wild access
__device__ __forceinline__ bool desc_ok(const spaa_png_img_t& d, int64_t payload_bytes, int64_t ws_bytes, int64_t out_bytes,
                                        int64_t adler_rows, int max_w) {
    if (d.H < 1 || d.W < 1 || d.W > max_w || (d.channels != 1 && d.channels != 3 && d.channels != 4)) return false;
    const int64_t row = 1 + (int64_t)d.W * d.channels, stream = row * d.H, plane = (int64_t)d.H * d.W;
    if (stream > 0x7fffffffll || d.src_len < 0 || d.src_len > 0x7fffffffll) return false;
    if (d.src_off < 0 || (d.src_off & 3) || d.src_off + d.src_len > payload_bytes) return false;
    if (d.ws_off < 0 || (d.ws_off & 15) || d.ws_off + stream > ws_bytes) return false;
    if (d.out_off < 0 || d.out_off + 3 * plane > out_bytes) return false;
    if (d.row0 < 0 || d.row0 + d.H > adler_rows) return false;
    return true;
}

// grid N, 64 threads
__global__ __launch_bounds__(64) void inflate_kernel(const uint8_t* __restrict__ payload, int64_t payload_bytes,
                                                     const spaa_png_img_t* __restrict__ imgs, uint8_t* __restrict__ ws, int64_t ws_bytes,
                                                     int32_t* __restrict__ status) {
    __shared__ __align__(16) uint8_t ring[RING];
    __shared__ __align__(16) uint8_t window[WINDOW];
    __shared__ pngi::Tables tables;
    const int n = blockIdx.x;
    const spaa_png_img_t d = imgs[n];
    if (!desc_ok(d, payload_bytes, ws_bytes, INT64_MAX, INT64_MAX, 0x7fffffff)) {
        if (threadIdx.x == 0) status[n] = SPAA_PNG_BAD_DESC;
        return;
    }
    const uint32_t expect = (uint32_t)d.H * (1u + (uint32_t)d.W * d.channels);
    WavePolicy p = {payload + d.src_off, (uint32_t)d.src_len, ws + d.ws_off, ring, window, 0, 0, 0, (int)threadIdx.x};
    uint32_t out_len = 0;
    const int rc = pngi::inflate(p, tables, (uint32_t)d.src_len, expect, out_len);
    if (rc == SPAA_PNG_OK) p.flush(out_len);
    if (threadIdx.x == 0) status[n] = rc;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// grid N, 64 threads; dynamic LDS: 4 max_w bytes.  Pixels travel packed, channel c in byte c of a dword.
__global__ __launch_bounds__(64) void unfilter_kernel(const uint8_t* __restrict__ ws, int64_t ws_bytes,
                                                      const spaa_png_img_t* __restrict__ imgs, int max_w, uint8_t* __restrict__ out,
                                                      int64_t out_bytes, uint32_t* __restrict__ adler, int64_t adler_rows,
                                                      int32_t* __restrict__ status) {
    extern __shared__ uint32_t last_row[];           // the finished last row of the previous band
    const int n = blockIdx.x, lane = threadIdx.x;
    const spaa_png_img_t d = imgs[n];
    if (status[n] != SPAA_PNG_OK) return;            // (inflate stopped this image: its scanlines are not complete)
    if (!desc_ok(d, INT64_MAX, ws_bytes, out_bytes, adler_rows, max_w)) {
        if (lane == 0) status[n] = SPAA_PNG_BAD_DESC;
        return;
    }
    const int H = d.H, W = d.W, ch = d.channels;
    const uint32_t L = 1u + (uint32_t)W * ch;
    const uint8_t* lines = ws + d.ws_off;
    uint8_t* dst = out + d.out_off;
    const size_t plane = (size_t)H * W;
    bool bad = false;
    for (int y0 = 0; y0 < H; y0 += 64) {
        const int y = y0 + lane;
        const bool row_ok = y < H;
        const uint8_t* line = lines + (size_t)(row_ok ? y : 0) * L;
        const int ft = row_ok ? line[0] : 0;
        if (row_ok && ft > 4) bad = true;
        uint64_t s1 = (uint64_t)ft, s2 = (uint64_t)ft * L;
        uint32_t left = 0, up = 0, upleft = 0, mine = 0;
        for (int t = 0; t < W + 63; ++t) {
            const int x = t - lane;
            const bool on = row_ok && x >= 0 && x < W;
            // the pixel above: lane r - 1 finished it in the step before this one; row y0 takes it from the band above
            const uint32_t from_above = __shfl_up(mine, 1, 64);
            if (x >= 0 && x < W) up = lane == 0 ? (y0 > 0 ? last_row[x] : 0u) : from_above;
            if (x == 0) left = upleft = 0;
            if (on) {
                uint32_t px = 0;
                for (int c = 0; c < ch; ++c) {
                    const uint32_t j = 1u + (uint32_t)x * ch + c;
                    const int f = line[j];
                    s1 += (uint64_t)f;
                    s2 += (uint64_t)f * (L - j);
                    const int a = (left >> 8 * c) & 255, b = (up >> 8 * c) & 255, cc = (upleft >> 8 * c) & 255;
                    const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, cc);
                    px |= (uint32_t)((f + pred) & 255) << 8 * c;
                }
                mine = px;
                left = px;
                upleft = up;
                const size_t at = (size_t)y * W + x;
                if (ch == 1) {
                    dst[at] = dst[plane + at] = dst[2 * plane + at] = (uint8_t)px;
                } else {                                           // RGB, or RGBA with the alpha dropped
                    dst[at] = (uint8_t)px;
                    dst[plane + at] = (uint8_t)(px >> 8);
                    dst[2 * plane + at] = (uint8_t)(px >> 16);
                }
                if (lane == 63) last_row[x] = px;                  // (read by lane 0 of the NEXT band only, after the barrier)
            }
        }
        if (row_ok) {
            adler[2 * (d.row0 + (int64_t)y)] = (uint32_t)(s1 % ADLER_MOD);
            adler[2 * (d.row0 + (int64_t)y) + 1] = (uint32_t)(s2 % ADLER_MOD);
        }
        __syncthreads();
    }
    if (__ballot(bad) != 0 && lane == 0) status[n] = SPAA_PNG_BAD_FILTER;
}

}  // namespace

extern "C" {

int spaa_png_inflate(const uint8_t* payload, int64_t payload_bytes, const spaa_png_img_t* imgs, int N, uint8_t* workspace,
                     int64_t workspace_bytes, int32_t* status, spaa_stream_t stream) {
    if (!payload || !imgs || !workspace || !status || N < 1 || N > (1 << 20) || payload_bytes < 0 || workspace_bytes < 1 ||
        ((uintptr_t)payload & 3) || ((uintptr_t)workspace & 15))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(inflate_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, payload, payload_bytes, imgs, workspace,
                       workspace_bytes, status);
    return (int)hipGetLastError();
}

int spaa_png_unfilter(const uint8_t* workspace, int64_t workspace_bytes, const spaa_png_img_t* imgs, int N, int max_w, uint8_t* out,
                      int64_t out_bytes, uint32_t* adler, int64_t adler_rows, int32_t* status, spaa_stream_t stream) {
    if (!workspace || !imgs || !out || !adler || !status || N < 1 || N > (1 << 20) || max_w < 1 || max_w > MAX_W ||
        workspace_bytes < 1 || out_bytes < 1 || adler_rows < 1 || ((uintptr_t)workspace & 15))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(unfilter_kernel, dim3(N), dim3(64), 4 * (size_t)max_w, (hipStream_t)stream, workspace, workspace_bytes, imgs,
                       max_w, out, out_bytes, adler, adler_rows, status);
    return (int)hipGetLastError();
}

}  // extern "C"
