// direct_mask.hip — the projector's direct-light mask of a camera view (load_data of the reference's train_network.py:68-80 and
// threshold_im of its img_proc.py:13-65, compensation=False), in three stages:
//   spaa_cb_direct_gray   Nayar's separation of the shifted-checkerboard captures (max / min over the captures), clip, grey byte image
//   spaa_mask_blur_hist   3 x 3 Gaussian (sigma 1.5) of the byte image in integer arithmetic + its 256-bin histogram
//   spaa_otsu_mask_bbox   two-class Otsu threshold from the histogram, the mask, its bounding box and pixel count
// Every result is integer or a fixed sequence of correctly rounded fp32 operations (no contraction, no reassociation), so a numpy
// restatement (tests/direct_mask_oracle.py) reproduces it bit for bit whatever the launch order.  One pass over a camera image:
// bandwidth-trivial, written plainly (one thread per pixel, coalesced along x, 256-thread workgroups, LDS bins / LDS box).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "../../include/spaa_hip.h"

// Every product below is rounded on its own: no contraction into FMAs in this file.  (The __fmul_rn / __fadd_rn intrinsics are
// header inlines compiled with the default contraction and DO fuse after inlining; plain operators under this pragma do not.
// IEEE division is the default for / in HIP device code: v_div_scale / v_div_fmas / v_div_fixup, correctly rounded.)
#pragma clang fp contract(off)

namespace {

// cb [N][3][npix]; N == 1: cb is the direct image itself.  den1 = (float)(1 - b), den2 = (float)(1 - b b), bf = (float)b.
__global__ __launch_bounds__(256) void cb_direct_gray_kernel(const float* __restrict__ cb, int N, int npix, float bf, float den1,
                                                             float den2, uint8_t* __restrict__ gray, float* __restrict__ direct,
                                                             float* __restrict__ indirect) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    float d[3];
    for (int c = 0; c < 3; ++c) {
        const float* p = cb + (size_t)c * npix + i;
        float l1 = p[0], l2 = l1;
        for (int n = 1; n < N; ++n) {
            const float v = p[(size_t)n * 3 * npix];
            l1 = fmaxf(l1, v);
            l2 = fminf(l2, v);
        }
        float dc = l1;
        if (N > 1) {
            dc = (l1 - l2) / den1;
            if (indirect != nullptr)
                indirect[(size_t)c * npix + i] = (2.f * (l2 - bf * l1)) / den2;
        }
        if (direct != nullptr) direct[(size_t)c * npix + i] = dc;      // (before the clip, as load_data's im_direct)
        d[c] = fminf(fmaxf(dc, 0.f), 1.f);
    }
    const float g = (0.299f * d[0] + 0.587f * d[1]) + 0.114f * d[2];
    const int q = (int)(g * 255.f);                            // truncation; g <= 1 + 2 ulp, so q <= 255
    gray[i] = (uint8_t)(q > 255 ? 255 : q);
}

// BORDER_REFLECT_101: -1 -> 1, n -> n - 2 (n >= 2)
__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__global__ __launch_bounds__(256) void blur_hist_kernel(const uint8_t* __restrict__ gray, int H, int W, uint8_t* __restrict__ smooth,
                                                        uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[256];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < H * W) {
        const int y = i / W, x = i - y * W;
        const int xl = reflect101(x - 1, W), xr = reflect101(x + 1, W);
        int hrow[3];
        for (int k = 0; k < 3; ++k) {
            const uint8_t* r = gray + (size_t)reflect101(y - 1 + k, H) * W;
            hrow[k] = 79 * (int)r[xl] + 98 * (int)r[x] + 79 * (int)r[xr];
        }
        const int v = 79 * hrow[0] + 98 * hrow[1] + 79 * hrow[2];       // <= 256 * 256 * 255
        const int s = (v + 32768) >> 16;
        smooth[i] = (uint8_t)s;
        atomicAdd(&bins[s], 1u);
    }
    __syncthreads();
    const uint32_t c = bins[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
}

// One thread: the histogram is 256 bins.  out = {t, xmin, ymin, xmax, ymax, count}, the box initialised for the atomics that follow.
__global__ void otsu_kernel(const uint32_t* __restrict__ hist, int32_t* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int vmin = -1, vmax = -1;
    unsigned long long total = 0, wsum = 0;
    for (int v = 0; v < 256; ++v) {
        const unsigned long long c = hist[v];
        if (c) {
            if (vmin < 0) vmin = v;
            vmax = v;
        }
        total += c;
        wsum += c * (unsigned long long)v;
    }
    int t = -1;
    if (vmin >= 0 && vmax > vmin) {
        unsigned long long w0 = 0, s0 = 0;
        double best = -1.0;
        int kbest = vmin;
        for (int k = vmin; k < vmax; ++k) {
            const unsigned long long c = hist[k];
            w0 += c;
            s0 += c * (unsigned long long)k;
            const unsigned long long w1 = total - w0, s1 = wsum - s0;   // both classes hold pixels: hist[vmin], hist[vmax] > 0
            const double dm = (double)s0 / (double)w0 - (double)s1 / (double)w1;
            const double var = (((double)w0 * (double)w1) * dm) * dm;
            if (var > best) {
                best = var;
                kbest = k;
            }
        }
        t = kbest + 1;
        while (hist[t] == 0) ++t;                                        // first value of the upper class (t <= vmax)
    }
    out[0] = t;
    out[1] = INT_MAX;
    out[2] = INT_MAX;
    out[3] = -1;
    out[4] = -1;
    out[5] = 0;
}

__global__ __launch_bounds__(256) void mask_bbox_kernel(const uint8_t* __restrict__ smooth, int H, int W, uint8_t* __restrict__ mask,
                                                        int32_t* __restrict__ out) {
    __shared__ int box[5];
    if (threadIdx.x == 0) {
        box[0] = box[1] = INT_MAX;
        box[2] = box[3] = -1;
        box[4] = 0;
    }
    __syncthreads();
    const int t = out[0];                                                // (written by otsu_kernel, earlier on the stream; never rewritten)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < H * W) {
        const bool fg = t >= 0 && (int)smooth[i] >= t;
        mask[i] = fg ? 1 : 0;
        if (fg) {
            const int y = i / W, x = i - y * W;
            atomicMin(&box[0], x);
            atomicMin(&box[1], y);
            atomicMax(&box[2], x);
            atomicMax(&box[3], y);
            atomicAdd(&box[4], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && box[4] > 0) {
        atomicMin(&out[1], box[0]);
        atomicMin(&out[2], box[1]);
        atomicMax(&out[3], box[2]);
        atomicMax(&out[4], box[3]);
        atomicAdd(&out[5], box[4]);
    }
}

inline bool bad_size(int H, int W) { return H < 2 || W < 2 || (int64_t)H * W > (int64_t)INT_MAX - 256; }

}  // namespace

extern "C" {

int spaa_cb_direct_gray(const float* cb, int N, int H, int W, double b, uint8_t* gray_u8, float* direct, float* indirect,
                        spaa_stream_t stream) {
    if (!cb || !gray_u8 || N < 1 || bad_size(H, W) || !(b >= 0.0 && b < 1.0)) return hipErrorInvalidValue;
    const int npix = H * W;
    hipLaunchKernelGGL(cb_direct_gray_kernel, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, cb, N, npix, (float)b,
                       (float)(1.0 - b), (float)(1.0 - b * b), gray_u8, direct, N > 1 ? indirect : nullptr);
    return (int)hipGetLastError();
}

int spaa_mask_blur_hist(const uint8_t* gray_u8, int H, int W, uint8_t* smooth_u8, uint32_t* hist, spaa_stream_t stream) {
    if (!gray_u8 || !smooth_u8 || !hist || gray_u8 == smooth_u8 || bad_size(H, W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blur_hist_kernel, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, gray_u8, H, W, smooth_u8, hist);
    return (int)hipGetLastError();
}

int spaa_otsu_mask_bbox(const uint8_t* smooth_u8, const uint32_t* hist, int H, int W, uint8_t* mask, int32_t* out6,
                        spaa_stream_t stream) {
    if (!smooth_u8 || !hist || !mask || !out6 || bad_size(H, W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(otsu_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hist, out6);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mask_bbox_kernel, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, smooth_u8, H, W, mask, out6);
    return (int)hipGetLastError();
}

}  // extern "C"
