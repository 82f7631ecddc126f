// attention_ops.hip — Grad-CAM of the classifier as a weight on the adversarial gradient image.  Per sample b with class
// t = target[b] and seed s = g_logits[b][t]:
//   alpha_k = sign(s) mean_ij G_ijk          G: the gradient at the feature map A [h][w][C] that enters the head's average pool
//   c_ij    = max(0, sum_k alpha_k A_ijk)
//   m       = c / max c   if max c > 0, else 1 everywhere (also when s == 0)
//   M       = m resampled bilinearly (half-pixel centres, edge clamped) onto the ch x cw classifier crop of the camera frame
//   g_y.rgb *= floor + (1 - floor) M         inside the crop; the pad channel and every pixel outside the crop are not written
// Three launches: spaa_cam_alpha (only where G is a map: VGG-16), spaa_cam_map, spaa_attention_apply.  No atomics anywhere and every
// sum in a fixed order: a run is bitwise repeatable.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "device_util.hpp"

namespace {

// alpha[b][k] = (sum_p G[b][p][k]) / HW, positions in index order.  One thread per (b, k): neighbouring threads read neighbouring
// channels.  grid (ceil(C / 256), B)
__global__ __launch_bounds__(256) void cam_alpha_kernel(const float* __restrict__ G, float* __restrict__ alpha, int HW, int C, int cstride) {
    const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= C) return;
    const float* g = G + (size_t)b * HW * cstride + k;
    float a = 0.f;
    for (int p = 0; p < HW; ++p) a += g[(size_t)p * cstride];
    alpha[(size_t)b * C + k] = a / (float)HW;
}

// One workgroup of four waves per sample; wave w owns the positions p = w, w + 4, ...  Per position the 64 lanes walk the C / 4 channel
// quads (float4 loads of A and of alpha), each lane adds its quads in index order, and the lanes' sums meet in the shuffle tree of
// wave_sum.  c[b][p] = max(0, sign(s) alpha_scale dot); cmax[b] = max_p c[b][p].  A sample whose seed is 0 (or whose target is no
// class) has sign 0: c = 0 everywhere and cmax = 0, which spaa_attention_apply reads as "m = 1".
__global__ __launch_bounds__(256) void cam_map_kernel(const float4* __restrict__ A, const float4* __restrict__ alpha, float alpha_scale,
                                                      const float* __restrict__ g_logits, int ncls, const int32_t* __restrict__ target,
                                                      float* __restrict__ c, float* __restrict__ cmax, int HW, int C4) {
    __shared__ float red[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = target[b];
    const float s = ((unsigned)t < (unsigned)ncls) ? g_logits[(size_t)b * ncls + t] : 0.f;
    const float sgn = s > 0.f ? alpha_scale : s < 0.f ? -alpha_scale : 0.f;
    const float4* al = alpha + (size_t)b * C4;
    float mx = 0.f;
    for (int p = wave; p < HW; p += 4) {
        const float4* a = A + ((size_t)b * HW + p) * C4;
        float acc = 0.f;
        for (int q = lane; q < C4; q += 64) {
            const float4 v = a[q], w = al[q];
            acc += v.x * w.x + v.y * w.y + v.z * w.z + v.w * w.w;
        }
        acc = wave_sum(acc);                       // (valid in lane 0)
        if (lane == 0) {
            const float cv = sgn != 0.f ? fmaxf(sgn * acc, 0.f) : 0.f;
            c[(size_t)b * HW + p] = cv;
            mx = fmaxf(mx, cv);
        }
    }
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) cmax[b] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// F.interpolate(mode='bilinear', align_corners=False) along one axis: output index o of `out` onto `in` source cells.  The source
// coordinate ((2 o + 1) in - out) / (2 out), clamped below at 0, in integers: the weight is one correctly rounded division.
__device__ __forceinline__ void bilinear_tap(int o, int out, int in, int& i0, int& i1, float& f) {
    const int n = (2 * o + 1) * in - out;
    if (n <= 0) {
        i0 = 0;
        f = 0.f;
    } else {
        i0 = n / (2 * out);
        f = (float)(n - i0 * 2 * out) / (float)(2 * out);
    }
    if (i0 >= in - 1) {   // past the last centre both taps are the last cell: weight 0, so that the cell comes back exactly
        i0 = in - 1;
        f = 0.f;
    }
    i1 = min(i0 + 1, in - 1);
}

// One thread per camera pixel, one float4 read and one float4 write of g_y inside the crop.  g_y and M_out may each be absent.
// grid (ceil(H W / 256), B)
__global__ __launch_bounds__(256) void attention_apply_kernel(const float* __restrict__ c, const float* __restrict__ cmax, float floor_w,
                                                              float4* __restrict__ g_y, float* __restrict__ M_out, int H, int W, int cy0,
                                                              int cx0, int ch, int cw, int fh, int fw) {
    const int b = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const float mx = cmax[b];
    if (M_out == nullptr && !(mx > 0.f)) return;   // m = 1: the gradient image stays as it is, bit for bit
    const int y = pix / W, x = pix - y * W;
    const int py = y - cy0, px = x - cx0;
    const size_t idx = (size_t)b * H * W + pix;
    if ((unsigned)py >= (unsigned)ch || (unsigned)px >= (unsigned)cw) {
        if (M_out != nullptr) M_out[idx] = 0.f;
        return;
    }
    float M = 1.f;
    if (mx > 0.f) {
        int y0, y1, x0, x1;
        float fy, fx;
        bilinear_tap(py, ch, fh, y0, y1, fy);
        bilinear_tap(px, cw, fw, x0, x1, fx);
        const float* cb = c + (size_t)b * fh * fw;
        const float top = (1.f - fx) * cb[y0 * fw + x0] + fx * cb[y0 * fw + x1];
        const float bot = (1.f - fx) * cb[y1 * fw + x0] + fx * cb[y1 * fw + x1];
        M = fminf(((1.f - fy) * top + fy * bot) / mx, 1.f);
    }
    if (M_out != nullptr) M_out[idx] = M;
    if (g_y != nullptr && mx > 0.f) {
        const float wgt = floor_w + (1.f - floor_w) * M;
        float4 v = g_y[idx];
        v.x *= wgt;
        v.y *= wgt;
        v.z *= wgt;
        g_y[idx] = v;
    }
}

}  // namespace

extern "C" {

int spaa_cam_alpha(const float* G, float* alpha, int B, int HW, int C, int cstride, spaa_stream_t stream) {
    if (!G || !alpha || B < 1 || B > 65535 || HW < 1 || C < 1 || cstride < C) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cam_alpha_kernel, dim3((C + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, G, alpha, HW, C, cstride);
    return (int)hipGetLastError();
}

int spaa_cam_map(const float* A, const float* alpha, float alpha_scale, const float* g_logits, int ncls, const int32_t* target, float* c,
                 float* cmax, int B, int HW, int C, spaa_stream_t stream) {
    if (!A || !alpha || !g_logits || !target || !c || !cmax || B < 1 || HW < 1 || HW > (1 << 20) || C < 4 || C % 4 != 0 || ncls < 1 ||
        !(alpha_scale > 0.f))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(cam_map_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const float4*)A, (const float4*)alpha, alpha_scale,
                       g_logits, ncls, target, c, cmax, HW, C / 4);
    return (int)hipGetLastError();
}

int spaa_attention_apply(const float* c, const float* cmax, float floor_w, float* g_y, float* M_out, int B, int H, int W, int cy0,
                         int cx0, int ch, int cw, int fh, int fw, spaa_stream_t stream) {
    if (!c || !cmax || (!g_y && !M_out) || B < 1 || B > 65535 || H < 1 || W < 1 || (int64_t)H * W > (1 << 30) || ch < 1 || cw < 1 ||
        cy0 < 0 || cx0 < 0 || cy0 + ch > H || cx0 + cw > W || fh < 1 || fw < 1 || fh > 16384 || fw > 16384 || ch > 16384 || cw > 16384 ||   // ((2 o + 1) in stays an int)
        !(floor_w >= 0.f && floor_w <= 1.f))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(attention_apply_kernel, dim3((H * W + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, c, cmax, floor_w,
                       (float4*)g_y, M_out, H, W, cy0, cx0, ch, cw, fh, fw);
    return (int)hipGetLastError();
}

}  // extern "C"
