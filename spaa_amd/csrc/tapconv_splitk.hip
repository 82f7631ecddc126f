// tapconv_splitk.hip — the second pass of a K-split layer, shared by the kernels that write raw fp32 partial sums of K ranges to
// `splitk_ws` [range][row][Npad] (tapconv_x6d.hip, tapconv_h16.hip, tapconv_h16p.hip, tapconv_wino.hip):
//   out = epilogue( sum over the ranges, in fixed order ), 4 channels per thread -- bitwise the same from run to run.
// (The forms that combine the ranges inside the kernel -- `splitk_fixup`, stream-K -- are their kernels' own.)
#include <hip/hip_runtime.h>
#include "launch_util.hpp"
#include <stdint.h>
#include "../../include/spaa_hip.h"
#include "device_util.hpp"
#include "epilogue.hpp"

namespace {

// T: storage type of the output.  CLASS_MAP: the workspace rows are the pixels of class 0's grid, mapped to output pixels by `out_pixel`
// (implicit-GEMM kernels); else they are the output pixels themselves (patch-staged kernels: stride 1, same-size grid).
template <typename T, bool CLASS_MAP>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const spaa_tapconv_t p, const int M, const int npad) {
    const int nq = (p.Cout + 3) >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)M * nq) return;
    const int m = (int)(idx / nq), n0 = (int)(idx - (int64_t)m * nq) * 4;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < p.ksplit; ++s) sum += *reinterpret_cast<const f32x4*>(p.splitk_ws + ((size_t)s * M + m) * npad + n0);
    size_t o = (size_t)m;
    if (CLASS_MAP && !out_pixel(p, p.cls[0], m, M, p.Hm * p.Wm, o)) return;
    float v[4] = {sum[0], sum[1], sum[2], sum[3]};
    store4_t<T>(p, o, n0, v, store4_vec_ok(p));
}

template <typename T, bool CLASS_MAP>
void launch(const spaa_tapconv_t& d, int64_t M, hipStream_t stream) {
    const int npad = (d.Cout + 127) & ~127;
    const int64_t nthr = M * ((d.Cout + 3) >> 2);
    hipLaunchKernelGGL((splitk_reduce_kernel<T, CLASS_MAP>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, stream, d, (int)M, npad);
}

}  // namespace

void spaa_launch_splitk_reduce(const spaa_tapconv_t& d, int64_t M, bool class_map, hipStream_t stream) {
    if (d.io_dtype & SPAA_IO_OUT_F16) {
        if (class_map) launch<_Float16, true>(d, M, stream); else launch<_Float16, false>(d, M, stream);
    } else {
        if (class_map) launch<float, true>(d, M, stream); else launch<float, false>(d, M, stream);
    }
}
