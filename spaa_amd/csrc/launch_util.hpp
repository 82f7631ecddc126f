// launch_util.hpp — host-side helpers shared by the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spaa_hip.h"

// Second pass of a K-split layer (tapconv_splitk.hip): adds the `d.ksplit` partial sums of `splitk_ws` [range][M rows][Npad] in fixed
// order and applies the layer's epilogue; fp16 or fp32 output by `io_dtype`, one thread per 4 channels.  `class_map`: row m is pixel m of
// class 0's grid (implicit-GEMM kernels), else output pixel m itself.  Enqueues only: the caller reads hipGetLastError.
void spaa_launch_splitk_reduce(const spaa_tapconv_t& d, int64_t M, bool class_map, hipStream_t stream);

namespace {

constexpr int SPAA_MAX_DEVICES = 32;

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: a process that drives several GPUs
// (one AttackState per device) must set it on each of them, once.  `done` is the calling launcher's own static table.
inline hipError_t ensure_dynamic_lds(const void* kernel, int bytes, bool (&done)[SPAA_MAX_DEVICES]) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= SPAA_MAX_DEVICES) return hipErrorInvalidDevice;
    if (!done[dev]) {
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
        done[dev] = true;
    }
    return hipSuccess;
}

// The multi-bit form flags of a descriptor that launchers read (include/spaa_hip.h: SPAA_DBG_* / SPAA_H16P_*): shifted and masked here, once
// per field.  (Fields a kernel reads have their accessor next to the kernel: wino_pad, thinmf_dbg, x6p_ablate.)
inline int dbg_persist_cap(const spaa_tapconv_t& d) { return (d.reserved0 & SPAA_DBG_PERSIST_CAP) >> SPAA_DBG_PERSIST_CAP_SHIFT; }
inline int dbg_wino_var(const spaa_tapconv_t& d) { return (d.reserved0 & SPAA_DBG_WINO_VAR) >> SPAA_DBG_WINO_VAR_SHIFT; }
inline int dbg_wino_ablate(const spaa_tapconv_t& d) { return (d.reserved0 & SPAA_DBG_WINO_ABLATE) >> SPAA_DBG_WINO_ABLATE_SHIFT; }
inline int h16p_cv_bn(const spaa_tapconv_t& d) { return (d.reserved1 & SPAA_H16P_CV_BN) >> SPAA_H16P_CV_BN_SHIFT; }   // 0 = chosen, 1 = 64, 2 = 128

}  // namespace
