// ptr_table.hpp — the per-member / per-view / per-draw tensors of the ensemble, multi-view, jitter and pose entry points (one copy for
// group_ops.hip, jitter_ops.hip, pose_ops.hip).  They arrive as HOST arrays of n device pointers; the launchers
// copy them into a kernel argument passed by value, so there is no device pointer table and a captured graph holds no copy.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/spaa_hip.h"

namespace {

template <typename T, int N = 4>
struct PtrTable {
    T* p[N];
};

static_assert(SPAA_ENS_MAX == 4 && SPAA_VIEWS_MAX == 4 && SPAA_JITTER_MAX == 4, "ptr_of selects among four entries");

// entry i's pointer (i is uniform per workgroup; selects, so that the argument struct stays in the kernel-argument segment)
template <typename T>
__device__ __forceinline__ T* ptr_of(const PtrTable<T, 4>& t, int i) {
    return i == 0 ? t.p[0] : i == 1 ? t.p[1] : i == 2 ? t.p[2] : t.p[3];
}

// the n host pointers into the kernel argument: n in 2..N, entries from `first` on must be set, those beyond n are null
template <typename T, int N>
bool gather(PtrTable<T, N>& t, T* const* host, int n, int first = 0) {
    if (!host || n < 2 || n > N) return false;
    for (int i = 0; i < N; ++i) {
        t.p[i] = (i >= first && i < n) ? host[i] : nullptr;
        if (i >= first && i < n && !host[i]) return false;
    }
    return true;
}

}  // namespace
