// The hook / jump steps of the connected-components kernels (csrc/mesh_graph.hip, csrc/mesh_quality.hip, csrc/group_stats.hip).  Device
// code only.  parent[] is read and written by other threads during a pass: every read is an agent-scope atomic load.  A stale value is
// still an ancestor (parents only decrease), so a stale read costs at most one more round.
#pragma once
#include <hip/hip_runtime.h>

namespace oai {

__device__ __forceinline__ int load_agent(const int* p) { return __hip_atomic_load(const_cast<int*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a root only ever hooks onto a smaller index, so the components do not depend on the order
__device__ __forceinline__ bool hook(int* parent, int u, int v) {
    const int pu = load_agent(parent + u), pv = load_agent(parent + v);
    if (pu == pv) return false;
    atomicMin(parent + max(pu, pv), min(pu, pv));
    return true;
}

// Roots do not change during a jump pass and every non-root points strictly down, so the walk ends at the root.
__device__ __forceinline__ void jump(int* parent, int i) {
    const int p0 = load_agent(parent + i);
    int p = p0;
    for (;;) {
        const int q = load_agent(parent + p);
        if (q == p) break;
        p = q;
    }
    if (p != p0) __hip_atomic_store(parent + i, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace oai
