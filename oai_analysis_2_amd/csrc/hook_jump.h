// The hook / jump steps of the connected-components kernels (csrc/mesh_graph.hip and csrc/mesh_quality.hip, whose rounds run over edge
// lists and are their own), and the whole round loop of the two that walk the CSR vertex graph with one workgroup per row
// (graph_clusters_kernel of csrc/group_stats.hip, graph_tfce_kernel of csrc/graph_tfce.hip).  Device code only.  parent[] is read and
// written by other threads during a pass: every read is an agent-scope atomic load.  A stale value is still an ancestor (parents only
// decrease), so a stale read costs at most one more round.
#pragma once
#include <hip/hip_runtime.h>

#include "csr_graph.h"

namespace oai {

__device__ __forceinline__ int load_agent(const int* p) { return __hip_atomic_load(const_cast<int*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a root only ever hooks onto a smaller index, so the components do not depend on the order
__device__ __forceinline__ bool hook(int* parent, int u, int v) {
    const int pu = load_agent(parent + u), pv = load_agent(parent + v);
    if (pu == pv) return false;
    atomicMin(parent + max(pu, pv), min(pu, pv));
    return true;
}

// Roots do not change during a jump pass and every non-root points strictly down, so the walk ends at the root.  p0: parent[i] as the
// caller has just loaded it.
__device__ __forceinline__ void jump_from(int* parent, int i, int p0) {
    int p = p0;
    for (;;) {
        const int q = load_agent(parent + p);
        if (q == p) break;
        p = q;
    }
    if (p != p0) __hip_atomic_store(parent + i, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void jump(int* parent, int i) { jump_from(parent, i, load_agent(parent + i)); }

// One workgroup of T threads, all of which call this together, on the V vertices of one row: rounds of hook then jump with a barrier
// between, until a round hooks nothing (every round that hooks removes a root: at most V + 1 rounds), as topo_loops_kernel
// (csrc/mesh_quality.hip) does over edges.  A vertex is active iff it has a parent (parent[i] >= 0); every active vertex jumps.
//   set_of(i)    the non-zero set in which vertex i hooks to its neighbours this round, or 0: it does not hook
//   same(s, u)   whether neighbour u is active and of set s
template <int T, class SetOf, class Same>
__device__ __forceinline__ void hook_jump_rounds(int* parent, long long V, const int* __restrict__ offsets, const int* __restrict__ neighbours,
                                                 long long n_nbrs, SetOf set_of, Same same) {
    __shared__ int changed;
    const int n = (int)V;
    for (long long it = 0; it <= V + 1; ++it) {
        if (threadIdx.x == 0) changed = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += T) {
            const int s = set_of(i);
            if (s == 0) continue;
            const CsrSlots slots = csr_slots(offsets, i, n_nbrs);
            bool ch = false;
            for (long long k = slots.a; k < slots.b; ++k) {
                const int u = neighbours[k];
                if (csr_neighbour(u, i, n) && same(s, u)) ch = hook(parent, i, u) || ch;
            }
            if (ch) changed = 1;
        }
        __syncthreads();
        const int c = changed;
        for (int i = threadIdx.x; i < n; i += T) {
            const int p0 = load_agent(parent + i);
            if (p0 >= 0) jump_from(parent, i, p0);
        }
        __syncthreads();
        if (!c) break;
    }
}

}  // namespace oai
