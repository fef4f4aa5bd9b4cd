// The CSR vertex adjacency as the graph kernels read it (include/oai_hip.h, oai_graph_clusters: "an offset outside [0, n_neighbours] is
// clamped, a neighbour outside [0, n_verts) is ignored"), stated once for csrc/hook_jump.h (oai_graph_clusters, oai_graph_tfce) and
// csrc/graph_smooth.hip.  No graph that a caller hands in makes a kernel read outside offsets[0 .. n_verts], neighbours[0 .. n_neighbours)
// or a row of the tile.
#pragma once
#include <hip/hip_runtime.h>

namespace oai {

struct CsrSlots {
    long long a, b;                                // the slots [a, b) of neighbours[]; empty when b <= a
};

__device__ __forceinline__ CsrSlots csr_slots(const int* __restrict__ offsets, long long i, long long n_nbrs) {
    long long a = offsets[i], b = offsets[i + 1];
    a = a < 0 ? 0 : a;
    b = b > n_nbrs ? n_nbrs : b;
    return {a, b};
}

// What the component kernels walk: a neighbour in [0, n_verts) other than the vertex itself -- a vertex listed among its own neighbours
// joins nothing.  The sweep of graph_smooth.hip shares csr_slots only: there a vertex among its own neighbours is a neighbour like any
// other, and the range test is part of a select (no branch), so it stays written out in that loop.
__device__ __forceinline__ bool csr_neighbour(int u, int i, int n_verts) { return !(u < 0 || u >= n_verts || u == i); }

}  // namespace oai
