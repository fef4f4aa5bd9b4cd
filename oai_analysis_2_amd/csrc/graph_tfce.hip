// Threshold-free cluster enhancement for gfx950 (include/oai_hip.h, "Threshold-free cluster enhancement"; tests/graph_tfce_ref.py restates
// the definition by brute force): per row of a float64 tile and per vertex, the sum over the levels h_k = k * dh at or below |t| of
// extent^E * h_k^H * dh, where the extent is the weight of the vertex' connected component of {|t| >= h_k, same sign} on the surface graph.
//   oai_graph_tfce     one workgroup per row; the tile in, the TFCE tile and each row's count of clipped vertices out
//
// fp64 without contraction.  The order IS the contract: a vertex' sum runs from its highest level K(v) down to 1 with one accumulator.
// Component weights are 64-bit integer sums (atomics: an integer sum has no order); there are no floating-point atomics.
//
// Shape, and why.  Components only grow as the threshold falls, so ONE union-find per row is carried through all levels, top level first:
// at level k the vertices with K(v) = k activate (parent[i] = i) and only THEY hook, since every edge the level adds has a new vertex at
// one end; every active vertex then jumps to its root, and rounds repeat until one hooks nothing (csrc/hook_jump.h: a root only ever
// hooks onto a smaller index, so a vertex that activates below an existing root takes the component over through the ordinary atomicMin).
// The weights are then recounted at the roots and every active vertex adds its term.  A level at which nothing activates has the same
// components as the level above: the walk goes straight to the next level that some vertex has (their maximum is found during the
// activation pass), and the add pass runs the skipped levels' terms in a register, in descending order, with the same weight -- so a
// row with an infinity in it and max_steps = 65536 costs one pass, not 65536.
//   Workgroup = 1024 threads (the maximum; one row has V / 1024 vertices per thread and every pass ends in a barrier, so the passes
//     are latency-bound and the widest workgroup is the shortest); rows are independent and fill the CUs.
//   The workspace holds parent (int), the signed level side * K(v) (int) and the component weight (int64) per (row, vertex): n_verts is
//     not bounded by LDS.  The accumulator is the output row itself, touched by its owning thread only.
//   parent[] and weight[] are read by other threads between barriers: agent-scope relaxed atomics, as in oai_graph_clusters.  level[]
//     is written once before the first barrier and only read afterwards.
// Measured (profiles/group_tfce.md).
#include "cohort.h"

#include <cmath>

#include "hook_jump.h"

#pragma clang fp contract(off)

namespace {

using namespace oai;

constexpr int kTfceT = 1024;                       // the workgroup of one row
constexpr int kMaxSteps = 1 << 16;

struct TfceWs {
    int *parent, *level;
    unsigned long long* weight;
    size_t bytes;
    TfceWs(const void* base, long long rows, long long V) {
        Ws ws(base);
        parent = ws.take<int>((size_t)(rows * V));
        level = ws.take<int>((size_t)(rows * V));
        weight = ws.take<unsigned long long>((size_t)(rows * V));
        bytes = ws.off;
    }
};

// K(v): the largest k in 1 .. max_steps with (double)k * dh <= a, 0 if there is none (a NaN included).  The quotient only says where to
// look; the answer is decided by the stated products, which do not decrease with k.
__device__ __forceinline__ int top_level(double a, double dh, int max_steps) {
    if (!(a >= dh)) return 0;
    const double q = a / dh;
    int k = q >= (double)max_steps ? max_steps : (int)q;
    k = k < 1 ? 1 : k;
    while (k < max_steps && (double)(k + 1) * dh <= a) ++k;
    while (k > 1 && (double)k * dh > a) --k;
    return k;
}

__device__ __forceinline__ unsigned long long load_agent64(const unsigned long long* p) {
    return __hip_atomic_load(const_cast<unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kTfceT) graph_tfce_kernel(const double* __restrict__ values, long long V, const int* __restrict__ offsets,
                                                            const int* __restrict__ neighbours, long long n_nbrs,
                                                            const long long* __restrict__ weight_in, double unit, double dh, int e_mode, int h_mode,
                                                            int max_steps, int* parent_all, int* level_all, unsigned long long* weight_all,
                                                            double* tfce_all, int* __restrict__ clipped) {
    __shared__ int top, next, n_clipped;
    const double* val = values + (long long)blockIdx.x * V;
    int* parent = parent_all + (long long)blockIdx.x * V;
    int* level = level_all + (long long)blockIdx.x * V;
    unsigned long long* weight = weight_all + (long long)blockIdx.x * V;
    double* acc = tfce_all + (long long)blockIdx.x * V;
    const int n = (int)V;
    if (threadIdx.x == 0) { top = 0; n_clipped = 0; }
    __syncthreads();
    {
        const double h_clip = (double)(max_steps + 1) * dh;
        int my_top = 0, my_clipped = 0;
        for (int i = threadIdx.x; i < n; i += kTfceT) {
            const double t = val[i], a = fabs(t);
            const int kv = top_level(a, dh, max_steps);                    // 0 for +-0 and NaN: side 0 is never active
            level[i] = t < 0.0 ? -kv : kv;
            __hip_atomic_store(parent + i, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            acc[i] = 0.0;
            my_top = kv > my_top ? kv : my_top;
            my_clipped += a >= h_clip ? 1 : 0;
        }
        if (my_top) atomicMax(&top, my_top);
        if (my_clipped) atomicAdd(&n_clipped, my_clipped);
    }
    __syncthreads();
    int k = top;
    if (threadIdx.x == 0) clipped[blockIdx.x] = n_clipped;
    while (k >= 1) {                                                       // k is the same in every thread: it comes from LDS
        __syncthreads();                                                   // everybody has read `next` of the level before
        if (threadIdx.x == 0) next = 0;
        __syncthreads();
        int my_next = 0;
        for (int i = threadIdx.x; i < n; i += kTfceT) {
            const int l = level[i], al = l < 0 ? -l : l;
            if (al == k) __hip_atomic_store(parent + i, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (al >= k) __hip_atomic_store(weight + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (al < k) my_next = al > my_next ? al : my_next;
        }
        if (my_next) atomicMax(&next, my_next);
        __syncthreads();
        // only the vertices of this level hook, since every edge the level adds has a new vertex at one end; a neighbour counts when it is
        // active at this level and of the same side
        hook_jump_rounds<kTfceT>(
            parent, V, offsets, neighbours, n_nbrs,
            [&](int i) { const int l = level[i]; return l == k || l == -k ? l : 0; },
            [&](int l, int u) { const int lu = level[u]; return l > 0 ? lu >= k : lu <= -k; });
        for (int i = threadIdx.x; i < n; i += kTfceT) {
            const int l = level[i];
            if (l >= k || l <= -k) atomicAdd(weight + load_agent(parent + i), weight_in ? (unsigned long long)weight_in[i] : 1ull);
        }
        __syncthreads();
        const int nx = next;
        for (int i = threadIdx.x; i < n; i += kTfceT) {
            const int l = level[i];
            if (!(l >= k || l <= -k)) continue;
            const double e = (double)(long long)load_agent64(weight + load_agent(parent + i)) * unit;
            const double eE = e_mode == OAI_TFCE_E_HALF ? sqrt(e) : e;
            double s = acc[i];
            for (int j = k; j > nx; --j) {                                 // levels k-1 .. nx+1 activate nothing: the same components
                const double h = (double)j * dh;
                const double hH = h_mode == OAI_TFCE_H_TWO ? h * h : h;
                s = s + (eE * hH) * dh;
            }
            acc[i] = s;
        }
        k = nx;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kTfceT) {
        const double t = val[i], s = acc[i];
        acc[i] = t != t ? (double)NAN : (t < 0.0 ? -s : s);
    }
}

}  // namespace

extern "C" {

size_t oai_graph_tfce_workspace_bytes(long long n_rows, long long n_verts) {
    if (!tile_shape_ok(n_rows, n_verts)) return 0;
    return TfceWs(nullptr, n_rows, n_verts).bytes;
}

int oai_graph_tfce(const double* values_dev, long long n_rows, long long n_verts, const int* offsets_dev, const int* neighbours_dev,
                   long long n_neighbours, const long long* weight_dev, double unit, double dh, int e_mode, int h_mode, int max_steps,
                   void* workspace_dev, size_t workspace_bytes, double* tfce_dev, int* clipped_dev, void* stream) {
    OAI_CHECK_GRAPH_TILE("oai_graph_tfce", n_rows, n_verts, n_neighbours);
    OAI_CHECK_ARG(dh > 0.0 && dh < (double)INFINITY, "oai_graph_tfce: the step dh must be finite and > 0 (got %g)", dh);
    OAI_CHECK_ARG(unit > 0.0, "oai_graph_tfce: the unit of extent must be > 0 (got %g)", unit);
    OAI_CHECK_ARG(e_mode == OAI_TFCE_E_HALF || e_mode == OAI_TFCE_E_ONE, "oai_graph_tfce: e_mode must be 0 (E = 1/2) or 1 (E = 1), got %d", e_mode);
    OAI_CHECK_ARG(h_mode == OAI_TFCE_H_ONE || h_mode == OAI_TFCE_H_TWO, "oai_graph_tfce: h_mode must be 0 (H = 1) or 1 (H = 2), got %d", h_mode);
    OAI_CHECK_ARG(max_steps >= 1 && max_steps <= kMaxSteps, "oai_graph_tfce: max_steps must be 1 .. 65536, got %d", max_steps);
    OAI_CHECK_ARG(workspace_dev && tfce_dev && clipped_dev && values_dev && offsets_dev && (n_neighbours == 0 || neighbours_dev),
                  "oai_graph_tfce: null pointer");
    OAI_CHECK_WORKSPACE("oai_graph_tfce", workspace_bytes, oai_graph_tfce_workspace_bytes(n_rows, n_verts));
    const TfceWs ws(workspace_dev, n_rows, n_verts);
    graph_tfce_kernel<<<(unsigned)n_rows, kTfceT, 0, (hipStream_t)stream>>>(values_dev, n_verts, offsets_dev, neighbours_dev, n_neighbours, weight_dev,
                                                                           unit, dh, e_mode, h_mode, max_steps, ws.parent, ws.level, ws.weight,
                                                                           tfce_dev, clipped_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
