// Mesh graph steps of the thickness chain for gfx950: the host graph code of mesh_processing.get_mesh on the device, so that
// probability map -> marching cubes -> large regions -> edge graph -> smoothing -> split -> distance stays resident.
//
//   oai_mesh_components          connected components of the face graph (vertices joined when they share a face).  Label = the
//                                smallest vertex index of the component; an unreferenced vertex is its own component.  Hook / jump
//                                rounds, one launch each: a hook pass atomicMin's the larger of an edge's two roots onto the smaller,
//                                a jump pass points every vertex at its root.  A root only ever hooks to a smaller index, so the
//                                labels do not depend on the order the atomics land in.
//   oai_mesh_keep_large_regions  keep_large_regions (mesh_processing.py:120): faces of components with > min_cells faces in their
//                                original order, the vertices they use in ascending original index, remapped.
//   oai_mesh_adjacency           vertex_adjacency (mesh_processing.py:108): the CSR edge graph, neighbours ascending and unique,
//                                self-loops of degenerate faces kept.  Degree count, scatter through atomic cursors (order not fixed),
//                                then each vertex's list sorted and deduplicated (fixed again), scanned and compacted.
//   oai_mesh_grid_params         what point_distance's uniform-grid broad phase derives from the mesh: the float32 bounding box and
//                                the largest squared edge length in fp64, numpy's norm order (dx*dx + dy*dy) + dz*dz.
// Everything is integer work or exact min / max, so the results are the same bits as the host code's on every run.
#include "common.h"
#include "hook_jump.h"

#include <algorithm>
#include <climits>

namespace {

constexpr int kT = 256;
using oai::kMaxFaces;
using oai::face_ok;
using oai::hook;
using oai::load_agent;
constexpr int kBatch = 4;                      // hook / jump rounds launched between two reads of the "changed" flags
constexpr int kRedBlocks = 512;                // blocks of the grid-parameter reductions

// ---------------------------------------------------------------------------------------------------------------------
// connected components
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT) iota_kernel(int* __restrict__ parent, long long n) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i < n) parent[i] = (int)i;
}

__global__ void __launch_bounds__(kT) hook_kernel(const int* __restrict__ faces, long long n_faces, long long n_verts, int* parent,
                                                  int* __restrict__ changed, int* __restrict__ bad_index) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    bool ch = false;
    if (i < n_faces) {
        const int* f = faces + 3 * i;
        if (!face_ok(f, n_verts)) {
            atomicOr(bad_index, 1);
        } else {
            ch = hook(parent, f[0], f[1]);             // the host's edges f0-f1 and f1-f2
            ch = hook(parent, f[1], f[2]) || ch;
        }
    }
    if (__ballot(ch) && (threadIdx.x & 63) == 0) *changed = 1;     // one store per wave
}

// Roots do not change during this pass and every non-root points strictly down, so the walk ends at the root.
__global__ void __launch_bounds__(kT) jump_kernel(int* parent, long long n) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int p0 = load_agent(parent + i);
    int p = p0;
    for (;;) {
        const int q = load_agent(parent + p);
        if (q == p) break;
        p = q;
    }
    if (p != p0) __hip_atomic_store(parent + i, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Workspaces: one struct of typed pointers per entry-point family, filled by one carve() that returns the bytes walked (oai::Ws,
// common.h): over a null base that is the *_workspace_bytes answer, over the caller's buffer the carving.
struct CompWs { int *changed, *bad; };
size_t carve(CompWs& w, const void* base) {
    oai::Ws ws(base);
    w.changed = ws.take<int>(kBatch);
    w.bad = ws.take<int>(1);
    return ws.off;
}

// labels into label_dev (n_verts); reads the flags after every kBatch rounds (synchronises the stream)
int components(const int* faces, long long n_faces, long long n_verts, const CompWs& w, int* label, int* rounds_out, hipStream_t st, const char* who) {
    int *changed = w.changed, *bad = w.bad;
    iota_kernel<<<oai::cdiv(n_verts, kT), kT, 0, st>>>(label, n_verts);
    OAI_CHECK_LAUNCH();
    int rounds = 0;
    if (n_faces > 0) {
        OAI_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
        for (;;) {
            OAI_CHECK_HIP(hipMemsetAsync(changed, 0, kBatch * sizeof(int), st));
            for (int r = 0; r < kBatch; ++r) {
                hook_kernel<<<oai::cdiv(n_faces, kT), kT, 0, st>>>(faces, n_faces, n_verts, label, changed + r, bad);
                OAI_CHECK_LAUNCH();
                jump_kernel<<<oai::cdiv(n_verts, kT), kT, 0, st>>>(label, n_verts);
                OAI_CHECK_LAUNCH();
            }
            int h[kBatch + 1];
            OAI_CHECK_HIP(hipMemcpyAsync(h, changed, kBatch * sizeof(int), hipMemcpyDeviceToHost, st));
            OAI_CHECK_HIP(hipMemcpyAsync(h + kBatch, bad, sizeof(int), hipMemcpyDeviceToHost, st));
            OAI_CHECK_HIP(hipStreamSynchronize(st));
            if (h[kBatch]) return oai::set_error(OAI_ERR_ARG, "%s: a face indexes outside the %lld vertices", who, n_verts);
            int r = 0;
            while (r < kBatch && h[r]) ++r;
            if (r < kBatch) { rounds += r + 1; break; }                // round r changed nothing: converged
            rounds += kBatch;
            // every round that changes something removes at least one root
            if (rounds > n_verts + kBatch) return oai::set_error(OAI_ERR_HIP, "%s: no convergence after %d rounds", who, rounds);
        }
    }
    if (rounds_out) *rounds_out = rounds;
    return OAI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// large-region filter
// ---------------------------------------------------------------------------------------------------------------------
// cells[label of face f] += 1, one atomic per (wave, label): the lanes of a wave that share the first pending lane's label add at once
__global__ void __launch_bounds__(kT) region_cells_kernel(const int* __restrict__ faces, long long n_faces, const int* __restrict__ label,
                                                          int* __restrict__ cells) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool pending = i < n_faces;
    const int lab = pending ? label[faces[3 * i]] : -1;
    unsigned long long live = __ballot(pending);
    while (live) {
        const int lead = __shfl(lab, __ffsll((long long)live) - 1, 64);
        const unsigned long long same = __ballot(pending && lab == lead);
        if (pending && lab == lead) {
            if (lane == __ffsll((long long)same) - 1) atomicAdd(cells + lead, __popcll(same));
            pending = false;
        }
        live &= ~same;
    }
}

// keep[f] = the face's component has > min_cells faces (keep[n_faces] = 0); used[v] = 1 for the vertices of kept faces
__global__ void __launch_bounds__(kT) keep_faces_kernel(const int* __restrict__ faces, long long n_faces, const int* __restrict__ label,
                                                        const int* __restrict__ cells, long long min_cells, int* __restrict__ keep,
                                                        int* __restrict__ used) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i > n_faces) return;
    int k = 0;
    if (i < n_faces) {
        k = (long long)cells[label[faces[3 * i]]] > min_cells;
        if (k)
            for (int j = 0; j < 3; ++j) used[faces[3 * i + j]] = 1;
    }
    keep[i] = k;
}

__global__ void __launch_bounds__(kT) keep_verts_kernel(const float* __restrict__ verts, long long n_verts, const int* __restrict__ used,
                                                        const int* __restrict__ remap, float* __restrict__ verts_out) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= n_verts || !used[v]) return;
    const long long o = remap[v];
    for (int k = 0; k < 3; ++k) verts_out[3 * o + k] = verts[3 * v + k];
}

__global__ void __launch_bounds__(kT) keep_faces_scatter_kernel(const int* __restrict__ faces, long long n_faces, const int* __restrict__ keep,
                                                                const int* __restrict__ fpos, const int* __restrict__ remap, int* __restrict__ faces_out) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n_faces || !keep[i]) return;
    const long long o = fpos[i];
    for (int k = 0; k < 3; ++k) faces_out[3 * o + k] = remap[faces[3 * i + k]];
}

struct KeepWs { CompWs comp; int *label, *cells, *keep, *fpos, *used, *remap, *scratch; };
size_t carve(KeepWs& w, const void* base, long long nv, long long nf) {
    oai::Ws ws(base);
    ws.off = carve(w.comp, base);
    w.label = ws.take<int>(nv);
    w.cells = ws.take<int>(nv);
    w.keep = ws.take<int>(nf + 1);
    w.fpos = ws.take<int>(nf + 1);
    w.used = ws.take<int>(nv + 1);
    w.remap = ws.take<int>(nv + 1);
    w.scratch = ws.take<int>(std::max(oai::scan_scratch_bytes(nf + 1), oai::scan_scratch_bytes(nv + 1)) / 4);
    return ws.off;
}

// ---------------------------------------------------------------------------------------------------------------------
// edge graph
// ---------------------------------------------------------------------------------------------------------------------
// every vertex of a face gets the face's other two corners: the host's 6 half-edges, duplicates and self-loops included
__global__ void __launch_bounds__(kT) degree_kernel(const int* __restrict__ faces, long long n_faces, long long n_verts, int* __restrict__ deg,
                                                    int* __restrict__ bad_index) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n_faces) return;
    const int* f = faces + 3 * i;
    if (!face_ok(f, n_verts)) { atomicOr(bad_index, 1); return; }
    for (int k = 0; k < 3; ++k) atomicAdd(deg + f[k], 2);
}

__global__ void __launch_bounds__(kT) scatter_kernel(const int* __restrict__ faces, long long n_faces, long long n_verts, const int* __restrict__ start,
                                                     int* __restrict__ cursor, int* __restrict__ half) {
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= n_faces) return;
    const int f[3] = {faces[3 * i], faces[3 * i + 1], faces[3 * i + 2]};
    if (!face_ok(f, n_verts)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long p = (long long)start[f[k]] + atomicAdd(cursor + f[k], 2);
        half[p] = f[(k + 1) % 3];
        half[p + 1] = f[(k + 2) % 3];
    }
}

template <int N>
__device__ __forceinline__ void bitonic_sort(int (&r)[N]) {
#pragma unroll
    for (int k = 2; k <= N; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0;
                    const int x = r[i], y = r[l];
                    const bool sw = up ? x > y : x < y;
                    r[i] = sw ? y : x;
                    r[l] = sw ? x : y;
                }
            }
}

// sorts the d <= N entries at list[0..d) in registers and writes the unique ones back to the front; returns their count
template <int N>
__device__ __forceinline__ int sort_unique_regs(int* list, int d) {
    int r[N];
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = i < d ? list[i] : INT_MAX;
    bitonic_sort<N>(r);
    int u = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (i < d && (i == 0 || r[i] != r[i - 1])) list[u++] = r[i];
    return u;
}

// vertex v: its d half-edge targets at half[start[v] ..) sorted, deduplicated in place; ucount[v] = unique count (ucount[n] = 0)
__global__ void __launch_bounds__(kT) sort_unique_kernel(const int* __restrict__ start, long long n_verts, int* __restrict__ half,
                                                         int* __restrict__ ucount) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v > n_verts) return;
    if (v == n_verts) { ucount[v] = 0; return; }
    int* list = half + start[v];
    const int d = start[v + 1] - start[v];
    int u;
    if (d <= 16) {
        u = sort_unique_regs<16>(list, d);
    } else if (d <= 32) {
        u = sort_unique_regs<32>(list, d);
    } else {                                           // a high-valence vertex (a fan): insertion sort in memory, then unique
        for (int i = 1; i < d; ++i) {
            const int x = list[i];
            int j = i - 1;
            while (j >= 0 && list[j] > x) { list[j + 1] = list[j]; --j; }
            list[j + 1] = x;
        }
        u = 1;
        for (int i = 1; i < d; ++i)
            if (list[i] != list[u - 1]) list[u++] = list[i];
    }
    ucount[v] = u;
}

__global__ void __launch_bounds__(kT) compact_kernel(const int* __restrict__ start, const int* __restrict__ offsets, long long n_verts,
                                                     const int* __restrict__ half, int* __restrict__ nbrs) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= n_verts) return;
    const int* src = half + start[v];
    int* dst = nbrs + offsets[v];
    const int u = offsets[v + 1] - offsets[v];
    for (int i = 0; i < u; ++i) dst[i] = src[i];
}

struct AdjWs { int *deg, *start, *half, *ucount, *bad, *scratch; };
size_t carve(AdjWs& w, const void* base, long long nv, long long nf) {
    oai::Ws ws(base);
    w.deg = ws.take<int>(nv + 1);
    w.start = ws.take<int>(nv + 1);
    ws.take<int>(nv);                              // unused (deg is its own fill cursor): keeps oai_mesh_adjacency_workspace_bytes where it was
    w.half = ws.take<int>(nf * 6);
    w.ucount = ws.take<int>(nv + 1);
    w.bad = ws.take<int>(1);
    w.scratch = ws.take<int>(oai::scan_scratch_bytes(nv + 1) / 4);
    return ws.off;
}

// ---------------------------------------------------------------------------------------------------------------------
// grid parameters: bounding box (float order through an integer key) and the largest squared edge (non-negative fp64: bit order)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int float_key(float f) {
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float key_float(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

struct GridAcc { int lo[3]; int hi[3]; int bad; int pad; unsigned long long max_sq; };

__global__ void grid_init_kernel(GridAcc* acc) {
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 3; ++k) { acc->lo[k] = INT_MAX; acc->hi[k] = INT_MIN; }
    acc->bad = 0;
    acc->max_sq = 0;
}

template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T x, Op op, T* sh) {
    for (int d = 32; d > 0; d >>= 1) x = op(x, __shfl_xor(x, d, 64));
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[wave] = x;
    __syncthreads();
    x = sh[0];
    for (int w = 1; w < kT / 64; ++w) x = op(x, sh[w]);
    return x;
}

__global__ void __launch_bounds__(kT) bounds_kernel(const float* __restrict__ verts, long long n_verts, GridAcc* acc) {
    __shared__ int sh[kT / 64];
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
    for (long long v = (long long)blockIdx.x * kT + threadIdx.x; v < n_verts; v += (long long)gridDim.x * kT)
        for (int k = 0; k < 3; ++k) {
            const int key = float_key(verts[3 * v + k]);
            lo[k] = min(lo[k], key);
            hi[k] = max(hi[k], key);
        }
    auto mn = [](int a, int b) { return min(a, b); };
    auto mx = [](int a, int b) { return max(a, b); };
    for (int k = 0; k < 3; ++k) {
        const int l = block_reduce(lo[k], mn, sh), h = block_reduce(hi[k], mx, sh);
        if (threadIdx.x == 0) { atomicMin(acc->lo + k, l); atomicMax(acc->hi + k, h); }
    }
}

__device__ __forceinline__ double sq_edge(const float* p, const float* q) {
    const double dx = __dsub_rn((double)p[0], (double)q[0]);
    const double dy = __dsub_rn((double)p[1], (double)q[1]);
    const double dz = __dsub_rn((double)p[2], (double)q[2]);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

__global__ void __launch_bounds__(kT) edge_kernel(const float* __restrict__ verts, long long n_verts, const int* __restrict__ faces, long long n_faces,
                                                  GridAcc* acc) {
    __shared__ unsigned long long sh[kT / 64];
    unsigned long long m = 0;
    bool bad = false;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n_faces; i += (long long)gridDim.x * kT) {
        const int* f = faces + 3 * i;
        if (!face_ok(f, n_verts)) { bad = true; continue; }
        const float *pa = verts + 3LL * f[0], *pb = verts + 3LL * f[1], *pc = verts + 3LL * f[2];
        const double e = fmax(fmax(sq_edge(pa, pb), sq_edge(pb, pc)), sq_edge(pc, pa));
        m = max(m, (unsigned long long)__double_as_longlong(e));
    }
    auto mx = [](unsigned long long a, unsigned long long b) { return max(a, b); };
    m = block_reduce(m, mx, sh);
    if (threadIdx.x == 0) atomicMax(&acc->max_sq, m);
    if (bad) atomicOr(&acc->bad, 1);
}

__global__ void grid_final_kernel(const GridAcc* acc, double* out7) {
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 3; ++k) {
        out7[k] = (double)key_float(acc->lo[k]);
        out7[3 + k] = (double)key_float(acc->hi[k]);
    }
    out7[6] = acc->bad ? __longlong_as_double(0x7ff8000000000000LL) : __longlong_as_double((long long)acc->max_sq);
}

}  // namespace

extern "C" {

size_t oai_mesh_components_workspace_bytes(long long n_verts, long long n_faces) {
    if (n_verts <= 0 || n_verts >= (1LL << 31) || n_faces < 0 || n_faces >= kMaxFaces) return 0;
    CompWs w;
    return carve(w, nullptr);
}

int oai_mesh_components(const int* faces_dev, long long n_faces, long long n_verts, void* workspace_dev, size_t workspace_bytes, int* label_dev,
                        int* rounds_host, void* stream) {
    OAI_CHECK_ARG(workspace_dev && label_dev && (faces_dev || n_faces == 0), "oai_mesh_components: null pointer");
    OAI_CHECK_ARG(n_faces >= 0 && n_faces < kMaxFaces, "oai_mesh_components: needs 0 .. 2^28-1 faces (got %lld)", n_faces);
    OAI_CHECK_ARG(n_verts >= 1 && n_verts < (1LL << 31), "oai_mesh_components: needs 1 .. 2^31-1 vertices (got %lld)", n_verts);
    CompWs w;
    OAI_CHECK_WORKSPACE("oai_mesh_components", workspace_bytes, carve(w, workspace_dev));
    return components(faces_dev, n_faces, n_verts, w, label_dev, rounds_host, (hipStream_t)stream, "oai_mesh_components");
}

size_t oai_mesh_keep_large_regions_workspace_bytes(long long n_verts, long long n_faces) {
    if (n_verts < 0 || n_verts >= (1LL << 31) || n_faces < 0 || n_faces >= kMaxFaces) return 0;
    KeepWs w;
    return carve(w, nullptr, n_verts, n_faces);
}

int oai_mesh_keep_large_regions(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, long long min_cells,
                                void* workspace_dev, size_t workspace_bytes, float* verts_out_dev, int* faces_out_dev, long long* n_verts_out_host,
                                long long* n_faces_out_host, void* stream) {
    OAI_CHECK_ARG(workspace_dev && n_verts_out_host && n_faces_out_host && (n_verts == 0 || (verts_dev && verts_out_dev)) &&
                      (n_faces == 0 || (faces_dev && faces_out_dev)), "oai_mesh_keep_large_regions: null pointer");
    OAI_CHECK_ARG(n_faces >= 0 && n_faces < kMaxFaces, "oai_mesh_keep_large_regions: needs 0 .. 2^28-1 faces (got %lld)", n_faces);
    OAI_CHECK_ARG(n_verts >= 0 && n_verts < (1LL << 31), "oai_mesh_keep_large_regions: needs 0 .. 2^31-1 vertices (got %lld)", n_verts);
    OAI_CHECK_ARG(n_faces == 0 || n_verts > 0, "oai_mesh_keep_large_regions: faces without vertices");
    KeepWs w;
    OAI_CHECK_WORKSPACE("oai_mesh_keep_large_regions", workspace_bytes, carve(w, workspace_dev, n_verts, n_faces));
    *n_verts_out_host = 0;
    *n_faces_out_host = 0;
    if (n_faces == 0) return OAI_OK;                   // the host returns verts[:0] and the empty face list
    hipStream_t st = (hipStream_t)stream;
    // validates every face index (error before anything below reads one)
    if (int rc = components(faces_dev, n_faces, n_verts, w.comp, w.label, nullptr, st, "oai_mesh_keep_large_regions")) return rc;
    OAI_CHECK_HIP(hipMemsetAsync(w.cells, 0, (size_t)n_verts * 4, st));
    OAI_CHECK_HIP(hipMemsetAsync(w.used, 0, (size_t)(n_verts + 1) * 4, st));
    region_cells_kernel<<<oai::cdiv(n_faces, kT), kT, 0, st>>>(faces_dev, n_faces, w.label, w.cells);
    OAI_CHECK_LAUNCH();
    keep_faces_kernel<<<oai::cdiv(n_faces + 1, kT), kT, 0, st>>>(faces_dev, n_faces, w.label, w.cells, min_cells, w.keep, w.used);
    OAI_CHECK_LAUNCH();
    if (int rc = oai::exclusive_scan_i32(w.keep, w.fpos, n_faces + 1, w.scratch, st)) return rc;
    if (int rc = oai::exclusive_scan_i32(w.used, w.remap, n_verts + 1, w.scratch, st)) return rc;
    keep_verts_kernel<<<oai::cdiv(n_verts, kT), kT, 0, st>>>(verts_dev, n_verts, w.used, w.remap, verts_out_dev);
    OAI_CHECK_LAUNCH();
    keep_faces_scatter_kernel<<<oai::cdiv(n_faces, kT), kT, 0, st>>>(faces_dev, n_faces, w.keep, w.fpos, w.remap, faces_out_dev);
    OAI_CHECK_LAUNCH();
    int counts[2];
    if (int rc = oai::read_ints(counts, {w.remap + n_verts, w.fpos + n_faces}, st)) return rc;
    *n_verts_out_host = counts[0];
    *n_faces_out_host = counts[1];
    return OAI_OK;
}

size_t oai_mesh_adjacency_workspace_bytes(long long n_verts, long long n_faces) {
    if (n_verts < 0 || n_verts >= (1LL << 31) || n_faces < 0 || n_faces >= kMaxFaces) return 0;
    AdjWs w;
    return carve(w, nullptr, n_verts, n_faces);
}

int oai_mesh_adjacency(const int* faces_dev, long long n_faces, long long n_verts, void* workspace_dev, size_t workspace_bytes, int* offsets_dev,
                       int* nbrs_dev, long long* n_nbrs_host, void* stream) {
    OAI_CHECK_ARG(workspace_dev && offsets_dev && n_nbrs_host && (n_faces == 0 || (faces_dev && nbrs_dev)), "oai_mesh_adjacency: null pointer");
    OAI_CHECK_ARG(n_faces >= 0 && n_faces < kMaxFaces, "oai_mesh_adjacency: needs 0 .. 2^28-1 faces (got %lld)", n_faces);
    OAI_CHECK_ARG(n_verts >= 0 && n_verts < (1LL << 31), "oai_mesh_adjacency: needs 0 .. 2^31-1 vertices (got %lld)", n_verts);
    AdjWs w;
    OAI_CHECK_WORKSPACE("oai_mesh_adjacency", workspace_bytes, carve(w, workspace_dev, n_verts, n_faces));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = oai::bucket_clear(w.deg, n_verts, st)) return rc;
    OAI_CHECK_HIP(hipMemsetAsync(w.bad, 0, sizeof(int), st));
    if (n_faces > 0) {
        degree_kernel<<<oai::cdiv(n_faces, kT), kT, 0, st>>>(faces_dev, n_faces, n_verts, w.deg, w.bad);
        OAI_CHECK_LAUNCH();
    }
    if (int rc = oai::bucket_starts(w.deg, w.start, n_verts, w.scratch, st)) return rc;
    if (n_faces > 0) {
        scatter_kernel<<<oai::cdiv(n_faces, kT), kT, 0, st>>>(faces_dev, n_faces, n_verts, w.start, w.deg, w.half);
        OAI_CHECK_LAUNCH();
    }
    sort_unique_kernel<<<oai::cdiv(n_verts + 1, kT), kT, 0, st>>>(w.start, n_verts, w.half, w.ucount);
    OAI_CHECK_LAUNCH();
    if (int rc = oai::exclusive_scan_i32(w.ucount, offsets_dev, n_verts + 1, w.scratch, st)) return rc;
    if (n_verts > 0) {
        compact_kernel<<<oai::cdiv(n_verts, kT), kT, 0, st>>>(w.start, offsets_dev, n_verts, w.half, nbrs_dev);
        OAI_CHECK_LAUNCH();
    }
    int h[2];
    if (int rc = oai::read_ints(h, {offsets_dev + n_verts, w.bad}, st)) return rc;
    if (h[1]) return oai::set_error(OAI_ERR_ARG, "oai_mesh_adjacency: a face indexes outside the %lld vertices", n_verts);
    *n_nbrs_host = h[0];
    return OAI_OK;
}

size_t oai_mesh_grid_params_workspace_bytes(void) { return 256; }

int oai_mesh_grid_params(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, void* workspace_dev,
                         size_t workspace_bytes, double* out7_dev, void* stream) {
    OAI_CHECK_ARG(verts_dev && workspace_dev && out7_dev && (faces_dev || n_faces == 0), "oai_mesh_grid_params: null pointer");
    OAI_CHECK_ARG(n_verts >= 1 && n_verts < (1LL << 31), "oai_mesh_grid_params: needs 1 .. 2^31-1 vertices (got %lld)", n_verts);
    OAI_CHECK_ARG(n_faces >= 0 && n_faces < kMaxFaces, "oai_mesh_grid_params: needs 0 .. 2^28-1 faces (got %lld)", n_faces);
    static_assert(sizeof(GridAcc) <= 256, "grid accumulator outgrew its workspace");
    OAI_CHECK_WORKSPACE("oai_mesh_grid_params", workspace_bytes, oai_mesh_grid_params_workspace_bytes());
    hipStream_t st = (hipStream_t)stream;
    GridAcc* acc = (GridAcc*)workspace_dev;
    grid_init_kernel<<<1, 64, 0, st>>>(acc);
    OAI_CHECK_LAUNCH();
    bounds_kernel<<<std::min<unsigned>(oai::cdiv(n_verts, kT), kRedBlocks), kT, 0, st>>>(verts_dev, n_verts, acc);
    OAI_CHECK_LAUNCH();
    if (n_faces > 0) {
        edge_kernel<<<std::min<unsigned>(oai::cdiv(n_faces, kT), kRedBlocks), kT, 0, st>>>(verts_dev, n_verts, faces_dev, n_faces, acc);
        OAI_CHECK_LAUNCH();
    }
    grid_final_kernel<<<1, 64, 0, st>>>(acc, out7_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
