// Mesh QC for gfx950 (include/oai_hip.h, "Mesh quality"; tests/mesh_quality_ref.py restates this file): what can be asked of the surface
// that the mesh-based thickness is measured on, before the distance is taken.
//   oai_mesh_topology            edge classes (boundary / manifold / misoriented / non-manifold, interface between the two sides of a
//                                split), their counts, Euler characteristic, boundary and interface loops
//   oai_mesh_geometry            area, signed enclosed volume, boundary and interface length, edge-length, face-area and triangle-quality figures
//   oai_mesh_self_intersections  pairs of faces without a common vertex of which one's edge properly pierces the other, through a uniform grid
//
// Topology is integer work: a CSR of half-edges keyed by the smaller vertex (count -> exclusive scan -> scatter; the atomics decide slots
// only), then every half-edge walks its vertex's list and decides by itself whether it owns its edge and what the edge is, so the scatter
// order never shows.  Loops are the connected components of an edge subset: one workgroup per subset runs hook / jump rounds (the scheme
// of csrc/mesh_graph.hip) over a compacted edge list until nothing changes -- inside the kernel, so nothing is read back.
// Geometry is fp64 without contraction; its sums follow csrc/ordered_reduce.h with the thread layout of surface_partials_kernel
// (csrc/edt.hip).  The predicates of the intersection test are fp64 determinants in one expansion order; what they add up are integers.
// No floating-point atomics.  Gather- and latency-bound VALU work on <= 10^5 faces: one element per thread, no LDS beyond the reductions.
#include "common.h"

#include <cmath>

#include "hook_jump.h"
#include "ordered_reduce.h"
#include "uniform_grid.h"

#pragma clang fp contract(off)

namespace {

using namespace oai;

constexpr int kT = 256;
constexpr int kLoopT = 1024;                       // the one workgroup of a loop count
constexpr long long kStreamBlocks = 2048;          // surface_partials_kernel's cap: grid-stride beyond that
constexpr int kTopoRec = 16, kSiRec = 4;         // int64 slots of the topology and intersection records (geometry: 16 doubles)

// slots of the topology record (and of its counters)
enum { kFaces, kDegenerate, kReferenced, kEdges, kBoundary, kMisoriented, kNonManifold, kInterface, kSideNeg, kSideZero, kSidePos, kEuler,
       kBoundaryLoops, kInterfaceLoops, kBadFaces, kManifold };
// edge classes
enum : unsigned char { kClsBoundary = 1, kClsManifold = 2, kClsMisoriented = 3, kClsNonManifold = 4, kClsMask = 15, kClsInterface = 16 };

typedef unsigned long long u64;

// *c += the number of lanes with p: one atomic per wave
__device__ __forceinline__ void wave_count(u64* c, bool p) {
    const u64 b = __ballot(p);
    if (p && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) atomicAdd(c, (u64)__popcll(b));
}

// 0: an index outside the mesh, 1: degenerate (two equal indices), 2: a triangle
__device__ __forceinline__ int face_state(const int* __restrict__ f, long long n) {
    if (!face_ok(f, n)) return 0;
    return (f[0] == f[1] || f[1] == f[2] || f[2] == f[0]) ? 1 : 2;
}
__device__ __forceinline__ void half_edge(const int* __restrict__ faces, int h, int& a, int& b) {
    const int f = h / 3, k = h - 3 * f;
    a = faces[3 * f + k];
    b = faces[3 * f + (k == 2 ? 0 : k + 1)];
}

// ---- oai_mesh_topology ---------------------------------------------------------------------------------------------------------------
// one thread per face: what it is, its side, one count per half-edge at the edge's smaller vertex, its corners referenced
__global__ void __launch_bounds__(kT) topo_face_kernel(const int* __restrict__ faces, long long nf, long long nv, const signed char* __restrict__ side,
                                                       int* __restrict__ count, int* __restrict__ used, u64* __restrict__ cnt) {
    const long long f = (long long)blockIdx.x * kT + threadIdx.x;
    int st = -1, sv = 2;
    if (f < nf) {
        const int* c = faces + 3 * f;
        st = face_state(c, nv);
        if (side) sv = side[f];
        if (st == 2)
            for (int k = 0; k < 3; ++k) {
                atomicAdd(&count[min(c[k], c[k == 2 ? 0 : k + 1])], 1);
                used[c[k]] = 1;
            }
    }
    wave_count(cnt + kBadFaces, st == 0);
    wave_count(cnt + kDegenerate, st == 1);
    wave_count(cnt + kSideNeg, sv == -1);
    wave_count(cnt + kSideZero, sv == 0);
    wave_count(cnt + kSidePos, sv == 1);
}

// one thread per half-edge: a slot in its smaller vertex's list (the order inside a list is whatever the atomics gave)
__global__ void __launch_bounds__(kT) topo_scatter_kernel(const int* __restrict__ faces, long long nf, long long nv, const int* __restrict__ start,
                                                          int* __restrict__ cursor, int* __restrict__ list) {
    const long long h = (long long)blockIdx.x * kT + threadIdx.x;
    if (h >= 3 * nf || face_state(faces + 3 * (h / 3), nv) != 2) return;
    int a, b;
    half_edge(faces, (int)h, a, b);
    const int lo = min(a, b);
    list[start[lo] + atomicAdd(&cursor[lo], 1)] = (int)h;
}

// one thread per half-edge: the half-edges of its edge among its smaller vertex's list -- how many, whether one has a smaller index (then
// this one is not the owner), how many others run the same way
__global__ void __launch_bounds__(kT) topo_classify_kernel(const int* __restrict__ faces, long long nf, long long nv, const signed char* __restrict__ side,
                                                           const int* __restrict__ start, const int* __restrict__ list,
                                                           unsigned char* __restrict__ edge_class, u64* __restrict__ cnt) {
    const long long h = (long long)blockIdx.x * kT + threadIdx.x;
    unsigned char cls = 0;
    if (h < 3 * nf && face_state(faces + 3 * (h / 3), nv) == 2) {
        int a, b;
        half_edge(faces, (int)h, a, b);
        const int lo = min(a, b), hi = max(a, b);
        int m = 0, same = 0, other = -1;
        bool owner = true;
        for (int t = start[lo], e = start[lo + 1]; t < e; ++t) {
            const int h2 = list[t];
            int a2, b2;
            half_edge(faces, h2, a2, b2);
            if (max(a2, b2) != hi) continue;
            ++m;
            if (h2 < h) owner = false;
            if (h2 != h) {
                other = h2;
                if ((a2 < b2) == (a < b)) ++same;
            }
        }
        if (owner) {
            cls = m == 1 ? kClsBoundary : (m == 2 ? (same ? kClsMisoriented : kClsManifold) : kClsNonManifold);
            if (cls == kClsManifold && side) {
                const int s1 = side[h / 3], s2 = side[other / 3];
                if ((s1 == -1 && s2 == 1) || (s1 == 1 && s2 == -1)) cls |= kClsInterface;
            }
        }
    }
    if (h < 3 * nf) edge_class[h] = cls;
    wave_count(cnt + kBoundary, (cls & kClsMask) == kClsBoundary);
    wave_count(cnt + kManifold, (cls & kClsMask) == kClsManifold);
    wave_count(cnt + kMisoriented, (cls & kClsMask) == kClsMisoriented);
    wave_count(cnt + kNonManifold, (cls & kClsMask) == kClsNonManifold);
    wave_count(cnt + kInterface, (cls & kClsInterface) != 0);
}

__global__ void __launch_bounds__(kT) topo_referenced_kernel(const int* __restrict__ used, long long nv, u64* __restrict__ cnt) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    wave_count(cnt + kReferenced, v < nv && used[v] != 0);
}

// the boundary edges into list 0 and the interface edges into list 1 (any order: only the number of components is taken), each end
// point its own parent
__global__ void __launch_bounds__(kT) topo_collect_kernel(const int* __restrict__ faces, long long nf, long long nv, const unsigned char* __restrict__ edge_class,
                                                          int* __restrict__ n_list, int* __restrict__ lists, int* __restrict__ parent) {
    const long long h = (long long)blockIdx.x * kT + threadIdx.x;
    if (h >= 3 * nf) return;
    const unsigned char cls = edge_class[h];
    const bool in0 = (cls & kClsMask) == kClsBoundary, in1 = (cls & kClsInterface) != 0;
    if (!in0 && !in1) return;
    int a, b;
    half_edge(faces, (int)h, a, b);
    const int w = in0 ? 0 : 1;                     // an interface edge is manifold: never both
    lists[(long long)w * 3 * nf + atomicAdd(&n_list[w], 1)] = (int)h;
    parent[(long long)w * nv + a] = a;
    parent[(long long)w * nv + b] = b;
}

// workgroup w: the connected components of edge list w.  Rounds of hook then jump with a barrier between, until a round hooks nothing
// (every round that hooks removes a root: at most n + 1 rounds); then each root is claimed once.
__global__ void __launch_bounds__(kLoopT) topo_loops_kernel(const int* __restrict__ faces, long long nf, long long nv, const int* __restrict__ n_list,
                                                            const int* __restrict__ lists, int* parent_all, u64* __restrict__ cnt) {
    __shared__ int changed, roots;
    const int w = blockIdx.x, n = n_list[w];
    const int* list = lists + (long long)w * 3 * nf;
    int* parent = parent_all + (long long)w * nv;
    for (long long it = 0; it <= (long long)n + 1; ++it) {
        if (threadIdx.x == 0) changed = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kLoopT) {
            int a, b;
            half_edge(faces, list[i], a, b);
            if (hook(parent, a, b)) changed = 1;
        }
        __syncthreads();
        const int c = changed;
        for (int i = threadIdx.x; i < n; i += kLoopT) {
            int a, b;
            half_edge(faces, list[i], a, b);
            jump(parent, a);
            jump(parent, b);
        }
        __syncthreads();
        if (!c) break;
    }
    if (threadIdx.x == 0) roots = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kLoopT) {
        int ab[2];
        half_edge(faces, list[i], ab[0], ab[1]);
        for (int k = 0; k < 2; ++k)
            if (atomicCAS(parent + ab[k], ab[k], -1) == ab[k]) atomicAdd(&roots, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) cnt[kBoundaryLoops + w] = (u64)roots;
}

__global__ void topo_finish_kernel(const u64* __restrict__ cnt, long long nf, long long* __restrict__ rec) {
    if (threadIdx.x != 0) return;
    long long r[kTopoRec];
    for (int i = 0; i < kTopoRec; ++i) r[i] = (long long)cnt[i];
    r[kFaces] = nf;
    r[kEdges] = r[kBoundary] + r[kManifold] + r[kMisoriented] + r[kNonManifold];
    r[kEuler] = r[kReferenced] - r[kEdges] + (nf - r[kDegenerate] - r[kBadFaces]);
    for (int i = 0; i < kTopoRec; ++i) rec[i] = r[i];
}

struct TopoWs {
    u64* cnt;
    int *n_list, *count, *start, *used, *list, *lists, *parent, *scratch;
    size_t bytes;
    TopoWs(void* workspace, long long nv, long long nf) {
        Ws ws(workspace);
        cnt = ws.take<u64>(kTopoRec);
        n_list = ws.take<int>(2);
        count = ws.take<int>((size_t)nv + 1);
        start = ws.take<int>((size_t)nv + 1);
        used = ws.take<int>((size_t)nv + 1);
        list = ws.take<int>((size_t)(3 * nf));
        lists = ws.take<int>((size_t)(6 * nf));
        parent = ws.take<int>((size_t)(2 * nv));
        scratch = ws.take<int>(scan_scratch_bytes(nv + 1) / 4);
        bytes = ws.off;
    }
};

// ---- oai_mesh_geometry ---------------------------------------------------------------------------------------------------------------
constexpr int kGA = 14;
// sum area, sum det, min area, max area, min q, sum q, faces with q < q_min, faces | boundary length, interface length, min, max, sum edge length, edges
struct GeoAcc {
    double v[kGA];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < kGA; ++i) v[i] = 0.0;
        v[2] = INFINITY; v[3] = -INFINITY; v[4] = INFINITY; v[10] = INFINITY; v[11] = -INFINITY;
    }
    __device__ __forceinline__ void merge(const double* o) {       // this (the earlier elements) on the left of every operation
#pragma unroll
        for (int i = 0; i < kGA; ++i)
            v[i] = (i == 2 || i == 4 || i == 10) ? fmin(v[i], o[i]) : ((i == 3 || i == 11) ? fmax(v[i], o[i]) : v[i] + o[i]);
    }
};

__device__ __forceinline__ double sq_len(const double* p, const double* q) {
    const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
    return (dx * dx + dy * dy) + dz * dz;
}
// det of the rows u, v, w, the one expansion order of this file
__device__ __forceinline__ double det3(double ux, double uy, double uz, double vx, double vy, double vz, double wx, double wy, double wz) {
    return (ux * (vy * wz - vz * wy) - uy * (vx * wz - vz * wx)) + uz * (vx * wy - vy * wx);
}
__device__ __forceinline__ void corner(const float* __restrict__ verts, int i, double* p) {
    const float* s = verts + 3 * (long long)i;
    p[0] = (double)s[0]; p[1] = (double)s[1]; p[2] = (double)s[2];
}

__global__ void __launch_bounds__(kT)
geo_partials_kernel(const float* __restrict__ verts, long long nv, const int* __restrict__ faces, long long nf, const unsigned char* __restrict__ edge_class,
                    double ox, double oy, double oz, double q_min, double* __restrict__ partials) {
    __shared__ double lds[kT / 64][kGA];
    GeoAcc acc;
    acc.clear();
    for (long long f = (long long)blockIdx.x * kT + threadIdx.x; f < nf; f += (long long)gridDim.x * kT) {
        const int* c = faces + 3 * f;
        if (!face_ok(c, nv)) continue;
        double p[3][3];
        for (int k = 0; k < 3; ++k) corner(verts, c[k], p[k]);
        const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
        const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
        const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
        const double area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
        const double l[3] = {sq_len(p[0], p[1]), sq_len(p[1], p[2]), sq_len(p[2], p[0])};
        const double den = (l[0] + l[1]) + l[2];
        const double q = den > 0.0 ? (6.928203230275509 * area) / den : 0.0;
        const double det = det3(p[0][0] - ox, p[0][1] - oy, p[0][2] - oz, p[1][0] - ox, p[1][1] - oy, p[1][2] - oz, p[2][0] - ox, p[2][1] - oy,
                                p[2][2] - oz);
        acc.v[0] = acc.v[0] + area; acc.v[1] = acc.v[1] + det;
        acc.v[2] = fmin(acc.v[2], area); acc.v[3] = fmax(acc.v[3], area);
        acc.v[4] = fmin(acc.v[4], q); acc.v[5] = acc.v[5] + q;
        if (q < q_min) acc.v[6] = acc.v[6] + 1.0;
        acc.v[7] = acc.v[7] + 1.0;
        for (int k = 0; k < 3; ++k) {
            const unsigned char cls = edge_class[3 * f + k];
            if (!cls) continue;
            const double len = sqrt(l[k]);
            if ((cls & kClsMask) == kClsBoundary) acc.v[8] = acc.v[8] + len;
            if (cls & kClsInterface) acc.v[9] = acc.v[9] + len;
            acc.v[10] = fmin(acc.v[10], len); acc.v[11] = fmax(acc.v[11], len);
            acc.v[12] = acc.v[12] + len; acc.v[13] = acc.v[13] + 1.0;
        }
    }
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0)
        for (int i = 0; i < kGA; ++i) partials[(long long)blockIdx.x * kGA + i] = acc.v[i];
}

__global__ void __launch_bounds__(kT) geo_finish_kernel(const double* __restrict__ partials, long long nb, double* __restrict__ out) {
    __shared__ double lds[kT / 64][kGA];
    GeoAcc acc;
    reduce_slots<kT>(partials, nb, acc);
    block_reduce<kT>(acc, lds);
    if (threadIdx.x != 0) return;
    const double* a = acc.v;
    const bool faces = a[7] > 0.0, edges = a[13] > 0.0;
    out[0] = a[0];
    out[1] = a[1] / 6.0;
    out[2] = a[8];
    out[3] = a[9];
    out[4] = edges ? a[10] : 0.0;
    out[5] = edges ? a[11] : 0.0;
    out[6] = edges ? a[12] / a[13] : 0.0;
    out[7] = faces ? a[2] : 0.0;
    out[8] = faces ? a[3] : 0.0;
    out[9] = faces ? a[4] : 0.0;
    out[10] = faces ? a[5] / a[7] : 0.0;
    out[11] = a[6];
    out[12] = a[13];
    out[13] = a[7];
    out[14] = 0.0;
    out[15] = 0.0;
}

struct GeoWs {
    double* partials;
    long long blocks;
    size_t bytes;
    GeoWs(void* workspace, long long nf) {
        Ws ws(workspace);
        blocks = (long long)grid_stride_blocks(nf, kT * 4, kStreamBlocks);
        partials = ws.take<double>((size_t)blocks * kGA);
        bytes = ws.off;
    }
};

// ---- oai_mesh_self_intersections -----------------------------------------------------------------------------------------------------
enum { kPairs, kFlagged, kNeeded, kOverflow };

// one thread per face: the cells its bounding box spans (range[f] = lo xyz, hi xyz; hi < lo for a face with a bad index), and their number
__global__ void __launch_bounds__(kT) si_range_kernel(const float* __restrict__ verts, long long nv, const int* __restrict__ faces, long long nf, UniformGrid g,
                                                      int* __restrict__ range, u64* __restrict__ cnt) {
    const long long f = (long long)blockIdx.x * kT + threadIdx.x;
    u64 cells = 0;
    if (f < nf) {
        const int* c = faces + 3 * f;
        int r[6] = {0, 0, 0, -1, -1, -1};
        if (face_ok(c, nv)) {
            const float *a = verts + 3 * (long long)c[0], *b = verts + 3 * (long long)c[1], *d = verts + 3 * (long long)c[2];
            cells = 1;
            for (int k = 0; k < 3; ++k) {
                r[k] = grid_cell(g, k, fminf(fminf(a[k], b[k]), d[k]));
                r[3 + k] = max(r[k], grid_cell(g, k, fmaxf(fmaxf(a[k], b[k]), d[k])));
                cells *= (u64)(r[3 + k] - r[k] + 1);
            }
        }
        for (int k = 0; k < 6; ++k) range[6 * f + k] = r[k];
    }
    for (int off = 32; off >= 1; off >>= 1) cells += __shfl_xor(cells, off, 64);
    if ((threadIdx.x & 63) == 0 && cells) atomicAdd(cnt + kNeeded, cells);
}

// count (cursor null) or scatter the (cell, face) entries; nothing when they would not fit
__global__ void __launch_bounds__(kT) si_bin_kernel(const int* __restrict__ range, long long nf, UniformGrid g, const u64* __restrict__ cnt, long long capacity,
                                                    int* __restrict__ count, const int* __restrict__ start, int* __restrict__ entries) {
    const long long f = (long long)blockIdx.x * kT + threadIdx.x;
    if (f >= nf || cnt[kNeeded] > (u64)capacity) return;
    const int* r = range + 6 * f;
    grid_walk_box(r[0], r[1], r[2], r[3], r[4], r[5], [&](int x, int y, int z) {
        const int cell = grid_index(g, x, y, z);
        const int slot = atomicAdd(&count[cell], 1);
        if (entries) entries[start[cell] + slot] = (int)f;
    });
}

// orient(a, b, c, d) = det(b - a, c - a, d - a)
__device__ __forceinline__ double orient(const double* a, const double* b, const double* c, const double* d) {
    return det3(b[0] - a[0], b[1] - a[1], b[2] - a[2], c[0] - a[0], c[1] - a[1], c[2] - a[2], d[0] - a[0], d[1] - a[1], d[2] - a[2]);
}
// the edge pq properly pierces the triangle abc
__device__ __forceinline__ bool pierces(const double* p, const double* q, const double* a, const double* b, const double* c) {
    const double s1 = orient(a, b, c, p), s2 = orient(a, b, c, q);
    if (!((s1 > 0.0 && s2 < 0.0) || (s1 < 0.0 && s2 > 0.0))) return false;
    const double t1 = orient(p, q, a, b), t2 = orient(p, q, b, c), t3 = orient(p, q, c, a);
    return (t1 > 0.0 && t2 > 0.0 && t3 > 0.0) || (t1 < 0.0 && t2 < 0.0 && t3 < 0.0);
}

// one thread per face f: in each of its cells the faces g > f of the cell's list, tested only where the cell is the one that holds the
// lower corner of the two cell ranges' intersection
__global__ void __launch_bounds__(kT) si_pairs_kernel(const float* __restrict__ verts, const int* __restrict__ faces, long long nf, UniformGrid g,
                                                      const int* __restrict__ range, const int* __restrict__ start, const int* __restrict__ entries,
                                                      long long capacity, unsigned char* __restrict__ flag, u64* __restrict__ cnt) {
    const long long f = (long long)blockIdx.x * kT + threadIdx.x;
    u64 pairs = 0;
    if (f < nf && cnt[kNeeded] <= (u64)capacity && range[6 * f + 3] >= range[6 * f]) {
        const int* r = range + 6 * f;
        const int fi[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        double P[3][3];
        for (int k = 0; k < 3; ++k) corner(verts, fi[k], P[k]);
        double plo[3], phi[3];
        for (int k = 0; k < 3; ++k) {
            plo[k] = fmin(fmin(P[0][k], P[1][k]), P[2][k]);
            phi[k] = fmax(fmax(P[0][k], P[1][k]), P[2][k]);
        }
        bool mine = false;
        grid_walk_box(r[0], r[1], r[2], r[3], r[4], r[5], [&](int x, int y, int z) {
            const int cell = grid_index(g, x, y, z);
            for (int t = start[cell], e = start[cell + 1]; t < e; ++t) {
                const int gf = entries[t];
                if (gf <= f) continue;
                const int* s = range + 6 * (long long)gf;
                if (max(r[0], s[0]) != x || max(r[1], s[1]) != y || max(r[2], s[2]) != z) continue;
                const int gi[3] = {faces[3 * (long long)gf], faces[3 * (long long)gf + 1], faces[3 * (long long)gf + 2]};
                bool shared = false;
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) shared = shared || fi[i] == gi[j];
                if (shared) continue;
                double Q[3][3];
                for (int k = 0; k < 3; ++k) corner(verts, gi[k], Q[k]);
                bool apart = false;                        // disjoint boxes cannot pierce: skips the determinants, changes no answer
                for (int k = 0; k < 3; ++k) {
                    const double qlo = fmin(fmin(Q[0][k], Q[1][k]), Q[2][k]), qhi = fmax(fmax(Q[0][k], Q[1][k]), Q[2][k]);
                    apart = apart || qhi < plo[k] || phi[k] < qlo;
                }
                if (apart) continue;
                bool hit = false;
                for (int k = 0; k < 3 && !hit; ++k) hit = pierces(P[k], P[k == 2 ? 0 : k + 1], Q[0], Q[1], Q[2]);
                for (int k = 0; k < 3 && !hit; ++k) hit = pierces(Q[k], Q[k == 2 ? 0 : k + 1], P[0], P[1], P[2]);
                if (!hit) continue;
                ++pairs;
                mine = true;
                flag[gf] = 1;
            }
        });
        if (mine) flag[f] = 1;
    }
    for (int off = 32; off >= 1; off >>= 1) pairs += __shfl_xor(pairs, off, 64);
    if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(cnt + kPairs, pairs);
}

__global__ void __launch_bounds__(kT) si_flagged_kernel(const unsigned char* __restrict__ flag, long long nf, u64* __restrict__ cnt) {
    const long long f = (long long)blockIdx.x * kT + threadIdx.x;
    wave_count(cnt + kFlagged, f < nf && flag[f] != 0);
}

__global__ void si_finish_kernel(const u64* __restrict__ cnt, long long capacity, long long* __restrict__ rec) {
    if (threadIdx.x != 0) return;
    rec[kPairs] = (long long)cnt[kPairs];
    rec[kFlagged] = (long long)cnt[kFlagged];
    rec[kNeeded] = (long long)cnt[kNeeded];
    rec[kOverflow] = cnt[kNeeded] > (u64)capacity ? 1 : 0;
}

struct SiWs {
    u64* cnt;
    int *range, *count, *start, *entries, *scratch;
    long long cells;
    size_t bytes;
    SiWs(void* workspace, long long nf, const int* dims, long long capacity) {
        Ws ws(workspace);
        cells = (long long)dims[0] * dims[1] * dims[2];
        cnt = ws.take<u64>(kSiRec);
        range = ws.take<int>((size_t)(6 * nf));
        count = ws.take<int>((size_t)cells + 1);
        start = ws.take<int>((size_t)cells + 1);
        entries = ws.take<int>((size_t)capacity);
        scratch = ws.take<int>(scan_scratch_bytes(cells + 1) / 4);
        bytes = ws.off;
    }
};

bool grid_ok(const int* d) {
    return d && d[0] >= 1 && d[1] >= 1 && d[2] >= 1 && (long long)d[0] * d[1] <= (1LL << 31) - 2 && (long long)d[0] * d[1] * d[2] <= (1LL << 31) - 2;
}
bool capacity_ok(long long c) { return c >= 0 && c <= (1LL << 31) - 2; }

}  // namespace

extern "C" {

size_t oai_mesh_topology_workspace_bytes(long long n_verts, long long n_faces) {
    if (!mesh_ok(n_verts, n_faces)) return 0;
    return TopoWs(nullptr, n_verts, n_faces).bytes;
}

int oai_mesh_topology(const int* faces_dev, long long n_faces, long long n_verts, const signed char* side_dev, void* workspace_dev, size_t workspace_bytes,
                      unsigned char* edge_class_dev, long long* record_dev, void* stream) {
    OAI_CHECK_ARG(mesh_ok(n_verts, n_faces), "oai_mesh_topology: needs 0 .. 2^31-2 vertices and 0 .. 2^28 faces (got %lld, %lld)", n_verts, n_faces);
    OAI_CHECK_ARG(workspace_dev && record_dev && (n_faces == 0 || (faces_dev && edge_class_dev)), "oai_mesh_topology: null pointer");
    OAI_CHECK_WORKSPACE("oai_mesh_topology", workspace_bytes, oai_mesh_topology_workspace_bytes(n_verts, n_faces));
    const TopoWs ws(workspace_dev, n_verts, n_faces);
    const hipStream_t st = (hipStream_t)stream;
    const long long nf = n_faces, nv = n_verts;
    OAI_CHECK_HIP(hipMemsetAsync(ws.cnt, 0, kTopoRec * sizeof(u64), st));
    if (nf) {
        OAI_CHECK_HIP(hipMemsetAsync(ws.n_list, 0, 2 * sizeof(int), st));
        if (int rc = bucket_clear(ws.count, nv, st)) return rc;
        OAI_CHECK_HIP(hipMemsetAsync(ws.used, 0, (size_t)(nv + 1) * 4, st));
        topo_face_kernel<<<cdiv(nf, kT), kT, 0, st>>>(faces_dev, nf, nv, side_dev, ws.count, ws.used, ws.cnt);
        OAI_CHECK_LAUNCH();
        if (int rc = bucket_starts(ws.count, ws.start, nv, ws.scratch, st)) return rc;
        topo_scatter_kernel<<<cdiv(3 * nf, kT), kT, 0, st>>>(faces_dev, nf, nv, ws.start, ws.count, ws.list);
        OAI_CHECK_LAUNCH();
        topo_classify_kernel<<<cdiv(3 * nf, kT), kT, 0, st>>>(faces_dev, nf, nv, side_dev, ws.start, ws.list, edge_class_dev, ws.cnt);
        OAI_CHECK_LAUNCH();
        if (nv) {
            topo_referenced_kernel<<<cdiv(nv, kT), kT, 0, st>>>(ws.used, nv, ws.cnt);
            OAI_CHECK_LAUNCH();
        }
        topo_collect_kernel<<<cdiv(3 * nf, kT), kT, 0, st>>>(faces_dev, nf, nv, edge_class_dev, ws.n_list, ws.lists, ws.parent);
        OAI_CHECK_LAUNCH();
        topo_loops_kernel<<<2, kLoopT, 0, st>>>(faces_dev, nf, nv, ws.n_list, ws.lists, ws.parent, ws.cnt);
        OAI_CHECK_LAUNCH();
    }
    topo_finish_kernel<<<1, 64, 0, st>>>(ws.cnt, nf, record_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_mesh_geometry_workspace_bytes(long long n_faces) {
    if (n_faces < 0 || n_faces > kMaxFaces) return 0;
    return GeoWs(nullptr, n_faces).bytes;
}

int oai_mesh_geometry(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, const unsigned char* edge_class_dev,
                      const double origin[3], double q_min, void* workspace_dev, size_t workspace_bytes, double* record_dev, void* stream) {
    OAI_CHECK_ARG(mesh_ok(n_verts, n_faces), "oai_mesh_geometry: needs 0 .. 2^31-2 vertices and 0 .. 2^28 faces (got %lld, %lld)", n_verts, n_faces);
    OAI_CHECK_ARG(workspace_dev && record_dev && origin && (n_faces == 0 || (faces_dev && edge_class_dev && (verts_dev || n_verts == 0))),
                  "oai_mesh_geometry: null pointer");
    OAI_CHECK_WORKSPACE("oai_mesh_geometry", workspace_bytes, oai_mesh_geometry_workspace_bytes(n_faces));
    const GeoWs ws(workspace_dev, n_faces);
    const hipStream_t st = (hipStream_t)stream;
    geo_partials_kernel<<<(unsigned)ws.blocks, kT, 0, st>>>(verts_dev, n_verts, faces_dev, n_faces, edge_class_dev, origin[0], origin[1], origin[2], q_min,
                                                            ws.partials);
    OAI_CHECK_LAUNCH();
    geo_finish_kernel<<<1, kT, 0, st>>>(ws.partials, ws.blocks, record_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_mesh_self_intersections_workspace_bytes(long long n_faces, const int grid_dims[3], long long capacity) {
    if (n_faces < 0 || n_faces > kMaxFaces || !grid_ok(grid_dims) || !capacity_ok(capacity)) return 0;
    return SiWs(nullptr, n_faces, grid_dims, capacity).bytes;
}

int oai_mesh_self_intersections(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, const double grid_lo[3],
                                double cell_size, const int grid_dims[3], long long capacity, void* workspace_dev, size_t workspace_bytes,
                                unsigned char* flag_dev, long long* record_dev, void* stream) {
    OAI_CHECK_ARG(mesh_ok(n_verts, n_faces), "oai_mesh_self_intersections: needs 0 .. 2^31-2 vertices and 0 .. 2^28 faces (got %lld, %lld)", n_verts,
                  n_faces);
    OAI_CHECK_ARG(workspace_dev && record_dev && grid_lo && grid_dims && (n_faces == 0 || (faces_dev && flag_dev && (verts_dev || n_verts == 0))),
                  "oai_mesh_self_intersections: null pointer");
    OAI_CHECK_ARG(cell_size > 0.0 && cell_size < INFINITY, "oai_mesh_self_intersections: cell_size must be positive and finite (got %g)", cell_size);
    OAI_CHECK_ARG(grid_lo[0] - grid_lo[0] == 0.0 && grid_lo[1] - grid_lo[1] == 0.0 && grid_lo[2] - grid_lo[2] == 0.0,
                  "oai_mesh_self_intersections: grid_lo must be finite");
    OAI_CHECK_ARG(grid_dims[0] >= 1 && grid_dims[1] >= 1 && grid_dims[2] >= 1, "oai_mesh_self_intersections: empty grid (%d x %d x %d)", grid_dims[0],
                  grid_dims[1], grid_dims[2]);
    OAI_CHECK_ARG(grid_ok(grid_dims), "oai_mesh_self_intersections: the grid has more than 2^31-2 cells (%d x %d x %d)", grid_dims[0], grid_dims[1],
                  grid_dims[2]);
    OAI_CHECK_ARG(capacity_ok(capacity), "oai_mesh_self_intersections: capacity must be in [0, 2^31-2] (got %lld)", capacity);
    OAI_CHECK_WORKSPACE("oai_mesh_self_intersections", workspace_bytes, oai_mesh_self_intersections_workspace_bytes(n_faces, grid_dims, capacity));
    const SiWs ws(workspace_dev, n_faces, grid_dims, capacity);
    const hipStream_t st = (hipStream_t)stream;
    const long long nf = n_faces;
    const UniformGrid g = make_uniform_grid(grid_lo, cell_size, grid_dims);
    OAI_CHECK_HIP(hipMemsetAsync(ws.cnt, 0, kSiRec * sizeof(u64), st));
    if (nf) {
        OAI_CHECK_HIP(hipMemsetAsync(flag_dev, 0, (size_t)nf, st));
        if (int rc = bucket_clear(ws.count, ws.cells, st)) return rc;
        si_range_kernel<<<cdiv(nf, kT), kT, 0, st>>>(verts_dev, n_verts, faces_dev, nf, g, ws.range, ws.cnt);
        OAI_CHECK_LAUNCH();
        si_bin_kernel<<<cdiv(nf, kT), kT, 0, st>>>(ws.range, nf, g, ws.cnt, capacity, ws.count, nullptr, nullptr);
        OAI_CHECK_LAUNCH();
        if (int rc = bucket_starts(ws.count, ws.start, ws.cells, ws.scratch, st)) return rc;
        si_bin_kernel<<<cdiv(nf, kT), kT, 0, st>>>(ws.range, nf, g, ws.cnt, capacity, ws.count, ws.start, ws.entries);
        OAI_CHECK_LAUNCH();
        si_pairs_kernel<<<cdiv(nf, kT), kT, 0, st>>>(verts_dev, faces_dev, nf, g, ws.range, ws.start, ws.entries, capacity, flag_dev, ws.cnt);
        OAI_CHECK_LAUNCH();
        si_flagged_kernel<<<cdiv(nf, kT), kT, 0, st>>>(flag_dev, nf, ws.cnt);
        OAI_CHECK_LAUNCH();
    }
    si_finish_kernel<<<1, 64, 0, st>>>(ws.cnt, capacity, record_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
