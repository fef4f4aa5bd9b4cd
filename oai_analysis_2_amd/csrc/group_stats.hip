// Cohort statistics for gfx950 (include/oai_hip.h, "Cohort statistics"; tests/group_stats_ref.py restates this file operation for
// operation): permutation tests on N per-knee vectors that share the atlas inner vertices.
//   oai_group_prepare        per vertex: n, mean, std, and the (centred) values c and their squares q that every permutation re-sums
//   oai_permutation_t        a batch of labellings -> one t per (labelling, vertex): pooled two-sample t, or one-sample t under sign flips
//   oai_permutation_reduce   per labelling max |t|; per vertex the count of labellings with |t| >= the observed |t|
//   oai_graph_clusters       per row of a value tile, the connected components of {t > t0} and {t < -t0} on the surface graph
//
// fp64 without contraction.  The order IS the contract: every sum over knees runs in ascending knee index with one accumulator, in one
// thread.  No floating-point atomics; max |t| is an exact maximum (csrc/ordered_reduce.h), the counts are integers.
//
// Shape of the t kernel, and why.  A wave64 covers 64 consecutive vertices of the same R labellings, so knee i's c and q are two
// coalesced 512-byte loads per wave, used R times, and the label word of (labelling, knee / 32) is the same for the whole wave: its
// address is made of kernel arguments, blockIdx and loop counters only, so it is a scalar load into SGPRs and the bit test is scalar.
//   R = 16 labellings per thread.  The cost per (knee, thread) is 17 bytes of load against 2 R fp64 operations; fp64 VALU runs at half
//     the fp32 rate (MI355X_MICROARCH.md: 157.3 TFLOPS fp32 vector counts an FMA as two, so 39.3e12 fp64 instructions per second over
//     256 CUs at 2.4 GHz: 64 lanes per clock and CU, a wave64 instruction every 4 clocks on its SIMD).  At R = 16 the 32 operations of
//     a wave take 128 issue clocks per 1088 bytes loaded: 34 B/clk/CU, which the L2 holds (the c / q block of a vertex span is
//     N x 256 x 16 B = 0.8 MB at N = 200 and is re-read by every row group); at R = 8 the kernel would ask twice that and sit on the
//     memory side.  R = 32 would need 160 accumulator VGPRs (S1, Q1: 4 each, n1: 1) and leave one wave per SIMD.  R = 16 has 80; with
//     four knees of loads in flight the compiler allocates 130 with a mask (102 without, 55 one-sample): 3 waves per SIMD (4, 8), no
//     scratch.  Capping it at 128 spills, so it is not capped.
//   Block = 256 threads = 4 waves = 256 vertices x 16 labellings (cdna_hip_programming.md: 256-thread blocks, <= 4 per CU); the grid
//     is one-dimensional, row groups fastest.  No LDS: nothing is shared between lanes, reuse is in registers.
//   Knee tile = 32 = one label word: R scalar loads, then 32 knees of vector work.
//   Measured (profiles/group_stats.md): N = 200, V = 30 002, 1000 labellings in 1.37 ms, 22 % of the fp64 vector issue rate.
// The other kernels are latency-bound integer or streaming work: one element per thread or one workgroup per row.
#include "cohort.h"

#include <cmath>

#include "hook_jump.h"
#include "ordered_reduce.h"

#pragma clang fp contract(off)

namespace {

using namespace oai;

constexpr int kT = 256;                            // vertices of a block (prepare, t, exceed)
constexpr int kR = 16;                             // labellings per thread of the t kernel
constexpr int kClusterT = 1024;                    // the workgroup of one row of oai_graph_clusters
constexpr long long kMaxBlocks = 1024;             // of a row's max |t| partials

// ---- the prepared block ----------------------------------------------------------------------------------------------------------------
struct Prepared {
    double *C, *Qm, *S, *Q, *mean, *sd;
    int* n;
    size_t bytes;
    Prepared(const void* base, long long N, long long V) {
        Ws ws(base);
        C = ws.take<double>((size_t)(N * V));
        Qm = ws.take<double>((size_t)(N * V));
        S = ws.take<double>((size_t)V);
        Q = ws.take<double>((size_t)V);
        mean = ws.take<double>((size_t)V);
        sd = ws.take<double>((size_t)V);
        n = ws.take<int>((size_t)V);
        bytes = ws.off;
    }
};

// one thread per vertex, knees in ascending index: the counted sum, then the (centred) values and their sums
__global__ void __launch_bounds__(kT) prepare_kernel(const float* __restrict__ Y, const unsigned char* __restrict__ mask, long long N, long long V,
                                                     int centre, Prepared out) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= V) return;
    const CountedMean counted = counted_mean(Y, mask, N, V, v);
    const int n = counted.n;
    const double mu = counted.mean;
    double s = 0.0, q = 0.0, qd = 0.0;
    for (long long i = 0; i < N; ++i) {
        const bool m = mask ? mask[i * V + v] != 0 : true;
        const double y = m ? (double)Y[i * V + v] : 0.0;
        const double d = m ? y - mu : 0.0;
        const double c = centre ? d : y;
        const double cc = c * c;
        out.C[i * V + v] = c;
        out.Qm[i * V + v] = cc;
        s = s + c;
        q = q + cc;
        qd = qd + d * d;
    }
    out.n[v] = n;
    out.mean[v] = mu;
    out.sd[v] = n >= 2 ? sqrt(qd / (double)(n - 1)) : (double)NAN;
    out.S[v] = s;
    out.Q[v] = q;
}

// ---- oai_permutation_t -----------------------------------------------------------------------------------------------------------------
// Block b of a one-dimensional grid is row group b % groups of vertex span b / groups: the row groups of a span are dispatched next
// to each other and read the span's c / q block from L2 while it is there (spans-fastest order walks the whole N x V block once per
// row group, 96 MB at N = 200, V = 30 000: every read then comes from beyond L2, and the kernel ran at 4.5 TB/s of such traffic).
// Thread = one vertex x kR labellings.  A lane past V works on vertex V - 1 and stores nothing.
// "s + (b ? c : 0.0)" is issued as ONE operation, fma(c, b ? 1.0 : 0.0, s) with the factor in scalar registers: the product c * 1.0 or
// c * 0.0 is exact, so the fused result is the rounded sum s + c, or s itself (s + -0.0 = s, and a sum that starts at +0.0 never becomes
// -0.0): the bits of the stated add, at a third of the VALU work of two selects and an add.  Likewise fma(c, b ? -1.0 : 1.0, s).  The
// one difference needs a non-finite c (a NaN or an infinity under a set mask byte): 0.0 * c is NaN where the select gives 0.0 -- but then
// S or Q is not finite either and t is NaN on both routes.
template <int MODE, bool MASKED>
__global__ void __launch_bounds__(kT) permutation_t_kernel(Prepared in, const unsigned char* __restrict__ mask, const unsigned* __restrict__ bits,
                                                           long long N, long long V, long long W, long long p0, long long p1,
                                                           unsigned groups, double* __restrict__ tile) {
    const long long v = (long long)(blockIdx.x / groups) * kT + threadIdx.x;
    const long long vc = v < V ? v : V - 1;
    const long long r0 = p0 + (long long)(blockIdx.x % groups) * kR;
    const int rows = (int)(p1 - r0 < kR ? p1 - r0 : kR);
    double s1[kR], q1[kR];
    int n1[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) { s1[r] = 0.0; q1[r] = 0.0; n1[r] = 0; }
    for (long long wi = 0; wi < W; ++wi) {
        unsigned w[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r) w[r] = r < rows ? bits[(r0 + r) * W + wi] : 0u;
        const long long i0 = wi * 32;
        const int jn = (int)(N - i0 < 32 ? N - i0 : 32);
#pragma unroll 4
        for (int j = 0; j < jn; ++j) {
            const long long at = (i0 + j) * V + vc;
            const double c = in.C[at];
            if (MODE == OAI_STATS_TWO_SAMPLE) {
                const double q = in.Qm[at];
                const int m = MASKED ? (mask[at] != 0 ? -1 : 0) : -1;          // all ones or none: the count adds b & m
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const unsigned b = (w[r] >> j) & 1u;
                    const double f = __hiloint2double((int)(b * 0x3ff00000u), 0);          // 1.0 or 0.0, built in scalar registers
                    s1[r] = __builtin_fma(c, f, s1[r]);
                    q1[r] = __builtin_fma(q, f, q1[r]);
                    n1[r] += (int)b & m;
                }
            } else {
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const double f = __hiloint2double((int)(0x3ff00000u | ((w[r] >> j) << 31)), 0);      // -1.0 or 1.0
                    s1[r] = __builtin_fma(c, f, s1[r]);
                }
            }
        }
    }
    if (v >= V) return;
    const int n = in.n[v];
    const double nd = (double)n, S = in.S[v], Q = in.Q[v];
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        if (r >= rows) continue;
        double t;
        bool ok;
        if (MODE == OAI_STATS_TWO_SAMPLE) {
            const int n2 = n - n1[r];
            const double n1d = (double)n1[r], n2d = (double)n2;
            const double S1 = s1[r], Q1 = q1[r], S2 = S - S1, Q2 = Q - Q1;
            const double ss = (Q1 - S1 * S1 / n1d) + (Q2 - S2 * S2 / n2d);
            const double sp2 = ss / (double)(n - 2);
            t = (S1 / n1d - S2 / n2d) / sqrt(sp2 * (1.0 / n1d + 1.0 / n2d));
            ok = n1[r] >= 2 && n2 >= 2 && sp2 > 0.0;
        } else {
            const double Sf = s1[r];
            const double var = (Q - Sf * Sf / nd) / (double)(n - 1);
            t = (Sf / nd) / sqrt(var / nd);
            ok = n >= 2 && var > 0.0;
        }
        tile[((r0 - p0) + r) * V + v] = ok ? t : (double)NAN;
    }
}

// ---- oai_permutation_reduce ------------------------------------------------------------------------------------------------------------
struct MaxAcc {
    double v[1];
    __device__ __forceinline__ void clear() { v[0] = 0.0; }
    __device__ __forceinline__ void merge(const double* o) { v[0] = fmax(v[0], o[0]); }
};

struct ReduceWs {
    double* partials;
    long long blocks;
    size_t bytes;
    ReduceWs(const void* base, long long rows, long long V) {
        Ws ws(base);
        blocks = (long long)grid_stride_blocks(V, kT * 4, kMaxBlocks);
        partials = ws.take<double>((size_t)(rows * blocks));
        bytes = ws.off;
    }
};

// grid (blocks, rows): an exact maximum of non-negative numbers, so the walk's order does not matter; NaN (no valid t) is skipped
__global__ void __launch_bounds__(kT) row_max_partials_kernel(const double* __restrict__ tile, long long V, double* __restrict__ partials) {
    __shared__ double lds[kT / 64][1];
    const double* row = tile + (long long)blockIdx.y * V;
    MaxAcc acc;
    acc.clear();
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < V; i += (long long)gridDim.x * kT) {
        const double a = fabs(row[i]);
        if (a == a) acc.v[0] = fmax(acc.v[0], a);
    }
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0) partials[(long long)blockIdx.y * gridDim.x + blockIdx.x] = acc.v[0];
}

__global__ void __launch_bounds__(kT) row_max_finish_kernel(const double* __restrict__ partials, long long nb, double* __restrict__ max_abs) {
    __shared__ double lds[kT / 64][1];
    MaxAcc acc;
    reduce_slots<kT>(partials + (long long)blockIdx.x * nb, nb, acc);
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0) max_abs[blockIdx.x] = acc.v[0];
}

// one thread per vertex: the batch's rows against the observed t.  The batch that holds row 0 records it and starts the count.
__global__ void __launch_bounds__(kT) exceed_kernel(const double* __restrict__ tile, long long V, long long rows, int first, double* __restrict__ t0,
                                                    long long* __restrict__ exceed) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= V) return;
    const double obs = first ? tile[v] : t0[v];
    const double a0 = fabs(obs);
    long long count = 0;
    for (long long r = 0; r < rows; ++r) count += fabs(tile[r * V + v]) >= a0 ? 1 : 0;      // false when either side is NaN
    if (first) t0[v] = obs;
    exceed[v] = first ? count : exceed[v] + count;
}

// ---- oai_graph_clusters ----------------------------------------------------------------------------------------------------------------
struct ClusterWs {
    int *parent, *count;
    size_t bytes;
    ClusterWs(const void* base, long long rows, long long V) {
        Ws ws(base);
        parent = ws.take<int>((size_t)(rows * V));
        count = ws.take<int>((size_t)(rows * V));
        bytes = ws.off;
    }
};

__device__ __forceinline__ int side_of(double t, double t0) { return t > t0 ? 1 : (t < -t0 ? -1 : 0); }      // NaN: 0

// workgroup = one row.  Every vertex of either set hooks to its neighbours of the same set until nothing hooks (csrc/hook_jump.h); then
// every vertex counts itself at its root.
__global__ void __launch_bounds__(kClusterT) graph_clusters_kernel(const double* __restrict__ values, long long V, const int* __restrict__ offsets,
                                                                   const int* __restrict__ neighbours, long long n_nbrs, double t0, int* parent_all,
                                                                   int* count_all, int* __restrict__ max_extent, int* __restrict__ label0,
                                                                   int* __restrict__ size0) {
    __shared__ int largest;
    const double* val = values + (long long)blockIdx.x * V;
    int* parent = parent_all + (long long)blockIdx.x * V;
    int* count = count_all + (long long)blockIdx.x * V;
    const int n = (int)V;
    for (int i = threadIdx.x; i < n; i += kClusterT) {
        __hip_atomic_store(parent + i, side_of(val[i], t0) != 0 ? i : -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(count + i, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) largest = 0;
    __syncthreads();
    hook_jump_rounds<kClusterT>(
        parent, V, offsets, neighbours, n_nbrs,
        [&](int i) { return side_of(val[i], t0); },
        [&](int s, int u) { return side_of(val[u], t0) == s; });
    for (int i = threadIdx.x; i < n; i += kClusterT) {
        const int p = load_agent(parent + i);
        if (p >= 0) atomicAdd(count + p, 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kClusterT) {
        const int p = load_agent(parent + i);
        const int size = p >= 0 ? load_agent(count + p) : 0;
        if (p == i) atomicMax(&largest, size);
        if (blockIdx.x == 0 && label0) label0[i] = p;
        if (blockIdx.x == 0 && size0) size0[i] = size;
    }
    __syncthreads();
    if (threadIdx.x == 0) max_extent[blockIdx.x] = largest;
}

}  // namespace

extern "C" {

size_t oai_group_prepare_workspace_bytes(long long n_knees, long long n_verts) {
    if (!cohort_shape_ok(n_knees, n_verts)) return 0;
    return Prepared(nullptr, n_knees, n_verts).bytes;
}

int oai_group_prepare(const float* y_dev, const unsigned char* mask_dev, long long n_knees, long long n_verts, int centre, void* workspace_dev,
                      size_t workspace_bytes, void* stream) {
    OAI_CHECK_ARG(cohort_shape_ok(n_knees, n_verts), "oai_group_prepare: needs 2 .. 2^24 knees and 1 .. 2^31-2 vertices (got %lld, %lld)", n_knees, n_verts);
    OAI_CHECK_ARG(centre == 0 || centre == 1, "oai_group_prepare: centre must be 0 or 1, got %d", centre);
    OAI_CHECK_ARG(workspace_dev && y_dev, "oai_group_prepare: null pointer");
    OAI_CHECK_WORKSPACE("oai_group_prepare", workspace_bytes, oai_group_prepare_workspace_bytes(n_knees, n_verts));
    const Prepared out(workspace_dev, n_knees, n_verts);
    prepare_kernel<<<cdiv(n_verts, kT), kT, 0, (hipStream_t)stream>>>(y_dev, mask_dev, n_knees, n_verts, centre, out);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_permutation_t_workspace_bytes(long long n_rows, long long n_verts) {
    if (!tile_shape_ok(n_rows, n_verts)) return 0;
    return round256((size_t)n_rows * (size_t)n_verts * sizeof(double));
}

int oai_permutation_t(const void* prepared_dev, size_t prepared_bytes, const unsigned char* mask_dev, const unsigned* bits_dev, long long n_knees,
                      long long n_verts, long long p0, long long p1, int mode, void* workspace_dev, size_t workspace_bytes, void* stream) {
    OAI_CHECK_ARG(cohort_shape_ok(n_knees, n_verts), "oai_permutation_t: needs 2 .. 2^24 knees and 1 .. 2^31-2 vertices (got %lld, %lld)", n_knees, n_verts);
    OAI_CHECK_ARG(p0 >= 0 && p1 > p0 && p1 - p0 <= kMaxRows, "oai_permutation_t: rows [p0, p1) must hold 1 .. 2^20 rows from p0 >= 0 (got %lld, %lld)", p0, p1);
    OAI_CHECK_ARG(mode == OAI_STATS_TWO_SAMPLE || mode == OAI_STATS_ONE_SAMPLE, "oai_permutation_t: mode must be 0 (two-sample) or 1 (one-sample), got %d", mode);
    OAI_CHECK_ARG(prepared_dev && bits_dev && workspace_dev, "oai_permutation_t: null pointer");
    OAI_CHECK_WORKSPACE("oai_permutation_t (prepared block)", prepared_bytes, oai_group_prepare_workspace_bytes(n_knees, n_verts));
    OAI_CHECK_WORKSPACE("oai_permutation_t", workspace_bytes, oai_permutation_t_workspace_bytes(p1 - p0, n_verts));
    const Prepared in(prepared_dev, n_knees, n_verts);
    const unsigned groups = cdiv(p1 - p0, kR);
    const long long blocks = (long long)cdiv(n_verts, kT) * groups;
    OAI_CHECK_ARG(blocks < (1LL << 31), "oai_permutation_t: %lld rows of %lld vertices are more than one launch takes: use smaller batches", p1 - p0, n_verts);
    const unsigned grid = (unsigned)blocks;
    const long long W = (n_knees + 31) / 32;
    const hipStream_t st = (hipStream_t)stream;
    double* tile = (double*)workspace_dev;
    if (mode == OAI_STATS_ONE_SAMPLE)
        permutation_t_kernel<OAI_STATS_ONE_SAMPLE, false><<<grid, kT, 0, st>>>(in, nullptr, bits_dev, n_knees, n_verts, W, p0, p1, groups, tile);
    else if (mask_dev)
        permutation_t_kernel<OAI_STATS_TWO_SAMPLE, true><<<grid, kT, 0, st>>>(in, mask_dev, bits_dev, n_knees, n_verts, W, p0, p1, groups, tile);
    else
        permutation_t_kernel<OAI_STATS_TWO_SAMPLE, false><<<grid, kT, 0, st>>>(in, nullptr, bits_dev, n_knees, n_verts, W, p0, p1, groups, tile);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_permutation_reduce_workspace_bytes(long long n_rows, long long n_verts) {
    if (!tile_shape_ok(n_rows, n_verts)) return 0;
    return ReduceWs(nullptr, n_rows, n_verts).bytes;
}

int oai_permutation_reduce(const double* tile_dev, long long n_verts, long long p0, long long p1, void* workspace_dev, size_t workspace_bytes,
                           double* t0_dev, double* max_abs_dev, long long* exceed_dev, void* stream) {
    OAI_CHECK_ARG(n_verts >= 1 && n_verts <= kMaxVerts, "oai_permutation_reduce: needs 1 .. 2^31-2 vertices (got %lld)", n_verts);
    OAI_CHECK_ARG(p0 >= 0 && p1 > p0 && p1 - p0 <= kMaxRows, "oai_permutation_reduce: rows [p0, p1) must hold 1 .. 2^20 rows from p0 >= 0 (got %lld, %lld)", p0, p1);
    OAI_CHECK_ARG(workspace_dev && max_abs_dev && tile_dev && t0_dev && exceed_dev, "oai_permutation_reduce: null pointer");
    OAI_CHECK_WORKSPACE("oai_permutation_reduce", workspace_bytes, oai_permutation_reduce_workspace_bytes(p1 - p0, n_verts));
    const long long rows = p1 - p0;
    const ReduceWs ws(workspace_dev, rows, n_verts);
    const hipStream_t st = (hipStream_t)stream;
    row_max_partials_kernel<<<dim3((unsigned)ws.blocks, (unsigned)rows), kT, 0, st>>>(tile_dev, n_verts, ws.partials);
    OAI_CHECK_LAUNCH();
    row_max_finish_kernel<<<(unsigned)rows, kT, 0, st>>>(ws.partials, ws.blocks, max_abs_dev + p0);
    OAI_CHECK_LAUNCH();
    exceed_kernel<<<cdiv(n_verts, kT), kT, 0, st>>>(tile_dev, n_verts, rows, p0 == 0 ? 1 : 0, t0_dev, exceed_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_graph_clusters_workspace_bytes(long long n_rows, long long n_verts) {
    if (!tile_shape_ok(n_rows, n_verts)) return 0;
    return ClusterWs(nullptr, n_rows, n_verts).bytes;
}

int oai_graph_clusters(const double* values_dev, long long n_rows, long long n_verts, const int* offsets_dev, const int* neighbours_dev,
                       long long n_neighbours, double t0, void* workspace_dev, size_t workspace_bytes, int* max_extent_dev, int* label0_dev,
                       int* size0_dev, void* stream) {
    OAI_CHECK_GRAPH_TILE("oai_graph_clusters", n_rows, n_verts, n_neighbours);
    OAI_CHECK_ARG(t0 > 0.0, "oai_graph_clusters: the threshold must be > 0 (got %g)", t0);
    OAI_CHECK_ARG(workspace_dev && max_extent_dev && values_dev && offsets_dev && (n_neighbours == 0 || neighbours_dev),
                  "oai_graph_clusters: null pointer");
    OAI_CHECK_WORKSPACE("oai_graph_clusters", workspace_bytes, oai_graph_clusters_workspace_bytes(n_rows, n_verts));
    const ClusterWs ws(workspace_dev, n_rows, n_verts);
    graph_clusters_kernel<<<(unsigned)n_rows, kClusterT, 0, (hipStream_t)stream>>>(values_dev, n_verts, offsets_dev, neighbours_dev, n_neighbours, t0,
                                                                                  ws.parent, ws.count, max_extent_dev, label0_dev, size0_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
