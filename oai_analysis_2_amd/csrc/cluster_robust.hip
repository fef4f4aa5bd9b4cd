// Cluster-robust regression for gfx950 (include/oai_hip.h, "Cluster-robust regression"; tests/cluster_robust_ref.py restates this file
// operation for operation): the marginal model of repeated measures -- ordinary least squares over all rows (knee-visits), the sandwich
// variance that sums scores within a cluster (subject), and the restricted wild cluster bootstrap, which flips the sign of every
// cluster's null-model residuals as a block.
//   oai_cluster_prepare   appends to the block of oai_regression_prepare: per vertex the factor L of M = D^T D over the valid rows, and per
//                         (cluster, vertex) the sums H (D^T r), K (D^T w) and U (w . r), w = D M^-1 e_p; G, the CR1 factor c, okc
//   oai_cluster_t         a batch of packed flip rows -> one sandwich t per (row, vertex); row 0 also the slope and its standard error
// The tile feeds oai_permutation_reduce, oai_graph_clusters and oai_graph_tfce as it is.
//
// fp64 without contraction; the order IS the contract, as in csrc/group_regression.hip: every sum over rows or clusters in ascending
// index with one accumulator in one thread that starts at +0.0; cholesky<P>, forward_solve<P> and backward_solve<P> are those of
// csrc/regression_solve.h.  No floating-point atomics.
//
// Shape of the t kernel.  As permutation_t_kernel and regression_rows: a thread owns one vertex x R flip rows, a wave64 covers 64
// consecutive vertices, 256-thread blocks, the row groups of a vertex span next to each other in a one-dimensional grid (they re-read
// the span's H, K and U planes while the L2 holds them), no LDS.  A flip word is the same for the whole wave: its address is made of
// kernel arguments, blockIdx and loop counters only, so it is a scalar load and the sign factor is built in scalar registers.
//   Two passes over the clusters, the direct form the header states.  Pass 1: b_c = sum_s +-h_sc, issued as fma(h, +-1.0, b) -- the
//     product is exact, so these are the bits of the stated add (csrc/group_stats.hip has the argument) -- p operations per (row,
//     cluster) against p loads of 8 bytes per cluster, shared by the R rows.  Then the two triangular solves in registers, L from its
//     planes.  Pass 2: e = +-u - k_0 beta_0 issued as fma(u, +-1.0, -(k_0*beta_0)), exact for the same reason, then for c >= 1 a
//     multiply and a subtract each, then the multiply and the add of W: 2 p + 1 operations per (row, cluster) against p + 1 loads.
//   Together 3 p + 1 fp64 operations per (row, cluster, vertex) and (2 p + 1) 8 bytes per (cluster, vertex) and R rows.  R is chosen
//     per p by measurement; the accumulators are R p doubles (b, then beta in their place) and R more for W:
//         p        1      2      3      4      5      6
//         R       16     16     16     16      8      8
//     VGPRs / waves per SIMD from the compiler's kernel-resource remarks on the gfx950 build; scratch is 0 for all six (a condition):
//               104/4  156/3  202/2  244/2  165/3  211/2
//     Measured at V = 30 002, 1000 flip rows, ms (profiles/cluster_robust.md has the spreads), S = 200 / S = 2000, the chosen R first:
//       p = 4    R = 16: 3.98 / 37.9     8: 4.35 / 51.4     4: 6.31 / 128     32: 10.6 / 101 (636 bytes of scratch per lane)
//       p = 6    R =  8: 6.19 / 66.5     4: 8.86 / 194      2: 16.6 / 347     16: 8.62 / 86.0 (256 VGPRs, one wave per SIMD)
//     With few rows per thread the kernel sits on the memory side: at half the first table the threads read 17 .. 19 TB/s at S = 200
//     (the L2s) and 8.4 .. 9.0 TB/s at S = 2000 (beyond them), and every doubling of R took that traffic away one for one.  At the
//     chosen R it reads 6.8 .. 12.8 TB/s and runs at 44 .. 53 % of the fp64 vector issue rate with two waves per SIMD, about where
//     the masked oai_regression_t sits (56 % at p = 4, 47 % at p = 6).  p = 1, 2, 3 and 5 were not measured: 3 and 5 take the R of
//     their neighbours, 1 and 2 the sixteen rows of permutation_t_kernel.  A block of 64 vertices x 4 row groups, one per wave, so
//     that three of four waves would hit the CU's L1, was measured too and changed nothing (3.9 .. 4.2 / 38.2 and 6.9 / 65.3): it is
//     not in the source.  The result does not depend on R or on the batch.
// The prepare kernels stream over the rows with one thread per vertex, as prepare_kernel of csrc/group_regression.hip does.  Without a
// mask M, L, a, w and K do not depend on the vertex: uniform_kernel forms them once, in the stated order, and the per-vertex kernel
// copies them into the planes, so oai_cluster_t has one path and a null mask gives the bits of a mask of ones.
#include "cohort.h"

#include <cmath>

#pragma clang fp contract(off)

#include "regression_rows.h"

namespace {

using namespace oai;

constexpr int kT = 256;                            // vertices of a block
constexpr long long kMaxClusterRows = 1LL << 20;   // rows (knee-visits) of one cohort

#if defined(OAI_DIAG) && defined(OAI_CLUSTER_ROWS_SHIFT)    // diagnostic builds only: the table below doubled (1) or halved (-1), to measure against
constexpr int kRowsShift = OAI_CLUSTER_ROWS_SHIFT;
#else
constexpr int kRowsShift = 0;
#endif

__host__ __device__ constexpr int rows_per_thread(int p) {
    const int r = p <= 4 ? 16 : 8;
    return kRowsShift > 0 ? r << kRowsShift : (r >> -kRowsShift) > 0 ? r >> -kRowsShift : 1;
}

// ---- the cluster block: that of "Cohort regression", then the arrays of "Cluster-robust regression" ------------------------------------
struct ClusterBlock {
    Prepared head;
    double *H, *K, *U, *L, *c;
    int* G;
    unsigned char* okc;
    double *wu, *ku, *fu;                          // without a mask only: w [n_rows], K [p][S], and L, 1.0 / 0.0 = every pivot passed, a
    size_t bytes;
    ClusterBlock(const void* base, long long N, long long V, long long S, int p) : head(base, N, V) {
        Ws ws(base);
        ws.off = head.bytes;
        H = ws.take<double>((size_t)p * (size_t)(S * V));
        K = ws.take<double>((size_t)p * (size_t)(S * V));
        U = ws.take<double>((size_t)(S * V));
        L = ws.take<double>((size_t)tri(p) * (size_t)V);
        c = ws.take<double>((size_t)V);
        G = ws.take<int>((size_t)V);
        okc = ws.take<unsigned char>((size_t)V);
        wu = ws.take<double>((size_t)N);
        ku = ws.take<double>((size_t)p * (size_t)S);
        fu = ws.take<double>((size_t)(tri(p) + 1 + p));
        bytes = ws.off;
    }
};

static inline bool cluster_shape_ok(long long N, long long V, long long S, int p) {
    return S >= 2 && N >= S && N <= kMaxClusterRows && V >= 1 && V <= kMaxVerts && p >= 1 && p <= kMaxCols;
}

__device__ __forceinline__ long long clamp_offset(int o, long long N) { return o < 0 ? 0 : (o > N ? N : (long long)o); }

// a = M^-1 e_p from the factor: L z = e_p forward, L^T a = z backward
template <int P>
__device__ __forceinline__ void last_column_of_inverse(const double* L, double* a) {
#pragma unroll
    for (int k = 0; k < P; ++k) a[k] = k == P - 1 ? 1.0 : 0.0;
    forward_solve<P>(L, a);
    backward_solve<P>(L, a);
}

// Without a mask, one block: M entry by entry (one thread each, rows ascending), its factor and a (thread 0), w row by row, K entry by
// entry (rows of the cluster ascending).  What a thread wrote before a barrier the block reads after it.
template <int P>
__global__ void __launch_bounds__(kT) uniform_kernel(const double* __restrict__ D, const int* __restrict__ offsets, long long N, long long S,
                                                     ClusterBlock out) {
    constexpr int T = tri(P);
    __shared__ double Ms[T], av[P];
    const int tid = threadIdx.x;
    if (tid < T) {
        int a = 0;
        while (tri(a + 1) <= tid) ++a;
        const int c = tid - tri(a);
        double s = 0.0;
        for (long long j = 0; j < N; ++j) s = s + D[j * P + a] * D[j * P + c];
        Ms[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double L[T], a[P];
#pragma unroll
        for (int k = 0; k < T; ++k) L[k] = Ms[k];
        const bool pass = cholesky<P>(L);
        last_column_of_inverse<P>(L, a);
#pragma unroll
        for (int k = 0; k < T; ++k) out.fu[k] = L[k];
        out.fu[T] = pass ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            out.fu[T + 1 + k] = a[k];
            av[k] = a[k];
        }
    }
    __syncthreads();
    for (long long j = tid; j < N; j += kT) {
        double w = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) w = w + D[j * P + c] * av[c];
        out.wu[j] = w;
    }
    __syncthreads();
    for (long long at = tid; at < S * P; at += kT) {
        const long long s = at / P;
        const int c = (int)(at - s * P);
        const long long lo = clamp_offset(offsets[s], N), hi = clamp_offset(offsets[s + 1], N);
        double k = 0.0;
        for (long long j = lo; j < hi; ++j) k = k + out.wu[j] * D[j * P + c];
        out.ku[c * S + s] = k;
    }
}

// one thread per vertex: M and its factor over the valid rows (MASKED) or the uniform ones, then the sums of every cluster, rows ascending
template <int P, bool MASKED>
__global__ void __launch_bounds__(kT) cluster_prepare_kernel(const unsigned char* __restrict__ mask, const double* __restrict__ D,
                                                             const int* __restrict__ offsets, long long N, long long V, long long S,
                                                             ClusterBlock out) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= V) return;
    constexpr int T = tri(P);
    double L[T], a[P];
    bool pass;
    if (MASKED) {
#pragma unroll
        for (int k = 0; k < T; ++k) L[k] = 0.0;
        for (long long j = 0; j < N; ++j) {
            const bool m = mask[j * V + v] != 0;
#pragma unroll
            for (int r = 0; r < P; ++r) {
#pragma unroll
                for (int c = 0; c <= r; ++c) {
                    const double dd = D[j * P + r] * D[j * P + c];
                    L[tri(r) + c] = L[tri(r) + c] + (m ? dd : 0.0);
                }
            }
        }
        pass = cholesky<P>(L);
        last_column_of_inverse<P>(L, a);
    } else {
#pragma unroll
        for (int k = 0; k < T; ++k) L[k] = out.fu[k];
        pass = out.fu[T] != 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) a[k] = out.fu[T + 1 + k];
    }
#pragma unroll
    for (int k = 0; k < T; ++k) out.L[k * V + v] = L[k];
    const long long plane = S * V;
    int G = 0;
    for (long long s = 0; s < S; ++s) {
        const long long lo = clamp_offset(offsets[s], N), hi = clamp_offset(offsets[s + 1], N);
        double h[P], k[P], u = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            h[c] = 0.0;
            k[c] = 0.0;
        }
        bool present = false;
        for (long long j = lo; j < hi; ++j) {
            const bool m = MASKED ? mask[j * V + v] != 0 : true;
            const double r = out.head.R[j * V + v];
            double w;
            if (MASKED) {
                double s2 = 0.0;
#pragma unroll
                for (int c = 0; c < P; ++c) s2 = s2 + D[j * P + c] * a[c];
                w = m ? s2 : 0.0;
            } else {
                w = out.wu[j];
            }
            present = present || m;
#pragma unroll
            for (int c = 0; c < P; ++c) {
                const double d = D[j * P + c];
                const double dr = d * r;
                h[c] = h[c] + (m ? dr : 0.0);
                if (MASKED) {
                    const double wd = w * d;
                    k[c] = k[c] + (m ? wd : 0.0);
                }
            }
            const double wr = w * r;
            u = u + (m ? wr : 0.0);
        }
#pragma unroll
        for (int c = 0; c < P; ++c) {
            out.H[c * plane + s * V + v] = h[c];
            out.K[c * plane + s * V + v] = MASKED ? k[c] : out.ku[c * S + s];
        }
        out.U[s * V + v] = u;
        G += present ? 1 : 0;
    }
    const int n = out.head.n[v];
    out.G[v] = G;
    out.c[v] = ((double)G / (double)(G - 1)) * ((double)(n - 1) / (double)(n - P));
    out.okc[v] = out.head.ok[v] != 0 && pass && G >= 2 && n - P >= 1 ? 1 : 0;
}

// ---- oai_cluster_t ---------------------------------------------------------------------------------------------------------------------
// Block b of a one-dimensional grid is row group b % groups of vertex span b / groups.  Thread = one vertex x R flip rows; a lane past V
// works on vertex V - 1 and stores nothing; a row past the batch takes flip word 0 and is not stored.
template <int P>
__global__ void __launch_bounds__(kT) cluster_t_kernel(ClusterBlock in, const unsigned* __restrict__ bits, long long V, long long S, long long Wd,
                                                       long long p0, long long p1, unsigned groups, int first, double* __restrict__ tile,
                                                       double* __restrict__ slope0, double* __restrict__ se0) {
    constexpr int R = rows_per_thread(P);
    constexpr int T = tri(P);
    const long long v = (long long)(blockIdx.x / groups) * kT + threadIdx.x;
    const long long vc = v < V ? v : V - 1;
    const long long r0 = p0 + (long long)(blockIdx.x % groups) * R;
    const int rows = (int)(p1 - r0 < R ? p1 - r0 : R);
    const long long plane = S * V;
    double b[R][P], W[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        W[r] = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) b[r][c] = 0.0;
    }
    // pass 1: b = sum_s +-h_s
    for (long long wi = 0; wi < Wd; ++wi) {
        unsigned w[R];
#pragma unroll
        for (int r = 0; r < R; ++r) w[r] = r < rows ? bits[(r0 + r) * Wd + wi] : 0u;
        const long long s0 = wi * 32;
        const int jn = (int)(S - s0 < 32 ? S - s0 : 32);
#pragma unroll 2
        for (int j = 0; j < jn; ++j) {
            const long long at = (s0 + j) * V + vc;
            double h[P];
#pragma unroll
            for (int c = 0; c < P; ++c) h[c] = in.H[c * plane + at];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double f = __hiloint2double((int)(0x3ff00000u | ((w[r] >> j) << 31)), 0);      // -1.0 or 1.0
#pragma unroll
                for (int c = 0; c < P; ++c) b[r][c] = __builtin_fma(h[c], f, b[r][c]);
            }
        }
    }
    // L z = b, L^T beta = z
    {
        double L[T];
#pragma unroll
        for (int k = 0; k < T; ++k) L[k] = in.L[k * V + vc];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            forward_solve<P>(L, b[r]);
            backward_solve<P>(L, b[r]);
        }
    }
    // pass 2: W = sum_s e_s^2, e_s = +-u_s - k_s . beta
    for (long long wi = 0; wi < Wd; ++wi) {
        unsigned w[R];
#pragma unroll
        for (int r = 0; r < R; ++r) w[r] = r < rows ? bits[(r0 + r) * Wd + wi] : 0u;
        const long long s0 = wi * 32;
        const int jn = (int)(S - s0 < 32 ? S - s0 : 32);
#pragma unroll 2
        for (int j = 0; j < jn; ++j) {
            const long long at = (s0 + j) * V + vc;
            const double u = in.U[at];
            double k[P];
#pragma unroll
            for (int c = 0; c < P; ++c) k[c] = in.K[c * plane + at];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double f = __hiloint2double((int)(0x3ff00000u | ((w[r] >> j) << 31)), 0);
                const double kb0 = k[0] * b[r][0];
                double e = __builtin_fma(u, f, -kb0);
#pragma unroll
                for (int c = 1; c < P; ++c) e = e - k[c] * b[r][c];
                W[r] = W[r] + e * e;
            }
        }
    }
    if (v >= V) return;
    const double cf = in.c[v];
    const bool okc = in.okc[v] != 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r >= rows) continue;
        const double se = sqrt(cf * W[r]);
        const bool valid = okc && W[r] > 0.0;
        tile[((r0 - p0) + r) * V + v] = valid ? b[r][P - 1] / se : (double)NAN;
        if (first && r0 + r == 0) {
            if (slope0) slope0[v] = valid ? b[r][P - 1] : (double)NAN;
            if (se0) se0[v] = valid ? se : (double)NAN;
        }
    }
}

}  // namespace

extern "C" {

size_t oai_cluster_prepare_workspace_bytes(long long n_rows, long long n_verts, long long n_clusters, int n_columns) {
    if (!cluster_shape_ok(n_rows, n_verts, n_clusters, n_columns)) return 0;
    return ClusterBlock(nullptr, n_rows, n_verts, n_clusters, n_columns).bytes;
}

#define OAI_CHECK_CLUSTER_SHAPE(who)                                                                                                          \
    do {                                                                                                                                      \
        OAI_CHECK_ARG(n_clusters >= 2, who ": needs at least 2 clusters, got %lld", n_clusters);                                              \
        OAI_CHECK_ARG(n_columns >= 1 && n_columns <= kMaxCols, who ": needs 1 .. 6 design columns, got %d", n_columns);                       \
        OAI_CHECK_ARG(n_rows <= kMaxClusterRows, who ": at most 2^20 rows, got %lld", n_rows);                                                \
        OAI_CHECK_ARG(n_rows >= n_clusters, who ": fewer rows than clusters (n_rows %lld < n_clusters %lld)", n_rows, n_clusters);            \
        OAI_CHECK_ARG(n_verts >= 1 && n_verts <= kMaxVerts, who ": needs 1 .. 2^31-2 vertices, got %lld", n_verts);                           \
    } while (0)

int oai_cluster_prepare(const unsigned char* mask_dev, const double* design_dev, const int* offsets_dev, long long n_rows, long long n_verts,
                        long long n_clusters, int n_columns, void* prepared_dev, size_t prepared_bytes, void* stream) {
    OAI_CHECK_CLUSTER_SHAPE("oai_cluster_prepare");
    OAI_CHECK_ARG(design_dev && offsets_dev && prepared_dev, "oai_cluster_prepare: null pointer");
    OAI_CHECK_WORKSPACE("oai_cluster_prepare", prepared_bytes, oai_cluster_prepare_workspace_bytes(n_rows, n_verts, n_clusters, n_columns));
    const ClusterBlock out(prepared_dev, n_rows, n_verts, n_clusters, n_columns);
    const unsigned grid = cdiv(n_verts, kT);
    const hipStream_t st = (hipStream_t)stream;
    switch (n_columns) {
#define OAI_CASE(P)                                                                                                                          \
    case P:                                                                                                                                  \
        if (mask_dev) {                                                                                                                      \
            cluster_prepare_kernel<P, true><<<grid, kT, 0, st>>>(mask_dev, design_dev, offsets_dev, n_rows, n_verts, n_clusters, out);       \
        } else {                                                                                                                             \
            uniform_kernel<P><<<1, kT, 0, st>>>(design_dev, offsets_dev, n_rows, n_clusters, out);                                           \
            OAI_CHECK_LAUNCH();                                                                                                              \
            cluster_prepare_kernel<P, false><<<grid, kT, 0, st>>>(nullptr, design_dev, offsets_dev, n_rows, n_verts, n_clusters, out);       \
        }                                                                                                                                    \
        break;
        OAI_CASE(1) OAI_CASE(2) OAI_CASE(3) OAI_CASE(4) OAI_CASE(5) OAI_CASE(6)
#undef OAI_CASE
    }
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_cluster_t_workspace_bytes(long long n_rows, long long n_verts) {
    if (!tile_shape_ok(n_rows, n_verts)) return 0;
    Ws ws(nullptr);
    ws.take<double>((size_t)(n_rows * n_verts));
    return ws.off;
}

int oai_cluster_t(const void* prepared_dev, size_t prepared_bytes, const unsigned* bits_dev, long long n_rows, long long n_verts,
                  long long n_clusters, int n_columns, long long p0, long long p1, void* workspace_dev, size_t workspace_bytes,
                  double* slope0_dev, double* se0_dev, void* stream) {
    OAI_CHECK_CLUSTER_SHAPE("oai_cluster_t");
    OAI_CHECK_ARG(p0 >= 0 && p1 > p0 && p1 - p0 <= kMaxRows, "oai_cluster_t: flip rows [p0, p1) must hold 1 .. 2^20 rows from p0 >= 0 (got %lld, %lld)", p0,
                  p1);
    OAI_CHECK_ARG(prepared_dev && bits_dev && workspace_dev, "oai_cluster_t: null pointer");
    OAI_CHECK_WORKSPACE("oai_cluster_t (cluster block)", prepared_bytes, oai_cluster_prepare_workspace_bytes(n_rows, n_verts, n_clusters, n_columns));
    OAI_CHECK_WORKSPACE("oai_cluster_t", workspace_bytes, oai_cluster_t_workspace_bytes(p1 - p0, n_verts));
    const ClusterBlock in(prepared_dev, n_rows, n_verts, n_clusters, n_columns);
    const long long Wd = (n_clusters + 31) / 32;
    const hipStream_t st = (hipStream_t)stream;
    double* tile = (double*)workspace_dev;
    const int first = p0 == 0 ? 1 : 0;
    switch (n_columns) {
#define OAI_CASE(P)                                                                                                                          \
    case P: {                                                                                                                                \
        const unsigned groups = cdiv(p1 - p0, rows_per_thread(P));                                                                           \
        const long long blocks = (long long)cdiv(n_verts, kT) * groups;                                                                      \
        OAI_CHECK_ARG(blocks < (1LL << 31), "oai_cluster_t: %lld rows of %lld vertices are more than one launch takes: use smaller batches", \
                      p1 - p0, n_verts);                                                                                                     \
        cluster_t_kernel<P><<<(unsigned)blocks, kT, 0, st>>>(in, bits_dev, n_verts, n_clusters, Wd, p0, p1, groups, first, tile, slope0_dev, \
                                                             se0_dev);                                                                       \
    } break;
        OAI_CASE(1) OAI_CASE(2) OAI_CASE(3) OAI_CASE(4) OAI_CASE(5) OAI_CASE(6)
#undef OAI_CASE
    }
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
