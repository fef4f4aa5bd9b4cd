// Normative deviation for gfx950 (include/oai_hip.h, "Normative deviation"; tests/normative_ref.py restates this file operation for
// operation): score ONE knee against a reference cohort, vertex by vertex, adjusted for covariates.
//   oai_normative_fit        per vertex the linear model y ~ Z gamma over the reference knees that have a value there: gamma, the Cholesky
//                            factor L of Z^T Z, the residual sum of squares, n and ok -- the MODEL BLOCK, component-major
//   oai_normative_score      a batch of rows (knees) -> one z per (row, vertex): the prediction-interval t of a knee that is not in the
//                            fit (loo = 0), or the externally studentised residual of the fit's own row (loo = 1); optionally e in mm
//   oai_deviation_summary    per row of a z tile: the valid count, max |z| and where, min and max, and the vertex count and integer
//                            area of {z < -z0} and of {z > z0}
// The z tile feeds oai_graph_clusters and oai_graph_tfce (rows = knees) as it is.
//
// fp64 without contraction; the order IS the contract, as in csrc/group_stats.hip: every sum over knees runs in ascending knee index with
// one accumulator in one thread, a missing entry is skipped by a select, the Cholesky factor and the triangular solves are the
// regression's own device code (csrc/regression_solve.h).  No floating-point atomics; the summary is made of exact maxima and integer
// sums, so its tree needs no stating beyond the tie rule of the arg max.  Nothing synchronises.
//
// Shapes, and why.
//   fit_kernel: a thread owns one vertex and walks the knees twice (the normal equations, then the residuals), as the prepare kernels
//     do.  That is V threads of parallelism -- 469 waves at V = 30 002 on 1024 SIMDs -- and the walk is a chain of dependent adds per
//     accumulator by contract, so the kernel is bound by the latency of a knee's loads, four knees in flight.  It runs once per model
//     and is NOT split over the knees: a split would change the order of the sums.  Design rows are wave-uniform (scalar loads).
//   score_kernel: a thread owns one vertex x kScoreRows = 8 rows, a wave64 covers 64 consecutive vertices, the row groups of a vertex span
//     lie next to each other in a one-dimensional grid (csrc/group_stats.hip says why).  gamma, L, rss, n and ok of the vertex -- at
//     most 6 + 21 + 1 doubles and two small integers at p = 6 -- are loaded once per group from the component-major block (a wave reads
//     512 contiguous bytes per component) and kept in registers over the group's rows; the row's design g is wave-uniform.  Per (row,
//     vertex) the work is 5 bytes in and 8 or 16 out against p divisions of the forward solve, two or three more and a square root: fp64
//     divisions dominate, which the stated formulas leave no way around (a reciprocal would be other bits).
//   summary: grid (blocks, rows) of partial records, then one block per row that merges them (csrc/ordered_reduce.h's tree, whose order
//     does not matter here).  The number of partials depends on V alone.
// Registers, scratch and times: profiles/normative.md.
#include "cohort.h"

#include <cmath>

#include "ordered_reduce.h"

#pragma clang fp contract(off)

#include "regression_solve.h"

namespace {

using namespace oai;

constexpr int kT = 256;                            // vertices of a block
constexpr int kScoreRows = 8;                      // rows per thread of the score kernel
constexpr double kMinDen = 1e-10;                  // 1 - leverage must exceed it for a leave-one-out score
constexpr long long kSummaryBlocks = 64;           // at most, of a row's partial records
constexpr int kRec = 9;                            // int64 words of a summary record

// ---- the model block: component-major, so that 64 consecutive vertices of one component are 512 contiguous bytes --------------------------
struct Model {
    double *gamma, *L, *rss;
    int* n;
    unsigned char* ok;
    size_t bytes;
    Model(const void* base, long long V, int p) {
        Ws ws(base);
        gamma = ws.take<double>((size_t)p * (size_t)V);
        L = ws.take<double>((size_t)tri(p) * (size_t)V);
        rss = ws.take<double>((size_t)V);
        n = ws.take<int>((size_t)V);
        ok = ws.take<unsigned char>((size_t)V);
        bytes = ws.off;
    }
};

// ---- oai_normative_fit -----------------------------------------------------------------------------------------------------------------
template <int P>
__global__ void __launch_bounds__(kT) fit_kernel(const float* __restrict__ Y, const unsigned char* __restrict__ mask, const double* __restrict__ Z,
                                                 long long N, long long V, Model out) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= V) return;
    constexpr int T = tri(P);
    double A[T], h[P];
    int n = 0;
#pragma unroll
    for (int k = 0; k < T; ++k) A[k] = 0.0;
#pragma unroll
    for (int a = 0; a < P; ++a) h[a] = 0.0;
#pragma unroll 4
    for (long long i = 0; i < N; ++i) {
        const bool m = mask ? mask[i * V + v] != 0 : true;
        const double y = (double)Y[i * V + v];
        n += m ? 1 : 0;
#pragma unroll
        for (int a = 0; a < P; ++a) {
            const double za = Z[i * P + a];
#pragma unroll
            for (int c = 0; c <= a; ++c) {
                const double zz = za * Z[i * P + c];
                A[tri(a) + c] = A[tri(a) + c] + (m ? zz : 0.0);
            }
            const double zy = za * y;
            h[a] = h[a] + (m ? zy : 0.0);
        }
    }
    const bool pass = cholesky<P>(A);
    forward_solve<P>(A, h);                                                    // L w = h
    backward_solve<P>(A, h);                                                   // L^T gamma = w
    double rss = 0.0;
#pragma unroll 4
    for (long long i = 0; i < N; ++i) {
        const bool m = mask ? mask[i * V + v] != 0 : true;
        double e = (double)Y[i * V + v];
#pragma unroll
        for (int a = 0; a < P; ++a) e = e - Z[i * P + a] * h[a];
        const double ee = e * e;
        rss = rss + (m ? ee : 0.0);
    }
#pragma unroll
    for (int a = 0; a < P; ++a) out.gamma[(long long)a * V + v] = h[a];
#pragma unroll
    for (int k = 0; k < T; ++k) out.L[(long long)k * V + v] = A[k];
    out.rss[v] = rss;
    out.n[v] = n;
    out.ok[v] = pass && n - P >= 1 ? 1 : 0;
}

// ---- oai_normative_score ---------------------------------------------------------------------------------------------------------------
// Block b of a one-dimensional grid is row group b % groups of vertex span b / groups.  Thread = one vertex x kScoreRows rows; a row past
// the last ends the thread's loop (uniform over the block).
template <int P, bool LOO>
__global__ void __launch_bounds__(kT) score_kernel(Model in, const float* __restrict__ X, const unsigned char* __restrict__ xmask,
                                                   const double* __restrict__ G, long long rows, long long V, unsigned groups,
                                                   double* __restrict__ tile, double* __restrict__ diff) {
    const long long v = (long long)(blockIdx.x / groups) * kT + threadIdx.x;
    if (v >= V) return;
    const long long r0 = (long long)(blockIdx.x % groups) * kScoreRows;
    constexpr int T = tri(P);
    double gamma[P], L[T];
#pragma unroll
    for (int a = 0; a < P; ++a) gamma[a] = in.gamma[(long long)a * V + v];
#pragma unroll
    for (int k = 0; k < T; ++k) L[k] = in.L[(long long)k * V + v];
    const double rss = in.rss[v];
    const bool ok = in.ok[v] != 0;
    const int dof = in.n[v] - P - (LOO ? 1 : 0);
    const double dofd = (double)dof;
#pragma unroll 2
    for (int r = 0; r < kScoreRows; ++r) {
        const long long k = r0 + r;
        if (k >= rows) break;
        const double* g = G + k * P;
        const bool mx = xmask ? xmask[k * V + v] != 0 : true;
        double e = (double)X[k * V + v];
        double u[P];
#pragma unroll
        for (int a = 0; a < P; ++a) {
            e = e - g[a] * gamma[a];
            u[a] = g[a];
        }
        forward_solve<P>(L, u);                                                // L u = g
        double lev = 0.0;
#pragma unroll
        for (int a = 0; a < P; ++a) lev = lev + u[a] * u[a];
        double s2, se2;
        bool cond = true;
        if (LOO) {
            const double den = 1.0 - lev;
            s2 = (rss - (e * e) / den) / dofd;
            se2 = s2 * den;
            cond = den > kMinDen;
        } else {
            s2 = rss / dofd;
            se2 = s2 * (1.0 + lev);
        }
        const double z = e / sqrt(se2);
        const bool valid = mx && ok && dof >= 1 && s2 > 0.0 && cond;
        tile[k * V + v] = valid ? z : (double)NAN;
        if (diff) diff[k * V + v] = (mx && ok) ? e : (double)NAN;
    }
}

template <int P>
int launch_score(const Model& in, const float* x, const unsigned char* xmask, const double* g, long long rows, long long V, int loo, double* tile,
                 double* diff, hipStream_t st) {
    const unsigned groups = cdiv(rows, kScoreRows);
    const long long blocks = (long long)cdiv(V, kT) * groups;
    OAI_CHECK_ARG(blocks < (1LL << 31), "oai_normative_score: %lld rows of %lld vertices are more than one launch takes: use smaller batches", rows, V);
    if (loo)
        score_kernel<P, true><<<(unsigned)blocks, kT, 0, st>>>(in, x, xmask, g, rows, V, groups, tile, diff);
    else
        score_kernel<P, false><<<(unsigned)blocks, kT, 0, st>>>(in, x, xmask, g, rows, V, groups, tile, diff);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// ---- oai_deviation_summary -------------------------------------------------------------------------------------------------------------
// A record as nine int64 words, so that one tree carries it: [0] valid count, [1] max |z| (the bits of a double >= 0, or of -1.0 while there
// is none), [2] its vertex, [3] min z and [4] max z (bits), [5] count and [6] weight of {z < -z0}, [7] count and [8] weight of {z > z0}.
struct SummaryAcc {
    long long v[kRec];
    __device__ __forceinline__ void clear() {
        v[0] = 0;
        v[1] = __double_as_longlong(-1.0);
        v[2] = 1LL << 40;
        v[3] = __double_as_longlong((double)INFINITY);
        v[4] = __double_as_longlong(-(double)INFINITY);
        v[5] = v[6] = v[7] = v[8] = 0;
    }
    // the larger |z|; at a tie the smaller vertex index
    __device__ __forceinline__ void take_abs(double a, long long at) {
        const double mine = __longlong_as_double(v[1]);
        if (a > mine || (a == mine && at < v[2])) {
            v[1] = __double_as_longlong(a);
            v[2] = at;
        }
    }
    __device__ __forceinline__ void merge(const long long* o) {
        v[0] += o[0];
        take_abs(__longlong_as_double(o[1]), o[2]);
        v[3] = __double_as_longlong(fmin(__longlong_as_double(v[3]), __longlong_as_double(o[3])));
        v[4] = __double_as_longlong(fmax(__longlong_as_double(v[4]), __longlong_as_double(o[4])));
        v[5] += o[5];
        v[6] += o[6];
        v[7] += o[7];
        v[8] += o[8];
    }
};

struct SummaryWs {
    long long* partials;
    long long blocks;
    size_t bytes;
    SummaryWs(const void* base, long long rows, long long V) {
        Ws ws(base);
        blocks = (long long)grid_stride_blocks(V, kT * 4, kSummaryBlocks);
        partials = ws.take<long long>((size_t)(rows * blocks) * kRec);
        bytes = ws.off;
    }
};

// grid (blocks, rows)
__global__ void __launch_bounds__(kT) summary_partials_kernel(const double* __restrict__ tile, long long V, const long long* __restrict__ weight,
                                                              double z0, long long* __restrict__ partials) {
    __shared__ long long lds[kT / 64][kRec];
    const double* row = tile + (long long)blockIdx.y * V;
    SummaryAcc acc;
    acc.clear();
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < V; i += (long long)gridDim.x * kT) {
        const double z = row[i];
        if (z != z) continue;                                                  // no score here
        const long long w = weight ? weight[i] : 1;
        acc.v[0] += 1;
        acc.take_abs(fabs(z), i);
        acc.v[3] = __double_as_longlong(fmin(__longlong_as_double(acc.v[3]), z));
        acc.v[4] = __double_as_longlong(fmax(__longlong_as_double(acc.v[4]), z));
        const bool below = z < -z0, above = z > z0;
        acc.v[5] += below ? 1 : 0;
        acc.v[6] += below ? w : 0;
        acc.v[7] += above ? 1 : 0;
        acc.v[8] += above ? w : 0;
    }
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0) {
        long long* out = partials + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * kRec;
        for (int k = 0; k < kRec; ++k) out[k] = acc.v[k];
    }
}

// one block per row: stats = (max |z|, min z, max z), counts = (valid, arg max, n below, weight below, n above, weight above)
__global__ void __launch_bounds__(kT) summary_finish_kernel(const long long* __restrict__ partials, long long nb, double* __restrict__ stats,
                                                            long long* __restrict__ counts) {
    __shared__ long long lds[kT / 64][kRec];
    SummaryAcc acc;
    reduce_slots<kT>(partials + (long long)blockIdx.x * nb * kRec, nb, acc);
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0) {
        const bool any = acc.v[0] > 0;
        double* s = stats + (long long)blockIdx.x * 3;
        long long* c = counts + (long long)blockIdx.x * 6;
        s[0] = any ? __longlong_as_double(acc.v[1]) : 0.0;
        s[1] = any ? __longlong_as_double(acc.v[3]) : (double)NAN;
        s[2] = any ? __longlong_as_double(acc.v[4]) : (double)NAN;
        c[0] = acc.v[0];
        c[1] = any ? acc.v[2] : -1;
        c[2] = acc.v[5];
        c[3] = acc.v[6];
        c[4] = acc.v[7];
        c[5] = acc.v[8];
    }
}

static inline bool columns_ok(int p) { return p >= 1 && p <= kMaxCols; }

}  // namespace

extern "C" {

size_t oai_normative_fit_workspace_bytes(long long n_verts, int n_columns) {
    if (n_verts < 1 || n_verts > kMaxVerts || !columns_ok(n_columns)) return 0;
    return Model(nullptr, n_verts, n_columns).bytes;
}

int oai_normative_fit(const float* y_dev, const unsigned char* mask_dev, const double* design_dev, long long n_knees, long long n_verts, int n_columns,
                      void* model_dev, size_t model_bytes, void* stream) {
    OAI_CHECK_ARG(cohort_shape_ok(n_knees, n_verts), "oai_normative_fit: needs 2 .. 2^24 knees and 1 .. 2^31-2 vertices (got %lld, %lld)", n_knees, n_verts);
    OAI_CHECK_ARG(columns_ok(n_columns), "oai_normative_fit: needs 1 .. 6 design columns, got %d", n_columns);
    OAI_CHECK_ARG(y_dev && design_dev && model_dev, "oai_normative_fit: null pointer");
    OAI_CHECK_WORKSPACE("oai_normative_fit (model block)", model_bytes, oai_normative_fit_workspace_bytes(n_verts, n_columns));
    const Model out(model_dev, n_verts, n_columns);
    const unsigned grid = cdiv(n_verts, kT);
    const hipStream_t st = (hipStream_t)stream;
    switch (n_columns) {
#define OAI_CASE(P) \
    case P: fit_kernel<P><<<grid, kT, 0, st>>>(y_dev, mask_dev, design_dev, n_knees, n_verts, out); break;
        OAI_CASE(1) OAI_CASE(2) OAI_CASE(3) OAI_CASE(4) OAI_CASE(5) OAI_CASE(6)
#undef OAI_CASE
    }
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_normative_score_workspace_bytes(long long n_rows, long long n_verts) {
    if (!tile_shape_ok(n_rows, n_verts)) return 0;
    return round256((size_t)n_rows * (size_t)n_verts * sizeof(double));
}

int oai_normative_score(const void* model_dev, size_t model_bytes, const float* x_dev, const unsigned char* x_mask_dev, const double* design_rows_dev,
                        long long n_rows, long long n_verts, int n_columns, int loo, void* workspace_dev, size_t workspace_bytes, double* diff_dev,
                        void* stream) {
    OAI_CHECK_ARG(tile_shape_ok(n_rows, n_verts), "oai_normative_score: needs 1 .. 2^20 rows and 1 .. 2^31-2 vertices (got %lld, %lld)", n_rows, n_verts);
    OAI_CHECK_ARG(columns_ok(n_columns), "oai_normative_score: needs 1 .. 6 design columns, got %d", n_columns);
    OAI_CHECK_ARG(loo == 0 || loo == 1, "oai_normative_score: loo must be 0 or 1, got %d", loo);
    OAI_CHECK_ARG(model_dev && x_dev && design_rows_dev && workspace_dev, "oai_normative_score: null pointer");
    OAI_CHECK_WORKSPACE("oai_normative_score (model block)", model_bytes, oai_normative_fit_workspace_bytes(n_verts, n_columns));
    OAI_CHECK_WORKSPACE("oai_normative_score", workspace_bytes, oai_normative_score_workspace_bytes(n_rows, n_verts));
    const Model in(model_dev, n_verts, n_columns);
    const hipStream_t st = (hipStream_t)stream;
    double* tile = (double*)workspace_dev;
    switch (n_columns) {
#define OAI_CASE(P) \
    case P: return launch_score<P>(in, x_dev, x_mask_dev, design_rows_dev, n_rows, n_verts, loo, tile, diff_dev, st);
        OAI_CASE(1) OAI_CASE(2) OAI_CASE(3) OAI_CASE(4) OAI_CASE(5) OAI_CASE(6)
#undef OAI_CASE
    }
    return OAI_OK;
}

size_t oai_deviation_summary_workspace_bytes(long long n_rows, long long n_verts) {
    if (!tile_shape_ok(n_rows, n_verts)) return 0;
    return SummaryWs(nullptr, n_rows, n_verts).bytes;
}

int oai_deviation_summary(const double* tile_dev, long long n_rows, long long n_verts, const long long* weight_dev, double z0, void* workspace_dev,
                          size_t workspace_bytes, double* stats_dev, long long* counts_dev, void* stream) {
    OAI_CHECK_ARG(tile_shape_ok(n_rows, n_verts), "oai_deviation_summary: needs 1 .. 2^20 rows and 1 .. 2^31-2 vertices (got %lld, %lld)", n_rows, n_verts);
    OAI_CHECK_ARG(z0 > 0.0, "oai_deviation_summary: the threshold must be > 0 (got %g)", z0);
    OAI_CHECK_ARG(tile_dev && workspace_dev && stats_dev && counts_dev, "oai_deviation_summary: null pointer");
    OAI_CHECK_WORKSPACE("oai_deviation_summary", workspace_bytes, oai_deviation_summary_workspace_bytes(n_rows, n_verts));
    const SummaryWs ws(workspace_dev, n_rows, n_verts);
    const hipStream_t st = (hipStream_t)stream;
    // grid.y holds at most 65 535 rows: a tile of more goes through in slices
    constexpr long long kSlice = 65535;
    for (long long r0 = 0; r0 < n_rows; r0 += kSlice) {
        const long long r1 = r0 + kSlice < n_rows ? r0 + kSlice : n_rows;
        summary_partials_kernel<<<dim3((unsigned)ws.blocks, (unsigned)(r1 - r0)), kT, 0, st>>>(tile_dev + r0 * n_verts, n_verts, weight_dev, z0,
                                                                                              ws.partials + r0 * ws.blocks * kRec);
        OAI_CHECK_LAUNCH();
    }
    summary_finish_kernel<<<(unsigned)n_rows, kT, 0, st>>>(ws.partials, ws.blocks, stats_dev, counts_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
