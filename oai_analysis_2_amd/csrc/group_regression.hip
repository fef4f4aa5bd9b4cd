// Cohort regression for gfx950 (include/oai_hip.h, "Cohort regression"; tests/group_regression_ref.py restates this file operation for
// operation): per vertex the general linear model y ~ Z gamma + x beta over the knees that have a value there, the t of beta, and its
// null distribution under Freedman-Lane permutation of the design rows.
//   oai_regression_prepare   per vertex: n, mean, the residuals r of the (centred) values on the nuisance columns Z, Q = sum r r, ok
//   oai_regression_t         a batch of index rows -> one t per (row, vertex); row 0 also the slope beta
//   oai_regression_f         ("Cohort F test"; tests/group_f_ref.py) the same batch -> one F of the LAST k design columns, tested jointly,
//                            per (row, vertex); row 0 also their k coefficients.  The hot loop is the t kernel's: after L z = b the extra
//                            sum of squares of the last k columns given those before them is the sum of their z_a^2, so F differs from t in
//                            its epilogue alone (regression_rows<P, MASKED, FSTAT>), and k is a runtime argument of that epilogue.
// The tile feeds oai_permutation_reduce and oai_graph_clusters (csrc/group_stats.hip) as it is.
//
// fp64 without contraction; the order IS the contract, as in csrc/group_stats.hip: every sum over knees runs in ascending knee index
// with one accumulator in one thread, the Cholesky factor is formed column by column with its inner sums in ascending k, and a pivot s
// is accepted iff s > 1e-10 * (the diagonal entry it started from).  No floating-point atomics.
//
// Shape of the t kernel.  As permutation_t_kernel: a thread owns one vertex x R rows, a wave64 covers 64 consecutive vertices, 256-thread
// blocks, the row groups of a vertex span next to each other in a one-dimensional grid, no LDS.  Everything that depends on (row, knee)
// alone is wave-uniform and is read through scalar loads into SGPRs.  What differs:
//   The permuted design is reached through an index, two dependent uniform loads per (row, knee).  gather_kernel takes them out of the
//     hot loop: per batch it writes the table [rows][N][E] of the permuted design rows g (p doubles) and, for the masked path, their
//     p (p + 1) / 2 products G_ac = g_a g_c (formed once, in fp64: exact to restate), E = p + p (p + 1) / 2; the hot kernel then reads E
//     contiguous doubles per (row, knee), whose address is made of kernel arguments, blockIdx and loop counters only.
//   Without a mask M = sum g g^T does not depend on the vertex: row_factor_kernel forms it and its Cholesky factor once per row, in the
//     stated order (the same bits as fma(G, 1.0, M) per thread), the table holds g alone (E = p) and the hot kernel accumulates only
//     b = sum g r: 2 p fp64 operations per (row, knee, vertex) -- a multiply and an add each, b being a product THEN an add -- against
//     2 p + p (p + 1) / 2 with a mask, where M_ac is carried per thread and "M + (m ? G : 0.0)" is issued as fma(G, m ? 1.0 : 0.0, M): the
//     product is exact, so these are the bits of the stated add for every finite design (group_stats.hip has the argument in full).
//   R is chosen per (p, masked) by measurement.  The accumulators are R (p + p (p + 1) / 2) doubles with a mask and R p without:
//         p            1     2     3     4     5     6
//     R   masked      16     8     2     2     1     1         accumulators: 18 .. 40 doubles
//     R   no mask     16    16     8     8     8     8         accumulators: 16 .. 48 doubles
//     VGPRs / waves per SIMD from the compiler's kernel-resource remarks on the gfx950 build; scratch is 0 for all 24 instances:
//       t masked      94/5  126/4  67/7  91/5  76/6  94/5
//       t no mask     62/8  94/5   70/7  94/5  126/4 128/4
//       F masked      94/5  126/4  66/7  90/5  70/7  92/5      the F kernel takes the same R in every instance
//       F no mask     62/8  94/5   78/6  94/5  126/4 128/4
//     With a mask the R x E table doubles of a knee must all sit in SGPRs at once (scalar loads return out of order, so the wave waits
//     for all of them before the first use) and nothing can be loaded ahead within the ~100 SGPRs: a knee's latency is hidden by other
//     waves only.  R = 4 at p = 4 (158 VGPRs, 3 waves) took 6.39 ms for the shape below, R = 2 (5 waves) takes 4.91 ms; R = 2 against
//     R = 1 at p = 6: 12.6 against 10.7 ms.
//   The residual and mask byte are written as a two-knee look-ahead; hipcc keeps the addresses in flight rather than the values, and
//     forcing the values into registers early (an empty asm on them) cost 18 .. 33 % in every instance measured, so it is left to hipcc.
//   The load side is light: 9 bytes per (knee, thread) with a mask and 8 without against R (2 p + p (p + 1) / 2) or 2 R p operations.
//   Measured (profiles/group_regression.md): N = 200, V = 30 002, 1000 rows: p = 4 without a mask 1.81 ms (68 % of the fp64 vector issue
//     rate), with one 4.91 ms (56 %); p = 6 with a mask 10.7 ms (47 %).
// prepare_kernel streams over the knees three times with one thread per vertex, as group_stats.hip's.
#include "cohort.h"

#include <cmath>

#pragma clang fp contract(off)

#include "regression_solve.h"
#include "regression_rows.h"

namespace {

using namespace oai;

constexpr int kT = 256;                            // vertices of a block
// kMaxCols (p), kPivot, tri(), cholesky<P>, forward_solve<P> and backward_solve<P>: csrc/regression_solve.h, which names its users
// Prepared (the prepared block): csrc/regression_rows.h; the epilogue of a row: csrc/regression_epilogue_body.h -- both shared with
// csrc/group_regression_vx.hip.  The 24 instances of the hot kernels were compared before and after the two moved there: the same VGPR,
// SGPR and scratch figures, instance by instance (code-object metadata and the compiler's kernel-resource remarks for gfx950).

__host__ __device__ constexpr int rows_per_thread(int p, bool masked) {
    return masked ? (p == 1 ? 16 : p == 2 ? 8 : p <= 4 ? 2 : 1) : (p <= 2 ? 16 : 8);
}

// one thread per vertex, knees in ascending index: the counted sum; the normal equations of the nuisance columns; the residuals
template <int QN>
__global__ void __launch_bounds__(kT) prepare_kernel(const float* __restrict__ Y, const unsigned char* __restrict__ mask, const double* __restrict__ Z,
                                                     long long N, long long V, int centre, Prepared out) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= V) return;
    const CountedMean counted = counted_mean(Y, mask, N, V, v);
    const int n = counted.n;
    const double mu = counted.mean;
    constexpr int QA = QN > 0 ? QN : 1;
    double A[tri(QA)], h[QA];
    bool pass = true;
    if (QN > 0) {
#pragma unroll
        for (int k = 0; k < tri(QA); ++k) A[k] = 0.0;
#pragma unroll
        for (int a = 0; a < QA; ++a) h[a] = 0.0;
        for (long long i = 0; i < N; ++i) {
            const bool m = mask ? mask[i * V + v] != 0 : true;
            const double y = (double)Y[i * V + v];
            const double d = m ? (centre ? y - mu : y) : 0.0;
#pragma unroll
            for (int a = 0; a < QA; ++a) {
                const double za = Z[i * QN + a];
#pragma unroll
                for (int c = 0; c <= a; ++c) {
                    const double zz = za * Z[i * QN + c];
                    A[tri(a) + c] = A[tri(a) + c] + (m ? zz : 0.0);
                }
                h[a] = h[a] + za * d;
            }
        }
        pass = cholesky<QA>(A);
        forward_solve<QA>(A, h);
        backward_solve<QA>(A, h);                                             // L^T gamma = w
    }
    double q = 0.0;
    for (long long i = 0; i < N; ++i) {
        const bool m = mask ? mask[i * V + v] != 0 : true;
        const double y = (double)Y[i * V + v];
        double s = centre ? y - mu : y;
        if (QN > 0) {
#pragma unroll
            for (int a = 0; a < QA; ++a) s = s - Z[i * QN + a] * h[a];
        }
        const double r = m ? s : 0.0;
        out.R[i * V + v] = r;
        q = q + r * r;
    }
    out.n[v] = n;
    out.mean[v] = mu;
    out.Q[v] = q;
    out.ok[v] = pass && n - (QN + 1) >= 1 ? 1 : 0;
}

// ---- oai_regression_t ------------------------------------------------------------------------------------------------------------------
constexpr int kRowPad = 16;                        // the largest R: the table and the factors hold the batch's rows rounded up to a multiple of R

struct TWs {
    double *tile, *table, *factor;
    size_t bytes;
    TWs(const void* base, long long rows, long long V, long long N, int p) {
        Ws ws(base);
        tile = ws.take<double>((size_t)(rows * V));
        table = ws.take<double>((size_t)((rows + kRowPad - 1) * N) * (size_t)(p + tri(p)));
        factor = ws.take<double>((size_t)(rows + kRowPad - 1) * (size_t)(tri(p) + 1));          // per row: L, then 1.0 / 0.0 = every pivot passed
        bytes = ws.off;
    }
};

// One thread per (knee, row) of the batch, rows padded to `padded` (a row past the last repeats the last): the permuted design row, and
// with a mask its products.  E doubles per entry, KNEE-MAJOR [N][padded][E]: the R rows of a thread of the t kernel are then R * E
// contiguous doubles per knee, one run of wide scalar loads.
template <int P, bool MASKED>
__global__ void __launch_bounds__(kT) gather_kernel(const double* __restrict__ D, const int* __restrict__ perm, long long N, long long p0, long long rows,
                                                    long long padded, double* __restrict__ table) {
    constexpr int E = MASKED ? P + tri(P) : P;
    const long long at = (long long)blockIdx.x * kT + threadIdx.x;
    if (at >= padded * N) return;
    const long long j = at / padded, row = at - j * padded;
    long long src = perm[(p0 + (row < rows ? row : rows - 1)) * N + j];
    src = src < 0 ? 0 : (src >= N ? N - 1 : src);
    double g[P];
#pragma unroll
    for (int a = 0; a < P; ++a) g[a] = D[src * P + a];
    double* e = table + at * E;
#pragma unroll
    for (int a = 0; a < P; ++a) e[a] = g[a];
    if (MASKED) {
#pragma unroll
        for (int a = 0; a < P; ++a) {
#pragma unroll
            for (int c = 0; c <= a; ++c) e[P + tri(a) + c] = g[a] * g[c];
        }
    }
}

// without a mask, one thread per (padded) row of the batch: M = sum_j g_j g_j^T, knees ascending, and its factor
template <int P>
__global__ void __launch_bounds__(64) row_factor_kernel(const double* __restrict__ table, long long N, long long padded, double* __restrict__ factor) {
    const long long row = (long long)blockIdx.x * 64 + threadIdx.x;
    if (row >= padded) return;
    double M[tri(P)];
#pragma unroll
    for (int k = 0; k < tri(P); ++k) M[k] = 0.0;
#pragma unroll 4
    for (long long j = 0; j < N; ++j) {
        const double* e = table + (j * padded + row) * P;
        double g[P];
#pragma unroll
        for (int a = 0; a < P; ++a) g[a] = e[a];
#pragma unroll
        for (int a = 0; a < P; ++a) {
#pragma unroll
            for (int c = 0; c <= a; ++c) M[tri(a) + c] = M[tri(a) + c] + g[a] * g[c];
        }
    }
    const bool pass = cholesky<P>(M);
#pragma unroll
    for (int k = 0; k < tri(P); ++k) factor[row * (tri(P) + 1) + k] = M[k];
    factor[row * (tri(P) + 1) + tri(P)] = pass ? 1.0 : 0.0;
}

// Block b of a one-dimensional grid is row group b % groups of vertex span b / groups (group_stats.hip says why).  Thread = one vertex
// x R rows of the batch; a lane past V works on vertex V - 1 and stores nothing; a padded row is worked on and not stored.  Rows here are
// relative to the batch.  The body of both hot kernels: the accumulate loop, the factor and the forward solve are one text, and FSTAT
// picks the epilogue -- the t of the last column (out0: its coefficient), or the F of the last k columns (out0: their k coefficients).
template <int P, bool MASKED, bool FSTAT>
__device__ __forceinline__ void regression_rows(const double* __restrict__ res, const double* __restrict__ Qv, const int* __restrict__ nv,
                                                const unsigned char* __restrict__ okv, const unsigned char* __restrict__ mask,
                                                const double* __restrict__ table, const double* __restrict__ factor, long long N, long long V,
                                                long long rows, long long padded, unsigned groups, int first, int ki, double* __restrict__ tile,
                                                double* __restrict__ out0) {
    constexpr int R = rows_per_thread(P, MASKED);
    constexpr int T = tri(P);
    constexpr int E = MASKED ? P + T : P;
    const long long v = (long long)(blockIdx.x / groups) * kT + threadIdx.x;
    const long long vc = v < V ? v : V - 1;
    const long long r0 = (long long)(blockIdx.x % groups) * R;
    double b[R][P], M[R][MASKED ? T : 1];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int a = 0; a < P; ++a) b[r][a] = 0.0;
        if (MASKED) {
#pragma unroll
            for (int k = 0; k < T; ++k) M[r][k] = 0.0;
        }
    }
    const double* g = table + r0 * E;
    const long long step = padded * E;
    double r1 = res[vc], r2 = res[(N > 1 ? 1 : 0) * V + vc];
    int m1 = MASKED ? mask[vc] : 1, m2 = MASKED ? mask[(N > 1 ? 1 : 0) * V + vc] : 1;
#pragma unroll 1
    for (long long j = 0; j < N; ++j) {
        const double rj = r1;
        const double f = MASKED ? (m1 != 0 ? 1.0 : 0.0) : 1.0;
        const long long ahead = (j + 2 < N ? j + 2 : N - 1) * V + vc;
        r1 = r2;
        m1 = m2;
        r2 = res[ahead];
        if (MASKED) m2 = mask[ahead];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int a = 0; a < P; ++a) b[r][a] = b[r][a] + g[r * E + a] * rj;
            if (MASKED) {
#pragma unroll
                for (int k = 0; k < T; ++k) M[r][k] = __builtin_fma(g[r * E + P + k], f, M[r][k]);
            }
        }
        g += step;
    }
    if (v >= V) return;
    const int dof = nv[v] - P;
    const double Q = Qv[v];
    const bool ok = okv[v] != 0 && dof >= 1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r0 + r >= rows) continue;
        double L[T];
        bool pass;
        if (MASKED) {
#pragma unroll
            for (int k = 0; k < T; ++k) L[k] = M[r][k];
            pass = cholesky<P>(L);
        } else {
            const double* fr = factor + (r0 + r) * (T + 1);
#pragma unroll
            for (int k = 0; k < T; ++k) L[k] = fr[k];
            pass = fr[T] != 0.0;
        }
#include "regression_epilogue_body.h"
    }
}

template <int P, bool MASKED>
__global__ void __launch_bounds__(kT) regression_t_kernel(const double* __restrict__ res, const double* __restrict__ Qv, const int* __restrict__ nv,
                                                          const unsigned char* __restrict__ okv, const unsigned char* __restrict__ mask,
                                                          const double* __restrict__ table, const double* __restrict__ factor, long long N, long long V,
                                                          long long rows, long long padded, unsigned groups, int first, double* __restrict__ tile,
                                                          double* __restrict__ slope0) {
    regression_rows<P, MASKED, false>(res, Qv, nv, okv, mask, table, factor, N, V, rows, padded, groups, first, 1, tile, slope0);
}

// k, 1 <= k <= P, is the caller's to guarantee: coef0 is [k][V] and entry a - (P - k) is column a's.  The four-wave hint keeps every
// instance within the 128 VGPRs of its t twin: without it hipcc spreads the epilogue of <6, no mask> over 166 VGPRs (3 waves); with it
// that instance takes 128 (4 waves) and no instance has scratch, so R stays as rows_per_thread gives it.
template <int P, bool MASKED>
__global__ void __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(4)))
regression_f_kernel(const double* __restrict__ res, const double* __restrict__ Qv, const int* __restrict__ nv, const unsigned char* __restrict__ okv,
                    const unsigned char* __restrict__ mask, const double* __restrict__ table, const double* __restrict__ factor, long long N,
                    long long V, long long rows, long long padded, unsigned groups, int first, int k, double* __restrict__ tile,
                    double* __restrict__ coef0) {
    regression_rows<P, MASKED, true>(res, Qv, nv, okv, mask, table, factor, N, V, rows, padded, groups, first, k, tile, coef0);
}

// the launches of a batch; k = 0: the t kernel (out0 = slope0), k >= 1: the F kernel of the last k columns (out0 = coef0)
template <int P, bool MASKED>
int launch(const char* name, const Prepared& in, const unsigned char* mask, const double* design, const int* perm, long long N, long long V,
           long long p0, long long p1, const TWs& ws, int k, double* out0, hipStream_t st) {
    constexpr int R = rows_per_thread(P, MASKED);
    const long long rows = p1 - p0;
    const unsigned groups = cdiv(rows, R);
    const long long padded = (long long)groups * R;
    const long long blocks = (long long)cdiv(V, kT) * groups;
    OAI_CHECK_ARG(blocks < (1LL << 31) && padded * N < (1LL << 31) * kT,
                  "%s: %lld rows of %lld vertices and %lld knees are more than one launch takes: use smaller batches", name, rows, V, N);
    gather_kernel<P, MASKED><<<cdiv(padded * N, kT), kT, 0, st>>>(design, perm, N, p0, rows, padded, ws.table);
    OAI_CHECK_LAUNCH();
    if (!MASKED) {
        row_factor_kernel<P><<<cdiv(padded, 64), 64, 0, st>>>(ws.table, N, padded, ws.factor);
        OAI_CHECK_LAUNCH();
    }
    if (k == 0)
        regression_t_kernel<P, MASKED><<<(unsigned)blocks, kT, 0, st>>>(in.R, in.Q, in.n, in.ok, mask, ws.table, ws.factor, N, V, rows, padded, groups,
                                                                        p0 == 0 ? 1 : 0, ws.tile, out0);
    else
        regression_f_kernel<P, MASKED><<<(unsigned)blocks, kT, 0, st>>>(in.R, in.Q, in.n, in.ok, mask, ws.table, ws.factor, N, V, rows, padded, groups,
                                                                        p0 == 0 ? 1 : 0, k, ws.tile, out0);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// what oai_regression_t and oai_regression_f share once their own arguments are checked
int run(const char* name, const void* prepared_dev, const unsigned char* mask_dev, const double* design_dev, const int* perm_dev, long long n_knees,
        long long n_verts, int n_columns, long long p0, long long p1, void* workspace_dev, int k, double* out0, void* stream) {
    const Prepared in(prepared_dev, n_knees, n_verts);
    const TWs ws(workspace_dev, p1 - p0, n_verts, n_knees, n_columns);
    const hipStream_t st = (hipStream_t)stream;
    switch (n_columns) {
#define OAI_CASE(P)                                                                                                                      \
    case P:                                                                                                                              \
        return mask_dev ? launch<P, true>(name, in, mask_dev, design_dev, perm_dev, n_knees, n_verts, p0, p1, ws, k, out0, st)           \
                        : launch<P, false>(name, in, nullptr, design_dev, perm_dev, n_knees, n_verts, p0, p1, ws, k, out0, st);
        OAI_CASE(1) OAI_CASE(2) OAI_CASE(3) OAI_CASE(4) OAI_CASE(5) OAI_CASE(6)
#undef OAI_CASE
    }
    return OAI_OK;
}

}  // namespace

extern "C" {

size_t oai_regression_prepare_workspace_bytes(long long n_knees, long long n_verts) {
    if (!cohort_shape_ok(n_knees, n_verts)) return 0;
    return Prepared(nullptr, n_knees, n_verts).bytes;
}

int oai_regression_prepare(const float* y_dev, const unsigned char* mask_dev, const double* nuisance_dev, long long n_knees, long long n_verts,
                           int n_nuisance, int centre, void* prepared_dev, size_t prepared_bytes, void* stream) {
    OAI_CHECK_ARG(cohort_shape_ok(n_knees, n_verts), "oai_regression_prepare: needs 2 .. 2^24 knees and 1 .. 2^31-2 vertices (got %lld, %lld)", n_knees, n_verts);
    OAI_CHECK_ARG(n_nuisance >= 0 && n_nuisance <= kMaxCols - 1, "oai_regression_prepare: needs 0 .. 5 nuisance columns, got %d", n_nuisance);
    OAI_CHECK_ARG(centre == 0 || centre == 1, "oai_regression_prepare: centre must be 0 or 1, got %d", centre);
    OAI_CHECK_ARG(prepared_dev && y_dev && (n_nuisance == 0 || nuisance_dev), "oai_regression_prepare: null pointer");
    OAI_CHECK_WORKSPACE("oai_regression_prepare", prepared_bytes, oai_regression_prepare_workspace_bytes(n_knees, n_verts));
    const Prepared out(prepared_dev, n_knees, n_verts);
    const unsigned grid = cdiv(n_verts, kT);
    const hipStream_t st = (hipStream_t)stream;
    switch (n_nuisance) {
#define OAI_CASE(QN) \
    case QN: prepare_kernel<QN><<<grid, kT, 0, st>>>(y_dev, mask_dev, nuisance_dev, n_knees, n_verts, centre, out); break;
        OAI_CASE(0) OAI_CASE(1) OAI_CASE(2) OAI_CASE(3) OAI_CASE(4) OAI_CASE(5)
#undef OAI_CASE
    }
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_regression_t_workspace_bytes(long long n_rows, long long n_verts, long long n_knees, int n_columns) {
    if (n_rows < 1 || n_rows > kMaxRows || !cohort_shape_ok(n_knees, n_verts) || n_columns < 1 || n_columns > kMaxCols) return 0;
    return TWs(nullptr, n_rows, n_verts, n_knees, n_columns).bytes;
}

int oai_regression_t(const void* prepared_dev, size_t prepared_bytes, const unsigned char* mask_dev, const double* design_dev, const int* perm_dev,
                     long long n_knees, long long n_verts, int n_columns, long long p0, long long p1, void* workspace_dev, size_t workspace_bytes,
                     double* slope0_dev, void* stream) {
    OAI_CHECK_ARG(cohort_shape_ok(n_knees, n_verts), "oai_regression_t: needs 2 .. 2^24 knees and 1 .. 2^31-2 vertices (got %lld, %lld)", n_knees, n_verts);
    OAI_CHECK_ARG(n_columns >= 1 && n_columns <= kMaxCols, "oai_regression_t: needs 1 .. 6 design columns, got %d", n_columns);
    OAI_CHECK_ARG(p0 >= 0 && p1 > p0 && p1 - p0 <= kMaxRows, "oai_regression_t: rows [p0, p1) must hold 1 .. 2^20 rows from p0 >= 0 (got %lld, %lld)", p0, p1);
    OAI_CHECK_ARG(prepared_dev && design_dev && perm_dev && workspace_dev, "oai_regression_t: null pointer");
    OAI_CHECK_WORKSPACE("oai_regression_t (prepared block)", prepared_bytes, oai_regression_prepare_workspace_bytes(n_knees, n_verts));
    OAI_CHECK_WORKSPACE("oai_regression_t", workspace_bytes, oai_regression_t_workspace_bytes(p1 - p0, n_verts, n_knees, n_columns));
    return run("oai_regression_t", prepared_dev, mask_dev, design_dev, perm_dev, n_knees, n_verts, n_columns, p0, p1, workspace_dev, 0, slope0_dev, stream);
}

size_t oai_regression_f_workspace_bytes(long long n_rows, long long n_verts, long long n_knees, int n_columns) {
    return oai_regression_t_workspace_bytes(n_rows, n_verts, n_knees, n_columns);
}

int oai_regression_f(const void* prepared_dev, size_t prepared_bytes, const unsigned char* mask_dev, const double* design_dev, const int* perm_dev,
                     long long n_knees, long long n_verts, int n_columns, int n_interest, long long p0, long long p1, void* workspace_dev,
                     size_t workspace_bytes, double* coef0_dev, void* stream) {
    OAI_CHECK_ARG(cohort_shape_ok(n_knees, n_verts), "oai_regression_f: needs 2 .. 2^24 knees and 1 .. 2^31-2 vertices (got %lld, %lld)", n_knees, n_verts);
    OAI_CHECK_ARG(n_columns >= 1 && n_columns <= kMaxCols, "oai_regression_f: needs 1 .. 6 design columns, got %d", n_columns);
    OAI_CHECK_ARG(n_interest >= 1 && n_interest <= n_columns, "oai_regression_f: needs 1 .. %d columns of interest (n_interest), got %d", n_columns,
                  n_interest);
    OAI_CHECK_ARG(p0 >= 0 && p1 > p0 && p1 - p0 <= kMaxRows, "oai_regression_f: rows [p0, p1) must hold 1 .. 2^20 rows from p0 >= 0 (got %lld, %lld)", p0, p1);
    OAI_CHECK_ARG(prepared_dev && design_dev && perm_dev && workspace_dev, "oai_regression_f: null pointer");
    OAI_CHECK_WORKSPACE("oai_regression_f (prepared block)", prepared_bytes, oai_regression_prepare_workspace_bytes(n_knees, n_verts));
    OAI_CHECK_WORKSPACE("oai_regression_f", workspace_bytes, oai_regression_f_workspace_bytes(p1 - p0, n_verts, n_knees, n_columns));
    return run("oai_regression_f", prepared_dev, mask_dev, design_dev, perm_dev, n_knees, n_verts, n_columns, p0, p1, workspace_dev, n_interest, coef0_dev,
               stream);
}

}  // extern "C"
