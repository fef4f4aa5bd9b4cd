// Vertex-wise design columns for the cohort regression and F test, for gfx950 (include/oai_hip.h, "Vertex-wise design columns";
// tests/vertex_regression_ref.py restates this file operation for operation): the general linear model of csrc/group_regression.hip in
// which S = 1 or 2 of the p design columns are MAPS on the atlas -- one number per (knee, vertex), baseline thickness at the same vertex
// above all -- and not one number per knee.  The design at a vertex is [ vertex nuisance (s_n) | global nuisance | global interest |
// vertex interest (s_i) ], so the position of every per-vertex column is a compile-time constant.
//   oai_regression_vx_prepare   per vertex: the effective (complete-case) mask, n, n_dropped, the completed per-vertex columns WC, and
//                               mean, the residuals r on the nuisance columns, Q = sum r r, ok -- as oai_regression_prepare has them
//   oai_regression_vx_t         a batch of index rows -> one t of the LAST column per (row, vertex); row 0 also its coefficient
//   oai_regression_vx_f         the same batch -> one F of the last k (global) columns per (row, vertex); row 0 also their coefficients
// The tile feeds oai_permutation_reduce, oai_graph_clusters and oai_graph_tfce as it is.
//
// fp64 without contraction; the order IS the contract, as in csrc/group_regression.hip: every sum over knees in ascending knee index with
// one accumulator in one thread; cholesky<P> and forward_solve<P> are those of csrc/regression_solve.h and the epilogue of a row is
// csrc/regression_epilogue_body.h, the text that csrc/group_regression.hip runs.  No floating-point atomics.  (That file's 24 hot-kernel
// instances were compared with their figures before the epilogue and the prepared block moved to shared headers: unchanged.)
//
// Shape of the hot kernel: that of the masked regression_rows.  A thread owns one vertex x R rows, a wave64 covers 64 consecutive
// vertices, 256-thread blocks, the row groups of a vertex span next to each other in a one-dimensional grid, no LDS; everything that
// depends on (row, knee) alone is wave-uniform and is read through scalar loads.  There is no unmasked path: M depends on the vertex.
//   gather_vx_kernel writes, per batch, the table [N][padded rows][E]: the PG = p - S global entries of the dealt design row, their
//     PG (PG + 1) / 2 products (formed once, in fp64), and -- in the last of the E = PG + PG (PG + 1) / 2 + 1 slots, as an int64 -- the
//     clamped index times V: the offset of the dealt knee's row in a plane of WC.  The address of a WC load is then one scalar load
//     away, not two (perm, then the clamp), and that load arrives with the row's design entries.
//   New per (knee, thread): R S loads of 8 bytes, WC[s][idx][v] -- idx is wave-uniform, so the row offset is scalar and the load is
//     coalesced over v -- and S (p + 1) multiplies per row, the products with a per-vertex factor, each rounded once before its fma with
//     m ? 1.0 : 0.0 (the bits of the stated "M + (m ? g g : 0.0)" for every finite design, as in csrc/group_regression.hip).
//   The WC values are written as a one-knee look-ahead beside the two-knee look-ahead of the residual and the mask byte: the loads of
//     knee j + 1 are issued before the arithmetic of knee j.  As there, what hipcc keeps in flight is left to hipcc.
//   R is chosen per (p, S) by measurement, starting from the masked table of csrc/group_regression.hip (16, 8, 2, 2, 1, 1).  The
//     accumulators are R (p + p (p + 1) / 2) doubles and the per-vertex values 2 R S more (this knee's and the next one's):
//         p            1     2     3     4     5     6
//     R   S = 1        8     8     2     2     2     2
//     R   S = 2              4     2     4     2     2
//     VGPRs / waves per SIMD from the compiler's kernel-resource remarks on the gfx950 build; scratch is 0 for all 29 instances (a
//     condition, checked from those remarks):
//       t  s_i = 1, s_n = 0   86/5  126/4  70/7   94/5  122/4  154/3
//       t  s_n = 1, s_i = 0         126/4  70/7   94/5  122/4  154/3       F the same
//       t  s_n = 1, s_i = 1          86/5  70/7  166/3  126/4  166/3
//       t  s_n = 2, s_i = 0                70/7  166/3  126/4  166/3       F the same
//     Measured at N = 200, V = 30 002, 1000 rows, ms (profiles/vertex_covariates.md has the spreads), the chosen R first:
//       p = 1        R = 8: 3.32   16: 3.27    4: 3.60   (8 and 16 within each other's spread; 8 takes 16 VGPRs fewer)
//       p = 2 S = 1  R = 8: 3.42   16: 4.07    4: 3.83
//       p = 4 S = 1  R = 2: 6.44    4: 6.62    1: 7.34
//       p = 4 S = 2  R = 4: 7.13    2: 7.73    1: 9.13
//       p = 6 S = 1  R = 2: 11.8    1: 12.6
//       p = 6 S = 2  R = 2: 11.1    1: 13.0
//     p = 3, p = 5 and (p = 2, S = 2) were not measured: they take the R of their neighbours.  Two rows pay at p = 6 here and not in
//     the masked kernel (12.6 against 10.7 ms there) -- known: the table entry of a (row, knee) is E = 15 or 21 doubles here against 27
//     there, so two rows' entries fit the SGPRs; supposed: that this is the whole reason.
//   The result does not depend on R or on the batch.
// prepare_vx_kernel streams over the knees three times with one thread per vertex, as prepare_kernel does.
#include "cohort.h"

#include <cmath>

#pragma clang fp contract(off)

#include "regression_rows.h"

namespace {

using namespace oai;

constexpr int kT = 256;                            // vertices of a block
constexpr int kMaxVx = 2;                          // S

#if defined(OAI_DIAG) && defined(OAI_VX_ROWS_SHIFT)    // diagnostic builds only: the table below doubled (1) or halved (-1), to measure against
constexpr int kRowsShift = OAI_VX_ROWS_SHIFT;
#else
constexpr int kRowsShift = 0;
#endif

__host__ __device__ constexpr int rows_per_thread(int p, int S) {
    const int r = p == 1 ? 8 : p == 2 ? (S == 1 ? 8 : 4) : p == 4 && S == 2 ? 4 : 2;
    return kRowsShift > 0 ? r << kRowsShift : (r >> -kRowsShift) > 0 ? r >> -kRowsShift : 1;
}

// ---- the prepared block: that of "Cohort regression", then n_dropped, the effective mask and the completed columns ---------------------
struct PreparedVx {
    Prepared head;
    int* n_dropped;
    unsigned char* m;
    double* WC;
    size_t bytes;
    PreparedVx(const void* base, long long N, long long V, int S) : head(base, N, V) {
        Ws ws(base);
        ws.off = head.bytes;
        n_dropped = ws.take<int>((size_t)V);
        m = ws.take<unsigned char>((size_t)(N * V));
        WC = ws.take<double>((size_t)S * (size_t)(N * V));
        bytes = ws.off;
    }
};

// One thread per vertex, knees in ascending index.  SN of the S per-vertex columns are nuisance and come first; QG global ones follow.
template <int SN, int QG>
__global__ void __launch_bounds__(kT) prepare_vx_kernel(const float* __restrict__ Y, const unsigned char* __restrict__ mask, const float* __restrict__ W,
                                                        const unsigned char* __restrict__ wmask, const double* __restrict__ Z, long long N, long long V,
                                                        int S, int centre, PreparedVx out) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= V) return;
    constexpr int QN = SN + QG;
    const long long plane = N * V;
    // the complete cases: their count, what the covariates dropped, the counted sums
    int n = 0, dropped = 0;
    double sum = 0.0, wsum[kMaxVx] = {0.0, 0.0};
    for (long long i = 0; i < N; ++i) {
        const bool my = mask ? mask[i * V + v] != 0 : true;
        bool m = my;
#pragma unroll
        for (int s = 0; s < kMaxVx; ++s) m = m && (s < S && wmask ? wmask[s * plane + i * V + v] != 0 : true);
        n += m ? 1 : 0;
        dropped += my && !m ? 1 : 0;
        sum = sum + (m ? (double)Y[i * V + v] : 0.0);
#pragma unroll
        for (int s = 0; s < kMaxVx; ++s) {
            if (s < S) wsum[s] = wsum[s] + (m ? (double)W[s * plane + i * V + v] : 0.0);
        }
        out.m[i * V + v] = m ? 1 : 0;
    }
    const double mu = sum / (double)n;
    double shift[kMaxVx], fill[kMaxVx];              // what a valid entry loses, and what stands where the covariate itself is missing
#pragma unroll
    for (int s = 0; s < kMaxVx; ++s) {
        const double wbar = wsum[s] / (double)n;
        shift[s] = centre ? wbar : 0.0;
        fill[s] = centre ? 0.0 : wbar;              // a select: a centred missing entry is exactly 0.0
    }
    // the completed columns; the normal equations of the nuisance columns [wc_0 .. | z ..]
    constexpr int QA = QN > 0 ? QN : 1;
    double A[tri(QA)], h[QA];
#pragma unroll
    for (int k = 0; k < tri(QA); ++k) A[k] = 0.0;
#pragma unroll
    for (int a = 0; a < QA; ++a) h[a] = 0.0;
    for (long long i = 0; i < N; ++i) {
        double wc[kMaxVx] = {0.0, 0.0};
#pragma unroll
        for (int s = 0; s < kMaxVx; ++s) {
            if (s < S) {
                const bool mw = wmask ? wmask[s * plane + i * V + v] != 0 : true;
                const double w = (double)W[s * plane + i * V + v];
                wc[s] = n > 0 ? (mw ? w - shift[s] : fill[s]) : 0.0;
                out.WC[s * plane + i * V + v] = wc[s];
            }
        }
        if (QN > 0) {
            const bool m = out.m[i * V + v] != 0;
            const double y = (double)Y[i * V + v];
            const double d = m ? (centre ? y - mu : y) : 0.0;
            double z[QA];
#pragma unroll
            for (int a = 0; a < QA; ++a) z[a] = a < SN ? wc[a < kMaxVx ? a : 0] : Z[i * QG + (a - SN)];
#pragma unroll
            for (int a = 0; a < QA; ++a) {
#pragma unroll
                for (int c = 0; c <= a; ++c) {
                    const double zz = z[a] * z[c];
                    A[tri(a) + c] = A[tri(a) + c] + (m ? zz : 0.0);
                }
                h[a] = h[a] + z[a] * d;
            }
        }
    }
    bool pass = true;
    if (QN > 0) {
        pass = cholesky<QA>(A);
        forward_solve<QA>(A, h);
        backward_solve<QA>(A, h);                                             // h is gamma from here on
    }
    double q = 0.0;
    for (long long i = 0; i < N; ++i) {
        const bool m = out.m[i * V + v] != 0;
        const double y = (double)Y[i * V + v];
        double s = centre ? y - mu : y;
        if (QN > 0) {
#pragma unroll
            for (int a = 0; a < QA; ++a) {
                const double za = a < SN ? out.WC[a * plane + i * V + v] : Z[i * QG + (a - SN)];
                s = s - za * h[a];
            }
        }
        const double r = m ? s : 0.0;
        out.head.R[i * V + v] = r;
        q = q + r * r;
    }
    out.head.n[v] = n;
    out.head.mean[v] = mu;
    out.head.Q[v] = q;
    out.head.ok[v] = pass && n - (QN + 1) >= 1 ? 1 : 0;
    out.n_dropped[v] = dropped;
}

// ---- oai_regression_vx_t, oai_regression_vx_f ------------------------------------------------------------------------------------------
constexpr int kRowPad = 16;                        // the largest R: the table holds the batch's rows rounded up to a multiple of R

__host__ __device__ constexpr int table_entry(int pg) { return pg + tri(pg) + 1; }         // E

struct VxWs {
    double *tile, *table;
    size_t bytes;
    VxWs(const void* base, long long rows, long long V, long long N, int pg) {
        Ws ws(base);
        tile = ws.take<double>((size_t)(rows * V));
        table = ws.take<double>((size_t)((rows + kRowPad - 1) * N) * (size_t)table_entry(pg));
        bytes = ws.off;
    }
};

// One thread per (knee, row) of the batch, rows padded to `padded` (a row past the last repeats the last), KNEE-MAJOR [N][padded][E] as
// gather_kernel of csrc/group_regression.hip writes it: the global entries of the dealt design row, their products, and the offset of the
// dealt knee's row in a plane of WC.
template <int PG>
__global__ void __launch_bounds__(kT) gather_vx_kernel(const double* __restrict__ D, const int* __restrict__ perm, long long N, long long V, long long p0,
                                                       long long rows, long long padded, double* __restrict__ table) {
    constexpr int E = table_entry(PG);
    const long long at = (long long)blockIdx.x * kT + threadIdx.x;
    if (at >= padded * N) return;
    const long long j = at / padded, row = at - j * padded;
    long long src = perm[(p0 + (row < rows ? row : rows - 1)) * N + j];
    src = src < 0 ? 0 : (src >= N ? N - 1 : src);
    double* e = table + at * E;
    if (PG > 0) {
        constexpr int PA = PG > 0 ? PG : 1;
        double g[PA];
#pragma unroll
        for (int a = 0; a < PA; ++a) g[a] = D[src * PG + a];
#pragma unroll
        for (int a = 0; a < PA; ++a) e[a] = g[a];
#pragma unroll
        for (int a = 0; a < PA; ++a) {
#pragma unroll
            for (int c = 0; c <= a; ++c) e[PG + tri(a) + c] = g[a] * g[c];
        }
    }
    e[E - 1] = __longlong_as_double(src * V);
}

// Block b of a one-dimensional grid is row group b % groups of vertex span b / groups; thread = one vertex x R rows of the batch; a lane
// past V works on vertex V - 1 and stores nothing; a padded row is worked on and not stored.  Column a of the design is per-vertex for
// a < SN and, with SI, for a = P - 1 (plane S - 1 of WC); the others are the PG global ones, a - SN of the table entry.
template <int P, int SN, int SI, bool FSTAT>
__device__ __forceinline__ void vx_rows(const double* __restrict__ res, const double* __restrict__ Qv, const int* __restrict__ nv,
                                        const unsigned char* __restrict__ okv, const unsigned char* __restrict__ mask, const double* __restrict__ WC,
                                        const double* __restrict__ table, long long N, long long V, long long rows, long long padded, unsigned groups,
                                        int first, int ki, double* __restrict__ tile, double* __restrict__ out0) {
    constexpr int S = SN + SI, PG = P - S;
    constexpr int R = rows_per_thread(P, S);
    constexpr int T = tri(P);
    constexpr int E = table_entry(PG);
    const long long v = (long long)(blockIdx.x / groups) * kT + threadIdx.x;
    const long long vc = v < V ? v : V - 1;
    const long long r0 = (long long)(blockIdx.x % groups) * R;
    const long long plane = N * V;
    double b[R][P], M[R][T], wn[R][S];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int a = 0; a < P; ++a) b[r][a] = 0.0;
#pragma unroll
        for (int k = 0; k < T; ++k) M[r][k] = 0.0;
    }
    const double* g = table + r0 * E;
    const long long step = padded * E;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long at = __double_as_longlong(g[r * E + E - 1]) + vc;
#pragma unroll
        for (int s = 0; s < S; ++s) wn[r][s] = WC[s * plane + at];
    }
    double r1 = res[vc], r2 = res[(N > 1 ? 1 : 0) * V + vc];
    int m1 = mask[vc], m2 = mask[(N > 1 ? 1 : 0) * V + vc];
#pragma unroll 1
    for (long long j = 0; j < N; ++j) {
        const double rj = r1;
        const double f = m1 != 0 ? 1.0 : 0.0;
        const long long ahead = (j + 2 < N ? j + 2 : N - 1) * V + vc;
        r1 = r2;
        m1 = m2;
        r2 = res[ahead];
        m2 = mask[ahead];
        double w[R][S];
        const double* gn = j + 1 < N ? g + step : g;                             // the last knee looks ahead at itself
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const long long at = __double_as_longlong(gn[r * E + E - 1]) + vc;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                w[r][s] = wn[r][s];
                wn[r][s] = WC[s * plane + at];
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double col[P];
#pragma unroll
            for (int a = 0; a < P; ++a) col[a] = a < SN ? w[r][a < S ? a : 0] : (SI && a == P - 1) ? w[r][S - 1] : g[r * E + (a - SN)];
#pragma unroll
            for (int a = 0; a < P; ++a) b[r][a] = b[r][a] + col[a] * rj;
#pragma unroll
            for (int a = 0; a < P; ++a) {
#pragma unroll
                for (int c = 0; c <= a; ++c) {
                    const bool both_global = c >= SN && !(SI && a == P - 1);      // c <= a: then a is global too
                    const double prod = both_global ? g[r * E + PG + tri(a - SN) + (c - SN)] : col[a] * col[c];
                    M[r][tri(a) + c] = __builtin_fma(prod, f, M[r][tri(a) + c]);
                }
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
#pragma unroll
        for (int k = 0; k < T; ++k) L[k] = M[r][k];
        const bool pass = cholesky<P>(L);
#include "regression_epilogue_body.h"
    }
}

template <int P, int SN, int SI>
__global__ void __launch_bounds__(kT) regression_vx_t_kernel(const double* __restrict__ res, const double* __restrict__ Qv, const int* __restrict__ nv,
                                                             const unsigned char* __restrict__ okv, const unsigned char* __restrict__ mask,
                                                             const double* __restrict__ WC, const double* __restrict__ table, long long N, long long V,
                                                             long long rows, long long padded, unsigned groups, int first, double* __restrict__ tile,
                                                             double* __restrict__ slope0) {
    vx_rows<P, SN, SI, false>(res, Qv, nv, okv, mask, WC, table, N, V, rows, padded, groups, first, 1, tile, slope0);
}

// k, 1 <= k <= P - SN, is the caller's to guarantee: coef0 is [k][V] and entry a - (P - k) is column a's
template <int P, int SN>
__global__ void __launch_bounds__(kT) regression_vx_f_kernel(const double* __restrict__ res, const double* __restrict__ Qv, const int* __restrict__ nv,
                                                             const unsigned char* __restrict__ okv, const unsigned char* __restrict__ mask,
                                                             const double* __restrict__ WC, const double* __restrict__ table, long long N, long long V,
                                                             long long rows, long long padded, unsigned groups, int first, int k,
                                                             double* __restrict__ tile, double* __restrict__ coef0) {
    vx_rows<P, SN, 0, true>(res, Qv, nv, okv, mask, WC, table, N, V, rows, padded, groups, first, k, tile, coef0);
}

// the launches of a batch; k = 0: the t kernel (out0 = slope0), k >= 1: the F kernel of the last k columns (out0 = coef0; SI = 0)
template <int P, int SN, int SI>
int launch(const char* name, const PreparedVx& in, const double* global, const int* perm, long long N, long long V, long long p0, long long p1,
           const VxWs& ws, int k, double* out0, hipStream_t st) {
    constexpr int S = SN + SI, PG = P - S;
    constexpr int R = rows_per_thread(P, S);
    const long long rows = p1 - p0;
    const unsigned groups = cdiv(rows, R);
    const long long padded = (long long)groups * R;
    const long long blocks = (long long)cdiv(V, kT) * groups;
    OAI_CHECK_ARG(blocks < (1LL << 31) && padded * N < (1LL << 31) * kT,
                  "%s: %lld rows of %lld vertices and %lld knees are more than one launch takes: use smaller batches", name, rows, V, N);
    gather_vx_kernel<PG><<<cdiv(padded * N, kT), kT, 0, st>>>(global, perm, N, V, p0, rows, padded, ws.table);
    OAI_CHECK_LAUNCH();
    const Prepared& h = in.head;
    if (k == 0) {
        regression_vx_t_kernel<P, SN, SI><<<(unsigned)blocks, kT, 0, st>>>(h.R, h.Q, h.n, h.ok, in.m, in.WC, ws.table, N, V, rows, padded, groups,
                                                                           p0 == 0 ? 1 : 0, ws.tile, out0);
    } else if constexpr (SI == 0) {
        regression_vx_f_kernel<P, SN><<<(unsigned)blocks, kT, 0, st>>>(h.R, h.Q, h.n, h.ok, in.m, in.WC, ws.table, N, V, rows, padded, groups,
                                                                       p0 == 0 ? 1 : 0, k, ws.tile, out0);
    }
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// what oai_regression_vx_t and oai_regression_vx_f share once their own arguments are checked
int run(const char* name, const void* prepared_dev, const double* global_dev, const int* perm_dev, long long N, long long V, int p, int sn, int si,
        long long p0, long long p1, void* workspace_dev, int k, double* out0, void* stream) {
    const PreparedVx in(prepared_dev, N, V, sn + si);
    const VxWs ws(workspace_dev, p1 - p0, V, N, p - sn - si);
    const hipStream_t st = (hipStream_t)stream;
#define OAI_CASE(P, SN, SI) \
    if (p == P && sn == SN && si == SI) return launch<P, SN, SI>(name, in, global_dev, perm_dev, N, V, p0, p1, ws, k, out0, st);
    OAI_CASE(1, 0, 1) OAI_CASE(2, 0, 1) OAI_CASE(3, 0, 1) OAI_CASE(4, 0, 1) OAI_CASE(5, 0, 1) OAI_CASE(6, 0, 1)      // the map is x
    OAI_CASE(2, 1, 0) OAI_CASE(3, 1, 0) OAI_CASE(4, 1, 0) OAI_CASE(5, 1, 0) OAI_CASE(6, 1, 0)                        // one map adjusts
    OAI_CASE(2, 1, 1) OAI_CASE(3, 1, 1) OAI_CASE(4, 1, 1) OAI_CASE(5, 1, 1) OAI_CASE(6, 1, 1)                        // one adjusts, one is x
    OAI_CASE(3, 2, 0) OAI_CASE(4, 2, 0) OAI_CASE(5, 2, 0) OAI_CASE(6, 2, 0)                                          // two maps adjust
#undef OAI_CASE
    return set_error(OAI_ERR_ARG, "%s: no kernel for %d columns of which %d + %d are per-vertex", name, p, sn, si);
}

#define OAI_VX_CHECK_BATCH(who, p, sn, si)                                                                                                           \
    do {                                                                                                                                             \
        OAI_CHECK_ARG(cohort_shape_ok(n_knees, n_verts), who ": needs 2 .. 2^24 knees and 1 .. 2^31-2 vertices (got %lld, %lld)", n_knees, n_verts); \
        OAI_CHECK_ARG((p) >= 1 && (p) <= kMaxCols, who ": needs 1 .. 6 design columns, got %d", p);                                                  \
        OAI_CHECK_ARG((sn) >= 0 && ((si) == 0 || (si) == 1) && (sn) + (si) >= 1 && (sn) + (si) <= kMaxVx,                                            \
                      who ": needs S = 1 or 2 per-vertex columns, at most one of them of interest (got s_n = %d, s_i = %d)", sn, si);                \
        OAI_CHECK_ARG(p0 >= 0 && p1 > p0 && p1 - p0 <= kMaxRows, who ": rows [p0, p1) must hold 1 .. 2^20 rows from p0 >= 0 (got %lld, %lld)", p0,   \
                      p1);                                                                                                                           \
    } while (0)

}  // namespace

extern "C" {

size_t oai_regression_vx_prepare_workspace_bytes(long long n_knees, long long n_verts, int n_vertex_columns) {
    if (!cohort_shape_ok(n_knees, n_verts) || n_vertex_columns < 1 || n_vertex_columns > kMaxVx) return 0;
    return PreparedVx(nullptr, n_knees, n_verts, n_vertex_columns).bytes;
}

int oai_regression_vx_prepare(const float* y_dev, const unsigned char* mask_dev, const float* w_dev, const unsigned char* wmask_dev,
                              const double* nuisance_dev, long long n_knees, long long n_verts, int n_vertex_nuisance, int n_vertex_interest,
                              int n_global_nuisance, int centre, void* prepared_dev, size_t prepared_bytes, void* stream) {
    const int sn = n_vertex_nuisance, si = n_vertex_interest, qg = n_global_nuisance;
    OAI_CHECK_ARG(cohort_shape_ok(n_knees, n_verts), "oai_regression_vx_prepare: needs 2 .. 2^24 knees and 1 .. 2^31-2 vertices (got %lld, %lld)", n_knees,
                  n_verts);
    OAI_CHECK_ARG(sn >= 0 && (si == 0 || si == 1) && sn + si >= 1 && sn + si <= kMaxVx,
                  "oai_regression_vx_prepare: needs S = 1 or 2 per-vertex columns, at most one of them of interest (got s_n = %d, s_i = %d)", sn, si);
    OAI_CHECK_ARG(qg >= 0 && sn + qg <= kMaxCols - 1, "oai_regression_vx_prepare: needs 0 .. 5 nuisance columns in all, got %d + %d", sn, qg);
    OAI_CHECK_ARG(centre == 0 || centre == 1, "oai_regression_vx_prepare: centre must be 0 or 1, got %d", centre);
    OAI_CHECK_ARG(prepared_dev && y_dev && w_dev && (qg == 0 || nuisance_dev), "oai_regression_vx_prepare: null pointer");
    OAI_CHECK_WORKSPACE("oai_regression_vx_prepare", prepared_bytes, oai_regression_vx_prepare_workspace_bytes(n_knees, n_verts, sn + si));
    const PreparedVx out(prepared_dev, n_knees, n_verts, sn + si);
    const unsigned grid = cdiv(n_verts, kT);
    const hipStream_t st = (hipStream_t)stream;
#define OAI_CASE(SN, QG)                                                                                                                            \
    if (sn == SN && qg == QG)                                                                                                                       \
        prepare_vx_kernel<SN, QG><<<grid, kT, 0, st>>>(y_dev, mask_dev, w_dev, wmask_dev, nuisance_dev, n_knees, n_verts, sn + si, centre, out);
    OAI_CASE(0, 0) OAI_CASE(0, 1) OAI_CASE(0, 2) OAI_CASE(0, 3) OAI_CASE(0, 4) OAI_CASE(0, 5)
    OAI_CASE(1, 0) OAI_CASE(1, 1) OAI_CASE(1, 2) OAI_CASE(1, 3) OAI_CASE(1, 4)
    OAI_CASE(2, 0) OAI_CASE(2, 1) OAI_CASE(2, 2) OAI_CASE(2, 3)
#undef OAI_CASE
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_regression_vx_t_workspace_bytes(long long n_rows, long long n_verts, long long n_knees, int n_columns, int n_vertex_columns) {
    if (n_rows < 1 || n_rows > kMaxRows || !cohort_shape_ok(n_knees, n_verts) || n_columns < 1 || n_columns > kMaxCols || n_vertex_columns < 1 ||
        n_vertex_columns > kMaxVx || n_vertex_columns > n_columns)
        return 0;
    return VxWs(nullptr, n_rows, n_verts, n_knees, n_columns - n_vertex_columns).bytes;
}

int oai_regression_vx_t(const void* prepared_dev, size_t prepared_bytes, const double* global_dev, const int* perm_dev, long long n_knees,
                        long long n_verts, int n_columns, int n_vertex_nuisance, int n_vertex_interest, long long p0, long long p1, void* workspace_dev,
                        size_t workspace_bytes, double* slope0_dev, void* stream) {
    const int p = n_columns, sn = n_vertex_nuisance, si = n_vertex_interest;
    OAI_VX_CHECK_BATCH("oai_regression_vx_t", p, sn, si);
    OAI_CHECK_ARG(p - (sn + si) >= (si ? 0 : 1),
                  "oai_regression_vx_t: %d columns leave no column of interest beside %d per-vertex nuisance columns (n_columns too small)", p, sn);
    OAI_CHECK_ARG(prepared_dev && perm_dev && workspace_dev && (p == sn + si || global_dev), "oai_regression_vx_t: null pointer");
    OAI_CHECK_WORKSPACE("oai_regression_vx_t (prepared block)", prepared_bytes, oai_regression_vx_prepare_workspace_bytes(n_knees, n_verts, sn + si));
    OAI_CHECK_WORKSPACE("oai_regression_vx_t", workspace_bytes, oai_regression_vx_t_workspace_bytes(p1 - p0, n_verts, n_knees, p, sn + si));
    return run("oai_regression_vx_t", prepared_dev, global_dev, perm_dev, n_knees, n_verts, p, sn, si, p0, p1, workspace_dev, 0, slope0_dev, stream);
}

size_t oai_regression_vx_f_workspace_bytes(long long n_rows, long long n_verts, long long n_knees, int n_columns, int n_vertex_columns) {
    return oai_regression_vx_t_workspace_bytes(n_rows, n_verts, n_knees, n_columns, n_vertex_columns);
}

int oai_regression_vx_f(const void* prepared_dev, size_t prepared_bytes, const double* global_dev, const int* perm_dev, long long n_knees,
                        long long n_verts, int n_columns, int n_vertex_nuisance, int n_vertex_interest, int n_interest, long long p0, long long p1,
                        void* workspace_dev, size_t workspace_bytes, double* coef0_dev, void* stream) {
    const int p = n_columns, sn = n_vertex_nuisance, si = n_vertex_interest;
    OAI_VX_CHECK_BATCH("oai_regression_vx_f", p, sn, si);
    OAI_CHECK_ARG(!(si == 1 && n_interest > 0),
                  "oai_regression_vx_f: a per-vertex column of interest (s_i = 1) stands alone: no global columns of interest beside it (n_interest = %d); "
                  "test it with oai_regression_vx_t",
                  n_interest);
    OAI_CHECK_ARG(n_interest >= 1 && n_interest <= p - sn, "oai_regression_vx_f: needs 1 .. %d global columns of interest (n_interest), got %d", p - sn,
                  n_interest);
    OAI_CHECK_ARG(prepared_dev && global_dev && perm_dev && workspace_dev, "oai_regression_vx_f: null pointer");
    OAI_CHECK_WORKSPACE("oai_regression_vx_f (prepared block)", prepared_bytes, oai_regression_vx_prepare_workspace_bytes(n_knees, n_verts, sn + si));
    OAI_CHECK_WORKSPACE("oai_regression_vx_f", workspace_bytes, oai_regression_vx_f_workspace_bytes(p1 - p0, n_verts, n_knees, p, sn + si));
    return run("oai_regression_vx_f", prepared_dev, global_dev, perm_dev, n_knees, n_verts, p, sn, si, p0, p1, workspace_dev, n_interest, coef0_dev, stream);
}

}  // extern "C"
