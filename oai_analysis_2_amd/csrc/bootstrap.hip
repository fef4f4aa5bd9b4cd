// Bootstrap intervals for gfx950 (include/oai_hip.h, "Bootstrap intervals"; tests/bootstrap_ref.py restates this file operation for
// operation): how large is an effect, give or take what -- the coefficient of the LAST column of the per-vertex general linear model,
// re-estimated on resamples of the knees, and what an interval needs from the replicates.
//   oai_bootstrap_coef          rows of integer weights on the knees -> one coefficient per (row, vertex) of a vertex span
//   oai_bootstrap_moments       per vertex over rows 1..: the finite replicates, their mean and standard error, below / equal counts
//   oai_column_quantiles        exact order statistics of float64 per vertex, numpy's "linear" quantile
//   oai_bootstrap_sup           per row the largest |theta* - theta^| / se over the span, folded into a running maximum
//   oai_jackknife_acceleration  the BCa acceleration from a leave-one-knee-out tile, per stratum
//
// fp64 without contraction; the order IS the contract, as in csrc/group_regression.hip: every sum over knees and over replicates runs in
// ascending index with one accumulator in one thread; the Cholesky factor, its pivot rule and the forward solve are
// csrc/regression_solve.h's.  No floating-point atomics.
//
// Shape of the coefficient kernel.  As regression_rows: a thread owns one vertex x R rows, a wave64 covers 64 consecutive vertices of the
// span, 256-thread blocks, the row groups of a vertex block next to each other in a one-dimensional grid, no LDS.  What depends on
// (row, knee) alone is wave-uniform and is read through scalar loads: table_kernel writes the per-knee table [N][E] of the design row g
// (p doubles) and its p (p + 1) / 2 products G_ac = g_a g_c (formed once per call, in fp64), E = p + p (p + 1) / 2, which all rows share;
// weights_kernel writes the batch's counts as doubles, KNEE-MAJOR [N][padded], so that the R weights of a thread are contiguous.
//   With a mask a thread carries h (p) and M (p (p + 1) / 2) per row.  Both are a product THEN an add: w*G is not exact for w > 1, so no
//     fma stands in for the pair.
//   Without a mask M_r = sum_i c_ri G_i does not depend on the vertex: row_factor_kernel forms it and its Cholesky factor once per row in
//     the stated order, and the hot loop carries h alone.
//   R is chosen per (p, masked) by measurement (profiles/bootstrap.md; N = 200, V = 30 002, 2001 rows).  The accumulators are
//   R (p + p (p + 1) / 2) doubles with a mask and R p without:
//         p            1     2     3     4     5     6
//     R   masked       8     4     2     4     2     2
//     R   no mask     16    16     8     8     8     8         the table of csrc/group_regression.hip; 74 .. 87 % of the fp64 issue rate
//     VGPRs / waves per SIMD from the compiler's kernel-resource remarks on the gfx950 build; scratch is 0 for all 12 instances:
//       masked       62/8  64/8  62/8  142/3 114/4 146/3
//       no mask      45/8  76/6  60/8  80/6  96/5  108/4
//     With a mask, ms at R / 2R of the table of csrc/group_regression.hip (16, 8, 2, 2, 1, 1), the starting guess: p = 1: 3.57 at 8
//     against 4.69 at 16; p = 2: 5.88 at 4 against 6.89 at 8; p = 3: 9.94 at 2 against 10.87 at 4 and 15.19 at 1; p = 4: 15.23 at 4
//     against 15.91 at 2 and 17.44 at 1; p = 5: 19.94 at 2 against 24.21 at 1; p = 6: 27.51 at 2 against 30.72 at 1.  Unlike the t
//     kernel's fused M, the multiply and the add of M here are two instructions per entry that share one scalar operand, so more rows
//     per knee's table loads pay at p >= 4 in spite of fewer waves.
// The quantile kernel has ONE path for every 1 <= R <= 2^20: the tile is transposed to vertex-major 64-bit keys (the order-preserving
// map below; a NaN becomes the largest key), then one workgroup per vertex runs an 8-pass radix select, most significant byte first, for
// all 2 K ranks at once, with a 256-bin histogram per rank in LDS (integer atomics only).
#include "cohort.h"

#include <cmath>

#pragma clang fp contract(off)

#include "ordered_reduce.h"
#include "regression_solve.h"

namespace {

using namespace oai;

constexpr int kT = 256;
constexpr int kRowPad = 16;                        // the largest R
constexpr int kMaxProbs = 4;                       // K
constexpr int kMaxStrata = 1 << 16;

__host__ __device__ constexpr int rows_per_thread(int p, bool masked) {
    return masked ? (p == 1 ? 8 : p == 2 ? 4 : p == 3 ? 2 : p == 4 ? 4 : 2) : (p <= 2 ? 16 : 8);
}

__device__ __forceinline__ bool finite_f64(double x) {
    return (__double_as_longlong(x) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}

// ---- oai_bootstrap_coef ----------------------------------------------------------------------------------------------------------------
struct CoefWs {
    double *tile, *table, *weights, *factor;
    size_t bytes;
    CoefWs(const void* base, long long rows, long long span, long long N, int p) {
        Ws ws(base);
        tile = ws.take<double>((size_t)(rows * span));
        table = ws.take<double>((size_t)N * (size_t)(p + tri(p)));
        weights = ws.take<double>((size_t)((rows + kRowPad - 1) * N));
        factor = ws.take<double>((size_t)(rows + kRowPad - 1) * (size_t)(tri(p) + 1));      // per row: L, then 1.0 / 0.0 = every pivot passed
        bytes = ws.off;
    }
};

// one thread per knee: g and the products G_ac = g_a*g_c, c <= a
template <int P>
__global__ void __launch_bounds__(kT) table_kernel(const double* __restrict__ D, long long N, double* __restrict__ table) {
    constexpr int E = P + tri(P);
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i >= N) return;
    double g[P];
#pragma unroll
    for (int a = 0; a < P; ++a) g[a] = D[i * P + a];
    double* e = table + i * E;
#pragma unroll
    for (int a = 0; a < P; ++a) e[a] = g[a];
#pragma unroll
    for (int a = 0; a < P; ++a) {
#pragma unroll
        for (int c = 0; c <= a; ++c) e[P + tri(a) + c] = g[a] * g[c];
    }
}

// one thread per (knee, padded row): the count as a double; a row past the last repeats the last
__global__ void __launch_bounds__(kT) weights_kernel(const unsigned short* __restrict__ counts, long long N, long long r0, long long rows,
                                                     long long padded, double* __restrict__ weights) {
    const long long at = (long long)blockIdx.x * kT + threadIdx.x;
    if (at >= padded * N) return;
    const long long j = at / padded, row = at - j * padded;
    weights[at] = (double)counts[(r0 + (row < rows ? row : rows - 1)) * N + j];
}

// without a mask, one thread per (padded) row: M = sum_i c_i G_i, knees ascending, a product then an add, and its factor
template <int P>
__global__ void __launch_bounds__(64) row_factor_kernel(const double* __restrict__ table, const double* __restrict__ weights, long long N,
                                                        long long padded, double* __restrict__ factor) {
    constexpr int T = tri(P), E = P + T;
    const long long row = (long long)blockIdx.x * 64 + threadIdx.x;
    if (row >= padded) return;
    double M[T];
#pragma unroll
    for (int k = 0; k < T; ++k) M[k] = 0.0;
    for (long long i = 0; i < N; ++i) {
        const double w = weights[i * padded + row];
#pragma unroll
        for (int k = 0; k < T; ++k) M[k] = M[k] + w * table[i * E + P + k];
    }
    const bool pass = cholesky<P>(M);
#pragma unroll
    for (int k = 0; k < T; ++k) factor[row * (T + 1) + k] = M[k];
    factor[row * (T + 1) + T] = pass ? 1.0 : 0.0;
}

// Block b is row group b % groups of vertex block b / groups of the span.  A lane past the span works on its last vertex and stores
// nothing; a padded row is worked on and not stored.  Rows here are relative to the batch.
template <int P, bool MASKED>
__global__ void __launch_bounds__(kT) coef_kernel(const float* __restrict__ Y, const unsigned char* __restrict__ mask, const double* __restrict__ table,
                                                  const double* __restrict__ weights, const double* __restrict__ factor, long long N, long long V,
                                                  long long v0, long long span, long long rows, long long padded, unsigned groups, int first,
                                                  double* __restrict__ tile, int* __restrict__ n_out, int* __restrict__ ok_out) {
    constexpr int R = rows_per_thread(P, MASKED);
    constexpr int T = tri(P);
    constexpr int E = P + T;
    const long long sv = (long long)(blockIdx.x / groups) * kT + threadIdx.x;
    const long long vc = v0 + (sv < span ? sv : span - 1);
    const long long r0 = (long long)(blockIdx.x % groups) * R;
    double h[R][P], M[R][MASKED ? T : 1];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int a = 0; a < P; ++a) h[r][a] = 0.0;
        if (MASKED) {
#pragma unroll
            for (int k = 0; k < T; ++k) M[r][k] = 0.0;
        }
    }
    const double* g = table;
    const double* w = weights + r0;
    int n = 0;
#pragma unroll 1
    for (long long i = 0; i < N; ++i) {
        const bool m = MASKED ? mask[i * V + vc] != 0 : true;
        const double y = m ? (double)Y[i * V + vc] : 0.0;
        n += m ? 1 : 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double wr = m ? w[r] : 0.0;
            const double u = wr * y;
#pragma unroll
            for (int a = 0; a < P; ++a) h[r][a] = h[r][a] + g[a] * u;
            if (MASKED) {
#pragma unroll
                for (int k = 0; k < T; ++k) M[r][k] = M[r][k] + wr * g[P + k];
            }
        }
        g += E;
        w += padded;
    }
    if (sv >= span) return;
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
        forward_solve<P>(L, h[r]);
        const double theta = h[r][P - 1] / L[T - 1];
        tile[(r0 + r) * span + sv] = pass ? theta : (double)NAN;
        if (first && r0 + r == 0) {
            if (n_out) n_out[vc] = n;
            if (ok_out) ok_out[vc] = pass ? 1 : 0;
        }
    }
}

template <int P, bool MASKED>
int launch_coef(const float* Y, const unsigned char* mask, const double* design, const unsigned short* counts, long long N, long long V, long long v0,
                long long v1, long long r0, long long r1, const CoefWs& ws, int* n_out, int* ok_out, hipStream_t st) {
    constexpr int R = rows_per_thread(P, MASKED);
    const long long rows = r1 - r0, span = v1 - v0;
    const unsigned groups = cdiv(rows, R);
    const long long padded = (long long)groups * R;
    const long long blocks = (long long)cdiv(span, kT) * groups;
    OAI_CHECK_ARG(blocks < (1LL << 31) && padded * N < (1LL << 31) * kT,
                  "oai_bootstrap_coef: %lld rows of %lld vertices and %lld knees are more than one launch takes: use fewer rows or a shorter span", rows,
                  span, N);
    table_kernel<P><<<cdiv(N, kT), kT, 0, st>>>(design, N, ws.table);
    OAI_CHECK_LAUNCH();
    weights_kernel<<<cdiv(padded * N, kT), kT, 0, st>>>(counts, N, r0, rows, padded, ws.weights);
    OAI_CHECK_LAUNCH();
    if (!MASKED) {
        row_factor_kernel<P><<<cdiv(padded, 64), 64, 0, st>>>(ws.table, ws.weights, N, padded, ws.factor);
        OAI_CHECK_LAUNCH();
    }
    coef_kernel<P, MASKED><<<(unsigned)blocks, kT, 0, st>>>(Y, mask, ws.table, ws.weights, ws.factor, N, V, v0, span, rows, padded, groups,
                                                            r0 == 0 ? 1 : 0, ws.tile, n_out, ok_out);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// ---- oai_bootstrap_moments -------------------------------------------------------------------------------------------------------------
// one thread per vertex, rows 1 .. R - 1 ascending, twice
__global__ void __launch_bounds__(kT) moments_kernel(const double* __restrict__ tile, long long R, long long V, int* __restrict__ n_finite,
                                                     double* __restrict__ mean_out, double* __restrict__ se_out, int* __restrict__ below_out,
                                                     int* __restrict__ equal_out) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= V) return;
    const double hat = tile[v];
    int n = 0, below = 0, equal = 0;
    double sum = 0.0;
    for (long long r = 1; r < R; ++r) {
        const double t = tile[r * V + v];
        const bool f = finite_f64(t);
        n += f ? 1 : 0;
        sum = sum + (f ? t : 0.0);
        below += f && t < hat ? 1 : 0;
        equal += f && t == hat ? 1 : 0;
    }
    const double mean = sum / (double)n;
    double ss = 0.0;
    for (long long r = 1; r < R; ++r) {
        const double t = tile[r * V + v];
        const double d = t - mean;
        ss = ss + (finite_f64(t) ? d * d : 0.0);
    }
    n_finite[v] = n;
    mean_out[v] = mean;
    se_out[v] = n >= 2 ? sqrt(ss / (double)(n - 1)) : (double)NAN;
    below_out[v] = below;
    equal_out[v] = equal;
}

// ---- oai_column_quantiles --------------------------------------------------------------------------------------------------------------
constexpr unsigned long long kSign = 0x8000000000000000ULL;
constexpr unsigned long long kNanKey = ~0ULL;      // above the key of +inf (0xfff0000000000000); the key of no number

__device__ __forceinline__ unsigned long long key_of(double x) {      // monotone double -> uint64 map; -0.0 before +0.0; every NaN last
    if (x != x) return kNanKey;
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u & kSign) ? ~u : (u | kSign);
}
__device__ __forceinline__ double double_of(unsigned long long k) {
    return __longlong_as_double((long long)((k & kSign) ? (k & ~kSign) : ~k));
}

// rows [first, R) of the tile [R][V] -> keys [V][n], n = R - first; 32 x 32 tiles through LDS, 256 threads as 32 x 8
__global__ void __launch_bounds__(kT) keys_kernel(const double* __restrict__ tile, long long first, long long n, long long V,
                                                  unsigned long long* __restrict__ keys) {
    __shared__ unsigned long long t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long long vb = (long long)blockIdx.x * 32, rb = (long long)blockIdx.y * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long r = rb + ty + 8 * k, v = vb + tx;
        t[ty + 8 * k][tx] = r < n && v < V ? key_of(tile[(first + r) * V + v]) : kNanKey;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long v = vb + ty + 8 * k, r = rb + tx;
        if (v < V && r < n) keys[v * n + r] = t[tx][ty + 8 * k];
    }
}

struct Probs {
    double q[kMaxProbs];
};

// numpy's _lerp
__device__ __forceinline__ double numpy_lerp(double a, double b, double t) {
    const double diff = b - a;
    return t < 0.5 ? a + diff * t : b - diff * (1.0 - t);
}

// One workgroup per vertex.  count = the keys that are not NaN; per probability the ranks fl and fl + 1 (the last element twice at or
// past n' - 1); eight passes, most significant byte first: the histogram of the byte among the keys that share a rank's prefix, then one
// thread per rank walks its 256 bins to the bin that holds the rank.
__global__ void __launch_bounds__(kT) quantile_kernel(const unsigned long long* __restrict__ keys, long long n, long long V, int K, Probs shared,
                                                      const double* __restrict__ per_vertex, double* __restrict__ out, int* __restrict__ count) {
    constexpr int NR = 2 * kMaxProbs;
    __shared__ unsigned hist[NR][256];
    __shared__ unsigned long long prefix[NR];
    __shared__ long long rank[NR];
    __shared__ double gamma[kMaxProbs];
    __shared__ int valid[kMaxProbs];
    __shared__ int cnt;
    const long long v = blockIdx.x;
    const unsigned long long* col = keys + v * n;
    const int nr = 2 * K;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int mine = 0;
    for (long long i = threadIdx.x; i < n; i += kT) mine += col[i] != kNanKey ? 1 : 0;
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    const long long np = cnt;
    if ((int)threadIdx.x < K) {
        const int k = threadIdx.x;
        const double q = per_vertex ? per_vertex[(long long)k * V + v] : shared.q[k];
        const bool ok = np > 0 && q >= 0.0 && q <= 1.0;
        long long lo = 0, hi = 0;
        double gm = 0.0;
        if (ok) {
            const double vi = (double)(np - 1) * q;
            const double fl = floor(vi);
            gm = vi - fl;
            lo = (long long)fl;
            if (lo >= np - 1) {
                lo = np - 1;
                hi = lo;
                gm = 0.0;
            } else {
                hi = lo + 1;
            }
        }
        rank[2 * k] = lo;
        rank[2 * k + 1] = hi;
        prefix[2 * k] = 0;
        prefix[2 * k + 1] = 0;
        gamma[k] = gm;
        valid[k] = ok ? 1 : 0;
    }
    if (np > 0) {                                          // uniform over the block
        for (int pass = 0; pass < 8; ++pass) {
            for (int i = threadIdx.x; i < NR * 256; i += kT) hist[i >> 8][i & 255] = 0;
            __syncthreads();
            const int shift = 56 - 8 * pass;
            unsigned long long pre[NR];
#pragma unroll
            for (int j = 0; j < NR; ++j) pre[j] = j < nr ? prefix[j] : 0;
            for (long long i = threadIdx.x; i < n; i += kT) {
                const unsigned long long key = col[i];
                if (key == kNanKey) continue;
                const unsigned long long hi = pass == 0 ? 0 : key >> (shift + 8);
                const unsigned d = (unsigned)(key >> shift) & 255u;
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    if (j < nr && hi == pre[j]) atomicAdd(&hist[j][d], 1u);
            }
            __syncthreads();
            if ((int)threadIdx.x < nr) {
                const int j = threadIdx.x;
                long long left = rank[j];
                int d = 0;
                for (; d < 255; ++d) {
                    const long long c = hist[j][d];
                    if (left < c) break;
                    left -= c;
                }
                rank[j] = left;
                prefix[j] = (prefix[j] << 8) | (unsigned long long)d;
            }
            __syncthreads();
        }
    } else {
        __syncthreads();
    }
    if ((int)threadIdx.x < K) {
        const int k = threadIdx.x;
        double r = (double)NAN;
        if (valid[k]) r = numpy_lerp(double_of(prefix[2 * k]), double_of(prefix[2 * k + 1]), gamma[k]);
        out[(long long)k * V + v] = r;
    }
    if (threadIdx.x == 0) count[v] = (int)np;
}

// ---- oai_bootstrap_sup -----------------------------------------------------------------------------------------------------------------
struct MaxAcc {
    double v[1];
    __device__ void clear() { v[0] = 0.0; }
    __device__ void merge(const double* o) { v[0] = o[0] > v[0] ? o[0] : v[0]; }
};

// one block per row; a max is exact in any order, so the row's running entry is read, raised and written by thread 0 alone
__global__ void __launch_bounds__(kT) sup_kernel(const double* __restrict__ tile, long long V, const double* __restrict__ se,
                                                 double* __restrict__ sup) {
    __shared__ double lds[kT / 64][1];
    const long long r = blockIdx.x;
    MaxAcc acc;
    acc.clear();
    for (long long v = threadIdx.x; v < V; v += kT) {
        const double hat = tile[v], s = se[v], t = tile[r * V + v];
        const double d = fabs(t - hat) / s;
        const bool take = finite_f64(hat) && s > 0.0 && t == t && d == d;
        const double o = take ? d : 0.0;
        acc.merge(&o);
    }
    block_reduce<kT>(acc, lds);
    if (threadIdx.x == 0) {
        const double old = sup[r];
        sup[r] = acc.v[0] > old ? acc.v[0] : old;
    }
}

// ---- oai_jackknife_acceleration --------------------------------------------------------------------------------------------------------
// one thread per vertex of the span; strata ascending, within a stratum the knees valid at the vertex ascending, twice
__global__ void __launch_bounds__(kT) acceleration_kernel(const double* __restrict__ jack, const unsigned char* __restrict__ mask,
                                                          const int* __restrict__ stratum, long long N, long long V, long long v0, long long span,
                                                          int S, double* __restrict__ accel) {
    const long long sv = (long long)blockIdx.x * kT + threadIdx.x;
    if (sv >= span) return;
    const long long v = v0 + sv;
    double num = 0.0, den = 0.0;
    bool bad = false;
    for (int s = 0; s < S; ++s) {
        int ns = 0;
        double sum = 0.0;
        for (long long i = 0; i < N; ++i) {
            const bool in = stratum[i] == s && (mask ? mask[i * V + v] != 0 : true);
            const double t = jack[i * span + sv];
            ns += in ? 1 : 0;
            sum = sum + (in ? t : 0.0);
            bad = bad || (in && t != t);
        }
        if (ns == 0) continue;
        const double nd = (double)ns;
        const double mean = sum / nd;
        const double nm1 = (double)(ns - 1);
        double s2 = 0.0, s3 = 0.0;
        for (long long i = 0; i < N; ++i) {
            const bool in = stratum[i] == s && (mask ? mask[i * V + v] != 0 : true);
            const double U = nm1 * (mean - jack[i * span + sv]);
            const double U2 = U * U;
            s2 = s2 + (in ? U2 : 0.0);
            s3 = s3 + (in ? U2 * U : 0.0);
        }
        num = num + s3 / (nd * nd * nd);
        den = den + s2 / (nd * nd);
    }
    const double a = (num / (den * sqrt(den))) / 6.0;
    accel[sv] = !bad && den > 0.0 ? a : (double)NAN;
}

}  // namespace

extern "C" {

size_t oai_bootstrap_coef_workspace_bytes(long long n_rows, long long n_span, long long n_knees, int n_columns) {
    if (n_rows < 1 || n_rows > kMaxRows || !cohort_shape_ok(n_knees, n_span) || n_columns < 1 || n_columns > kMaxCols) return 0;
    return CoefWs(nullptr, n_rows, n_span, n_knees, n_columns).bytes;
}

int oai_bootstrap_coef(const float* y_dev, const unsigned char* mask_dev, const double* design_dev, const unsigned short* counts_dev, long long n_knees,
                       long long n_verts, int n_columns, long long v0, long long v1, long long r0, long long r1, void* workspace_dev,
                       size_t workspace_bytes, int* n_dev, int* ok_dev, void* stream) {
    OAI_CHECK_ARG(cohort_shape_ok(n_knees, n_verts), "oai_bootstrap_coef: needs 2 .. 2^24 knees and 1 .. 2^31-2 vertices (got %lld, %lld)", n_knees, n_verts);
    OAI_CHECK_ARG(n_columns >= 1 && n_columns <= kMaxCols, "oai_bootstrap_coef: needs 1 .. 6 design columns, got %d", n_columns);
    OAI_CHECK_ARG(r0 >= 0 && r1 > r0 && r1 - r0 <= kMaxRows, "oai_bootstrap_coef: rows [r0, r1) must hold 1 .. 2^20 rows from r0 >= 0 (got %lld, %lld)", r0, r1);
    OAI_CHECK_ARG(v0 >= 0 && v1 > v0 && v1 <= n_verts, "oai_bootstrap_coef: the span [v0, v1) must lie in the %lld vertices (got %lld, %lld)", n_verts, v0, v1);
    OAI_CHECK_ARG(y_dev && design_dev && counts_dev && workspace_dev, "oai_bootstrap_coef: null pointer");
    OAI_CHECK_WORKSPACE("oai_bootstrap_coef", workspace_bytes, oai_bootstrap_coef_workspace_bytes(r1 - r0, v1 - v0, n_knees, n_columns));
    const CoefWs ws(workspace_dev, r1 - r0, v1 - v0, n_knees, n_columns);
    const hipStream_t st = (hipStream_t)stream;
    switch (n_columns) {
#define OAI_CASE(P)                                                                                                                            \
    case P:                                                                                                                                    \
        return mask_dev ? launch_coef<P, true>(y_dev, mask_dev, design_dev, counts_dev, n_knees, n_verts, v0, v1, r0, r1, ws, n_dev, ok_dev, st) \
                        : launch_coef<P, false>(y_dev, nullptr, design_dev, counts_dev, n_knees, n_verts, v0, v1, r0, r1, ws, n_dev, ok_dev, st);
        OAI_CASE(1) OAI_CASE(2) OAI_CASE(3) OAI_CASE(4) OAI_CASE(5) OAI_CASE(6)
#undef OAI_CASE
    }
    return OAI_OK;
}

int oai_bootstrap_moments(const double* tile_dev, long long n_rows, long long n_verts, int* n_finite_dev, double* mean_dev, double* se_dev,
                          int* below_dev, int* equal_dev, void* stream) {
    OAI_CHECK_ARG(tile_shape_ok(n_rows, n_verts), "oai_bootstrap_moments: needs 1 .. 2^20 rows and 1 .. 2^31-2 vertices (got %lld, %lld)", n_rows, n_verts);
    OAI_CHECK_ARG(tile_dev && n_finite_dev && mean_dev && se_dev && below_dev && equal_dev, "oai_bootstrap_moments: null pointer");
    moments_kernel<<<cdiv(n_verts, kT), kT, 0, (hipStream_t)stream>>>(tile_dev, n_rows, n_verts, n_finite_dev, mean_dev, se_dev, below_dev, equal_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

size_t oai_column_quantiles_workspace_bytes(long long n_rows, long long n_verts) {
    if (!tile_shape_ok(n_rows, n_verts)) return 0;
    return round256((size_t)n_rows * (size_t)n_verts * sizeof(unsigned long long));
}

int oai_column_quantiles(const double* tile_dev, long long n_rows, long long n_verts, long long first_row, int n_probs, const double* probs_host,
                         const double* probs_dev, void* workspace_dev, size_t workspace_bytes, double* out_dev, int* count_dev, void* stream) {
    OAI_CHECK_ARG(tile_shape_ok(n_rows, n_verts), "oai_column_quantiles: needs 1 .. 2^20 rows and 1 .. 2^31-2 vertices (got %lld, %lld)", n_rows, n_verts);
    OAI_CHECK_ARG(first_row >= 0 && first_row <= n_rows, "oai_column_quantiles: first_row must be 0 .. %lld, got %lld", n_rows, first_row);
    OAI_CHECK_ARG(n_probs >= 1 && n_probs <= kMaxProbs, "oai_column_quantiles: needs 1 .. 4 probabilities, got %d", n_probs);
    OAI_CHECK_ARG((probs_host != nullptr) != (probs_dev != nullptr),
                  "oai_column_quantiles: give the probabilities either shared on the host or per vertex on the device, one and not both");
    OAI_CHECK_ARG(tile_dev && workspace_dev && out_dev && count_dev, "oai_column_quantiles: null pointer");
    OAI_CHECK_WORKSPACE("oai_column_quantiles", workspace_bytes, oai_column_quantiles_workspace_bytes(n_rows, n_verts));
    const long long n = n_rows - first_row;
    OAI_CHECK_ARG(cdiv(n, 32) <= 65535u, "oai_column_quantiles: %lld rows are more than one launch takes", n);
    const hipStream_t st = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)workspace_dev;
    if (n > 0) {
        keys_kernel<<<dim3(cdiv(n_verts, 32), cdiv(n, 32)), kT, 0, st>>>(tile_dev, first_row, n, n_verts, keys);
        OAI_CHECK_LAUNCH();
    }
    Probs shared = {};
    if (probs_host)
        for (int k = 0; k < n_probs; ++k) shared.q[k] = probs_host[k];
    quantile_kernel<<<(unsigned)n_verts, kT, 0, st>>>(keys, n, n_verts, n_probs, shared, probs_dev, out_dev, count_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

int oai_bootstrap_sup(const double* tile_dev, long long n_rows, long long n_verts, const double* se_dev, double* sup_dev, void* stream) {
    OAI_CHECK_ARG(tile_shape_ok(n_rows, n_verts), "oai_bootstrap_sup: needs 1 .. 2^20 rows and 1 .. 2^31-2 vertices (got %lld, %lld)", n_rows, n_verts);
    OAI_CHECK_ARG(tile_dev && se_dev && sup_dev, "oai_bootstrap_sup: null pointer");
    sup_kernel<<<(unsigned)n_rows, kT, 0, (hipStream_t)stream>>>(tile_dev, n_verts, se_dev, sup_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

int oai_jackknife_acceleration(const double* jack_dev, const unsigned char* mask_dev, const int* stratum_dev, long long n_knees, long long n_verts,
                               long long v0, long long v1, int n_strata, double* accel_dev, void* stream) {
    OAI_CHECK_ARG(cohort_shape_ok(n_knees, n_verts), "oai_jackknife_acceleration: needs 2 .. 2^24 knees and 1 .. 2^31-2 vertices (got %lld, %lld)", n_knees,
                  n_verts);
    OAI_CHECK_ARG(v0 >= 0 && v1 > v0 && v1 <= n_verts, "oai_jackknife_acceleration: the span [v0, v1) must lie in the %lld vertices (got %lld, %lld)", n_verts,
                  v0, v1);
    OAI_CHECK_ARG(n_strata >= 1 && n_strata <= kMaxStrata, "oai_jackknife_acceleration: needs 1 .. 65536 strata, got %d", n_strata);
    OAI_CHECK_ARG(jack_dev && stratum_dev && accel_dev, "oai_jackknife_acceleration: null pointer");
    acceleration_kernel<<<cdiv(v1 - v0, kT), kT, 0, (hipStream_t)stream>>>(jack_dev, mask_dev, stratum_dev, n_knees, n_verts, v0, v1 - v0, n_strata,
                                                                          accel_dev);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // extern "C"
