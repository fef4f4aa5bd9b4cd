// The small dense solves that the per-vertex linear models share: the Cholesky factor of a packed lower triangle and the forward and
// backward solves with it, in the order and with the pivot rule that include/oai_hip.h states under "Cohort regression"
// (tests/group_regression_ref.py restates them operation for operation).  Five translation units use them: csrc/group_regression.hip,
// csrc/normative.hip and csrc/bootstrap.hip include this file, csrc/group_regression_vx.hip and csrc/cluster_robust.hip reach it
// through csrc/regression_rows.h; bootstrap.hip alone has no use for the backward solve.  Device code only; fp64 without contraction --
// the pragma below holds for the rest of the translation unit, and every user states it itself as well.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace oai {

constexpr int kMaxCols = 6;                        // p
constexpr double kPivot = 1e-10;

__host__ __device__ constexpr int tri(int p) { return p * (p + 1) / 2; }               // entries of a lower triangle; index of (a, 0)

// In place: the packed lower triangle A (entry (a, c), c <= a, at tri(a) + c) becomes its Cholesky factor L, column by column, inner sums
// in ascending k as s = s - L_ak * L_ck.  Returns whether every pivot passed; the arithmetic goes on after one that did not.
template <int P>
__device__ __forceinline__ bool cholesky(double* A) {
    bool pass = true;
#pragma unroll
    for (int a = 0; a < P; ++a) {
        const double diag = A[tri(a) + a];
        double s = diag;
#pragma unroll
        for (int k = 0; k < a; ++k) s = s - A[tri(a) + k] * A[tri(a) + k];
        pass = pass && s > kPivot * diag;
        const double l = sqrt(s);
        A[tri(a) + a] = l;
#pragma unroll
        for (int c = a + 1; c < P; ++c) {
            double u = A[tri(c) + a];
#pragma unroll
            for (int k = 0; k < a; ++k) u = u - A[tri(c) + k] * A[tri(a) + k];
            A[tri(c) + a] = u / l;
        }
    }
    return pass;
}

// L z = b in place, ascending rows, s = s - L_ak * z_k
template <int P>
__device__ __forceinline__ void forward_solve(const double* L, double* b) {
#pragma unroll
    for (int a = 0; a < P; ++a) {
        double s = b[a];
#pragma unroll
        for (int k = 0; k < a; ++k) s = s - L[tri(a) + k] * b[k];
        b[a] = s / L[tri(a) + a];
    }
}

// L^T x = w in place, from the last row up, s = s - L_ka * x_k with k ascending
template <int P>
__device__ __forceinline__ void backward_solve(const double* L, double* w) {
#pragma unroll
    for (int a = P - 1; a >= 0; --a) {
        double s = w[a];
#pragma unroll
        for (int k = a + 1; k < P; ++k) s = s - L[tri(k) + a] * w[k];
        w[a] = s / L[tri(a) + a];
    }
}

}  // namespace oai
