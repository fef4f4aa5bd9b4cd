// The epilogue of one row r of a thread of the regression hot kernels, included INSIDE their loop over the thread's rows, once in
// regression_rows of csrc/group_regression.hip and once in vx_rows of csrc/group_regression_vx.hip: the forward solve, the residual sum
// of squares and the statistic -- the t of the last column or, with FSTAT, the F of the last ki -- and row 0's coefficient(s), in the
// order that include/oai_hip.h states under "Cohort regression" and "Cohort F test" (tests/group_regression_ref.py and
// tests/group_f_ref.py restate it operation for operation).  One text, so that the statistics of the two files cannot drift apart; a
// body and not a __device__ function, as csrc/unet_wino_body.h is, because it is the text that regression_rows has always had: its 24
// instances compile to the VGPR, SGPR and scratch figures they had before csrc/group_regression_vx.hip existed, which a forced-inline
// function did not give (two of the 24 moved by 2 VGPRs and 4 SGPRs).  No include guard.
// It reads P, FSTAT and T = tri(P); L (the factor of M, packed lower triangle) and pass (every pivot of it accepted); b[r] (the
// right-hand side, solved in place); Q, dof, ok; ki, V, v, r, r0, first; and writes tile and out0.
        forward_solve<P>(L, b[r]);
        double rss = Q;
#pragma unroll
        for (int a = 0; a < P; ++a) rss = rss - b[r][a] * b[r][a];
        const double s2 = rss / (double)dof;
        const bool valid = ok && pass && s2 > 0.0;
        if (!FSTAT) {
            const double t = b[r][P - 1] / sqrt(s2);
            tile[(r0 + r) * V + v] = valid ? t : (double)NAN;
            if (first && out0 && r0 + r == 0) out0[v] = valid ? b[r][P - 1] / L[T - 1] : (double)NAN;
        } else {
            const int q = P - ki;                                                 // the columns of interest are q .. P - 1
            double ess = 0.0;
#pragma unroll
            for (int a = 0; a < P; ++a) ess = a >= q ? ess + b[r][a] * b[r][a] : ess;
            const double F = (ess / (double)ki) / s2;
            tile[(r0 + r) * V + v] = valid ? F : (double)NAN;
            if (r == 0 && first && out0 && r0 == 0) {                             // L^T beta = z on the trailing block, from the last row up
                double beta[P];
#pragma unroll
                for (int a = P - 1; a >= 0; --a) {
                    if (a < q) continue;
                    double s = b[r][a];
#pragma unroll
                    for (int j = a + 1; j < P; ++j) s = s - L[tri(j) + a] * beta[j];
                    beta[a] = s / L[tri(a) + a];
                    out0[(long long)(a - q) * V + v] = valid ? beta[a] : (double)NAN;
                }
            }
        }
