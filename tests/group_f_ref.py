"""The numpy restatement of oai_regression_f (csrc/group_regression.hip; include/oai_hip.h, "Cohort F test"), operation for operation, in
the manner of group_regression_ref.py, whose ``cholesky``, ``forward`` and ``prepare`` it uses as they are: every sum over knees is a
sequential ``for`` with one float64 accumulator that starts at +0.0, and every expression is vectorised only over what is independent
(vertices, and rows of the permutation matrix).  Also the host side of stats.f_test and stats.anova_test, restated: how the design is
built from what the caller passes."""
import numpy as np

from group_regression_ref import cholesky, forward, prepare            # noqa: F401  (prepare: for the callers of this module)


def regression_f(prep, mask, design, perm, n_interest, with_coef=False):
    """float64 [P, V]: the F of the last ``n_interest`` design columns for every row of ``perm`` (int [P, N]), NaN where it is not valid;
    with ``with_coef`` also row 0's coefficients of those columns (float64 [n_interest, V]).  ``prep``: ``prepare`` with the first
    p - n_interest columns as the nuisance."""
    R, Q, n, ok0 = prep["R"], prep["Q"], prep["n"], prep["ok"] != 0
    N, V = R.shape
    D = np.asarray(design, np.float64).reshape(N, -1)
    p, k = D.shape[1], int(n_interest)
    q = p - k
    assert 1 <= k <= p
    idx = np.clip(np.asarray(perm, np.int64), 0, N - 1)
    P = idx.shape[0]
    m = np.ones((N, V), bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(all="ignore"):
        M = [[np.zeros((P, V)) for _ in range(a + 1)] for a in range(p)]
        b = [np.zeros((P, V)) for _ in range(p)]
        for j in range(N):
            g = D[idx[:, j]]                                               # [P, p]
            for a in range(p):
                for c in range(a + 1):
                    G = (g[:, a] * g[:, c])[:, None]
                    M[a][c] = M[a][c] + np.where(m[j][None, :], G, 0.0)
                b[a] = b[a] + g[:, a, None] * R[j][None, :]
        L, pivots = cholesky(M)
        z = forward(L, b)
        rss = np.broadcast_to(Q[None, :], (P, V))
        for a in range(p):
            rss = rss - z[a] * z[a]
        ess = np.zeros((P, V))
        for a in range(q, p):
            ess = ess + z[a] * z[a]
        dof = n.astype(np.int64) - p
        s2 = rss / dof.astype(np.float64)[None, :]
        F = (ess / float(k)) / s2
        valid = ok0[None, :] & pivots & (dof >= 1)[None, :] & (s2 > 0.0)
        F = np.where(valid, F, np.nan)
        if with_coef:
            beta = [None] * p
            for a in range(p - 1, q - 1, -1):
                s = z[a][0]
                for j in range(a + 1, p):
                    s = s - L[j][a][0] * beta[j]
                beta[a] = s / L[a][a][0]
            return F, np.stack([np.where(valid[0], beta[a], np.nan) for a in range(q, p)])
    return F


def design_matrix(X, covariates=None, intercept=True):
    """The host side of stats.f_test, restated: (nuisance [N, q], design [N, q + k], the k scales of the columns of X).  Columns are
    centred over all N knees when there is an intercept and scaled to unit sum of squares; the intercept is a column of ones, first; the
    covariates follow; the columns of X are last, in their order."""
    X = np.asarray(X, np.float64)
    X = X[:, None] if X.ndim == 1 else X
    N = len(X)
    cols = [] if covariates is None else [c for c in np.asarray(covariates, np.float64).reshape(N, -1).T]
    n_cov = len(cols)
    out = []
    for c in cols + [x for x in X.T]:
        c = c - c.mean() if intercept else c.copy()
        out.append((c, np.sqrt((c * c).sum())))
    Z = ([np.ones(N)] if intercept else []) + [c / s for c, s in out[:n_cov]]
    nuisance = np.stack(Z, axis=1) if Z else np.zeros((N, 0))
    design = np.concatenate([nuisance] + [(c / s)[:, None] for c, s in out[n_cov:]], axis=1)
    return nuisance, np.ascontiguousarray(design), np.asarray([s for _, s in out[n_cov:]])


def anova_dummies(groups):
    """The host side of stats.anova_test, restated: (the sorted labels, [N, G - 1] with a 0 / 1 column for every level after the smallest)."""
    g = np.asarray(groups)
    levels = np.unique(g)
    return levels, np.stack([(g == lab).astype(np.float64) for lab in levels[1:]], axis=1)
