"""The numpy restatement of csrc/group_regression.hip (include/oai_hip.h, "Cohort regression"), operation for operation: every sum over
knees is a sequential ``for`` with one float64 accumulator that starts at +0.0, the Cholesky factor and the triangular solves loop over
their columns in the header's order and association, and every expression is vectorised only over what is independent (vertices, and
rows of the permutation matrix).  numpy's float64 add, subtract, multiply, divide and sqrt are IEEE and unfused, as the device's are
without contraction.  Lower triangles are lists indexed [a][c], c <= a."""
import numpy as np

PIVOT = 1e-10


def cholesky(A):
    """In the header's order; A[a][c] arrays of one shape.  Returns (L, every pivot accepted); the arithmetic goes on after a refusal."""
    size = len(A)
    L = [[None] * (a + 1) for a in range(size)]
    ok = np.ones(np.shape(A[0][0]), bool)
    for a in range(size):
        s = A[a][a]
        for k in range(a):
            s = s - L[a][k] * L[a][k]
        ok = ok & (s > PIVOT * A[a][a])
        L[a][a] = np.sqrt(s)
        for c in range(a + 1, size):
            s = A[c][a]
            for k in range(a):
                s = s - L[c][k] * L[a][k]
            L[c][a] = s / L[a][a]
    return L, ok


def forward(L, b):
    z = []
    for a in range(len(b)):
        s = b[a]
        for k in range(a):
            s = s - L[a][k] * z[k]
        z.append(s / L[a][a])
    return z


def prepare(Y, mask=None, nuisance=None, centre=True):
    """dict of R (float64 [N, V]), Q, mean (float64 [V]), n (int32 [V]), ok (uint8 [V])."""
    Y = np.asarray(Y, np.float32)
    N, V = Y.shape
    m = np.ones((N, V), bool) if mask is None else np.asarray(mask) != 0
    Z = np.zeros((N, 0)) if nuisance is None else np.asarray(nuisance, np.float64).reshape(N, -1)
    q = Z.shape[1]
    with np.errstate(all="ignore"):
        y = Y.astype(np.float64)
        n = np.zeros(V, np.int32)
        total = np.zeros(V, np.float64)
        for i in range(N):
            n = n + m[i]
            total = total + np.where(m[i], y[i], 0.0)
        mean = total / n.astype(np.float64)
        d = np.where(m, (y - mean[None, :]) if centre else y, 0.0)
        ok = np.ones(V, bool)
        gamma = []
        if q > 0:
            A = [[np.zeros(V) for _ in range(a + 1)] for a in range(q)]
            h = [np.zeros(V) for _ in range(q)]
            for i in range(N):
                for a in range(q):
                    for c in range(a + 1):
                        A[a][c] = A[a][c] + np.where(m[i], Z[i, a] * Z[i, c], 0.0)
                    h[a] = h[a] + Z[i, a] * d[i]
            L, ok = cholesky(A)
            w = forward(L, h)
            gamma = [None] * q
            for a in range(q - 1, -1, -1):
                s = w[a]
                for k in range(a + 1, q):
                    s = s - L[k][a] * gamma[k]
                gamma[a] = s / L[a][a]
        R = np.empty((N, V), np.float64)
        Q = np.zeros(V, np.float64)
        for i in range(N):
            s = d[i]
            for a in range(q):
                s = s - Z[i, a] * gamma[a]
            R[i] = np.where(m[i], s, 0.0)
            Q = Q + R[i] * R[i]
        ok = ok & (n.astype(np.int64) - (q + 1) >= 1)
    return {"R": R, "Q": Q, "mean": mean, "n": n.astype(np.int32), "ok": ok.astype(np.uint8)}


def regression_t(prep, mask, design, perm, with_slope=False):
    """float64 [P, V]: the t of the last design column for every row of ``perm`` (int [P, N]), NaN where it is not valid; with
    ``with_slope`` also row 0's coefficient (float64 [V])."""
    R, Q, n, ok0 = prep["R"], prep["Q"], prep["n"], prep["ok"] != 0
    N, V = R.shape
    D = np.asarray(design, np.float64).reshape(N, -1)
    p = D.shape[1]
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
        dof = n.astype(np.int64) - p
        s2 = rss / dof.astype(np.float64)[None, :]
        t = z[p - 1] / np.sqrt(s2)
        valid = ok0[None, :] & pivots & (dof >= 1)[None, :] & (s2 > 0.0)
        t = np.where(valid, t, np.nan)
        if with_slope:
            return t, np.where(valid[0], z[p - 1][0] / L[p - 1][p - 1][0], np.nan)
    return t


def design_columns(x, covariates=None, intercept=True):
    """The host side of stats.regression_test, restated: (nuisance [N, q], design [N, q + 1], scale of x).  Columns are centred over all
    N knees when there is an intercept and scaled to unit sum of squares; the intercept is a column of ones, first; x is last."""
    x = np.asarray(x, np.float64)
    cols = [] if covariates is None else [c for c in np.asarray(covariates, np.float64).reshape(len(x), -1).T]
    out = []
    for c in cols + [x]:
        c = c - c.mean() if intercept else c.copy()
        out.append((c, np.sqrt((c * c).sum())))
    scale = out[-1][1]
    Z = ([np.ones(len(x))] if intercept else []) + [c / s for c, s in out[:-1]]
    nuisance = np.stack(Z, axis=1) if Z else np.zeros((len(x), 0))
    return nuisance, np.concatenate([nuisance, (out[-1][0] / scale)[:, None]], axis=1), scale
