"""The numpy restatement of csrc/group_regression_vx.hip (include/oai_hip.h, "Vertex-wise design columns"), operation for operation, in
the manner of group_regression_ref.py and group_f_ref.py, whose ``cholesky`` and ``forward`` it uses as they are: every sum over knees is a
sequential ``for`` with one float64 accumulator that starts at +0.0, every product is rounded once before it is added, and every
expression is vectorised only over what is independent (vertices, and rows of the permutation matrix).

The design at a vertex has p columns in the order [vertex nuisance (s_n) | global nuisance (q_g) | global interest (k_g) | vertex
interest (s_i)]; ``W`` float32 [S, N, V] holds the S = s_n + s_i per-vertex columns in that order and ``design`` float64 [N, q_g + k_g] the
global ones."""
import numpy as np

from group_regression_ref import cholesky, forward


def _masks(shape, mask, wmask, S):
    my = np.ones(shape, bool) if mask is None else np.asarray(mask) != 0
    mw = np.ones((S,) + tuple(shape), bool) if wmask is None else np.asarray(wmask).reshape((S,) + tuple(shape)) != 0
    return my, mw


def prepare(Y, mask, W, wmask, nuisance, s_n, centre=True):
    """dict of R (float64 [N, V]), Q, mean (float64 [V]), n (int32 [V]), ok (uint8 [V]), n_dropped (int32 [V]), m (uint8 [N, V]: the effective
    mask) and WC (float64 [S, N, V]: the completed per-vertex columns).  ``nuisance``: the q_g global nuisance columns [N, q_g] or None;
    the first ``s_n`` planes of ``W`` are nuisance too."""
    Y = np.asarray(Y, np.float32)
    N, V = Y.shape
    W = np.asarray(W, np.float32).reshape(-1, N, V)
    S = W.shape[0]
    my, mw = _masks((N, V), mask, wmask, S)
    Z = np.zeros((N, 0)) if nuisance is None or np.size(nuisance) == 0 else np.asarray(nuisance, np.float64).reshape(N, -1)
    q_g = Z.shape[1]
    q = s_n + q_g
    with np.errstate(all="ignore"):
        y, w = Y.astype(np.float64), W.astype(np.float64)
        m = my.copy()
        for s in range(S):
            m = m & mw[s]
        n = np.zeros(V, np.int32)
        dropped = np.zeros(V, np.int32)
        total = np.zeros(V, np.float64)
        wsum = [np.zeros(V, np.float64) for _ in range(S)]
        for i in range(N):
            n = n + m[i]
            dropped = dropped + (my[i] & ~m[i])
            total = total + np.where(m[i], y[i], 0.0)
            for s in range(S):
                wsum[s] = wsum[s] + np.where(m[i], w[s, i], 0.0)
        count = n.astype(np.float64)
        mean = total / count
        WC = np.empty((S, N, V), np.float64)
        for s in range(S):
            wbar = wsum[s] / count
            c = wbar if centre else np.zeros(V)
            fill = np.zeros(V) if centre else wbar                        # a select, not a subtraction: exactly 0.0 when centred
            WC[s] = np.where((n > 0)[None, :], np.where(mw[s], w[s] - c[None, :], fill[None, :]), 0.0)
        d = np.where(m, (y - mean[None, :]) if centre else y, 0.0)

        def column(a, i):                                                 # nuisance column a at knee i: [V], or a scalar
            return WC[a, i] if a < s_n else Z[i, a - s_n]

        ok = np.ones(V, bool)
        gamma = []
        if q > 0:
            A = [[np.zeros(V) for _ in range(a + 1)] for a in range(q)]
            h = [np.zeros(V) for _ in range(q)]
            for i in range(N):
                for a in range(q):
                    for c in range(a + 1):
                        A[a][c] = A[a][c] + np.where(m[i], column(a, i) * column(c, i), 0.0)
                    h[a] = h[a] + column(a, i) * d[i]
            L, ok = cholesky(A)
            wv = forward(L, h)
            gamma = [None] * q
            for a in range(q - 1, -1, -1):
                s_ = wv[a]
                for k in range(a + 1, q):
                    s_ = s_ - L[k][a] * gamma[k]
                gamma[a] = s_ / L[a][a]
        R = np.empty((N, V), np.float64)
        Q = np.zeros(V, np.float64)
        for i in range(N):
            s_ = d[i]
            for a in range(q):
                s_ = s_ - column(a, i) * gamma[a]
            R[i] = np.where(m[i], s_, 0.0)
            Q = Q + R[i] * R[i]
        ok = ok & (n.astype(np.int64) - (q + 1) >= 1)
    return {"R": R, "Q": Q, "mean": mean, "n": n.astype(np.int32), "ok": ok.astype(np.uint8), "n_dropped": dropped.astype(np.int32),
            "m": m.astype(np.uint8), "WC": WC}


def _solve(prep, design, perm, s_n, s_i):
    """(L, every pivot accepted, z, p) of every (row, vertex): knee j of a row takes the WHOLE design row perm[row][j] -- the global entries
    of that knee and WC[s][perm[row][j]][v] -- against the fixed residuals and the fixed effective mask."""
    R, m, WC = prep["R"], prep["m"] != 0, prep["WC"]
    N, V = R.shape
    S = s_n + s_i
    assert WC.shape[0] == S and S in (1, 2) and s_i in (0, 1)
    D = np.zeros((N, 0)) if design is None or np.size(design) == 0 else np.asarray(design, np.float64).reshape(N, -1)
    pg = D.shape[1]
    p = S + pg
    idx = np.clip(np.asarray(perm, np.int64), 0, N - 1)
    P = idx.shape[0]
    M = [[np.zeros((P, V)) for _ in range(a + 1)] for a in range(p)]
    b = [np.zeros((P, V)) for _ in range(p)]
    for j in range(N):
        g = D[idx[:, j]]                                                  # [P, pg]
        cols = [WC[a][idx[:, j]] for a in range(s_n)] + [g[:, a, None] for a in range(pg)] + [WC[S - 1][idx[:, j]] for _ in range(s_i)]
        for a in range(p):
            for c in range(a + 1):
                M[a][c] = M[a][c] + np.where(m[j][None, :], cols[a] * cols[c], 0.0)
            b[a] = b[a] + cols[a] * R[j][None, :]
    L, pivots = cholesky(M)
    return L, pivots, forward(L, b), p


def regression_t(prep, design, perm, s_n, s_i, with_slope=False):
    """float64 [P, V]: the t of the LAST design column (the per-vertex one when s_i = 1) for every row of ``perm``, NaN where it is not
    valid; with ``with_slope`` also row 0's coefficient (float64 [V]).  ``design``: the global columns [N, q_g + k_g] or None."""
    Q, n, ok0 = prep["Q"], prep["n"], prep["ok"] != 0
    with np.errstate(all="ignore"):
        L, pivots, z, p = _solve(prep, design, perm, s_n, s_i)
        P, V = z[0].shape
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


def regression_f(prep, design, perm, s_n, n_interest, with_coef=False):
    """float64 [P, V]: the F of the last ``n_interest`` (global) design columns; with ``with_coef`` also row 0's coefficients of those
    columns (float64 [n_interest, V]).  Every per-vertex column is nuisance here (s_i = 0)."""
    Q, n, ok0 = prep["Q"], prep["n"], prep["ok"] != 0
    k = int(n_interest)
    with np.errstate(all="ignore"):
        L, pivots, z, p = _solve(prep, design, perm, s_n, 0)
        q = p - k
        assert 1 <= k <= p - s_n
        P, V = z[0].shape
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
                s_ = z[a][0]
                for j in range(a + 1, p):
                    s_ = s_ - L[j][a][0] * beta[j]
                beta[a] = s_ / L[a][a][0]
            return F, np.stack([np.where(valid[0], beta[a], np.nan) for a in range(q, p)])
    return F
