"""The numpy restatement of csrc/cluster_robust.hip (include/oai_hip.h, "Cluster-robust regression"), operation for operation: every sum
over rows or clusters is a sequential ``for`` with one float64 accumulator that starts at +0.0, the Cholesky factor and the triangular
solves are those of tests/group_regression_ref.py, and every expression is vectorised only over what is independent (vertices, and the
rows of the flip matrix).  numpy's float64 add, subtract, multiply, divide and sqrt are IEEE and unfused, as the device's are without
contraction.  Beside it: a generator of hostile cases, and a DENSE INDEPENDENT ROUTE -- ``np.linalg.lstsq`` of the full model and the
explicit sandwich inv(X'X) . sum_s X_s' e_s e_s' X_s . inv(X'X) per vertex, for row 0 and for explicitly rebuilt y* rows."""
import numpy as np

import group_regression_ref as rref


def tri(a):
    return a * (a + 1) // 2


def backward(L, w):
    """L^T x = w from the last row up, s = s - L_ka * x_k with k ascending."""
    size = len(w)
    x = [None] * size
    for a in range(size - 1, -1, -1):
        s = w[a]
        for k in range(a + 1, size):
            s = s - L[k][a] * x[k]
        x[a] = s / L[a][a]
    return x


def clamp_offsets(offsets, n_rows):
    return np.clip(np.asarray(offsets, np.int64), 0, n_rows)


def prepare(Y, mask, design, offsets, centre=True):
    """The cluster block as a dict: R, Q, mean, n, ok of rref.prepare on the first p - 1 columns, then H, K float64 [p, S, V], U float64
    [S, V], L float64 [p (p + 1) / 2, V], c float64 [V], G int32 [V], okc uint8 [V]."""
    Y = np.asarray(Y, np.float32)
    N, V = Y.shape
    D = np.asarray(design, np.float64).reshape(N, -1)
    p = D.shape[1]
    off = clamp_offsets(offsets, N)
    S = len(off) - 1
    m = np.ones((N, V), bool) if mask is None else np.asarray(mask) != 0
    block = rref.prepare(Y, mask, D[:, :-1] if p > 1 else None, centre)
    R, n = block["R"], block["n"].astype(np.int64)
    with np.errstate(all="ignore"):
        M = [[np.zeros(V) for _ in range(a + 1)] for a in range(p)]
        for j in range(N):
            for a in range(p):
                for c in range(a + 1):
                    M[a][c] = M[a][c] + np.where(m[j], D[j, a] * D[j, c], 0.0)
        L, pivots = rref.cholesky(M)
        e_p = [np.zeros(V) for _ in range(p - 1)] + [np.ones(V)]
        a_vec = backward(L, rref.forward(L, e_p))
        H, K, U = np.zeros((p, S, V)), np.zeros((p, S, V)), np.zeros((S, V))
        G = np.zeros(V, np.int64)
        for s in range(S):
            present = np.zeros(V, bool)
            for j in range(off[s], off[s + 1]):
                w = np.zeros(V)
                for c in range(p):
                    w = w + D[j, c] * a_vec[c]
                w = np.where(m[j], w, 0.0)
                for c in range(p):
                    H[c, s] = H[c, s] + np.where(m[j], D[j, c] * R[j], 0.0)
                    K[c, s] = K[c, s] + np.where(m[j], w * D[j, c], 0.0)
                U[s] = U[s] + np.where(m[j], w * R[j], 0.0)
                present = present | m[j]
            G = G + present
        cf = (G.astype(np.float64) / (G - 1).astype(np.float64)) * ((n - 1).astype(np.float64) / (n - p).astype(np.float64))
        okc = (block["ok"] != 0) & pivots & (G >= 2) & (n - p >= 1)
    block.update(H=H, K=K, U=U, L=np.stack([L[a][c] for a in range(p) for c in range(a + 1)]), c=cf, G=G.astype(np.int32), okc=okc.astype(np.uint8))
    return block


def cluster_t(block, flips, with_row0=False):
    """float64 [P, V]: the sandwich t of the last column for every row of ``flips`` (bool [P, S]: True flips the cluster), NaN where it is
    not valid; with ``with_row0`` also row 0's coefficient and standard error (float64 [V] each)."""
    H, K, U, cf, okc = block["H"], block["K"], block["U"], block["c"], block["okc"] != 0
    p, S, V = H.shape
    flips = np.atleast_2d(np.asarray(flips, bool))
    P = flips.shape[0]
    L = [[block["L"][tri(a) + c][None, :] for c in range(a + 1)] for a in range(p)]
    with np.errstate(all="ignore"):
        b = [np.zeros((P, V)) for _ in range(p)]
        for s in range(S):
            bit = flips[:, s, None]
            for c in range(p):
                b[c] = b[c] + np.where(bit, -H[c, s][None, :], H[c, s][None, :])
        beta = backward(L, rref.forward(L, b))
        W = np.zeros((P, V))
        for s in range(S):
            bit = flips[:, s, None]
            e = np.where(bit, -U[s][None, :], U[s][None, :])
            for c in range(p):
                e = e - K[c, s][None, :] * beta[c]
            W = W + e * e
        se = np.sqrt(cf[None, :] * W)
        valid = okc[None, :] & (W > 0.0)
        t = np.where(valid, beta[p - 1] / se, np.nan)
        if with_row0:
            return t, np.where(valid[0], beta[p - 1][0], np.nan), np.where(valid[0], se[0], np.nan)
    return t


def scores(block, flips_row):
    """float64 [S, V]: e_s of one flip row -- the cluster scores whose squares W sums."""
    p, S, V = block["H"].shape
    row = np.asarray(flips_row, bool)
    L = [[block["L"][tri(a) + c] for c in range(a + 1)] for a in range(p)]
    b = [np.zeros(V) for _ in range(p)]
    for s in range(S):
        for c in range(p):
            b[c] = b[c] + (-block["H"][c, s] if row[s] else block["H"][c, s])
    beta = backward(L, rref.forward(L, b))
    out = np.zeros((S, V))
    for s in range(S):
        e = -block["U"][s] if row[s] else block["U"][s]
        for c in range(p):
            e = e - block["K"][c, s] * beta[c]
        out[s] = e
    return out


# ---- the dense independent route -------------------------------------------------------------------------------------------------------
def dense_t(Y, mask, design, offsets, flips, centre=True):
    """float64 [P, V]: per vertex and flip row, over the valid rows alone: the null model's fit and residuals by lstsq, y* = fit + f o r,
    the full model refitted to y* by lstsq, the explicit CR1 sandwich, and beta_p over its standard error.  NaN where the vertex has fewer
    than two clusters or n - p < 1.  Shares no arithmetic with ``prepare`` / ``cluster_t``."""
    Y = np.asarray(Y, np.float64)
    N, V = Y.shape
    X = np.asarray(design, np.float64).reshape(N, -1)
    p = X.shape[1]
    off = clamp_offsets(offsets, N)
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
    flips = np.atleast_2d(np.asarray(flips, bool))
    m = np.ones((N, V), bool) if mask is None else np.asarray(mask) != 0
    out = np.full((flips.shape[0], V), np.nan)
    for v in range(V):
        keep = m[:, v]
        Xv, yv, own = X[keep], Y[keep, v], owner[keep]
        n, G = len(yv), len(np.unique(own))
        if G < 2 or n - p < 1 or np.linalg.matrix_rank(Xv) < p:
            continue
        if centre:
            yv = yv - yv.mean()
        Z = Xv[:, :-1]
        fit = Z @ np.linalg.lstsq(Z, yv, rcond=None)[0] if p > 1 else np.zeros(n)
        r = yv - fit
        bread = np.linalg.inv(Xv.T @ Xv)
        cf = (G / (G - 1)) * ((n - 1) / (n - p))
        for k, row in enumerate(flips):
            ystar = fit + np.where(row[own], -r, r)
            beta = np.linalg.lstsq(Xv, ystar, rcond=None)[0]
            e = ystar - Xv @ beta
            meat = np.zeros((p, p))
            for s in np.unique(own):
                g = Xv[own == s].T @ e[own == s]
                meat += np.outer(g, g)
            var = cf * (bread @ meat @ bread)[-1, -1]
            if var > 0:
                out[k, v] = beta[-1] / np.sqrt(var)
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
PLANTED = {"cluster_missing": 1, "one_cluster": 2, "rank": 3}              # vertices of a case with V >= 8 and a mask


def design_of(counts, p, rng):
    """[N, p] with x last and rows that vary WITHIN a cluster.  p = 1: a continuous x alone (no intercept).  p = 2: intercept and a dummy
    x.  p = 4: intercept, a sex dummy, years, a dummy x.  p = 6: intercept, a sex dummy, years, two continuous covariates, a continuous
    x.  The dummies alternate over the rows (sex with period 2, x with period 4)."""
    N = int(np.sum(counts))
    i = np.arange(N)
    sex, dummy = (i % 2).astype(np.float64), ((i // 2) % 2).astype(np.float64)
    years = np.concatenate([np.arange(k, dtype=np.float64) + rng.uniform(0.0, 0.5, k) for k in counts])
    cont = lambda: rng.normal(0.0, 1.0, N)
    cols = {1: [cont()], 2: [np.ones(N), dummy], 3: [np.ones(N), years, dummy], 4: [np.ones(N), sex, years, dummy],
            5: [np.ones(N), sex, years, cont(), dummy], 6: [np.ones(N), sex, years, 27 + 4 * cont(), cont(), cont()]}[p]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def hostile_case(seed, V, counts, with_mask, p=2):
    """(Y float32 [N, V], mask bool [N, V] or None, design float64 [N, p], offsets int32 [S + 1]) for clusters of ``counts`` rows: a random
    intercept per cluster (sd 0.3) under noise of sd 0.1, an effect of the last column at some vertices; with a mask, a tenth of the
    entries missing and -- where V >= 8 -- the corners of ``PLANTED``: a cluster wholly missing at a vertex (G < S), a vertex where one
    cluster alone has values (G = 1: no t), and one whose valid rows make M rank-deficient (the x dummy, or for p = 6 the sex dummy,
    constant among them: no t; for p = 1 a single valid row).  offsets[0] and offsets[S] lie outside [0, N]: clamped."""
    counts = tuple(int(k) for k in counts)
    rng = np.random.default_rng([seed, V, len(counts), int(np.sum(counts)), p, int(with_mask)])
    N, S = int(np.sum(counts)), len(counts)
    D = design_of(counts, p, rng)
    owner = np.repeat(np.arange(S), counts)
    Y = (2.0 + 0.3 * rng.normal(size=(S, V))[owner] + 0.1 * rng.normal(size=(N, V)) + 0.2 * D[:, -1:] * rng.random(V)[None, :]).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    offsets[0], offsets[S] = -3, N + 5
    mask = None
    if with_mask:
        mask = rng.random((N, V)) >= 0.1
        if V >= 8:
            mask[:, :4] = True
            mask[owner == 0, PLANTED["cluster_missing"]] = False
            mask[:, PLANTED["one_cluster"]] = owner == int(np.argmax(counts))
            if p == 1:
                mask[:, PLANTED["rank"]] = np.arange(N) == 0
            else:
                mask[:, PLANTED["rank"]] = D[:, 1 if p == 6 else -1] == 1.0
    for a in (Y, mask, D, offsets):
        if a is not None:
            a.setflags(write=False)
    return Y, mask, D, offsets


def flip_rows(seed, S, P):
    """bool [P, S]: row 0 flips nothing, row 1 flips every cluster, the others are drawn."""
    rng = np.random.default_rng([seed, S, P])
    rows = rng.integers(0, 2, size=(P, S)).astype(bool)
    rows[0] = False
    if P > 1:
        rows[1] = True
    return rows
