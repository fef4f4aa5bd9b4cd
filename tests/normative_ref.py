"""The numpy restatement of csrc/normative.hip (include/oai_hip.h, "Normative deviation"), operation for operation: every sum over knees is
a sequential ``for`` with one float64 accumulator that starts at +0.0, a missing entry is dropped by ``np.where`` (a select), the Cholesky
factor and the triangular solves are those of tests/group_regression_ref.py (the device shares them too: csrc/regression_solve.h), and
every expression is vectorised only over what is independent (vertices, and the rows of a tile).  numpy's float64 add, subtract,
multiply, divide and sqrt are IEEE and unfused, as the device's are without contraction.  Lower triangles are lists indexed [a][c],
c <= a; packed, entry (a, c) is component a (a + 1) / 2 + c."""
import numpy as np

import group_regression_ref as rref

MIN_DEN = 1e-10


def fit(Y, mask, Z):
    """dict of gamma (float64 [p, V]), L (float64 [p (p + 1) / 2, V]), rss (float64 [V]), n (int32 [V]), ok (uint8 [V]) -- the model block --
    and pivots (bool [V]: every pivot accepted, which the block holds only folded into ok)."""
    Y = np.asarray(Y, np.float32)
    N, V = Y.shape
    m = np.ones((N, V), bool) if mask is None else np.asarray(mask) != 0
    Z = np.asarray(Z, np.float64).reshape(N, -1)
    p = Z.shape[1]
    with np.errstate(all="ignore"):
        y = Y.astype(np.float64)
        n = np.zeros(V, np.int64)
        A = [[np.zeros(V) for _ in range(a + 1)] for a in range(p)]
        h = [np.zeros(V) for _ in range(p)]
        for i in range(N):
            n = n + m[i]
            for a in range(p):
                for c in range(a + 1):
                    A[a][c] = A[a][c] + np.where(m[i], Z[i, a] * Z[i, c], 0.0)
                h[a] = h[a] + np.where(m[i], Z[i, a] * y[i], 0.0)
        L, pivots = rref.cholesky(A)
        w = rref.forward(L, h)
        gamma = [None] * p
        for a in range(p - 1, -1, -1):
            s = w[a]
            for k in range(a + 1, p):
                s = s - L[k][a] * gamma[k]
            gamma[a] = s / L[a][a]
        rss = np.zeros(V)
        for i in range(N):
            e = y[i]
            for a in range(p):
                e = e - Z[i, a] * gamma[a]
            rss = rss + np.where(m[i], e * e, 0.0)
        ok = pivots & (n - p >= 1)
    return {"gamma": np.stack(gamma), "L": np.stack([L[a][c] for a in range(p) for c in range(a + 1)]), "rss": rss, "n": n.astype(np.int32),
            "ok": ok.astype(np.uint8), "pivots": pivots}


def score(model, X, xmask, G, loo, details=False):
    """(z, diff): float64 [rows, V] each; z NaN where it is not valid, diff NaN where the entry or the model is missing.  ``details``: a
    dict of z, diff and what they were made of (mx, lev, den, s2, dof) instead."""
    X = np.asarray(X, np.float32)
    rows, V = X.shape
    mx = np.ones((rows, V), bool) if xmask is None else np.asarray(xmask) != 0
    G = np.asarray(G, np.float64).reshape(rows, -1)
    p = G.shape[1]
    gamma, rss, n, ok = model["gamma"], model["rss"], model["n"].astype(np.int64), model["ok"] != 0
    L = [[model["L"][a * (a + 1) // 2 + c][None, :] for c in range(a + 1)] for a in range(p)]
    with np.errstate(all="ignore"):
        e = X.astype(np.float64)
        for a in range(p):
            e = e - G[:, a, None] * gamma[a][None, :]
        u = rref.forward(L, [np.broadcast_to(G[:, a, None], (rows, V)) for a in range(p)])
        lev = np.zeros((rows, V))
        for a in range(p):
            lev = lev + u[a] * u[a]
        if loo:
            den = 1.0 - lev
            dof = n - p - 1
            s2 = (rss[None, :] - (e * e) / den) / dof.astype(np.float64)[None, :]
            se2 = s2 * den
            cond = den > MIN_DEN
        else:
            den = None
            dof = n - p
            s2 = np.broadcast_to(rss / dof.astype(np.float64), (rows, V))
            se2 = s2 * (1.0 + lev)
            cond = np.ones((rows, V), bool)
        z = e / np.sqrt(se2)
        valid = mx & ok[None, :] & (dof >= 1)[None, :] & (s2 > 0.0) & cond
    z, diff = np.where(valid, z, np.nan), np.where(mx & ok[None, :], e, np.nan)
    return {"z": z, "diff": diff, "mx": mx, "lev": lev, "den": den, "s2": s2, "dof": dof} if details else (z, diff)


def nan_classes(Y, mask, Z):
    """How often each reason for a NaN occurs when the reference's own rows are scored, from the restatement alone -- what a hostile case
    must contain: "nothing" (vertices with n = p), "loo_dof" ((row, vertex) with n = p + 1: a z for loo = 0 and none for loo = 1), "den"
    (the leverage leaves no leave-one-out score: 1 - lev <= 1e-10 where everything else holds), "s2" (no residual variance, either loo)
    "pivot" (vertices whose factor has a rejected pivot) and "pivot_alone" (those of them with n - p >= 1, where nothing else says no)."""
    model = fit(Y, mask, Z)
    p = np.shape(Z)[1]
    n = model["n"].astype(np.int64)
    d0, d1 = (score(model, Y, mask, Z, loo, details=True) for loo in (0, 1))
    held = d1["mx"] & (model["ok"] != 0)[None, :] & (n - p - 1 >= 1)[None, :]
    return {"nothing": int(((n == p) & np.isnan(d0["z"]).all(axis=0)).sum()),
            "loo_dof": int(((n == p + 1)[None, :] & ~np.isnan(d0["z"]) & np.isnan(d1["z"])).sum()),
            "den": int((held & ~(d1["den"] > MIN_DEN) & ~np.isnan(d0["z"]) & np.isnan(d1["z"])).sum()),
            "s2": int((held & ~(d0["s2"] > 0.0) & ~(d1["s2"] > 0.0) & np.isnan(d0["z"]) & np.isnan(d1["z"])).sum()),
            "pivot": int((~model["pivots"]).sum()), "pivot_alone": int((~model["pivots"] & (n - p >= 1)).sum())}


def summary(tile, z0, weight=None):
    """(stats float64 [rows, 3], counts int64 [rows, 6]) of a z tile, as oai_deviation_summary states them."""
    tile = np.asarray(tile, np.float64)
    rows, V = tile.shape
    w = np.ones(V, np.int64) if weight is None else np.asarray(weight, np.int64)
    stats, counts = np.zeros((rows, 3)), np.zeros((rows, 6), np.int64)
    for r in range(rows):
        z = tile[r]
        valid = ~np.isnan(z)
        if not valid.any():
            stats[r], counts[r] = (0.0, np.nan, np.nan), (0, -1, 0, 0, 0, 0)
            continue
        a = np.where(valid, np.abs(z), -1.0)
        below, above = valid & (z < -z0), valid & (z > z0)
        stats[r] = (a.max(), z[valid].min(), z[valid].max())
        counts[r] = (valid.sum(), int(np.argmax(a)), below.sum(), w[below].sum(), above.sum(), w[above].sum())      # argmax: the first
    return stats, counts


def rank_p(stat, reference, member=False):
    """The family-wise p of a knee's statistic against the reference's own leave-one-out statistics: (1 + #{j: ref_j >= stat}) / (N' + 1);
    for a ``member`` of the reference itself is left out of the count and N' = N - 1."""
    reference = np.asarray(reference)
    stat = np.atleast_1d(stat)
    ge = (reference[None, :] >= stat[:, None]).sum(axis=1)
    N = len(reference)
    return (1.0 + (ge - 1)) / float(N - 1 + 1) if member else (1.0 + ge) / float(N + 1)      # a member is one of the j, and counted itself


def plain_design(seed, N, p):
    """float64 [N, p]: ones, then centred columns: age ~ N(60, 9), an alternating 0 / 1 column, then standard normals."""
    rng = np.random.default_rng(seed)
    cols = [np.ones(N)]
    for a in range(1, p):
        c = rng.normal(60.0, 9.0, N) if a == 1 else ((np.arange(N) % 2).astype(np.float64) if a == 2 else rng.normal(size=N))
        cols.append(c - c.mean())
    return np.ascontiguousarray(np.stack(cols, axis=1))


def hostile_case(seed, V, N, p, with_mask=True):
    """(Y float32 [N, V], mask uint8 [N, V] or None, Z float64 [N, p]) for N >= p + 2, holding every reason for a NaN that its size admits:
      with p >= 2 THE LAST COLUMN IS A DUMMY WHOSE ONLY MEMBER IS KNEE 0: its leverage is 1 wherever it has a value, so it has no
        leave-one-out score there (den), and a z as a new knee;
      vertex 0 (with a mask) has exactly n = p knees: nothing is valid;
      vertex 1 (V >= 2, with a mask) has the n = p + 1 knees 0 .. p: a z for loo = 0, none for loo = 1;
      vertex 2 (V >= 3) is 0.0 in every knee, every knee valid: no residual variance, exactly (s2 = 0);
      vertex 3 (V >= 4, with a mask) lacks knee 0 alone, so with p >= 2 the dummy column is all zeros there and its pivot is rejected
        with n - p >= 1; with p = 1 it has no knee at all, the only way to a rejected pivot with one column;
      elsewhere (with a mask) knees 0 .. p + 1 are valid and the others with probability 0.8.
    Under a 0 mask byte lie NaNs and 3e38.  p = 1 admits no den class: the leverage of an intercept alone is 1 / n."""
    rng = np.random.default_rng(seed)
    Z = plain_design(seed + 1, N, p)
    if p >= 2:
        Z[:, p - 1] = 0.0
        Z[0, p - 1] = 1.0
    Y = (2.4 + 0.3 * rng.normal(size=(N, V))).astype(np.float32)
    if p >= 3:
        Y += (0.01 * Z[:, 1])[:, None].astype(np.float32)
    if V >= 3:
        Y[:, 2] = np.float32(0.0)
    mask = None
    if with_mask:
        mask = (rng.random((N, V)) < 0.8).astype(np.uint8)
        mask[:p + 2] = 1
        mask[:, 0] = 0
        mask[rng.permutation(N)[:p], 0] = 1
        if V >= 2:
            mask[:, 1] = 0
            mask[:p + 1, 1] = 1
        if V >= 3:
            mask[:, 2] = 1
        if V >= 4:
            mask[:, 3] = 1 if p >= 2 else 0
            mask[0, 3] = 0
        gone = mask == 0
        Y[gone] = np.where(rng.random(int(gone.sum())) < 0.5, np.float32(np.nan), np.float32(3e38))
    return Y, mask, np.ascontiguousarray(Z)
