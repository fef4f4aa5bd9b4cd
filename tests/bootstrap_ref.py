"""The numpy restatement of csrc/bootstrap.hip (include/oai_hip.h, "Bootstrap intervals"), operation for operation: every sum over knees
and over replicates is a sequential ``for`` with one float64 accumulator that starts at +0.0, products and adds are separate numpy
operations (numpy has no fma), the Cholesky factor and the forward solve are tests/group_regression_ref.py's, and every expression is
vectorised only over what is independent (vertices, and rows of the count matrix).  ``ci`` restates the host side of
``oai_analysis_2_amd.stats.bootstrap_ci`` as well.  Test infrastructure: no GPU, no library."""
import numpy as np

from group_regression_ref import cholesky, design_columns, forward

SIGN = np.uint64(1 << 63)


def counts(n_knees, n_bootstrap, seed=0, blocks=None):
    """uint16 [B + 1, N]: row 0 ones; per block in ascending label, rng.integers(0, n_b, (B, n_b)) binned, knee by knee."""
    N, B = int(n_knees), int(n_bootstrap)
    labels = np.zeros(N, np.int64) if blocks is None else np.asarray(blocks)
    rng = np.random.Generator(np.random.PCG64(seed))
    c = np.zeros((B + 1, N), np.int64)
    c[0] = 1
    for lab in np.unique(labels):
        idx = np.nonzero(labels == lab)[0]
        draws = rng.integers(0, len(idx), size=(B, len(idx)))
        for r in range(B):
            for d in draws[r]:
                c[r + 1, idx[d]] += 1
    return c.astype(np.uint16)


def coef(Y, mask, design, count_rows, v0=0, v1=None):
    """(theta float64 [R, v1 - v0], n int32 [v1 - v0], ok int32 [v1 - v0]) for the rows of ``count_rows`` [R, N]."""
    Y = np.asarray(Y, np.float32)
    N, V = Y.shape
    v1 = V if v1 is None else v1
    m = (np.ones((N, V), bool) if mask is None else np.asarray(mask) != 0)[:, v0:v1]
    D = np.asarray(design, np.float64).reshape(N, -1)
    p = D.shape[1]
    c = np.asarray(count_rows).astype(np.float64)
    R, S = c.shape[0], v1 - v0
    with np.errstate(all="ignore"):
        y = np.where(m, Y[:, v0:v1].astype(np.float64), 0.0)
        h = [np.zeros((R, S)) for _ in range(p)]
        M = [[np.zeros((R, S)) for _ in range(a + 1)] for a in range(p)]
        n = np.zeros(S, np.int32)
        for i in range(N):
            n = n + m[i]
            w = np.where(m[i][None, :], c[:, i, None], 0.0)
            u = w * y[i][None, :]
            for a in range(p):
                h[a] = h[a] + D[i, a] * u
                for k in range(a + 1):
                    G = D[i, a] * D[i, k]
                    M[a][k] = M[a][k] + w * G
        L, ok = cholesky(M)
        z = forward(L, h)
        theta = np.where(ok, z[p - 1] / L[p - 1][p - 1], np.nan)
    return theta, n.astype(np.int32), ok[0].astype(np.int32)


def moments(tile):
    """dict of n_finite, below, equal (int32 [V]) and mean, se (float64 [V]) over rows 1.. of ``tile`` [R, V], ascending."""
    tile = np.asarray(tile, np.float64)
    R, V = tile.shape
    hat = tile[0]
    n, below, equal = np.zeros(V, np.int32), np.zeros(V, np.int32), np.zeros(V, np.int32)
    total = np.zeros(V)
    with np.errstate(all="ignore"):
        for r in range(1, R):
            t = tile[r]
            f = np.isfinite(t)
            n = n + f
            total = total + np.where(f, t, 0.0)
            below = below + (f & (t < hat))
            equal = equal + (f & (t == hat))
        mean = total / n.astype(np.float64)
        ss = np.zeros(V)
        for r in range(1, R):
            t = tile[r]
            d = t - mean
            ss = ss + np.where(np.isfinite(t), d * d, 0.0)
        se = np.where(n >= 2, np.sqrt(ss / (n - 1).astype(np.float64)), np.nan)
    return {"n_finite": n.astype(np.int32), "mean": mean, "se": se, "below": below.astype(np.int32), "equal": equal.astype(np.int32)}


def keys(x):
    """The order-preserving map float64 -> uint64: -0.0 before +0.0."""
    u = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return np.where(u & SIGN != 0, ~u, u | SIGN)


def column_quantiles(tile, probabilities, first_row=0):
    """(float64 [K, V], int32 [V]): numpy's "linear" quantile of the entries of rows [first_row, R) that are not NaN, per vertex, in the
    order of ``keys``.  ``probabilities``: [K] shared or [K, V] per vertex."""
    tile = np.asarray(tile, np.float64)
    V = tile.shape[1]
    probs = np.asarray(probabilities, np.float64)
    K = probs.shape[0]
    out, count = np.full((K, V), np.nan), np.zeros(V, np.int32)
    with np.errstate(all="ignore"):
        for v in range(V):
            col = tile[first_row:, v]
            col = col[~np.isnan(col)]
            n = len(col)
            count[v] = n
            srt = col[np.argsort(keys(col), kind="stable")]
            for k in range(K):
                q = probs[k] if probs.ndim == 1 else probs[k, v]
                if n == 0 or not (q >= 0.0 and q <= 1.0):
                    continue
                vi = np.float64(n - 1) * q
                fl = np.floor(vi)
                gamma = vi - fl
                lo = int(fl)
                if lo >= n - 1:
                    lo, hi, gamma = n - 1, n - 1, np.float64(0.0)
                else:
                    hi = lo + 1
                a, b = srt[lo], srt[hi]
                diff = b - a
                out[k, v] = a + diff * gamma if gamma < 0.5 else b - diff * (np.float64(1.0) - gamma)
    return out, count


def sup(tile, se, running):
    """The running maximum [R] raised by each row's max of |theta* - theta^| / se where theta^ is finite, se > 0 and the entry is not NaN."""
    tile = np.asarray(tile, np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(tile - tile[0][None, :]) / se[None, :]
        take = np.isfinite(tile[0])[None, :] & (se > 0.0)[None, :] & ~np.isnan(tile) & ~np.isnan(d)
        row = np.where(take, d, 0.0).max(axis=1)
    return np.maximum(running, row)


def acceleration(jack, mask, strata, n_strata, v0=0):
    """float64 [span]: the BCa acceleration from the jackknife tile [N, span]."""
    jack = np.asarray(jack, np.float64)
    N, S = jack.shape
    m = np.ones((N, S), bool) if mask is None else (np.asarray(mask) != 0)[:, v0:v0 + S]
    num, den, bad = np.zeros(S), np.zeros(S), np.zeros(S, bool)
    with np.errstate(all="ignore"):
        for s in range(n_strata):
            ns, total = np.zeros(S, np.int64), np.zeros(S)
            for i in range(N):
                inside = m[i] & (strata[i] == s)
                ns = ns + inside
                total = total + np.where(inside, jack[i], 0.0)
                bad = bad | (inside & np.isnan(jack[i]))
            nd = ns.astype(np.float64)
            mean = total / nd
            nm1 = (ns - 1).astype(np.float64)
            s2, s3 = np.zeros(S), np.zeros(S)
            for i in range(N):
                inside = m[i] & (strata[i] == s)
                U = nm1 * (mean - jack[i])
                U2 = U * U
                s2 = s2 + np.where(inside, U2, 0.0)
                s3 = s3 + np.where(inside, U2 * U, 0.0)
            num = np.where(ns > 0, num + s3 / (nd * nd * nd), num)
            den = np.where(ns > 0, den + s2 / (nd * nd), den)
        a = (num / (den * np.sqrt(den))) / 6.0
    return np.where(~bad & (den > 0.0), a, np.nan)


def bca_probabilities(below, equal, n_finite, accel, level):
    """(z0, probabilities [2, V]) as scipy.stats.bootstrap forms them."""
    from scipy import special
    alpha = (1.0 - float(level)) / 2.0
    with np.errstate(all="ignore"):
        z0 = special.ndtri((below + (below + equal)).astype(np.float64) / (2.0 * n_finite.astype(np.float64)))
        z_alpha = special.ndtri(alpha)
        z_1alpha = -z_alpha
        num1 = z0 + z_alpha
        p_low = special.ndtr(z0 + num1 / (1.0 - accel * num1))
        num2 = z0 + z_1alpha
        p_high = special.ndtr(z0 + num2 / (1.0 - accel * num2))
    return z0, np.stack([p_low, p_high])


def design_of(n_knees, x=None, groups=None, covariates=None, intercept=True, blocks=None):
    """(design, scale, the block label of every knee) as stats.bootstrap_ci forms them."""
    N = n_knees
    labels = np.zeros(N, np.int64) if blocks is None else np.unique(np.asarray(blocks), return_inverse=True)[1].reshape(-1)
    if x is None and groups is None:
        return np.ones((N, 1)), 1.0, labels
    if groups is not None:
        which = np.unique(np.asarray(groups), return_inverse=True)[1].reshape(-1)
        _, D, scale = design_columns(which.astype(np.float64), covariates, intercept)
        return D, scale, labels * 2 + which
    _, D, scale = design_columns(x, covariates, intercept)
    return D, scale, labels


def ci(Y, mask, count_rows, level, method, simultaneous=False, x=None, groups=None, covariates=None, intercept=True, blocks=None):
    """dict of the fields of stats.BootstrapResult, every step restated on the host."""
    Y = np.asarray(Y, np.float32)
    N = Y.shape[0]
    D, scale, labels = design_of(N, x, groups, covariates, intercept, blocks)
    tile, n, _ = coef(Y, mask, D, count_rows)
    mom = moments(tile)
    est, se = tile[0], mom["se"]
    alpha = (1.0 - level) / 2.0
    out = {}
    if method == "bca":
        strata = np.unique(labels, return_inverse=True)[1].reshape(-1)
        jack, _, _ = coef(Y, mask, D, 1 - np.eye(N, dtype=np.int64))
        accel = acceleration(jack, mask, strata, len(np.unique(labels)))
        z0, probs = bca_probabilities(mom["below"], mom["equal"], mom["n_finite"], accel, level)
        q, _ = column_quantiles(tile, probs, 1)
        out.update(z0=z0, acceleration=accel)
    else:
        q, _ = column_quantiles(tile, np.array([alpha, 1.0 - alpha]), 1)
    low, high = (2.0 * est - q[1], 2.0 * est - q[0]) if method == "basic" else (q[0], q[1])
    out.update(estimate=est / scale, se=se / scale, lower=low / scale, upper=high / scale, n=n, n_finite=mom["n_finite"])
    if simultaneous:
        s = sup(tile, se, np.zeros(tile.shape[0]))
        critical = float(np.quantile(s[1:], level))
        out.update(sup=s, critical=critical, lower_simultaneous=out["estimate"] - critical * out["se"],
                   upper_simultaneous=out["estimate"] + critical * out["se"])
    return out
