"""The restatement of csrc/rank_transform.hip (include/oai_hip.h, "Rank transform"), built a different way from the kernel: per column,
over the valid entries, scipy.stats.rankdata(method="average") on the key, doubled; the tie term from np.unique's counts as the sum of
t^3 - t; the rank sums with numpy; the scores with scipy.special.ndtri.  The kernel counts pairs; nothing here does."""
import numpy as np
import scipy.special
import scipy.stats

CONSTANTS = {"blom": 0.375, "tukey": 1.0 / 3.0, "rankit": 0.5, "waerden": 0.0}


def valid_entries(values, mask=None, signed=False):
    """bool [N, V]: the mask is non-zero (every entry without one), the value is not NaN and, in signed mode, not zero."""
    y = np.asarray(values, np.float32)
    ok = ~np.isnan(y)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    if signed:
        ok &= y != 0
    return ok


def column_ranks(values, mask=None, signed=False):
    """(twice_rank int32 [N, V], n_valid int32 [V], tie_term int64 [V])."""
    y = np.asarray(values, np.float32)
    N, V = y.shape
    ok = valid_entries(y, mask, signed)
    twice = np.zeros((N, V), np.int32)
    n_valid = ok.sum(axis=0).astype(np.int32)
    tie_term = np.zeros(V, np.int64)
    for v in range(V):
        rows = np.nonzero(ok[:, v])[0]
        if len(rows) == 0:
            continue
        col = y[rows, v]
        key = np.abs(col) if signed else col
        rank = scipy.stats.rankdata(key, method="average")
        doubled = np.rint(2.0 * rank).astype(np.int32)
        assert (doubled == 2.0 * rank).all()
        twice[rows, v] = np.where(col < 0, -doubled, doubled) if signed else doubled
        t = np.unique(key, return_counts=True)[1].astype(np.int64)
        tie_term[v] = (t ** 3 - t).sum()
    return twice, n_valid, tie_term


def counted_ranks(values, mask=None, signed=False):
    """The header's counting definition, literally, O(N^2) per column: (twice_rank, sum over valid i of equal_i^2 - 1)."""
    y = np.asarray(values, np.float32)
    N, V = y.shape
    ok = valid_entries(y, mask, signed)
    key = np.abs(y) if signed else y
    twice = np.zeros((N, V), np.int64)
    tie = np.zeros(V, np.int64)
    for v in range(V):
        for i in range(N):
            if not ok[i, v]:
                continue
            less = int(sum(1 for j in range(N) if ok[j, v] and key[j, v] < key[i, v]))
            equal = int(sum(1 for j in range(N) if ok[j, v] and key[j, v] == key[i, v]))
            twice[i, v] = (2 * less + equal + 1) * (-1 if signed and y[i, v] < 0 else 1)
            tie[v] += equal * equal - 1
    return twice.astype(np.int32), tie


def rank_sums(twice_rank, labels=None, n_groups=2):
    """(n_g int32 [G, V], twice_sum_g int64 [G, V]); labels None: group 0 the negative entries, group 1 the positive ones."""
    tr = np.asarray(twice_rank, np.int64)
    N, V = tr.shape
    n_g = np.zeros((n_groups, V), np.int32)
    sums = np.zeros((n_groups, V), np.int64)
    for g in range(n_groups):
        if labels is None:
            member = tr < 0 if g == 0 else tr > 0
        else:
            member = (np.asarray(labels) == g)[:, None] & (tr != 0)
        n_g[g] = member.sum(axis=0)
        sums[g] = (np.abs(tr) * member).sum(axis=0)
    return n_g, sums


def rank_scores(twice_rank, n_valid, kind="rank", c=0.375):
    """(score float64 [N, V], mask uint8 [N, V]); 0.0 where the entry is not valid."""
    tr = np.asarray(twice_rank, np.int32)
    n = np.asarray(n_valid, np.float64)[None, :]
    valid = tr != 0
    if kind == "rank":
        score = 0.5 * tr.astype(np.float64)
    elif kind == "centred":
        score = 0.5 * tr.astype(np.float64) - 0.5 * (n + 1.0)
    else:
        r = 0.5 * np.abs(tr).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            p = (r - c) / ((n - 2.0 * c) + 1.0)
            score = np.where(tr < 0, -1.0, 1.0) * scipy.special.ndtri(np.where(valid, p, 0.5))
    return np.where(valid, score, 0.0), valid.astype(np.uint8)


# ---- the classical statistics, per column over the valid knees -------------------------------------------------------------------------
def mann_whitney_u1(values, mask, group1):
    """U of the knees with ``group1`` True, per vertex (float64 [V]) and (n1, n2)."""
    tr, _, _ = column_ranks(values, mask)
    n_g, sums = rank_sums(tr, np.where(np.asarray(group1, bool), 0, 1), 2)
    n1 = n_g[0].astype(np.float64)
    return 0.5 * sums[0] - 0.5 * n1 * (n1 + 1.0), n_g[0], n_g[1]


def signed_rank_w(values, mask):
    """(W+, W-, n_nonzero) per vertex."""
    tr, n_valid, _ = column_ranks(values, mask, signed=True)
    _, sums = rank_sums(tr, None, 2)
    return 0.5 * sums[1], 0.5 * sums[0], n_valid


def kruskal_h(values, mask, where, n_levels):
    """The tie-corrected H per vertex; NaN where every valid value ties or a level is empty."""
    tr, n_valid, tie = column_ranks(values, mask)
    n_g, sums = rank_sums(tr, where, n_levels)
    n, ng, R = n_valid.astype(np.float64), n_g.astype(np.float64), 0.5 * sums.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = 12.0 / (n * (n + 1.0)) * (R * R / ng).sum(axis=0) - 3.0 * (n + 1.0)
        h = h / (1.0 - tie.astype(np.float64) / (n * n * n - n))
    return np.where((n_g == 0).any(axis=0) | (tie == n * n * n - n), np.nan, h)
