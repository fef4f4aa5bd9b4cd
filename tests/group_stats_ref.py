"""The numpy restatement of csrc/group_stats.hip (include/oai_hip.h, "Cohort statistics"), operation for operation: every sum over knees
is a sequential ``for i in range(N)`` with one float64 accumulator that starts at +0.0 (vectorised over rows and vertices, which are
independent), a knee that does not take part adds +0.0, and every expression is written in the header's association.  numpy's float64
add, subtract, multiply, divide and sqrt are IEEE and unfused, as the device's are without contraction.  Clusters come from
scipy.sparse.csgraph.connected_components, relabelled to the smallest vertex index."""
import numpy as np

TWO_SAMPLE, ONE_SAMPLE = 0, 1


def pack_bits(rows):
    """bool / 0-1 [P, N] -> uint32 [P, ceil(N / 32)]: knee i of row p is bit i % 32 of word i // 32."""
    rows = np.asarray(rows).astype(bool)
    P, N = rows.shape
    padded = np.zeros((P, (N + 31) // 32 * 32), np.uint64)
    padded[:, :N] = rows
    words = (padded.reshape(P, -1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2)
    return words.astype(np.uint32)


def unpack_bits(bits, n_knees):
    bits = np.asarray(bits).view(np.uint32) if np.asarray(bits).dtype == np.int32 else np.asarray(bits, np.uint32)
    rows = (bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return rows.reshape(bits.shape[0], -1)[:, :n_knees].astype(bool)


def prepare(Y, mask=None, centre=True):
    """dict of n (int32 [V]), mean, std, S, Q (float64 [V]) and C, Qm (float64 [N, V])."""
    Y = np.asarray(Y, np.float32)
    N, V = Y.shape
    m = np.ones((N, V), bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(all="ignore"):
        y = np.where(m, Y.astype(np.float64), 0.0)
        n = np.zeros(V, np.int32)
        total = np.zeros(V, np.float64)
        for i in range(N):
            n = n + m[i]
            total = total + y[i]
        mean = total / n.astype(np.float64)
        C, Qm = np.empty((N, V), np.float64), np.empty((N, V), np.float64)
        S, Q, qd = np.zeros(V, np.float64), np.zeros(V, np.float64), np.zeros(V, np.float64)
        for i in range(N):
            d = np.where(m[i], y[i] - mean, 0.0)
            c = d if centre else y[i]
            cc = c * c
            C[i], Qm[i] = c, cc
            S = S + c
            Q = Q + cc
            qd = qd + d * d
        std = np.where(n >= 2, np.sqrt(qd / (n - 1).astype(np.float64)), np.nan)
    return {"n": n.astype(np.int32), "mean": mean, "std": std, "S": S, "Q": Q, "C": C, "Qm": Qm}


def permutation_t(prep, mask, bits, mode):
    """float64 [P, V]: the t of every row of ``bits`` (packed, or bool [P, N]), NaN where it is not valid."""
    C, Qm, n, S, Q = prep["C"], prep["Qm"], prep["n"], prep["S"], prep["Q"]
    N, V = C.shape
    rows = np.asarray(bits)
    b = rows.astype(bool) if rows.dtype == bool else unpack_bits(rows, N)
    P = b.shape[0]
    m = np.ones((N, V), bool) if mask is None else np.asarray(mask) != 0
    nd = n.astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == TWO_SAMPLE:
            n1 = np.zeros((P, V), np.int64)
            S1, Q1 = np.zeros((P, V), np.float64), np.zeros((P, V), np.float64)
            for i in range(N):
                bi = b[:, i, None]
                S1 = S1 + np.where(bi, C[i][None, :], 0.0)
                Q1 = Q1 + np.where(bi, Qm[i][None, :], 0.0)
                n1 = n1 + (bi & m[i][None, :])
            n2 = n[None, :].astype(np.int64) - n1
            n1d, n2d = n1.astype(np.float64), n2.astype(np.float64)
            S2, Q2 = S[None, :] - S1, Q[None, :] - Q1
            ss = (Q1 - S1 * S1 / n1d) + (Q2 - S2 * S2 / n2d)
            sp2 = ss / (n[None, :] - 2).astype(np.float64)
            t = (S1 / n1d - S2 / n2d) / np.sqrt(sp2 * (1.0 / n1d + 1.0 / n2d))
            ok = (n1 >= 2) & (n2 >= 2) & (sp2 > 0.0)
        else:
            Sf = np.zeros((P, V), np.float64)
            for i in range(N):
                Sf = Sf + np.where(b[:, i, None], -C[i][None, :], C[i][None, :])
            var = (Q[None, :] - Sf * Sf / nd[None, :]) / (n[None, :] - 1).astype(np.float64)
            t = (Sf / nd[None, :]) / np.sqrt(var / nd[None, :])
            ok = (n[None, :] >= 2) & (var > 0.0)
        return np.where(ok, t, np.nan)


def reduce_tiles(t):
    """(max_abs float64 [P], exceed int64 [V]) of the whole t matrix [P, V], row 0 observed."""
    a = np.abs(t)
    max_abs = np.where(np.isnan(a), 0.0, a).max(axis=1)
    with np.errstate(invalid="ignore"):
        exceed = (a >= a[0][None, :]).sum(axis=0).astype(np.int64)        # a comparison with NaN is False
    return max_abs, exceed


def clusters(values, offsets, neighbours, t0):
    """(label int32 [R, V], size int32 [R, V], max_extent int32 [R]).  The CSR adjacency is read as the header states it: an offset outside
    [0, len(neighbours)] is clamped, a neighbour outside [0, V) or equal to its owner is ignored."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    values = np.atleast_2d(np.asarray(values, np.float64))
    R, V = values.shape
    offsets, neighbours = np.asarray(offsets, np.int64), np.asarray(neighbours, np.int64)
    lo, hi = np.clip(offsets[:-1], 0, len(neighbours)), np.clip(offsets[1:], 0, len(neighbours))
    src = np.repeat(np.arange(V), np.maximum(hi - lo, 0))
    dst = np.concatenate([neighbours[a:b] for a, b in zip(lo, hi)] + [np.zeros(0, np.int64)])
    ok = (dst >= 0) & (dst < V) & (dst != src)
    src, dst = src[ok], dst[ok]
    label, size, extent = np.full((R, V), -1, np.int32), np.zeros((R, V), np.int32), np.zeros(R, np.int32)
    for r in range(R):
        with np.errstate(invalid="ignore"):
            side = np.where(values[r] > t0, 1, np.where(values[r] < -t0, -1, 0))
        keep = (side[src] != 0) & (side[src] == side[dst])
        g = coo_matrix((np.ones(int(keep.sum()), np.int8), (src[keep], dst[keep])), shape=(V, V))
        _, comp = connected_components(g, directed=False)
        inside = np.nonzero(side != 0)[0]
        if len(inside) == 0:
            continue
        smallest = np.full(comp.max() + 1, V, np.int64)
        np.minimum.at(smallest, comp[inside], inside)
        label[r, inside] = smallest[comp[inside]]
        counts = np.bincount(comp[inside], minlength=comp.max() + 1)
        size[r, inside] = counts[comp[inside]]
        extent[r] = counts.max()
    return label, size, extent


def hostile_graph(V=40):
    """(offsets int32 [V + 1], neighbours int32) of a symmetric random graph on the vertices 1 .. V - 2 that is then bent in every way the
    header allows for: offsets[0] below 0 and offsets[V] beyond the neighbour count (vertices 0 and V - 1 have no neighbour: after the
    clamp their ranges are empty), and among the neighbours of vertex 5 a negative index, V itself, V + 1 and vertex 5.  What is left
    after the clamp is the symmetric graph."""
    rng = np.random.default_rng(V)
    lists = [[] for _ in range(V)]
    for a, b in rng.integers(1, V - 1, (3 * V // 2, 2)).tolist():
        if a != b and b not in lists[a]:
            lists[a].append(b)
            lists[b].append(a)
    lists[5] = [-1] + lists[5][:1] + [V, 5] + lists[5][1:] + [V + 1]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    nbr = np.asarray([u for x in lists for u in x], np.int32)
    assert not lists[0] and not lists[V - 1] and len(lists[5]) > 4
    off[0], off[V] = -3, off[V] + 5
    return off, nbr
