"""The numpy restatement of csrc/graph_tfce.hip (include/oai_hip.h, "Threshold-free cluster enhancement"), by brute force: for every row
and every level k it runs scipy.sparse.csgraph.connected_components FROM SCRATCH on the edges whose two ends are active at that level and
of the same side, sums the int64 weights of every component with np.add.at, forms the level's term in the header's association and adds
it, levels in descending order, under np.where(active, acc + c, acc).  Nothing is carried from one level to the next but the
accumulator: the kernel's incremental union-find has nothing in common with this file but the definition.  numpy's float64 multiply,
add and sqrt are IEEE and unfused, and int64 -> float64 is exact below 2^53, so the device must give the same bits."""
import numpy as np


def _edges(offsets, neighbours, V):
    """(src, dst) of the CSR adjacency with the header's clamping: offsets into [0, len(neighbours)], neighbours outside [0, V) ignored."""
    offsets, neighbours = np.asarray(offsets, np.int64), np.asarray(neighbours, np.int64)
    lo, hi = np.clip(offsets[:-1], 0, len(neighbours)), np.clip(offsets[1:], 0, len(neighbours))
    src = np.repeat(np.arange(V), np.maximum(hi - lo, 0))
    dst = np.concatenate([neighbours[a:b] for a, b in zip(lo, hi)]) if V else np.zeros(0, np.int64)
    ok = (dst >= 0) & (dst < V) & (dst != src)
    return src[ok], dst[ok]


def tfce(values, offsets, neighbours, dh=0.1, E=1.0, H=2.0, weights=None, unit=1.0, max_steps=1000):
    """(tfce float64 [R, V], clipped int32 [R]) of the float64 ``values`` [R, V]."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    assert E in (0.5, 1.0) and H in (1.0, 2.0) and dh > 0 and unit > 0 and 1 <= max_steps <= 65536
    values = np.atleast_2d(np.asarray(values, np.float64))
    R, V = values.shape
    src, dst = _edges(offsets, neighbours, V)
    w = np.ones(V, np.int64) if weights is None else np.asarray(weights, np.int64)
    dh, unit = float(dh), float(unit)
    levels = np.arange(1, max_steps + 1).astype(np.float64) * dh          # h_k = (double)k * dh
    out, clipped = np.empty((R, V), np.float64), np.zeros(R, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(R):
            t = values[r]
            a = np.abs(t)
            side = np.where(t > 0, 1, np.where(t < 0, -1, 0))
            clipped[r] = int((a >= float(max_steps + 1) * dh).sum())
            acc = np.zeros(V, np.float64)
            inside = side != 0
            top = int((levels <= a[inside].max()).sum()) if inside.any() else 0      # h_k does not decrease: the True entries are a prefix
            for k in range(top, 0, -1):
                h = float(k) * dh
                active = inside & (a >= h)
                keep = active[src] & active[dst] & (side[src] == side[dst])
                g = coo_matrix((np.ones(int(keep.sum()), np.int8), (src[keep], dst[keep])), shape=(V, V))
                n_comp, comp = connected_components(g, directed=False)
                W = np.zeros(n_comp, np.int64)
                np.add.at(W, comp[active], w[active])
                e = W[comp].astype(np.float64) * unit
                eE = e if E == 1.0 else np.sqrt(e)
                hH = h if H == 1.0 else h * h
                c = (eE * hH) * dh
                acc = np.where(active, acc + c, acc)
            out[r] = np.where(np.isnan(t), np.nan, np.where(side < 0, -acc, acc))
    return out, clipped


def path_graph(n):
    """The CSR adjacency of the path 0 - 1 - ... - n-1."""
    if n == 1:
        return np.zeros(2, np.int32), np.zeros(0, np.int32)
    off = np.concatenate([[0], np.cumsum([1] + [2] * (n - 2) + [1])]).astype(np.int32)
    nbr = np.concatenate([[1]] + [[i - 1, i + 1] for i in range(1, n - 1)] + [[n - 2]]).astype(np.int32)
    return off, nbr


def relabel(offsets, neighbours, new_of_old):
    """The CSR adjacency of the same graph with vertex i renamed new_of_old[i] (neighbour lists in ascending new index)."""
    V = len(offsets) - 1
    new_of_old = np.asarray(new_of_old, np.int64)
    old_of_new = np.argsort(new_of_old)
    lists = [np.sort(new_of_old[np.asarray(neighbours[offsets[o]:offsets[o + 1]], np.int64)]) for o in old_of_new]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    nbr = (np.concatenate(lists) if V and off[-1] else np.zeros(0)).astype(np.int32)
    return off, nbr
