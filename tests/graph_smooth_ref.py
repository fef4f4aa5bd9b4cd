"""The numpy restatement of csrc/graph_smooth.hip (include/oai_hip.h, "Surface smoothing"): K sweeps of normalised neighbourhood averaging
of every row of a float64 tile on a weighted CSR graph under a validity mask.  ``smooth`` is vectorised over rows and vertices and loops
over the sweeps and over the neighbour SLOT 0 .. maxdeg - 1, so that every vertex still adds its neighbours in ascending CSR position with
one accumulator; an entry that is skipped is skipped by np.where, never multiplied by 0.  ``smooth_loop`` is the header's rule written
out as a plain Python loop per row and vertex, for tiny graphs: the two must agree to the bit.  numpy's float64 multiply, add and divide
are IEEE and unfused, so the device must give the same bits.  The graphs the tests use are built here as well."""
import numpy as np


def _csr(offsets, neighbours, V):
    """(lo, count, nbr): the offsets clamped into [0, E] as the header says."""
    off, nbr = np.asarray(offsets, np.int64), np.asarray(neighbours, np.int64)
    assert len(off) == V + 1
    lo, hi = np.clip(off[:-1], 0, len(nbr)), np.clip(off[1:], 0, len(nbr))
    return lo, np.maximum(hi - lo, 0), nbr


def smooth(values, mask, offsets, neighbours, edge_weight, self_weight=None, sweeps=1, fill=False):
    """(values float64 [R, V] with +0.0 where the result is missing, mask uint8 [R, V]) after ``sweeps`` sweeps."""
    x = np.atleast_2d(np.asarray(values, np.float64))
    R, V = x.shape
    m = np.ones((R, V), bool) if mask is None else np.atleast_2d(np.asarray(mask)) != 0
    lo, count, nbr = _csr(offsets, neighbours, V)
    w = np.asarray(edge_weight, np.float64)
    assert len(w) == len(nbr) and 1 <= sweeps <= 4096
    sw = np.ones(V) if self_weight is None else np.asarray(self_weight, np.float64)
    x = np.where(m, x, 0.0)
    maxdeg = int(count.max()) if V else 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _ in range(int(sweeps)):
            num, den = np.zeros((R, V)), np.zeros((R, V))
            num, den = np.where(m, num + sw[None, :] * x, num), np.where(m, den + sw[None, :], den)
            for s in range(maxdeg):
                has = count > s
                e = np.where(has, lo + s, 0)
                j = nbr[e] if len(nbr) else np.zeros(V, np.int64)
                has = has & (j >= 0) & (j < V)
                j = np.where(has, j, 0)
                we = w[e] if len(w) else np.zeros(V)
                take = has[None, :] & m[:, j]
                num, den = np.where(take, num + we[None, :] * x[:, j], num), np.where(take, den + we[None, :], den)
            ok = (m | bool(fill)) & (den > 0)
            x, m = np.where(ok, num / np.where(ok, den, 1.0), 0.0), ok
    return x, m.astype(np.uint8)


def smooth_loop(values, mask, offsets, neighbours, edge_weight, self_weight=None, sweeps=1, fill=False):
    """The same by the header's rule, one Python float at a time."""
    x = np.atleast_2d(np.asarray(values, np.float64)).copy()
    R, V = x.shape
    m = np.ones((R, V), bool) if mask is None else np.atleast_2d(np.asarray(mask)) != 0
    E = len(neighbours)
    for _ in range(int(sweeps)):
        xn, mn = np.zeros((R, V)), np.zeros((R, V), bool)
        for r in range(R):
            for i in range(V):
                num, den = 0.0, 0.0
                if m[r, i]:
                    sw = 1.0 if self_weight is None else float(self_weight[i])
                    num, den = num + sw * float(x[r, i]), den + sw
                for e in range(max(int(offsets[i]), 0), min(int(offsets[i + 1]), E)):
                    j = int(neighbours[e])
                    if 0 <= j < V and m[r, j]:
                        num, den = num + float(edge_weight[e]) * float(x[r, j]), den + float(edge_weight[e])
                ok = (bool(fill) or m[r, i]) and den > 0
                xn[r, i], mn[r, i] = (num / den if ok else 0.0), ok
        x, m = xn, mn
    return x, m.astype(np.uint8)


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------
def from_lists(lists):
    """(offsets int32 [V + 1], neighbours int32) of per-vertex neighbour lists, kept in the order given."""
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    nbr = np.asarray([j for x in lists for j in x], np.int32)
    return off, nbr


def path_graph(n):
    """The path 0 - 1 - ... - n-1."""
    return from_lists([[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)])


def star_graph(leaves):
    """Vertex 0 is the hub of ``leaves`` leaves 1 .. leaves; a leaf's only neighbour is the hub."""
    return from_lists([list(range(1, leaves + 1))] + [[0]] * leaves)


def triangular_lattice(n):
    """(verts float64 [n * n, 3], offsets, neighbours) of an n x n patch of the unit triangular lattice: vertex r * n + c sits at
    (c + r / 2, r * sqrt(3) / 2, 0) and has up to six neighbours at distance 1, listed in ascending index."""
    verts = np.array([(c + 0.5 * r, r * np.sqrt(3.0) / 2.0, 0.0) for r in range(n) for c in range(n)])
    lists = []
    for r in range(n):
        for c in range(n):
            around = [(r - 1, c), (r - 1, c + 1), (r, c - 1), (r, c + 1), (r + 1, c - 1), (r + 1, c)]
            lists.append(sorted(rr * n + cc for rr, cc in around if 0 <= rr < n and 0 <= cc < n))
    return (verts,) + from_lists(lists)


def icosphere(level):
    """(verts float32 [n, 3] on the unit sphere, faces int32 [m, 3]): 42 vertices at level 1, 642 at level 3."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def face_adjacency(n_verts, faces):
    """(offsets, neighbours) of a triangle mesh: every vertex' distinct neighbours in ascending index."""
    around = [set() for _ in range(n_verts)]
    for a, b, c in np.asarray(faces).tolist():
        around[a] |= {b, c}
        around[b] |= {a, c}
        around[c] |= {a, b}
    return from_lists([sorted(s) for s in around])
