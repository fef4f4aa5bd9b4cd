"""numpy restatement of the inner / outer split (mesh_processing.py:197-294) that csrc/mesh_split.hip implements (not collected).

KMeans(n_clusters=2, algorithm="lloyd") as scikit-learn >= 1.4 runs it (_kmeans.py: fit, _kmeans_plusplus, _kmeans_single_lloyd) on
dense fp64 features with unit sample weights.  tests/test_mesh_split_cpu.py checks it against the installed sklearn and against the
reference's own split functions (tests/golden/mesh_split.npz)."""
import numpy as np

N_DIVISIONS = 3


def cell_centroids(verts, faces):
    v = np.asarray(verts, np.float32).astype(np.float64)
    return v[faces].sum(axis=1) / 3.0


def cell_normals(verts, faces):
    v = np.asarray(verts, np.float32).astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = np.cross(b - a, c - a)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return n / np.where(length > 0, length, 1.0)


def _sqdist(c, X, xx):
    """_euclidean_distances(c, X, Y_norm_squared=xx, squared=True)"""
    d = -2 * (np.atleast_2d(c) @ X.T)
    d += (np.atleast_2d(c) ** 2).sum(axis=1)[:, None]
    d += xx[None, :]
    return np.maximum(d, 0)


def kmeans_plusplus(X, xx, rs):
    n = len(X)
    w = np.ones(n)
    c0 = rs.choice(n, p=w / w.sum())
    d = _sqdist(X[c0], X, xx)[0]
    pot = d @ w
    r = rs.uniform(size=2) * pot
    cand = np.minimum(np.searchsorted(np.cumsum(w * d), r), n - 1)
    dc = np.minimum(d, _sqdist(X[cand], X, xx))
    best = int(np.argmin(dc @ w))
    return np.stack([X[c0], X[cand[best]]])


def lloyd(X, centres, max_iter, tol):
    """_kmeans_single_lloyd: (labels, n_iter, inertia, centres, stopped_strictly)"""
    old = np.full(len(X), -1)
    strict = False
    c = centres.copy()
    for i in range(max_iter):
        labels = np.argmin((c ** 2).sum(axis=1)[None, :] - 2 * (X @ c.T), axis=1)   # the first centre on a tie
        cnt = np.bincount(labels, minlength=2).astype(np.float64)
        if (cnt == 0).any():
            raise RuntimeError("a cluster became empty (sklearn relocates a point; not restated)")
        new = np.stack([X[labels == j].sum(axis=0) * (1.0 / cnt[j]) for j in range(2)])
        shift = np.sqrt(((new - c) ** 2).sum(axis=1))
        c = new
        if np.array_equal(labels, old):
            strict = True
            break
        if (shift ** 2).sum() <= tol:
            break
        old = labels
    if not strict:
        labels = np.argmin((c ** 2).sum(axis=1)[None, :] - 2 * (X @ c.T), axis=1)
    inertia = ((X - c[labels]) ** 2).sum()
    return labels, i + 1, inertia, c, strict


def same_clustering(a, b):
    """_is_same_clustering(a, b, 2)"""
    mapping = [-1, -1]
    for lab in (0, 1):
        idx = np.flatnonzero(a == lab)
        if len(idx):
            mapping[lab] = b[idx[0]]
    return bool(np.all(b == np.where(a == 1, mapping[1], mapping[0])))


def kmeans(X, n_init, seed=5, max_iter=300, tol=1e-4):
    """KMeans(2, algorithm="lloyd", n_init=n_init, random_state=seed).fit(X): (labels, n_iter, inertia, centres + mean, strict)"""
    X = np.array(X, dtype=np.float64)
    if len(X) < 2:
        raise ValueError(f"n_samples={len(X)} should be >= n_clusters=2.")
    tol_abs = np.mean(np.var(X, axis=0)) * tol
    mean = X.mean(axis=0)
    X -= mean
    xx = np.einsum("ij,ij->i", X, X)
    rs = np.random.RandomState(seed)
    best = None
    for _ in range(n_init):
        res = lloyd(X, kmeans_plusplus(X, xx, rs), max_iter, tol_abs)
        if best is None or (res[2] < best[2] and not same_clustering(res[0], best[0])):
            best = res
    labels, n_iter, inertia, c, strict = best
    return labels, n_iter, inertia, c + mean, strict


def orient(labels, ny):
    """labels * 2 - 1, flipped if the mean normal y of side -1 is negative (:212-217, :234-238)"""
    io = labels * 2 - 1
    sel = ny[io == -1]
    if len(sel) and sel.mean() < 0:
        io = -io
    return io


def features(verts, faces, mesh_type):
    """(features [n, 6 | 9], slab masks [S, n], normals): cn = (c - mean c) / (max c - min c); TC [cn, 10 n]; FC [cn, n, (centre - c) n]
    with centre the midpoint of the float32 vertex bounds taken in float32 (Mesh.GetBounds), slabs lower <= cn_x < lower + step"""
    c, n = cell_centroids(verts, faces), cell_normals(verts, faces)
    cn = (c - np.mean(c, axis=0)) / (np.max(c, axis=0) - np.min(c, axis=0))
    if mesh_type != "FC":
        return np.concatenate((cn * 1, n * 10), axis=1), np.ones((1, len(c)), bool), n
    v = np.asarray(verts, np.float32)
    centre = (v.min(axis=0) + v.max(axis=0)) / np.float32(2)
    f = np.concatenate((cn * 1, n, np.multiply(centre - c, n)), axis=1)
    x = cn[:, 0]
    min_x, max_x = np.min(x), np.max(x)
    step = (max_x - min_x) / N_DIVISIONS
    masks = []
    for i in range(N_DIVISIONS):
        lower = min_x + step * i
        masks.append((x >= lower) & (x < lower + step))
    return f, np.array(masks), n


def split_sides(verts, faces, mesh_type="FC"):
    """side per face (int8, -1 inner / +1 outer / 0 in no slab) and each fit's n_iter"""
    f, masks, n = features(verts, faces, mesh_type)
    side = np.zeros(len(f), np.int8)
    n_iter = []
    for m in masks:
        idx = np.flatnonzero(m)
        labels, it, _, _, _ = kmeans(f[idx], 5 if mesh_type == "FC" else 1)
        side[idx] = orient(labels, n[idx, 1])
        n_iter.append(it)
    return side, np.array(n_iter)


def sub_mesh(verts, faces, face_list):
    """get_vtk_sub_mesh: the faces in list order, vertices in order of first use, remapped"""
    f = faces[np.asarray(face_list, dtype=np.int64)]
    flat = f.reshape(-1)
    uniq, first = np.unique(flat, return_index=True)
    order = uniq[np.argsort(first)]
    remap = np.full(len(verts), -1, dtype=np.int64)
    remap[order] = np.arange(len(order))
    return verts[order], remap[f].astype(np.int32)
