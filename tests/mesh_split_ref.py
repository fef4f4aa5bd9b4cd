"""numpy restatement of the inner / outer split (mesh_processing.py:197-294) that csrc/mesh_split.hip implements (not collected).

KMeans(n_clusters=2, algorithm="lloyd") as scikit-learn >= 1.4 runs it (_kmeans.py: fit, _kmeans_plusplus, _kmeans_single_lloyd) on
dense fp64 features with unit sample weights.  tests/test_mesh_split_cpu.py checks it against the installed sklearn and against the
reference's own split functions (tests/golden/mesh_split.npz).

kmeans_draws() takes the random numbers of a fit as arguments, as oai_mesh_split_kmeans does, and returns with the fit the evidence
that the fit is decided in fp64: how far every comparison the fit makes is from going the other way (Evidence).  A device result
may be compared face for face with this restatement wherever those margins are far above the rounding of an fp64 sum."""
from dataclasses import dataclass, field

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


@dataclass
class Evidence:
    """How far the comparisons of one fit (all its inits) are from going the other way; inf where a comparison cannot matter.
    label_margin      min |d0 - d1| over the samples of every E-step (all inits, all iterations, the final E-step)
    candidate_margin  min |cumsum_i - r| / pot over the two draws of every init and the i that decide a candidate: not i = n - 1
                      (a search that ends at n is clipped to n - 1 either way), and none for r = 0 (no distance is negative, so
                      the candidate is sample 0 whatever the rounding)
    trial_margin      min |pot_a - pot_b| / pot between the two local trials of an init whose candidates differ
    tol_margin        min |shift^2 - tol| / tol over the iterations that reach the tolerance test
    inertia_gap       min |I_a - I_b| / max(I_a, I_b) over the pairs of inits that are not the same clustering
    stops             how each init ended: "strict" (labels unchanged), "tol" (shift^2 <= tol) or "max_iter"
    n_iters           the iterations of each init;  best: the init fit() keeps
    raw_candidates    searchsorted's answers before the clip (n: the clip acted);  draws: (first centre, u0, u1) of each init"""
    label_margin: float = np.inf
    candidate_margin: float = np.inf
    trial_margin: float = np.inf
    tol_margin: float = np.inf
    inertia_gap: float = np.inf
    stops: list = field(default_factory=list)
    n_iters: list = field(default_factory=list)
    best: int = 0
    raw_candidates: list = field(default_factory=list)
    draws: list = field(default_factory=list)
    flipped: bool = False
    flip_margin: float = np.inf                       # |mean n_y over side -1| (orientation())


def kmeans_plusplus(X, xx, c0, u, ev=None):
    """_kmeans_plusplus for two clusters with the draws given: c0 = rs.choice(n, p=w / w.sum()), u = rs.uniform(size=2)"""
    n = len(X)
    w = np.ones(n)
    d = _sqdist(X[c0], X, xx)[0]
    pot = d @ w
    r = np.asarray(u, np.float64) * pot
    cum = np.cumsum(w * d)
    raw = np.searchsorted(cum, r)
    cand = np.minimum(raw, n - 1)
    dc = np.minimum(d, _sqdist(X[cand], X, xx))
    pots = dc @ w
    best = int(np.argmin(pots))
    if ev is not None:
        ev.raw_candidates.append([int(t) for t in raw])
        ev.draws.append((int(c0), float(u[0]), float(u[1])))
        if pot > 0:
            for rt in r:
                if rt > 0 and n > 1:
                    ev.candidate_margin = min(ev.candidate_margin, float(np.abs(cum[:-1] - rt).min() / pot))
            if cand[0] != cand[1]:
                ev.trial_margin = min(ev.trial_margin, float(abs(pots[0] - pots[1]) / pot))
    return np.stack([X[c0], X[cand[best]]])


def _e_step(X, c, ev=None):
    d = (c ** 2).sum(axis=1)[None, :] - 2 * (X @ c.T)
    if ev is not None:
        ev.label_margin = min(ev.label_margin, float(np.abs(d[:, 0] - d[:, 1]).min()))
    return np.argmin(d, axis=1)                                                    # the first centre on a tie


def lloyd(X, centres, max_iter, tol, ev=None):
    """_kmeans_single_lloyd: (labels, n_iter, inertia, centres, stopped_strictly)"""
    old = np.full(len(X), -1)
    strict = False
    stop = "max_iter"
    c = centres.copy()
    for i in range(max_iter):
        labels = _e_step(X, c, ev)
        cnt = np.bincount(labels, minlength=2).astype(np.float64)
        if (cnt == 0).any():
            raise RuntimeError("a cluster became empty (sklearn relocates a point; not restated)")
        new = np.stack([X[labels == j].sum(axis=0) * (1.0 / cnt[j]) for j in range(2)])
        shift = np.sqrt(((new - c) ** 2).sum(axis=1))
        c = new
        if np.array_equal(labels, old):
            strict = True
            stop = "strict"
            break
        if ev is not None and tol > 0:
            ev.tol_margin = min(ev.tol_margin, float(abs((shift ** 2).sum() - tol) / tol))
        if (shift ** 2).sum() <= tol:
            stop = "tol"
            break
        old = labels
    if not strict:
        labels = _e_step(X, c, ev)
    inertia = ((X - c[labels]) ** 2).sum()
    if ev is not None:
        ev.stops.append(stop)
        ev.n_iters.append(i + 1)
    return labels, i + 1, inertia, c, strict


def same_clustering(a, b):
    """_is_same_clustering(a, b, 2)"""
    mapping = [-1, -1]
    for lab in (0, 1):
        idx = np.flatnonzero(a == lab)
        if len(idx):
            mapping[lab] = b[idx[0]]
    return bool(np.all(b == np.where(a == 1, mapping[1], mapping[0])))


def draws(n, n_init, seed=5):
    """What KMeans(random_state=seed).fit draws on n samples: per init rs.choice(n, p=w / w.sum()), then rs.uniform(size=2)"""
    rs = np.random.RandomState(seed)
    w = np.ones(n)
    first, uniforms = [], []
    for _ in range(n_init):
        first.append(int(rs.choice(n, p=w / w.sum())))
        uniforms.append(rs.uniform(size=2))
    return first, np.array(uniforms).reshape(n_init, 2)


def kmeans_draws(X, first, uniforms, n_init=None, max_iter=300, tol=1e-4):
    """KMeans(2, algorithm="lloyd", n_init=n_init, max_iter=max_iter, tol=tol).fit(X) with the draws of each init given (what
    oai_mesh_split_kmeans takes): first[r] the first k-means++ centre, uniforms[r] the two uniforms in [0, 1) of its local trials.
    Returns (labels, n_iter, inertia, centres + mean, strict, Evidence)."""
    X = np.array(X, dtype=np.float64)
    if len(X) < 2:
        raise ValueError(f"n_samples={len(X)} should be >= n_clusters=2.")
    n_init = len(first) if n_init is None else n_init
    uniforms = np.asarray(uniforms, np.float64).reshape(-1, 2)
    tol_abs = np.mean(np.var(X, axis=0)) * tol
    mean = X.mean(axis=0)
    X -= mean
    xx = np.einsum("ij,ij->i", X, X)
    ev = Evidence()
    runs = []
    best = None
    for r in range(n_init):
        res = lloyd(X, kmeans_plusplus(X, xx, int(first[r]), uniforms[r], ev), max_iter, tol_abs, ev)
        runs.append(res)
        if best is None or (res[2] < best[2] and not same_clustering(res[0], best[0])):
            best = res
            ev.best = r
    for a in range(n_init):
        for b in range(a + 1, n_init):
            if not same_clustering(runs[b][0], runs[a][0]):
                ia, ib = runs[a][2], runs[b][2]
                ev.inertia_gap = min(ev.inertia_gap, float(abs(ia - ib) / max(ia, ib)) if max(ia, ib) > 0 else 0.0)
    labels, n_iter, inertia, c, strict = best
    return labels, n_iter, inertia, c + mean, strict, ev


def kmeans(X, n_init, seed=5, max_iter=300, tol=1e-4):
    """KMeans(2, algorithm="lloyd", n_init=n_init, random_state=seed).fit(X): (labels, n_iter, inertia, centres + mean, strict)"""
    if len(X) < 2:
        raise ValueError(f"n_samples={len(X)} should be >= n_clusters=2.")
    first, uniforms = draws(len(X), n_init, seed)
    return kmeans_draws(X, first, uniforms, n_init, max_iter, tol)[:5]


def flip_mean(labels, ny):
    """the mean normal y of side -1 (label 0); None if that side is empty"""
    sel = ny[np.asarray(labels) == 0]
    return float(sel.mean()) if len(sel) else None


def orient(labels, ny):
    """labels * 2 - 1, flipped if the mean normal y of side -1 is negative (:212-217, :234-238)"""
    io = labels * 2 - 1
    m = flip_mean(labels, ny)
    if m is not None and m < 0:
        io = -io
    return io


def slab_masks(x):
    """The half-open x slabs of :259-270 on the normalised centroid x: (masks [3, n], faces in no slab, faces in two slabs).
    lower_s and lower_s + step are rounded one by one, so that a face can fall between two slabs, or at a seam into both."""
    min_x, max_x = np.min(x), np.max(x)
    step = (max_x - min_x) / N_DIVISIONS
    masks = []
    for i in range(N_DIVISIONS):
        lower = min_x + step * i
        masks.append((x >= lower) & (x < lower + step))
    masks = np.array(masks)
    held = masks.sum(axis=0)
    return masks, np.flatnonzero(held == 0), np.flatnonzero(held > 1)


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
    return f, slab_masks(cn[:, 0])[0], n


def split_sides_draws(verts, faces, mesh_type="FC", n_init=None, max_iter=300, slab_draws=None):
    """split_sides with each slab's draws given (slab_draws[s] = (first, uniforms); None: RandomState(5)'s, as the product draws
    them): (side, n_iter per slab, Evidence per slab).  A face in two slabs takes the later slab's side (np.put in slab order)."""
    f, masks, n = features(verts, faces, mesh_type)
    n_init = (5 if mesh_type == "FC" else 1) if n_init is None else n_init
    side = np.zeros(len(f), np.int8)
    n_iter, evidence = [], []
    for s, m in enumerate(masks):
        idx = np.flatnonzero(m)
        if len(idx) < 2:
            raise ValueError(f"n_samples={len(idx)} should be >= n_clusters=2.")
        first, uniforms = slab_draws[s] if slab_draws is not None else draws(len(idx), n_init)
        labels, it, _, _, _, ev = kmeans_draws(f[idx], first, uniforms, n_init, max_iter)
        m_y = flip_mean(labels, n[idx, 1])
        ev.flipped = m_y is not None and m_y < 0
        ev.flip_margin = abs(m_y) if m_y is not None else np.inf
        side[idx] = orient(labels, n[idx, 1])
        n_iter.append(it)
        evidence.append(ev)
    return side, np.array(n_iter), evidence


def split_sides(verts, faces, mesh_type="FC"):
    """side per face (int8, -1 inner / +1 outer / 0 in no slab) and each fit's n_iter"""
    side, n_iter, _ = split_sides_draws(verts, faces, mesh_type)
    return side, n_iter


def sub_mesh(verts, faces, face_list):
    """get_vtk_sub_mesh: the faces in list order, vertices in order of first use, remapped"""
    f = faces[np.asarray(face_list, dtype=np.int64)]
    flat = f.reshape(-1)
    uniq, first = np.unique(flat, return_index=True)
    order = uniq[np.argsort(first)]
    remap = np.full(len(verts), -1, dtype=np.int64)
    remap[order] = np.arange(len(order))
    return verts[order], remap[f].astype(np.int32)
