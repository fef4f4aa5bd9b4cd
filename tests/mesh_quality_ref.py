"""numpy restatement of csrc/mesh_quality.hip (not collected): a dict-based edge count for the topology, the figures of oai_mesh_geometry
operation for operation in plain fp64 with the reductions of ordered_reduce_ref.py, and the piercing predicate over all pairs of faces.
IEEE add, subtract, multiply, divide, compare, fmin, fmax and a correctly rounded sqrt are bit-faithful in numpy, so every figure
restated here is the device's bit for bit.  Also the small meshes the tests share."""
import functools

import numpy as np

import ordered_reduce_ref as oref

TOPO = ("faces", "degenerate_faces", "referenced_vertices", "edges", "boundary_edges", "misoriented_edges", "non_manifold_edges", "interface_edges",
        "faces_inner", "faces_unassigned", "faces_outer", "euler_characteristic", "boundary_loops", "interface_loops", "bad_faces", "manifold_edges")
GEO_OPS = ("add", "add", "min", "max", "min", "add", "add", "add", "add", "add", "min", "max", "add", "add")
GEO_CLEAR = np.array([0.0, 0.0, np.inf, -np.inf, np.inf, 0.0, 0.0, 0.0, 0.0, 0.0, np.inf, -np.inf, 0.0, 0.0])
K_Q = 6.928203230275509                    # 4 sqrt 3


def _faces(faces):
    return np.asarray(faces, np.int64).reshape(-1, 3)


def _components(pairs):
    """Connected components of the graph whose edges are ``pairs``, counted over the vertices the edges name."""
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs:
        parent.setdefault(a, a)
        parent.setdefault(b, b)
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return len({find(x) for x in parent})


def topology(faces, n_verts, side=None):
    """(record int64 [16], edge_class uint8 [m, 3]) of oai_mesh_topology."""
    f = _faces(faces)
    m = len(f)
    ok = ((f >= 0) & (f < n_verts)).all(axis=1)
    degenerate = ok & ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0]))
    good = ok & ~degenerate
    edges = {}                                                    # (lo, hi) -> [(half-edge, runs from lo to hi)] in ascending half-edge
    for i in np.flatnonzero(good):
        for k in range(3):
            a, b = int(f[i, k]), int(f[i, (k + 1) % 3])
            edges.setdefault((min(a, b), max(a, b)), []).append((3 * int(i) + k, a < b))
    cls = np.zeros((m, 3), np.uint8)
    count = np.zeros(5, np.int64)
    boundary, interface = [], []
    for key, hs in edges.items():
        owner = hs[0][0]
        c = 1 if len(hs) == 1 else (4 if len(hs) > 2 else (3 if hs[0][1] == hs[1][1] else 2))
        count[c] += 1
        if c == 1:
            boundary.append(key)
        if c == 2 and side is not None and {int(side[hs[0][0] // 3]), int(side[hs[1][0] // 3])} == {-1, 1}:
            c |= 16
            interface.append(key)
        cls[owner // 3, owner % 3] = c
    rec = np.zeros(16, np.int64)
    rec[0], rec[1], rec[14] = m, degenerate.sum(), (~ok).sum()
    rec[2] = len(np.unique(f[good]))
    rec[4], rec[15], rec[5], rec[6] = count[1], count[2], count[3], count[4]
    rec[3] = count[1:].sum()
    rec[7] = len(interface)
    if side is not None:
        s = np.asarray(side).reshape(-1)
        rec[8], rec[9], rec[10] = (s == -1).sum(), (s == 0).sum(), (s == 1).sum()
    rec[11] = rec[2] - rec[3] + good.sum()
    rec[12], rec[13] = _components(boundary), _components(interface)
    return rec, cls


def _det3(u, v, w):
    return (u[..., 0] * (v[..., 1] * w[..., 2] - v[..., 2] * w[..., 1]) - u[..., 1] * (v[..., 0] * w[..., 2] - v[..., 2] * w[..., 0])) + \
        u[..., 2] * (v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0])


def _sq_len(p, q):
    d = q - p
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def face_figures(verts, faces, origin=(0.0, 0.0, 0.0)):
    """Per face (ok, area, q, det, l [m, 3]) as geo_partials_kernel computes them."""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    f = _faces(faces)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    a, b, c = (v[np.where(ok, f[:, k], 0)] if len(v) else np.zeros((len(f), 3)) for k in range(3))
    e1, e2 = b - a, c - a
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    l = np.stack([_sq_len(a, b), _sq_len(b, c), _sq_len(c, a)], axis=1)
    den = (l[:, 0] + l[:, 1]) + l[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(den > 0.0, (K_Q * area) / den, 0.0)
    o = np.asarray(origin, np.float64).reshape(1, 3)
    det = _det3(a - o, b - o, c - o)
    return ok, area, q, det, l


def geometry(verts, faces, edge_class, origin=(0.0, 0.0, 0.0), q_min=0.1):
    """float64 [16] of oai_mesh_geometry, driven the way geo_partials_kernel is: blocks = max(1, min(2048, ceil(m / 1024))), thread g takes
    the faces g, g + 256 blocks, ...; per face its own figures, then its owned half-edges k = 0, 1, 2; block_reduce, one slot row per block,
    the one-block finish."""
    ok, area, q, det, l = face_figures(verts, faces, origin)
    cls = np.asarray(edge_class, np.uint8).reshape(-1, 3)
    m = len(ok)
    blocks = max(1, min(oref.STREAM_BLOCKS, -(-m // (4 * oref.KT))))
    threads = blocks * oref.KT
    acc = np.tile(GEO_CLEAR, (threads, 1))
    for start in range(0, m, threads):
        sl = slice(start, min(start + threads, m))
        t = np.flatnonzero(ok[sl])
        A, Q, D = area[sl][t], q[sl][t], det[sl][t]
        acc[t, 0] = acc[t, 0] + A
        acc[t, 1] = acc[t, 1] + D
        acc[t, 2] = np.fmin(acc[t, 2], A)
        acc[t, 3] = np.fmax(acc[t, 3], A)
        acc[t, 4] = np.fmin(acc[t, 4], Q)
        acc[t, 5] = acc[t, 5] + Q
        low = t[Q < q_min]
        acc[low, 6] = acc[low, 6] + 1.0
        acc[t, 7] = acc[t, 7] + 1.0
        for k in range(3):
            c = cls[sl][:, k]
            e = np.flatnonzero(ok[sl] & (c != 0))
            ln = np.sqrt(l[sl][e, k])
            bd = (c[e] & 15) == 1
            it = (c[e] & 16) != 0
            acc[e[bd], 8] = acc[e[bd], 8] + ln[bd]
            acc[e[it], 9] = acc[e[it], 9] + ln[it]
            acc[e, 10] = np.fmin(acc[e, 10], ln)
            acc[e, 11] = np.fmax(acc[e, 11], ln)
            acc[e, 12] = acc[e, 12] + ln
            acc[e, 13] = acc[e, 13] + 1.0
    a = oref.finish(oref.block_reduce(acc.reshape(blocks, oref.KT, len(GEO_OPS)), GEO_OPS), GEO_CLEAR, GEO_OPS)
    faces_n, edges_n = a[7] > 0.0, a[13] > 0.0
    out = np.zeros(16)
    out[0], out[1], out[2], out[3] = a[0], a[1] / 6.0, a[8], a[9]
    if edges_n:
        out[4], out[5], out[6] = a[10], a[11], a[12] / a[13]
    if faces_n:
        out[7], out[8], out[9], out[10] = a[2], a[3], a[4], a[5] / a[7]
    out[11], out[12], out[13] = a[6], a[13], a[7]
    return out


def _orient(a, b, c, d):
    return _det3(b - a, c - a, d - a)


def _pierces(p, q, a, b, c):
    s1, s2 = _orient(a, b, c, p), _orient(a, b, c, q)
    t1, t2, t3 = _orient(p, q, a, b), _orient(p, q, b, c), _orient(p, q, c, a)
    return (((s1 > 0) & (s2 < 0)) | ((s1 < 0) & (s2 > 0))) & (((t1 > 0) & (t2 > 0) & (t3 > 0)) | ((t1 < 0) & (t2 < 0) & (t3 < 0)))


def self_intersections(verts, faces):
    """(pairs, flag uint8 [m]) by brute force over all pairs f < g without a common vertex index."""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    f = _faces(faces)
    m = len(f)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    tri = v[np.where(ok[:, None], f, 0)] if len(v) else np.zeros((m, 3, 3))
    flag = np.zeros(m, np.uint8)
    pairs = 0
    for i in range(m - 1):
        if not ok[i]:
            continue
        g = np.arange(i + 1, m)
        g = g[ok[g] & ~(f[g][:, :, None] == f[i][None, None, :]).any(axis=(1, 2))]
        if not len(g):
            continue
        P = np.broadcast_to(tri[i], (len(g), 3, 3))
        Q = tri[g]
        hit = np.zeros(len(g), bool)
        for k in range(3):
            hit |= _pierces(P[:, k], P[:, (k + 1) % 3], Q[:, 0], Q[:, 1], Q[:, 2])
            hit |= _pierces(Q[:, k], Q[:, (k + 1) % 3], P[:, 0], P[:, 1], P[:, 2])
        if hit.any():
            pairs += int(hit.sum())
            flag[i] = 1
            flag[g[hit]] = 1
    return pairs, flag


# ---- the meshes -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uv_sphere(stacks=16, slices=24, centre=(0.0, 0.0, 0.0), radius=1.0):
    """A closed UV sphere with outward faces: 2 + (stacks - 1) slices vertices, 2 slices (stacks - 1) faces (16 x 24: 362 and 720)."""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, stacks):
        th = np.pi * i / stacks
        for j in range(slices):
            ph = 2.0 * np.pi * j / slices
            v.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * slices + j % slices
    f = []
    for j in range(slices):
        f.append((0, ring(1, j), ring(1, j + 1)))
    for i in range(1, stacks - 1):
        for j in range(slices):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    south = len(v) - 1
    for j in range(slices):
        f.append((south, ring(stacks - 1, j + 1), ring(stacks - 1, j)))
    verts = (np.asarray(v) * radius + np.asarray(centre)).astype(np.float32)
    faces = np.asarray(f, np.int32)
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


@functools.lru_cache(maxsize=None)
def two_spheres():
    """Two unit spheres at (0, 0, 0) and (1.1, 0.13, 0.07) in one mesh: 724 vertices, 1440 faces, the surfaces cross."""
    (v1, f1), (v2, f2) = uv_sphere(), uv_sphere(centre=(1.1, 0.13, 0.07))
    verts, faces = np.concatenate([v1, v2]), np.concatenate([f1, f2 + len(v1)]).astype(np.int32)
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


@functools.lru_cache(maxsize=None)
def torus(nu=12, nv=20, R=2.0, r=0.7):
    v = [((R + r * np.cos(2 * np.pi * i / nu)) * np.cos(2 * np.pi * j / nv), (R + r * np.cos(2 * np.pi * i / nu)) * np.sin(2 * np.pi * j / nv),
          r * np.sin(2 * np.pi * i / nu)) for i in range(nu) for j in range(nv)]
    idx = lambda i, j: (i % nu) * nv + j % nv
    f = []
    for i in range(nu):
        for j in range(nv):
            f.append((idx(i, j), idx(i, j + 1), idx(i + 1, j + 1)))
            f.append((idx(i, j), idx(i + 1, j + 1), idx(i + 1, j)))
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def fan(n_faces, seed=3):
    """``n_faces`` triangles around vertex 0: an open disc whose hub has valence n_faces + 1, rim points at slightly varied radii."""
    rng = np.random.default_rng([seed, n_faces])
    ang = 2.0 * np.pi * np.arange(n_faces + 1) / (n_faces + 1)
    rad = 1.0 + 0.2 * rng.uniform(size=n_faces + 1)
    v = np.concatenate([[(0.0, 0.0, 0.0)], np.stack([rad * np.cos(ang), rad * np.sin(ang), 0.1 * rng.uniform(size=n_faces + 1)], axis=1)])
    f = [(0, 1 + k, 2 + k) for k in range(n_faces)]
    return v.astype(np.float32), np.asarray(f, np.int32).reshape(-1, 3)


def cube():
    """The cube [-1, 1]^3 on 12 outward faces: every coordinate and every product is exact."""
    v = np.array([(x, y, z) for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float32)
    f = np.array([(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5)],
                 np.int32)
    return v, f


def equator_side(faces, verts, island=False):
    """int8 per face of a sphere: +1 where the centroid is above the equator, -1 below; ``island``: one face and its edge neighbours far
    inside the upper half flipped to -1, a second interface loop."""
    cz = np.asarray(verts, np.float64)[np.asarray(faces)].mean(axis=1)[:, 2]
    side = np.where(cz > 0.0, 1, -1).astype(np.int8)
    if island:
        side[np.argsort(-cz)[:24]] = -1                           # the polar cap of 24 faces: a closed patch around the north pole
    return side
