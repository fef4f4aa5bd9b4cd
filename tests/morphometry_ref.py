"""numpy restatement of the cartilage-morphometry primitives (csrc/morphometry.hip and oai_point_footprint of csrc/thickness_map.hip),
operation for operation in plain fp64 (not collected).  IEEE add, multiply, compare, min, max and a correctly rounded sqrt are
bit-faithful in numpy, so every figure restated here is the device's bit for bit, and a reordered sum on the device shows."""
import numpy as np

import ordered_reduce_ref as oref
from thickness_map_ref import pairwise_d2

SLOTS = 12
REGION_OPS = ("add",) * 8 + ("min", "max", "add", "add")
REGION_CLEAR = np.array([0.0] * 8 + [np.inf, -np.inf, 0.0, 0.0])


def face_areas(verts, faces):
    """face_area float64 [m]: 0.5 * sqrt((cx*cx + cy*cy) + cz*cz) of e1 x e2; NaN for a face with an index outside [0, n)."""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    a, b, c = (v[np.where(ok, f[:, k], 0)] for k in range(3))
    e1, e2 = b - a, c - a
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    with np.errstate(invalid="ignore"):
        area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    return np.where(ok, area, np.nan)


def vertex_areas(n_verts, faces, face_area, descending=False):
    """vertex_area float64 [n]: per vertex the areas of the corners that name it, added one by one in ascending corner index 3 f + k
    (``descending``: the other way round, for the test that the order shows), then divided by 3.0."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < n_verts)).all(axis=1)
    corner = np.flatnonzero(np.repeat(ok, 3))
    corner = corner[::-1] if descending else corner
    vert = f.reshape(-1)[corner]
    order = np.argsort(vert, kind="stable")                      # by vertex; inside a vertex the corners keep their order
    vert, area = vert[order], np.asarray(face_area, np.float64)[corner[order] // 3]
    rank = np.arange(len(vert)) - np.searchsorted(vert, vert, side="left")
    out = np.zeros(n_verts)
    for k in range(int(rank.max()) + 1 if len(rank) else 0):      # step k: every vertex adds its k-th corner
        sel = rank == k
        out[vert[sel]] = out[vert[sel]] + area[sel]
    return out / 3.0


def mesh_areas(verts, faces):
    fa = face_areas(verts, faces)
    return vertex_areas(len(np.asarray(verts).reshape(-1, 3)), faces, fa), fa


def point_footprint(src_pts, tgt_pts, radius=1.0):
    """(count int32, nearest_d2 float64, nearest_j int32) per target: the source points with d2 <= r^2, the minimum d2 and the smallest
    index at it (-1 and +inf when no source point is at a finite distance)."""
    r2 = float(radius) * float(radius)
    n = len(tgt_pts)
    count, best, best_j = np.empty(n, np.int32), np.empty(n), np.empty(n, np.int32)
    for a in range(0, n, 2048):
        d2 = pairwise_d2(tgt_pts[a:a + 2048], src_pts)
        count[a:a + 2048] = (d2 <= r2).sum(axis=1)
        d2 = np.where(np.isfinite(d2), d2, np.inf)
        j = np.argmin(d2, axis=1)                                 # first index among equal minima
        m = d2[np.arange(len(j)), j]
        best[a:a + 2048], best_j[a:a + 2048] = m, np.where(np.isfinite(m), j, -1)
    return count, best, best_j


def region_stats(values, weights, labels=None, covered=None, n_regions=1):
    """float64 [R, 12], driven the way region_partials_kernel is: blocks = max(1, min(2048, ceil(n / 1024))), thread g takes
    i = g, g + 256 blocks, ...; block_reduce, one slot row per block, the one-block finish -- per region.  An element outside a region
    performs no operation on that region's accumulator."""
    values = np.asarray(values, np.float32).reshape(-1)
    n = values.size
    t_all, w_all = values.astype(np.float64), np.asarray(weights, np.float64).reshape(-1)
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels, np.int64).reshape(-1)
    cov = np.ones(n, bool) if covered is None else np.asarray(covered).reshape(-1) != 0
    fin = np.isfinite(values)
    blocks = max(1, min(oref.STREAM_BLOCKS, -(-n // (4 * oref.KT))))
    threads = blocks * oref.KT
    out = np.empty((n_regions, SLOTS))
    for r in range(n_regions):
        acc = np.tile(REGION_CLEAR, (threads, 1))
        for start in range(0, n, threads):
            sl = slice(start, min(start + threads, n))
            inr = lab[sl] == r
            a = np.flatnonzero(inr)
            c = np.flatnonzero(inr & cov[sl])
            m = np.flatnonzero(inr & cov[sl] & fin[sl])
            t, w = t_all[sl][m], w_all[sl][m]
            wt = w * t
            acc[a, 0] = acc[a, 0] + 1.0
            acc[a, 3] = acc[a, 3] + w_all[sl][a]
            acc[c, 1] = acc[c, 1] + 1.0
            acc[c, 4] = acc[c, 4] + w_all[sl][c]
            acc[m, 2] = acc[m, 2] + 1.0
            acc[m, 5] = acc[m, 5] + w
            acc[m, 6] = acc[m, 6] + wt
            acc[m, 7] = acc[m, 7] + wt * t
            acc[m, 8] = np.fmin(acc[m, 8], t)
            acc[m, 9] = np.fmax(acc[m, 9], t)
            acc[m, 10] = acc[m, 10] + t
            acc[m, 11] = acc[m, 11] + t * t
        with np.errstate(invalid="ignore", over="ignore"):
            out[r] = oref.finish(oref.block_reduce(acc.reshape(blocks, oref.KT, SLOTS), REGION_OPS), REGION_CLEAR, REGION_OPS)
    return out
