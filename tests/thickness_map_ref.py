"""numpy restatement of the atlas thickness map (mesh_processing.py:400-534) that the library's kernels implement (not collected).

map_attributes: vtkPointInterpolator with VTK 9 defaults (vtkLinearKernel, RADIUS footprint, NormalizeWeights on) plus the
closest-point null strategy -- unpinned, restated from VTK's documentation.  project_thickness: the circle fit by Gauss-Newton and
the TC plateaus by the 3x3 scatter matrix; tests/test_thickness_map_cpu.py checks both against the reference's own outputs
(tests/golden/thickness_projection.npz)."""
import numpy as np


def pairwise_d2(tgt, src):
    """fp64 |p - q|^2 [n_tgt, n_src] of float32 points, summed as dx*dx + dy*dy + dz*dz (the kernels' order)"""
    t, s = np.asarray(tgt, np.float32).astype(np.float64), np.asarray(src, np.float32).astype(np.float64)
    d = [t[:, None, k] - s[None, :, k] for k in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def map_attributes(src_pts, src_vals, tgt_pts, radius=1.0):
    """src_vals [n_src, k] -> (out float32 [n_tgt, k], margin [n_tgt]).  out: fp64 mean over |p - q|^2 <= r^2, else the closest source
    point (ties: smallest index).  margin: how far the target is from changing its answer (distance of the nearest |d2 - r^2| to the
    footprint boundary, and for closest-point targets the gap to the second closest), in units of r^2."""
    vals = np.asarray(src_vals, np.float32).reshape(len(src_pts), -1).astype(np.float64)
    r2 = float(radius) * float(radius)
    out = np.empty((len(tgt_pts), vals.shape[1]), np.float32)
    margin = np.empty(len(tgt_pts))
    for a in range(0, len(tgt_pts), 2048):
        d2 = pairwise_d2(tgt_pts[a:a + 2048], src_pts)
        inside = d2 <= r2
        cnt = inside.sum(axis=1)
        sums = inside.astype(np.float64) @ vals
        closest = np.argmin(d2, axis=1)                          # first index among equal minima
        mean = sums / np.maximum(cnt, 1)[:, None]
        out[a:a + 2048] = np.where(cnt[:, None] > 0, mean, vals[closest]).astype(np.float32)
        m = np.abs(d2 - r2).min(axis=1) / max(r2, 1e-30)
        part = np.partition(d2, 1, axis=1)[:, :2] if d2.shape[1] > 1 else np.concatenate([d2, np.full_like(d2, np.inf)], axis=1)
        tie = (part[:, 1] - part[:, 0]) / max(r2, 1e-30)
        margin[a:a + 2048] = np.where(cnt > 0, m, np.minimum(m, tie))
    return out, margin


def grid_cells(pts, h, dims, lo):
    """cell (x, y, z) of float32 points in the grid (h, dims, lo) of mesh_processing._grid_from_params, as csrc/uniform_grid.h bins
    them: floor((p - lo) * (1 / h)) in float64, clamped to [0, dims - 1]"""
    t = np.floor((np.asarray(pts, np.float32).astype(np.float64) - np.asarray(lo, np.float64)) * (1.0 / float(h)))
    return np.clip(t, 0, np.asarray(dims) - 1).astype(np.int64)


def map_attributes_grid_order(src_pts, src_vals, tgt_pts, grid, radius=1.0):
    """One component through the grid path of map_attributes, in ITS summation order: per target the 27 cells around the target's
    cell in (z, y, x) order (clipped to the grid), within a cell ascending point index, one fp64 accumulator, then the mean as float32.
    ``grid`` = (h, dims, lo).  Returns (out, ascending, count): the same mean summed in ascending point index over the whole footprint
    (the brute-force order) beside it; both are NaN where ``count`` is 0 (the closest-point fallback is not restated here)."""
    h, dims, lo = grid
    vals = np.asarray(src_vals, np.float32).astype(np.float64)
    r2 = float(radius) * float(radius)
    d2 = pairwise_d2(tgt_pts, src_pts)
    sc, tc = grid_cells(src_pts, h, dims, lo), grid_cells(tgt_pts, h, dims, lo)
    out = np.full(len(tgt_pts), np.nan, np.float32)
    ascending = out.copy()
    count = np.zeros(len(tgt_pts), np.int64)
    for i, c in enumerate(tc):
        inside = np.flatnonzero(d2[i] <= r2)                                 # ascending point index
        count[i] = len(inside)
        if len(inside) == 0:
            continue
        s_grid, n_grid = 0.0, 0
        for z in range(max(c[2] - 1, 0), min(c[2] + 1, dims[2] - 1) + 1):
            for y in range(max(c[1] - 1, 0), min(c[1] + 1, dims[1] - 1) + 1):
                for x in range(max(c[0] - 1, 0), min(c[0] + 1, dims[0] - 1) + 1):
                    for j in inside[(sc[inside] == (x, y, z)).all(axis=1)]:
                        s_grid, n_grid = s_grid + vals[j], n_grid + 1
        assert n_grid == len(inside)                                         # h >= radius: the 27 cells hold the whole footprint
        s_asc = 0.0
        for j in inside:
            s_asc = s_asc + vals[j]
        out[i], ascending[i] = np.float32(s_grid / len(inside)), np.float32(s_asc / len(inside))
    return out, ascending, count


def fit_circle(x, y, iters=100):
    """centre minimising sum (R_i - mean R)^2 (Gauss-Newton on the centred Jacobian, from the centroid) and mean R_i"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    c = np.array([x.mean(), y.mean()])
    scale = np.sqrt(((x - c[0]) ** 2 + (y - c[1]) ** 2).mean())
    for _ in range(iters):
        dx, dy = c[0] - x, c[1] - y
        R = np.sqrt(dx * dx + dy * dy)
        J = np.stack([dx / R, dy / R], axis=1)
        J -= J.mean(axis=0)
        f = R - R.mean()
        step = -np.linalg.solve(J.T @ J, J.T @ f)
        c = c + step
        if np.hypot(*step) <= 1e-12 * scale:
            break
    return c, np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2).mean()


def plateau_scores(v):
    """KernelPCA(n_components=2, linear kernel).fit_transform(v) by the 3x3 scatter matrix, signs as sklearn's svd_flip(u)"""
    v = np.asarray(v, np.float64)
    d = v - v.mean(axis=0)
    w, U = np.linalg.eigh(d.T @ d)
    s = d @ U[:, ::-1][:, :2]
    big = np.argmax(np.abs(s), axis=0)
    return s * np.sign(s[big, [0, 1]])


def rotate(e, angle):
    t = angle / 180.0 * np.pi
    return e @ np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])


def circle_cost(x, y, c):
    R = np.hypot(np.asarray(x, np.float64) - c[0], np.asarray(y, np.float64) - c[1])
    return ((R - R.mean()) ** 2).sum()


def project_thickness(verts, thickness, mesh_type="FC", centre=None):
    """``centre``: FC only, use this circle centre instead of fitting one"""
    v = np.asarray(verts, np.float64)
    th = np.asarray(thickness, np.float64)
    if mesh_type == "FC":
        sw = v[:, [1, 0, 2]]
        c = fit_circle(sw[:, 0], sw[:, 1])[0] if centre is None else np.asarray(centre, np.float64)
        return np.arctan2(sw[:, 1] - c[1], sw[:, 0] - c[0]), sw[:, 2].copy(), th.copy()
    left, right = v[:, 2] < 50, v[:, 2] >= 50
    el = rotate(plateau_scores(v[left]), -50)
    er = rotate(plateau_scores(v[right]), -160)
    er[:, 0] = -er[:, 0]
    return (np.concatenate([er[:, 0], el[:, 0]]), np.concatenate([er[:, 1] + 50, el[:, 1]]),
            np.concatenate([th[right], th[left]]))
