"""An independent float64 reference for csrc/mesh.hip's point-to-mesh distance (tri_dist2, point_distance_kernel,
grid_distance_kernel), a float32 restatement of the grid's cell arithmetic and ring walk, and the seeded inputs the CPU and GPU
tests share.  The reference is NOT Ericson's branch ladder (oracle/mesh.py restates that one): it is the minimum of the three
point-segment distances and, where the triangle has a normal and the projection falls inside it, the plane distance -- exact for
zero-area triangles by construction.  Not collected as a test."""
import numpy as np

EPS32 = 2.0 ** -23


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _segment_d2(p, u, e):
    """squared distance from p[n,1,3] to the segments u + t e, t in [0,1] ([1,m,3]); a zero-length segment is the point u"""
    up = p - u
    ee = (e * e).sum(-1)
    t = np.clip((up * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
    d = up - t[..., None] * e
    return (d * d).sum(-1)


def point_triangle_d2_f64(p, a, b, c):
    """squared distances [n,m] from points p[n,3] to triangles (a,b,c)[m,3], float64"""
    p = np.asarray(p, np.float64)[:, None, :]
    a, b, c = (np.asarray(t, np.float64)[None] for t in (a, b, c))
    ab, bc, ca = b - a, c - b, a - c
    d2 = np.minimum(np.minimum(_segment_d2(p, a, ab), _segment_d2(p, b, bc)), _segment_d2(p, c, ca))
    n = np.cross(ab, -ca)
    nn = (n * n).sum(-1)
    ap, bp, cp = p - a, p - b, p - c
    inside = ((np.cross(ab, ap) * n).sum(-1) >= 0) & ((np.cross(bc, bp) * n).sum(-1) >= 0) & ((np.cross(ca, cp) * n).sum(-1) >= 0) & (nn > 0)
    plane = (ap * n).sum(-1) ** 2 / np.where(nn > 0, nn, 1.0)
    return np.where(inside, np.minimum(d2, plane), d2)


def distance_to_mesh_f64(points, verts, faces, chunk=128):
    """unsigned distance of each point to the triangle soup, float64, `chunk` points at a time"""
    points, verts, faces = np.asarray(points), np.asarray(verts), np.asarray(faces)
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    out = np.empty(len(points), np.float64)
    for s in range(0, len(points), chunk):
        out[s:s + chunk] = point_triangle_d2_f64(points[s:s + chunk], a, b, c).min(axis=1)
    return np.sqrt(out)


def tolerance(points, verts, d_ref):
    """4 * 2^-23 * (max|coordinate| + d_ref) per point: the well-conditioned float32 algorithm rounds q = a + ... at the ulp of the
    coordinate magnitude (the mesh's largest, or the point's own where that is larger), in three components and two additions."""
    m = np.maximum(np.abs(np.asarray(verts, np.float64)).max(), np.abs(np.asarray(points, np.float64)).reshape(-1, 3).max(axis=1))
    return 4.0 * EPS32 * (m + d_ref)


def ulp32(x):
    """spacing of float32 at |x|"""
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


# ---- float32 cell arithmetic and the ring walk built on it ------------------------------------------------------------------------
# The kernel bins with csrc/uniform_grid.h's grid_cell, the same formula in float64, whose slip is 2^29 times smaller: float32 is the
# coarse case, where the slip can be constructed in float32 coordinates (stop_rule_case) and a walk without slack stops too early.
def cell_coord_f32(p, lo, h, n):
    """floorf((p - lo) * inv_h) clamped to [0, n), inv_h = 1.0f / h, in numpy float32"""
    p, lo, h = np.asarray(p, np.float32), np.float32(lo), np.float32(h)
    inv_h = np.float32(1.0) / h
    c = np.floor(((p - lo).astype(np.float32) * inv_h).astype(np.float32)).astype(np.int64)
    return np.clip(c, 0, int(n) - 1)


def cell_coord_exact(p, lo, h, n):
    """the cell a float32 coordinate really lies in: the same float32 lo and h, the arithmetic in float64"""
    c = np.floor((np.asarray(p, np.float32).astype(np.float64) - np.float64(np.float32(lo))) / np.float64(np.float32(h))).astype(np.int64)
    return np.clip(c, 0, int(n) - 1)


def grid_walk_emulated(point, verts, faces, lo, h, dims, slack_cells=0.0):
    """grid_distance_kernel's ring walk for ONE point with float32 binning (cell_coord_f32 for the triangles' bounding
    boxes and for the point) and float64 triangle distances; the stop is best <= (max(0, (r - 1) - slack_cells) * h)^2 in float32, as
    in the kernel.  Returns (distance, index of the triangle that gave it)."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces)
    tri = verts[faces]                                                          # [m, 3 corners, 3 axes]
    tlo = np.stack([cell_coord_f32(tri[:, :, k].min(axis=1), lo[k], h, dims[k]) for k in range(3)], axis=1)
    thi = np.stack([cell_coord_f32(tri[:, :, k].max(axis=1), lo[k], h, dims[k]) for k in range(3)], axis=1)
    pc = np.array([int(cell_coord_f32(point[k], lo[k], h, dims[k])) for k in range(3)])
    d2 = point_triangle_d2_f64(np.asarray(point)[None], tri[:, 0], tri[:, 1], tri[:, 2])[0]
    # a triangle is first met in the ring whose number is the Chebyshev distance from the point's cell to its cell box
    ring = np.maximum(np.maximum(tlo - pc, pc - thi), 0).max(axis=1)
    rmax = int(max(pc.max(), (np.asarray(dims) - 1 - pc).max()))
    best, arg = np.float32(3.4e38), -1
    for r in range(rmax + 1):
        covered = np.float32(max(0.0, (r - 1) - slack_cells)) * np.float32(h)
        if r > 0 and best <= covered * covered:
            break
        for t in np.flatnonzero(ring == r):
            if np.float32(d2[t]) < best:
                best, arg = np.float32(d2[t]), int(t)
    return float(np.sqrt(np.float64(best))), arg


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------
def noisy_mesh():
    """an ordinary noisy marching-cubes mesh, 1743 triangles (a handful of them slivers)"""
    from oai_analysis_2_amd.synth import make_volume
    from oracle import mesh as om
    vol = make_volume(0, (12, 14, 13))
    return om.marching_cubes(vol, float(np.median(vol)))


def exact_iso_mesh(iso=0.5, frac=0.3, seed=3):
    """marching cubes through a volume with `frac` of its voxels exactly AT the iso level: an edge that starts at such a voxel puts
    its vertex on the voxel, so the voxel's edges share one position and the mesh is full of zero-area triangles"""
    from oai_analysis_2_amd.synth import make_volume
    from oracle import mesh as om
    vol = make_volume(1, (10, 12, 11)).copy()
    rng = np.random.default_rng(seed)
    vol[rng.random(vol.shape) < frac] = np.float32(iso)
    return om.marching_cubes(vol, iso)


def triangle_area2(verts, faces):
    """|ab x ac|^2 per triangle, float64"""
    v = np.asarray(verts, np.float64)
    n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    return (n * n).sum(-1)


def points_near(verts, faces, n, spread, seed):
    """n float32 points scattered with sigma `spread` around random positions ON random triangles"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, len(faces), n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    on = (np.asarray(verts, np.float64)[faces[t]] * w[:, :, None]).sum(axis=1)
    return (on + rng.normal(size=(n, 3)) * spread).astype(np.float32)


NEEDLE_HEIGHTS = (1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 1e-6, 0.0)


def needles(height, offset, n=300, seed=7):
    """(verts, faces, points): n isolated needle triangles of base 1 and the given height -- random pose, random foot of the apex
    along the base, random vertex order -- in a box of side 12 translated by `offset`; 400 points within 0.5 of the needles and 300
    within 1e-3 of a needle's long edge.  Everything is rounded to float32 after the translation."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0.0, 12.0, (n, 3))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    foot = rng.uniform(0.05, 0.95, (n, 1))
    tri = np.stack([centre - 0.5 * u, centre + 0.5 * u, centre + (foot - 0.5) * u + height * w], axis=1)      # [n, 3, 3]
    tri = np.take_along_axis(tri, np.argsort(rng.random((n, 3)), axis=1)[:, :, None], axis=1)                 # random vertex order
    verts = (tri.reshape(-1, 3) + offset).astype(np.float32)
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    k = rng.integers(0, n, 400)
    d = rng.normal(size=(400, 3))
    d *= (rng.uniform(0.0, 0.5, (400, 1)) / np.linalg.norm(d, axis=1, keepdims=True))
    near = centre[k] + rng.uniform(-0.5, 0.5, (400, 1)) * u[k] + d
    k = rng.integers(0, n, 300)
    d = rng.normal(size=(300, 3))
    d *= (rng.uniform(0.0, 1e-3, (300, 1)) / np.linalg.norm(d, axis=1, keepdims=True))
    edge = centre[k] + rng.uniform(-0.6, 0.6, (300, 1)) * u[k] + d
    return verts, faces, (np.concatenate([near, edge]) + offset).astype(np.float32)


ZERO_AREA_KINDS = ("a==b", "b==c", "a==c", "a==b==c", "collinear")


def zero_area_case(kind, offset=0.0, n=40, seed=11):
    """(verts, faces, points): n zero-area triangles of one kind, far enough apart not to interfere, and for each of them points whose
    nearest feature is the segment (or the point) that survives: beside its interior, beyond both ends, and on it."""
    rng = np.random.default_rng(seed)
    # everything on the lattice of 1/256, so that the float32 vertices -- translated or not -- are EXACTLY coincident or collinear
    p0 = np.round(rng.uniform(0.0, 20.0, (n, 3)) * 256.0) / 256.0
    u = rng.normal(size=(n, 3))
    step = np.round(u / np.linalg.norm(u, axis=1, keepdims=True) * 32.0) / 256.0
    u = step / np.linalg.norm(step, axis=1, keepdims=True)
    p1, mid = p0 + 8.0 * step, p0 + 3.0 * step
    a, b, c = {"a==b": (p0, p0, p1), "b==c": (p0, p1, p1), "a==c": (p0, p1, p0), "a==b==c": (p0, p0, p0), "collinear": (p0, mid, p1)}[kind]
    verts = (np.stack([a, b, c], axis=1).reshape(-1, 3) + offset).astype(np.float32)
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    pts = [p0 + (p1 - p0) * t + w * r for t in (-0.3, 0.0, 0.25, 0.5, 0.9, 1.0, 1.4) for r in (0.0, 1e-3, 0.3)]
    return verts, faces, (np.concatenate(pts) + offset).astype(np.float32)


# ---- the stopping-rule construction ---------------------------------------------------------------------------------------------
STOP_LO = np.array([-130.2137, 95.0, 210.0])                    # a patient-space corner
STOP_REACH = 0.31417 / 1.0001                                   # so that the grid's cell is h = 0.31417
STOP_CELLS = 509                                                # cells along x: close to the 512 cap, where float32 binning is worst


def stop_rule_case():
    """(verts, faces, point, grid, (lo32, h32, dims)): a point just under a cell boundary that float32 bins one cell up, a small
    triangle at h - delta/2 on the near side (inside the point's computed cell) and one at h - delta on the far side (two cells from
    the computed cell, one from the true cell).  A ring walk that trusts (r - 1) * h stops before it reaches the nearer one.
    ``grid`` = (lo, hi, reach) for _point_distance_dev; the rest is what _grid_from_params makes of it, in float32."""
    from oai_analysis_2_amd.mesh_processing import _grid_from_params
    hi = STOP_LO + np.array([STOP_CELLS - 1.5, 8.0, 8.0]) * 0.31417
    grid = (STOP_LO, hi, STOP_REACH)
    h, dims, lo = _grid_from_params(*grid)
    h32, lo32 = np.float32(h), lo.astype(np.float32)
    hd, lod = np.float64(h32), np.float64(lo32[0])
    best = None
    for k in range(300, int(dims[0]) - 2):                        # the boundary between cells k-1 and k
        bound = lod + k * hd
        x = np.float32(bound)
        if np.float64(x) >= bound:
            x = np.nextafter(x, np.float32(-np.inf))
        for _ in range(12):                                       # float32 neighbours below the boundary, nearest first
            if int(cell_coord_exact(x, lo32[0], h32, dims[0])) == k - 1 and int(cell_coord_f32(x, lo32[0], h32, dims[0])) == k:
                eps = bound - np.float64(x)
                if best is None or eps > best[0]:
                    best = (eps, k, x)
            x = np.nextafter(x, np.float32(-np.inf))
    assert best is not None, "no misbinned coordinate under any boundary of this grid"
    eps, k, px = best
    # near triangle: the farthest plane x = const that float32 still bins into cell k and that lies clearly within h of the point
    xa = np.float32(np.float64(px) + hd)
    while not (np.float64(xa) - np.float64(px) < hd * (1.0 - 1e-5) and int(cell_coord_f32(xa, lo32[0], h32, dims[0])) == k):
        xa = np.nextafter(xa, np.float32(-np.inf))
    # far triangle: the plane nearest to the point that float32 bins into cell k - 2
    xb = np.float32(np.float64(px) - hd)
    while int(cell_coord_f32(xb, lo32[0], h32, dims[0])) != k - 2:
        xb = np.nextafter(xb, np.float32(-np.inf))
    while int(cell_coord_f32(np.nextafter(xb, np.float32(np.inf)), lo32[0], h32, dims[0])) == k - 2:
        xb = np.nextafter(xb, np.float32(np.inf))
    py, pz = np.float32(lo32[1] + 3.5 * h32), np.float32(lo32[2] + 3.5 * h32)
    s = np.float32(0.02)
    plane = lambda x: [[x, py - s, pz - s], [x, py + 2 * s, pz - s], [x, py - s, pz + 2 * s]]       # the point projects inside
    verts = np.array(plane(xa) + plane(xb), np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    return verts, faces, np.array([px, py, pz], np.float32), grid, (lo32, h32, dims)
