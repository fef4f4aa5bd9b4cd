"""GPU: csrc/mesh.hip's point-to-mesh distance -- tri_dist2, point_distance_kernel (brute force) and grid_distance_kernel (uniform-grid
broad phase) -- against the independent float64 reference of tests/point_distance_ref.py, at the tile and block boundaries, far from
the origin, on needles and zero-area triangles, on points that lie on the mesh, and on the grid's own edge cases: float32 cell
boundaries, the 512-cell cap, one cell on an axis, the ring walk's stopping rule and the cell-size refusal.

Every case runs both kernels.  Per point: |got - ref| <= 4 * 2^-23 * (max|coordinate| + ref)  (point_distance_ref.tolerance), and
|grid - brute| <= 1 ulp32(brute).  Each case prints its worst err/tol and the number of points where the two kernels differ in any bit
("Point-to-mesh distance: what the tests pin", keeps the table)."""
import numpy as np
import pytest

import point_distance_ref as pr

pytestmark = pytest.mark.gpu


def _both(pts, verts, faces):
    from oai_analysis_2_amd import mesh_processing as mp
    mesh = mp.Mesh(np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32))
    return mp.point_distance(pts, mesh, broad_phase=False), mp.point_distance(pts, mesh, broad_phase=True)


def _report(name, brute, grid, ref, tol):
    worst = [float(np.max(np.where(np.isfinite(g), np.abs(g - ref) / tol, np.inf))) if len(ref) else 0.0 for g in (brute, grid)]
    unequal = int((brute.view(np.uint32) != grid.view(np.uint32)).sum())
    print(f"point_distance[{name}]: err/tol brute {worst[0]:.3g} grid {worst[1]:.3g}; grid != brute in {unequal} of {len(ref)} points")


def _check(name, pts, verts, faces, ref=None):
    """both kernels against the float64 reference, and the grid form against brute force; returns (brute, grid, ref, tol)"""
    pts = np.ascontiguousarray(pts, np.float32)
    ref = pr.distance_to_mesh_f64(pts, verts, faces) if ref is None else ref
    tol = pr.tolerance(pts, verts, ref)
    brute, grid = _both(pts, verts, faces)
    assert brute.shape == grid.shape == (len(pts),) and brute.dtype == grid.dtype == np.float32
    _report(name, brute, grid, ref, tol)
    for kind, got in (("brute", brute), ("grid", grid)):
        assert np.all(np.abs(got - ref) <= tol), (name, kind, float(np.nanmax(np.abs(got - ref) / tol)), int((~np.isfinite(got)).sum()))
    assert np.all(np.abs(grid.astype(np.float64) - brute) <= pr.ulp32(brute)), (name, "grid vs brute")
    return brute, grid, ref, tol


# ---- tile and block boundaries ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noisy():
    verts, faces = pr.noisy_mesh()
    assert len(faces) >= 1025
    return verts, faces


@pytest.mark.parametrize("nt", [1, 511, 512, 513, 1025])
def test_triangle_tile_and_point_block_boundaries(noisy, nt):
    """the brute-force kernel stages 512 triangles per LDS tile and runs 256 points per block: one under, at, one over, two tiles + 1"""
    verts, faces = noisy
    faces = faces[200:200 + nt]
    pts = pr.points_near(verts, faces, 257, 0.6, seed=nt)
    ref = pr.distance_to_mesh_f64(pts, verts, faces)
    for n_pts in (1, 255, 256, 257):
        _check(f"nt={nt} np={n_pts}", pts[:n_pts], verts, faces, ref[:n_pts])


def test_no_points_is_an_empty_result(noisy):
    verts, faces = noisy
    for got in _both(np.zeros((0, 3), np.float32), verts, faces):
        assert got.shape == (0,) and got.dtype == np.float32
    _check("after np=0", pr.points_near(verts, faces, 64, 0.6, seed=0), verts, faces)           # and the device is still sound


# ---- coordinates of patient space ---------------------------------------------------------------------------------------------------
def test_far_from_the_origin(noisy):
    verts, faces = noisy
    shift = np.array([-130.0, 95.0, 210.0])
    pts = pr.points_near(verts, faces, 1000, 0.6, seed=21).astype(np.float64) + shift
    _check("noisy mesh", pr.points_near(verts, faces, 1000, 0.6, seed=21), verts, faces)
    _check("noisy mesh at (-130, 95, 210)", pts.astype(np.float32), (verts.astype(np.float64) + shift).astype(np.float32), faces)


# ---- thin and zero-area triangles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 150.0])
@pytest.mark.parametrize("height", pr.NEEDLE_HEIGHTS)
def test_needle_ladder(height, offset):
    """300 isolated needles of base 1, random pose and vertex order.  Ericson's interior branch in float32 missed this tolerance from
    height 1e-2 down (4.4 x tol at 1e-2, 1e3 x at 1e-3, the distance itself from 3e-4 down); the plane-distance interior holds it down
    to the needles that kThin (csrc/mesh.hip) hands to the double path -- most of 3e-3, all from 1e-3 down."""
    verts, faces, pts = pr.needles(height, offset)
    _check(f"needles h={height:g} offset={offset:g}", pts, verts, faces)


@pytest.mark.parametrize("offset", [0.0, 150.0])
@pytest.mark.parametrize("kind", pr.ZERO_AREA_KINDS)
def test_zero_area_triangles(kind, offset):
    """coincident and collinear vertices: the nearest feature is the surviving segment (or point), never 'no triangle'"""
    verts, faces, pts = pr.zero_area_case(kind, offset)
    assert (pr.triangle_area2(verts, faces) == 0).all()
    _check(f"zero area {kind} offset={offset:g}", pts, verts, faces)


def test_exact_iso_marching_cubes_raw_and_smoothed():
    """a probability map with voxels exactly at the iso level: a third of the mesh has no area, before and after smoothing"""
    from oai_analysis_2_amd import mesh_processing as mp
    verts, faces = pr.exact_iso_mesh()
    flat = int((pr.triangle_area2(verts, faces) == 0).sum())
    assert flat > 100 and len(faces) <= 2400, (flat, len(faces))
    pts = pr.points_near(verts, faces, 1000, 0.7, seed=31)
    _check(f"exact-iso raw ({flat} of {len(faces)} flat)", pts, verts, faces)
    smoothed = mp.smooth_mesh(mp.Mesh(verts, faces), 150, 0.01).verts                          # coincident vertices drift apart: slivers
    _check("exact-iso after 150 sweeps at 0.01", pts, smoothed, faces)


# ---- points on the mesh ---------------------------------------------------------------------------------------------------------------
def test_points_on_vertices_edges_and_faces(noisy):
    verts, faces = noisy
    v = verts.astype(np.float64)
    tri = v[faces[::2]]
    on = np.concatenate([v[:300], 0.5 * (tri[:, 0] + tri[:, 1])[:250], 0.5 * (tri[:, 1] + tri[:, 2])[:250], tri.mean(axis=1)[:300]]).astype(np.float32)
    brute, grid, ref, tol = _check("on vertices, edge midpoints, centroids", on, verts, faces)
    assert np.all(brute <= tol) and np.all(grid <= tol)                                      # on the mesh up to the points' own rounding
    # straight above the centroids of well-shaped triangles, at a height no other triangle undercuts by more than the reference says
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    good = (n * n).sum(-1) > 0.05 * ((tri[:, 1] - tri[:, 0]) ** 2).sum(-1) * ((tri[:, 2] - tri[:, 0]) ** 2).sum(-1)
    height = 0.01
    above = (tri.mean(axis=1) + height * n / np.linalg.norm(n, axis=1, keepdims=True))[good][:600].astype(np.float32)
    brute, grid, ref, tol = _check("0.01 above centroids", above, verts, faces)
    assert np.all(ref <= height + 1e-6) and np.all(brute <= height + 1e-6 + tol) and (np.abs(ref - height) <= 1e-6).sum() > len(ref) // 2


# ---- shapes of the grid ---------------------------------------------------------------------------------------------------------------
def _lattice(nx, ny, z, jitter, seed):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    xy = np.stack([x, y], axis=-1) * 0.5 + rng.uniform(-jitter, jitter, (nx, ny, 2))
    verts = np.concatenate([xy.reshape(-1, 2), np.full((nx * ny, 1), z)], axis=1).astype(np.float32)
    i = (np.arange(nx - 1)[:, None] * ny + np.arange(ny - 1)[None, :]).reshape(-1)
    faces = np.concatenate([np.stack([i, i + ny, i + 1], axis=1), np.stack([i + 1, i + ny, i + ny + 1], axis=1)]).astype(np.int32)
    return verts, faces


def test_planar_mesh_has_one_cell_on_an_axis():
    verts, faces = _lattice(21, 23, 3.25, 0.1, seed=41)
    rng = np.random.default_rng(42)
    over = np.concatenate([rng.uniform(1.0, 9.0, (300, 2)), np.full((300, 1), 4.0)], axis=1).astype(np.float32)   # 0.75 above the interior
    brute, grid, ref, tol = _check("planar mesh, 0.75 above", over, verts, faces)
    assert np.all(np.abs(ref - 0.75) < 1e-12) and np.all(np.abs(brute - 0.75) <= tol)
    _check("planar mesh, around", pr.points_near(verts, faces, 500, 1.5, seed=43), verts, faces)


def test_single_triangle():
    verts = np.array([[1.0, 2.0, 3.0], [2.5, 2.25, 3.5], [1.25, 3.75, 2.5]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    rng = np.random.default_rng(44)
    pts = np.concatenate([pr.points_near(verts, faces, 300, 1.0, seed=45), rng.uniform(-60.0, 60.0, (100, 3)).astype(np.float32), verts])
    _check("single triangle", pts, verts, faces)


def test_polyline_at_the_512_cell_cap():
    """a 1000-unit line of tiny triangles: the cell is extent / 512, not the longest edge, and x runs over all 513 cells"""
    from oai_analysis_2_amd.mesh_processing import _grid_from_params
    rng = np.random.default_rng(46)
    x0 = np.sort(rng.uniform(0.0, 1000.0, 700))
    x0[0], x0[-1] = 0.0, 1000.0
    a = np.stack([x0, 5.0 + np.sin(x0 / 40.0), 2.0 + np.cos(x0 / 25.0)], axis=1)
    verts = np.stack([a, a + rng.uniform(-0.2, 0.2, (700, 3)), a + rng.uniform(-0.2, 0.2, (700, 3))], axis=1).reshape(-1, 3).astype(np.float32)
    faces = np.arange(2100, dtype=np.int32).reshape(700, 3)
    h, dims, _ = _grid_from_params(verts.min(axis=0).astype(np.float64), verts.max(axis=0).astype(np.float64), 0.7)
    assert h > 1.9 and dims[0] == 513
    pts = np.concatenate([pr.points_near(verts, faces, 700, 1.0, seed=47), pr.points_near(verts, faces, 300, 30.0, seed=48)])
    _check("polyline, 513 cells", pts, verts, faces)


def test_points_exactly_on_cell_boundaries(noisy):
    """every coordinate at lo + k * h as float32 computes it, for the grid that point_distance derives from the mesh -- at the origin and
    in patient space, where float32 puts some of these into the cell below"""
    from oai_analysis_2_amd.mesh_processing import _grid_from_params
    verts0, faces = noisy
    rng = np.random.default_rng(49)
    for shift in (np.zeros(3), np.array([-130.0, 95.0, 210.0])):
        verts = (verts0.astype(np.float64) + shift).astype(np.float32)
        tri = verts[faces].astype(np.float64)
        edge = max(np.linalg.norm(tri[:, i] - tri[:, (i + 1) % 3], axis=1).max() for i in range(3))
        h, dims, lo = _grid_from_params(verts.min(axis=0).astype(np.float64), verts.max(axis=0).astype(np.float64), edge)
        lo32, h32 = lo.astype(np.float32), np.float32(h)
        k = np.stack([rng.integers(0, dims[c] + 1, 600) for c in range(3)], axis=1).astype(np.float32)
        pts = (lo32[None, :] + k * h32).astype(np.float32)
        pts[300:, 1:] += rng.uniform(0.0, float(h), (300, 2)).astype(np.float32)              # half of them on one boundary only
        _check(f"points on cell boundaries, shift {shift[0]:g}", pts, verts, faces)


def test_points_far_outside_the_box_walk_every_ring(noisy):
    verts, faces = noisy
    rng = np.random.default_rng(50)
    centre = verts.mean(axis=0).astype(np.float64)
    dirs = np.array([[sx, sy, sz] for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1) if (sx, sy, sz) != (0, 0, 0)], np.float64)
    pts = np.concatenate([centre + dirs * r + rng.uniform(-2.0, 2.0, (26, 3)) for r in (15.0, 60.0, 250.0)]).astype(np.float32)
    _check("far outside on every side", pts, verts, faces)


def test_one_long_triangle_among_tiny_ones():
    """the cell is the longest edge: one triangle of edge 9 makes a 2 x 2 x 2 grid around 1500 triangles of edge 0.05"""
    rng = np.random.default_rng(51)
    a = rng.uniform(0.0, 10.0, (1500, 3))
    tiny = np.stack([a, a + rng.uniform(-0.05, 0.05, (1500, 3)), a + rng.uniform(-0.05, 0.05, (1500, 3))], axis=1).reshape(-1, 3)
    verts = np.concatenate([tiny, [[0.5, 0.5, 0.5], [9.5, 0.75, 0.5], [0.75, 9.25, 1.0]]]).astype(np.float32)
    faces = np.arange(4503, dtype=np.int32).reshape(1501, 3)
    pts = np.concatenate([pr.points_near(verts, faces, 600, 0.3, seed=52), pr.points_near(verts, faces[-1:], 300, 0.3, seed=53)])
    _check("one long triangle among 1500 tiny", pts, verts, faces)


# ---- the ring walk's stopping rule ------------------------------------------------------------------------------------------------------
def test_ring_walk_does_not_stop_one_ring_early():
    """tests/test_point_distance_cpu.py proves the construction on the emulated walk: float32 bins the point one cell up, a triangle at
    h - delta/2 sits in that cell and a nearer one at h - delta two cells down.  The grid kernel must find the nearer one."""
    import torch
    from oai_analysis_2_amd import mesh_processing as mp
    verts, faces, point, grid, _ = pr.stop_rule_case()
    pts = np.repeat(point[None], 3, axis=0)
    pts[1:, 1] += np.float32([0.005, -0.005])                                                  # (still over both triangles' interiors)
    ref = pr.distance_to_mesh_f64(pts, verts, faces)
    p, v, f = torch.from_numpy(pts).cuda(), torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()
    brute = mp._point_distance_dev(p, v, f, None).cpu().numpy()
    walked = mp._point_distance_dev(p, v, f, grid).cpu().numpy()
    tol = pr.tolerance(pts, verts, ref)
    _report("stopping rule", brute, walked, ref, tol)
    assert np.all(np.abs(brute - ref) <= tol)
    assert np.all(np.abs(walked.astype(np.float64) - brute) <= pr.ulp32(brute)), (walked - ref, brute - ref)     # the gap is ~60 ulp


# ---- the refusal ------------------------------------------------------------------------------------------------------------------------
def test_cell_smaller_than_the_triangles_is_refused_and_the_device_survives(noisy):
    """a cell of a tenth of the longest edge: the triangle-cell pairs exceed the 8 per triangle the workspace holds, which the library
    finds from the count BEFORE it fills the list"""
    import torch
    from oai_analysis_2_amd import mesh_processing as mp
    from oai_analysis_2_amd._lib import OaiError
    verts, faces = noisy
    tri = verts[faces].astype(np.float64)
    edge = max(np.linalg.norm(tri[:, i] - tri[:, (i + 1) % 3], axis=1).max() for i in range(3))
    lo, hi = verts.min(axis=0).astype(np.float64), verts.max(axis=0).astype(np.float64)
    pts = pr.points_near(verts, faces, 200, 0.6, seed=60)
    p, v, f = torch.from_numpy(pts).cuda(), torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()
    with pytest.raises(OaiError, match="cell_size"):
        mp._point_distance_dev(p, v, f, (lo, hi, 0.1 * edge))
    torch.cuda.synchronize()
    _check("after the refusal", pts, verts, faces)
