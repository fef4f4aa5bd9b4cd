"""CPU: the independent float64 point-to-mesh reference (tests/point_distance_ref.py) against closed forms -- every Voronoi region of a
triangle and every kind of zero-area triangle -- and against the oracle's Ericson ladder on a well-conditioned mesh; the oracle on
zero-area triangles; float32 cell arithmetic (coarser than the kernel's float64) against exact flooring; and the stopping-rule construction
that tests/test_point_distance_gpu.py runs on the device, verified here on the emulated ring walk."""
import numpy as np
import pytest

import point_distance_ref as pr
from oracle import mesh as om

A, B, C = np.array([0.0, 0.0, 0.0]), np.array([4.0, 0.0, 0.0]), np.array([0.0, 3.0, 0.0])


def _one(p, a, b, c):
    verts = np.array([a, b, c], np.float64)
    return float(pr.distance_to_mesh_f64(np.array([p], np.float64), verts, np.array([[0, 1, 2]]))[0])


@pytest.mark.parametrize("p,expect", [
    ((1.0, 1.0, 2.5), 2.5),                                   # over the interior
    ((1.0, 1.0, -0.75), 0.75),                                # under it
    ((2.0, -1.0, 0.0), 1.0),                                  # in the plane, beyond edge ab
    ((2.0, -3.0, 4.0), 5.0),                                  # beyond edge ab and off the plane
    ((-2.0, 1.5, 0.0), 2.0),                                  # beyond edge ac
    ((4.0, 3.0, 0.0), 2.4),                                   # beyond the hypotenuse bc: 12/5
    ((-3.0, -4.0, 0.0), 5.0),                                 # beyond vertex a
    ((7.0, -4.0, 0.0), 5.0),                                  # beyond vertex b
    ((-1.0, 5.0, 2.0), 3.0),                                  # beyond vertex c: (1, 2, 2)
    ((1.0, 1.0, 0.0), 0.0),                                   # in the plane, inside
    ((4.0, 0.0, 0.0), 0.0),                                   # on a vertex
    ((2.0, 1.5, 0.0), 0.0),                                   # on an edge
])
def test_reference_closed_forms_on_a_3_4_5_triangle(p, expect):
    for a, b, c in ((A, B, C), (B, C, A), (C, A, B), (A, C, B)):                      # every vertex order, both windings
        assert abs(_one(p, a, b, c) - expect) < 1e-14
    shift = np.array([-130.0, 95.0, 210.0])                                            # exactly representable: the closed form holds
    assert abs(_one(np.asarray(p) + shift, A + shift, B + shift, C + shift) - expect) < 1e-12


@pytest.mark.parametrize("kind,tri", [
    ("a==b", (A, A, B)), ("b==c", (A, B, B)), ("a==c", (A, B, A)), ("collinear", (A, B / 4, B)), ("collinear, b beyond c", (A, B, B / 2)),
])
def test_reference_on_zero_area_triangles_is_the_segment_distance(kind, tri):
    for p, expect in (((2.0, 3.0, 0.0), 3.0), ((-3.0, 0.0, 4.0), 5.0), ((7.0, 4.0, 0.0), 5.0), ((1.0, 0.0, 0.0), 0.0), ((4.0, 0.0, 0.0), 0.0)):
        assert abs(_one(p, *tri) - expect) < 1e-14, (kind, p)


def test_reference_on_a_point_triangle_is_the_point_distance():
    assert abs(_one((3.0, 4.0, 12.0), A, A, A) - 13.0) < 1e-14
    assert _one((0.0, 0.0, 0.0), A, A, A) == 0.0


def test_reference_agrees_with_the_ericson_oracle_on_a_well_conditioned_mesh():
    """two formulations, one answer: an icosphere-like closed mesh without slivers, points in every Voronoi region"""
    rng = np.random.default_rng(2)
    v = rng.normal(size=(60, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([(i, j, k) for i in range(60) for j in range(i + 1, 60) for k in range(j + 1, 60)
                  if max(np.linalg.norm(v[i] - v[j]), np.linalg.norm(v[j] - v[k]), np.linalg.norm(v[i] - v[k])) < 0.75], np.int64)
    area2 = pr.triangle_area2(v, f)
    edge2 = ((v[f[:, 1]] - v[f[:, 0]]) ** 2).sum(-1) * ((v[f[:, 2]] - v[f[:, 0]]) ** 2).sum(-1)
    f = f[area2 > 0.05 * edge2]                                                        # sin^2 of the angle at a: no slivers
    assert len(f) > 100
    pts = np.concatenate([rng.normal(size=(400, 3)), v[:20], v[f[:30]].mean(axis=1), rng.normal(size=(100, 3)) * 10.0])
    ours, ericson = pr.distance_to_mesh_f64(pts, v, f), om.distance_to_mesh(pts, v, f)
    assert np.abs(ours - ericson).max() <= 1e-12
    assert ours[400:420].max() <= 1e-15 and ours[420:450].max() <= 1e-15             # vertices and centroids lie on the mesh


def test_reference_stays_small_in_memory_and_chunks_agree():
    rng = np.random.default_rng(4)
    v, f = rng.normal(size=(300, 3)), rng.integers(0, 300, (2000, 3))
    pts = rng.normal(size=(1000, 3))
    whole = pr.distance_to_mesh_f64(pts, v, f)                                        # 128 x 2000 pairs at a time
    assert np.array_equal(whole, pr.distance_to_mesh_f64(pts, v, f, chunk=7))


@pytest.mark.parametrize("kind", pr.ZERO_AREA_KINDS)
@pytest.mark.parametrize("offset", [0.0, 150.0])
def test_oracle_handles_zero_area_triangles(kind, offset):
    """oracle.mesh.distance_to_mesh used to return NaN for EVERY point of a mesh that holds one zero-area triangle"""
    verts, faces, pts = pr.zero_area_case(kind, offset)
    assert (pr.triangle_area2(verts, faces) == 0).all()                                # exactly, translated or not
    got = om.distance_to_mesh(pts, verts, faces)
    assert np.isfinite(got).all()
    ref = pr.distance_to_mesh_f64(pts, verts, faces)
    assert np.abs(got - ref).max() <= 1e-9 * (1.0 + offset)


def test_oracle_on_the_exact_iso_mesh_and_unchanged_elsewhere():
    verts, faces = pr.exact_iso_mesh()
    assert (pr.triangle_area2(verts, faces) == 0).sum() > 100
    pts = pr.points_near(verts, faces, 200, 0.7, seed=1)
    got = om.distance_to_mesh(pts, verts, faces)
    assert np.isfinite(got).all() and np.abs(got - pr.distance_to_mesh_f64(pts, verts, faces)).max() <= 1e-9
    # a mesh whose every triangle has a normal and every edge a length takes the ladder's own arithmetic, bit for bit
    verts, faces = pr.noisy_mesh()
    keep = pr.triangle_area2(verts, faces) > 0
    pts = pr.points_near(verts, faces[keep], 100, 0.7, seed=2)
    a, b, c = verts[faces[keep][:, 0]], verts[faces[keep][:, 1]], verts[faces[keep][:, 2]]
    assert np.array_equal(om.distance_to_mesh(pts, verts, faces[keep]), om.point_triangle_distance(pts, a, b, c).min(axis=1))


def test_cell_coord_f32_against_exact_flooring():
    lo, h, n = np.float32(0.0), np.float32(1.0), 512                                  # an integer grid: float32 bins every probe right
    k = np.arange(1, 511, dtype=np.float32)
    probes = np.concatenate([np.nextafter(k, np.float32(-np.inf)), k, np.nextafter(k, np.float32(np.inf))])
    assert np.array_equal(pr.cell_coord_f32(probes, lo, h, n), pr.cell_coord_exact(probes, lo, h, n))
    assert np.array_equal(pr.cell_coord_f32(np.float32([-5.0, 0.0, 0.5, 511.99, 512.0, 1e9]), lo, h, n), [0, 0, 0, 511, 511, 511])
    # the far-origin grid: coordinates within a few float32 steps of a boundary land in the neighbouring cell
    lo, h, n = np.float32(-130.2137), np.float32(0.31417), 512
    bounds = (np.float64(lo) + np.arange(1, 511) * np.float64(h)).astype(np.float32)
    probes, up, down = [bounds], bounds, bounds
    for _ in range(3):                                                                # +-3 float32 steps around every boundary
        up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
        probes += [up, down]
    probes = np.concatenate(probes)
    got, exact = pr.cell_coord_f32(probes, lo, h, n), pr.cell_coord_exact(probes, lo, h, n)
    assert np.abs(got - exact).max() == 1 and (got != exact).sum() >= 1
    off = np.abs((probes[got != exact].astype(np.float64) - np.float64(lo)) / np.float64(h) - np.maximum(got, exact)[got != exact])
    assert off.max() < 3 * pr.EPS32 * 512                                             # the bound the ring walk's slack is sized by, in cells


def test_stop_rule_construction_defeats_a_walk_without_slack():
    """the emulated ring walk (float32 binning) returns the farther triangle when it trusts (r - 1) * h, the nearer one with the
    kernel's slack of 2^-10 cells; brute force is the reference either way"""
    verts, faces, point, grid, (lo32, h32, dims) = pr.stop_rule_case()
    assert abs(float(lo32[0]) + 130.2137) < 1e-3 and abs(float(h32) - 0.31417) < 1e-6 and int(dims[0]) <= 512
    cx = int(pr.cell_coord_f32(point[0], lo32[0], h32, dims[0]))
    assert int(pr.cell_coord_exact(point[0], lo32[0], h32, dims[0])) == cx - 1                  # binned one cell up
    assert int(pr.cell_coord_f32(verts[0, 0], lo32[0], h32, dims[0])) == cx                    # near side: the computed cell
    assert int(pr.cell_coord_f32(verts[3, 0], lo32[0], h32, dims[0])) == cx - 2                # far side: two cells away
    ref = pr.distance_to_mesh_f64(point[None], verts, faces)[0]
    each = np.sqrt(pr.point_triangle_d2_f64(point[None], verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]])[0])
    assert each[1] < each[0] < float(h32) and ref == each[1]
    assert each[0] - each[1] > 16 * pr.ulp32(ref)                                                # far beyond rounding in the distance
    d, arg = pr.grid_walk_emulated(point, verts, faces, lo32, h32, dims, slack_cells=0.0)
    assert arg == 0 and d > ref
    d, arg = pr.grid_walk_emulated(point, verts, faces, lo32, h32, dims, slack_cells=2.0 ** -10)
    assert arg == 1 and abs(d - ref) <= pr.ulp32(ref)
