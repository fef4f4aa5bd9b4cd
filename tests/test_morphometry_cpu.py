"""CPU: the numpy restatement of the morphometry primitives (tests/morphometry_ref.py) against closed forms, and the host-side record
(thickness.RegionMorphometry.from_slots) on hand-made slot rows."""
import math

import numpy as np
import pytest

import morphometry_ref as mref


def _grid_mesh(k):
    """(k+1)^2 vertices of a k x k grid of unit squares in the plane z = 0, each square cut along its (0,0)-(1,1) diagonal."""
    j, i = np.mgrid[0:k + 1, 0:k + 1]
    verts = np.stack([i.ravel(), j.ravel(), np.zeros(i.size)], axis=1).astype(np.float32)
    v = lambda jj, ii: jj * (k + 1) + ii
    faces = []
    for jj in range(k):
        for ii in range(k):
            faces += [[v(jj, ii), v(jj, ii + 1), v(jj + 1, ii + 1)], [v(jj, ii), v(jj + 1, ii + 1), v(jj + 1, ii)]]
    return verts, np.asarray(faces, np.int32)


def test_right_triangle():
    va, fa = mref.mesh_areas(np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    assert fa.tolist() == [6.0] and va.tolist() == [2.0, 2.0, 2.0]


@pytest.mark.parametrize("k", [1, 2, 5])
def test_unit_square_grid(k):
    verts, faces = _grid_mesh(k)
    va, fa = mref.mesh_areas(verts, faces)
    assert np.array_equal(fa, np.full(2 * k * k, 0.5))
    va = va.reshape(k + 1, k + 1)
    third = lambda n_faces: sum([0.5] * n_faces) / 3.0           # a vertex owns a third of each incident half square
    if k >= 2:
        assert np.array_equal(va[1:-1, 1:-1], np.full((k - 1, k - 1), third(6)))       # interior: six faces
        for edge in (va[0, 1:-1], va[-1, 1:-1], va[1:-1, 0], va[1:-1, -1]):
            assert np.array_equal(edge, np.full(k - 1, third(3)))                       # edge: three
    # corners: the two on the diagonal have two faces, the other two one
    assert va[0, 0] == va[-1, -1] == third(2) and va[0, -1] == va[-1, 0] == third(1)
    assert abs(va.sum() - k * k) <= 4 * np.finfo(np.float64).eps * k * k


def test_vertex_areas_add_up_to_the_surface_and_follow_the_stated_order():
    rng = np.random.default_rng(0)
    verts = rng.normal(size=(200, 3)).astype(np.float32) * 7
    faces = rng.integers(0, 200, size=(900, 3)).astype(np.int32)
    faces[5] = [7, 7, 9]                                          # names a vertex twice: area 0, two corners at vertex 7
    faces[6] = [1, 2, 200]                                        # not a triangle of this mesh
    va, fa = mref.mesh_areas(verts, faces)
    assert fa[5] == 0.0 and np.isnan(fa[6]) and np.isfinite(np.delete(fa, 6)).all()
    total = math.fsum(np.delete(fa, 6))
    assert abs(math.fsum(va) - total) <= 900 * np.finfo(np.float64).eps * total        # a third of each face three times, each sum rounded
    # the order: a plain loop over the corners in ascending index, per vertex
    want = np.zeros(200)
    for c, v in enumerate(faces.reshape(-1)):
        if c // 3 != 6:
            want[v] = want[v] + fa[c // 3]
    assert np.array_equal(va, want / 3.0)
    assert not np.array_equal(mref.vertex_areas(200, faces, fa, descending=True), va)  # and the other order is another sum
    assert mref.vertex_areas(5, np.zeros((0, 3), np.int32), np.zeros(0)).tolist() == [0.0] * 5


def test_footprint_restatement_on_a_line():
    src = np.array([[0, 0, 0], [2, 0, 0], [2, 0, 0], [10, 0, 0]], np.float32)
    tgt = np.array([[0.5, 0, 0], [2, 0, 0], [6, 0, 0], [1, 0, 0]], np.float32)
    count, d2, j = mref.point_footprint(src, tgt, radius=1.0)
    assert count.tolist() == [1, 2, 0, 3] and d2.tolist() == [0.25, 0.0, 16.0, 1.0] and j.tolist() == [0, 1, 1, 0]
    count, d2, j = mref.point_footprint(np.array([[np.nan, 0, 0]], np.float32), tgt)
    assert count.tolist() == [0] * 4 and np.isinf(d2).all() and j.tolist() == [-1] * 4


@pytest.mark.parametrize("n", [1, 65, 1025, 1024 * 3 + 7])
def test_region_sums_against_fsum(n):
    rng = np.random.default_rng([3, n])
    R = 3
    values = rng.uniform(0.5, 4.0, n).astype(np.float32)
    values[rng.uniform(size=n) < 0.05] = np.nan
    weights = np.exp(rng.uniform(-20.0, 20.0, n))
    labels = rng.integers(-1, R + 1, n).astype(np.int32)
    covered = (rng.uniform(size=n) < 0.7).astype(np.uint8)
    got = mref.region_stats(values, weights, labels, covered, R)
    assert got.shape == (R, 12)
    eps = np.finfo(np.float64).eps
    for r in range(R):
        a = labels == r
        c = a & (covered != 0)
        m = c & np.isfinite(values)
        t, w = values[m].astype(np.float64), weights[m]
        assert got[r, :3].tolist() == [a.sum(), c.sum(), m.sum()]
        # positive terms: any summation order is within (terms - 1) eps of the exact sum, relatively; each term is itself rounded once or twice
        for slot, terms in ((3, weights[a]), (4, weights[c]), (5, w), (6, w * t), (7, w * t * t), (10, t), (11, t * t)):
            exact = math.fsum(terms)
            assert abs(got[r, slot] - exact) <= (len(terms) + 2) * eps * exact, (r, slot)
        assert got[r, 8] == (t.min() if len(t) else np.inf) and got[r, 9] == (t.max() if len(t) else -np.inf)
    whole = mref.region_stats(values, weights, None, None, 1)
    assert whole[0, 0] == whole[0, 1] == n and whole[0, 2] == np.isfinite(values).sum()
    empty = mref.region_stats(values, weights, np.full(n, 5, np.int32), None, 2)
    assert np.array_equal(empty, np.tile(mref.REGION_CLEAR, (2, 1)))


def test_the_record_on_hand_made_slots():
    from oai_analysis_2_amd.thickness import CartilageMorphometry, KneeThickness, RegionMorphometry, morphometry_rows
    inf = float("inf")
    empty = RegionMorphometry.from_slots("TC", "z_lt_50", [0.0] * 8 + [inf, -inf, 0.0, 0.0])
    assert empty.n_vertices == 0 and empty.area_mm2 == 0.0 and empty.denuded_mm2 == 0.0
    for name in ("denuded_fraction", "mean_thickness_covered", "mean_thickness_total", "std", "min", "max", "vertex_mean", "vertex_std"):
        assert math.isnan(getattr(empty, name)), name
    # all denuded: 10 vertices of area 2.5 each, none covered
    bare = RegionMorphometry.from_slots("FC", "all", [10.0, 0.0, 0.0, 25.0, 0.0, 0.0, 0.0, 0.0, inf, -inf, 0.0, 0.0])
    assert (bare.area_mm2, bare.covered_mm2, bare.denuded_mm2, bare.denuded_fraction) == (25.0, 0.0, 25.0, 1.0)
    assert bare.mean_thickness_total == 0.0 and math.isnan(bare.mean_thickness_covered) and math.isnan(bare.std) and math.isnan(bare.vertex_mean)
    # min == max: the deviations are exactly 0 whatever the sums rounded to (0.1 is not exact: sum w t t / sum w - mean^2 != 0)
    t = float(np.float32(0.1))
    w = [0.3, 1.7, 2.9]
    one = RegionMorphometry.from_slots("FC", "all", [4.0, 3.0, 3.0, 6.0, sum(w), sum(w), sum(x * t for x in w), sum(x * t * t for x in w), t, t, 3 * t, 3 * t * t],
                                       space="patient", cover=0.5)
    assert one.std == 0.0 and one.vertex_std == 0.0 and one.min == one.max == t
    assert one.mean_thickness_covered == sum(x * t for x in w) / sum(w) and one.mean_thickness_total == sum(x * t for x in w) / 6.0
    assert one.denuded_mm2 == 6.0 - sum(w) and one.denuded_fraction == (6.0 - sum(w)) / 6.0 and (one.space, one.cover) == ("patient", 0.5)
    assert (one.n_vertices, one.n_covered, one.n_measured) == (4, 3, 3)
    # two values: weighted against unweighted
    two = RegionMorphometry.from_slots("TC", "all", [2.0, 2.0, 2.0, 4.0, 4.0, 4.0, 3.0 * 1.0 + 1.0 * 3.0, 3.0 * 1.0 + 1.0 * 9.0, 1.0, 3.0, 4.0, 10.0])
    assert two.mean_thickness_covered == 1.5 and two.vertex_mean == 2.0 and two.vertex_std == 1.0 and two.std == math.sqrt(3.0 - 2.25)
    # a cartilage that could not be measured keeps the area and nothing else
    failed = RegionMorphometry.from_slots("FC", "all", [10.0, 0.0, 0.0, 25.0, 0.0, 0.0, 0.0, 0.0, inf, -inf, 0.0, 0.0], failed=True)
    assert failed.area_mm2 == 25.0 and failed.n_vertices == 10 and math.isnan(failed.denuded_mm2) and math.isnan(failed.mean_thickness_total)
    knee = KneeThickness(np.zeros(1, np.float32), np.zeros(1, np.float32),
                         morphometry={"FC": CartilageMorphometry("FC", bare), "TC": CartilageMorphometry("TC", two, {"z_lt_50": empty})})
    rows = morphometry_rows(knee)
    assert [(r["kind"], r["region"]) for r in rows] == [("FC", "all"), ("TC", "all"), ("TC", "z_lt_50")]
    assert rows[0]["denuded_mm2"] == 25.0 and set(rows[0]) >= {"area_mm2", "covered_mm2", "mean_thickness_covered", "space", "cover", "n_measured"}
    assert knee.morphometry["TC"]["z_lt_50"] is empty and knee.morphometry["TC"]["all"] is two
    assert morphometry_rows(KneeThickness(np.zeros(1, np.float32), np.zeros(1, np.float32))) == []
