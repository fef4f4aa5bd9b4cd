"""GPU: the atlas thickness map (mesh_processing.py:400-534) through csrc/thickness_map.hip -- map_attributes against the numpy
restatement (unpinned: VTK's defaults restated), project_thickness and its circle helpers against the reference's own outputs
(tests/golden/thickness_projection.npz), and the demo's chain end to end."""
import os

import numpy as np
import pytest

import thickness_map_ref as tref
from oai_analysis_2_amd.image import Image

pytestmark = pytest.mark.gpu

EMPTY_FACES = np.zeros((0, 3), np.int32)


def _ulp_close(got, ref, ulps=1):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulps * np.spacing(np.abs(ref)).astype(np.float64)


def _case(seed, n_src, n_tgt, box, far=0):
    rng = np.random.default_rng(seed)
    src = rng.uniform(0, box, size=(n_src, 3)).astype(np.float32)
    tgt = rng.uniform(-0.2 * box, 1.2 * box, size=(n_tgt, 3)).astype(np.float32)          # some targets outside the source box
    if far:
        tgt = np.concatenate([tgt, rng.uniform(-30 * box, 30 * box, size=(far, 3)).astype(np.float32)])
    data = {"Distance": rng.uniform(0.5, 4.0, n_src).astype(np.float32),
            "vec": rng.normal(size=(n_src, 3)).astype(np.float32) * 100,
            "w": rng.uniform(-1, 1, n_src).astype(np.float32)}                         # 5 components: two launches of the kernel
    return src, tgt, data


@pytest.mark.parametrize("seed,n_src,n_tgt,box,radius,far", [
    (0, 4000, 3000, 10.0, 1.0, 40),        # dense overlap: ~17 source points per footprint
    (1, 300, 2000, 40.0, 1.0, 40),         # sparse: most targets fall back to the closest point
    (2, 2500, 2500, 12.0, 2.5, 0),         # a larger radius
    (3, 1, 50, 1.0, 1.0, 10)])             # one source point
def test_map_attributes_matches_restatement(seed, n_src, n_tgt, box, radius, far):
    from oai_analysis_2_amd import mesh_processing as mp
    src, tgt, data = _case(seed, n_src, n_tgt, box, far)
    source = mp.Mesh(src, EMPTY_FACES, data)
    target = mp.Mesh(tgt, EMPTY_FACES, {"Distance": np.zeros(len(tgt), np.float32), "own": np.arange(len(tgt), dtype=np.int32)})
    vals = np.concatenate([data["Distance"][:, None], data["vec"], data["w"][:, None]], axis=1)
    ref, margin = tref.map_attributes(src, vals, tgt, radius)
    keep = margin > 1e-5                                                    # neighbour test / closest tie clear of the boundary
    assert keep.mean() > 0.95
    results = []
    for broad in (True, False):
        out = mp.map_attributes(source, target, radius=radius, broad_phase=broad)
        assert set(out.point_data) == {"Distance", "vec", "w", "own"}
        assert np.array_equal(out.point_data["own"], target.point_data["own"]) and out.verts is target.verts
        got = np.concatenate([out.point_data["Distance"][:, None], out.point_data["vec"], out.point_data["w"][:, None]], axis=1)
        assert got.dtype == np.float32 and out.point_data["vec"].shape == (len(tgt), 3)
        ok = _ulp_close(got, ref)[keep]
        assert ok.all(), (broad, np.argwhere(~ok)[:5])
        results.append(got)
    assert _ulp_close(results[0], results[1]).all()                        # grid == brute force (same neighbour sets, fp64 sums)
    again = mp.map_attributes(source, target, radius=radius, broad_phase=True)
    got = np.concatenate([again.point_data["Distance"][:, None], again.point_data["vec"], again.point_data["w"][:, None]], axis=1)
    assert np.array_equal(got.view(np.int32), results[0].view(np.int32))                                   # run to run: same bits


def test_map_attributes_grid_sums_in_cell_order():
    """The grid path's fp64 sums run over the 27 cells in (z, y, x) order, each cell in ascending point index: bit for bit against that
    restatement.  The values make the order show in the float32 result: 300 source points and, 300 indices later, a partner within 0.05
    with the opposite value, magnitudes log-uniform over 24 decades -- a footprint's exact sum is mostly 0, and what is left of it is
    the rounding of the partial sums, which depends on when each value was added."""
    from oai_analysis_2_amd import mesh_processing as mp
    rng = np.random.default_rng(4)
    a = rng.uniform(0.0, 6.0, (300, 3))
    src = np.concatenate([a, np.clip(a + rng.uniform(-0.05, 0.05, (300, 3)), 0.0, 6.0)]).astype(np.float32)
    tgt = rng.uniform(-0.5, 6.5, (200, 3)).astype(np.float32)
    v = (10.0 ** rng.uniform(-12.0, 12.0, 300) * rng.choice([-1.0, 1.0], 300)).astype(np.float32)
    vals = np.concatenate([v, -v])
    grid = mp._grid_from_params(src.min(axis=0).astype(np.float64), src.max(axis=0).astype(np.float64), 1.0)
    ref, ascending, count = tref.map_attributes_grid_order(src, vals, tgt, grid, 1.0)
    # the inputs tell the two orders apart: the restatement summed in ascending index gives other bits on >= 10 % of the targets
    many = count >= 2
    told_apart = (ref.view(np.int32) != ascending.view(np.int32))[many].mean()
    print(f"grid order != ascending order on {told_apart:.1%} of {many.sum()} targets; {int((count == 0).sum())} empty footprints")
    assert many.sum() >= 150 and told_apart >= 0.10
    out = mp.map_attributes(mp.Mesh(src, EMPTY_FACES, {"v": vals}), mp.Mesh(tgt, EMPTY_FACES), radius=1.0, broad_phase=True).point_data["v"]
    assert out.dtype == np.float32 and out.shape == (200,)
    full = count > 0
    differ = np.flatnonzero(out.view(np.int32)[full] != ref.view(np.int32)[full])
    assert len(differ) == 0, (len(differ), differ[:5])


def test_map_attributes_empty_source_raises():
    from oai_analysis_2_amd import mesh_processing as mp
    with pytest.raises(ValueError):
        mp.map_attributes(mp.Mesh(np.zeros((0, 3), np.float32), EMPTY_FACES, {"Distance": np.zeros(0, np.float32)}),
                          mp.Mesh(np.ones((4, 3), np.float32), EMPTY_FACES))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "thickness_projection.npz")))


def _angle_diff(a, b):
    return np.abs((a - b + np.pi) % (2 * np.pi) - np.pi)


def test_project_thickness_matches_reference_golden(golden):
    from oai_analysis_2_amd import mesh_processing as mp
    fc = mp.Mesh(golden["fc_verts"].astype(np.float32), EMPTY_FACES, {"Distance": golden["fc_thickness"].astype(np.float32)})
    x, y, t = mp.project_thickness(fc, "FC")
    assert x.dtype == y.dtype == t.dtype == np.float64
    assert _angle_diff(x, golden["fc_x"]).max() < 1e-6
    assert np.array_equal(y, golden["fc_y"]) and np.array_equal(t, golden["fc_t"])
    tc = mp.Mesh(golden["tc_verts"].astype(np.float32), EMPTY_FACES, {"thickness": golden["tc_thickness"].astype(np.float32)})   # the only array
    x, y, t = mp.project_thickness(tc, "TC")
    assert x.dtype == y.dtype == t.dtype == np.float64 and len(x) == len(golden["tc_x"])
    for got, ref in ((x, golden["tc_x"]), (y, golden["tc_y"])):
        assert np.abs(got - ref).max() < 1e-6 * (ref.max() - ref.min())
    assert np.array_equal(t, golden["tc_t"])
    x2, y2, _ = mp.project_thickness(tc, "TC")
    assert np.array_equal(x, x2) and np.array_equal(y, y2)                 # deterministic reductions


def test_circle_helpers_match_reference_golden(golden):
    from oai_analysis_2_amd import mesh_processing as mp
    sw = golden["fc_verts"][:, [1, 0, 2]]
    centre, r = mp.compute_least_square_circle(sw[:, 0], sw[:, 1])
    assert centre.dtype == np.float64 and centre.shape == (2,)
    assert np.abs(centre - golden["circle_centre"]).max() < 1e-6 * np.abs(golden["circle_centre"]).max()
    assert abs(r - golden["circle_radius"]) < 1e-6 * golden["circle_radius"]
    (c2, r2), (zmin, zmax) = mp.get_cylinder(sw)
    assert np.array_equal(c2, centre) and r2 == r and zmin == sw[:, 2].min() and zmax == sw[:, 2].max()
    emb, plot_xy = mp.get_projection_from_circle_and_vertice(sw, (golden["circle_centre"], golden["circle_radius"]))
    assert _angle_diff(emb[:, 0], golden["embedded"][:, 0]).max() < 1e-6 and np.array_equal(emb[:, 1], golden["embedded"][:, 1])
    ref = golden["plot_xy"]
    assert np.abs(plot_xy - ref).max() < 1e-6 * (np.abs(ref).max())


def test_project_thickness_errors():
    from oai_analysis_2_amd import mesh_processing as mp
    v = np.random.default_rng(0).uniform(0, 40, size=(100, 3)).astype(np.float32)          # every z < 50: the right plateau is empty
    with pytest.raises(ValueError):
        mp.project_thickness(mp.Mesh(v, EMPTY_FACES, {"Distance": np.ones(100, np.float32)}), "TC")
    with pytest.raises(ValueError):
        mp.project_thickness(mp.Mesh(v, EMPTY_FACES, {"a": np.ones(100, np.float32), "b": np.ones(100, np.float32)}), "FC")


def _bowl(shift_x=0.0, T=6.0):
    D, H, W = 48, 96, 96
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    x = x - shift_x
    r = np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4 + (y + 30) ** 2)
    sig = lambda t: 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))
    prob = sig(2.0 * (np.abs(r - 60.0) - T / 2)) * sig(2.0 * (np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4) - 30))
    return Image(prob.astype(np.float32), [1.0, 1.0, 1.0])


def test_thickness_map_end_to_end():
    """FullDemo's chain on a curved shell of known thickness and a slightly shifted 'atlas' shell: get_thickness_mesh ->
    map_attributes onto the atlas inner mesh -> project_thickness."""
    from oai_analysis_2_amd import mesh_processing as mp
    T = 6.0
    distance_inner, _ = mp.get_thickness_mesh(_bowl(0.0, T), mesh_type="TC", min_cells=100)
    atlas_inner, _ = mp.get_thickness_mesh(_bowl(1.5, T), mesh_type="TC", min_cells=100)
    mapped = mp.map_attributes(distance_inner, atlas_inner)
    assert mapped.GetNumberOfPoints() == atlas_inner.GetNumberOfPoints()
    x, y, t = mp.project_thickness(mapped, mesh_type="FC")
    assert len(x) == len(y) == len(t) == atlas_inner.GetNumberOfPoints()
    src = distance_inner.point_data["Distance"]
    assert np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(t).all()
    assert t.min() >= src.min() and t.max() <= src.max()
    assert abs(np.median(t) - T) < 0.15 * T, np.median(t)
