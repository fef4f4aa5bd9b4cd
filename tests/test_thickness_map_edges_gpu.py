"""GPU: the atlas thickness map (csrc/thickness_map.hip) against its float64 restatements at the edges the random-point tests of
tests/test_thickness_map_gpu.py leave out -- exact ties and footprint-boundary points on lattices, degenerate grids, the brute-force
tile, NaN points, every reduction beyond its first stride of 65 536, near-exact and short-arc circle fits, plateau splits at z == 50
and the sign rule on exact score ties.  The inputs are tests/thickness_map_cases.py; tests/test_thickness_map_edges_cpu.py shows that
they reach those edges.

Measured on an MI355X (each test prints its figures, pytest -s):
    circle fit, |centre - ref| / |R - ref| / angle (gates 6.1e-5 / 3.1e-5 / 1e-6):
        arc n = 3: 1.3e-13 / 1.1e-13 / 2.7e-15 (to the circumcentre 1.2e-13);  255: 7.1e-15 / 3.6e-15 / 4.4e-16;
        256: 4.1e-7 / 3.5e-7 / 1.2e-8;  257: 7.1e-9 / 5.7e-9 / 2.1e-10;  65 535: 4.3e-13 / 3.5e-13 / 1.3e-14;
        65 536: 2.6e-7 / 2.1e-7 / 7.9e-9;  65 537: 1.8e-11 / 1.4e-11 / 5.2e-13;  131 073: 9.0e-13 / 7.3e-13 / 2.8e-14;
        full ring: 0 / 0 / 4.4e-16;  40 degree arc: 5.5e-9 / 5.4e-9 / 6.4e-11;  far centre: 6.0e-8 / 4.9e-8 / 1.8e-9 (centre gate 1.9e-4);
        noise 0: 7.1e-14 / 6.0e-14 / 2.2e-15.
      Where the figure is 1e-7 rather than 1e-13 (256, 65 536, far centre) the fit stopped a Gauss-Newton step early, its cost about
      1e-12 above the reference's: presumably the next step's gain lay below the rounding of the cost sums, so that the step halving of
      oai_fit_circle turned it down.  That is 150 times inside the gate.
    half-axis angles: 0 from np.arctan2 on all ten points.
    plateaus: x and y at most 3.3e-16 of the range on every size and tie case (gate 1e-9); a flipped axis would be of the order of 1.
    reference golden: fc3 centre 9.3e-12, radius 8.6e-12; fc40 centre 9.3e-9, radius 7.9e-9 (leastsq's own stopping rule)."""
import functools
import os

import numpy as np
import pytest

import thickness_map_cases as cases
import thickness_map_ref as tref

pytestmark = pytest.mark.gpu

EMPTY_FACES = np.zeros((0, 3), np.int32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _angle_diff(a, b):
    return np.abs((a - b + np.pi) % (2 * np.pi) - np.pi)


@functools.lru_cache(maxsize=None)
def _map_reference(name):
    return cases.map_reference(_MAP_CASES[name]())


_MAP_CASES = {"lattice": cases.lattice_case, "cross_ring": cases.cross_ring_case, "some_nan": lambda: cases.nan_cases()[0],
              "all_nan": lambda: cases.nan_cases()[1]}
_MAP_CASES.update({name: (lambda k=k: cases.degenerate_cases()[k]) for k, name in enumerate(("planar", "coincident", "line"))})
_MAP_CASES.update({f"tile_{s}_{t}": functools.partial(cases.tile_case, s, t) for s in cases.TILE_N_SRC for t in cases.TILE_N_TGT})


def _check_map_attributes(name, broad_phases=(True, False)):
    """map_attributes through the public call: the reference's bits on every target"""
    from oai_analysis_2_amd import mesh_processing as mp
    case = _MAP_CASES[name]()
    ref = _map_reference(name)[0]
    for broad in broad_phases:
        out = mp.map_attributes(mp.Mesh(case.src, EMPTY_FACES, {"v": case.vals}), mp.Mesh(case.tgt, EMPTY_FACES), radius=case.radius,
                                broad_phase=broad).point_data["v"]
        assert out.dtype == np.float32 and out.shape == ref.shape
        wrong = np.flatnonzero((_bits(out) != _bits(ref)).any(axis=1))
        assert len(wrong) == 0, (name, broad, len(wrong), wrong[:5], out[wrong[:2]], ref[wrong[:2]])


def _check_footprint(name, forms=("grid", "brute"), bounds=None):
    """_point_footprint_dev in grid and in brute form: the reference's count and nearest index, the same bits for the distance"""
    from oai_analysis_2_amd import mesh_processing as mp
    case = _MAP_CASES[name]()
    _, _, count, d2, j = _map_reference(name)
    s, t = mp._dev(case.src, np.float32, (3,)), mp._dev(case.tgt, np.float32, (3,))
    for form in forms:
        grid = (bounds if bounds is not None else cases.finite_bounds(case)) if form == "grid" else None
        got_count, got_d2, got_j = (x.cpu().numpy() for x in mp._point_footprint_dev(s, t, case.radius, grid))
        assert got_count.dtype == np.int32 and got_d2.dtype == np.float64 and got_j.dtype == np.int32
        for what, got, want in (("count", got_count, count), ("nearest_j", got_j, j), ("nearest_d2", got_d2.view(np.uint64), d2.view(np.uint64))):
            wrong = np.flatnonzero(got != want)
            assert len(wrong) == 0, (name, form, what, len(wrong), wrong[:5], got[wrong[:5]], want[wrong[:5]])


def test_lattice_map_attributes_matches_bit_for_bit():
    _check_map_attributes("lattice")


def test_lattice_footprint_matches_exactly():
    _check_footprint("lattice")


def test_cross_ring_tie_goes_to_the_smaller_index():
    from oai_analysis_2_amd import mesh_processing as mp
    case = cases.cross_ring_case()
    h, dims, lo = mp._grid_from_params(case.src.min(axis=0).astype(np.float64), case.src.max(axis=0).astype(np.float64), case.radius)
    ring = np.abs(tref.grid_cells(case.src, h, dims, lo) - tref.grid_cells(case.tgt, h, dims, lo)).max(axis=1)
    assert ring[0] != ring[1] and ring[0] > ring[1]            # the smaller index lies in the farther ring of the broad phase
    assert _map_reference("cross_ring")[4][0] == 0
    _check_footprint("cross_ring")
    _check_map_attributes("cross_ring")


@pytest.mark.parametrize("name", ["planar", "coincident", "line"])
def test_degenerate_grids(name):
    _check_map_attributes(name)
    _check_footprint(name)


@pytest.mark.parametrize("n_tgt", cases.TILE_N_TGT)
@pytest.mark.parametrize("n_src", cases.TILE_N_SRC)
def test_brute_force_tile_edges(n_src, n_tgt):
    name = f"tile_{n_src}_{n_tgt}"
    _check_map_attributes(name, broad_phases=(False,))
    _check_footprint(name, forms=("brute",))


def test_nan_sources_are_never_counted_and_never_nearest():
    from oai_analysis_2_amd import mesh_processing as mp
    case = cases.nan_cases()[0]
    out, _, count, d2, j = _map_reference("some_nan")
    bad = ~np.isfinite(case.src).all(axis=1)
    assert bad[0] and not bad[j[j >= 0]].any()
    _check_footprint("some_nan")                                 # the grid over the finite points: the NaN rows land in cell 0
    _check_map_attributes("some_nan")                            # the public call: the grid from the mesh's own (NaN) bounds, and brute force
    s, v, t = mp._dev(case.src, np.float32, (3,)), mp._dev(case.vals.T, np.float32), mp._dev(case.tgt, np.float32, (3,))
    got = mp._map_attributes_dev(s, v, t, case.radius, grid=cases.finite_bounds(case)).cpu().numpy().T
    assert np.array_equal(_bits(got), _bits(out))
    # a NaN target: no finite distance
    assert (_bits(out[-2:]) == cases.NAN_BITS).all() and (count[-2:] == 0).all() and np.isinf(d2[-2:]).all() and (j[-2:] == -1).all()


def test_every_source_nan():
    _, _, count, d2, j = ref = _map_reference("all_nan")
    assert (_bits(ref[0]) == cases.NAN_BITS).all() and (count == 0).all() and (d2 == np.inf).all() and (j == -1).all()
    _check_footprint("all_nan")
    _check_map_attributes("all_nan")


def test_map_attributes_onto_no_targets():
    from oai_analysis_2_amd import mesh_processing as mp
    case = cases.cross_ring_case()
    source = mp.Mesh(case.src, EMPTY_FACES, {"v": case.vals, "Distance": case.vals[:, 0].copy(), "vec": case.vals[:, :3].copy()})
    for broad in (True, False):
        out = mp.map_attributes(source, mp.Mesh(np.zeros((0, 3), np.float32), EMPTY_FACES), broad_phase=broad)
        assert out.GetNumberOfPoints() == 0 and set(out.point_data) == {"v", "Distance", "vec"}
        assert out.point_data["v"].shape == (0, 9) and out.point_data["Distance"].shape == (0,) and out.point_data["vec"].shape == (0, 3)
        assert all(a.dtype == np.float32 for a in out.point_data.values())


# ---- circle fit and FC projection ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.arc_cases(), ids=lambda c: c.name)
def test_circle_fit_and_fc_projection_match_float64(case):
    """The project's gates (test_thickness_map_gpu.py): centre within 1e-6 max|centre|, radius within 1e-6 R, angles within 1e-6
    (wrap-aware), y == z and the thickness exactly."""
    from oai_analysis_2_amd import mesh_processing as mp
    v64 = case.verts.astype(np.float64)
    sx, sy = v64[:, 1], v64[:, 0]                                # the fitted (x, y): project_thickness swaps the columns
    ref_c, ref_r = tref.fit_circle(sx, sy)
    ref_x, ref_y, ref_t = tref.project_thickness(v64, case.thickness, "FC")
    centre, r = mp.compute_least_square_circle(case.verts[:, 1], case.verts[:, 0])
    x, y, t = mp.project_thickness(mp.Mesh(case.verts, EMPTY_FACES, {"Distance": case.thickness}), "FC")
    dc, dr, da = np.abs(centre - ref_c).max(), abs(r - ref_r), _angle_diff(x, ref_x).max()
    cost, ref_cost = tref.circle_cost(sx, sy, centre), tref.circle_cost(sx, sy, ref_c)
    print(f"{case.name}: centre {dc:.3e} (gate {1e-6 * np.abs(ref_c).max():.3e}), radius {dr:.3e} (gate {1e-6 * ref_r:.3e}), "
          f"angle {da:.3e} (gate 1e-6), cost {cost:.17g} vs {ref_cost:.17g}")
    assert centre.dtype == np.float64 and x.dtype == y.dtype == t.dtype == np.float64 and len(x) == len(case.verts)
    assert dc < 1e-6 * np.abs(ref_c).max()
    assert dr < 1e-6 * ref_r
    assert da < 1e-6
    assert np.array_equal(y, v64[:, 2]) and np.array_equal(y, ref_y)
    assert np.array_equal(t, case.thickness.astype(np.float64)) and np.array_equal(t, ref_t)
    if len(case.verts) == 3:
        cc, rr = cases.circumcentre(sx, sy)
        print(f"{case.name}: to the circumcentre {np.abs(centre - cc).max():.3e}, radius {abs(r - rr):.3e}")
        assert np.abs(centre - cc).max() < 1e-6 * np.abs(cc).max() and abs(r - rr) < 1e-6 * rr


def test_projection_angles_on_the_half_axes():
    """A given integer centre, points on the four half-axes (the -x one twice) and the centre itself: atan2's branches"""
    from oai_analysis_2_amd import mesh_processing as mp
    pts = cases.half_axis_points()
    centre = np.array([60.0, 48.0])
    emb, plot_xy = mp.get_projection_from_circle_and_vertice(pts, (centre, 31.0))
    ref = np.arctan2(pts[:, 1].astype(np.float64) - centre[1], pts[:, 0].astype(np.float64) - centre[0])
    print("angles", emb[:, 0].tolist(), "largest difference", np.abs(emb[:, 0] - ref).max())
    assert np.abs(emb[:, 0] - ref).max() <= 1e-12
    assert ref[4] == ref[5] == np.pi and ref[-1] == 0.0
    assert np.array_equal(emb[:, 1], pts[:, 2].astype(np.float64)) and np.array_equal(plot_xy[:, 1], pts[:, 2])


# ---- TC plateaus ---------------------------------------------------------------------------------------------------------------------
def _check_plateaus(case):
    from oai_analysis_2_amd import mesh_processing as mp
    ref_x, ref_y, ref_t = tref.project_thickness(case.verts.astype(np.float64), case.thickness, "TC")
    mesh = mp.Mesh(case.verts, EMPTY_FACES, {"thickness": case.thickness})
    x, y, t = mp.project_thickness(mesh, "TC")
    z = case.verts[:, 2]
    assert x.dtype == y.dtype == t.dtype == np.float64
    assert len(x) == len(y) == len(t) == len(z) - int(np.isnan(z).sum()) == len(ref_x)
    dx, dy = np.abs(x - ref_x).max() / (ref_x.max() - ref_x.min()), np.abs(y - ref_y).max() / (ref_y.max() - ref_y.min())
    print(f"{case.name}: x {dx:.3e}, y {dy:.3e} of the range (gate 1e-9)")
    # right then left, each in point order: the thickness is carried along exactly
    order = np.concatenate([np.flatnonzero(z >= 50), np.flatnonzero(z < 50)])
    assert np.array_equal(t, case.thickness[order].astype(np.float64)) and np.array_equal(t, ref_t)
    assert dx < 1e-9 and dy < 1e-9
    x2, y2, t2 = mp.project_thickness(mesh, "TC")
    assert np.array_equal(x.view(np.uint64), x2.view(np.uint64)) and np.array_equal(y.view(np.uint64), y2.view(np.uint64)) and np.array_equal(t, t2)
    return x, y


@pytest.mark.parametrize("case", cases.plateau_cases(), ids=lambda c: c.name)
def test_plateaus_match_float64(case):
    _check_plateaus(case)


@pytest.mark.parametrize("minus_first", [False, True])
@pytest.mark.parametrize("kind", list(cases.TIE_PLACEMENTS))
def test_plateau_sign_rule_on_exact_ties(kind, minus_first):
    """Two points tie exactly for the largest |score| on each axis: the earlier index scores positive (np.argmax in the restatement).
    The other tie-break flips the whole axis, an error of the size of the range."""
    _check_plateaus(cases.tie_case(kind, minus_first))


# ---- the reference's own outputs at the smallest sizes ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "thickness_projection_edges.npz")))


@pytest.mark.parametrize("name", ["fc3", "fc40"])
def test_fc_projection_matches_reference_golden_at_small_sizes(golden, name):
    from oai_analysis_2_amd import mesh_processing as mp
    verts = golden[f"{name}_verts"].astype(np.float32)
    x, y, t = mp.project_thickness(mp.Mesh(verts, EMPTY_FACES, {"Distance": golden[f"{name}_thickness"].astype(np.float32)}), "FC")
    assert x.dtype == y.dtype == t.dtype == np.float64
    assert _angle_diff(x, golden[f"{name}_x"]).max() < 1e-6
    assert np.array_equal(y, golden[f"{name}_y"]) and np.array_equal(t, golden[f"{name}_t"])
    centre, r = mp.compute_least_square_circle(verts[:, 1], verts[:, 0])
    ref_c, ref_r = golden[f"{name}_circle_centre"], golden[f"{name}_circle_radius"]
    print(f"{name}: centre {np.abs(centre - ref_c).max():.3e}, radius {abs(r - ref_r):.3e}")
    assert np.abs(centre - ref_c).max() < 1e-6 * np.abs(ref_c).max()
    assert abs(r - ref_r) < 1e-6 * ref_r


@pytest.mark.parametrize("name", ["tc3_3", "tc150_60"])
def test_tc_projection_matches_reference_golden_at_small_sizes(golden, name):
    from oai_analysis_2_amd import mesh_processing as mp
    tc = mp.Mesh(golden[f"{name}_verts"].astype(np.float32), EMPTY_FACES, {"thickness": golden[f"{name}_thickness"].astype(np.float32)})
    x, y, t = mp.project_thickness(tc, "TC")
    assert x.dtype == y.dtype == t.dtype == np.float64 and len(x) == len(golden[f"{name}_x"])
    for got, ref in ((x, golden[f"{name}_x"]), (y, golden[f"{name}_y"])):
        assert np.abs(got - ref).max() < 1e-6 * (ref.max() - ref.min())
    assert np.array_equal(t, golden[f"{name}_t"])
