"""CPU: the edge cases of tests/thickness_map_cases.py reach what tests/test_thickness_map_edges_gpu.py needs them to reach (computed
from the restatements alone, so that the GPU tests cannot pass vacuously), and the restated projection reproduces the reference's own
outputs on its smallest inputs (tests/golden/thickness_projection_edges.npz)."""
import os

import numpy as np
import pytest

import thickness_map_cases as cases
import thickness_map_ref as tref


def _is_float32(a):
    a = np.asarray(a)
    return a.dtype == np.float32


def _angle_diff(a, b):
    return np.abs((a - b + np.pi) % (2 * np.pi) - np.pi)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "thickness_projection_edges.npz")))


def test_lattice_case_is_mostly_exact_ties():
    c = cases.lattice_case()
    assert len(c.tgt) == 13824 and c.vals.shape == (len(c.src), 9)
    out, margin, count, d2, j = cases.map_reference(c)
    D = tref.pairwise_d2(c.tgt, c.src)
    two = np.partition(D, 1, axis=1)[:, :2]
    fallback = count == 0
    stats = {"margin == 0": (margin == 0).mean(), "a source at d2 == r^2": (D == 1.0).any(axis=1).mean(),
             "fallback with an exact tie": (fallback & (two[:, 0] == two[:, 1])).mean()}
    print(f"{len(c.src)} sources; " + "; ".join(f"{k}: {v:.1%}" for k, v in stats.items()) + f"; largest fallback d2 {d2[fallback].max()}")
    assert stats["margin == 0"] >= 0.25 and stats["a source at d2 == r^2"] >= 0.02 and stats["fallback with an exact tie"] >= 0.20
    # a fallback whose nearest point is more than two cells away (the cells are 1.0001 wide)
    assert d2[fallback].max() > (2 * 1.0001 * np.sqrt(3.0)) ** 2
    # the coincident points: some target's tie is between two indices of one position
    same = (c.src[j] == c.src[np.argsort(D, axis=1, kind="stable")[:, 1]]).all(axis=1) & (two[:, 0] == two[:, 1])
    assert same.any()
    # integer values and lattice points: the fp64 sums are exact in any order
    assert np.array_equal(c.vals, np.round(c.vals)) and np.array_equal(c.src, np.round(c.src)) and np.array_equal(2 * c.tgt, np.round(2 * c.tgt))


def test_cross_ring_case_ties_across_two_rings():
    from oai_analysis_2_amd import mesh_processing as mp
    c = cases.cross_ring_case()
    h, dims, lo = mp._grid_from_params(c.src.min(axis=0).astype(np.float64), c.src.max(axis=0).astype(np.float64), c.radius)
    ring = np.abs(tref.grid_cells(c.src, h, dims, lo) - tref.grid_cells(c.tgt, h, dims, lo)).max(axis=1)
    D = tref.pairwise_d2(c.tgt, c.src)[0]
    assert ring[0] == 3 and ring[1] == 2                       # the smaller index lies in the farther ring
    assert D[0] == D[1] == 9.0 and (D[2:] > 9.0).all()
    assert cases.map_reference(c)[4][0] == 0


def test_degenerate_tile_and_nan_cases_reach_their_edges():
    from oai_analysis_2_amd import mesh_processing as mp
    planar, coincident, line = cases.degenerate_cases()
    dims = lambda c: mp._grid_from_params(c.src.min(axis=0).astype(np.float64), c.src.max(axis=0).astype(np.float64), c.radius)[1]
    assert dims(planar)[2] == 1 and dims(planar)[0] > 4
    assert tuple(dims(coincident)) == (1, 1, 1) and len(coincident.src) == 600
    assert tuple(dims(line)) == (513, 1, 1)
    for c in (planar, coincident, line):
        count = cases.map_reference(c)[2]
        assert (count > 0).any() and (count == 0).any(), c.name     # both the mean and the fallback
    assert (tref.pairwise_d2(coincident.tgt, coincident.src[:1]) == 1.0).any()
    for n_src in cases.TILE_N_SRC:
        for n_tgt in cases.TILE_N_TGT:
            c = cases.tile_case(n_src, n_tgt)
            assert c.src.shape == (n_src, 3) and c.tgt.shape == (n_tgt, 3) and c.vals.shape == (n_src, 9)
    c = cases.tile_case(1025, 257)
    out, margin, count, d2, j = cases.map_reference(c)
    assert (margin == 0).mean() > 0.25 and (j >= 0).all() and j.max() < len(cases.lattice_case().src)   # ties go to the first copy
    some, every = cases.nan_cases()
    bad = ~np.isfinite(some.src).all(axis=1)
    assert bad[0] and np.isnan(some.src[bad]).all(axis=1).sum() == 6 and bad.sum() == 12
    assert (np.isnan(some.src[:, 0]) & np.isfinite(some.src[:, 1])).sum() == 6
    out, margin, count, d2, j = cases.map_reference(some)
    assert not bad[j[j >= 0]].any() and (j[-2:] == -1).all() and np.isinf(d2[-2:]).all() and (count[-2:] == 0).all()
    assert (out[-2:].view(np.uint32) == cases.NAN_BITS).all() and np.isfinite(out[:-2]).all()
    out, margin, count, d2, j = cases.map_reference(every)
    assert (out.view(np.uint32) == cases.NAN_BITS).all() and (count == 0).all() and np.isinf(d2).all() and (j == -1).all()
    for c in (some, every):
        lo, hi = cases.finite_bounds(c)
        assert mp._grid_from_params(lo, hi, c.radius)[1].max() <= 16


def test_arc_cases_fit_like_the_closed_form_and_cover_the_strides():
    arcs = {a.name: a for a in cases.arc_cases()}
    assert [len(arcs[f"arc_{n}"].verts) for n in cases.ARC_SIZES] == list(cases.ARC_SIZES)
    assert max(cases.ARC_SIZES) > 2 * 65536 and {255, 256, 257, 65535, 65536, 65537} <= set(cases.ARC_SIZES)
    for a in arcs.values():
        assert _is_float32(a.verts) and _is_float32(a.thickness)
        x, y = a.verts[:, 1].astype(np.float64), a.verts[:, 0].astype(np.float64)
        c, r = tref.fit_circle(x, y)
        want = (191.5, 178.25) if a.name.startswith("far") else (61.5, 48.25)
        assert np.abs(c - want).max() < 3.0 and abs(r - 31.0) < 2.0, (a.name, c, r)
        angle = np.arctan2(y - c[1], x - c[0])
        assert angle.min() < -2.0 and angle.max() > 2.0, a.name                  # the arc crosses +-pi
    a = arcs["arc_3"]
    x, y = a.verts[:, 1].astype(np.float64), a.verts[:, 0].astype(np.float64)
    c, r = tref.fit_circle(x, y)
    cc, rr = cases.circumcentre(x, y)
    assert np.abs(c - cc).max() < 1e-9 * np.abs(cc).max() and abs(r - rr) < 1e-9 * rr
    a = arcs["exact_3000"]
    x, y = a.verts[:, 1].astype(np.float64), a.verts[:, 0].astype(np.float64)
    R = np.hypot(x - 61.5, y - 48.25)
    assert np.abs(R - 31.0).max() < 8 * np.spacing(np.float32(92.5))               # the residual is float32 rounding only
    pts = cases.half_axis_points()
    assert _is_float32(pts) and np.array_equal(pts[4, :2], pts[5, :2]) and np.array_equal(pts[-1, :2], [60.0, 48.0])


def test_plateau_cases_are_anisotropic_and_split_where_stated():
    got = cases.plateau_cases()
    assert [((p.verts[:, 2] < 50).sum(), (p.verts[:, 2] >= 50).sum()) for p in got] == list(cases.PLATEAU_SIZES)
    for p in got:
        assert _is_float32(p.verts) and _is_float32(p.thickness)
        z = p.verts[:, 2]
        for half in (z < 50, z >= 50):
            w = cases.scatter_eigenvalues(p.verts[half])
            assert w[0] >= 2 * w[1] and w[1] >= 2 * w[2], (p.name, w)
        order = np.flatnonzero(z >= 50)
        assert order[0] < np.flatnonzero(z < 50)[-1] and np.flatnonzero(z < 50)[0] < order[-1]      # interleaved
    assert [int(np.isnan(p.verts[:, 2]).sum()) for p in got] == [0, 50, 0, 0]
    z = got[2].verts[:, 2]
    assert (z == np.float32(50.0)).sum() >= 8 and (z == cases.BELOW_50).sum() == 8 and cases.BELOW_50 < 50.0


@pytest.mark.parametrize("minus_first", [False, True])
@pytest.mark.parametrize("kind", list(cases.TIE_PLACEMENTS))
def test_tie_cases_tie_exactly(kind, minus_first):
    case = cases.tie_case(kind, minus_first)
    v = case.verts.astype(np.float64)
    n = len(v)
    assert _is_float32(case.verts) and np.array_equal(v, np.round(v)) and n == cases.TIE_PLACEMENTS[kind]
    slots = cases.tie_slots(kind, n)
    for s, (side, half) in enumerate((("right", v[:, 2] >= 50), ("left", v[:, 2] < 50))):
        idx = np.flatnonzero(half)
        assert np.array_equal(v[idx].mean(axis=0), cases._TIE_CENTRES[side])             # the mean is the centre exactly
        scores = tref.plateau_scores(v[idx])
        for axis in range(2):
            first, second = (int(np.searchsorted(idx, g)) for g in slots[2 * s + axis])
            assert idx[first] == slots[2 * s + axis][0] and idx[second] == slots[2 * s + axis][1]
            a = np.abs(scores[:, axis])
            assert a[first] == a[second] and scores[first, axis] == -scores[second, axis]    # bit-equal |scores|
            others = np.delete(a, [first, second])
            assert others.max() < 0.99 * a[first], (side, axis, others.max(), a[first])
            assert scores[first, axis] > 0                                                  # the rule: the earlier index scores positive
            # ... whichever of c + p, c - p stands there: the axis itself turns with the order
            p = v[idx[first]] - cases._TIE_CENTRES[side]
            assert np.array_equal(p, (-1 if minus_first else 1) * (cases._SHEAR @ np.array(((9, 0, 0), (0, 7, 0))[axis])))
        w = cases.scatter_eigenvalues(v[idx])
        assert w[0] >= 2 * w[1] and w[1] >= 2 * w[2]
    if kind == "two_strides":
        assert all(b - a == 65536 for a, b in slots) and slots[0] == (5, 5 + 65536)
    elif kind == "ends":
        assert slots[0] == (0, n - 1)
    else:
        assert slots[0] == (300, 301)


def test_edge_golden_inputs_are_float32_and_small(golden):
    for name, n in (("fc3", 3), ("fc40", 40), ("tc3_3", 6), ("tc150_60", 210)):
        for k in ("verts", "thickness"):
            a = golden[f"{name}_{k}"]
            assert len(a) == n and np.array_equal(a, a.astype(np.float32).astype(np.float64)), (name, k)
    z = golden["tc150_60_verts"][:, 2]
    assert ((z < 50).sum(), (z >= 50).sum()) == (150, 60)                          # both below 200: KernelPCA's dense path
    z = golden["tc3_3_verts"][:, 2]
    assert ((z < 50).sum(), (z >= 50).sum()) == (3, 3)


@pytest.mark.parametrize("name", ["fc3", "fc40"])
def test_restated_fc_projection_reproduces_the_reference_at_small_sizes(golden, name):
    verts, th, centre, radius = (golden[f"{name}_{k}"] for k in ("verts", "thickness", "circle_centre", "circle_radius"))
    x, y, t = tref.project_thickness(verts, th, "FC", centre=centre)
    assert _angle_diff(x, golden[f"{name}_x"]).max() < 1e-9
    assert np.array_equal(y, golden[f"{name}_y"]) and np.array_equal(t, golden[f"{name}_t"])
    sw = verts[:, [1, 0, 2]]
    c, r = tref.fit_circle(sw[:, 0], sw[:, 1])
    assert np.abs(c - centre).max() < 1e-8 * np.abs(centre).max()
    assert abs(r - radius) < 1e-8 * radius
    if name == "fc3":                                    # three points: the circle through them, both costs are rounding
        cc, rr = cases.circumcentre(sw[:, 0], sw[:, 1])
        assert np.abs(c - cc).max() < 1e-9 * np.abs(cc).max() and abs(r - rr) < 1e-9 * rr
    else:
        # no worse a minimum, up to the rounding of the cost itself: each R_i - mean R carries an error of about 2 eps R, so the
        # sum of squares one of at most 4 eps R sum |f_i| <= 4 eps R sqrt(n cost) (here 5e-13 on a cost of 8.8)
        cost, ref_cost = tref.circle_cost(sw[:, 0], sw[:, 1], c), tref.circle_cost(sw[:, 0], sw[:, 1], centre)
        assert cost <= ref_cost + 4 * np.finfo(np.float64).eps * radius * np.sqrt(len(sw) * ref_cost), (cost, ref_cost)
    x, _, _ = tref.project_thickness(verts, th, "FC")
    assert _angle_diff(x, golden[f"{name}_x"]).max() < 1e-7


@pytest.mark.parametrize("name", ["tc3_3", "tc150_60"])
def test_restated_tc_projection_reproduces_the_reference_at_small_sizes(golden, name):
    x, y, t = tref.project_thickness(golden[f"{name}_verts"], golden[f"{name}_thickness"], "TC")
    for got, ref in ((x, golden[f"{name}_x"]), (y, golden[f"{name}_y"])):
        assert np.abs(got - ref).max() < 1e-9 * (ref.max() - ref.min())
    assert np.array_equal(t, golden[f"{name}_t"])
