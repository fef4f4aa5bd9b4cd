"""CPU: the case list of tests/mesh_split_cases.py is worth running on the device.  The restatement (tests/mesh_split_ref.py) shows
that the list reaches every ending of the Lloyd loop, a best run other than init 0, both orientations, side 0, a clipped candidate
and a draw of 0, and that every case is decided in fp64: each comparison a fit makes is far enough from going the other way that
the order of a sum cannot turn it.  These are conditions on the inputs; tests/test_mesh_split_edges_gpu.py then compares every face.

The bounds: an fp64 sum of n terms is off by at most about n eps relative, 8e-12 for the largest case (65836 faces); the margins
asked for are more than 100 times that."""
import numpy as np
import pytest

import mesh_split_cases as mc
import mesh_split_ref as sref

LABEL_MARGIN, CANDIDATE_MARGIN, TOL_MARGIN, INERTIA_GAP = 1e-9, 1e-10, 1e-6, 1e-9
TRIAL_MARGIN = FLIP_MARGIN = 1e-9          # the two comparisons the fit makes besides: between the local trials, and the sign of mean n_y
N_INITS, MAX_ITERS = (1, 5), (1, 2, 300)


def _check_margins(name, evidence):
    for s, ev in enumerate(evidence):
        what = f"{name} slab {s}"
        assert ev.label_margin >= LABEL_MARGIN, what
        assert ev.candidate_margin >= CANDIDATE_MARGIN, what
        assert ev.trial_margin >= TRIAL_MARGIN, what
        assert ev.tol_margin >= TOL_MARGIN, what
        assert ev.inertia_gap >= INERTIA_GAP, what
        assert ev.flip_margin >= FLIP_MARGIN, what


@pytest.fixture(scope="module")
def runs():
    """(case, n_init, max_iter) -> (side, n_iter, evidence, slab sizes) over the whole list"""
    out = {}
    for case in mc.cases():
        sizes = sref.features(case.verts, case.faces, case.mesh_type)[1].sum(axis=1)
        for n_init in N_INITS:
            for max_iter in MAX_ITERS:
                out[case.name, n_init, max_iter] = sref.split_sides_draws(case.verts, case.faces, case.mesh_type, n_init, max_iter) + (sizes,)
    return out


def test_every_case_is_decided_in_fp64(runs):
    low = {k: np.inf for k in ("label_margin", "candidate_margin", "trial_margin", "tol_margin", "inertia_gap", "flip_margin")}
    for (name, n_init, max_iter), (_, _, evidence, _) in runs.items():
        _check_margins(f"{name} n_init={n_init} max_iter={max_iter}", evidence)
        for ev in evidence:
            for k in low:
                low[k] = min(low[k], getattr(ev, k))
    print("least margins over the case list: " + ", ".join(f"{k} {v:.2e}" for k, v in low.items()))


def test_the_list_reaches_every_ending_and_every_choice(runs):
    stops, best, flips, side0 = set(), set(), set(), 0
    for (name, n_init, max_iter), (side, n_iter, evidence, _) in runs.items():
        for ev, it in zip(evidence, n_iter):
            stops.update(ev.stops)
            best.add(ev.best)
            flips.add(ev.flipped)
            assert it == ev.n_iters[ev.best] and it <= max_iter
        side0 += int((side == 0).sum())
    assert stops == {"strict", "tol", "max_iter"}
    assert best - {0}, "no slab whose best run is a later init"
    assert flips == {True, False}
    assert side0 > 0
    # each ending also at max_iter 1 and 2, and more than two iterations ending on tol in a TC (six-column) fit
    for max_iter in (1, 2):
        assert any("max_iter" in ev.stops for (n, i, m), r in runs.items() if m == max_iter for ev in r[2])
    assert any(ev.stops[ev.best] == "tol" and it > 2 for (n, i, m), r in runs.items() if n.startswith("arch-tc") for ev, it in zip(r[2], r[1]))


def test_every_size_is_one_fit_of_each_width(runs):
    sizes = {"TC": set(), "FC": set()}
    for case in mc.cases():
        sizes[case.mesh_type].update(int(n) for n in runs[case.name, 1, 300][3])
    assert sizes["TC"] >= set(mc.SIZES) and sizes["FC"] >= set(mc.SIZES)
    assert {len(c.faces) for c in mc.cases() if c.name.startswith("sheets-fc-") and "slabs" not in c.name} == set(mc.FC_TOTALS)


def test_hand_picked_draws_clip_and_draw_zero(runs):
    by_name = {c.name: c for c in mc.cases()}
    clipped = zero = False
    for name in mc.HAND_DRAW_MESHES:
        case, sizes = by_name[name], runs[name, 1, 300][3]
        for kind in ("clip", "zero", "last"):
            side, n_iter, evidence = sref.split_sides_draws(case.verts, case.faces, case.mesh_type, 1, 300, mc.hand_draws(kind, sizes))
            _check_margins(f"{name} {kind}", evidence)
            for ev, n in zip(evidence, sizes):
                first, u0, u1 = ev.draws[0]
                if kind == "clip":
                    assert set(ev.raw_candidates[0]) <= {n - 1, n}         # the last sample, with or without the clip
                    clipped |= n in ev.raw_candidates[0]
                if kind == "zero":
                    assert u0 == 0.0 and ev.raw_candidates[0][0] == 0
                    zero = True
                if kind == "last":
                    assert first == n - 1
        with pytest.raises(RuntimeError, match="a cluster became empty"):
            sref.split_sides_draws(case.verts, case.faces, case.mesh_type, 1, 300, mc.hand_draws("empty", sizes))
    assert clipped and zero


def test_kmeans_still_draws_from_randomstate_5():
    X = np.random.default_rng(0).normal(size=(300, 6))
    first, uniforms = sref.draws(300, 5)
    rs = np.random.RandomState(5)
    for r in range(5):
        assert first[r] == rs.choice(300, p=np.ones(300) / 300) and np.array_equal(uniforms[r], rs.uniform(size=2))
    a, b = sref.kmeans(X, 5), sref.kmeans_draws(X, first, uniforms, 5)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and len(b[5].stops) == 5


def test_slab_masks_report_faces_in_no_slab_and_in_two():
    x = np.array([0.0, 0.1, 0.5, 0.9, 1.0, 2.0, 2.9, 3.0])
    masks, none, double = sref.slab_masks(x)
    assert masks.shape == (3, 8) and none.tolist() == [7] and double.tolist() == []          # the greatest x is in no half-open slab
    assert masks.sum(axis=1).tolist() == [4, 1, 2]
    # split_sides takes the later slab for a face in two: side[idx] is written in slab order
    masks[1, 3] = True
    assert np.flatnonzero(masks.sum(axis=0) > 1).tolist() == [3]
    side = np.zeros(8, np.int8)
    for s, m in enumerate(masks):
        side[np.flatnonzero(m)] = s + 1
    assert side[3] == 2


def test_the_big_mesh_has_every_extreme_past_the_first_stride():
    case = mc.big_case("FC")
    assert len(case.faces) == mc.BIG_FACES == 65536 + 300 and len(case.verts) > 65536
    c = sref.cell_centroids(case.verts, case.faces)
    for arr in (c, case.verts):
        for k in range(3):
            col = arr[:, k]
            assert np.flatnonzero(col == col.min()).min() >= 65536 and np.flatnonzero(col == col.max()).min() >= 65536
    for mesh_type in ("FC", "TC"):
        side, n_iter, evidence = sref.split_sides_draws(case.verts, case.faces, mesh_type)
        _check_margins(f"big {mesh_type}", evidence)
        assert (sref.features(case.verts, case.faces, mesh_type)[1].sum(axis=1) >= 2).all()


def test_degenerate_members():
    verts, faces = mc.degenerate(410, False)
    n = sref.cell_normals(verts, faces)
    assert (np.abs(n).sum(axis=1) == 0).sum() == 1                   # the face (v, v, w)
    assert faces[120, 0] == faces[120, 1]
    verts, faces = mc.bad_indices(420)
    assert faces.max() == len(verts) and faces.min() == -1
    for counts in mc.FC_SLAB_COUNTS:                                # the last face is alone at the greatest x
        verts, faces = mc.fc_slabs(300, counts)
        cx = sref.cell_centroids(verts, faces)[:, 0]
        assert np.argmax(cx) == len(faces) - 1 and (cx == cx.max()).sum() == 1
