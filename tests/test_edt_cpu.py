"""CPU: the numpy restatement of the surface-distance QC (tests/edt_ref.py) -- the exhaustive separable distance transform against
the brute-force minimum bit for bit, both against scipy, the surface rule and the surface-distance figures against the MedPy recipe on
scipy, analytic cases, and the argument checks of oai_mask_surface / oai_edt / oai_surface_distance (which touch no GPU); and the restated summation order of csrc/ordered_reduce.h
(tests/ordered_reduce_ref.py) on the inputs that tests/test_edt_gpu.py pins the device with."""
import ctypes as C
import math

import numpy as np
import pytest

import edt_ref as er
import ordered_reduce_ref as orr

DENSITIES = (0.003, 0.05)


def _medpy_surface_distances(result, reference, spacing_xyz):
    """medpy.metric.binary.__surface_distances on scipy: the border of each mask by erosion, the transform of the reference's."""
    ndi = pytest.importorskip("scipy.ndimage")
    footprint = ndi.generate_binary_structure(3, 1)
    result_border = result ^ ndi.binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ ndi.binary_erosion(reference, structure=footprint, iterations=1)
    dt = ndi.distance_transform_edt(~reference_border, sampling=tuple(spacing_xyz)[::-1])
    return dt[result_border]


def _figures(map_a, map_b, spacing, percentiles=(95.0,)):
    """The restated chain on two maps: surfaces, float32 distance maps of the brute-force transform, the eight figures."""
    sa, sb = er.surface_ref(map_a), er.surface_ref(map_b)
    to_a, to_b = er.edt_dist32(er.edt_sq_brute(sa, spacing)), er.edt_dist32(er.edt_sq_brute(sb, spacing))
    return er.surface_distance_ref(sa, to_b, sb, to_a, percentiles)


@pytest.mark.parametrize("spacing", er.SPACINGS)
@pytest.mark.parametrize("shape", er.SHAPES_SMALL)
def test_separable_form_equals_brute_force_bitwise_and_scipy(shape, spacing):
    ndi = pytest.importorskip("scipy.ndimage")
    for density in DENSITIES:
        f = er.sparse_features(shape, density, seed=11)
        assert f.any()
        brute, lines = er.edt_sq_brute(f, spacing), er.edt_sq_lines(f, spacing)
        assert np.array_equal(brute, lines)
        want = ndi.distance_transform_edt(f == 0, sampling=spacing[::-1])
        got = np.sqrt(brute)
        rel = float(np.max(np.abs(got - want) / np.where(want > 0, want, 1.0)))
        print(shape, spacing, density, "largest relative error against scipy", rel)
        # three multiplies, three squares, two adds and a square root, each correctly rounded to 2^-53 relative; sums of non-negative
        # terms do not amplify
        assert rel <= 1e-15 and np.array_equal(got == 0, want == 0)
    none = np.zeros(shape, np.uint8)
    assert np.isposinf(er.edt_sq_brute(none, spacing)).all() and np.isposinf(er.edt_sq_lines(none, spacing)).all()
    assert not er.edt_sq_lines(np.ones(shape, np.uint8), spacing).any()


@pytest.mark.parametrize("shape", er.SHAPES_SMALL)
def test_surface_rule_is_the_erosion_recipe(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    m = er.blobs(shape, seed=3, roll=(2, 5, 3))
    m[0, 0, 0], m[-1, -1, -1], m[1, 2, 3] = np.nan, np.inf, -np.inf
    A = er.in_set(m)
    assert A[0].any() and A[:, 0].any() and A[:, :, 0].any() and not A[0, 0, 0] and not A[-1, -1, -1]      # the set touches the border
    assert np.array_equal(er.surface_ref(m, 0.5, 1).astype(bool), A ^ ndi.binary_erosion(A, ndi.generate_binary_structure(3, 1)))
    assert np.array_equal(er.surface_ref(m, 0.5, 0).astype(bool), A) and np.array_equal(er.surface_ref(m, 0.5, 2).astype(bool), ~A)


@pytest.mark.parametrize("spacing", er.SPACINGS)
def test_figures_against_the_medpy_recipe(spacing):
    shape = (12, 20, 24)
    a, b = er.blobs(shape, seed=5, roll=(1, 2, 3)), er.blobs(shape, seed=5, roll=(2, 4, 1))
    got = _figures(a, b, spacing)
    ab = _medpy_surface_distances(er.in_set(a), er.in_set(b), spacing)
    ba = _medpy_surface_distances(er.in_set(b), er.in_set(a), spacing)
    assert (got["n_a"], got["n_b"]) == (ab.size, ba.size) and ab.size and ba.size
    pooled = np.concatenate([ab, ba])
    want = dict(assd=pooled.mean(), hausdorff=pooled.max(), hd95=np.percentile(pooled, 95))
    have = dict(assd=got["assd"], hausdorff=got["hausdorff"], hd95=float(got["percentiles"][0]))
    print(spacing, have, want)
    for k in want:                                                     # float32 storage of the distances: 2^-24, with margin
        assert abs(have[k] - want[k]) <= 1e-6 * want[k], k


def test_analytic_cases():
    shape, spacing = (12, 20, 24), er.SPACINGS[1]
    sx, sy, sz = spacing
    one, other = er.box(shape, (2, 3, 4), (1, 1, 1)), er.box(shape, (7, 15, 20), (1, 1, 1))
    d = np.float32(math.sqrt((16 * sx) ** 2 + (12 * sy) ** 2 + (5 * sz) ** 2))
    got = _figures(one, other, spacing, (0.0, 95.0))
    assert (got["n_a"], got["n_b"]) == (1, 1)
    assert abs(got["max_ab"] - d) <= np.spacing(d) and got["max_ab"] == got["max_ba"] == got["sum_ab"] == got["sum_ba"] == got["assd"]
    assert got["hausdorff"] == got["max_ab"] and [float(p) for p in got["percentiles"]] == [got["max_ab"]] * 2
    m = er.blobs(shape, seed=8, roll=(3, 1, 2))
    same = _figures(m, m, spacing, (50.0, 100.0))
    assert same["n_a"] == same["n_b"] > 0
    assert [same[k] for k in ("sum_ab", "sum_ba", "max_ab", "max_ba", "assd", "hausdorff")] == [0.0] * 6 and not any(same["percentiles"])
    b6 = er.box(shape, (3, 4, 5), (6, 11, 9))
    for sp in er.SPACINGS:                                             # a box against itself shifted 3 voxels along x
        got = _figures(b6, np.roll(b6, 3, axis=2), sp)
        assert got["n_a"] == got["n_b"] == 2 * (6 * 11 + 6 * 9 + 11 * 9) - 4 * (6 + 11 + 9) + 8
        assert got["hausdorff"] == float(np.float32(3 * np.float64(sp[0])))
    empty = _figures(m, np.zeros(shape, np.float32), spacing)
    assert empty["n_a"] == same["n_a"] and empty["n_b"] == 0
    assert all(math.isnan(empty[k]) for k in ("sum_ab", "sum_ba", "max_ab", "max_ba", "assd", "hausdorff")) and math.isnan(empty["percentiles"][0])


def test_argument_checks_of_the_surface_distance_entry_points():
    """Bad arguments come back as a non-zero status with a message -- no GPU is touched before the checks."""
    from oai_analysis_2_amd import _lib
    lib = _lib.load()
    dummy = (C.c_float * 8)()
    big = 1 << 30
    sp = lambda *v: (C.c_double * 3)(*v)
    err = lib.oai_last_error
    assert lib.oai_mask_surface(None, 2, 2, 2, 0.5, 1, dummy, None) != 0 and b"null" in err()
    assert lib.oai_mask_surface(dummy, 2, 2, 2, 0.5, 1, None, None) != 0 and b"null" in err()
    assert lib.oai_mask_surface(dummy, 2, 2, 2, 0.5, 3, dummy, None) != 0 and b"mode" in err()
    assert lib.oai_mask_surface(dummy, 2, 2, 2, float("nan"), 1, dummy, None) != 0 and b"NaN" in err()
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (32768, 2, 2), (2, 32768, 2), (2, 2, 32768)):
        assert lib.oai_mask_surface(dummy, *dims, 0.5, 1, dummy, None) != 0 and b"every axis" in err()
        assert lib.oai_edt(dummy, *dims, sp(1, 1, 1), 1.0, 0, dummy, None, dummy, big, None, None) != 0 and b"every axis" in err()
        assert lib.oai_edt_workspace_bytes(*dims) == 0
    need = lib.oai_edt_workspace_bytes(2, 3, 4)
    assert need >= 6 * 24 + 4 * 6 and lib.oai_edt_workspace_bytes(32767, 1, 1) > 0
    for args in ((None, dummy, dummy), (dummy, None, dummy), (dummy, dummy, None)):
        assert lib.oai_edt(args[0], 2, 3, 4, sp(1, 1, 1), 1.0, 0, args[1], None, args[2], big, None, None) != 0 and b"null" in err()
    assert lib.oai_edt(dummy, 2, 3, 4, None, 1.0, 0, dummy, None, dummy, big, None, None) != 0 and b"null" in err()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for c in range(3):
            v = [1.0, 1.0, 1.0]
            v[c] = bad
            assert lib.oai_edt(dummy, 2, 3, 4, sp(*v), 1.0, 0, dummy, None, dummy, big, None, None) != 0 and b"spacing" in err()
    for scale in (2.0, 0.0, float("nan")):
        assert lib.oai_edt(dummy, 2, 3, 4, sp(1, 1, 1), scale, 0, dummy, None, dummy, big, None, None) != 0 and b"scale" in err()
    assert lib.oai_edt(dummy, 2, 3, 4, sp(1, 1, 1), -1.0, 1, dummy, None, dummy, need - 1, None, None) != 0 and b"oai_edt: workspace" in err()
    pct = lambda *v: (C.c_float * 2)(*v)
    call = lambda *a, n=8, p=pct(95, 50), k=1, ws=big, out=dummy: lib.oai_surface_distance(*a, n, p, k, dummy, ws, out, None)
    four = (dummy, dummy, dummy, dummy)
    for i in range(4):
        assert call(*[None if j == i else dummy for j in range(4)]) != 0 and b"null" in err()
    assert call(*four, out=None) != 0 and b"null" in err()
    assert call(*four, p=None) != 0 and b"null" in err()
    assert call(*four, n=-1) != 0 and b"negative" in err()
    assert call(*four, k=3) != 0 and b"percentiles" in err()
    assert call(*four, k=-1) != 0 and b"percentiles" in err()
    for bad in (-0.5, 100.5, float("nan")):
        assert call(*four, p=pct(50, bad), k=2) != 0 and b"outside" in err()
    need = lib.oai_surface_distance_workspace_bytes(8)
    assert need > 0 and lib.oai_surface_distance_workspace_bytes(-1) == 0
    assert lib.oai_surface_distance_workspace_bytes(384 * 384 * 160) == lib.oai_surface_distance_workspace_bytes(1 << 40)      # the grid is capped
    assert call(*four, ws=need - 1) != 0 and b"oai_surface_distance: workspace" in err()


@pytest.mark.parametrize("n", orr.ORDER_SIZES)
def test_restated_order_is_a_valid_sum_and_not_the_serial_one(n):
    """The restated tree is a summation (within the any-order bound of the exactly rounded sum), and from two blocks on it is
    distinguishable from the plain left-to-right sum: that is what lets the GPU test tell orders apart."""
    (sa, db, sb, da), want, terms, exact, serial = orr.order_case(n)
    assert (want[0], want[1]) == (int(sa.sum()), int(sb.sum())) == (terms[0].size, terms[1].size) and want[0] >= 1 and want[1] >= 1
    assert (want[4], want[5]) == (terms[0].max(), terms[1].max())
    for k in (0, 1):
        got = float(want[2 + k])
        print(n, "direction", k, "terms", terms[k].size, "restated", got.hex(), "serial", serial[k].hex(), "fsum", exact[k].hex())
        assert abs(got - exact[k]) <= terms[k].size * 2.0 ** -52 * exact[k]
        if n >= 1025:
            assert got != serial[k]
        if terms[k].size == 1:
            assert got == exact[k] == serial[k]


def test_restated_tree_on_a_hand_checked_block():
    """A case small enough to write the order out by hand (lanes 0, 1, 32 and 33 of wave 0, and lane 0 of wave 2), sums of small
    integers, which no order rounds, and the runs of the finish step."""
    v = np.zeros((orr.KT, 1))
    v[[0, 1, 32, 33, 128], 0] = [1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53]
    # off = 32: lane 0 = 1 + 2^-53 = 1 (ties to even), lane 1 = 2^-53 + 2^-53 = 2^-52; off = 1: lane 0 = 1 + 2^-52; then wave 2: ties to even, up
    assert orr.block_reduce(v, ("add",))[0] == (1.0 + 2.0 ** -52) + 2.0 ** -52
    assert float(np.add.accumulate(v[:, 0])[-1]) == 1.0                    # left to right every 2^-53 is lost
    ints = np.arange(orr.KT * 3, dtype=np.float64).reshape(orr.KT, 3)
    assert np.array_equal(orr.block_reduce(ints, ("add", "min", "max")), [ints[:, 0].sum(), 1.0, ints[:, 2].max()])
    slots = np.arange(600.0).reshape(300, 2)                               # 300 slots: runs of two, threads 150.. stay cleared
    runs = orr.reduce_slots(slots, [0.0, -np.inf], ("add", "max"))
    assert np.array_equal(runs[:150, 0], slots[0::2, 0] + slots[1::2, 0]) and np.array_equal(runs[:150, 1], slots[1::2, 1])
    assert np.array_equal(runs[150:], np.tile([0.0, -np.inf], (orr.KT - 150, 1)))
    assert np.array_equal(orr.finish(slots, [0.0, -np.inf], ("add", "max")), [slots[:, 0].sum(), 599.0])
