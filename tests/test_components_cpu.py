"""CPU: the numpy restatement of the segmentation-shape QC (tests/components_ref.py) -- its labels against scipy.ndimage.label to the
element, the twelve summary slots against numpy, the cavities against binary_fill_holes, the fixed layouts, the arithmetic of
qc.segmentation_shape from two summaries -- and the argument checks of oai_label_components / oai_component_sizes, which touch no GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import components_ref as cr

STRUCTURE_RANK = {6: 1, 18: 2, 26: 3}


def _structure(ndi, connectivity):
    return ndi.generate_binary_structure(3, STRUCTURE_RANK[connectivity])


@pytest.mark.parametrize("connectivity", cr.CONNECTIVITIES)
@pytest.mark.parametrize("shape", cr.SHAPES_CPU)
def test_restatement_equals_scipy_label_to_the_element(shape, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    for density in cr.DENSITIES:
        for complement in (False, True):
            m = cr.random_mask(shape, density)
            labels, _, summary = cr.label_ref(m, connectivity=connectivity, complement=complement)
            want, k = ndi.label((m != 0) != complement, _structure(ndi, connectivity))
            assert labels.dtype == np.int32 and np.array_equal(labels, want) and int(summary[2]) == k, (shape, density, connectivity, complement)


@pytest.mark.parametrize("connectivity", cr.CONNECTIVITIES)
def test_summary_slots_against_numpy(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    shape = (9, 14, 17)
    for density in (0.1, 0.31, 0.0, 1.0):
        v = cr.as_map(cr.random_mask(shape, density))
        v[0, 0, 0], v[4, 5, 6], v[-1, -1, -1] = np.nan, np.inf, -np.inf
        for complement in (False, True):
            for min_voxels in (0, 1, 2, 5, 10 ** 6):
                labels, size_map, s = cr.label_ref(v, 0.5, connectivity, complement, min_voxels)
                the_set = cr.the_set(v, 0.5, complement)
                want, k = ndi.label(the_set, _structure(ndi, connectivity))
                assert np.array_equal(labels, want)
                sizes = np.bincount(want.ravel())[1:]
                border = np.ones(shape, bool)
                border[1:-1, 1:-1, 1:-1] = False
                touching = np.unique(want[border & (want > 0)])
                assert s[0] == v.size and s[1] == the_set.sum() == sizes.sum() and s[2] == k
                assert s[3] == (sizes.max() if k else 0) and s[4] == (int(np.flatnonzero(sizes == sizes.max())[0]) + 1 if k else 0)
                assert s[5] == (np.sort(sizes)[-2] if k > 1 else 0)
                assert s[6] == (sizes < min_voxels).sum() and s[7] == sizes[sizes < min_voxels].sum()
                assert s[8] == touching.size and s[9] == sizes[touching - 1].sum()
                assert s[10] == 3 and s[11] == 0
                assert np.array_equal(size_map, np.where(want > 0, np.concatenate([[0], sizes])[want], 0))
                # a non-finite value is in no set, hence in the complement
                assert bool(the_set[0, 0, 0]) == bool(the_set[4, 5, 6]) == bool(the_set[-1, -1, -1]) == complement
    assert cr.label_ref(cr.random_mask(shape, 0.3))[2][10] == 0          # a mask has no non-finite positions


@pytest.mark.parametrize("shape", [(9, 14, 17), (5, 6, 7), (3, 4, 70)])
def test_cavities_are_what_binary_fill_holes_fills(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    for density in (0.31, 0.6, 0.8, 0.95):
        m = cr.random_mask(shape, density) != 0
        bg = cr.label_ref(m.astype(np.uint8), connectivity=6, complement=True)[2]
        filled = ndi.binary_fill_holes(m, structure=_structure(ndi, 6))
        assert int(bg[1] - bg[9]) == int(filled.sum() - m.sum()), (shape, density)
        assert int(bg[2] - bg[8]) == ndi.label(filled & ~m, _structure(ndi, 6))[1]
    for shape_f in cr.SHAPES_FIXED:
        for pinhole, want in ((False, {6: 1, 18: 1, 26: 1}), (True, {6: 0, 18: 1, 26: 1})):      # by FOREGROUND connectivity
            box = cr.hollow_box(shape_f, pinhole)
            for fg_conn in cr.CONNECTIVITIES:
                bg = cr.label_ref(box, connectivity=cr.dual(fg_conn), complement=True)[2]
                assert int(bg[2] - bg[8]) == want[fg_conn], (shape_f, pinhole, fg_conn)
        inner = int(np.prod([n - 6 for n in shape_f]))
        assert int(np.subtract(*cr.label_ref(cr.hollow_box(shape_f), connectivity=6, complement=True)[2][[1, 9]])) == inner


@pytest.mark.parametrize("shape", cr.SHAPES_FIXED)
def test_fixed_layouts(shape):
    n = int(np.prod(shape))
    for c in cr.CONNECTIVITIES:
        for layout in (cr.serpentine(shape), cr.comb(shape)):
            labels, size_map, s = cr.label_ref(layout, connectivity=c)
            assert s[2] == 1 and s[3] == s[1] == layout.sum() and s[4] == 1 and np.array_equal(labels, layout)
        s = cr.label_ref(cr.checkerboard(shape), connectivity=c)[2]
        assert (s[2], s[3]) == (((n + 1) // 2, 1) if c == 6 else (1, (n + 1) // 2))
        for name, kind, a, b in cr.touching_pairs(shape):
            assert cr.label_ref(cr.pair_mask(shape, a, b), connectivity=c)[2][2] == cr.PAIR_COMPONENTS[kind][c], (name, c)
        labels, _, s = cr.label_ref(cr.last_voxel(shape), connectivity=c)
        assert s[2] == 3 and labels[-1, -1, -1] == 3 and labels[0, 0, 0] == 1 and s[4] == 1      # three singletons: the tie goes to label 1
    # the serpentine is a path: under 6-connectivity every voxel but the two ends has exactly two neighbours in the set
    m = np.pad(cr.serpentine(shape).astype(np.int64), 1)
    nb = (m[:-2, 1:-1, 1:-1] + m[2:, 1:-1, 1:-1] + m[1:-1, :-2, 1:-1] + m[1:-1, 2:, 1:-1] + m[1:-1, 1:-1, :-2] + m[1:-1, 1:-1, 2:])[m[1:-1, 1:-1, 1:-1] == 1]
    assert sorted(np.bincount(nb).tolist()) == [0, 2, nb.size - 2] and nb.size > n // 5


def test_segmentation_shape_arithmetic_from_two_summaries():
    from oai_analysis_2_amd import qc
    import dataclasses
    v = cr.planted()
    for connectivity, min_voxels in ((26, 0), (6, 2), (18, 10)):
        fg = cr.label_ref(v, 0.5, connectivity, False, min_voxels)[2]
        bg = cr.label_ref(v, 0.5, cr.dual(connectivity), True, 0)[2]
        lo, hi = int((v > np.float32(0.1)).sum()), int((v > np.float32(0.9)).sum())
        got = dataclasses.asdict(qc.shape_from_summaries(fg, bg, lo, hi, connectivity, min_voxels, 0.25))
        assert got == cr.shape_record(fg, bg, lo, hi, connectivity, min_voxels, 0.25)
        assert got["islands"] == got["components"] - 1 >= 2 and got["island_voxels"] == got["voxels"] - got["largest_voxels"] >= 2
        assert got["mm3"] == got["voxels"] * 0.25 and got["uncertain_voxels"] == lo - hi > 0
        assert got["cavities"] >= (1 if connectivity != 6 else 0) and got["cavity_voxels"] >= got["cavities"]
        assert got["small_components"] == (0 if min_voxels == 0 else int(fg[6])) and (min_voxels < 2 or got["small_components"] >= 2)
    assert qc.dual_connectivity(6) == 26 and qc.dual_connectivity(18) == 6 and qc.dual_connectivity(26) == 6
    with pytest.raises(ValueError):
        qc.dual_connectivity(8)
    zero = np.zeros(12, np.int64)
    empty = qc.shape_from_summaries(zero, zero, 0, 0, 26, 0)
    assert math.isnan(empty.largest_fraction) and empty.islands == 0 and empty.mm3 is None and empty.components == 0
    assert [f.name for f in dataclasses.fields(qc.SegmentationShape)] == list(cr.shape_record(zero, zero, 0, 0, 26, 0))


def test_planted_layout_is_what_it_says():
    v = cr.planted()
    base = cr.label_ref(v)[2]
    sizes = np.bincount(cr.label_ref(v)[0].ravel())[1:]
    assert (sizes == 1).sum() >= 2 and base[2] >= 3
    bg = cr.label_ref(v, connectivity=6, complement=True)[2]
    assert bg[2] - bg[8] >= 1 and bg[1] - bg[9] >= 1


def test_argument_checks_of_the_component_entry_points():
    """Bad arguments come back as a non-zero status with a message -- no GPU is touched before the checks."""
    from oai_analysis_2_amd import _lib
    lib = _lib.load()
    dummy = (C.c_float * 8)()
    big = 1 << 40
    err = lib.oai_last_error

    def call(map_=dummy, mask=None, dims=(2, 3, 4), thr=0.5, complement=0, connectivity=26, min_voxels=0, labels=dummy, sizes=dummy, ws=dummy,
             ws_bytes=big, summary=dummy):
        return lib.oai_label_components(map_, mask, *dims, thr, complement, connectivity, min_voxels, labels, sizes, ws, ws_bytes, summary, None)

    assert call(summary=None) != 0 and b"null" in err()
    assert call(ws=None) != 0 and b"null" in err()
    assert call(map_=None, mask=None) != 0 and b"exactly one" in err()
    assert call(map_=dummy, mask=dummy) != 0 and b"exactly one" in err()
    for bad in (8, 0, 4, 27, -6):
        assert call(connectivity=bad) != 0 and b"connectivity" in err()
        assert call(map_=None, mask=dummy, connectivity=bad) != 0 and b"connectivity" in err()
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (32768, 2, 2), (2, 32768, 2), (2, 2, 32768), (-1, 2, 2)):
        assert call(dims=dims) != 0 and b"every axis" in err()
        assert lib.oai_label_components_workspace_bytes(*dims) == 0
    for dims in ((32767, 32767, 3), (2048, 1024, 1024), (1291, 1290, 1290)):          # every axis fine, the product above 2^31 - 1
        assert np.prod(dims, dtype=np.int64) > 2 ** 31 - 1
        assert call(dims=dims) != 0 and b"2^31" in err()
        assert lib.oai_label_components_workspace_bytes(*dims) == 0
    assert lib.oai_label_components_workspace_bytes(2047, 1024, 1024) > 8 * 2047 * 1024 * 1024      # just below the limit
    assert lib.oai_label_components_workspace_bytes(32767, 1, 1) > 0
    need = lib.oai_label_components_workspace_bytes(2, 3, 4)
    assert need >= 8 * 24
    assert call(ws_bytes=need - 1) != 0 and b"oai_label_components: workspace" in err()
    assert call(ws_bytes=0) != 0 and b"workspace" in err()
    assert call(min_voxels=-1) != 0 and b"min_voxels" in err()
    assert call(thr=float("nan")) != 0 and b"NaN" in err()
    full = 160 * 384 * 384
    assert 8 * full < lib.oai_label_components_workspace_bytes(160, 384, 384) < 8.2 * full
    sizes = lambda labels, n, k, out: lib.oai_component_sizes(labels, n, k, out, None)
    assert sizes(None, 8, 2, dummy) != 0 and b"null" in err()
    assert sizes(dummy, 8, 2, None) != 0 and b"null" in err()
    assert sizes(dummy, -1, 2, dummy) != 0 and b"negative" in err()
    assert sizes(dummy, 8, -1, dummy) != 0 and b"negative" in err()
    assert sizes(dummy, 8, 1 << 31, dummy) != 0 and b"int32" in err()
    assert sizes(None, 0, 5, None) == 0 and sizes(None, 8, 0, None) == 0           # the documented no-ops
