"""GPU: csrc/components.hip through ops.label_components / ops.component_sizes, qc.segmentation_shape, qc.clean_segmentation,
VolumePipeline.run(seg_qc=True) and dask_processing.seg_qc_stream, against the numpy restatement of tests/components_ref.py (which
tests/test_components_cpu.py holds to scipy.ndimage.label to the element).  Everything is integers: every comparison is exact.

The shapes are written in terms of the kernel's brick of 4 x 4 x 64 voxels (components_ref.BRICK): one voxel, less than a brick, a
brick edge + 1 on every axis, a row longer than a block's threads, and volumes of many bricks."""
import dataclasses

import numpy as np
import pytest
import torch

import components_ref as cr
from oai_analysis_2_amd import ops, qc
from oai_analysis_2_amd.image import Image

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(vol, **kw):
    """(labels, sizes, summary) on the host of one ops.label_components with both maps."""
    summary, labels, sizes = ops.label_components(vol, return_labels=True, return_sizes=True, **kw)
    return labels.cpu().numpy(), sizes.cpu().numpy(), summary.cpu().numpy()


def check(vol_np, connectivity, complement=False, min_voxels=0, threshold=0.5, also=None, what=""):
    """One input against the restatement: labels and sizes to the element, the summary, and the summary again without the maps.
    ``also``: a second tensor with the same set (the byte mask beside the map) that must give the same."""
    want_l, want_s, want = cr.label_ref(vol_np, threshold, connectivity, complement, min_voxels)
    kw = dict(threshold=threshold, connectivity=connectivity, complement=complement, min_voxels=min_voxels)
    vol = dev(vol_np)
    labels, sizes, summary = run(vol, **kw)
    print(what, vol_np.shape, "connectivity", connectivity, "complement", complement, "summary", summary.tolist(), "want", want.tolist())
    assert labels.dtype == np.int32 and np.array_equal(labels, want_l), what
    assert np.array_equal(sizes, want_s) and np.array_equal(summary, want), what
    bare, none_l, none_s = ops.label_components(vol, return_labels=False, return_sizes=False, **kw)
    assert none_l is None and none_s is None and np.array_equal(bare.cpu().numpy(), want), what
    if also is not None:
        l2, s2, sum2 = run(dev(also), **kw)
        want2 = want.copy()
        want2[10] = 0                                                      # a mask has no non-finite positions
        assert np.array_equal(l2, want_l) and np.array_equal(s2, want_s) and np.array_equal(sum2, want2), what
    return want_l, want


# ---- 1. labels to the element ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", cr.CONNECTIVITIES)
@pytest.mark.parametrize("shape", cr.SHAPES_GPU)
def test_labels_to_the_element(shape, connectivity):
    for density in cr.DENSITIES:
        mask = cr.random_mask(shape, density)
        as_map = cr.as_map(mask)
        assert np.array_equal(cr.the_set(as_map), mask != 0)
        for complement in (False, True):
            check(as_map, connectivity, complement, also=mask, what=f"density {density}")
    b = torch.from_numpy(cr.random_mask(shape, 0.31) != 0).cuda()             # a bool tensor is a mask
    assert torch.equal(ops.label_components(b, connectivity=connectivity)[1], ops.label_components(b.to(torch.uint8), connectivity=connectivity)[1])


def test_scipy_as_a_second_witness():
    ndi = pytest.importorskip("scipy.ndimage")
    mask = cr.random_mask((17, 33, 65), 0.1)
    for connectivity, rank in ((6, 1), (18, 2), (26, 3)):
        want, k = ndi.label(mask, ndi.generate_binary_structure(3, rank))
        summary, labels, _ = ops.label_components(dev(mask), connectivity=connectivity)
        assert np.array_equal(labels.cpu().numpy(), want) and int(summary[2]) == k


# ---- 2. fixed layouts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cr.SHAPES_FIXED)
def test_fixed_layouts(shape):
    n = int(np.prod(shape))
    for c in cr.CONNECTIVITIES:
        for name, layout in (("serpentine", cr.serpentine(shape)), ("comb", cr.comb(shape))):
            _, s = check(layout, c, what=name)
            assert s[2] == 1 and s[3] == layout.sum()
        _, s = check(cr.checkerboard(shape), c, what="checkerboard")
        assert (s[2], s[3]) == (((n + 1) // 2, 1) if c == 6 else (1, (n + 1) // 2))
        for name, kind, a, b in cr.touching_pairs(shape):
            _, s = check(cr.pair_mask(shape, a, b), c, what=name)
            assert s[2] == cr.PAIR_COMPONENTS[kind][c], (name, c)
        labels, s = check(cr.last_voxel(shape), c, what="last voxel")
        assert s[2] == 3 and labels[-1, -1, -1] == 3
        for pinhole in (False, True):
            check(cr.hollow_box(shape, pinhole), c, what="hollow box")
            check(cr.hollow_box(shape, pinhole), c, complement=True, what="hollow box, complement")
    # a closed box has one cavity; the corner-only pinhole opens it for a 26-connected background (foreground 6) and for no other
    for pinhole, want in ((False, {6: 1, 18: 1, 26: 1}), (True, {6: 0, 18: 1, 26: 1})):
        m = cr.as_map(cr.hollow_box(shape, pinhole))
        for c in cr.CONNECTIVITIES:
            rec = qc.segmentation_shape(dev(m), connectivity=c)
            assert rec.cavities == want[c] and rec.components == 1, (pinhole, c)
            assert rec.cavity_voxels == (int(np.prod([v - 6 for v in shape])) if want[c] else 0)


# ---- 3. numbering and sizes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", cr.CONNECTIVITIES)
def test_numbering_sizes_ties_and_min_voxels(connectivity):
    shape = (17, 33, 65)
    mask = cr.random_mask(shape, 0.1)
    want_l, want_size, want = cr.label_ref(mask, connectivity=connectivity)
    K = int(want[2])
    table = np.bincount(want_l.ravel())[1:]
    summary, labels, sizes = ops.label_components(dev(mask), connectivity=connectivity, return_sizes=True)
    got = ops.component_sizes(labels, K).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, table) and K > 10
    assert np.array_equal(sizes.cpu().numpy(), np.where(want_l > 0, np.concatenate([[0], table])[want_l], 0))
    assert np.array_equal(ops.component_sizes(labels, K - 3).cpu().numpy(), table[:K - 3])          # labels above the table are ignored
    wild = labels.clone()
    wild[0, 0, :4] = torch.tensor([-5, K + 1, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    first = np.bincount(want_l[0, 0, :4], minlength=K + 1)[1:]
    assert np.array_equal(ops.component_sizes(wild, K).cpu().numpy(), table - first)
    assert ops.component_sizes(labels, 0).numel() == 0 and not ops.component_sizes(labels[:0], 4).cpu().numpy().any()
    for min_voxels in (0, 1, 2, int(want[3]) + 1):
        _, s = check(mask, connectivity, min_voxels=min_voxels, what=f"min_voxels {min_voxels}")
        assert s[6] == (table < min_voxels).sum() and (min_voxels <= want[3] or (s[6], s[7]) == (K, want[1]))
    # ties for the largest: two equal boxes and a smaller one in between -- the smaller label wins, the second largest equals the largest
    tie = np.zeros(shape, np.uint8)
    tie[10:13, 20:23, 60:65] = 1          # across the x brick face; first in raster order
    tie[11, 28, 1] = 1
    tie[13:16, 1:4, 2:7] = 1
    labels_t, s = check(tie, connectivity, what="tie")
    assert s[2] == 3 and s[3] == s[5] == 45 and s[4] == 1 == labels_t[10, 20, 60] and labels_t[13, 1, 2] == 3


# ---- 4. non-finite values ----------------------------------------------------------------------------------------------------------------
def test_nonfinite_values_are_in_no_set_and_in_the_complement():
    shape = (9, 14, 17)
    v = cr.as_map(cr.random_mask(shape, 0.31))
    rng = np.random.default_rng(2)
    at = rng.choice(v.size, 30, replace=False)
    v.ravel()[at] = np.tile(np.array([np.nan, np.inf, -np.inf], np.float32), 10)
    for c in cr.CONNECTIVITIES:
        for complement in (False, True):
            labels, s = check(v, c, complement, what="non-finite")
            assert s[10] == 30 and bool((labels.ravel()[at] > 0).all()) == complement and bool((labels.ravel()[at] == 0).all()) != complement
    allbad = np.full(shape, np.nan, np.float32)
    assert check(allbad, 26)[1][[1, 2, 10]].tolist() == [0, 0, v.size] and check(allbad, 6, True)[1][[1, 2]].tolist() == [v.size, 1]
    for thr in (-np.inf, np.inf, 0.0, 0.75):                                # +-inf are thresholds like any other
        check(v, 26, threshold=float(thr), what=f"threshold {thr}")


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------------
def test_five_runs_on_two_streams_are_bit_identical():
    shape = (40, 96, 96)
    vol = dev(cr.as_map(cr.random_mask(shape, 0.31)))
    first = None
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got = []
    for i in range(5):
        with torch.cuda.stream(streams[i % 2]):
            got.append(ops.label_components(vol, connectivity=6, min_voxels=3, return_sizes=True))
    torch.cuda.synchronize()
    for summary, labels, sizes in got:
        if first is None:
            first = (summary, labels, sizes)
        assert torch.equal(summary, first[0]) and torch.equal(labels, first[1]) and torch.equal(sizes, first[2])
    assert int(first[0][2]) > 100


# ---- 6. through the layers ---------------------------------------------------------------------------------------------------------------
def _want_record(v, connectivity, min_voxels, band, voxel_mm3, threshold=0.5):
    fg = cr.label_ref(v, threshold, connectivity, False, min_voxels)[2]
    bg = cr.label_ref(v, threshold, cr.dual(connectivity), True, 0)[2]
    return cr.shape_record(fg, bg, cr.the_set(v, band[0]).sum(), cr.the_set(v, band[1]).sum(), connectivity, min_voxels, voxel_mm3)


def test_segmentation_shape_on_planted_blobs():
    v = cr.planted()
    spacing = (0.36, 0.37, 0.7)
    for connectivity, min_voxels, band in ((26, 0, (0.1, 0.9)), (6, 2, (0.2, 0.6)), (18, 50, (0.1, 0.9))):
        want = _want_record(v, connectivity, min_voxels, band, float(np.prod(np.float64(spacing))))
        for form in (Image(v, spacing), dev(v)):
            got = dataclasses.asdict(qc.segmentation_shape(form, spacing_xyz=None if isinstance(form, Image) else spacing,
                                                           connectivity=connectivity, min_voxels=min_voxels, band=band))
            print(connectivity, got)
            assert got == want
        assert want["islands"] >= 2 and want["cavities"] >= (0 if connectivity == 6 else 1) and want["uncertain_voxels"] > 0
    bare = qc.segmentation_shape(v)                                         # an array without a spacing: no volume
    assert bare.mm3 is None and bare.voxels == _want_record(v, 26, 0, (0.1, 0.9), None)["voxels"]
    with pytest.raises(ValueError):
        qc.segmentation_shape(dev(v), connectivity=8)


def test_clean_segmentation_in_both_modes():
    v = cr.planted()
    for connectivity in (26, 6):
        labels, sizes, s = cr.label_ref(v, connectivity=connectivity)
        largest = qc.clean_segmentation(dev(v), connectivity=connectivity)
        assert largest.dtype == torch.float32 and np.array_equal(largest.cpu().numpy(), np.where((labels > 0) & (labels != s[4]), np.float32(0), v))
        for min_voxels in (0, 2, 30, int(s[3]) + 1):
            kept = qc.clean_segmentation(dev(v), keep_largest=False, min_voxels=min_voxels, connectivity=connectivity)
            assert np.array_equal(kept.cpu().numpy(), np.where((sizes > 0) & (sizes < min_voxels), np.float32(0), v)), min_voxels
    tie = np.zeros((9, 14, 17), np.float32)
    tie[1:3, 1:3, 1:3] = tie[5:7, 5:7, 5:7] = 0.8                           # two components of eight: exactly the first one stays
    tie[4, 0, 0] = 0.3                                                      # off the set: left as it is
    want = tie.copy()
    want[5:7, 5:7, 5:7] = 0
    assert np.array_equal(qc.clean_segmentation(tie).cpu().numpy(), want)
    assert np.array_equal(qc.clean_segmentation(Image(tie, (1, 1, 1)), keep_largest=False, min_voxels=8).cpu().numpy(), tie)


def _same_records(a, b):
    return set(a) == set(b) == {"FC", "TC"} and all(dataclasses.asdict(a[k]) == dataclasses.asdict(b[k]) for k in a)


def test_pipeline_run_with_seg_qc_changes_no_bit():
    """tests/test_registration_qc_gpu.py::_small_pipe, the smallest pipeline the QC tests use."""
    from oai_analysis_2_amd.dask_processing import seg_qc_stream
    from oai_analysis_2_amd.pipeline import VolumePipeline, VolumeResult
    from oai_analysis_2_amd.registration import IconEngine
    from oai_analysis_2_amd.segmentation.engine import UNetEngine
    from oai_analysis_2_amd.synth import make_icon_state_dict, make_unet_state_dict, make_volume
    shape, net = (24, 72, 72), (40, 48, 48)
    atlas = Image(make_volume(10, shape), [0.4, 0.35, 0.75], [0.0, -1.0, 2.0])
    pipe = VolumePipeline(UNetEngine(make_unet_state_dict(1, width_div=2), precision="fp16x3"),
                          IconEngine(make_icon_state_dict(1, last_scale=0.1), net_shape=net), atlas,
                          tile_zyx=(16, 32, 32), overlap_zyx=(4, 8, 8), crop_zyx=(4, 8, 8), batch=8)
    vol = make_volume(9, shape)
    meta = Image(vol, [0.36, 0.37, 0.7], [1.0, 2.0, 3.0])
    v = dev(vol)
    base, on = pipe.run(v, meta, qc=True), pipe.run(v, meta, qc=True, seg_qc=True)
    for name in ("fc", "tc", "phi", "fc_atlas", "tc_atlas"):
        assert torch.equal(getattr(on, name), getattr(base, name)), name
    assert dataclasses.asdict(on.qc) == dataclasses.asdict(base.qc) or repr(on.qc) == repr(base.qc)
    assert base.seg_qc is None and VolumeResult.seg_qc is None and "seg_qc" not in [f.name for f in dataclasses.fields(VolumeResult)]
    alone = {kind: qc.segmentation_shape(getattr(on, kind.lower()), spacing_xyz=meta.spacing) for kind in ("FC", "TC")}
    assert _same_records(on.seg_qc, alone)
    for kind in ("FC", "TC"):                                               # ... and the restatement on the downloaded map
        m = getattr(on, kind.lower()).cpu().numpy()
        assert dataclasses.asdict(on.seg_qc[kind]) == _want_record(m, 26, 0, (0.1, 0.9), float(np.prod(np.float64(meta.spacing))))
        assert on.seg_qc[kind].voxels == on.qc.cartilage_voxels[kind]
    out = list(seg_qc_stream(iter([(7, on), (3, base)])))
    assert [i for i, _ in out] == [7, 3] and all(_same_records(rec, on.seg_qc) for _, rec in out)
