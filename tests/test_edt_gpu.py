"""GPU: surface-distance QC (csrc/edt.hip; ops.mask_surface / distance_transform / signed_distance / surface_distance;
qc.surface_distance, segmentation_qc, QCReference(surface=True), registration_qc) -- the squared distances bit for bit against the
brute-force restatement of tests/edt_ref.py, the float32 distances to one step, the surfaces exactly, the figures on the device's own
maps (counts, maxima and percentiles exactly, sums within the summation bound), the sums bit for bit against the restated order of
csrc/ordered_reduce.h (tests/ordered_reduce_ref.py), and the record through every layer."""
import dataclasses
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import edt_ref as er
import ordered_reduce_ref as orr
import phi_jacobian_ref as pj
from oai_analysis_2_amd import _lib, ops
from oai_analysis_2_amd.image import Image

pytestmark = pytest.mark.gpu

# beyond edt_ref.SHAPES_SMALL: degenerate; unit axes; an axis longer than a block's threads and than any 256-entry slab, along x and
# along y; a line longer than the 64 KB slab of each staged pass (H > 512, D > 256: read from global memory); many blocks on every axis
SHAPES_BRUTE = er.SHAPES_SMALL + [(1, 1, 1), (1, 5, 7), (3, 4, 300), (5, 300, 4), (2, 520, 3), (260, 3, 2)]
LARGE = (40, 96, 96)
DENSITIES = (0.003, 0.05, 1.0, 0.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _want_sq(shape, density, spacing):
    f = er.sparse_features(shape, density, seed=17)
    return f, (er.edt_sq_lines if shape == LARGE else er.edt_sq_brute)(f, spacing)


def _one_step(got32, want32):
    """Float32 maps equal, or one float32 step apart; infinities and signs exactly.  Returns the number of voxels that differ."""
    got32, want32 = np.asarray(got32), np.asarray(want32)
    assert got32.dtype == want32.dtype == np.float32 and got32.shape == want32.shape
    inf = np.isinf(want32)
    assert np.array_equal(got32[inf], want32[inf]) and np.isfinite(got32[~inf]).all()
    assert np.array_equal(np.signbit(got32) & (got32 != 0), np.signbit(want32) & (want32 != 0)) and np.array_equal(got32 == 0, want32 == 0)
    steps = np.abs(np.abs(got32[~inf]).view(np.int32).astype(np.int64) - np.abs(want32[~inf]).view(np.int32).astype(np.int64))
    assert steps.max(initial=0) <= 1
    return int((steps != 0).sum())


def _check_edt(f, spacing, want_sq, label):
    dist, sq, n = ops.distance_transform(dev(f), spacing, return_squared=True, return_count=True)
    assert dist.dtype == torch.float32 and sq.dtype == torch.float64 and n.dtype == torch.int64 and tuple(dist.shape) == f.shape
    sq, d = sq.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(sq.view(np.int64), want_sq.view(np.int64)), label                # +inf where the restatement has it
    differ = _one_step(d, er.edt_dist32(want_sq))
    print(label, "features", int(n.item()), "float32 distances that differ from float32(sqrt(sq))", differ, "(expected 0)")
    assert int(n.item()) == int((f != 0).sum())
    assert np.array_equal(ops.distance_transform(dev(f), spacing).cpu().numpy().view(np.int32), d.view(np.int32))      # without sq_out_dev


@pytest.mark.parametrize("spacing", er.SPACINGS)
@pytest.mark.parametrize("shape", SHAPES_BRUTE + [LARGE])
def test_squared_distances_are_the_brute_force_minimum_bit_for_bit(shape, spacing):
    for density in DENSITIES:
        f, want = _want_sq(shape, density, spacing)
        _check_edt(f, spacing, want, (shape, spacing, density))
    if shape == (1, 1, 1):
        assert _want_sq(shape, 1.0, spacing)[1][0, 0, 0] == 0.0 and np.isposinf(_want_sq(shape, 0.0, spacing)[1][0, 0, 0])


@pytest.mark.parametrize("spacing", er.SPACINGS)
def test_fixed_feature_layouts(spacing):
    shape = (9, 14, 17)
    corner = np.zeros(shape, np.uint8)
    corner[-1, -1, -1] = 1                                               # every scan runs to the far end of its line
    face = np.zeros(shape, np.uint8)
    face[:, :, 0] = er.sparse_features((9, 14), 0.3, 2)                  # features on one face only
    gaps = er.sparse_features(shape, 0.2, 3)
    gaps[[1, 2, 7]] = 0                                                  # whole slices ...
    gaps[:, [0, 5, 6, 13]] = 0                                           # ... and whole rows without any feature
    long_x = np.zeros((3, 4, 300), np.uint8)
    long_x[1, 2, 299] = long_x[0, 0, 64] = 1
    for name, f in (("corner", corner), ("face", face), ("gaps", gaps), ("long x", long_x)):
        _check_edt(f, spacing, er.edt_sq_brute(f, spacing), (name, spacing))


def _planted(shape, seed):
    m = er.blobs(shape, seed, roll=(shape[0] // 3, shape[1] // 2, shape[2] // 4))
    flat = m.reshape(-1)
    where = np.random.default_rng(seed).choice(flat.size, size=min(flat.size, 9), replace=False)
    flat[where] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), where.size)
    return m


@pytest.mark.parametrize("shape", SHAPES_BRUTE + [LARGE])
def test_mask_surface_equals_the_restatement(shape):
    m = _planted(shape, 21)
    for thr in (0.5, 0.25):
        for name, mode in ops.SURFACE_MODES.items():
            got = ops.mask_surface(dev(m), thr, name)
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), er.surface_ref(m, thr, mode)), (name, thr)


@pytest.mark.parametrize("spacing", er.SPACINGS)
@pytest.mark.parametrize("shape", [(12, 20, 24), (3, 4, 300), (1, 1, 1)])
def test_signed_distance_is_the_difference_of_the_two_restated_maps(shape, spacing):
    for m in (_planted(shape, 22), np.zeros(shape, np.float32), np.ones(shape, np.float32)):
        s = er.in_set(m)
        with np.errstate(invalid="ignore"):
            want = er.edt_dist32(er.edt_sq_brute(s, spacing)) - er.edt_dist32(er.edt_sq_brute(~s, spacing))
        got = ops.signed_distance(dev(m), spacing).cpu().numpy()
        print(shape, spacing, "inside", int(s.sum()), "differ", _one_step(got, want))
        if s.any() and not s.all():
            assert (got[s] < 0).all() and (got[~s] > 0).all()


# ---- oai_surface_distance ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair(shape, spacing):
    """Two rolled blobs and, from the device, their surfaces and the distance maps to them (device tensors and host copies)."""
    a, b = er.blobs(shape, 31, roll=(1, 2, 3)), er.blobs(shape, 31, roll=(2, 4, 1))
    sa, sb = ops.mask_surface(dev(a), 0.5, "surface"), ops.mask_surface(dev(b), 0.5, "surface")
    to_a, to_b = ops.distance_transform(sa, spacing), ops.distance_transform(sb, spacing)
    return (sa, to_b, sb, to_a), tuple(t.cpu().numpy() for t in (sa, to_b, sb, to_a))


def _check_figures(dev4, host4, percentiles, label=""):
    want = er.surface_distance_ref(*host4, percentiles)
    got = ops.surface_distance(*dev4, percentiles)
    assert got.dtype == torch.float64 and got.shape == (8,) and got.is_cuda
    s = got.cpu().numpy()
    assert (s[0], s[1]) == (want["n_a"], want["n_b"])
    if want["n_a"] == 0 or want["n_b"] == 0:
        assert np.isnan(s[2:]).all()
        return s
    assert (s[4], s[5]) == (want["max_ab"], want["max_ba"])
    for k, name, n in ((2, "sum_ab", want["n_a"]), (3, "sum_ba", want["n_b"])):       # non-negative terms: sum |d| is the sum
        print(label, name, s[k], "error", s[k] - want[name], "bound", n * 2.0 ** -52 * want[name])
        assert abs(s[k] - want[name]) <= n * 2.0 ** -52 * want[name]
    for i, q in enumerate(percentiles):
        assert np.float32(s[6 + i]) == s[6 + i] and np.float32(s[6 + i]).view(np.int32) == np.float32(want["percentiles"][i]).view(np.int32), q
    assert np.isnan(s[6 + len(percentiles):]).all()
    return s


@pytest.mark.parametrize("spacing", er.SPACINGS)
@pytest.mark.parametrize("shape", [(12, 20, 24), LARGE])
def test_surface_distance_figures_on_the_devices_own_maps(shape, spacing):
    dev4, host4 = _pair(shape, spacing)
    assert host4[0].sum() > 0 and host4[2].sum() > 0
    for pair in itertools.combinations((0.0, 50.0, 95.0, 100.0), 2):
        _check_figures(dev4, host4, pair, (shape, spacing, pair))
    one = _check_figures(dev4, host4, (95.0,))
    none = _check_figures(dev4, host4, ())
    again = ops.surface_distance(*dev4, (95.0,)).cpu().numpy()                          # no atomics in the sums: the same bits
    assert np.array_equal(one.view(np.int64), again.view(np.int64)) and np.array_equal(one[:6], none[:6])
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    assert ops.surface_distance(*dev4, (95.0,), out=out) is out and np.array_equal(out.cpu().numpy().view(np.int64), one.view(np.int64))


@pytest.mark.parametrize("n", orr.ORDER_SIZES)
def test_sums_follow_the_restated_order_bit_for_bit(n):
    """The summation order is the contract (csrc/ordered_reduce.h): on terms spread over 17 decades, where any other order gives
    other bits (tests/test_edt_cpu.py asserts that the restated sum is not the serial one), the device equals the restatement."""
    host4, want, terms, exact, _ = orr.order_case(n)
    dev4 = tuple(dev(a) for a in host4)
    s = ops.surface_distance(*dev4, ()).cpu().numpy()
    print(n, "device", [float(v).hex() for v in s[:6]], "restated", [float(v).hex() for v in want])
    assert (s[0], s[1]) == (want[0], want[1]) == (terms[0].size, terms[1].size)
    assert (s[4], s[5]) == (want[4], want[5]) == (terms[0].max(), terms[1].max())
    assert np.array_equal(s[2:4].view(np.int64), want[2:4].view(np.int64))
    for k in (0, 1):
        assert abs(s[2 + k] - exact[k]) <= terms[k].size * 2.0 ** -52 * exact[k]
    assert np.isnan(s[6:]).all()
    again = ops.surface_distance(*dev4, (50.0,)).cpu().numpy()                          # the same bits with the select behind it
    assert np.array_equal(again[:6].view(np.int64), s[:6].view(np.int64))
    assert np.float32(again[6]).view(np.int32) == np.percentile(np.concatenate([t.astype(np.float32) for t in terms]), 50.0).view(np.int32)


def test_surface_distance_with_empty_surfaces():
    (sa, to_b, sb, to_a), _ = _pair((12, 20, 24), er.SPACINGS[1])
    zero = torch.zeros_like(sa)
    inf = ops.distance_transform(zero, er.SPACINGS[1])
    assert torch.isinf(inf).all()
    for d4 in ((zero, to_b, sb, inf), (sa, inf, zero, to_a), (zero, inf, zero, inf)):
        s = _check_figures(d4, tuple(t.cpu().numpy() for t in d4), (50.0, 95.0))
        assert np.isnan(s[2:]).all() and s[0] == int(d4[0].sum()) and s[1] == int(d4[2].sum())
    e = torch.empty(0, dtype=torch.uint8, device="cuda")
    s = ops.surface_distance(e, e.float(), e, e.float()).cpu().numpy()
    assert s[0] == 0 and s[1] == 0 and np.isnan(s[2:]).all()


def test_analytic_cases_on_the_device():
    from oai_analysis_2_amd.qc import surface_distance
    shape = (12, 20, 24)
    for sp in er.SPACINGS:
        sx, sy, sz = sp
        one, other = er.box(shape, (2, 3, 4), (1, 1, 1)), er.box(shape, (7, 15, 20), (1, 1, 1))
        tx, ty, tz = 16.0 * np.float64(sx), 12.0 * np.float64(sy), 5.0 * np.float64(sz)
        d = float(np.float32(np.sqrt((tx * tx + ty * ty) + tz * tz)))
        r = surface_distance(one, other, sp, percentiles=(0.0, 95.0))
        assert (r.n_a, r.n_b) == (1, 1) and abs(r.hausdorff - d) <= float(np.spacing(np.float32(d)))
        assert r.mean_ab == r.mean_ba == r.assd == r.hausdorff == r.percentiles[0.0] == r.hd95
        b6 = er.box(shape, (3, 4, 5), (6, 11, 9))
        r = surface_distance(b6, np.roll(b6, 3, axis=2), sp)
        assert r.n_a == r.n_b == 342 and r.hausdorff == float(np.float32(3 * np.float64(sx)))
        r = surface_distance(b6, b6, sp)
        assert (r.mean_ab, r.mean_ba, r.assd, r.hausdorff, r.hd95) == (0.0,) * 5
        r = surface_distance(b6, np.zeros(shape, np.float32), sp)
        assert (r.n_a, r.n_b) == (342, 0) and all(math.isnan(v) for v in (r.mean_ab, r.mean_ba, r.assd, r.hausdorff, r.hd95))


# ---- the layers ----------------------------------------------------------------------------------------------------------------------
def _same(x, y) -> bool:
    """Two records, field for field (a NaN equals a NaN)."""
    if dataclasses.is_dataclass(x):
        return type(x) is type(y) and all(_same(getattr(x, f.name), getattr(y, f.name)) for f in dataclasses.fields(x))
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(_same(x[k], y[k]) for k in x)
    if isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y):
        return True
    return type(x) is type(y) and x == y


def test_qc_surface_distance_on_images_equals_the_ops_chain():
    from oai_analysis_2_amd.qc import SurfaceDistance, segmentation_qc, surface_distance
    shape, sp = (12, 20, 24), (0.3, 0.7, 1.1)
    a, b = er.blobs(shape, 41, roll=(1, 2, 3)), er.blobs(shape, 41, roll=(2, 3, 5))
    r = surface_distance(Image(a, sp), Image(b, sp), percentiles=(50.0, 95.0))
    sa, sb = ops.mask_surface(dev(a), 0.5, "surface"), ops.mask_surface(dev(b), 0.5, "surface")
    s = ops.surface_distance(sa, ops.distance_transform(sb, sp), sb, ops.distance_transform(sa, sp), (50.0, 95.0)).cpu().tolist()
    want = SurfaceDistance(int(s[0]), int(s[1]), s[2] / s[0], s[3] / s[1], (s[2] + s[3]) / (s[0] + s[1]), max(s[4], s[5]), {50.0: s[6], 95.0: s[7]})
    assert _same(r, want) and r.hd95 == s[7] and r.n_a > 0 and r.assd > 0
    assert _same(surface_distance(dev(a), b, sp, percentiles=(50.0, 95.0)), r)              # a tensor and an array with the spacing
    assert surface_distance(a, b).assd != r.assd                                            # unit spacing otherwise
    with pytest.raises(ValueError, match="spacing"):
        surface_distance(Image(a, sp), Image(b, (0.3, 0.7, 1.0)))
    with pytest.raises(ValueError, match="grid"):
        surface_distance(a, b[1:], sp)
    seg = segmentation_qc(Image(a, sp), Image(a, sp))
    n = int((a > 0.5).sum())
    assert seg.dice == 1.0 and seg.counts == (n, n, n, 0) and seg.surface.assd == 0.0 and seg.surface.hausdorff == 0.0
    seg = segmentation_qc(a, b, sp)
    assert 0.0 < seg.dice < 1.0 and _same(seg.surface, surface_distance(a, b, sp))


def _meta(shape_zyx, spacing):
    return Image(np.broadcast_to(np.zeros((), np.float32), shape_zyx), spacing)


def test_registration_qc_surface_part():
    """tests/test_registration_qc_gpu.py::test_dice_and_cartilage_volume's synthetic VolumeResult, on a grid large enough for blobs."""
    from oai_analysis_2_amd.pipeline import VolumeResult
    from oai_analysis_2_amd.qc import QCReference, registration_qc, surface_distance
    shape, sp = (12, 20, 24), [0.4, 0.35, 0.75]
    fc, tc = er.blobs(shape, 51, roll=(1, 2, 3)), er.blobs(shape, 52, roll=(4, 1, 2))
    atlas_fc, atlas_tc = er.blobs(shape, 51, roll=(2, 3, 5)), er.blobs(shape, 52, roll=(4, 2, 2))
    phi = dev(pj.drawn_phi((3, 4, 5), 0.45))
    patient = np.random.default_rng(5).uniform(0, 1, size=(4, 8, 9)).astype(np.float32)
    res = VolumeResult(dev(patient), dev(np.zeros((4, 8, 9), np.float32)), phi, dev(fc), dev(tc), meta_A=_meta((4, 8, 9), [0.36, 0.37, 0.7]),
                       meta_B=_meta(shape, sp))
    reference = QCReference(Image(atlas_fc, sp), Image(atlas_tc, sp), surface=True)
    held = {k: (reference.surfaces[k], reference.distance_maps[k]) for k in ("FC", "TC")}
    qc = registration_qc(res, reference=reference)
    again = registration_qc(res, reference=reference)
    for k in ("FC", "TC"):                                                                 # the atlas maps are computed once
        assert reference.surfaces[k] is held[k][0] and reference.distance_maps[k] is held[k][1]
    assert _same(qc, again) and set(qc.surface) == {"FC", "TC"}
    assert _same(qc.surface["FC"], surface_distance(res.fc_atlas, atlas_fc, sp)) and qc.surface["FC"].assd > 0
    assert _same(qc.surface["TC"], surface_distance(res.tc_atlas, Image(atlas_tc, sp), sp))
    via_tensors = QCReference(dev(atlas_fc), dev(atlas_tc), surface=True, spacing_xyz=sp)
    assert _same(registration_qc(res, reference=via_tensors), qc)
    with pytest.raises(ValueError, match="spacing"):
        QCReference(dev(atlas_fc), dev(atlas_tc), surface=True)
    # with the option off the record is today's: the same fields, and nothing under .surface
    plain = QCReference(Image(atlas_fc, sp), Image(atlas_tc, sp))
    off = registration_qc(res, reference=plain)
    assert plain.surfaces is None and off.surface is None and registration_qc(res).surface is None
    today = ("jacobian", "volume_scale", "dice", "overlap_counts", "cartilage_voxels", "cartilage_mm3")
    a, b = dataclasses.asdict(off), dataclasses.asdict(qc)
    assert tuple(a) == today + ("surface",) and all(_same(a[k], b[k]) for k in today)
    assert _same(dataclasses.asdict(registration_qc(res, reference=QCReference(Image(atlas_fc, sp), Image(atlas_tc, sp), surface=False))), a)


def test_pipeline_run_with_a_surface_reference():
    """tests/test_registration_qc_gpu.py::_small_pipe: the record flows through VolumePipeline.run(qc=) and qc_stream unchanged."""
    from oai_analysis_2_amd.dask_processing import qc_stream
    from oai_analysis_2_amd.pipeline import VolumePipeline
    from oai_analysis_2_amd.qc import QCReference, registration_qc
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
    base = pipe.run(v, meta)
    reference = QCReference(Image(base.fc_atlas.cpu().numpy(), atlas.spacing), Image(base.tc_atlas.cpu().numpy(), atlas.spacing), surface=True)
    on = pipe.run(v, meta, qc=reference)
    for name in ("fc", "tc", "phi", "fc_atlas", "tc_atlas"):
        assert torch.equal(getattr(on, name), getattr(base, name)), name
    assert _same(on.qc, registration_qc(on, reference=reference)) and _same(list(qc_stream([(4, on)], reference))[0][1], on.qc)
    for kind in ("FC", "TC"):                                                              # against its own warped maps: zero, or empty
        s = on.qc.surface[kind]
        assert s.n_a == s.n_b and (s.assd == 0.0 and s.hausdorff == 0.0 if s.n_a else math.isnan(s.assd))
    assert pipe.run(v, meta, qc=True).qc.surface is None


def test_bad_arguments_raise_and_do_not_fault():
    bad = (_lib.OaiError, ValueError)
    f = torch.zeros((3, 4, 5), dtype=torch.uint8, device="cuda")
    m = torch.zeros((3, 4, 5), device="cuda")
    for call in (lambda: ops.mask_surface(m, 0.5, "edge"), lambda: ops.mask_surface(m[0]), lambda: ops.mask_surface(f), lambda: ops.mask_surface(m.cpu()),
                 lambda: ops.distance_transform(m), lambda: ops.distance_transform(f[0]), lambda: ops.distance_transform(f, (1.0, 0.0, 1.0)),
                 lambda: ops.distance_transform(f, (1.0, float("nan"), 1.0)), lambda: ops.distance_transform(f.cpu()),
                 lambda: ops.surface_distance(f, m, f, m, (95.0, 50.0, 5.0)), lambda: ops.surface_distance(f, m, f, m, (101.0,)),
                 lambda: ops.surface_distance(f, m, f[1:], m), lambda: ops.surface_distance(m, m, f, m),
                 lambda: ops.surface_distance(f, m, f, m, out=torch.zeros(7, dtype=torch.float64, device="cuda"))):
        with pytest.raises(bad):
            call()
    f[1, 2, 3] = 1                                                                         # and the device is fine afterwards
    assert ops.distance_transform(f)[1, 2, 0].item() == 3.0
