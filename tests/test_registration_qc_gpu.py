"""GPU: registration QC (csrc/phi_jacobian.hip, ops.phi_jacobian / ops.mask_overlap, qc.registration_qc, VolumePipeline.run(qc=),
dask_processing.qc_stream) -- the determinant map against the fp64 restatement of tests/phi_jacobian_ref.py to one float32 ulp, the
statistics within their summation bounds, the overlap counts against numpy exactly, and the record through every layer."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import mesh_transform_ref as ref
import phi_jacobian_ref as pj
from oai_analysis_2_amd import _lib, ops
from oai_analysis_2_amd.image import Image
from oai_analysis_2_amd.synth import make_icon_state_dict, make_unet_state_dict, make_volume

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 2), (3, 4, 5), (6, 7, 9), (9, 33, 70)]      # one cell; odd tails; x > 64 lanes, more than one block on every axis
PRODUCTION = (80, 192, 192)                                   # 1440 blocks: the multi-block partials and the finishing kernel's runs


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


def _ulp32(x: float) -> float:
    return float(np.abs(np.spacing(np.float32(x))))


def _check_against_restatement(phi: np.ndarray, det: np.ndarray, label):
    """ops.phi_jacobian on ``phi`` against ``det`` = det_ref(phi).  Returns the float64 [7] stats on the host."""
    want = pj.stats_ref(det)
    stats, got = ops.phi_jacobian(torch.from_numpy(phi).cuda(), return_map=True)
    assert stats.dtype == torch.float64 and stats.shape == (7,) and stats.is_cuda
    assert got.dtype == torch.float32 and tuple(got.shape) == det.shape
    got, s = got.cpu().numpy(), stats.cpu().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        w32 = det.astype(np.float32)
    ok = np.isfinite(det)
    assert np.array_equal(np.isnan(got), np.isnan(w32)) and np.array_equal(got[np.isinf(w32)], w32[np.isinf(w32)])
    err = np.abs(got[ok].astype(np.float64) - w32[ok].astype(np.float64))
    ulp = np.abs(np.spacing(w32[ok])).astype(np.float64)
    print(label, "cells", want["cells"], "folds", want["folds"], "non-finite", want["nonfinite"], "max error in ulps",
          float((err / ulp).max()) if err.size else 0.0, "not bitwise", int((_bits(got)[ok] != _bits(w32)[ok]).sum()),
          "sum error", float(s[5]) - want["sum"], "sum of squares error", float(s[6]) - want["sum_sq"])
    assert (err <= ulp).all()
    assert (int(s[0]), int(s[1]), int(s[2])) == (want["cells"], want["folds"], want["nonfinite"]) and s[0] == want["cells"]
    if want["n_finite"]:
        for k, name in ((3, "min"), (4, "max")):
            assert abs(float(np.float32(s[k])) - float(np.float32(want[name]))) <= _ulp32(want[name]), name
        n = want["n_finite"]
        assert abs(float(s[5]) - want["sum"]) <= n * 2.0 ** -52 * want["sum_abs"]             # the any-order summation bound, doubled
        assert abs(float(s[6]) - want["sum_sq"]) <= n * 2.0 ** -52 * want["sum_sq_abs"]
    return s


@pytest.fixture(scope="module")
def production():
    """The production-shape input and its restatement, computed once."""
    phi, det = pj.clear_of_zero(pj.drawn_phi(PRODUCTION, 0.45))
    return phi, det


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("amp", [0, 0.45, 0.8])
def test_determinant_map_and_stats_against_the_restatement(shape, amp):
    phi, det = pj.clear_of_zero(pj.drawn_phi(shape, amp))
    assert np.abs(det).min() >= 1e-5                                      # no sign is open
    s = _check_against_restatement(phi, det, (shape, amp))
    if amp == 0:                                                          # the identity map: exactly
        assert s[1] == 0 and s[2] == 0 and s[3] == 1.0 and s[4] == 1.0 and s[5] == s[0] and s[6] == s[0]


@pytest.mark.parametrize("shape", [(3, 4, 5), (17, 33, 29)])
def test_determinant_map_is_the_stencil_on_the_stored_displacement(shape):
    """The displacement that phi_jacobian_kernel rebuilds is the one oai_phi_to_itk_displacement stores: the numpy stencil on the stored
    fp64 field rounds to the kernel's map bit for bit."""
    phi = torch.from_numpy(pj.drawn_phi(shape, 0.45)).cuda()
    u = ops.phi_to_itk_displacement(phi).cpu().numpy()
    _, got = ops.phi_jacobian(phi, return_map=True)
    assert np.array_equal(got.cpu().numpy(), pj.det_of_displacement(u).astype(np.float32))


def test_production_shape(production):
    phi, det = production
    assert np.abs(det).min() >= 1e-5
    s = _check_against_restatement(phi, det, (PRODUCTION, 0.45))
    assert 0 < s[1] < s[0]
    ident = ops.phi_jacobian(torch.from_numpy(pj.drawn_phi(PRODUCTION, 0)).cuda()).cpu().numpy()
    cells = float(np.prod([n - 1 for n in PRODUCTION]))
    assert ident.tolist() == [cells, 0.0, 0.0, 1.0, 1.0, cells, cells]


def test_axis_aligned_stretch_reads_its_volume_change():
    shape = (8, 16, 64)
    phi = pj.stretch_phi(shape)
    s = _check_against_restatement(phi, pj.det_ref(phi), ("stretch", shape))
    tol = pj.stretch_tolerance(shape)
    print("mean", s[5] / s[0], "min", s[3], "max", s[4], "tolerance", tol)
    assert s[1] == 0 and abs(s[5] / s[0] - 1.1) <= tol and abs(s[3] - 1.1) <= tol and abs(s[4] - 1.1) <= tol


def test_a_planted_nan_and_inf_are_counted_apart():
    phi, det0 = pj.clear_of_zero(pj.drawn_phi((9, 33, 70), 0.45))
    phi[0, 2, 3, 4], phi[2, 4, 20, 66] = np.nan, np.inf
    det = pj.det_ref(phi)
    assert (~np.isfinite(det)).sum() == 8 and np.abs(det[np.isfinite(det)]).min() >= 1e-5
    s = _check_against_restatement(phi, det, "planted")
    assert s[2] == 8 and np.isfinite(s[3:]).all()


def test_stats_are_reproducible_and_do_not_depend_on_the_map(production):
    phi = torch.from_numpy(production[0]).cuda()
    a = ops.phi_jacobian(phi)
    b, _ = ops.phi_jacobian(phi, return_map=True)
    c = ops.phi_jacobian(phi)
    assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 1_000_003])
def test_mask_overlap_counts_equal_numpy(n):
    rng = np.random.default_rng(200 + n)
    special = np.array([0.5, np.nan, np.inf, -np.inf, np.nextafter(np.float32(0.5), np.float32(1.0))], np.float32)

    def draw():
        v = rng.uniform(0, 1, size=n).astype(np.float32)
        where = rng.uniform(size=n) < 0.2
        v[where] = special[rng.integers(0, len(special), size=int(where.sum()))]
        return v
    a, b = draw(), draw()
    if n >= 63:                                                           # every special value in both arrays, against each of the others
        a[-25:], b[-25:] = np.repeat(special, 5), np.tile(special, 5)
    fa, fb = np.isfinite(a), np.isfinite(b)
    ina, inb = fa & (np.nan_to_num(a) > 0.5), fb & (np.nan_to_num(b) > 0.5)
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got = ops.mask_overlap(ad, bd)
    assert got.dtype == torch.int64 and got.shape == (4,) and got.is_cuda
    assert got.cpu().tolist() == [int(ina.sum()), int(inb.sum()), int((ina & inb).sum()), int((~(fa & fb)).sum())]
    assert ops.mask_overlap(ad).cpu().tolist() == [int(ina.sum()), 0, 0, int((~fa).sum())]
    assert ops.mask_overlap(ad, None, threshold=0.25).cpu().tolist() == [int((fa & (np.nan_to_num(a) > 0.25)).sum()), 0, 0, int((~fa).sum())]
    if n > 8:                                                             # views that do not start on a 16-byte boundary: the one-by-one path
        got = ops.mask_overlap(ad[1:], bd[1:])
        assert got.cpu().tolist() == [int(ina[1:].sum()), int(inb[1:].sum()), int((ina & inb)[1:].sum()), int((~(fa & fb))[1:].sum())]


# ---- qc.registration_qc ----------------------------------------------------------------------------------------------------------------
def _meta(shape_zyx, spacing, origin=(0.0, 0.0, 0.0), direction=None):
    return Image(np.broadcast_to(np.zeros((), np.float32), shape_zyx), spacing, origin, np.eye(3) if direction is None else direction)


def _rotated_flipped():
    """test_mesh_transform_gpu.py::_rotated_flipped: a rotation about a skew axis with the y axis flipped, det = -1."""
    k = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    d = (np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K) @ np.diag([1.0, -1.0, 1.0])
    assert np.linalg.det(d) < 0
    return d


def _same_qc(a, b) -> bool:
    """Two records, field for field (a NaN equals a NaN; the map, a device tensor, by torch.equal)."""
    def same(x, y):
        if dataclasses.is_dataclass(x):
            return type(x) is type(y) and all(same(getattr(x, f.name), getattr(y, f.name)) for f in dataclasses.fields(x))
        if isinstance(x, dict):
            return isinstance(y, dict) and x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
        if torch.is_tensor(x):
            return torch.is_tensor(y) and torch.equal(x, y)
        if isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y):
            return True
        return type(x) is type(y) and x == y
    return same(a, b)


def test_volume_scale_on_rotated_and_flipped_geometries():
    from oai_analysis_2_amd.qc import registration_qc
    from oai_analysis_2_amd.registration import DisplacementTransform
    net = (6, 7, 9)
    A = _meta((11, 13, 17), [0.36, 0.37, 0.7], [10.0, -20.0, 5.0], _rotated_flipped())
    B = _meta((8, 12, 10), [0.4, 0.35, 0.75], [0.0, -1.0, 2.0], _rotated_flipped().T)
    phi = pj.drawn_phi(net, 0.45)
    want_j = pj.stats_ref(pj.det_ref(phi))
    for a, b in ((A, B), (B, A), (A, A), (_meta((11, 13, 17), [0.36, 0.37, 0.7]), B)):
        M_a, M_b = (ref.network_affine(m.spacing, m.origin, m.direction, m.size_xyz, net)[0] for m in (a, b))
        want = abs(np.linalg.det(M_a)) / abs(np.linalg.det(M_b))             # net -> A physical over net -> B physical
        extent = np.prod(a.spacing * a.size_xyz) / np.prod(b.spacing * b.size_xyz)
        qc = registration_qc(torch.from_numpy(phi).cuda(), a, b)
        print("volume scale", qc.volume_scale, "numpy", want, "ratio of the extents", extent)
        assert qc.volume_scale > 0 and abs(qc.volume_scale - want) <= 1e-12 * want and abs(qc.volume_scale - extent) <= 1e-12 * extent
        assert qc.dice is None and qc.overlap_counts is None and qc.cartilage_voxels is None and qc.cartilage_mm3 is None
        j = qc.jacobian
        assert (j.cells, j.folds, j.nonfinite) == (want_j["cells"], want_j["folds"], 0) and j.fold_fraction == want_j["folds"] / want_j["cells"]
        assert j.det_map is None and j.det_min == want_j["min"] and j.det_max == want_j["max"]
        assert abs(j.det_mean - want_j["sum"] / j.cells) <= 1e-12
        assert abs(j.det_std - math.sqrt(want_j["sum_sq"] / j.cells - (want_j["sum"] / j.cells) ** 2)) <= 1e-9
    bare = registration_qc(phi, return_map=True)                              # phi as an array, no geometry: the Jacobian alone
    assert bare.volume_scale is None and bare.jacobian.det_map.is_cuda and tuple(bare.jacobian.det_map.shape) == (5, 6, 8)
    assert bare.jacobian.folds == want_j["folds"]
    via = DisplacementTransform(ref.displacement(phi), A, B, phi).jacobian()
    assert _same_qc(via, registration_qc(phi, A, B))
    with pytest.raises(ValueError, match="no phi"):
        DisplacementTransform(ref.displacement(phi), A, B, None).jacobian()


def test_dice_and_cartilage_volume():
    from oai_analysis_2_amd.pipeline import VolumeResult
    from oai_analysis_2_amd.qc import QCReference, registration_qc
    rng = np.random.default_rng(5)
    shape = (5, 6, 7)
    fc = rng.uniform(0, 1, size=shape).astype(np.float32)
    left = np.zeros(shape, np.float32)
    left[:, :, :3] = 0.9
    right = np.zeros(shape, np.float32)
    right[:, :, 3:] = 0.9
    empty = np.full(shape, 0.5, np.float32)                                   # exactly the threshold: in no set
    meta = _meta((4, 8, 9), [0.36, 0.37, 0.7], [1.0, 2.0, 3.0], _rotated_flipped())
    atlas = _meta(shape, [0.4, 0.35, 0.75])
    phi = torch.from_numpy(pj.drawn_phi((3, 4, 5), 0.45)).cuda()
    dev = lambda a: torch.from_numpy(a).cuda()
    patient_fc = rng.uniform(0, 1, size=(4, 8, 9)).astype(np.float32)
    res = VolumeResult(dev(patient_fc), dev(np.zeros((4, 8, 9), np.float32)), phi, dev(fc), dev(left), meta_A=meta, meta_B=atlas)
    qc = registration_qc(res, reference=QCReference(Image(fc, atlas.spacing), dev(right)))     # an Image and a device tensor
    assert qc.dice == {"FC": 1.0, "TC": 0.0}
    n_fc = int((fc > 0.5).sum())
    assert qc.overlap_counts == {"FC": (n_fc, n_fc, n_fc, 0), "TC": (5 * 6 * 3, 5 * 6 * 4, 0, 0)}
    count = int((patient_fc > 0.5).sum())
    assert qc.cartilage_voxels == {"FC": count, "TC": 0}
    assert qc.cartilage_mm3 == {"FC": count * float(np.prod(meta.spacing)), "TC": 0.0}
    assert qc.volume_scale > 0 and qc.jacobian.cells == 24
    res.fc_atlas = dev(empty)
    qc = registration_qc(res, reference=QCReference(empty, right))
    assert math.isnan(qc.dice["FC"]) and qc.overlap_counts["FC"] == (0, 0, 0, 0) and qc.dice["TC"] == 0.0
    plain = registration_qc(res)                                              # no reference: no Dice, the rest as before
    assert plain.dice is None and plain.overlap_counts is None and plain.cartilage_voxels == qc.cartilage_voxels
    res.meta_A = res.meta_B = None                                            # no geometry: counts, but no millimetres
    bare = registration_qc(res)
    assert bare.volume_scale is None and bare.cartilage_mm3 is None and bare.cartilage_voxels == qc.cartilage_voxels


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------------
def _small_pipe(unet_sd, precision="fp16x3"):
    """tests/test_thickness_native_gpu.py::_small_pipe"""
    from oai_analysis_2_amd.pipeline import VolumePipeline
    from oai_analysis_2_amd.registration import IconEngine
    from oai_analysis_2_amd.segmentation.engine import UNetEngine
    shape, net = (24, 72, 72), (40, 48, 48)
    atlas = Image(make_volume(10, shape), [0.4, 0.35, 0.75], [0.0, -1.0, 2.0])
    pipe = VolumePipeline(UNetEngine(unet_sd, precision=precision), IconEngine(make_icon_state_dict(1, last_scale=0.1), net_shape=net), atlas,
                          tile_zyx=(16, 32, 32), overlap_zyx=(4, 8, 8), crop_zyx=(4, 8, 8), batch=8)
    return pipe, shape


_FIVE = ("fc", "tc", "phi", "fc_atlas", "tc_atlas")


@pytest.fixture(scope="module")
def runs():
    """One small pipeline and one volume run without and with QC, shared by the tests below."""
    pipe, shape = _small_pipe(make_unet_state_dict(1, width_div=2))
    vol = make_volume(9, shape)
    meta = Image(vol, [0.36, 0.37, 0.7], [1.0, 2.0, 3.0])
    v = torch.from_numpy(vol).cuda()
    return pipe, v, meta, pipe.run(v, meta), pipe.run(v, meta, qc=True)


def test_pipeline_run_with_qc_changes_no_bit(runs):
    from oai_analysis_2_amd.qc import RegistrationQC, registration_qc
    pipe, v, meta, base, on = runs
    for name in _FIVE:
        assert torch.equal(getattr(on, name), getattr(base, name)), name
    assert base.qc is None and isinstance(on.qc, RegistrationQC)
    assert _same_qc(on.qc, registration_qc(on))
    assert _same_qc(on.qc, registration_qc(on.phi, meta, pipe.atlas)) is False          # (the bare-phi form has no patient-grid counts ...)
    assert on.qc.volume_scale == registration_qc(on.phi, meta, pipe.atlas).volume_scale > 0      # ... but the same Jacobian and scale
    assert _same_qc(on.qc.jacobian, registration_qc(on.phi).jacobian)
    j = on.qc.jacobian
    print("small pipeline: folds", j.folds, "of", j.cells, "det", j.det_min, "..", j.det_max, "mean", j.det_mean, "std", j.det_std,
          "volume scale", on.qc.volume_scale, "voxels", on.qc.cartilage_voxels)
    assert j.cells == 39 * 47 * 47 and j.nonfinite == 0 and j.det_min <= j.det_mean <= j.det_max
    want = pj.stats_ref(pj.det_ref(on.phi.cpu().numpy()))
    assert (j.folds, j.det_min, j.det_max) == (want["folds"], want["min"], want["max"])
    assert on.qc.dice is None and on.qc.cartilage_voxels == {k: int((getattr(on, k.lower()) > 0.5).sum()) for k in ("FC", "TC")}
    assert on.qc.cartilage_mm3 == {k: n * float(np.prod(meta.spacing)) for k, n in on.qc.cartilage_voxels.items()}
    with pytest.raises(ValueError, match="qc must be"):
        pipe.run(v, meta, qc="yes")


def test_pipeline_dice_against_its_own_warped_maps(runs):
    from oai_analysis_2_amd.qc import QCReference
    pipe, v, meta, base, on = runs
    reference = QCReference(on.fc_atlas, on.tc_atlas)
    again = pipe.run(v, meta, qc=reference)
    for name in _FIVE:
        assert torch.equal(getattr(again, name), getattr(base, name)), name
    for kind in ("FC", "TC"):
        n_a, n_b, n_both, n_bad = again.qc.overlap_counts[kind]
        assert n_a == n_b == n_both and n_bad == 0
        assert again.qc.dice[kind] == 1.0 if n_a else math.isnan(again.qc.dice[kind])
    assert _same_qc(again.qc.jacobian, on.qc.jacobian) and again.qc.cartilage_voxels == on.qc.cartilage_voxels


def test_qc_stream_reproduces_the_records_in_order(runs):
    from oai_analysis_2_amd.dask_processing import qc_stream
    from oai_analysis_2_amd.qc import QCReference, registration_qc
    pipe, v, meta, base, on = runs
    reference = QCReference(on.fc_atlas, on.tc_atlas)
    out = list(qc_stream(iter([(7, on), (3, base)]), reference))
    assert [i for i, _ in out] == [7, 3]
    assert _same_qc(out[0][1], registration_qc(on, reference=reference)) and _same_qc(out[1][1], registration_qc(base, reference=reference))
    assert out[0][1].dice is not None and _same_qc(list(qc_stream([(0, on)]))[0][1], on.qc)


def test_bad_arguments_raise_and_do_not_fault():
    from oai_analysis_2_amd.qc import registration_qc
    phi = torch.from_numpy(ref.identity_phi((4, 5, 6))).cuda()
    a = torch.zeros(10, device="cuda")
    bad = (_lib.OaiError, ValueError)
    for fn in (ops.phi_jacobian, registration_qc):
        with pytest.raises(bad):
            fn(phi[0])                                                        # rank 3
        with pytest.raises(bad):
            fn(phi[:2])                                                       # two channels
        with pytest.raises(bad):
            fn(phi.double())                                                  # dtype
        with pytest.raises(bad):
            fn(phi.cpu())                                                     # a host tensor
        with pytest.raises(bad):
            fn(phi[:, :1])                                                    # D = 1
    with pytest.raises(bad):
        ops.mask_overlap(a, torch.zeros(11, device="cuda"))                   # mismatched lengths
    with pytest.raises(bad):
        ops.mask_overlap(a.cpu())
    with pytest.raises(bad):
        ops.mask_overlap(a, a.double())
    with pytest.raises(bad):
        ops.phi_jacobian(phi, out=torch.zeros(6, dtype=torch.float64, device="cuda"))
    stats = ops.phi_jacobian(phi)                                             # and the device is fine afterwards
    assert stats.cpu().tolist() == [60.0, 0.0, 0.0, 1.0, 1.0, 60.0, 60.0]
    assert ops.mask_overlap(a + 1).cpu().tolist() == [10, 0, 0, 0]
