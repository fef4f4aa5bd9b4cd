"""GPU: image-similarity QC (csrc/similarity.hip, ops.image_moments / joint_histogram / histogram_entropies / lncc,
qc.image_similarity, QCReference(image=, roi_mm=), registration_qc(patient_image=), VolumePipeline.run(qc=)) against the numpy
restatement of tests/similarity_ref.py: counts and tables exactly, fp64 sums bit for bit, the map of cc to the last operations'
rounding, the entropies to the device's log, and the record through every layer."""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

import edt_ref
import mesh_transform_ref as mref
import similarity_ref as sr
from oai_analysis_2_amd import _lib, ops, qc
from oai_analysis_2_amd.image import Image
from oai_analysis_2_amd.synth import make_icon_state_dict, make_unet_state_dict, make_volume

pytestmark = pytest.mark.gpu

dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def image(shape, seed):
    """float32 in [0, 1]: smooth structure plus texture, so that local variances are neither zero nor all alike."""
    rng = np.random.default_rng([seed, *shape])
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    smooth = 0.5 + 0.2 * np.sin(0.31 * x + 0.4 + seed) * np.cos(0.23 * y) + 0.15 * np.sin(0.5 * z + 0.17 * x)
    return np.clip(smooth + 0.1 * rng.standard_normal(shape), 0.0, 1.0).astype(np.float32)


# ---- moments -----------------------------------------------------------------------------------------------------------------------------
# one past a block's share of 1024 positions; one past the grid-stride cap of 2048 blocks, where threads take a second position
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 1025, 2048 * 1024 + 1])
def test_moments_are_the_restated_ordered_sums(n):
    rng = np.random.default_rng(300 + n % 1000)
    a, b = (rng.uniform(-1, 2, size=n).astype(np.float32) for _ in range(2))
    mask = (rng.uniform(size=n) < 0.6).astype(np.uint8)
    if n >= 63:                                                    # NaN and Inf in a, in b and in both, inside and outside the mask
        a[[3, 10, 40]], b[[5, 10, 41]] = [np.nan, np.inf, -np.inf], [np.inf, np.nan, np.nan]
        mask[[3, 5, 10]], mask[[40, 41]] = 1, 0
    for m in (None, mask):
        got = ops.image_moments(dev(a), dev(b), None if m is None else dev(m))
        assert got.dtype == torch.float64 and got.shape == (8,) and got.is_cuda
        got, want = got.cpu().numpy(), sr.moments_stats(a, b, m)
        on = np.ones(n, bool) if m is None else m != 0
        fin = np.isfinite(a) & np.isfinite(b)
        assert got[0] == (on & fin).sum() and got[1] == (on & ~fin).sum()
        assert got.view(np.int64).tolist() == want.view(np.int64).tolist(), (got - want)
    if n == 1000:                                                  # a slot of a larger buffer; reproducible
        buf = torch.zeros(12, dtype=torch.float64, device="cuda")
        assert ops.image_moments(dev(a), dev(b), out=buf[2:10]) is not None and buf[2:10].cpu().numpy().tolist() == sr.moments_stats(a, b).tolist()
        assert buf[:2].tolist() == [0, 0] and buf[10:].tolist() == [0, 0]


# ---- joint histogram and entropies -----------------------------------------------------------------------------------------------------
BINS = (1, 2, 7, 32, 64, 128)          # one cell; odd; the LDS table's limit of 64; global atomics above it
BIG = (40, 96, 96)                     # 512 blocks and 2.8 positions per thread: the grid-stride loop


@functools.lru_cache(maxsize=None)
def hist_data(kind, bins):
    rng = np.random.default_rng(17)
    if kind == "one":
        return np.array([0.3], np.float32), np.array([0.9], np.float32), None
    if kind == "uniform":
        return rng.uniform(0, 1, BIG).astype(np.float32), rng.uniform(0, 1, BIG).astype(np.float32), None
    if kind == "constant":
        return np.full(BIG, 0.25, np.float32), np.full(BIG, 0.75, np.float32), None
    if kind == "zeros95":                                           # a knee volume: mostly background
        a, b = (np.where(rng.uniform(size=BIG) < 0.95, 0.0, rng.uniform(0, 1, BIG)).astype(np.float32) for _ in range(2))
        return a, b, None
    if kind == "masked":
        return rng.uniform(0, 1, (9, 33, 70)).astype(np.float32), rng.uniform(0, 1, (9, 33, 70)).astype(np.float32), (rng.uniform(size=(9, 33, 70)) < 0.4).astype(np.uint8)
    assert kind == "edges"                                          # lo, hi, every bin edge, its float32 neighbours, outside, non-finite
    edges = (np.arange(bins + 1, dtype=np.float64) / bins).astype(np.float32)
    vals = np.concatenate([edges, np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(2)),
                           np.array([-0.5, -1e30, 1.5, 1e30, np.nan, np.inf, -np.inf], np.float32)]).astype(np.float32)
    a, b = np.repeat(vals, len(vals)), np.tile(vals, len(vals))    # every value against every other
    return a, b, None


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("kind", ["one", "uniform", "constant", "zeros95", "masked", "edges"])
def test_joint_histogram_equals_the_restatement_and_its_entropies(kind, bins):
    a, b, mask = hist_data(kind, bins)
    want = sr.joint_histogram(a, b, bins, mask=mask)
    got = ops.joint_histogram(dev(a), dev(b), bins, mask=None if mask is None else dev(mask))
    assert got.dtype == torch.int64 and got.shape == (bins * bins + 1,) and got.is_cuda
    h = got.cpu().numpy()
    assert np.array_equal(h, want)
    assert h.sum() == (a.size if mask is None else int(mask.sum())) and h[-1] == (0 if kind != "edges" else want[-1])
    if kind == "constant":
        assert (h != 0).sum() == 1
    ent, want_e = ops.histogram_entropies(got, bins).cpu().numpy(), sr.entropies(want, bins)
    diff = float(np.abs(ent - want_e).max())
    print(kind, bins, "N", ent[0], "entropies", ent[1:].tolist(), "largest difference from the restatement", diff)
    assert ent[0] == want_e[0] == h[:-1].sum() and diff <= 1e-12
    if kind in ("one", "constant") or bins == 1:
        assert ent[1:].tolist() == [0.0, 0.0, 0.0]                  # a single occupied cell: exactly


def test_entropies_of_an_empty_table_and_other_ranges():
    empty = torch.zeros(65, dtype=torch.int64, device="cuda")
    ent = ops.histogram_entropies(empty, 8).cpu().numpy()
    assert ent[0] == 0 and np.isnan(ent[1:]).all()
    h = ops.joint_histogram(torch.zeros(0, device="cuda"), torch.zeros(0, device="cuda"), 8)      # n = 0: a zeroed table
    assert h.cpu().tolist() == [0] * 65
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=5000).astype(np.float32), rng.uniform(-7, 300, 5000).astype(np.float32)
    got = ops.joint_histogram(dev(a), dev(b), 13, (-1.5, 2.0), (0.0, 255.0)).cpu().numpy()
    assert np.array_equal(got, sr.joint_histogram(a, b, 13, (-1.5, 2.0), (0.0, 255.0)))
    stale = torch.full((13 * 13 + 1,), 99, dtype=torch.int64, device="cuda")                      # the call zeroes its table
    assert np.array_equal(ops.joint_histogram(dev(a), dev(b), 13, (-1.5, 2.0), (0.0, 255.0), out=stale).cpu().numpy(), got)


# ---- LNCC ----------------------------------------------------------------------------------------------------------------------------------
LNCC_CASES = [(0.0, (1, 1, 1)), (0.0, (2, 3, 5)),
              (1.0, (3, 3, 3)),                                     # the smallest legal: every tap reflects
              (1.0, (3, 4, 70)), (1.0, (5, 300, 4)), (1.0, (260, 3, 3)),       # a line longer than a wave / a block on each axis in turn
              (4.0, (9, 9, 9)), (4.0, (9, 33, 70)), (4.0, (12, 40, 130)),
              (16.0, (33, 33, 40)),
              (4.0, (40, 96, 96))]


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64).tolist()


def _same_stats(got, want) -> bool:
    """The six figures bit for bit; with no counted voxel, min and max are NaN on both sides."""
    if want[0] == 0:
        return _bits(got[:4]) == _bits(want[:4]) and bool(np.isnan(got[4:]).all() and np.isnan(want[4:]).all())
    return _bits(got) == _bits(want)


@pytest.mark.parametrize("sigma,shape", LNCC_CASES)
def test_lncc_map_and_stats_against_the_restatement(sigma, shape):
    a, b = image(shape, 1), image(shape, 2)
    taps, radius = sr.gaussian_taps(sigma)
    want = sr.lncc_map(a, b, taps, radius)
    stats, cc = ops.lncc(dev(a), dev(b), sigma, return_map=True)
    assert stats.dtype == torch.float64 and stats.shape == (6,) and cc.dtype == torch.float64 and tuple(cc.shape) == shape
    cc, s = cc.cpu().numpy(), stats.cpu().numpy()
    err = np.abs(cc - want)
    print(sigma, shape, "voxels that differ from the restatement (expected 0):", int((cc != want).sum()), "largest difference", float(err.max()),
          "mean cc", s[2] / s[0])
    assert np.isfinite(cc).all() and (err <= 4 * 2.0 ** -52 * np.maximum(np.abs(want), 1.0)).all()
    # the six statistics: the restated ordered reduction of the device's own map, bit for bit; the same without the map
    assert _bits(s) == _bits(sr.lncc_stats(cc)) and s[0] == cc.size and s[1] == 0
    assert _bits(ops.lncc(dev(a), dev(b), sigma).cpu().numpy()) == _bits(s)
    rng = np.random.default_rng(4)
    for mask in ((rng.uniform(size=shape) < 0.5).astype(np.uint8), np.zeros(shape, np.uint8), np.full(shape, 7, np.uint8)):
        m, cm = ops.lncc(dev(a), dev(b), sigma, mask=dev(mask), return_map=True)
        assert np.array_equal(cm.cpu().numpy(), cc)                 # the map covers every voxel, masked or not
        want_s = sr.lncc_stats(cc, mask)
        for got_s in (m.cpu().numpy(), ops.lncc(dev(a), dev(b), sigma, mask=dev(mask)).cpu().numpy()):
            assert got_s[0] == (mask != 0).sum() and _same_stats(got_s, want_s)
            assert not mask.all() or _same_stats(got_s, s)


def test_lncc_refuses_what_reflect_padding_cannot_do():
    a = torch.zeros((8, 9, 9), device="cuda")
    with pytest.raises(_lib.OaiError, match="longer than the radius"):
        ops.lncc(a, a, 4.0)
    big = torch.zeros((40, 40, 70), device="cuda")
    with pytest.raises(_lib.OaiError, match="radius"):
        ops.lncc(big, big, 16.5)                                    # radius 33
    bad = (_lib.OaiError, ValueError)
    with pytest.raises(bad):
        ops.lncc(big, big[:39])
    with pytest.raises(bad):
        ops.lncc(big, big.double())
    with pytest.raises(bad):
        ops.lncc(big.cpu(), big.cpu())
    with pytest.raises(bad):
        ops.lncc(big, big, mask=torch.zeros((40, 40, 70), device="cuda"))       # a float mask
    with pytest.raises(bad):
        ops.joint_histogram(big, big, 129)
    with pytest.raises(bad):
        ops.joint_histogram(big, big, 64, (1.0, 1.0))
    with pytest.raises(bad):
        ops.image_moments(big, big[:, :, :69])
    assert ops.lncc(big, big, 1.0).cpu().numpy()[:4].tolist() == [112000.0, 0.0, 0.0, 0.0]      # and the device is fine afterwards


def _reached(n, i0, radius):
    """The positions of an axis whose window holds i0: some j with reflect(i + j - radius) == i0."""
    hit = np.zeros(n, bool)
    for i in range(n):
        for d in range(-radius, radius + 1):
            k = i + d
            k = -k if k < 0 else (2 * (n - 1) - k if k >= n else k)
            hit[i] |= k == i0
    return hit


@pytest.mark.parametrize("at", [(5, 20, 60), (0, 39, 127)])
def test_a_nan_poisons_exactly_its_windows(at):
    shape, sigma, radius = (12, 40, 130), 4.0, 8
    a, b = image(shape, 1), image(shape, 2)
    a[at] = np.nan
    stats, cc = ops.lncc(dev(a), dev(b), sigma, return_map=True)
    cc, s = cc.cpu().numpy(), stats.cpu().numpy()
    want = np.einsum("i,j,k->ijk", *[_reached(n, i0, radius) for n, i0 in zip(shape, at)]).astype(bool)
    assert np.array_equal(~np.isfinite(cc), want)
    assert s[1] == want.sum() and s[0] == cc.size - want.sum() and np.isfinite(s).all()
    assert _bits(s) == _bits(sr.lncc_stats(cc))
    taps, _ = sr.gaussian_taps(sigma)
    ref = sr.lncc_map(a, b, taps, radius)
    assert np.array_equal(np.isfinite(ref), np.isfinite(cc)) and (np.abs(cc - ref)[~want] <= 4 * 2.0 ** -52).all()


# ---- the record --------------------------------------------------------------------------------------------------------------------------
def _same(x, y) -> bool:
    """Two records field for field: a NaN equals a NaN, device tensors by torch.equal."""
    if dataclasses.is_dataclass(x):
        return type(x) is type(y) and all(_same(getattr(x, f.name), getattr(y, f.name)) for f in dataclasses.fields(x))
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(_same(x[k], y[k]) for k in x)
    if torch.is_tensor(x):
        return torch.is_tensor(y) and torch.equal(x, y)
    if isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y):
        return True
    return type(x) is type(y) and x == y


def test_image_similarity_is_one_record_for_tensors_arrays_and_images():
    shape = (9, 33, 70)
    a, b = image(shape, 1), image(shape, 2)
    mask = (np.random.default_rng(8).uniform(size=shape) < 0.5)
    rec = qc.image_similarity(dev(a), dev(b))
    assert _same(rec, qc.image_similarity(a, b)) and _same(rec, qc.image_similarity(Image(a, [0.3, 0.4, 0.5]), dev(b)))
    taps, radius = sr.gaussian_taps(4.0)
    cc = sr.lncc_map(a, b, taps, radius)
    ent = sr.entropies(sr.joint_histogram(a, b, 64), 64)
    want = qc.similarity_from_stats(np.concatenate([sr.moments_stats(a, b), sr.lncc_stats(cc), ent]), 4.0, 64)
    print("device", rec, "\nrestatement", want)
    assert (rec.n, rec.nonfinite, rec.ncc, rec.mse, rec.sigma, rec.bins) == (want.n, 0, want.ncc, want.mse, 4.0, 64)
    for f in ("lncc", "lncc_std", "lncc_min", "lncc_max", "mi", "nmi", "entropy_a", "entropy_b", "entropy_joint"):
        assert abs(getattr(rec, f) - getattr(want, f)) <= 1e-11, f
    assert abs(rec.ncc - np.corrcoef(a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64))[0, 1]) <= 1e-12
    masked = qc.image_similarity(a, b, sigma=1.0, bins=32, mask=mask, return_map=True)
    assert _same(masked, qc.image_similarity(dev(a), dev(b), sigma=1.0, bins=32, mask=dev(mask.astype(np.uint8)), return_map=True))
    assert masked.n == mask.sum() and masked.cc_map.dtype == torch.float64 and tuple(masked.cc_map.shape) == shape and masked.bins == 32
    self_ = qc.image_similarity(a, a)
    assert self_.ncc == 1.0 and self_.mse == 0.0 and 0.99 < self_.lncc <= 1.0 and abs(self_.nmi - 2.0) <= 1e-12
    with pytest.raises(ValueError):
        qc.image_similarity(a, b[:8])


# On a grid whose every axis has 2^k + 1 voxels the identity map's float32 coordinates i / (n - 1) are exact and so is every step of
# the sampler's coordinate arithmetic: grid_sample3d returns the image itself and "after" is "before" to the bit.  On other grids the
# float32 coordinates are not lattice points (the observation csrc/phi_jacobian.hip makes) and the sampler interpolates by 1e-7.
EXACT = (9, 17, 33)


def _maps(shape):
    fc, tc = edt_ref.box(shape, (3, 4, 5), (2, 6, 9)), edt_ref.box(shape, (5, 9, 14), (2, 5, 12))
    return fc, tc


def test_identity_phi_changes_nothing():
    atlas, patient = image(EXACT, 1), image(EXACT, 2)
    fc, tc = _maps(EXACT)
    reference = qc.QCReference(dev(fc), dev(tc), image=dev(atlas), net_shape=EXACT, roi_mm=2.0, spacing_xyz=(0.5, 0.4, 0.7))
    assert torch.equal(reference.image_net, dev(atlas))             # resizing to its own shape is the identity
    phi = ops.warp_chain(EXACT, start=torch.zeros((3, *EXACT), device="cuda"))          # the device's own identity map
    rec = qc.registration_qc(phi, reference=reference, patient_image=dev(patient))
    assert sorted(rec.similarity) == ["after", "after_roi", "before", "before_roi"]
    assert _same(rec.similarity["after"], rec.similarity["before"]) and _same(rec.similarity["after_roi"], rec.similarity["before_roi"])
    assert _same(rec.similarity["before"], qc.image_similarity(patient, atlas))
    assert _same(rec.similarity["before_roi"], qc.image_similarity(patient, atlas, mask=reference.roi))
    assert 0 < rec.similarity["before_roi"].n == int(reference.roi.sum()) < patient.size
    assert rec.jacobian.folds == 0 and rec.dice is None
    # without a patient image, or without the atlas image, nothing is computed
    assert qc.registration_qc(phi, reference=reference).similarity is None
    assert qc.registration_qc(phi, reference=qc.QCReference(dev(fc), dev(tc)), patient_image=dev(patient)).similarity is None
    with pytest.raises(ValueError, match="spacing"):
        qc.QCReference(dev(fc), dev(tc), roi_mm=2.0)


def test_a_known_warp_is_recognised():
    """The patient image is the atlas image pulled through the inverse of a smooth map phi, so that warping it through phi gives the
    atlas image back up to two interpolations: the similarity after the warp must beat the similarity before it."""
    shape = (24, 48, 64)
    z, y, x = np.meshgrid(*[np.linspace(0, 1, n) for n in shape], indexing="ij")
    atlas = (0.5 + 0.25 * np.sin(28 * x + 1) * np.cos(22 * y) + 0.2 * np.sin(16 * z + 12 * x * y)).astype(np.float32)      # wavelengths of 9 to 14 voxels
    disp = np.stack([0.05 * np.sin(2 * np.pi * y) * np.ones_like(z), 0.04 * np.sin(2 * np.pi * x), 0.04 * np.cos(2 * np.pi * z) * np.sin(np.pi * x)])
    phi = dev((mref.identity_phi(shape) + disp).astype(np.float32))
    psi, record = ops.invert_phi(phi)
    patient = ops.grid_sample3d(dev(atlas)[None], psi)[0]
    fc, tc = _maps(shape)
    reference = qc.QCReference(dev(fc), dev(tc), image=dev(atlas), net_shape=shape)
    rec = qc.registration_qc(phi, reference=reference, patient_image=patient)
    before, after = rec.similarity["before"], rec.similarity["after"]
    print("the inverse:", record, "\nbefore", before, "\nafter", after)
    assert sorted(rec.similarity) == ["after", "before"]
    assert after.lncc > before.lncc and after.nmi > before.nmi and after.ncc > before.ncc and after.mse < before.mse
    assert after.lncc > 0.9 and rec.jacobian.folds == 0


def test_roi_equals_the_restatement():
    shape, net = (10, 20, 24), (9, 17, 33)
    spacing = np.array([0.5, 0.4, 0.7])
    fc, tc = _maps(shape)
    reference = qc.QCReference(Image(fc, spacing), Image(tc, spacing), net_shape=net, roi_mm=1.5)
    assert reference.image_net is None and reference.surfaces is None
    resized = [ops.resize_trilinear(dev(m)[None], net)[0].cpu().numpy() for m in (fc, tc)]
    cartilage = ((resized[0] > 0.5) | (resized[1] > 0.5)).astype(np.uint8)
    net_spacing = spacing * np.array(shape[::-1], np.float64) / np.array(net[::-1], np.float64)
    dist = edt_ref.edt_dist32(edt_ref.edt_sq_lines(cartilage, net_spacing))
    want = (dist <= np.float32(1.5)).astype(np.uint8)
    got = reference.roi.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == net and np.array_equal(got, want)
    assert cartilage.sum() < want.sum() < want.size and np.array_equal(reference.roi_spacing_xyz, net_spacing)


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------------
def _small_pipe(unet_sd, precision="fp16x3"):
    """tests/test_registration_qc_gpu.py::_small_pipe"""
    from oai_analysis_2_amd.pipeline import VolumePipeline
    from oai_analysis_2_amd.registration import IconEngine
    from oai_analysis_2_amd.segmentation.engine import UNetEngine
    shape, net = (24, 72, 72), (40, 48, 48)
    atlas = Image(make_volume(10, shape), [0.4, 0.35, 0.75], [0.0, -1.0, 2.0])
    pipe = VolumePipeline(UNetEngine(unet_sd, precision=precision), IconEngine(make_icon_state_dict(1, last_scale=0.1), net_shape=net), atlas,
                          tile_zyx=(16, 32, 32), overlap_zyx=(4, 8, 8), crop_zyx=(4, 8, 8), batch=8)
    return pipe, shape, net


_FIVE = ("fc", "tc", "phi", "fc_atlas", "tc_atlas")


def test_pipeline_run_with_the_similarity_changes_no_bit():
    from oai_analysis_2_amd.dask_processing import qc_stream
    pipe, shape, net = _small_pipe(make_unet_state_dict(1, width_div=2))
    vol = make_volume(9, shape)
    meta = Image(vol, [0.36, 0.37, 0.7], [1.0, 2.0, 3.0])
    v = dev(vol)
    base = pipe.run(v, meta)
    plain = pipe.run(v, meta, qc=qc.QCReference(base.fc_atlas, base.tc_atlas))
    for name in _FIVE:
        assert torch.equal(getattr(plain, name), getattr(base, name)), name
    assert base.qc is None and plain.qc.similarity is None and plain.image_net is None and base.image_net is None
    fc, tc = _maps(shape)                                            # atlas maps with cartilage in them, whatever the synthetic U-Net gives
    reference = qc.QCReference(Image(fc, pipe.atlas.spacing), Image(tc, pipe.atlas.spacing), image=pipe.atlas, net_shape=net, roi_mm=3.0)
    assert 0 < int(reference.roi.sum()) < 40 * 48 * 48
    full = pipe.run(v, meta, qc=reference)
    for name in _FIVE:
        assert torch.equal(getattr(full, name), getattr(base, name)), name
    assert torch.equal(full.image_net, ops.resize_trilinear(v[None], net)[0]) and torch.equal(reference.image_net, pipe._atlas_net)
    sim = full.qc.similarity
    print({k: r for k, r in sim.items()})
    assert sorted(sim) == ["after", "after_roi", "before", "before_roi"]
    for key, rec in sim.items():
        figures = [getattr(rec, f.name) for f in dataclasses.fields(rec) if f.name != "cc_map"]
        assert all(math.isfinite(x) for x in figures) and rec.cc_map is None and rec.nonfinite == 0, key
        assert rec.n == (40 * 48 * 48 if "roi" not in key else int(reference.roi.sum())) and -1.0 <= rec.lncc <= 1.0 and rec.nmi >= 1.0 - 1e-12
    assert _same(full.qc.jacobian, plain.qc.jacobian) and sorted(full.qc.dice) == ["FC", "TC"]
    # the same record from the result alone, from an explicit full-size patient image, and through qc_stream
    assert _same(qc.registration_qc(full, reference=reference).similarity, sim)
    assert _same(qc.registration_qc(base, reference=reference, patient_image=v).similarity, sim)
    assert _same(list(qc_stream([(4, full)], reference))[0][1].similarity, sim)
    assert list(qc_stream([(4, base)], reference))[0][1].similarity is None
