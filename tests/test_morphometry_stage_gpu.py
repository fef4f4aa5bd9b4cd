"""GPU: cartilage morphometry end to end (ThicknessAtlas.measure(..., morphometry=)) on a synthetic spherical cap of known inner radius:
the atlas measured against itself, a denuded cone against the analytic cap area, patient space under the identity and a doubled
spacing, regions painted on the thickness image, the default path left alone, the per-cartilage error path, and the pass-through of
VolumePipeline.run and thickness_stream."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import mesh_transform_ref as tref
import morphometry_ref as mref
from oai_analysis_2_amd.image import Image
from oai_analysis_2_amd.synth import make_icon_state_dict, make_unet_state_dict, make_volume

pytestmark = pytest.mark.gpu

_sig = lambda t: 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))
MIN_CELLS = {"FC": 3000, "TC": 100}
NO_REGION = "n_samples=0 should be >= n_clusters=2."
CENTRE = np.array([32.0, -30.0, 32.0])     # (x, y, z) of the sphere, in mm: the spacing S is 1
R_MID, T_CAP, RHO, S = 60.0, 6.0, 22.0, 1.0   # the shell |r - 60| < 3 inside the cylinder rho < 22 about the sphere's +y axis
THETA = math.radians(10.0)                 # half-angle of the denuded cone about that axis


def _cap(cone=None):
    """A cap of a SPHERICAL shell (test_thickness_map_gpu.py::_bowl with an isotropic z): thickness 6 about radius 60, so the two surfaces
    are spheres of radius 57 and 63; ``cone``: the probability is zeroed inside the cone of that half-angle about the +y axis, apex at the
    sphere's centre."""
    D, H, W = 64, 40, 64
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    r = np.sqrt((x - CENTRE[0]) ** 2 + (z - CENTRE[2]) ** 2 + (y - CENTRE[1]) ** 2)
    prob = _sig(2.0 * (np.abs(r - R_MID) - T_CAP / 2)) * _sig(2.0 * (np.sqrt((x - CENTRE[0]) ** 2 + (z - CENTRE[2]) ** 2) - RHO))
    if cone is not None:
        prob = np.where((y - CENTRE[1]) > r * math.cos(cone), 0.0, prob)
    return Image(prob.astype(np.float32), [S, S, S])


def _slab(shift_x=0.0):
    """test_thickness_stage_gpu.py::_slab: a femoral-cartilage-like slab, optionally shifted along x."""
    D, H, W = 80, 192, 192
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    x = x - shift_x
    R, T = 110.0, 5.0
    r = np.sqrt((x - 96) ** 2 + ((z - 40) * 1.9) ** 2 + (y + 30) ** 2)
    prob = _sig(2.0 * (np.abs(r - R) - T / 2)) * _sig(2.0 * (np.sqrt((x - 96) ** 2 + ((z - 40) * 1.9) ** 2) - 70))
    return Image(prob.astype(np.float32), [0.36, 0.36, 0.7])


def _meta(shape_zyx, spacing, origin=(0.0, 0.0, 0.0)):
    return Image(np.broadcast_to(np.zeros((), np.float32), shape_zyx), spacing, origin, np.eye(3))


def _f32bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


def _same(x, y):
    return x == y or (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y))


def _same_record(a, b, skip=()):
    a, b = dataclasses.asdict(a), dataclasses.asdict(b)
    return all(_same(a[k], b[k]) for k in a if k not in skip)


def _same_morphometry(a, b):
    return set(a) == set(b) and all(_same_record(a[k].all, b[k].all) and list(a[k].regions) == list(b[k].regions) and
                                    all(_same_record(a[k].regions[n], b[k].regions[n]) for n in a[k].regions) for k in a)


AREAS = ("area_mm2", "covered_mm2", "denuded_mm2")
LENGTHS = ("mean_thickness_covered", "mean_thickness_total", "std", "min", "max", "vertex_mean", "vertex_std")


@pytest.fixture(scope="module")
def atlas():
    from oai_analysis_2_amd.thickness import ThicknessAtlas
    return ThicknessAtlas(_slab(1.5), _cap(), image_shape=(96, 128), min_cells=MIN_CELLS)


@pytest.fixture(scope="module")
def maps():
    return {"FC": torch.from_numpy(_slab(1.5).array).cuda(), "TC": torch.from_numpy(_cap().array).cuda(),
            "hole": torch.from_numpy(_cap(THETA).array).cuda(), "none": torch.zeros((8, 8, 8), device="cuda")}


@pytest.fixture(scope="module")
def itself(atlas, maps):
    """(i) the knee is the atlas itself, both cartilages."""
    return atlas.measure(maps["FC"], maps["TC"], morphometry=True)


@pytest.fixture(scope="module")
def tc_only(atlas, maps):
    """The TC cap alone in atlas space (no FC cartilage: its error is recorded): the reference of the patient-space tests, computed once."""
    return atlas.measure(maps["none"], maps["TC"], morphometry=True)


def test_the_atlas_measured_against_itself_is_fully_covered(atlas, itself):
    from oai_analysis_2_amd import mesh_processing as mp
    from oai_analysis_2_amd.thickness import morphometry_rows
    assert itself.errors == {} and set(itself.morphometry) == {"FC", "TC"} and itself.space == "atlas"
    for kind, T in (("FC", 5.0 * 0.36), ("TC", T_CAP)):
        rec = itself.morphometry[kind].all
        print(kind, rec)
        assert rec.denuded_mm2 == 0.0 and rec.covered_mm2 == rec.area_mm2 and rec.mean_thickness_total == rec.mean_thickness_covered
        assert rec.n_vertices == rec.n_covered == rec.n_measured == atlas.n_points(kind) and rec.denuded_fraction == 0.0
        assert (rec.kind, rec.region, rec.space, rec.cover) == (kind, "all", "atlas", "footprint")
        # (the inner surface includes the rim wall, where the distance to the outer surface falls to 0: only the maximum is the shell's thickness)
        assert abs(rec.max - T) < 0.15 * T and rec.min <= rec.mean_thickness_covered <= rec.max and rec.min <= rec.vertex_mean <= rec.max and rec.std > 0.0
        cov = itself.coverage[kind]
        assert isinstance(cov, np.ndarray) and cov.dtype == np.uint8 and cov.shape == (atlas.n_points(kind),) and cov.all()
        # the record is the host arithmetic on the restated slots of the knee's own vector, the atlas' vertex areas and the coverage
        va, fa = mp.mesh_areas(atlas.inner[kind])
        assert abs(rec.area_mm2 - fa.sum()) <= len(fa) * np.finfo(np.float64).eps * fa.sum()
        labels, names = atlas.regions[kind]
        want = type(rec).from_slots(kind, "all", mref.region_stats(itself[kind], va, None, cov, 1)[0])
        assert _same_record(rec, want)
        if names:
            rows = mref.region_stats(itself[kind], va, labels, cov, len(names))
            for k, name in enumerate(names):
                assert _same_record(itself.morphometry[kind].regions[name], type(rec).from_slots(kind, name, rows[k]))
    # defaults invent no anatomy: FC is the whole surface only, TC the two sides of project_thickness's own split
    assert list(itself.morphometry["FC"].regions) == [] and list(itself.morphometry["TC"].regions) == ["z_lt_50", "z_ge_50"]
    tc = itself.morphometry["TC"]
    z = atlas.inner["TC"].verts[:, 2]
    assert tc["z_lt_50"].n_vertices == (z < 50).sum() > 0 and tc["z_ge_50"].n_vertices == (z >= 50).sum() > 0
    assert tc["z_lt_50"].n_vertices + tc["z_ge_50"].n_vertices == tc["all"].n_vertices
    rows = morphometry_rows(itself)
    assert [(r["kind"], r["region"]) for r in rows] == [("FC", "all"), ("TC", "all"), ("TC", "z_lt_50"), ("TC", "z_ge_50")]


def test_without_morphometry_nothing_changes(atlas, maps, itself):
    plain = atlas.measure(maps["FC"], maps["TC"])
    assert plain.morphometry == {} and plain.coverage == {} and plain.errors == {}
    assert np.array_equal(_f32bits(plain.fc), _f32bits(itself.fc)) and np.array_equal(_f32bits(plain.tc), _f32bits(itself.tc))
    dev = atlas.measure(maps["FC"], maps["TC"], morphometry=True, keep_on_device=True)
    assert dev.coverage["TC"].is_cuda and dev.coverage["TC"].dtype == torch.uint8 and dev.tc.is_cuda
    assert _same_morphometry(dev.morphometry, itself.morphometry) and np.array_equal(_f32bits(dev.tc), _f32bits(itself.tc))     # and twice the same record
    for bad in (-1.0, "footprint", None):
        with pytest.raises(ValueError):
            atlas.measure(maps["FC"], maps["TC"], morphometry=bad)


def test_a_denuded_cone_against_the_analytic_cap_and_the_error_path(atlas, maps, itself, tc_only):
    """(ii) and (vi): the TC probability zeroed inside a cone of half-angle THETA, and no FC cartilage at all."""
    inner = atlas.inner["TC"].verts.astype(np.float64)
    radii = np.linalg.norm(inner - CENTRE, axis=1)
    R = min((R_MID - T_CAP / 2, R_MID + T_CAP / 2), key=lambda v: abs(v - np.median(radii)))       # whichever sphere the split calls inner
    assert abs(np.median(radii) - R) < 0.5
    analytic = 2 * math.pi * R * R * (1.0 - math.sqrt(1.0 - (RHO / R) ** 2))                       # the sphere of radius R inside the cylinder rho < RHO
    cap = 2 * math.pi * R * R * (1.0 - math.cos(THETA))
    knee = atlas.measure(maps["none"], maps["hole"], morphometry=True)
    rec = knee.morphometry["TC"].all
    mesh_error = abs(itself.morphometry["TC"].all.area_mm2 - analytic) / analytic * cap
    rim_band = 2 * math.pi * R * math.sin(THETA) * (atlas.radius + S)
    print("R", R, "atlas area", itself.morphometry["TC"].all.area_mm2, "analytic", analytic, "denuded", rec.denuded_mm2, "cap", cap,
          "allowance", mesh_error + rim_band, "=", mesh_error, "+", rim_band, rec)
    assert abs(rec.denuded_mm2 - cap) <= mesh_error + rim_band
    assert rec.area_mm2 == itself.morphometry["TC"].all.area_mm2 and rec.covered_mm2 + rec.denuded_mm2 == pytest.approx(rec.area_mm2, rel=1e-15)
    assert 0 < rec.n_covered == rec.n_measured < rec.n_vertices and rec.mean_thickness_total < rec.mean_thickness_covered
    # the uncovered vertices lie in the cone (within the rim band), and the fallback values they carry are now excluded from the means
    cov = knee.coverage["TC"] != 0
    cos_axis = (inner[:, 1] - CENTRE[1]) / radii
    assert (np.arccos(cos_axis[~cov]) <= THETA + (atlas.radius + S) / R).all() and cov.sum() == rec.n_covered
    raw, kept = float(np.mean(knee.tc.astype(np.float64))), float(np.mean(knee.tc[cov].astype(np.float64)))
    assert np.isfinite(knee.tc).all() and abs(rec.vertex_mean - kept) <= len(cov) * np.finfo(np.float64).eps * kept
    assert rec.vertex_mean != raw
    # a coverage distance instead of the footprint: 2.5 mm reaches further into the hole than the radius does
    far = atlas.measure(maps["none"], maps["hole"], morphometry=2.5)
    assert far.morphometry["TC"].all.cover == 2.5 and 0.0 < far.morphometry["TC"].all.denuded_mm2 < rec.denuded_mm2
    assert np.array_equal(_f32bits(far.tc), _f32bits(knee.tc)) and (far.coverage["TC"] >= knee.coverage["TC"]).all()
    # (vi) the cartilage that raised: an errors entry, an all-NaN record with the atlas area; the other one is intact
    assert knee.errors == {"FC": NO_REGION} and np.isnan(knee.fc).all()
    fc = knee.morphometry["FC"].all
    assert fc.area_mm2 == itself.morphometry["FC"].all.area_mm2 and fc.n_vertices == atlas.n_points("FC") and fc.n_covered == fc.n_measured == 0
    assert all(math.isnan(getattr(fc, name)) for name in AREAS[1:] + LENGTHS + ("denuded_fraction",))
    assert not knee.coverage["FC"].any()
    assert tc_only.errors == {"FC": NO_REGION} and _same_morphometry({"TC": tc_only.morphometry["TC"]}, {"TC": itself.morphometry["TC"]})
    assert np.array_equal(_f32bits(tc_only.tc), _f32bits(itself.tc))


def test_patient_space_identity_and_doubled_spacing(atlas, maps, tc_only):
    """(iii) the identity phi on the atlas geometry gives the atlas-space record bit for bit; onto a patient grid of twice the spacing
    every pushed coordinate is exactly doubled, so every area is exactly 4 x and every thickness figure exactly 2 x."""
    shape = tuple(maps["TC"].shape)
    phi = torch.from_numpy(tref.identity_phi(shape)).cuda()
    base = tc_only.morphometry["TC"]
    same = atlas.measure(maps["none"], maps["TC"], phi=phi, image_A=_meta(shape, [S, S, S]), morphometry=True)
    assert same.space == "patient" and same.outside == {"TC": 0}
    for name in ("all", "z_lt_50", "z_ge_50"):
        assert same.morphometry["TC"][name].space == "patient" and _same_record(same.morphometry["TC"][name], base[name], skip=("space",)), name
    assert np.array_equal(same.coverage["TC"], tc_only.coverage["TC"])
    twice = atlas.measure(maps["none"], maps["TC"], phi=phi, image_A=_meta(shape, [2 * S, 2 * S, 2 * S], (5.0, -3.0, 1.0)), morphometry=True)
    for name in ("all", "z_lt_50", "z_ge_50"):
        got, ref = twice.morphometry["TC"][name], base[name]
        print(name, got)
        for f in AREAS:
            assert getattr(got, f) == 4.0 * getattr(ref, f), (name, f)
        for f in LENGTHS:
            assert getattr(got, f) == 2.0 * getattr(ref, f), (name, f)
        assert (got.n_vertices, got.n_covered, got.n_measured, got.denuded_fraction) == (ref.n_vertices, ref.n_covered, ref.n_measured, ref.denuded_fraction)
    # the native space: the same sources up to the point solver's 1e-7 voxels, the weights those of the pushed atlas mesh
    native = atlas.measure(maps["none"], maps["TC"], phi=phi, image_A=_meta(shape, [S, S, S]), space="patient_grid", morphometry=True)
    got = native.morphometry["TC"].all
    assert got.space == "patient_grid" and got.area_mm2 == base.all.area_mm2 and got.n_vertices == base.all.n_vertices
    assert got.mean_thickness_covered == pytest.approx(base.all.mean_thickness_covered, rel=1e-4) and got.denuded_fraction < 0.01


def test_regions_painted_on_the_thickness_image(atlas, maps, itself):
    """(iv) a two-label image split down a column: two regions whose counts add exactly and whose areas add to "all" within rounding."""
    H, W = atlas.image_shape
    img = np.zeros((H, W), np.int32)
    img[:, W // 2:] = 1
    try:
        atlas.regions_from_image("FC", img)
        assert atlas.regions["FC"][1] == ("label_0", "label_1")
        col = np.clip(np.floor((atlas.uv["FC"][:, 0] - atlas.raster["FC"].lo[0]) / atlas.raster["FC"].step[0]), 0, W - 1)
        assert np.array_equal(atlas.regions["FC"][0], (col >= W // 2).astype(np.int32))
        knee = atlas.measure(maps["FC"], maps["none"], morphometry=True)
        fc = knee.morphometry["FC"]
        left, right, whole = fc["label_0"], fc["label_1"], fc["all"]
        print(left, right, whole, sep="\n")
        assert left.n_vertices > 100 and right.n_vertices > 100
        for f in ("n_vertices", "n_covered", "n_measured"):
            assert getattr(left, f) + getattr(right, f) == getattr(whole, f)
        for f in AREAS[:2]:
            assert abs(getattr(left, f) + getattr(right, f) - getattr(whole, f)) <= whole.n_vertices * np.finfo(np.float64).eps * getattr(whole, f)
        assert _same_record(whole, itself.morphometry["FC"].all)                          # the regions do not touch the whole
        assert min(left.min, right.min) == whole.min and max(left.max, right.max) == whole.max
        atlas.set_regions("FC", np.zeros(atlas.n_points("FC"), np.int64), ["everything"])
        assert _same_record(atlas.measure(maps["FC"], maps["none"], morphometry=True).morphometry["FC"]["everything"], whole, skip=("region",))
        with pytest.raises(ValueError):
            atlas.set_regions("FC", np.zeros(3, np.int32), ["a"])
        with pytest.raises(ValueError):
            atlas.regions_from_image("FC", np.zeros((H, W + 1), np.int32))
    finally:
        atlas._set_default_regions("FC")
    assert atlas.regions["FC"][1] == ()


# ---- pass-through --------------------------------------------------------------------------------------------------------------------
def _small_pipe(unet_sd, precision="fp16x3"):
    """tests/test_pipeline_gpu.py::_small_pipe"""
    from oai_analysis_2_amd.pipeline import VolumePipeline
    from oai_analysis_2_amd.registration import IconEngine
    from oai_analysis_2_amd.segmentation.engine import UNetEngine
    shape, net = (24, 72, 72), (40, 48, 48)
    atlas = Image(make_volume(10, shape), [0.4, 0.35, 0.75], [0.0, -1.0, 2.0])
    pipe = VolumePipeline(UNetEngine(unet_sd, precision=precision), IconEngine(make_icon_state_dict(1, last_scale=0.1), net_shape=net), atlas,
                          tile_zyx=(16, 32, 32), overlap_zyx=(4, 8, 8), crop_zyx=(4, 8, 8), batch=8)
    return pipe, shape


def test_pipeline_run_passes_morphometry_through(atlas):
    pipe, shape = _small_pipe(make_unet_state_dict(1, width_div=2))
    vol = make_volume(9, shape)
    meta = Image(vol, [0.36, 0.37, 0.7], [1.0, 2.0, 3.0])
    v = torch.from_numpy(vol).cuda()
    off = pipe.run(v, meta, thickness=atlas)
    assert off.thickness.morphometry == {} and off.thickness.coverage == {}
    on = pipe.run(v, meta, thickness=atlas, morphometry=True)
    direct = atlas.measure(on.fc_atlas, on.tc_atlas, spacing_xyz=pipe.atlas.spacing, morphometry=True)
    assert set(on.thickness.morphometry) == {"FC", "TC"} and _same_morphometry(on.thickness.morphometry, direct.morphometry)
    assert on.thickness.errors == direct.errors == off.thickness.errors
    for kind in ("FC", "TC"):
        assert np.array_equal(on.thickness.coverage[kind], direct.coverage[kind])
        assert np.array_equal(_f32bits(on.thickness[kind]), _f32bits(off.thickness[kind]))
        assert on.thickness.morphometry[kind].all.area_mm2 > 0.0


def test_thickness_stream_yields_the_morphometry_per_knee(atlas, maps, itself):
    from oai_analysis_2_amd.dask_processing import thickness_stream
    from oai_analysis_2_amd.pipeline import VolumeResult
    tiny = torch.zeros(1, device="cuda")
    knees = [(maps["none"], maps["TC"]), (maps["none"], maps["hole"]), (maps["none"], maps["none"])]
    results = [(7 + i, VolumeResult(tiny, tiny, tiny, f, t)) for i, (f, t) in enumerate(knees)]
    direct = [atlas.measure(f, t, morphometry=True) for f, t in knees]
    got = list(thickness_stream(iter(results), atlas, morphometry=True))
    assert [i for i, _ in got] == [7, 8, 9]
    for (_, k), d in zip(got, direct):
        assert _same_morphometry(k.morphometry, d.morphometry) and k.errors == d.errors
        assert all(np.array_equal(k.coverage[kind], d.coverage[kind]) for kind in ("FC", "TC"))
    assert got[0][1].morphometry["TC"].all.denuded_mm2 == 0.0 < got[1][1].morphometry["TC"].all.denuded_mm2
    assert math.isnan(got[2][1].morphometry["TC"].all.mean_thickness_covered) and got[2][1].morphometry["TC"].all.area_mm2 == itself.morphometry["TC"].all.area_mm2
    plain = list(thickness_stream(iter(results[:1]), atlas))
    assert plain[0][1].morphometry == {} and np.array_equal(_f32bits(plain[0][1].tc), _f32bits(got[0][1].tc))
    dev = list(thickness_stream(iter(results[:1]), atlas, keep_on_device=True, results_complete=True, morphometry=True))
    torch.cuda.synchronize()
    assert dev[0][1].coverage["TC"].is_cuda and _same_morphometry(dev[0][1].morphometry, direct[0].morphometry)
