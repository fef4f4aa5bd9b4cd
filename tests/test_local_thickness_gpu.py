"""GPU: thickness QC (csrc/local_thickness.hip; ops.local_thickness / masked_stats; qc.local_thickness, local_thicknesses;
VolumePipeline.run(thickness_qc=), dask_processing.thickness_qc_stream) -- the squared radii bit for bit against the restatements of
tests/local_thickness_ref.py (the brute force over all pairs on the small shapes, the loop over offsets on the large ones), the float32
thickness to one step, the counts exactly, the statistics bit for bit against the restated order of csrc/ordered_reduce.h and
np.percentile, and the record through every layer."""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

import edt_ref as er
import local_thickness_ref as lt
from oai_analysis_2_amd import ops, qc
from oai_analysis_2_amd.image import Image

pytestmark = pytest.mark.gpu

SHAPES_BRUTE = er.SHAPES_SMALL + lt.EXTRA_SHAPES
LARGE = (40, 96, 96)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _one_step(got32, want32):
    """Float32 maps equal, or one float32 step apart (the rule of tests/test_edt_gpu.py); zeros exactly.  Returns the number of voxels
    that differ."""
    got32, want32 = np.asarray(got32), np.asarray(want32)
    assert got32.dtype == want32.dtype == np.float32 and got32.shape == want32.shape
    assert np.isfinite(got32).all() and not np.signbit(got32).any() and np.array_equal(got32 == 0, want32 == 0)
    steps = np.abs(got32.view(np.int32).astype(np.int64) - want32.view(np.int32).astype(np.int64))
    assert steps.max(initial=0) <= 1
    return int((steps != 0).sum())


def _check(field, spacing, want_sq, label, cap=None, want_capped=0):
    """One field against its restated squared radii: sq_out to the bit, thick to one step, the counts, and the same maps without the
    optional outputs.  Returns the four counts."""
    kw = {} if cap is None else dict(max_window_voxels=cap)
    thick, sq, stats = ops.local_thickness(dev(field), spacing, return_squared=True, return_stats=True, **kw)
    assert thick.dtype == torch.float32 and sq.dtype == torch.float64 and stats.dtype == torch.int64 and tuple(thick.shape) == field.shape
    sq, t, stats = sq.cpu().numpy(), thick.cpu().numpy(), [int(v) for v in stats.cpu().numpy()]
    assert np.array_equal(_bits(sq), _bits(want_sq)), label
    differ = _one_step(t, lt.thickness32(want_sq))
    print(label, "stats", stats, "float32 thicknesses that differ from 2 float32(sqrt(sq))", differ, "(expected 0)")
    assert stats[0] == int(lt.centres(field).sum()) and stats[2] == want_capped, label
    assert stats[3] == int(lt.windows(field, spacing).max(initial=0)), label
    alone = ops.local_thickness(dev(field), spacing, **kw)                       # without sq_out_dev and stats_dev
    assert np.array_equal(_bits(alone.cpu().numpy()), _bits(t)), label
    return stats


@functools.lru_cache(maxsize=None)
def _small_case(shape, spacing, kind):
    field = (lt.edt_field if kind == "edt" else lt.generic_field)(shape, spacing, 11)
    want = lt.sq_brute(field, spacing)
    field.setflags(write=False)
    want.setflags(write=False)
    return field, want


@pytest.mark.parametrize("spacing", er.SPACINGS)
@pytest.mark.parametrize("shape", SHAPES_BRUTE)
def test_squared_radii_are_the_brute_force_maximum_bit_for_bit(shape, spacing):
    for kind in ("edt", "generic"):
        field, want = _small_case(shape, spacing, kind)
        _check(field, spacing, want, (shape, spacing, kind))


def _mask_field(m, spacing):
    return er.edt_sq_lines(~er.in_set(m), spacing)


@functools.lru_cache(maxsize=None)
def _window_case(name, spacing):
    m = er.box((20, 20, 20), (2, 2, 2), (16, 16, 16)) if name == "box" else lt.ball((24, 24, 24), 9.0)
    field = _mask_field(m, spacing)
    return field, lt.sq_offsets(field, spacing)


@pytest.mark.parametrize("spacing", (er.SPACINGS[0], lt.DESS))
@pytest.mark.parametrize("name", ("box", "ball"))
def test_large_windows(name, spacing):
    """Windows of many hundred voxels: every lane group walks its window through many steps, rows and slices."""
    field, want = _window_case(name, spacing)
    stats = _check(field, spacing, want, (name, spacing))
    assert stats[3] >= 9 ** 3 and stats[1] == int(lt.windows(field, spacing).sum())


@pytest.mark.parametrize("spacing", er.SPACINGS)
def test_blobs_at_forty_by_ninety_six_squared(spacing):
    field = lt.edt_field(LARGE, spacing, 5)
    stats = _check(field, spacing, lt.sq_offsets(field, spacing), (LARGE, spacing))
    low, high = int(lt.windows(field, spacing).sum()), int(lt.windows(field, spacing, extra=1).sum())
    print("voxel tests", stats[1], "between", low, "and", high)
    assert stats[0] > 10000 and low <= stats[1] <= high


def test_degenerate_fields():
    spacing = lt.DESS
    for shape in ((1, 1, 1), (4, 5, 6)):
        for fill in (0.0, np.inf, np.nan, -2.0):
            assert _check(np.full(shape, fill), spacing, np.zeros(shape), (shape, fill))[:3] == [0, 0, 0]
    one = np.zeros((4, 5, 6))
    one[2, 3, 1] = 50.0                                            # a single centre: it covers itself, and nothing else is a centre
    stats = _check(one, spacing, one, "single centre")
    assert stats[0] == 1 and stats[1] == stats[3] == 4 * 5 * 6     # its ball holds the whole volume
    for shape in ((1, 1, 50), (1, 50, 1), (50, 1, 1)):             # a volume that is one line
        field = lt.generic_field(shape, spacing, 4)
        _check(field, spacing, lt.sq_brute(field, spacing), shape)
    line = np.zeros((1, 1, 50), np.float32)
    line[0, 0, 10:31] = 1.0                                        # 21 voxels in a row: the middle one reaches 11 voxels, strictly 10
    field = _mask_field(line, (1.0, 1.0, 1.0))
    want = lt.sq_brute(field, (1.0, 1.0, 1.0))
    assert want[0, 0, 20] == 121.0 and want[0, 0, 10] == 121.0 and want[0, 0, 9] == 0.0
    _check(field, (1.0, 1.0, 1.0), want, "run of 21")


def test_cap_rule():
    """A centre whose clipped window is above the cap covers itself only and is counted; at the default cap none is (every other
    test asserts stats[2] == 0)."""
    spacing = er.SPACINGS[0]
    field, free = _window_case("box", spacing)
    n_capped = int(lt.capped(field, spacing, 27).sum())
    want = lt.sq_offsets(field, spacing, 27)
    assert n_capped > 0 and (want < free).any()
    stats = _check(field, spacing, want, "cap 27", cap=27, want_capped=n_capped)
    vol = lt.windows(field, spacing)
    assert stats[1] == int(vol[vol <= 27].sum()) + n_capped        # a capped centre costs its own voxel
    at = int(vol.max())
    _check(field, spacing, free, "cap at the largest window", cap=at)
    _check(field, spacing, lt.sq_offsets(field, spacing, at - 1), "cap one below", cap=at - 1, want_capped=int((vol > at - 1).sum()))
    with pytest.raises(Exception):
        ops.local_thickness(dev(field), spacing, max_window_voxels=0)


def test_order_independence():
    """The atomics are integer maxima: the same bits on every run and on a side stream, beside other work."""
    field = dev(lt.edt_field(LARGE, lt.DESS, 5))
    first = ops.local_thickness(field, lt.DESS, return_squared=True, return_stats=True)
    again = ops.local_thickness(field, lt.DESS, return_squared=True, return_stats=True)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = ops.local_thickness(field, lt.DESS, return_squared=True, return_stats=True)
    torch.cuda.synchronize()
    for got in (again, other):
        assert all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
                   for a, b in zip(got, first))


# ---- oai_masked_stats --------------------------------------------------------------------------------------------------------------------
def _stats_case(n, seed=7):
    rng = np.random.default_rng([seed, n])
    v = (np.exp(rng.uniform(-20.0, 20.0, size=n)) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)      # sums on which the order shows
    mask = (rng.uniform(size=n) < 0.6).astype(np.uint8)
    mask[0] = 1
    return v, mask


def _same_stats(got, want, label):
    got = got.cpu().numpy()
    print(label, got.tolist())
    assert np.array_equal(np.isnan(got), np.isnan(want)), label
    ok = ~np.isnan(want)
    assert np.array_equal(_bits(got[ok]), _bits(want[ok])), (label, got, want)


# one element; two; partial waves; more than one block; more than 256 slots (the finish takes runs of two); the grid-stride cap
@pytest.mark.parametrize("n", (1, 2, 63, 65, 1025, 1024 * 257 + 3, 2048 * 1024 + 5))
def test_masked_stats_to_the_bit(n):
    v, mask = _stats_case(n)
    for pct in ((0.0, 50.0), (95.0, 100.0)):
        _same_stats(ops.masked_stats(dev(v), dev(mask), pct), lt.masked_stats(v, mask, pct), (n, pct, "mask"))
        _same_stats(ops.masked_stats(dev(v), None, pct), lt.masked_stats(v, None, pct), (n, pct, "null mask"))
    _same_stats(ops.masked_stats(dev(v), dev(mask != 0), (50.0,)), lt.masked_stats(v, mask, (50.0,)), (n, "bool mask, one percentile"))
    _same_stats(ops.masked_stats(dev(v), dev(mask), ()), lt.masked_stats(v, mask, ()), (n, "no percentile"))


def test_masked_stats_empty_and_non_finite():
    v, mask = _stats_case(5000)
    got = ops.masked_stats(dev(v), dev(np.zeros_like(mask))).cpu().numpy()
    assert got[0] == 0 and got[7] == 0 and np.isnan(got[1:7]).all()
    v[[3, 40, 41, 4999]] = np.nan, np.inf, -np.inf, np.nan
    mask[[3, 40, 4999]] = 1
    mask[41] = 0
    want = lt.masked_stats(v, mask)
    assert want[7] == 3 and want[0] == int(((mask != 0) & np.isfinite(v)).sum())
    _same_stats(ops.masked_stats(dev(v), dev(mask)), want, "non-finite under the mask")
    only_bad = np.zeros_like(mask)
    only_bad[[3, 40]] = 1
    got = ops.masked_stats(dev(v), dev(only_bad)).cpu().numpy()
    assert got[0] == 0 and got[7] == 2 and np.isnan(got[1:7]).all()
    got = ops.masked_stats(torch.empty(0, dtype=torch.float32, device="cuda")).cpu().numpy()
    assert got[0] == 0 and got[7] == 0 and np.isnan(got[1:7]).all()
    with pytest.raises(ValueError):
        ops.masked_stats(dev(v), dev(mask), (5.0, 50.0, 95.0))
    with pytest.raises(ValueError):
        ops.masked_stats(dev(v), dev(mask[:-1]))


# ---- through the layers ------------------------------------------------------------------------------------------------------------------
def _by_hand(vol, spacing, radius="voxel", threshold=0.5, cap=ops.MAX_WINDOW_VOXELS, mm3=True):
    """The record assembled from ops.* calls, each downloaded on its own."""
    if radius == "voxel":
        rsq = ops.distance_transform(ops.mask_surface(vol, threshold, "complement"), spacing, return_squared=True)[1]
    else:
        from oai_analysis_2_amd.mesh_processing import _point_distance_dev, mesh_grid_params_device
        idx, pts, verts, faces = qc.mesh_radius_points(vol, spacing, threshold)
        d = _point_distance_dev(pts, verts, faces, mesh_grid_params_device(verts, faces)).to(torch.float64)
        rsq = torch.zeros(tuple(vol.shape), dtype=torch.float64, device=vol.device)
        rsq[idx[:, 0], idx[:, 1], idx[:, 2]] = d * d
    thick, stats = ops.local_thickness(rsq, spacing, cap, return_stats=True)
    over_set = ops.masked_stats(thick, ops.mask_surface(vol, threshold, "set"), (50.0, 95.0)).cpu().numpy()
    over_surface = ops.masked_stats(thick, ops.mask_surface(vol, threshold, "surface"), (50.0,)).cpu().numpy()
    return qc.thickness_from_stats(stats.cpu().numpy(), over_set, over_surface, radius,
                                   float(np.prod(np.asarray(spacing, np.float64))) if mm3 else None), thick


def _same_record(a, b):
    a, b = dataclasses.asdict(a), dataclasses.asdict(b)
    a.pop("thickness_map"), b.pop("thickness_map")
    return set(a) == set(b) and all((a[k] == b[k]) or (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) for k in a)


def test_record_equals_the_one_assembled_by_hand(monkeypatch):
    spacing = lt.DESS
    v = er.blobs((12, 20, 24), 11, (4, 6, 8))
    want, thick = _by_hand(dev(v), spacing)
    assert want.voxels == int(er.in_set(v).sum()) and want.capped_centres == 0 and want.work > want.voxels and want.radius == "voxel"
    assert 0 < want.median <= want.p95 <= want.max and want.std > 0 and 0 < want.surface_median <= want.max
    for form in (Image(v, spacing), dev(v)):
        got = qc.local_thickness(form, spacing_xyz=None if isinstance(form, Image) else spacing, return_map=True)
        print(got)
        assert _same_record(got, want) and torch.equal(got.thickness_map, thick)
    assert qc.local_thickness(Image(v, spacing)).thickness_map is None
    # the figures against numpy on the downloaded map
    t = thick.cpu().numpy()[er.in_set(v)]
    assert want.max == float(t.max()) and want.median == float(np.percentile(t, 50.0)) and want.p95 == float(np.percentile(t, 95.0))
    assert math.isclose(want.mean, float(t.astype(np.float64).mean()), rel_tol=1e-12)
    assert math.isclose(want.std, float(t.astype(np.float64).std()), rel_tol=1e-9)
    s = thick.cpu().numpy()[er.surface_ref(v) != 0]
    assert math.isclose(want.surface_mean, float(s.astype(np.float64).mean()), rel_tol=1e-12) and want.surface_median == float(np.percentile(s, 50.0))
    bare = qc.local_thickness(dev(v))                                           # a tensor without a spacing: unit, and no volume
    assert bare.mm3 is None and _same_record(bare, _by_hand(dev(v), (1.0, 1.0, 1.0), mm3=False)[0])
    # two maps: one buffer, one download
    calls = []
    slots = qc._result_slots

    def counted(device, layout):
        views, download = slots(device, layout)
        calls.append(0)

        def once():
            calls[-1] += 1
            return download()
        return views, once
    monkeypatch.setattr(qc, "_result_slots", counted)
    w = er.blobs((12, 20, 24), 12)
    both = qc.local_thicknesses({"a": dev(v), "b": dev(w)}, spacing)
    assert calls == [1]
    assert _same_record(both["a"], want) and _same_record(both["b"], _by_hand(dev(w), spacing)[0])
    monkeypatch.undo()
    with pytest.raises(ValueError):
        qc.local_thickness(dev(v), radius="ball")
    with pytest.raises(ValueError):
        qc.local_thickness(dev(v), max_window_voxels=0)


def test_sets_without_a_centre():
    for fill in (0.0, 1.0):                                        # an empty set; a set that fills the volume (EDT = +inf)
        rec = qc.local_thickness(dev(np.full((5, 6, 7), fill, np.float32)), (1.0, 1.0, 1.0), return_map=True)
        assert rec.voxels == (210 if fill else 0) and rec.mm3 == rec.voxels and rec.work == 0 and rec.capped_centres == 0
        assert all(math.isnan(getattr(rec, k)) for k in ("mean", "std", "median", "p95", "max", "surface_mean", "surface_median"))
        assert not rec.thickness_map.any()


@pytest.mark.parametrize("spacing", er.SPACINGS)
def test_slab_law_through_the_record(spacing):
    for t in range(1, 7):
        rec = qc.local_thickness(dev(lt.slab((t + 4, 9, 10), t)), spacing)
        want = float(np.float32(2.0) * np.float32(np.sqrt((np.float64(math.ceil(t / 2)) * np.float64(spacing[2])) ** 2)))
        print(t, spacing, rec.mean, want)
        assert rec.voxels == t * 90 and rec.max == rec.median == rec.p95 == rec.surface_median == want and rec.std == 0.0
        assert math.isclose(rec.mean, want, rel_tol=1e-15) and math.isclose(rec.surface_mean, want, rel_tol=1e-15)


def test_mesh_radius():
    spacing = lt.DESS
    v = er.blobs((12, 20, 24), 11, (4, 6, 8))
    want, thick = _by_hand(dev(v), spacing, radius="mesh")
    got = qc.local_thickness(dev(v), spacing, radius="mesh", return_map=True)
    print(got)
    assert _same_record(got, want) and torch.equal(got.thickness_map, thick) and got.radius == "mesh" and got.voxels == int(er.in_set(v).sum())
    print("mean with the mesh radius", got.mean, "with the voxel radius", qc.local_thickness(dev(v), spacing).mean)
    assert 0 < got.mean <= got.max
    # two parallel planes T apart, normal to z and between voxel layers; the map ramps linearly through 0.5 across each, where marching
    # cubes is exact.  Every voxel centre of the set is min(z - a, b - z) from the surface, the layer nearest the medial plane at most
    # s_z / 2 off it: max lies in [T - s_z, T], up to the float32 arithmetic of the map, the vertices and the distances (1e-6 relative
    # each, far inside the 1e-4 T the interval is widened by).
    sz = spacing[2]
    a, b, slope = 1.9, 5.15, 0.4
    z = np.arange(12) * sz
    ramp = (0.5 + slope * np.minimum(z - a, b - z)).astype(np.float32)
    m = np.broadcast_to(ramp[:, None, None], (12, 16, 16)).copy()
    rec = qc.local_thickness(dev(m), spacing, radius="mesh", return_map=True)
    T = b - a
    print("planes", T, "apart: max", rec.max, "mean", rec.mean, "voxel radius", qc.local_thickness(dev(m), spacing).max)
    assert rec.voxels == int((ramp > 0.5).sum()) * 256 and rec.capped_centres == 0
    assert T - sz - 1e-4 * T <= rec.max <= T + 1e-4 * T
    assert float(rec.thickness_map.max()) == rec.max and rec.median <= rec.max


def _same_records(a, b):
    return set(a) == set(b) == {"FC", "TC"} and all(_same_record(a[k], b[k]) for k in a)


def test_pipeline_run_with_thickness_qc_changes_no_bit():
    """The smallest pipeline the QC tests use (tests/test_registration_qc_gpu.py::_small_pipe), built here."""
    from oai_analysis_2_amd.dask_processing import thickness_qc_stream
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
    base, on = pipe.run(v, meta), pipe.run(v, meta, thickness_qc=True)
    for name in ("fc", "tc", "phi", "fc_atlas", "tc_atlas"):
        assert torch.equal(getattr(on, name), getattr(base, name)), name
    assert base.thickness_qc is None and pipe.run(v, meta, thickness_qc=False).thickness_qc is None
    assert VolumeResult.thickness_qc is None and "thickness_qc" not in [f.name for f in dataclasses.fields(VolumeResult)]
    alone = {kind: qc.local_thickness(getattr(on, kind.lower()), spacing_xyz=meta.spacing) for kind in ("FC", "TC")}
    print(on.thickness_qc)
    assert _same_records(on.thickness_qc, alone) and all(r.radius == "voxel" for r in on.thickness_qc.values())
    mesh = pipe.run(v, meta, thickness_qc="mesh").thickness_qc
    assert _same_records(mesh, {kind: qc.local_thickness(getattr(on, kind.lower()), spacing_xyz=meta.spacing, radius="mesh") for kind in ("FC", "TC")})
    out = list(thickness_qc_stream(iter([(7, on), (3, base)])))
    assert [i for i, _ in out] == [7, 3] and all(_same_records(rec, on.thickness_qc) for _, rec in out)
    assert all(_same_records(rec, mesh) for _, rec in thickness_qc_stream(iter([(0, on)]), radius="mesh"))
    with pytest.raises(ValueError):
        pipe.run(v, meta, thickness_qc="ball")
