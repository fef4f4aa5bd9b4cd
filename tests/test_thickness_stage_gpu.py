"""GPU: the per-knee thickness stage (oai_analysis_2_amd/thickness.py) -- ThicknessAtlas.measure against the chain of public functions
it replaces, bit for bit; the atlas raster on a two-plateau tibial mesh; the per-cartilage error path; VolumePipeline.run(thickness=)
and the cohort's thickness_stream / process_cohort_thickness."""
import json
import os
import threading

import numpy as np
import pytest
import torch

from oai_analysis_2_amd.image import Image
from oai_analysis_2_amd.synth import make_icon_state_dict, make_unet_state_dict, make_volume

pytestmark = pytest.mark.gpu

_sig = lambda t: 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))
T_BOWL, T_SLAB = 6.0, 5.0 * 0.36                       # shell thickness: 6 voxels of 1 mm; 5 voxels of 0.36 mm
MIN_CELLS = {"FC": 3000, "TC": 100}
NO_REGION = "n_samples=0 should be >= n_clusters=2."


def _bowl(shift_x=0.0, T=T_BOWL):
    """test_thickness_map_gpu.py::_bowl: a cap of a spherical shell of thickness T (TC-sized), optionally shifted along x."""
    D, H, W = 48, 96, 96
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    x = x - shift_x
    r = np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4 + (y + 30) ** 2)
    prob = _sig(2.0 * (np.abs(r - 60.0) - T / 2)) * _sig(2.0 * (np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4) - 30))
    return Image(prob.astype(np.float32), [1.0, 1.0, 1.0])


def _slab(shift_x=0.0):
    """test_mesh_graph_gpu.py::_slab (scripts/bench_mesh.py's femoral-cartilage-like slab at half size), optionally shifted along x."""
    D, H, W = 80, 192, 192
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    x = x - shift_x
    R, T = 110.0, 5.0
    r = np.sqrt((x - 96) ** 2 + ((z - 40) * 1.9) ** 2 + (y + 30) ** 2)
    prob = _sig(2.0 * (np.abs(r - R) - T / 2)) * _sig(2.0 * (np.sqrt((x - 96) ** 2 + ((z - 40) * 1.9) ** 2) - 70))
    return Image(prob.astype(np.float32), [0.36, 0.36, 0.7])


def _two_caps():
    """A tibial map with two plateaus: two caps of a shell of thickness 6, centred at z = 25 and z = 75 (spacing 1: one each side of 50)."""
    D, H, W = 100, 64, 64
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    prob = np.zeros((D, H, W), np.float32)
    for zc in (25.0, 75.0):
        r = np.sqrt((x - 32) ** 2 + (z - zc) ** 2 + (y + 30) ** 2)
        prob = np.maximum(prob, _sig(2.0 * (np.abs(r - 60.0) - 3.0)) * _sig(2.0 * (np.sqrt((x - 32) ** 2 + (z - zc) ** 2) - 20)))
    return Image(prob.astype(np.float32), [1.0, 1.0, 1.0])


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


def _same_knee(a, b):
    return np.array_equal(_bits(a.fc), _bits(b.fc)) and np.array_equal(_bits(a.tc), _bits(b.tc)) and a.errors == b.errors


@pytest.fixture(scope="module")
def knee():
    return {"FC": _slab(0.0), "TC": _bowl(0.0)}


@pytest.fixture(scope="module")
def atlas():
    from oai_analysis_2_amd.thickness import ThicknessAtlas
    return ThicknessAtlas(_slab(1.5), _bowl(1.5), image_shape=(96, 128), min_cells=MIN_CELLS)


def test_measure_equals_the_chain_of_public_functions(atlas, knee):
    from oai_analysis_2_amd import mesh_processing as mp
    # the atlas inner meshes are what the public resident path gives for the atlas maps
    for kind, img in (("FC", _slab(1.5)), ("TC", _bowl(1.5))):
        ref_inner, _ = mp.get_thickness_mesh(img, kind, min_cells=MIN_CELLS[kind], on_device=True)
        assert np.array_equal(atlas.inner[kind].verts, ref_inner.verts) and np.array_equal(atlas.inner[kind].faces, ref_inner.faces)
        assert atlas.inner[kind].GetNumberOfCells() > 500
    fc_t, tc_t = (torch.from_numpy(knee[k].array).cuda() for k in ("FC", "TC"))
    got = atlas.measure(fc_t, tc_t)
    assert got.errors == {} and got.fc.dtype == got.tc.dtype == np.float32
    assert got.fc.shape == (atlas.n_points("FC"),) and got.tc.shape == (atlas.n_points("TC"),)
    for kind, t, vec, T in (("FC", fc_t, got.fc, T_SLAB), ("TC", tc_t, got.tc, T_BOWL)):
        src, _ = mp.get_thickness_mesh(Image(t.cpu().numpy(), knee[kind].spacing), kind, min_cells=MIN_CELLS[kind], on_device=True)
        ref = mp.map_attributes(src, atlas.inner[kind]).point_data["Distance"]
        print(kind, "points", len(vec), "median", float(np.median(vec)), "known", T, "differing", int((_bits(vec) != _bits(ref)).sum()))
        assert np.array_equal(_bits(vec), _bits(ref)), kind                          # the contract: bit for bit, no tolerance
        assert np.isfinite(vec).all()
        assert abs(np.median(vec) - T) < 0.15 * T, (kind, np.median(vec))
    again = atlas.measure(fc_t, tc_t)
    assert _same_knee(again, got)                                                     # twice in a row: the same bits
    dev = atlas.measure(fc_t, tc_t, keep_on_device=True)
    assert dev.fc.is_cuda and dev.tc.is_cuda and _same_knee(dev, got)
    # explicit spacing = the map's own: the same; the image of the knee is finite wherever a face owns the pixel
    assert np.array_equal(_bits(atlas.measure(fc_t, tc_t, spacing_xyz=knee["FC"].spacing).fc), _bits(got.fc))
    img = atlas.image(got.fc, "FC")
    own = atlas.raster["FC"].owner.cpu().numpy()
    assert img.shape == (96, 128) and img.dtype == np.float32 and np.array_equal(np.isnan(img), own < 0)
    assert atlas.raster["FC"].n_covered == (own >= 0).sum() > 0.25 * own.size
    assert abs(np.nanmedian(img) - T_SLAB) < 0.15 * T_SLAB
    x, y = atlas.scatter("FC")
    ref_x, ref_y, _ = mp.project_thickness(mp.map_attributes(src_fc(atlas, knee), atlas.inner["FC"]), "FC")
    assert np.array_equal(x, ref_x) and np.array_equal(y, ref_y)                      # the notebook's scatter coordinates, computed once
    from oai_analysis_2_amd.thickness import wrap_angle
    assert np.array_equal(atlas.uv["FC"][:, 0], wrap_angle(x - atlas.cut)) and np.array_equal(atlas.uv["FC"][:, 1], y)
    # this tibial atlas lies on one side of z = 50: project_thickness has no TC projection for it; measure is not affected
    assert "TC" in atlas.projection_errors and "plateau" in atlas.projection_errors["TC"]
    with pytest.raises(ValueError):
        atlas.image(got.tc, "TC")


def src_fc(atlas, knee):
    from oai_analysis_2_amd import mesh_processing as mp
    return mp.get_thickness_mesh(knee["FC"], "FC", min_cells=MIN_CELLS["FC"], on_device=True)[0]


def test_two_plateau_tibial_atlas_projection_and_image():
    from oai_analysis_2_amd import mesh_processing as mp
    from oai_analysis_2_amd.thickness import ThicknessAtlas, tc_face_skip
    caps = _two_caps()
    at = ThicknessAtlas(_slab(0.0), caps, image_shape=(128, 96), min_cells=MIN_CELLS)
    mesh = at.inner["TC"]
    z = mesh.verts[:, 2]
    assert (z >= 50).sum() > 300 and (z < 50).sum() > 300                              # both plateaus are there
    assert at.projection_errors == {}
    x, y = at.scatter("TC")
    ref_x, ref_y, ref_t = mp.project_thickness(mp.Mesh(mesh.verts, mesh.faces, {"anything": np.arange(len(z), dtype=np.float32)}), "TC")
    assert np.array_equal(x, ref_x) and np.array_equal(y, ref_y)
    order = np.concatenate([np.where(z >= 50)[0], np.where(z < 50)[0]])                # the documented permutation
    assert np.array_equal(at.point_order["TC"], order) and np.array_equal(ref_t, order.astype(np.float64))
    assert np.array_equal(at.uv["TC"][order, 0], x) and np.array_equal(at.uv["TC"][order, 1], y)   # vertex i of the mesh owns uv[i]
    # the image: two covered regions, one per plateau, that do not touch; no face bridges them
    r = at.raster["TC"]
    owner = r.owner.cpu().numpy()
    side = (z >= 50)[mesh.faces]                                                      # [m,3]
    bridging = tc_face_skip(z, mesh.faces)
    assert np.array_equal(bridging, ~(side.all(axis=1) | (~side).all(axis=1)))
    assert not np.isin(owner[owner >= 0], np.nonzero(bridging)[0]).any()
    right = np.zeros(owner.shape, bool); left = np.zeros(owner.shape, bool)
    right[owner >= 0] = side[owner[owner >= 0], 0]
    left[owner >= 0] = ~side[owner[owner >= 0], 0]
    print("pixels right", int(right.sum()), "left", int(left.sum()), "of", owner.size, "bridging faces", int(bridging.sum()))
    assert right.sum() > 200 and left.sum() > 200
    grown = np.zeros_like(right)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            grown[max(dj, 0):owner.shape[0] + min(dj, 0), max(di, 0):owner.shape[1] + min(di, 0)] |= \
                right[max(-dj, 0):owner.shape[0] + min(-dj, 0), max(-di, 0):owner.shape[1] + min(-di, 0)]
    assert not (grown & left).any()                                                   # not even diagonal neighbours
    # a face made to bridge the plateaus is marked, and owns nothing once marked
    faces2 = np.concatenate([mesh.faces, [[np.where(z >= 50)[0][0], np.where(z < 50)[0][0], np.where(z < 50)[0][1]]]]).astype(np.int32)
    skip2 = tc_face_skip(z, faces2)
    assert skip2[-1] and skip2.sum() == bridging.sum() + 1
    r2 = mp.thickness_image_build(at.uv["TC"], faces2, skip2, (128, 96))
    assert torch.equal(r2.owner, r.owner)
    r3 = mp.thickness_image_build(at.uv["TC"], faces2, None, (128, 96))
    assert (r3.owner == len(faces2) - 1).any()                                        # unmarked it would paint across the gap
    # the knee's image through this atlas: thickness 6 on both plateaus
    knee = at.measure(torch.from_numpy(_slab(0.0).array).cuda(), torch.from_numpy(caps.array).cuda())
    assert knee.errors == {}
    img = at.image(knee)["TC"]
    assert np.array_equal(np.isnan(img), owner < 0)
    for region in (right, left):
        assert abs(np.median(img[region]) - 6.0) < 0.15 * 6.0, np.median(img[region])


def test_one_bad_cartilage_does_not_take_the_other_with_it(atlas, knee):
    from oai_analysis_2_amd import mesh_processing as mp
    fc_t, tc_t = (torch.from_numpy(knee[k].array).cuda() for k in ("FC", "TC"))
    good = atlas.measure(fc_t, tc_t)
    with pytest.raises(ValueError) as e:
        mp.get_thickness_mesh(Image(np.zeros_like(knee["FC"].array), knee["FC"].spacing), "FC", on_device=True)
    assert str(e.value) == NO_REGION
    bad = atlas.measure(torch.zeros_like(fc_t), tc_t)
    assert bad.errors == {"FC": str(e.value)}
    assert bad.fc.shape == good.fc.shape and np.isnan(bad.fc).all() and np.array_equal(_bits(bad.tc), _bits(good.tc))
    both = atlas.measure(torch.zeros_like(fc_t), torch.zeros_like(tc_t), keep_on_device=True)
    assert sorted(both.errors) == ["FC", "TC"] and torch.isnan(both.fc).all() and torch.isnan(both.tc).all()
    assert np.isnan(atlas.image(bad.fc, "FC")).all()                                   # NaN vertices give a NaN image


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


_FIVE = ("fc", "tc", "phi", "fc_atlas", "tc_atlas")


def _check_knee_of_maps(atlas, knee_t, res, spacing=None):
    """Per cartilage a finite vector or a recorded error, and equal to a direct measure on the volume's maps."""
    direct = atlas.measure(res.fc_atlas.cuda(), res.tc_atlas.cuda(), spacing_xyz=spacing)
    assert _same_knee(knee_t, direct)
    for kind in ("FC", "TC"):
        vec = knee_t[kind]
        vec = vec.cpu().numpy() if isinstance(vec, torch.Tensor) else vec
        assert (kind in knee_t.errors and np.isnan(vec).all()) or (kind not in knee_t.errors and np.isfinite(vec).all())


def test_pipeline_run_with_and_without_the_thickness_stage(atlas):
    pipe, shape = _small_pipe(make_unet_state_dict(1, width_div=2))
    vol = make_volume(9, shape)
    meta = Image(vol, [0.36, 0.37, 0.7], [1.0, 2.0, 3.0])
    v = torch.from_numpy(vol).cuda()
    base = pipe.run(v, meta)
    off = pipe.run(v, meta, thickness=None)
    assert off.thickness is None and base.thickness is None
    on = pipe.run(v, meta, thickness=atlas)
    for name in _FIVE:
        assert torch.equal(getattr(off, name), getattr(base, name)) and torch.equal(getattr(on, name), getattr(base, name)), name
    from oai_analysis_2_amd.thickness import KneeThickness
    assert isinstance(on.thickness, KneeThickness)
    _check_knee_of_maps(atlas, on.thickness, on, pipe.atlas.spacing)


def _threads():
    return [t.name for t in threading.enumerate() if t.name.startswith("oai-thickness")]


def test_thickness_stream_over_hand_made_results(atlas, knee):
    from oai_analysis_2_amd.dask_processing import thickness_stream
    from oai_analysis_2_amd.pipeline import VolumeResult
    fc_t, tc_t = (torch.from_numpy(knee[k].array).cuda() for k in ("FC", "TC"))
    tc_other = torch.from_numpy(_bowl(0.7).array).cuda()
    tiny = torch.zeros(1, device="cuda")
    maps = [(fc_t, tc_t), (fc_t, tc_other), (torch.zeros_like(fc_t), torch.zeros_like(tc_t)), (fc_t, tc_t), (torch.zeros_like(fc_t), tc_other)]
    results = [(10 + i, VolumeResult(tiny, tiny, tiny, f, t)) for i, (f, t) in enumerate(maps)]
    direct = [atlas.measure(f, t) for f, t in maps]
    assert not np.array_equal(_bits(direct[0].tc), _bits(direct[1].tc))                # the knees differ
    got = list(thickness_stream(iter(results), atlas))
    assert [i for i, _ in got] == [10, 11, 12, 13, 14]                                 # input order
    for (_, k), d in zip(got, direct):
        assert _same_knee(k, d)
    assert got[2][1].errors == {"FC": NO_REGION, "TC": NO_REGION} and got[4][1].errors == {"FC": NO_REGION} and got[0][1].errors == {}
    assert _threads() == []                                                           # the worker is gone
    dev = list(thickness_stream(iter(results), atlas, keep_on_device=True, results_complete=True))
    torch.cuda.synchronize()
    assert all(k.fc.is_cuda for _, k in dev) and all(_same_knee(k, d) for (_, k), d in zip(dev, direct))
    gen = thickness_stream(iter(results), atlas)                                       # closed early: the worker goes as well
    assert next(gen)[0] == 10 and _threads() != []
    gen.close()
    assert _threads() == []
    assert list(thickness_stream(iter([]), atlas)) == [] and _threads() == []


def test_thickness_stream_behind_a_cohort_runner(atlas):
    from oai_analysis_2_amd.cohort import CohortRunner
    from oai_analysis_2_amd.dask_processing import thickness_stream
    pipe, shape = _small_pipe(make_unet_state_dict(1, width_div=2))
    vols = [Image(make_volume(20 + i, shape), [0.36, 0.37, 0.7], [1.0, 2.0, 3.0]) for i in range(3)]
    kept = {}

    def tap(it):
        for i, r in it:
            kept[i] = r
            yield i, r

    got = dict(thickness_stream(tap(CohortRunner(pipe, keep_on_device=True).run(vols)), atlas, results_complete=True))
    assert set(got) == {0, 1, 2} and _threads() == []
    for i in range(3):
        _check_knee_of_maps(atlas, got[i], kept[i])


def _write_models(td, patch, unet_seed, bn=False):
    """tests/test_surface_gpu.py::_write_models"""
    with open(os.path.join(td, "segmentation_train_config.pth.tar"), "w") as f:     # JSON under a .pth.tar name
        json.dump({"patch_size": list(patch), "model": "UNet",
                   "model_setting": {"in_channels": 1, "n_classes": 2, "bias": True, "BN": bn}}, f)
    torch.save({"model_state_dict": make_unet_state_dict(seed=unet_seed, bn=bn), "epoch": 3, "best_score": 0.5},
               os.path.join(td, "segmentation_model.pth.tar"))


def test_process_cohort_thickness_on_nifti_files(atlas, tmp_path):
    """The set-up of test_surface_gpu.py::test_dask_task_bodies_with_a_persistent_worker: three NIfTI files, a stand-in worker."""
    from oai_analysis_2_amd import dask_processing as dp
    from oai_analysis_2_amd.io_nifti import write_nifti
    td = str(tmp_path)
    _write_models(td, (64, 64, 32), 4)
    icon_sd = make_icon_state_dict(3, last_scale=0.1)
    dp.set_worker(dp.Worker(models_dir=td, icon_weights=icon_sd, icon_net_shape=(40, 48, 48)))
    try:
        atlas_img = Image(make_volume(31, (40, 80, 88)), [0.4, 0.35, 0.75], [0.0, -1.0, 2.0])
        paths = []
        for i in range(3):
            p = os.path.join(td, f"knee{i}.nii.gz")
            write_nifti(p, Image(make_volume(30 + i, (24, 72, 72)) * 900.0 + 17.0, [0.36, 0.37, 0.7], [1.0, 2.0, 3.0]))
            paths.append(p)
        got = dict(dp.process_cohort_thickness(paths, atlas_img, atlas))
        assert set(got) == {0, 1, 2} and _threads() == []
        maps = dict(dp.process_cohort(paths, atlas_img, keep_on_device=True))          # the same volumes again: the maps themselves
        for i in range(3):
            _check_knee_of_maps(atlas, got[i], maps[i])
    finally:
        dp.set_worker(None)
