"""CPU: the thickness image's semantics (tests/thickness_image_ref.py, the numpy restatement of csrc/thickness_image.hip), the exact
host rules of the atlas raster (thickness.fc_cut / fc_face_skip / tc_face_skip) and the argument checks of the new C-ABI entry points
(no GPU is touched before them)."""
import ctypes as C
import os
import re

import numpy as np

import thickness_image_ref as iref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("oai_thickness_image_workspace_bytes", "oai_thickness_image_build", "oai_thickness_image_apply")


def test_restatement_on_a_hand_made_case():
    # a unit square of two triangles sharing the diagonal (0,0)-(4,4), which runs through pixel centres; face 2 repeats face 0 with a
    # degenerate corner, face 3 is a good triangle over the whole image that is marked as skipped
    uv = np.array([[0, 0], [4, 0], [4, 4], [0, 4], [-8, -8], [16, -8], [-8, 16]], np.float64)
    faces = np.array([[0, 2, 3], [0, 1, 2], [0, 0, 2], [4, 5, 6]], np.int32)
    skip = np.array([0, 0, 0, 1], bool)
    lo, step, shape = np.array([0.0, 0.0]), np.array([0.5, 0.5]), (8, 8)             # centres at 0.25, 0.75, ...: (k + 0.5) / 2
    owner, corners, weights = iref.build(uv, faces, skip, lo, step, shape)
    j, i = np.mgrid[0:8, 0:8]
    assert (owner >= 0).all()                                                        # the square is the whole image
    assert np.array_equal(owner[j == i], np.zeros(8, np.int32))                      # on the shared edge: the lower face index
    assert np.array_equal(owner[j > i], np.zeros((j > i).sum(), np.int32)) and np.array_equal(owner[j < i], np.ones((j < i).sum(), np.int32))
    assert not np.isin(owner, (2, 3)).any()                                          # degenerate / skipped faces own nothing
    assert np.array_equal(corners[owner == 1], np.broadcast_to(faces[1], ((owner == 1).sum(), 3)))
    assert (np.abs(weights.sum(axis=-1) - 1.0) <= 4 * np.finfo(np.float64).eps).all()
    assert (weights >= 0).all()
    # the same faces the other way round (negative area): the same pixels, the same owners
    owner2, _, w2 = iref.build(uv, faces[:, ::-1], skip, lo, step, shape)
    assert np.array_equal(owner2, owner) and (np.abs(w2.sum(axis=-1) - 1.0) <= 4 * np.finfo(np.float64).eps).all()
    # without the skip mark the big triangle would own nothing either (faces 0 and 1 come first), alone it owns everything
    assert (iref.build(uv, faces[3:], None, lo, step, shape)[0] == 0).all()
    # apply: NaN where nobody owns, NaN spreads from a NaN point, K rows = K single calls
    owner3, c3, w3 = iref.build(uv, faces[1:2], None, lo, step, shape)
    vals = np.array([1, 2, 3, 4, 0, 0, 0], np.float32)
    img = iref.apply(owner3, c3, w3, vals)
    assert img.dtype == np.float32 and np.array_equal(np.isnan(img), owner3 < 0) and (owner3 < 0).any()
    vals_nan = vals.copy(); vals_nan[1] = np.nan
    assert np.isnan(iref.apply(owner3, c3, w3, vals_nan)).all()
    both = iref.apply(owner3, c3, w3, np.stack([vals, vals_nan]))
    assert both.shape == (2, 8, 8) and np.array_equal(both[0], img, equal_nan=True)


def test_restatement_on_a_warped_grid_mesh():
    uv, faces = iref.warped_grid(60)
    shape = (128, 128)
    lo, step = iref.grid(uv, shape)
    owner, corners, weights = iref.build(uv, faces, None, lo, step, shape)
    # the mesh covers the rectangle of the raster: every pixel centre lies in some face, so every pixel has an owner
    assert (owner >= 0).all()
    # a function linear in (u, v) comes back at every covered pixel (barycentric weights are exact for linear functions)
    lin = 0.7 * uv[:, 0] - 0.031 * uv[:, 1] + 2.0
    pu, pv = iref.centres(lo, step, shape)
    want = 0.7 * pu[None, :] - 0.031 * pv[:, None] + 2.0
    got = (weights * lin[corners]).sum(axis=-1)
    assert np.abs(got - want).max() < 1e-12, np.abs(got - want).max()
    assert np.abs(weights.sum(axis=-1) - 1.0).max() <= 4 * np.finfo(np.float64).eps
    # the face boxes are conservative: testing every face against every pixel gives the same raster (a smaller case: it is quadratic)
    uv, faces = iref.warped_grid(14, seed=3)
    lo, step = iref.grid(uv, (40, 36))
    a, b = iref.build(uv, faces, None, lo, step, (40, 36)), iref.build(uv, faces, None, lo, step, (40, 36), whole_image=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (a[0] >= 0).all()
    # ... and a mesh with a hole: pixels inside the hole have no owner, exactly those whose centre is in no face
    keep = np.ones(len(faces), bool); keep[60:90] = False
    a, b = iref.build(uv, faces[keep], None, lo, step, (40, 36)), iref.build(uv, faces[keep], None, lo, step, (40, 36), whole_image=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and 0 < (a[0] < 0).sum() < 200


def test_fc_cut_makes_an_arc_across_pi_contiguous():
    from oai_analysis_2_amd import thickness as th
    rng = np.random.default_rng(4)
    length = 2.2
    arc = np.sort(rng.uniform(0, length, 500)); arc[0], arc[-1] = 0.0, length
    across = th.wrap_angle(arc + (np.pi - 0.9))                                       # from pi - 0.9 over the seam to -pi + 1.3
    assert across.max() - across.min() > 6.0                                          # raw: almost the full circle wide
    cut = th.fc_cut(across)
    u = th.wrap_angle(across - cut)
    assert abs((u.max() - u.min()) - length) < 1e-12
    assert np.array_equal(np.argsort(u, kind="stable"), np.arange(len(u)))             # the order along the arc is kept
    assert np.abs(th.wrap_angle(u + cut) - across).max() < 1e-12                      # a pixel maps back to its raw angle
    assert abs(u.max() + u.min()) < 1e-12                                             # the seam is in the middle of the gap
    # an arc away from +-pi is only shifted
    away = arc - 1.0
    cut = th.fc_cut(away)
    u = th.wrap_angle(away - cut)
    assert np.abs((u - away) - (u[0] - away[0])).max() < 1e-12 and abs((u.max() - u.min()) - length) < 1e-12
    # order of the input does not matter
    assert th.fc_cut(away[rng.permutation(len(away))]) == cut


def test_face_rules_match_brute_force():
    from oai_analysis_2_amd import thickness as th
    rng = np.random.default_rng(9)
    # FC: a closed ring of angles (a surface round the full circle): the faces across the seam are the ones with an edge longer than pi
    n = 90
    ang = th.wrap_angle(np.linspace(-np.pi, np.pi, n, endpoint=False) + 0.3)
    u = np.repeat(ang, 2)                                                             # two rows of vertices
    i = np.arange(n); k = (i + 1) % n
    faces = np.concatenate([np.stack([2 * i, 2 * k, 2 * i + 1], 1), np.stack([2 * k, 2 * k + 1, 2 * i + 1], 1)]).astype(np.int32)
    got = th.fc_face_skip(u, faces)
    brute = np.array([any(abs(u[f[a]] - u[f[b]]) > np.pi for a, b in ((0, 1), (1, 2), (2, 0))) for f in faces])
    assert np.array_equal(got, brute) and got.sum() == 2
    assert not th.fc_face_skip(th.wrap_angle(u * 0.4), faces).any()                   # an arc: no face is dropped
    # TC: faces with vertices on both sides of z = 50 (49.999996 is < 50 in float32, 50.0 is not)
    z = rng.uniform(30, 70, 300).astype(np.float32)
    z[:4] = [50.0, np.nextafter(np.float32(50), np.float32(0)), 49.0, 51.0]
    faces = rng.integers(0, 300, size=(500, 3)).astype(np.int32)
    faces[:3] = [[0, 3, 3], [1, 2, 2], [0, 1, 3]]
    got = th.tc_face_skip(z, faces)
    brute = np.array([len({bool(z[v] >= 50) for v in f}) > 1 for f in faces])
    assert np.array_equal(got, brute) and got[:3].tolist() == [False, False, True]
    order = th.tc_point_order(z)
    assert np.array_equal(np.sort(order), np.arange(300)) and (z[order[:(z >= 50).sum()]] >= 50).all()
    assert np.array_equal(order, np.concatenate([np.where(z >= 50)[0], np.where(z < 50)[0]]))


def test_grid_of_the_raster():
    from oai_analysis_2_amd import mesh_processing as mp
    import pytest
    uv = np.array([[0.0, 10.0], [2.0, 30.0], [np.nan, 5.0], [1.0, 50.0]])
    lo, step = mp.thickness_image_grid(uv, (10, 4))                                   # (H, W): step_u = extent_u / W, step_v = extent_v / H
    assert lo.tolist() == [0.0, 10.0] and step.tolist() == [0.5, 4.0]
    rl, rs = iref.grid(uv, (10, 4))
    assert np.array_equal(lo, rl) and np.array_equal(step, rs)
    with pytest.raises(ValueError):
        mp.thickness_image_grid(np.array([[1.0, 0.0], [1.0, 2.0]]), (4, 4))           # no extent along u
    with pytest.raises(ValueError):
        mp.thickness_image_grid(uv, (0, 4))


def test_abi_names_and_argument_checks():
    from oai_analysis_2_amd import _lib
    text = open(os.path.join(ROOT, "include", "oai_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/oai_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    lib = _lib.load()
    err = lambda: lib.oai_last_error()
    assert lib.oai_thickness_image_workspace_bytes(0, 64, 64) == 0 and lib.oai_thickness_image_workspace_bytes(10, 0, 64) == 0
    w1, w2 = lib.oai_thickness_image_workspace_bytes(1000, 64, 64), lib.oai_thickness_image_workspace_bytes(2000, 64, 64)
    assert 0 < w1 < w2
    dummy = (C.c_double * 64)()
    lo, step = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(1.0, 1.0)
    n_cov = C.c_longlong(-7)
    ws = int(lib.oai_thickness_image_workspace_bytes(4, 8, 8))
    build = lambda *a: lib.oai_thickness_image_build(*a)
    assert build(None, 8, dummy, 4, None, lo, step, 8, 8, dummy, ws, dummy, dummy, dummy, C.byref(n_cov), None) != 0 and b"null" in err()
    assert build(dummy, 8, dummy, 4, None, lo, step, 8, 8, dummy, ws, dummy, dummy, None, C.byref(n_cov), None) != 0 and b"null" in err()
    assert build(dummy, 8, dummy, 4, None, lo, step, 0, 8, dummy, ws, dummy, dummy, dummy, C.byref(n_cov), None) != 0 and b"image" in err()
    assert build(dummy, 8, dummy, 4, None, lo, step, 8, -1, dummy, ws, dummy, dummy, dummy, C.byref(n_cov), None) != 0 and b"image" in err()
    assert build(dummy, 0, dummy, 4, None, lo, step, 8, 8, dummy, ws, dummy, dummy, dummy, C.byref(n_cov), None) != 0 and b"points" in err()
    for bad in ((0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        assert build(dummy, 8, dummy, 4, None, lo, (C.c_double * 2)(*bad), 8, 8, dummy, ws, dummy, dummy, dummy, C.byref(n_cov), None) != 0
        assert b"step" in err()
    assert build(dummy, 8, dummy, 4, None, lo, step, 8, 8, dummy, ws - 1, dummy, dummy, dummy, C.byref(n_cov), None) != 0 and b"workspace" in err()
    assert n_cov.value == -7                                                          # nothing was written
    apply = lambda *a: lib.oai_thickness_image_apply(*a)
    assert apply(dummy, dummy, None, 8, 8, dummy, 8, 1, dummy, None) != 0 and b"null" in err()
    assert apply(dummy, dummy, dummy, 8, 0, dummy, 8, 1, dummy, None) != 0 and b"image" in err()
    assert apply(dummy, dummy, dummy, 8, 8, dummy, 0, 1, dummy, None) != 0 and b"points" in err()
    assert apply(dummy, dummy, dummy, 8, 8, dummy, 8, -1, dummy, None) != 0 and b"knees" in err()


def test_python_layer_exports():
    import oai_analysis_2_amd as pkg
    from oai_analysis_2_amd import dask_processing, mesh_processing as mp, thickness
    assert pkg.ThicknessAtlas is thickness.ThicknessAtlas and pkg.KneeThickness is thickness.KneeThickness
    for name in ("thickness_image_build", "thickness_image", "ThicknessRaster", "_map_attributes_dev", "_thickness_inner_dev"):
        assert hasattr(mp, name), name
    assert callable(dask_processing.thickness_stream) and callable(dask_processing.process_cohort_thickness)
    from oai_analysis_2_amd.pipeline import VolumeResult
    import dataclasses
    fields = [f.name for f in dataclasses.fields(VolumeResult)]
    assert fields[-1] == "thickness" and fields[:7] == ["fc", "tc", "phi", "fc_atlas", "tc_atlas", "overflow", "repeated_f32"]
