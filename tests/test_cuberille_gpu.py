"""GPU: get_mesh_from_probability_map / cuberille_device (csrc/cuberille.hip) against the numpy restatement of the contract
(tests/cuberille_ref.py) bit for bit -- faces, vertex order, unprojected and projected vertices, step counts -- on seeded smooth maps
with several geometries; an analytic ellipsoid (distance to the 0.5 surface, steps, volume, same bits twice); device-tensor input;
and a thickness mesh written and read back through meshwrite / meshread."""
import numpy as np
import pytest
import torch

import cuberille_ref as ref
from oai_analysis_2_amd import meshread, meshwrite
from oai_analysis_2_amd import mesh_processing as mp
from oai_analysis_2_amd.image import Image

pytestmark = pytest.mark.gpu


def _smooth_map(seed, shape=(22, 26, 24)):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=shape)
    for _ in range(6):                                   # box smoothing: a few blobs per volume, with contacts and holes
        v = sum(np.roll(v, s, a) for a in range(3) for s in (-1, 1)) / 6.0
    v = (v - v.mean()) / v.std()
    return (1.0 / (1.0 + np.exp(-3.0 * v))).astype(np.float32)


def _rotation(seed, reflect=False):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q if np.linalg.det(q) > 0 else -q
    return q @ np.diag([1.0, 1.0, -1.0]) if reflect else q


GEOMETRIES = {
    "unit": dict(),
    "spacing_origin": dict(spacing=(0.36, 0.36, 0.7), origin=(-31.5, 12.25, 80.0)),
    "rotated": dict(spacing=(0.5, 0.6, 0.8), origin=(3.0, -4.0, 5.0), direction=_rotation(11)),
    "reflected": dict(spacing=(0.7, 0.5, 0.6), origin=(1.0, 2.0, -3.0), direction=_rotation(12, reflect=True)),
}


def _device(vol, g, **kw):
    v, f, k = mp.cuberille_device(Image(vol, g.get("spacing", (1, 1, 1)), g.get("origin", (0, 0, 0)), g.get("direction", np.eye(3))), 0.5, **kw)
    return v.cpu().numpy(), f.cpu().numpy(), k.cpu().numpy()


@pytest.mark.parametrize("move", [True, False])
@pytest.mark.parametrize("geo", list(GEOMETRIES))
@pytest.mark.parametrize("seed", [0, 1])
def test_bitwise_equal_to_the_restatement(seed, geo, move):
    vol, g = _smooth_map(seed), GEOMETRIES[geo]
    want = ref.cuberille(vol, 0.5, move_after_converged=move, **g)
    assert len(want["faces"]) > 500
    verts, faces, steps = _device(vol, g, move_after_converged=move)
    assert faces.dtype == np.int32 and np.array_equal(faces, want["faces"])
    assert verts.dtype == np.float32 and verts.tobytes() == want["verts"].tobytes()
    assert np.array_equal(steps, want["steps"]) and steps.max() > 1
    flat = ref.cuberille(vol, 0.5, project_vertices=False, **g)
    v0, f0, k0 = _device(vol, g, project_vertices_to_iso_surface=False)
    assert v0.tobytes() == flat["verts"].tobytes() and np.array_equal(f0, flat["faces"]) and not k0.any()
    quads = ref.cuberille(vol, 0.5, triangles=False, move_after_converged=move, **g)
    vq, fq, kq = _device(vol, g, generate_triangle_faces=False, move_after_converged=move)
    assert fq.shape == quads["faces"].shape and np.array_equal(fq, quads["faces"]) and vq.tobytes() == want["verts"].tobytes()


def test_other_settings_bitwise():
    vol = _smooth_map(5)
    kw = dict(threshold=0.01, step_length=0.1, relaxation=0.8, max_steps=3)
    want = ref.cuberille(vol, 0.4, spacing=(0.5, 0.5, 0.5), **kw)
    v, f, k = mp.cuberille_device(Image(vol, (0.5, 0.5, 0.5)), 0.4, project_vertex_surface_distance_threshold=0.01, project_vertex_step_length=0.1,
                                  project_vertex_step_length_relaxation_factor=0.8, project_vertex_maximum_number_of_steps=3)
    assert v.cpu().numpy().tobytes() == want["verts"].tobytes() and np.array_equal(f.cpu().numpy(), want["faces"])
    assert np.array_equal(k.cpu().numpy(), want["steps"]) and k.max().item() == 4          # k > max_steps stops after max_steps + 1 moves


def test_hand_cases_on_the_device():
    v = np.zeros((3, 3, 3), np.float32)
    v[1, 1, 1] = 0.5                                                       # exactly iso: inside
    m = mp.get_mesh_from_probability_map(Image(v), project_vertices_to_iso_surface=False)
    assert m.verts.shape == (8, 3) and m.faces.shape == (12, 3)
    e = np.zeros((1, 2, 2), np.float32)
    e[0, 0, 0] = e[0, 1, 1] = 1.0                                          # edge contact, at the border
    r = ref.cuberille(e, project_vertices=False)
    m = mp.get_mesh_from_probability_map(e, project_vertices_to_iso_surface=False)
    assert m.verts.shape == (14, 3) and np.array_equal(m.faces, r["faces"]) and m.verts.tobytes() == r["verts"].tobytes()
    empty = mp.get_mesh_from_probability_map(np.zeros((4, 5, 6), np.float32))
    assert empty.verts.shape == (0, 3) and empty.faces.shape == (0, 3)


@pytest.mark.parametrize("move", [False, True])
def test_analytic_ellipsoid(move):
    e = ref.ellipsoid_case()
    img = Image(e["vol"], e["spacing"])
    m = mp.get_mesh_from_probability_map(img, move_after_converged=move)
    _, _, steps = mp.cuberille_device(img, move_after_converged=move)
    steps = steps.cpu().numpy()
    smax = max(e["spacing"])
    dist = e["distance"](m.verts.astype(np.float64))
    slack = ref.last_step(steps, 0.25 * smax) if move else 0.0
    print(f"[ellipsoid move_after_converged={move}] {len(m.verts)} verts, max distance {dist.max() / smax:.4f} x spacing, "
          f"max steps {steps.max()}, volume rel err {ref.signed_volume6(m.verts, m.faces) / 6.0 / e['volume'] - 1:.2e}")
    # float32 storage adds < 1e-5 mm
    assert np.all(dist <= 0.1 * smax + slack + 1e-5)
    assert steps.max() < 50
    assert abs(ref.signed_volume6(m.verts, m.faces) / 6.0 / e["volume"] - 1.0) < 0.015
    again = mp.get_mesh_from_probability_map(img, move_after_converged=move)
    assert again.verts.tobytes() == m.verts.tobytes() and np.array_equal(again.faces, m.faces)


def test_reference_positional_call_uses_the_reference_settings():
    vol = _smooth_map(3)
    img = Image(vol, (0.36, 0.36, 0.7), (10.0, -5.0, 2.0))
    got = mp.get_mesh_from_probability_map(img)
    want = ref.cuberille(vol, 0.5, spacing=img.spacing, origin=img.origin, threshold=0.05, triangles=True, move_after_converged=True)
    assert got.verts.tobytes() == want["verts"].tobytes() and np.array_equal(got.faces, want["faces"])


def test_device_tensor_input_matches_image_input():
    vol, g = _smooth_map(4), GEOMETRIES["rotated"]
    img = Image(vol, g["spacing"], g["origin"], g["direction"])
    a = mp.get_mesh_from_probability_map(img)
    t = torch.from_numpy(vol).cuda()
    b = mp.get_mesh_from_probability_map(t, spacing_xyz=g["spacing"], origin_xyz=g["origin"], direction=g["direction"])
    assert a.verts.tobytes() == b.verts.tobytes() and np.array_equal(a.faces, b.faces)
    v, f, k = mp.cuberille_device(t, spacing_xyz=g["spacing"], origin_xyz=g["origin"], direction=g["direction"])
    assert v.is_cuda and f.is_cuda and k.is_cuda and v.cpu().numpy().tobytes() == a.verts.tobytes()


def _sig(t):
    return 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))


@pytest.mark.parametrize("binary", [False, True])
def test_thickness_mesh_round_trips_through_vtk(tmp_path, binary):
    D, H, W = 48, 96, 96                                   # test_mesh_gpu.py's TC-sized bowl
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    r = np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4 + (y + 30) ** 2)
    prob = _sig(2.0 * (np.abs(r - 60.0) - 3.0)) * _sig(2.0 * (np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4) - 30))
    inner, _ = mp.get_thickness_mesh(Image(prob.astype(np.float32), [1.0, 1.0, 1.0]), "TC", min_cells=100, on_device=True)
    assert inner.GetNumberOfCells() > 500 and inner.point_data["Distance"].dtype == np.float32
    path = str(tmp_path / "itk_distance_inner_TC.vtk")
    meshwrite(inner, path, binary=binary)
    back = meshread(path)
    assert back.verts.tobytes() == inner.verts.tobytes() and np.array_equal(back.faces, inner.faces)
    assert back.point_data["Distance"].tobytes() == inner.point_data["Distance"].tobytes()
