"""GPU: the device inner / outer split (csrc/mesh_split.hip) against the reference's own split functions (tests/golden/mesh_split.npz)
and against the host path."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "mesh_split.npz")))


def _mesh(golden, name):
    from oai_analysis_2_amd import mesh_processing as mp
    return mp.Mesh(golden[f"{name}_verts"], golden[f"{name}_faces"])


@pytest.mark.parametrize("name", ["fc", "tc"])
def test_attributes_sides_and_iterations_match_the_reference(golden, name):
    from oai_analysis_2_amd import mesh_processing as mp
    mesh = _mesh(golden, name)
    sp = mp.split_mesh_device(mesh, name.upper())
    assert np.array_equal(sp.centroids.cpu().numpy(), mp.get_cell_centroid(mesh))
    assert np.array_equal(sp.normals.cpu().numpy(), mp.get_cell_normals(mesh))
    side, ref, margin = sp.side.cpu().numpy(), golden[f"{name}_side"], golden[f"{name}_margin"]
    decided = margin > 1e-10
    print(f"{name}: {int((~decided).sum())} faces with a golden margin <= 1e-10, {int((ref == 0).sum())} faces in no slab")
    assert np.array_equal(side[decided], ref[decided])
    assert np.array_equal(sp.n_iter, golden[f"{name}_n_iter"])


@pytest.mark.parametrize("name", ["fc", "tc"])
def test_sub_meshes_are_get_sub_mesh_bit_for_bit(golden, name):
    from oai_analysis_2_amd import mesh_processing as mp
    mesh = _mesh(golden, name)
    split = mp.split_femoral_cartilage_surface_device if name == "fc" else mp.split_tibial_cartilage_surface_device
    inner, outer, inner_list, outer_list = split(mesh)
    ref = golden[f"{name}_side"]
    for sub, lst, s in ((inner, inner_list, -1), (outer, outer_list, 1)):
        want = np.flatnonzero(ref == s)
        assert np.array_equal(lst, want)
        exp = mp.get_sub_mesh(mesh, want)
        assert sub.verts.dtype == np.float32 and sub.faces.dtype == np.int32
        assert np.array_equal(sub.verts.view(np.uint32), exp.verts.view(np.uint32))
        assert np.array_equal(sub.faces, exp.faces)


def test_three_runs_give_the_same_bits(golden):
    from oai_analysis_2_amd import mesh_processing as mp
    mesh = _mesh(golden, "fc")
    runs = [mp.split_femoral_cartilage_surface_device(mesh) for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, b)
            else:
                assert np.array_equal(a.verts.view(np.uint32), b.verts.view(np.uint32)) and np.array_equal(a.faces, b.faces)


def test_a_slab_with_fewer_than_two_faces_raises_and_the_process_stays_usable(golden):
    from oai_analysis_2_amd import mesh_processing as mp
    mesh = _mesh(golden, "fc")
    # one extra triangle far out along x: the first slab holds only it
    v = np.concatenate([mesh.verts, np.array([[-1000, 0, 0], [-1000, 1, 0], [-1000, 0, 1]], np.float32)])
    n = len(mesh.verts)
    f = np.concatenate([mesh.faces, np.array([[n, n + 1, n + 2]], np.int32)])
    with pytest.raises(ValueError, match="n_samples=1 should be >= n_clusters=2"):
        mp.split_mesh(mp.Mesh(v, f), "FC", on_device=True)
    inner, outer = mp.split_mesh(mesh, "FC", on_device=True)
    assert inner.GetNumberOfCells() == int((golden["fc_side"] == -1).sum())


def test_the_device_path_does_not_import_sklearn(golden, monkeypatch):
    from oai_analysis_2_amd import mesh_processing as mp
    monkeypatch.setitem(sys.modules, "sklearn", None)
    monkeypatch.setitem(sys.modules, "sklearn.cluster", None)
    inner, outer = mp.split_mesh(_mesh(golden, "tc"), "TC", on_device=True)
    assert inner.GetNumberOfCells() == int((golden["tc_side"] == -1).sum())
    with pytest.raises(ImportError):
        mp.split_mesh(_mesh(golden, "tc"), "TC")


def test_thickness_of_a_shell_split_on_the_device():
    """the shell of test_mesh_gpu.test_thickness_of_a_shell through get_thickness_mesh(split_on_device=True): the same inner / outer
    faces and distances as the host path"""
    pytest.importorskip("sklearn")
    from oai_analysis_2_amd import mesh_processing as mp
    from oai_analysis_2_amd.image import Image
    D, H, W = 48, 96, 96
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    R, T = 60.0, 6.0
    r = np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4 + (y + 30) ** 2)
    sig = lambda t: 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))
    prob = sig(2.0 * (np.abs(r - R) - T / 2)) * sig(2.0 * (np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4) - 30))
    img = Image(prob.astype(np.float32), [1.0, 1.0, 1.0])
    host_inner = {}
    for mesh_type in ("TC", "FC"):
        host = mp.get_thickness_mesh(img, mesh_type, min_cells=100)
        dev = mp.get_thickness_mesh(img, mesh_type, min_cells=100, split_on_device=True)
        for a, b in zip(host, dev):
            assert np.array_equal(a.faces, b.faces) and np.array_equal(a.verts, b.verts)
            assert np.array_equal(a.point_data["Distance"], b.point_data["Distance"])
        assert dev[0].GetNumberOfCells() > 500 and dev[1].GetNumberOfCells() > 500
        if mesh_type == "TC":                                        # the shell is a plateau: the TC split recovers its thickness
            assert abs(np.median(dev[0].point_data["Distance"]) - T) < 1.5
        host_inner[mesh_type] = host[0]
    # the Dask task body with the device split
    from oai_analysis_2_amd.dask_processing import get_thickness
    inner_d = get_thickness(img, "TC", split_on_device=True)
    assert np.array_equal(inner_d.faces, host_inner["TC"].faces)
    assert np.array_equal(inner_d.point_data["Distance"], host_inner["TC"].point_data["Distance"])
