"""GPU: the mesh graph steps on the device (csrc/mesh_graph.hip) against the host graph code of mesh_processing, and the resident
thickness step (get_mesh / get_thickness_mesh with on_device=True) against the current path, bit for bit."""
import numpy as np
import pytest
import torch

from oai_analysis_2_amd.image import Image

pytestmark = pytest.mark.gpu

_sig = lambda t: 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))


def _scipy_min_labels(n, faces):
    """scipy's connected_components over the host's f0-f1 / f1-f2 edges, each label mapped to the smallest vertex of its component."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    g = coo_matrix((np.ones(2 * len(f), np.int8), (np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]]))), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    mins = np.full(lab.max() + 1, n, np.int64)
    np.minimum.at(mins, lab, np.arange(n))
    return mins[lab]


def _blobs():
    """Marching cubes of ~30 balls of mixed size (one of > 3000 faces) plus single-voxel specks."""
    from oai_analysis_2_amd import mesh_processing as mp
    rng = np.random.default_rng(11)
    D, H, W = 64, 96, 96
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    vol = np.zeros((D, H, W), np.float32)
    centres = [(32, 48, 48, 15.0)] + [(rng.uniform(6, D - 6), rng.uniform(6, H - 6), rng.uniform(6, W - 6), rng.uniform(1.2, 6.0)) for _ in range(30)]
    for cz, cy, cx, r in centres:
        vol = np.maximum(vol, _sig(2.0 * (np.sqrt((z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2) - r)))
    specks = rng.integers(1, [D - 1, H - 1, W - 1], size=(40, 3))
    vol[specks[:, 0], specks[:, 1], specks[:, 2]] = 1.0
    return mp.marching_cubes(vol, 0.5, (0.5, 0.5, 0.7))


def _spiral(n_steps=6000, seed=3):
    """A long thin strip wound as a spiral, vertex indices shuffled so that many hook / jump rounds are needed."""
    t = np.linspace(0, 40 * np.pi, n_steps)
    r = 1.0 + t
    v = np.zeros((2 * n_steps, 3), np.float32)
    v[0::2, 0], v[0::2, 1] = r * np.cos(t), r * np.sin(t)
    v[1::2, 0], v[1::2, 1], v[1::2, 2] = (r + 0.5) * np.cos(t), (r + 0.5) * np.sin(t), 0.1
    i = np.arange(n_steps - 1)
    f = np.concatenate([np.stack([2 * i, 2 * i + 1, 2 * i + 2], 1), np.stack([2 * i + 1, 2 * i + 3, 2 * i + 2], 1)])
    perm = np.random.default_rng(seed).permutation(len(v))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(v))
    return v[perm], inv[f].astype(np.int32)


def _soup(seed=5):
    """Random faces over 3000 vertices with duplicate faces, degenerate faces [a, a, b] / [a, a, a] and unreferenced vertices."""
    rng = np.random.default_rng(seed)
    n = 3000
    f = rng.integers(0, n - 200, size=(1500, 3))
    dup = f[rng.integers(0, len(f), 200)]
    a, b = rng.integers(0, n - 200, 100), rng.integers(0, n - 200, 100)
    deg = np.concatenate([np.stack([a, a, b], 1), np.stack([b, a, a], 1)[:50], np.stack([a, a, a], 1)[:20]])
    faces = np.concatenate([f, dup, deg])[rng.permutation(len(f) + len(dup) + len(deg))].astype(np.int32)
    return rng.normal(size=(n, 3)).astype(np.float32), faces


def _fan(k):
    v = np.zeros((k + 2, 3), np.float32)
    ang = np.linspace(0, np.pi, k + 1)
    v[1:, 0], v[1:, 1] = np.cos(ang), np.sin(ang)
    i = np.arange(1, k + 1)
    return v, np.stack([np.zeros(k, np.int64), i, i + 1], 1).astype(np.int32)


def _cases():
    v, f = _blobs()
    iso_v = np.concatenate([v, np.ones((7, 3), np.float32)])          # 7 unreferenced vertices at the end
    return {"blobs": (v, f), "spiral": _spiral(), "soup": _soup(), "isolated": (iso_v, f),
            "no_faces": (np.zeros((5, 3), np.float32), np.zeros((0, 3), np.int32))}


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.mark.parametrize("name", ["blobs", "spiral", "soup", "isolated", "no_faces"])
def test_components_match_scipy(cases, name):
    from oai_analysis_2_amd import mesh_processing as mp
    v, f = cases[name]
    lab, rounds = mp.mesh_components_device(torch.from_numpy(f).cuda(), len(v), return_rounds=True)
    lab = lab.cpu().numpy()
    assert lab.dtype == np.int32
    if len(f):
        assert np.array_equal(lab, _scipy_min_labels(len(v), f)), name
        assert rounds >= 1
    else:
        assert np.array_equal(lab, np.arange(len(v))) and rounds == 0
    if name == "blobs":
        assert len(np.unique(lab)) > 25
    if name == "spiral":
        assert len(np.unique(lab)) == 1 and rounds >= 2


@pytest.mark.parametrize("name", ["blobs", "soup", "isolated", "no_faces"])
def test_keep_large_regions_matches_host(cases, name):
    from oai_analysis_2_amd import mesh_processing as mp
    v, f = cases[name]
    counts = np.bincount(_scipy_min_labels(len(v), f)[f[:, 0]]) if len(f) else np.zeros(1, np.int64)
    for min_cells in (0, 100, 3000, int(counts.max()) + 1):
        hv, hf = mp.keep_large_regions(v, f, min_cells)
        dv, df = mp.keep_large_regions_device(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), min_cells)
        dv, df = dv.cpu().numpy(), df.cpu().numpy()
        assert dv.dtype == np.float32 and df.dtype == np.int32
        assert np.array_equal(dv, hv) and np.array_equal(df, hf), (name, min_cells)
    if name == "blobs":
        assert 0 < len(mp.keep_large_regions(v, f, 3000)[1]) < len(f)


@pytest.mark.parametrize("name", ["blobs", "spiral", "soup", "isolated", "no_faces", "fan200", "fan12"])
def test_adjacency_matches_host(cases, name):
    from oai_analysis_2_amd import mesh_processing as mp
    v, f = {"fan200": _fan(200), "fan12": _fan(12)}.get(name) or cases[name]
    ho, hn = mp.vertex_adjacency(len(v), f)
    do, dn = mp.vertex_adjacency_device(len(v), torch.from_numpy(f).cuda())
    assert np.array_equal(do.cpu().numpy(), ho) and np.array_equal(dn.cpu().numpy(), hn), name
    if name == "fan200":
        assert ho[1] - ho[0] == 201                           # the centre: 201 rim vertices, beyond the register-resident sort


@pytest.mark.parametrize("name", ["blobs", "spiral", "soup"])
def test_grid_params_match_numpy(cases, name):
    from oai_analysis_2_amd import mesh_processing as mp
    v, f = cases[name]
    lo, hi, edge = mp.mesh_grid_params_device(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda())
    tri = v[f].astype(np.float64)
    ref = max(np.linalg.norm(tri[:, 0] - tri[:, 1], axis=1).max(), np.linalg.norm(tri[:, 1] - tri[:, 2], axis=1).max(),
              np.linalg.norm(tri[:, 2] - tri[:, 0], axis=1).max())
    assert np.array_equal(lo, v.min(axis=0).astype(np.float64)) and np.array_equal(hi, v.max(axis=0).astype(np.float64))
    assert edge.tobytes() == np.float64(ref).tobytes()


def _bowl():
    """test_mesh_gpu.py::test_thickness_of_a_shell's cap of a spherical shell (TC-sized)."""
    D, H, W = 48, 96, 96
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    R, T = 60.0, 6.0
    r = np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4 + (y + 30) ** 2)
    prob = _sig(2.0 * (np.abs(r - R) - T / 2)) * _sig(2.0 * (np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4) - 30))
    return Image(prob.astype(np.float32), [1.0, 1.0, 1.0])


def _slab():
    """scripts/bench_mesh.py's femoral-cartilage-like slab at half size."""
    D, H, W = 80, 192, 192
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    R, T = 110.0, 5.0
    r = np.sqrt((x - 96) ** 2 + ((z - 40) * 1.9) ** 2 + (y + 30) ** 2)
    prob = _sig(2.0 * (np.abs(r - R) - T / 2)) * _sig(2.0 * (np.sqrt((x - 96) ** 2 + ((z - 40) * 1.9) ** 2) - 70))
    return Image(prob.astype(np.float32), [0.36, 0.36, 0.7])


def _same_mesh(a, b):
    return np.array_equal(a.verts, b.verts) and np.array_equal(a.faces, b.faces) and a.verts.dtype == b.verts.dtype and \
        a.faces.dtype == b.faces.dtype and sorted(a.point_data) == sorted(b.point_data) and \
        all(np.array_equal(a.point_data[k], b.point_data[k]) for k in a.point_data)


@pytest.mark.parametrize("num_iterations", [20, 0])
def test_get_mesh_on_device_is_bitwise(num_iterations):
    from oai_analysis_2_amd import mesh_processing as mp
    img = _bowl()
    ref = mp.get_mesh(img, num_iterations=num_iterations, min_cells=100)
    got = mp.get_mesh(img, num_iterations=num_iterations, min_cells=100, on_device=True)
    assert ref.GetNumberOfCells() > 3000 and _same_mesh(got, ref)
    t = torch.from_numpy(img.array).cuda()
    assert _same_mesh(mp.get_mesh(t, num_iterations=num_iterations, min_cells=100, on_device=True, spacing_xyz=img.spacing), ref)


def test_get_mesh_on_device_of_an_empty_map():
    from oai_analysis_2_amd import mesh_processing as mp
    img = Image(np.zeros((8, 9, 10), np.float32))
    ref, got = mp.get_mesh(img), mp.get_mesh(img, on_device=True)
    assert _same_mesh(got, ref) and got.verts.shape == (0, 3) and got.faces.shape == (0, 3)


@pytest.mark.parametrize("mesh_type", ["TC", "FC"])
def test_thickness_on_device_is_bitwise(mesh_type):
    from oai_analysis_2_amd import mesh_processing as mp
    img = _bowl() if mesh_type == "TC" else _slab()
    min_cells = 100 if mesh_type == "TC" else 3000
    ref_in, ref_out = mp.get_thickness_mesh(img, mesh_type, min_cells=min_cells, split_on_device=True)
    assert ref_in.GetNumberOfCells() > 500 and ref_out.GetNumberOfCells() > 500
    t = torch.from_numpy(img.array).cuda()
    runs = [mp.get_thickness_mesh(img, mesh_type, min_cells=min_cells, on_device=True),
            mp.get_thickness_mesh(img, mesh_type, min_cells=min_cells, on_device=True),
            mp.get_thickness_mesh(t, mesh_type, min_cells=min_cells, on_device=True, spacing_xyz=img.spacing)]
    for got_in, got_out in runs:
        assert _same_mesh(got_in, ref_in) and _same_mesh(got_out, ref_out)
        assert got_in.point_data["Distance"].dtype == np.float32


def test_thickness_via_dask_body_on_device():
    from oai_analysis_2_amd.dask_processing import get_thickness
    img = _bowl()
    assert _same_mesh(get_thickness(img, "TC", on_device=True), get_thickness(img, "TC", split_on_device=True))


def test_no_large_region_raises_the_same_error():
    from oai_analysis_2_amd import mesh_processing as mp
    D = 24
    z, y, x = np.mgrid[0:D, 0:D, 0:D].astype(np.float32)
    img = Image(_sig(2.0 * (np.sqrt((x - 12) ** 2 + (y - 12) ** 2 + (z - 12) ** 2) - 4.0)).astype(np.float32))
    with pytest.raises(ValueError) as host:
        mp.get_thickness_mesh(img, "FC", split_on_device=True)
    with pytest.raises(ValueError) as dev:
        mp.get_thickness_mesh(img, "FC", on_device=True)
    assert str(dev.value) == str(host.value) == "n_samples=0 should be >= n_clusters=2."
