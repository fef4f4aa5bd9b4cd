"""CPU: the restated split (tests/mesh_split_ref.py) against the reference's own split functions (the golden) and the installed
sklearn, and the argument checks of the device split's C-ABI entry points (no GPU is touched before them)."""
import ctypes as C
import os

import numpy as np
import pytest

from oai_analysis_2_amd import _lib

import mesh_split_ref as sref


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "mesh_split.npz")))


@pytest.mark.parametrize("name", ["fc", "tc"])
def test_restatement_gives_the_reference_split(golden, name):
    side, n_iter = sref.split_sides(golden[f"{name}_verts"], golden[f"{name}_faces"], name.upper())
    assert np.array_equal(side, golden[f"{name}_side"])
    assert np.array_equal(n_iter, golden[f"{name}_n_iter"])
    assert len(golden[f"{name}_faces"]) > 15000 and (golden[f"{name}_margin"] > 1e-10).all()
    if name == "fc":
        assert (golden["fc_side"] == 0).sum() > 0                  # the faces in no slab (the reference's half-open slabs)


def _blobs(rng, n, d, sep, spread):
    c = rng.normal(size=(2, d)) * sep
    lab = rng.integers(0, 2, n)
    return c[lab] + rng.normal(size=(n, d)) * spread


# (n, d, n_init, seed, separation, spread): well-separated blobs stop strictly, overlapping ones on tol
CASES = [(3000, 6, 1, 0, 3.0, 1.0), (3000, 9, 5, 1, 3.0, 1.0), (8000, 6, 5, 2, 0.3, 1.0), (8000, 9, 1, 3, 0.3, 1.0),
         (500, 9, 5, 4, 1.0, 1.0), (20000, 6, 1, 5, 0.5, 1.0), (6000, 9, 5, 6, 0.2, 1.0)]


def test_restated_kmeans_is_sklearns():
    KMeans = pytest.importorskip("sklearn.cluster").KMeans
    stops = set()
    for n, d, n_init, seed, sep, spread in CASES:
        X = _blobs(np.random.default_rng(seed), n, d, sep, spread)
        km = KMeans(n_clusters=2, algorithm="lloyd", n_init=n_init, random_state=5).fit(X)
        labels, n_iter, inertia, centres, strict = sref.kmeans(X, n_init)
        assert np.array_equal(labels, km.labels_), (n, d, n_init, seed)
        assert n_iter == km.n_iter_, (n, d, n_init, seed)
        assert abs(inertia - km.inertia_) <= 1e-9 * km.inertia_
        stops.add(strict)
    assert stops == {True, False}                                   # both stopping rules are exercised


def test_restated_best_of_init_rule():
    a = np.array([0, 0, 1, 1, 0])
    assert sref.same_clustering(a, 1 - a) and sref.same_clustering(a, a)
    assert not sref.same_clustering(a, np.array([0, 1, 1, 1, 0]))
    with pytest.raises(ValueError, match="n_samples=1"):
        sref.kmeans(np.zeros((1, 6)), 1)


def test_abi_argument_checks():
    lib = _lib.load()
    d = (C.c_double * 64)()
    counts = (C.c_longlong * 3)(10, 10, 10)
    first = (C.c_longlong * 15)()
    uni = (C.c_double * 30)()
    it = (C.c_int * 3)()
    err = lambda: lib.oai_last_error()
    assert lib.oai_mesh_split_workspace_bytes(100, 1, 0, 5) == 0 and lib.oai_mesh_split_workspace_bytes(100, 200, 2, 5) == 0
    assert lib.oai_mesh_split_workspace_bytes(100, 200, 0, 0) == 0 and lib.oai_mesh_split_workspace_bytes(100, 200, 0, 6) == 0
    fc, tc = int(lib.oai_mesh_split_workspace_bytes(100, 200, 0, 5)), int(lib.oai_mesh_split_workspace_bytes(100, 200, 1, 1))
    assert fc > tc > 200 * 6 * 8
    # sized by the rows the slabs need (n_faces + a seam allowance), not 3 x n_faces, and by the runs actually made
    n = 200000
    big = int(lib.oai_mesh_split_workspace_bytes(n, n, 0, 5))
    per_row = 9 * 8 + 4 + 5 * (1 + 8)                               # features, face index, 5 x (label, distance)
    assert big < (n * per_row + n * (1 + 2 * 3 * 4)) * 1.1           # + slab mask, 3 flag and 3 offset arrays
    assert int(lib.oai_mesh_split_workspace_bytes(n, n, 1, 5)) - int(lib.oai_mesh_split_workspace_bytes(n, n, 1, 1)) >= 4 * n * 9
    c3 = (C.c_longlong * 3)()
    assert lib.oai_mesh_split_features(None, 100, d, 200, 0, d, fc, d, d, c3, None) != 0 and b"null" in err()
    assert lib.oai_mesh_split_features(d, 100, d, 200, 7, d, fc, d, d, c3, None) != 0 and b"mesh_type" in err()
    assert lib.oai_mesh_split_features(d, 100, d, 1, 0, d, fc, d, d, c3, None) != 0 and b"faces" in err()
    assert lib.oai_mesh_split_features(d, 2, d, 200, 0, d, fc, d, d, c3, None) != 0 and b"vertices" in err()
    f1 = int(lib.oai_mesh_split_workspace_bytes(100, 200, 0, 1))       # the features call needs the rows of one run
    assert lib.oai_mesh_split_features(d, 100, d, 200, 0, d, f1 - 1, d, d, c3, None) != 0 and b"workspace" in err()
    k = lambda **kw: lib.oai_mesh_split_kmeans(kw.get("n", 200), kw.get("t", 0), kw.get("ws", d), kw.get("wb", fc), d, kw.get("n_init", 5),
                                               kw.get("max_iter", 300), kw.get("counts", counts), kw.get("first", first), uni,
                                               kw.get("side", d), it, None)
    assert k(side=None) != 0 and b"null" in err()
    assert k(t=3) != 0 and b"mesh_type" in err()
    assert k(n=1) != 0 and b"faces" in err()
    assert k(n_init=0) != 0 and b"n_init" in err() and k(n_init=6) != 0
    assert k(max_iter=0) != 0 and b"max_iter" in err()
    assert k(wb=fc - 1) != 0 and b"workspace" in err()
    assert k(t=1, n_init=2, wb=tc) != 0 and b"workspace" in err()          # a TC workspace holds one run's rows
    assert k(counts=(C.c_longlong * 3)(10, 1, 10)) != 0 and b"n_samples=1 should be >= n_clusters=2" in err()
    assert k(first=(C.c_longlong * 15)(10)) != 0 and b"first centre" in err()
    assert lib.oai_mesh_submesh_workspace_bytes(100, 0) == 0 and lib.oai_mesh_submesh_workspace_bytes(100, 200) > 200 * 4
    sb = int(lib.oai_mesh_submesh_workspace_bytes(100, 200))
    nv, nf = C.c_longlong(), C.c_longlong()
    s = lambda **kw: lib.oai_mesh_submesh(kw.get("v", d), kw.get("nv", 100), d, kw.get("nf", 200), d, -1, d, kw.get("wb", sb), d, d, d,
                                          C.byref(nv), C.byref(nf), None)
    assert s(v=None) != 0 and b"null" in err()
    assert s(nf=0) != 0 and b"faces" in err()
    assert s(nv=0) != 0 and b"vertices" in err()
    assert s(wb=sb - 1) != 0 and b"workspace" in err()


def test_python_layer_exports_the_device_split():
    import inspect
    from oai_analysis_2_amd import dask_processing, mesh_processing as mp
    for name in ("split_mesh_device", "split_femoral_cartilage_surface_device", "split_tibial_cartilage_surface_device", "get_sub_mesh_device"):
        assert callable(getattr(mp, name)), name
    assert inspect.signature(mp.split_mesh).parameters["on_device"].default is False
    assert inspect.signature(mp.get_thickness_mesh).parameters["split_on_device"].default is False
    assert inspect.signature(dask_processing.get_thickness).parameters["split_on_device"].default is False


def test_host_draws_follow_sklearn():
    from oai_analysis_2_amd.mesh_processing import _kmeans_draws
    first, uni = _kmeans_draws([50, 70], 2)
    rs = np.random.RandomState(5)
    assert first[0] == rs.choice(50, p=np.ones(50) / 50) and uni[:2] == list(rs.uniform(size=2))
    with pytest.raises(ValueError, match="n_samples=1 should be >= n_clusters=2"):
        _kmeans_draws([10, 1], 5)
