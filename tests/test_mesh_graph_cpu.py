"""CPU: the argument checks of the device mesh-graph entry points (csrc/mesh_graph.hip) -- every one returns an error before any GPU
work -- and the Python surface of the resident thickness step."""
import ctypes as C
import inspect

from oai_analysis_2_amd import _lib


def test_abi_argument_checks():
    lib = _lib.load()
    d = (C.c_double * 64)()
    err = lambda: lib.oai_last_error()
    rounds = C.c_int()
    nv, nf, nn = C.c_longlong(), C.c_longlong(), C.c_longlong()

    assert lib.oai_mesh_components_workspace_bytes(0, 10) == 0 and lib.oai_mesh_components_workspace_bytes(10, -1) == 0
    cb = int(lib.oai_mesh_components_workspace_bytes(100, 200))
    assert cb > 0
    c = lambda **kw: lib.oai_mesh_components(kw.get("f", d), kw.get("nf", 200), kw.get("nv", 100), kw.get("ws", d), kw.get("wb", cb),
                                             kw.get("label", d), C.byref(rounds), None)
    assert c(f=None) != 0 and b"null" in err()
    assert c(label=None) != 0 and b"null" in err()
    assert c(ws=None) != 0 and b"null" in err()
    assert c(nf=-1) != 0 and b"faces" in err()
    assert c(nv=0) != 0 and b"vertices" in err()
    assert c(nv=-5) != 0 and b"vertices" in err()
    assert c(wb=cb - 1) != 0 and b"workspace" in err()

    assert lib.oai_mesh_keep_large_regions_workspace_bytes(-1, 10) == 0 and lib.oai_mesh_keep_large_regions_workspace_bytes(10, -1) == 0
    kb = int(lib.oai_mesh_keep_large_regions_workspace_bytes(100, 200))
    assert kb > (100 + 200) * 4
    k = lambda **kw: lib.oai_mesh_keep_large_regions(kw.get("v", d), kw.get("nv", 100), kw.get("f", d), kw.get("nf", 200), 3000, kw.get("ws", d),
                                                     kw.get("wb", kb), kw.get("vo", d), kw.get("fo", d), kw.get("pnv", C.byref(nv)),
                                                     C.byref(nf), None)
    assert k(v=None) != 0 and b"null" in err()
    assert k(f=None) != 0 and b"null" in err()
    assert k(fo=None) != 0 and b"null" in err()
    assert k(pnv=None) != 0 and b"null" in err()
    assert k(nf=-1) != 0 and b"faces" in err()
    assert k(nv=-1) != 0 and b"vertices" in err()
    assert k(nv=0) != 0 and b"faces without vertices" in err()
    assert k(wb=kb - 1) != 0 and b"workspace" in err()

    assert lib.oai_mesh_adjacency_workspace_bytes(-1, 10) == 0 and lib.oai_mesh_adjacency_workspace_bytes(10, -1) == 0
    ab = int(lib.oai_mesh_adjacency_workspace_bytes(100, 200))
    assert ab > 200 * 6 * 4                                              # the half-edge lists
    a = lambda **kw: lib.oai_mesh_adjacency(kw.get("f", d), kw.get("nf", 200), kw.get("nv", 100), kw.get("ws", d), kw.get("wb", ab),
                                            kw.get("off", d), kw.get("nbr", d), kw.get("pn", C.byref(nn)), None)
    assert a(f=None) != 0 and b"null" in err()
    assert a(off=None) != 0 and b"null" in err()
    assert a(nbr=None) != 0 and b"null" in err()
    assert a(pn=None) != 0 and b"null" in err()
    assert a(nf=-1) != 0 and b"faces" in err()
    assert a(nv=-1) != 0 and b"vertices" in err()
    assert a(wb=ab - 1) != 0 and b"workspace" in err()

    gb = int(lib.oai_mesh_grid_params_workspace_bytes())
    assert gb > 0
    g = lambda **kw: lib.oai_mesh_grid_params(kw.get("v", d), kw.get("nv", 100), kw.get("f", d), kw.get("nf", 200), kw.get("ws", d),
                                              kw.get("wb", gb), kw.get("out", d), None)
    assert g(v=None) != 0 and b"null" in err()
    assert g(out=None) != 0 and b"null" in err()
    assert g(f=None) != 0 and b"null" in err()
    assert g(nv=0) != 0 and b"vertices" in err()
    assert g(nf=-1) != 0 and b"faces" in err()
    assert g(wb=gb - 1) != 0 and b"workspace" in err()


def test_python_layer_exports_the_resident_step():
    from oai_analysis_2_amd import dask_processing, mesh_processing as mp
    for name in ("keep_large_regions_device", "vertex_adjacency_device", "mesh_components_device", "mesh_grid_params_device"):
        assert callable(getattr(mp, name)), name
    assert inspect.signature(mp.get_mesh).parameters["on_device"].default is False
    assert inspect.signature(mp.get_thickness_mesh).parameters["on_device"].default is False
    assert inspect.signature(mp.get_thickness_mesh).parameters["split_on_device"].default is False
    assert inspect.signature(dask_processing.get_thickness).parameters["on_device"].default is False
