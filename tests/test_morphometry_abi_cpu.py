"""CPU: the morphometry entry points of the C ABI (include/oai_hip.h: oai_mesh_areas, oai_point_footprint(_grid), oai_region_stats) are
exported by the built library and refuse bad arguments with a status and a message -- no GPU is touched before the checks."""
import ctypes as C

import pytest

from abi_cases import check_symbols, refused as _refused
from oai_analysis_2_amd import _lib

NEW = ("oai_mesh_areas_workspace_bytes", "oai_mesh_areas", "oai_point_footprint", "oai_point_footprint_grid", "oai_region_stats_workspace_bytes",
       "oai_region_stats")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    check_symbols(NEW)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_mesh_areas_argument_checks(lib):
    d = (C.c_float * 16)()                                            # a host buffer: every call below must fail before it is read
    assert lib.oai_mesh_areas_workspace_bytes(-1, 4) == 0 and lib.oai_mesh_areas_workspace_bytes(4, -1) == 0
    assert lib.oai_mesh_areas_workspace_bytes(4, (1 << 28) + 1) == 0
    need = lib.oai_mesh_areas_workspace_bytes(100, 200)
    assert need >= 200 * 8 + 2 * 101 * 4 + 600 * 4
    _refused(lib, lib.oai_mesh_areas(None, 4, d, 2, d, need, d, d, None), b"oai_mesh_areas", b"null")
    _refused(lib, lib.oai_mesh_areas(d, 4, None, 2, d, need, d, d, None), b"null")
    _refused(lib, lib.oai_mesh_areas(d, 4, d, 2, None, need, d, d, None), b"null")
    _refused(lib, lib.oai_mesh_areas(d, 4, d, 2, d, need, d, None, None), b"null")
    _refused(lib, lib.oai_mesh_areas(d, -1, d, 2, d, need, d, d, None), b"oai_mesh_areas", b"-1")
    _refused(lib, lib.oai_mesh_areas(d, 4, d, -2, d, need, d, d, None), b"oai_mesh_areas", b"-2")
    _refused(lib, lib.oai_mesh_areas(d, 100, d, 200, d, 16, d, d, None), b"oai_mesh_areas", b"workspace")


def test_point_footprint_argument_checks(lib):
    d = (C.c_float * 16)()
    lo, dims = (C.c_double * 3)(0, 0, 0), (C.c_int * 3)(4, 4, 4)
    _refused(lib, lib.oai_point_footprint(None, 4, d, 4, 1.0, d, d, d, None), b"oai_point_footprint", b"null")
    _refused(lib, lib.oai_point_footprint(d, 4, d, 4, 1.0, None, d, d, None), b"null")
    _refused(lib, lib.oai_point_footprint(d, 4, d, 4, 1.0, d, None, d, None), b"null")
    _refused(lib, lib.oai_point_footprint(d, 4, d, 4, 1.0, d, d, None, None), b"null")
    _refused(lib, lib.oai_point_footprint(d, 0, d, 4, 1.0, d, d, d, None), b"oai_point_footprint", b"source points")
    _refused(lib, lib.oai_point_footprint(d, -3, d, 4, 1.0, d, d, d, None), b"source points")
    _refused(lib, lib.oai_point_footprint(d, 4, d, -1, 1.0, d, d, d, None), b"negative")
    _refused(lib, lib.oai_point_footprint(d, 4, d, 4, -1.0, d, d, d, None), b"radius")
    _refused(lib, lib.oai_point_footprint(d, 4, d, 4, float("nan"), d, d, d, None), b"radius")
    big = 1 << 20
    _refused(lib, lib.oai_point_footprint_grid(None, 4, d, 4, 1.0, lo, 1.0, dims, d, big, d, d, d, None), b"oai_point_footprint_grid", b"null")
    _refused(lib, lib.oai_point_footprint_grid(d, 4, d, 4, 1.0, None, 1.0, dims, d, big, d, d, d, None), b"null")
    _refused(lib, lib.oai_point_footprint_grid(d, 4, d, 4, 1.0, lo, 1.0, dims, None, big, d, d, d, None), b"null")
    _refused(lib, lib.oai_point_footprint_grid(d, 4, d, 4, 1.0, lo, 1.0, dims, d, big, d, d, None, None), b"null")
    _refused(lib, lib.oai_point_footprint_grid(d, 0, d, 4, 1.0, lo, 1.0, dims, d, big, d, d, d, None), b"oai_point_footprint_grid", b"source points")
    _refused(lib, lib.oai_point_footprint_grid(d, 4, d, -1, 1.0, lo, 1.0, dims, d, big, d, d, d, None), b"negative")
    _refused(lib, lib.oai_point_footprint_grid(d, 4, d, 4, 1.0, lo, 0.5, dims, d, big, d, d, d, None), b"cell_size")
    _refused(lib, lib.oai_point_footprint_grid(d, 4, d, 4, 1.0, lo, 1.0, (C.c_int * 3)(4, 0, 4), d, big, d, d, d, None), b"empty grid")
    assert lib.oai_point_grid_workspace_bytes(dims, 1000) > 16
    _refused(lib, lib.oai_point_footprint_grid(d, 1000, d, 4, 1.0, lo, 1.0, dims, d, 16, d, d, d, None), b"oai_point_footprint_grid", b"workspace")


def test_region_stats_argument_checks(lib):
    d = (C.c_float * 16)()
    assert lib.oai_region_stats_workspace_bytes(-1, 1) == 0
    assert lib.oai_region_stats_workspace_bytes(10, 0) == 0 and lib.oai_region_stats_workspace_bytes(10, 65) == 0
    assert lib.oai_region_stats_workspace_bytes(10, 64) >= 64 * 12 * 8
    assert lib.oai_region_stats_workspace_bytes(1024 * 257 + 3, 3) >= 258 * 3 * 12 * 8
    big = 1 << 20
    _refused(lib, lib.oai_region_stats(None, d, d, d, 10, 1, d, big, d, None), b"oai_region_stats", b"null")
    _refused(lib, lib.oai_region_stats(d, None, d, d, 10, 1, d, big, d, None), b"null")
    _refused(lib, lib.oai_region_stats(d, d, None, None, 10, 1, None, big, d, None), b"null")
    _refused(lib, lib.oai_region_stats(d, d, None, None, 10, 1, d, big, None, None), b"null")
    _refused(lib, lib.oai_region_stats(d, d, d, d, -1, 1, d, big, d, None), b"oai_region_stats", b"negative")
    _refused(lib, lib.oai_region_stats(d, d, d, d, 10, 0, d, big, d, None), b"n_regions", b"got 0")
    _refused(lib, lib.oai_region_stats(d, d, d, d, 10, 65, d, big, d, None), b"n_regions", b"got 65")
    _refused(lib, lib.oai_region_stats(d, d, None, None, 5000, 3, d, 16, d, None), b"oai_region_stats", b"workspace")


def test_the_python_wrappers_refuse_before_the_library(lib):
    from oai_analysis_2_amd import mesh_processing as mp
    import numpy as np
    with pytest.raises(ValueError, match="no source points"):
        mp.point_footprint(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.float32))
