"""CPU: the surface-smoothing entry points of the C ABI (include/oai_hip.h: oai_graph_smooth) are exported by the built library and refuse
bad arguments with a status and a message -- no GPU is touched before the checks."""
import ctypes as C
import os

import pytest

from abi_cases import BIG, ROOT, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_graph_smooth_workspace_bytes", "oai_graph_smooth")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    section = _section(raw, "\n * Surface smoothing (")
    for words in ("csrc/graph_smooth.hip", "tests/graph_smooth_ref.py", "skipped", "ascending", "pinned to no implementation",
                  "num = num + w[e] * x_s[j]", "ok = (fill ? 1 : m_s[i]) && den > 0", "never multiplied by 0"):
        assert words in section, words
    source = open(os.path.join(ROOT, "oai_analysis_2_amd", "csrc", "graph_smooth.hip")).read()
    assert "#pragma clang fp contract(off)" in source


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


BIG = 1 << 40                                                             # a workspace size no check below can find too small


def test_graph_smooth_argument_checks(lib):
    d = (C.c_float * 16)()                                                # a host buffer: every call below must fail before it is read
    size = lib.oai_graph_smooth_workspace_bytes
    assert size(0, 10) == 0 and size(4, 0) == 0 and size(-4, 10) == 0 and size((1 << 20) + 1, 10) == 0 and size(4, (1 << 31) - 1) == 0
    assert 2 * 200 * 30002 * (8 + 1) <= size(200, 30002) <= 2 * 200 * 30002 * (8 + 1) + 4 * 256

    def call(values=d, mask=None, rows=2, verts=10, offsets=d, neighbours=d, n_nbrs=18, edge_w=d, self_w=None, sweeps=3, fill=0, ws=d,
             ws_bytes=BIG, out=d, out_mask=None):
        return lib.oai_graph_smooth(values, mask, rows, verts, offsets, neighbours, n_nbrs, edge_w, self_w, sweeps, fill, ws, ws_bytes, out, out_mask,
                                    None)
    for null in ("values", "offsets", "neighbours", "edge_w", "ws", "out"):
        _refused(lib, call(**{null: None}), b"oai_graph_smooth", b"null")
    _refused(lib, call(sweeps=0), b"sweeps", b"got 0")
    _refused(lib, call(sweeps=4097), b"sweeps", b"got 4097")
    _refused(lib, call(sweeps=-1), b"sweeps", b"got -1")
    _refused(lib, call(fill=2), b"fill", b"got 2")
    _refused(lib, call(fill=-1), b"fill", b"got -1")
    _refused(lib, call(rows=0), b"rows", b"got 0")
    _refused(lib, call(rows=(1 << 20) + 1), b"rows")
    _refused(lib, call(verts=-10), b"vertices", b"-10")
    _refused(lib, call(verts=0), b"vertices")
    _refused(lib, call(verts=(1 << 31) - 1), b"vertices")
    _refused(lib, call(n_nbrs=-18), b"negative", b"-18")
    _refused(lib, call(verts=3000, ws_bytes=16), b"oai_graph_smooth", b"workspace")
    _refused(lib, call(ws_bytes=lib.oai_graph_smooth_workspace_bytes(2, 10) - 1), b"oai_graph_smooth", b"workspace")
