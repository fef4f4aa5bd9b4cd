"""CPU: the TFCE entry points of the C ABI (include/oai_hip.h: oai_graph_tfce) are exported by the built library and refuse bad arguments
with a status and a message -- no GPU is touched before the checks -- and the Python layer refuses the same before the library."""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import BIG, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_graph_tfce_workspace_bytes", "oai_graph_tfce")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)                      # a #define counts outside the comments only
    section = _section(raw, "Threshold-free cluster enhancement")
    for words in ("csrc/graph_tfce.hip", "tests/graph_tfce_ref.py", "k = K(v) down to 1", "c_k = (eE * hH) * dh", "NOT pinned to any implementation",
                  "a >= (double)(max_steps + 1) * dh"):
        assert words in section, words
    for name, value in (("OAI_TFCE_E_HALF", 0), ("OAI_TFCE_E_ONE", 1), ("OAI_TFCE_H_ONE", 0), ("OAI_TFCE_H_TWO", 1)):
        assert re.search(rf"#define {name} {value}\b", text), name
        from oai_analysis_2_amd import ops
        assert getattr(ops, name) == value


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_graph_tfce_argument_checks(lib):
    d = (C.c_float * 16)()                                                # a host buffer: every call below must fail before it is read
    size = lib.oai_graph_tfce_workspace_bytes
    assert size(0, 10) == 0 and size(4, 0) == 0 and size(-4, 10) == 0 and size((1 << 20) + 1, 10) == 0 and size(4, (1 << 31) - 1) == 0
    assert size(64, 30000) >= 64 * 30000 * (4 + 4 + 8)

    def call(values=d, rows=2, verts=10, offsets=d, neighbours=d, n_nbrs=18, weight=None, unit=1.0, dh=0.1, e=1, h=1, steps=100, ws=d,
             ws_bytes=BIG, out=d, clipped=d):
        return lib.oai_graph_tfce(values, rows, verts, offsets, neighbours, n_nbrs, weight, unit, dh, e, h, steps, ws, ws_bytes, out, clipped, None)
    for null in ("values", "offsets", "neighbours", "ws", "out", "clipped"):
        _refused(lib, call(**{null: None}), b"oai_graph_tfce", b"null")
    for dh in (0.0, -0.1, float("nan"), float("inf")):
        _refused(lib, call(dh=dh), b"oai_graph_tfce", b"dh")
    _refused(lib, call(unit=0.0), b"unit")
    _refused(lib, call(unit=-1.0), b"unit")
    _refused(lib, call(unit=float("nan")), b"unit")
    _refused(lib, call(e=2), b"e_mode", b"got 2")
    _refused(lib, call(e=-1), b"e_mode", b"got -1")
    _refused(lib, call(h=2), b"h_mode", b"got 2")
    _refused(lib, call(h=-1), b"h_mode", b"got -1")
    _refused(lib, call(steps=0), b"max_steps", b"got 0")
    _refused(lib, call(steps=65537), b"max_steps", b"got 65537")
    _refused(lib, call(rows=0), b"rows", b"got 0")
    _refused(lib, call(rows=(1 << 20) + 1), b"rows")
    _refused(lib, call(verts=-10), b"vertices", b"-10")
    _refused(lib, call(verts=0), b"vertices")
    _refused(lib, call(n_nbrs=-18), b"negative", b"-18")
    _refused(lib, call(verts=3000, ws_bytes=16), b"oai_graph_tfce", b"workspace")


def test_the_python_layer_refuses_before_the_library():
    from oai_analysis_2_amd import stats
    for bad, match in ((stats.TFCE(E=0.7), "E must be"), (stats.TFCE(H=3.0), "H must be"), (stats.TFCE(dh=0), "dh"), (stats.TFCE(dh=float("inf")), "dh"),
                       (stats.TFCE(extent="volume"), "extent"), (stats.TFCE(max_steps=0), "max_steps"), ("yes", "tfce must be")):
        with pytest.raises(ValueError, match=match):
            stats._tfce_settings(bad)
    assert stats._tfce_settings(None) is None and stats._tfce_settings(True) == stats.TFCE(0.1, 1.0, 2.0, "area", 1000)
    w = stats.tfce_weights(np.array([0.5, 2.0 ** -21, 3.0 * 2.0 ** -21, 1.0]))
    assert w.dtype == np.int64 and w.tolist() == [1 << 19, 0, 2, 1 << 20]          # round half to even
    with pytest.raises(ValueError, match="2\\^53"):
        stats.tfce_weights(np.array([2.0 ** 32, 2.0 ** 32]))
    with pytest.raises(ValueError, match=">= 0"):
        stats.tfce_weights(np.array([1.0, -1.0]))


def test_the_batch_sizes_count_the_tfce_tile_and_keep_their_old_values():
    from oai_analysis_2_amd import stats
    V, P = 30002, 100000
    assert stats.default_batch(V, P, False) == (256 << 20) // (V * 8) // 16 * 16 == 1104
    assert stats.default_batch(V, P, True) == (256 << 20) // (V * 16) // 16 * 16 == 544
    assert stats.default_batch(V, P, False, tfce=True) == (256 << 20) // (V * 32) // 16 * 16 == 272
    assert stats.default_batch(V, P, True, tfce=True) == (256 << 20) // (V * 40) // 16 * 16
    assert stats.default_batch(V, P, False, 64 << 20, True) == (64 << 20) // (V * 32) // 16 * 16
    assert stats.regression_batch(V, 200, 3, P, False) == (256 << 20) // (V * 8 + 200 * 8 * 9) // 16 * 16
    assert stats.regression_batch(V, 200, 3, P, False, tfce=True) == (256 << 20) // (V * 32 + 200 * 8 * 9) // 16 * 16
    assert stats.regression_batch(V, 200, 3, P, True, tfce=True) < stats.regression_batch(V, 200, 3, P, True)


def test_a_result_hands_its_tfce_maps_to_the_atlas_image():
    from oai_analysis_2_amd import stats

    class Atlas:
        def image(self, vector, kind):
            return kind, vector

    v = np.array([1.0, np.nan, -2.0])
    res = stats.PermutationResult("TC", v, v, v, v, v, v, v, 10, False)
    assert res.tfce is None and res.p_tfce is None and res.tfce_clipped == 0 and res.tfce_settings is None
    with pytest.raises(ValueError, match="without tfce"):
        res.image(Atlas(), "p_tfce")
    res.tfce, res.p_tfce = v * 3, v + 1
    assert np.array_equal(res.image(Atlas(), "tfce")[1], (v * 3).astype(np.float32), equal_nan=True)
    assert np.array_equal(res.image(Atlas(), "p_tfce")[1], (v + 1).astype(np.float32), equal_nan=True)
    reg = stats.RegressionResult("TC", v, v, v, v, v, v, v, v, 10, False)
    with pytest.raises(ValueError, match="without tfce"):
        reg.image(Atlas(), "tfce")
