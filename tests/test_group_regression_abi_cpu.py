"""CPU: the cohort-regression entry points of the C ABI (include/oai_hip.h: oai_regression_prepare, oai_regression_t) are exported by the
built library and refuse bad arguments with a status and a message -- no GPU is touched before the checks."""
import ctypes as C

import pytest

from abi_cases import BIG, check_reexported, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_regression_prepare_workspace_bytes", "oai_regression_prepare", "oai_regression_t_workspace_bytes", "oai_regression_t")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    # the header names the restatement, the pivot rule, the order and the t formula
    section = _section(raw, "Cohort regression")
    for words in ("tests/group_regression_ref.py", "csrc/group_regression.hip", "ASCENDING KNEE INDEX", "x LAST", "Freedman and Lane", "Winkler",
                  "NOT pinned", "pivot s is accepted iff s > 1e-10 * A_aa", "s = s - L_ak*L_ak", "h_a = sum_i z_ia*d_i",
                  "r_i = m_i ? d_i - sum_a z_ia*gamma_a : 0.0", "M_ac = sum_j (m_j ? g_ja*g_jc : 0.0)", "b_a = sum_j g_ja*r_j",
                  "rss = Q - sum_a z_a*z_a", "s2 = rss / (double)dof", "t = z_p / sqrt(s2)", "beta = z_p / L_pp", "THE SAME BITS",
                  "fma(G, m ? 1.0 : 0.0, M)", "R float64 [n_knees][n_verts]", "ok uint8 [n_verts]"):
        assert words in section, words


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_regression_prepare_argument_checks(lib):
    d = (C.c_float * 16)()                                                # a host buffer: every call below must fail before it is read
    size = lib.oai_regression_prepare_workspace_bytes
    assert size(1, 10) == 0 and size(-1, 10) == 0 and size(4, 0) == 0 and size(4, -1) == 0 and size((1 << 24) + 1, 10) == 0
    assert size(4, (1 << 31) - 1) == 0
    assert size(200, 30000) >= 200 * 30000 * 8 + 2 * 30000 * 8 + 30000 * 4 + 30000 and size(200, 30000) % 256 == 0
    call = lib.oai_regression_prepare
    _refused(lib, call(None, d, d, 4, 10, 1, 1, d, BIG, None), b"oai_regression_prepare", b"null")
    _refused(lib, call(d, d, d, 4, 10, 1, 1, None, BIG, None), b"null")
    _refused(lib, call(d, None, None, 4, 10, 1, 1, d, BIG, None), b"null")                # nuisance columns announced and not given
    _refused(lib, call(d, None, d, 1, 10, 1, 1, d, BIG, None), b"oai_regression_prepare", b"knees", b"got 1")
    _refused(lib, call(d, None, d, -3, 10, 1, 1, d, BIG, None), b"got -3")
    _refused(lib, call(d, None, d, (1 << 24) + 1, 10, 1, 1, d, BIG, None), b"knees")
    _refused(lib, call(d, None, d, 4, -10, 1, 1, d, BIG, None), b"-10")
    _refused(lib, call(d, None, d, 4, 0, 1, 1, d, BIG, None), b"vertices")
    _refused(lib, call(d, None, d, 4, 10, 6, 1, d, BIG, None), b"nuisance", b"got 6")
    _refused(lib, call(d, None, d, 4, 10, -1, 1, d, BIG, None), b"nuisance", b"got -1")
    _refused(lib, call(d, None, d, 4, 10, 1, 2, d, BIG, None), b"centre", b"got 2")
    _refused(lib, call(d, None, d, 4, 10, 1, -1, d, BIG, None), b"centre", b"got -1")
    _refused(lib, call(d, None, d, 4, 10, 1, 1, d, 16, None), b"oai_regression_prepare", b"workspace")


def test_regression_t_argument_checks(lib):
    d = (C.c_float * 16)()
    size = lib.oai_regression_t_workspace_bytes
    assert size(0, 10, 4, 2) == 0 and size(-1, 10, 4, 2) == 0 and size(4, 0, 4, 2) == 0 and size((1 << 20) + 1, 10, 4, 2) == 0
    assert size(4, 10, 1, 2) == 0 and size(4, 10, (1 << 24) + 1, 2) == 0 and size(4, 10, 4, 0) == 0 and size(4, 10, 4, 7) == 0
    assert size(64, 30000, 200, 4) >= 64 * 30000 * 8 + 64 * 200 * 14 * 8                  # the tile and the permuted design table
    call = lib.oai_regression_t
    _refused(lib, call(None, BIG, d, d, d, 4, 10, 2, 0, 2, d, BIG, None, None), b"oai_regression_t", b"null")
    _refused(lib, call(d, BIG, d, None, d, 4, 10, 2, 0, 2, d, BIG, None, None), b"null")
    _refused(lib, call(d, BIG, d, d, None, 4, 10, 2, 0, 2, d, BIG, None, None), b"null")
    _refused(lib, call(d, BIG, d, d, d, 4, 10, 2, 0, 2, None, BIG, None, None), b"null")
    _refused(lib, call(d, BIG, None, d, d, 1, 10, 2, 0, 2, d, BIG, None, None), b"knees", b"got 1")
    _refused(lib, call(d, BIG, None, d, d, 4, -1, 2, 0, 2, d, BIG, None, None), b"vertices")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 0, 0, 2, d, BIG, None, None), b"columns", b"got 0")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 7, 0, 2, d, BIG, None, None), b"columns", b"got 7")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, 2, 2, d, BIG, None, None), b"rows", b"2, 2")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, 3, 1, d, BIG, None, None), b"rows", b"3, 1")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, -1, 1, d, BIG, None, None), b"rows")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, 0, (1 << 20) + 1, d, BIG, None, None), b"rows")
    _refused(lib, call(d, 16, None, d, d, 4, 10, 2, 0, 2, d, BIG, None, None), b"prepared block", b"workspace")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, 0, 2, d, 16, None, None), b"oai_regression_t", b"workspace")


def test_the_names_are_exported_where_the_other_statistics_are():
    check_reexported(("RegressionResult", "IndexPermutations", "regression_test", "index_permutations"))
