"""CPU: the F-test entry points of the C ABI (include/oai_hip.h: oai_regression_f_workspace_bytes, oai_regression_f) are exported by the
built library and refuse bad arguments with a status and a message -- no GPU is touched before the checks."""
import ctypes as C

import pytest

from abi_cases import BIG, check_reexported, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_regression_f_workspace_bytes", "oai_regression_f")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    assert len(_lib.SIGNATURES["oai_regression_f"][1]) == len(_lib.SIGNATURES["oai_regression_t"][1]) + 1
    # the header names the kernel file and the restatement, where the columns of interest stand, and the arithmetic of F and the coefficients
    section = _section(raw, "Cohort F test")
    section = section[:section.index("oai_regression_f(")]
    for words in ("tests/group_f_ref.py", "csrc/group_regression.hip", "COME LAST", "n_nuisance = q", "RESPONSIBLE FOR HAVING PREPARED WITH THE MATCHING q",
                  "M, b, L, z   as in oai_regression_t", "rss = Q - sum_a z_a*z_a", "ess = sum_{a=q}^{p-1} z_a*z_a", "from +0.0, s = s + z_a*z_a",
                  "dof = n - p;  s2 = rss / (double)dof;  F = (ess / (double)k) / s2",
                  "valid iff ok[v] && every pivot of M accepted && dof >= 1 && s2 > 0, otherwise NaN", "float64 [k][n_verts]",
                  "for a = p-1 down to q { s = z_a;  for j = a+1 .. p-1 ascending: s = s - L_ja*beta_j;  beta_a = s / L_aa }", "THE SAME BITS",
                  "Freedman and Lane", "Winkler", "NOT pinned", "ASCENDING KNEE INDEX"):
        assert words in section, words


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_size_function_refuses_with_0_and_is_the_t_entry_points_otherwise(lib):
    size, size_t = lib.oai_regression_f_workspace_bytes, lib.oai_regression_t_workspace_bytes
    assert size(0, 10, 4, 2) == 0 and size(-1, 10, 4, 2) == 0 and size(4, 0, 4, 2) == 0 and size((1 << 20) + 1, 10, 4, 2) == 0
    assert size(4, -1, 4, 2) == 0 and size(4, (1 << 31) - 1, 4, 2) == 0
    assert size(4, 10, 1, 2) == 0 and size(4, 10, (1 << 24) + 1, 2) == 0 and size(4, 10, 4, 0) == 0 and size(4, 10, 4, 7) == 0
    assert size(64, 30000, 200, 4) >= 64 * 30000 * 8 + 64 * 200 * 14 * 8                  # the tile and the permuted design table
    for shape in ((1, 1, 2, 1), (4, 10, 4, 2), (17, 257, 33, 5), (64, 30000, 200, 4), (1000, 30002, 200, 6), (1 << 20, 3, 2, 6)):
        assert size(*shape) == size_t(*shape) > 0, shape


def test_regression_f_argument_checks(lib):
    d = (C.c_float * 16)()                                                # a host buffer: every call below must fail before it is read
    call = lib.oai_regression_f
    #             prepared, bytes, mask, design, perm, knees, verts, columns, interest, p0, p1, workspace, bytes, coef0, stream
    _refused(lib, call(None, BIG, d, d, d, 4, 10, 2, 1, 0, 2, d, BIG, None, None), b"oai_regression_f", b"null")
    _refused(lib, call(d, BIG, d, None, d, 4, 10, 2, 1, 0, 2, d, BIG, None, None), b"oai_regression_f", b"null")
    _refused(lib, call(d, BIG, d, d, None, 4, 10, 2, 1, 0, 2, d, BIG, None, None), b"null")
    _refused(lib, call(d, BIG, d, d, d, 4, 10, 2, 1, 0, 2, None, BIG, None, None), b"null")
    _refused(lib, call(d, BIG, None, d, d, 1, 10, 2, 1, 0, 2, d, BIG, None, None), b"oai_regression_f", b"knees", b"got 1")
    _refused(lib, call(d, BIG, None, d, d, (1 << 24) + 1, 10, 2, 1, 0, 2, d, BIG, None, None), b"knees")
    _refused(lib, call(d, BIG, None, d, d, 4, -1, 2, 1, 0, 2, d, BIG, None, None), b"vertices")
    _refused(lib, call(d, BIG, None, d, d, 4, 0, 2, 1, 0, 2, d, BIG, None, None), b"vertices")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 0, 1, 0, 2, d, BIG, None, None), b"oai_regression_f", b"columns", b"got 0")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 7, 1, 0, 2, d, BIG, None, None), b"columns", b"got 7")
    for p in (1, 2, 6):
        _refused(lib, call(d, BIG, None, d, d, 8, 10, p, 0, 0, 2, d, BIG, None, None), b"oai_regression_f", b"n_interest", b"got 0")
        _refused(lib, call(d, BIG, None, d, d, 8, 10, p, p + 1, 0, 2, d, BIG, None, None), b"oai_regression_f", b"n_interest", b"got %d" % (p + 1))
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, -1, 0, 2, d, BIG, None, None), b"n_interest", b"got -1")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, 1, 2, 2, d, BIG, None, None), b"oai_regression_f", b"rows", b"2, 2")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, 1, 3, 1, d, BIG, None, None), b"rows", b"3, 1")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, 1, -1, 1, d, BIG, None, None), b"rows")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, 1, 0, (1 << 20) + 1, d, BIG, None, None), b"rows")
    _refused(lib, call(d, 16, None, d, d, 4, 10, 2, 1, 0, 2, d, BIG, None, None), b"oai_regression_f", b"prepared block", b"workspace")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, 1, 0, 2, d, 16, None, None), b"oai_regression_f", b"workspace")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, 2, 0, 2, d, lib.oai_regression_f_workspace_bytes(2, 10, 4, 2) - 1, d, None), b"workspace")


def test_the_names_are_exported_where_the_other_statistics_are():
    check_reexported(("FResult", "f_test", "anova_test"))
