"""CPU: the normative-deviation entry points of the C ABI (include/oai_hip.h: oai_normative_fit, oai_normative_score,
oai_deviation_summary and their workspace sizes) are declared, exported and bound, the header section states the formulas and both
conditions, and every refusal is a status and a message -- no GPU is touched before the checks."""
import ctypes as C
import os

import pytest

from abi_cases import BIG, ROOT, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_normative_fit", "oai_normative_score", "oai_deviation_summary", "oai_normative_fit_workspace_bytes",
       "oai_normative_score_workspace_bytes", "oai_deviation_summary_workspace_bytes")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    section = _section(raw, "Normative deviation (csrc/normative.hip")
    for words in ("tests/normative_ref.py", "ASCENDING KNEE INDEX", "INTERCEPT (if any) COUNTED IN p",
                  "A_ac = sum_i (m_i ? z_ia*z_ic : 0.0), c <= a", "h_a = sum_i (m_i ? z_ia*y_i : 0.0)",
                  "pivot s is accepted iff s > 1e-10 * A_aa", "e_i  = y_i - sum_a z_ia*gamma_a", "rss  = sum_i (m_i ? e_i*e_i : 0.0)",
                  "ok   = every pivot accepted && n - p >= 1", "COMPONENT-MAJOR",
                  "e   = x - sum_a g_a*gamma_a", "L u = g forward", "lev = sum_a u_a*u_a",
                  "dof = n - p;  s2 = rss/dof;  se2 = s2*(1.0 + lev)",
                  "den = 1.0 - lev;  dof = n - p - 1;  s2 = (rss - (e*e)/den)/dof;  se2 = s2*den", "z   = e / sqrt(se2)",
                  "z is valid iff mx && ok && dof >= 1 && s2 > 0 && (loo == 0 || den > 1e-10), otherwise NaN",
                  "den > 1e-10 is A CONDITION and part of the contract", "THE SMALLEST INDEX AT A TIE", "units of 2^-20 mm^2"):
        assert words in section, words
    # the factor and the forward solve are the regression's device code, shared through a header: one copy
    csrc = os.path.join(ROOT, "oai_analysis_2_amd", "csrc")
    for name in ("group_regression.hip", "normative.hip"):
        source = open(os.path.join(csrc, name)).read()
        assert '#include "regression_solve.h"' in source and "bool cholesky(" not in source and "void forward_solve(" not in source, name
    shared = open(os.path.join(csrc, "regression_solve.h")).read()
    assert shared.count("bool cholesky(") == 1 and shared.count("void forward_solve(") == 1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_normative_fit_argument_checks(lib):
    d = (C.c_float * 16)()                                                # a host buffer: every call below must fail before it is read
    size = lib.oai_normative_fit_workspace_bytes
    assert size(0, 3) == 0 and size(-1, 3) == 0 and size(10, 0) == 0 and size(10, 7) == 0 and size(1 << 31, 3) == 0
    assert size(30002, 4) >= (4 + 10 + 1) * 30002 * 8 + 30002 * 5 and size(30002, 4) % 256 == 0
    call = lib.oai_normative_fit
    _refused(lib, call(None, d, d, 4, 10, 2, d, BIG, None), b"oai_normative_fit", b"null")
    _refused(lib, call(d, d, None, 4, 10, 2, d, BIG, None), b"null")
    _refused(lib, call(d, d, d, 4, 10, 2, None, BIG, None), b"null")
    _refused(lib, call(d, None, d, 1, 10, 2, d, BIG, None), b"oai_normative_fit", b"knees", b"got 1")
    _refused(lib, call(d, None, d, 4, -10, 2, d, BIG, None), b"vertices", b"-10")
    _refused(lib, call(d, None, d, 4, 10, 0, d, BIG, None), b"design columns", b"got 0")
    _refused(lib, call(d, None, d, 4, 10, 7, d, BIG, None), b"design columns", b"got 7")
    _refused(lib, call(d, None, d, 4, 10, 2, d, 16, None), b"model block", b"workspace")


def test_normative_score_argument_checks(lib):
    d = (C.c_float * 16)()
    size = lib.oai_normative_score_workspace_bytes
    assert size(0, 10) == 0 and size(-1, 10) == 0 and size(4, 0) == 0 and size((1 << 20) + 1, 10) == 0
    assert size(64, 30002) >= 64 * 30002 * 8
    call = lib.oai_normative_score
    _refused(lib, call(None, BIG, d, d, d, 4, 10, 2, 0, d, BIG, None, None), b"oai_normative_score", b"null")
    _refused(lib, call(d, BIG, None, d, d, 4, 10, 2, 0, d, BIG, None, None), b"null")
    _refused(lib, call(d, BIG, d, d, None, 4, 10, 2, 0, d, BIG, None, None), b"null")
    _refused(lib, call(d, BIG, d, d, d, 4, 10, 2, 0, None, BIG, None, None), b"null")
    _refused(lib, call(d, BIG, d, None, d, 0, 10, 2, 0, d, BIG, None, None), b"rows", b"got 0")
    _refused(lib, call(d, BIG, d, None, d, 4, -1, 2, 0, d, BIG, None, None), b"vertices")
    _refused(lib, call(d, BIG, d, None, d, 4, 10, 7, 0, d, BIG, None, None), b"design columns", b"got 7")
    _refused(lib, call(d, BIG, d, None, d, 4, 10, 0, 0, d, BIG, None, None), b"design columns", b"got 0")
    _refused(lib, call(d, BIG, d, None, d, 4, 10, 2, 2, d, BIG, None, None), b"loo", b"got 2")
    _refused(lib, call(d, BIG, d, None, d, 4, 10, 2, -1, d, BIG, None, None), b"loo", b"got -1")
    _refused(lib, call(d, 16, d, None, d, 4, 10, 2, 0, d, BIG, None, None), b"model block", b"workspace")
    _refused(lib, call(d, BIG, d, None, d, 4, 10, 2, 0, d, 16, None, None), b"oai_normative_score", b"workspace")


def test_deviation_summary_argument_checks(lib):
    d = (C.c_float * 16)()
    size = lib.oai_deviation_summary_workspace_bytes
    assert size(0, 10) == 0 and size(4, 0) == 0 and size(-4, 10) == 0 and size(64, 30002) >= 64 * 9 * 8
    call = lib.oai_deviation_summary
    _refused(lib, call(None, 2, 10, d, 2.0, d, BIG, d, d, None), b"oai_deviation_summary", b"null")
    _refused(lib, call(d, 2, 10, d, 2.0, None, BIG, d, d, None), b"null")
    _refused(lib, call(d, 2, 10, d, 2.0, d, BIG, None, d, None), b"null")
    _refused(lib, call(d, 2, 10, d, 2.0, d, BIG, d, None, None), b"null")
    _refused(lib, call(d, 0, 10, d, 2.0, d, BIG, d, d, None), b"rows", b"got 0")
    _refused(lib, call(d, 2, -10, d, 2.0, d, BIG, d, d, None), b"vertices", b"-10")
    _refused(lib, call(d, 2, 10, d, 0.0, d, BIG, d, d, None), b"threshold")
    _refused(lib, call(d, 2, 10, d, -2.0, d, BIG, d, d, None), b"threshold")
    _refused(lib, call(d, 2, 10, d, float("nan"), d, BIG, d, d, None), b"threshold")
    _refused(lib, call(d, 2, 30002, d, 2.0, d, 16, d, d, None), b"oai_deviation_summary", b"workspace")


def test_a_result_hands_its_maps_to_the_atlas_image():
    import numpy as np
    from oai_analysis_2_amd import stats

    class Atlas:
        def image(self, vector, kind):
            return kind, vector

    one, z = np.zeros(2), np.array([[1.0, np.nan, -2.5], [0.0, 0.5, np.nan]])
    res = stats.DeviationResult("TC", ["a", "b"], False, 2.0, *([one] * 10), np.zeros(3), one, one, one, z=z, diff_mm=z * 0.1, p_uncorrected=z * 0)
    kind, vec = res.image(Atlas(), "diff_mm", knee=1)
    assert kind == "TC" and vec.dtype == np.float32 and np.array_equal(vec, (z[1] * 0.1).astype(np.float32), equal_nan=True) and len(res) == 2
    with pytest.raises(ValueError, match="no image"):
        res.image(Atlas(), "max_abs")
    with pytest.raises(ValueError, match="knee must be"):
        res.image(Atlas(), "z", knee=2)
    bare = stats.DeviationResult("TC", ["a", "b"], False, 2.0, *([one] * 10), np.zeros(3), one, one, one)
    with pytest.raises(ValueError, match="without return_maps"):
        bare.image(Atlas(), "z")
