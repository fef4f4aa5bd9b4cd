"""CPU: the longitudinal entry points of the C ABI (include/oai_hip.h: oai_visit_slopes_workspace_bytes, oai_visit_slopes) are exported by
the built library and refuse bad arguments with a status and a message -- no GPU is touched before the checks."""
import ctypes as C

import pytest

from abi_cases import BIG, check_reexported, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_visit_slopes_workspace_bytes", "oai_visit_slopes")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    assert len(_lib.SIGNATURES["oai_visit_slopes"][1]) == 21 and len(_lib.SIGNATURES["oai_visit_slopes_workspace_bytes"][1]) == 4
    # the header names the kernel file and the restatement and states the three passes, the condition and the outputs
    section = _section(raw, "Longitudinal change")
    section = section[:section.index("oai_visit_slopes(")]
    for words in ("csrc/visit_slopes.hip", "tests/visit_slopes_ref.py", "long_mris_slopes", "AS RECALLED", "pinned to no implementation",
                  "THE SLOTS OF A SUBJECT IN ASCENDING CSR", "an offset outside [0, n_visits] is clamped",
                  "a slot whose row is outside [0, n_rows) is skipped",
                  "pass 1:  n = count;  St = St + t_e;  Sy = Sy + (double)y_e;  tmin, tmax over the valid slots",
                  "tb = St / n;  yb = Sy / n",
                  "pass 2:  dt = t_e - tb;  dy = (double)y_e - yb;  Sxx = Sxx + dt*dt;  Sxy = Sxy + dt*dy",
                  "ok = n >= min_visits && Sxx > 0 && (tmax - tmin) >= min_span",
                  "rate = Sxy / Sxx",
                  "pass 3:  r = dy - rate*dt;  rss = rss + r*r",
                  "avg = yb;  fit_ref = yb + rate * (tref_s - tb)",
                  "resid_sd = n >= 3 ? sqrt(rss / (double)(n - 2)) : NaN",
                  "skipped by a select, never multiplied", "ALWAYS the", "hold +0.0", "exactly where ok is true and n == 2"):
        assert words in section, words


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_size_function_refuses_with_0(lib):
    size = lib.oai_visit_slopes_workspace_bytes
    #            rows, vertices, subjects, visits
    assert size(0, 10, 3, 5) == 0 and size(-1, 10, 3, 5) == 0 and size((1 << 24) + 1, 10, 3, 5) == 0
    assert size(5, 0, 3, 5) == 0 and size(5, -1, 3, 5) == 0 and size(5, (1 << 31) - 1, 3, 5) == 0
    assert size(5, 10, 0, 5) == 0 and size(5, 10, -1, 5) == 0 and size(5, 10, (1 << 24) + 1, 5) == 0
    assert size(5, 10, 3, -1) == 0 and size(5, 10, 3, (1 << 24) + 1) == 0
    assert size(1, 1, 1, 0) > 0                                            # no visit at all is a shape it takes: every count is 0
    assert size(1400, 30002, 200, 1400) >= 200 * 8 + 1400 * 4              # a slot run per subject and a row per slot
    assert size(1 << 24, (1 << 31) - 2, 1 << 24, 1 << 24) >= (1 << 24) * 12


def test_visit_slopes_argument_checks(lib):
    d = (C.c_double * 16)()                                               # a host buffer: every call below must fail before it is read
    call = lib.oai_visit_slopes

    def args(values=d, mask=None, rows=5, verts=10, offsets=d, subjects=3, visit_row=d, visit_time=d, visits=5, reference=d, min_visits=2,
             min_span=0.0, workspace=d, nbytes=BIG):
        return (values, mask, rows, verts, offsets, subjects, visit_row, visit_time, visits, reference, min_visits, min_span, workspace, nbytes,
                d, d, d, d, d, d, None)
    for missing in ("values", "offsets", "visit_row", "visit_time", "reference", "workspace"):
        _refused(lib, call(*args(**{missing: None})), b"oai_visit_slopes", b"null")
    _refused(lib, call(*args(rows=0)), b"oai_visit_slopes", b"n_rows", b"got 0")
    _refused(lib, call(*args(rows=(1 << 24) + 1)), b"oai_visit_slopes", b"n_rows", b"got 16777217")
    _refused(lib, call(*args(verts=0)), b"oai_visit_slopes", b"n_verts", b"got 0")
    _refused(lib, call(*args(verts=-1)), b"oai_visit_slopes", b"n_verts", b"got -1")
    _refused(lib, call(*args(verts=(1 << 31) - 1)), b"oai_visit_slopes", b"n_verts")
    _refused(lib, call(*args(subjects=0)), b"oai_visit_slopes", b"n_subjects", b"got 0")
    _refused(lib, call(*args(subjects=(1 << 24) + 1)), b"oai_visit_slopes", b"n_subjects")
    _refused(lib, call(*args(visits=-1)), b"oai_visit_slopes", b"n_visits", b"got -1")
    _refused(lib, call(*args(visits=(1 << 24) + 1)), b"oai_visit_slopes", b"n_visits")
    _refused(lib, call(*args(min_visits=1)), b"oai_visit_slopes", b"min_visits", b"got 1")
    _refused(lib, call(*args(min_visits=-3)), b"oai_visit_slopes", b"min_visits", b"got -3")
    _refused(lib, call(*args(min_span=-0.5)), b"oai_visit_slopes", b"min_span", b"got -0.5")
    _refused(lib, call(*args(min_span=float("nan"))), b"oai_visit_slopes", b"min_span", b"nan")
    _refused(lib, call(*args(min_span=float("inf"))), b"oai_visit_slopes", b"min_span", b"inf")
    _refused(lib, call(*args(nbytes=16)), b"oai_visit_slopes", b"workspace")
    _refused(lib, call(*args(nbytes=lib.oai_visit_slopes_workspace_bytes(5, 10, 3, 5) - 1)), b"oai_visit_slopes", b"workspace")
    # with no visit the slot arrays may be null: the call then gets as far as the workspace check
    _refused(lib, call(*args(visit_row=None, visit_time=None, visits=0, nbytes=16)), b"oai_visit_slopes", b"workspace")


def test_the_names_are_exported_where_the_other_statistics_are():
    from oai_analysis_2_amd import ops, stats
    check_reexported(("LongitudinalCohort", "visit_table", "one_sample_test", "VisitSlopes"))
    assert stats.VisitSlopes is ops.VisitSlopes
