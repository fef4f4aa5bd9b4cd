"""CPU: the bootstrap entry points of the C ABI (include/oai_hip.h, "Bootstrap intervals") are declared, exported by the built library and
bound in _lib.SIGNATURES, the header states the contract word for word, and every entry point refuses bad arguments with a status and a
message that names it -- on host buffers, so no GPU is touched before the checks."""
import ctypes as C

import pytest

from abi_cases import BIG, check_reexported, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_bootstrap_coef_workspace_bytes", "oai_bootstrap_coef", "oai_bootstrap_moments", "oai_column_quantiles_workspace_bytes",
       "oai_column_quantiles", "oai_bootstrap_sup", "oai_jackknife_acceleration")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    section = _section(raw, "Bootstrap intervals")
    for words in ("tests/bootstrap_ref.py", "csrc/bootstrap.hip", "Efron 1987", "Davison", "NOT pinned", "ASCENDING INDEX",
                  "w_i  = m_iv ? (double)c_ri : 0.0", "u_i  = w_i * (double)y_iv", "h_a  = h_a + g_ia * u_i", "M_ac = M_ac + w_i * G_iac",
                  "product THEN an add", "not an fma", "theta = z_p / L_pp", "THE SAME BITS", "24 + 16 bits", "never multiplied in",
                  "B' = the number of finite entries", "NaN for B' < 2", "below = #{theta* < theta^}", "equal = #{theta* == theta^}",
                  "vi = (double)(n' - 1) * q", "fl = floor(vi)", "gamma = vi - fl", "a + (b - a)*t for t < 0.5, else b - (b - a)*(1 - t)",
                  "-0.0 sorts before +0.0", "ONE PATH FOR EVERY", "|theta*_rv - theta^_v| / se_v", "sup[r] = max(sup[r], sup_r)",
                  "U_i = (double)(n_s - 1) * (mean_s - theta_(i))", "a = (num / (den * sqrt(den))) / 6.0", "scipy.stats.bootstrap",
                  "counts_dev uint16 [R][n_knees]", "pivot rule"):
        assert words in section, words


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_bootstrap_coef_argument_checks(lib):
    d = (C.c_float * 16)()                                                # a host buffer: every call below must fail before it is read
    size = lib.oai_bootstrap_coef_workspace_bytes
    assert size(0, 10, 4, 2) == 0 and size(-1, 10, 4, 2) == 0 and size(4, 0, 4, 2) == 0 and size((1 << 20) + 1, 10, 4, 2) == 0
    assert size(4, 10, 1, 2) == 0 and size(4, 10, (1 << 24) + 1, 2) == 0 and size(4, 10, 4, 0) == 0 and size(4, 10, 4, 7) == 0
    assert size(2001, 30002, 200, 4) >= 2001 * 30002 * 8 + 200 * 14 * 8 + 2001 * 200 * 8 and size(2001, 30002, 200, 4) % 256 == 0
    assert size(1, 1, 2, 1) % 256 == 0 and size(1, 1, 2, 1) > 0
    call = lib.oai_bootstrap_coef
    #    y  mask design counts N  V  p v0 v1 r0 r1 ws  bytes n  ok stream
    _refused(lib, call(None, d, d, d, 4, 10, 2, 0, 10, 0, 2, d, BIG, d, d, None), b"oai_bootstrap_coef", b"null")
    _refused(lib, call(d, d, None, d, 4, 10, 2, 0, 10, 0, 2, d, BIG, d, d, None), b"oai_bootstrap_coef", b"null")
    _refused(lib, call(d, d, d, None, 4, 10, 2, 0, 10, 0, 2, d, BIG, d, d, None), b"null")
    _refused(lib, call(d, d, d, d, 4, 10, 2, 0, 10, 0, 2, None, BIG, d, d, None), b"null")
    _refused(lib, call(d, None, d, d, 1, 10, 2, 0, 10, 0, 2, d, BIG, None, None, None), b"oai_bootstrap_coef", b"knees", b"got 1")
    _refused(lib, call(d, None, d, d, (1 << 24) + 1, 10, 2, 0, 10, 0, 2, d, BIG, None, None, None), b"knees")
    _refused(lib, call(d, None, d, d, 4, 0, 2, 0, 10, 0, 2, d, BIG, None, None, None), b"vertices")
    _refused(lib, call(d, None, d, d, 4, 10, 0, 0, 10, 0, 2, d, BIG, None, None, None), b"columns", b"got 0")
    _refused(lib, call(d, None, d, d, 4, 10, 7, 0, 10, 0, 2, d, BIG, None, None, None), b"columns", b"got 7")
    _refused(lib, call(d, None, d, d, 4, 10, 2, 0, 10, 2, 2, d, BIG, None, None, None), b"rows", b"2, 2")
    _refused(lib, call(d, None, d, d, 4, 10, 2, 0, 10, -1, 2, d, BIG, None, None, None), b"rows")
    _refused(lib, call(d, None, d, d, 4, 10, 2, 0, 10, 0, (1 << 20) + 1, d, BIG, None, None, None), b"rows")
    _refused(lib, call(d, None, d, d, 4, 10, 2, -1, 10, 0, 2, d, BIG, None, None, None), b"oai_bootstrap_coef", b"span", b"-1, 10")
    _refused(lib, call(d, None, d, d, 4, 10, 2, 5, 5, 0, 2, d, BIG, None, None, None), b"span", b"5, 5")
    _refused(lib, call(d, None, d, d, 4, 10, 2, 0, 11, 0, 2, d, BIG, None, None, None), b"span", b"0, 11")
    _refused(lib, call(d, None, d, d, 4, 10, 2, 0, 10, 0, 2, d, 16, None, None, None), b"oai_bootstrap_coef", b"workspace")


def test_moments_sup_and_acceleration_argument_checks(lib):
    d = (C.c_float * 16)()
    call = lib.oai_bootstrap_moments
    _refused(lib, call(None, 4, 10, d, d, d, d, d, None), b"oai_bootstrap_moments", b"null")
    _refused(lib, call(d, 4, 10, d, d, None, d, d, None), b"oai_bootstrap_moments", b"null")
    _refused(lib, call(d, 0, 10, d, d, d, d, d, None), b"oai_bootstrap_moments", b"rows", b"got 0")
    _refused(lib, call(d, (1 << 20) + 1, 10, d, d, d, d, d, None), b"rows")
    _refused(lib, call(d, 4, 0, d, d, d, d, d, None), b"vertices")
    call = lib.oai_bootstrap_sup
    _refused(lib, call(None, 4, 10, d, d, None), b"oai_bootstrap_sup", b"null")
    _refused(lib, call(d, 4, 10, None, d, None), b"null")
    _refused(lib, call(d, 4, 10, d, None, None), b"null")
    _refused(lib, call(d, 0, 10, d, d, None), b"oai_bootstrap_sup", b"rows", b"got 0")
    _refused(lib, call(d, 4, -2, d, d, None), b"vertices", b"-2")
    call = lib.oai_jackknife_acceleration
    #    jack mask strata N V v0 v1 S accel stream
    _refused(lib, call(None, None, d, 4, 10, 0, 10, 1, d, None), b"oai_jackknife_acceleration", b"null")
    _refused(lib, call(d, None, None, 4, 10, 0, 10, 1, d, None), b"null")
    _refused(lib, call(d, None, d, 4, 10, 0, 10, 1, None, None), b"null")
    _refused(lib, call(d, None, d, 1, 10, 0, 10, 1, d, None), b"oai_jackknife_acceleration", b"knees", b"got 1")
    _refused(lib, call(d, None, d, 4, 10, 3, 2, 1, d, None), b"span", b"3, 2")
    _refused(lib, call(d, None, d, 4, 10, 0, 11, 1, d, None), b"span")
    _refused(lib, call(d, None, d, 4, 10, 0, 10, 0, d, None), b"strata", b"got 0")
    _refused(lib, call(d, None, d, 4, 10, 0, 10, (1 << 16) + 1, d, None), b"strata")


def test_column_quantiles_argument_checks(lib):
    d = (C.c_float * 16)()
    q = (C.c_double * 4)(0.05, 0.95, 0.5, 0.5)
    size = lib.oai_column_quantiles_workspace_bytes
    assert size(0, 10) == 0 and size((1 << 20) + 1, 10) == 0 and size(4, 0) == 0 and size(4, (1 << 31) - 1) == 0
    assert size(2001, 30002) >= 2001 * 30002 * 8 and size(2001, 30002) % 256 == 0 and size(1, 1) == 256
    call = lib.oai_column_quantiles
    #    tile R V first K host dev ws bytes out count stream
    _refused(lib, call(None, 4, 10, 1, 2, q, None, d, BIG, d, d, None), b"oai_column_quantiles", b"null")
    _refused(lib, call(d, 4, 10, 1, 2, q, None, None, BIG, d, d, None), b"null")
    _refused(lib, call(d, 4, 10, 1, 2, q, None, d, BIG, None, d, None), b"null")
    _refused(lib, call(d, 4, 10, 1, 2, q, None, d, BIG, d, None, None), b"null")
    _refused(lib, call(d, 0, 10, 0, 2, q, None, d, BIG, d, d, None), b"oai_column_quantiles", b"rows", b"got 0")
    _refused(lib, call(d, 4, 0, 1, 2, q, None, d, BIG, d, d, None), b"vertices")
    _refused(lib, call(d, 4, 10, -1, 2, q, None, d, BIG, d, d, None), b"first_row", b"got -1")
    _refused(lib, call(d, 4, 10, 5, 2, q, None, d, BIG, d, d, None), b"first_row", b"got 5")
    _refused(lib, call(d, 4, 10, 1, 0, q, None, d, BIG, d, d, None), b"probabilities", b"got 0")
    _refused(lib, call(d, 4, 10, 1, 5, q, None, d, BIG, d, d, None), b"probabilities", b"got 5")
    _refused(lib, call(d, 4, 10, 1, 2, None, None, d, BIG, d, d, None), b"oai_column_quantiles", b"either")
    _refused(lib, call(d, 4, 10, 1, 2, q, d, d, BIG, d, d, None), b"either")
    _refused(lib, call(d, 4, 10, 1, 2, q, None, d, 16, d, d, None), b"oai_column_quantiles", b"workspace")


def test_the_names_are_exported_where_the_other_statistics_are():
    from oai_analysis_2_amd import ops
    check_reexported(("BootstrapCounts", "BootstrapResult", "bootstrap_counts", "bootstrap_ci"))
    for name in ("bootstrap_coef", "bootstrap_moments", "column_quantiles", "bootstrap_sup", "jackknife_acceleration"):
        assert callable(getattr(ops, name))
