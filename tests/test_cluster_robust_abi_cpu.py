"""CPU: the cluster-robust entry points of the C ABI (include/oai_hip.h: oai_cluster_prepare, oai_cluster_t) are declared, exported by the
built library and listed in ``_lib.SIGNATURES``; the header states the definition; and every refusal returns a status and a message -- no
GPU is touched before the checks."""
import ctypes as C

import pytest

from abi_cases import BIG, check_reexported, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_cluster_prepare_workspace_bytes", "oai_cluster_prepare", "oai_cluster_t_workspace_bytes", "oai_cluster_t")

DEFINITION = (
    "M_ac = Σ_j (m_j ? d_ja·d_jc : 0.0), j ascending.  M = L Lᵀ.",
    "a = M⁻¹ e_p.  Forward-solve L z = e_p, then back-solve Lᵀ a = z.",
    "w_j = m_j ? Σ_c d_jc·a_c : 0.0, c ascending.",
    "h_sc = Σ (m_j ? d_jc·r_j : 0.0)",
    "k_sc = Σ (m_j ? w_j·d_jc : 0.0)",
    "u_s = Σ (m_j ? w_j·r_j : 0.0)",
    "present_s = any m_j",
    "G = Σ_s present_s.",
    "c = (G/(G−1)) · ((n−1)/(n−p)), each quotient taken in double, then one product.  This is Stata's CR1.",
    "okc = ok && every pivot of M accepted && G ≥ 2 && n − p ≥ 1.",
    "f_s = −1 where bit s of the row is set and +1 otherwise",
    "1. b_c = Σ_s (bit ? −h_sc : h_sc), s ascending.  The negation is exact.  Then forward-solve L z = b and back-solve Lᵀ β = z.",
    "2. For s ascending: e = bit ? −u_s : u_s.  For c ascending, e = e − k_sc·β_c.  Then W = W + e·e.",
    "3. t = β_p / sqrt(c·W).  It is valid iff okc && W > 0, otherwise NaN.",
    "slope0 = β_p and se0 = sqrt(c·W)",
    "A cluster with no valid row at the vertex holds +0.0 throughout and adds +0.0.",
    "THE SAME BITS",
)


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    section = _section(raw, "Cluster-robust regression")
    section = section[:section.index("Threshold-free cluster enhancement")]
    for words in DEFINITION + ("tests/cluster_robust_ref.py", "csrc/cluster_robust.hip", "CLUSTER-MAJOR ORDER", "THE REGRESSOR OF INTEREST IS THE LAST COLUMN",
                               "Liang and Zeger 1986", "Cameron, Gelbach and Miller 2008", "Guillaume et al. 2014", "NOT pinned",
                               "an offset outside [0, n_rows] is clamped", "PIVOT RULE", "H float64\n * [p][n_clusters][n_verts]",
                               "okc uint8 [n_verts]", "NOT part of the contract", "Frisch-Waugh"):
        assert words in section, words


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_cluster_prepare_argument_checks(lib):
    d = (C.c_float * 16)()                                                # a host buffer: every call below must fail before it is read
    size = lib.oai_cluster_prepare_workspace_bytes
    assert size(10, 10, 1, 2) == 0 and size(3, 10, 4, 2) == 0 and size((1 << 20) + 1, 10, 4, 2) == 0 and size(10, 0, 4, 2) == 0
    assert size(10, 10, 4, 0) == 0 and size(10, 10, 4, 7) == 0 and size(10, (1 << 31) - 1, 4, 2) == 0
    N, V, S, p = 1000, 30000, 200, 4
    assert size(N, V, S, p) >= lib.oai_regression_prepare_workspace_bytes(N, V) + (2 * p + 1) * S * V * 8 + 10 * V * 8 + V * 5
    assert size(N, V, S, p) % 256 == 0 and size(1 << 20, 10, 1 << 20, 6) > 0
    call = lib.oai_cluster_prepare
    _refused(lib, call(d, None, d, 10, 10, 4, 2, d, BIG, None), b"oai_cluster_prepare", b"null")
    _refused(lib, call(d, d, None, 10, 10, 4, 2, d, BIG, None), b"null")
    _refused(lib, call(d, d, d, 10, 10, 4, 2, None, BIG, None), b"null")
    _refused(lib, call(None, d, d, 10, 10, 1, 2, d, BIG, None), b"oai_cluster_prepare", b"at least 2 clusters", b"got 1")
    _refused(lib, call(None, d, d, 10, 10, -2, 2, d, BIG, None), b"clusters", b"got -2")
    _refused(lib, call(None, d, d, 10, 10, 4, 0, d, BIG, None), b"1 .. 6 design columns", b"got 0")
    _refused(lib, call(None, d, d, 10, 10, 4, 7, d, BIG, None), b"columns", b"got 7")
    _refused(lib, call(None, d, d, (1 << 20) + 1, 10, 4, 2, d, BIG, None), b"2^20 rows", str((1 << 20) + 1).encode())
    _refused(lib, call(None, d, d, 3, 10, 4, 2, d, BIG, None), b"fewer rows than clusters", b"n_rows 3 < n_clusters 4")
    _refused(lib, call(None, d, d, 10, 0, 4, 2, d, BIG, None), b"vertices", b"got 0")
    _refused(lib, call(None, d, d, 10, 10, 4, 2, d, 16, None), b"oai_cluster_prepare", b"workspace")


def test_cluster_t_argument_checks(lib):
    d = (C.c_float * 16)()
    size = lib.oai_cluster_t_workspace_bytes
    assert size(0, 10) == 0 and size(-1, 10) == 0 and size(4, 0) == 0 and size((1 << 20) + 1, 10) == 0
    assert size(64, 30000) == 64 * 30000 * 8 and size(3, 5) == 256
    call = lib.oai_cluster_t
    _refused(lib, call(None, BIG, d, 10, 10, 4, 2, 0, 2, d, BIG, None, None, None), b"oai_cluster_t", b"null")
    _refused(lib, call(d, BIG, None, 10, 10, 4, 2, 0, 2, d, BIG, None, None, None), b"null")
    _refused(lib, call(d, BIG, d, 10, 10, 4, 2, 0, 2, None, BIG, None, None, None), b"null")
    _refused(lib, call(d, BIG, d, 10, 10, 1, 2, 0, 2, d, BIG, None, None, None), b"oai_cluster_t", b"at least 2 clusters", b"got 1")
    _refused(lib, call(d, BIG, d, 10, 10, 4, 7, 0, 2, d, BIG, None, None, None), b"columns", b"got 7")
    _refused(lib, call(d, BIG, d, (1 << 20) + 1, 10, 4, 2, 0, 2, d, BIG, None, None, None), b"2^20 rows")
    _refused(lib, call(d, BIG, d, 3, 10, 4, 2, 0, 2, d, BIG, None, None, None), b"fewer rows than clusters")
    _refused(lib, call(d, BIG, d, 10, -1, 4, 2, 0, 2, d, BIG, None, None, None), b"vertices")
    _refused(lib, call(d, BIG, d, 10, 10, 4, 2, 2, 2, d, BIG, None, None, None), b"rows", b"2, 2")
    _refused(lib, call(d, BIG, d, 10, 10, 4, 2, -1, 1, d, BIG, None, None, None), b"rows")
    _refused(lib, call(d, BIG, d, 10, 10, 4, 2, 0, (1 << 20) + 1, d, BIG, None, None, None), b"rows")
    _refused(lib, call(d, 16, d, 10, 10, 4, 2, 0, 2, d, BIG, None, None, None), b"cluster block", b"workspace")
    _refused(lib, call(d, BIG, d, 10, 10, 4, 2, 0, 2, d, 16, None, None, None), b"oai_cluster_t", b"workspace")


def test_the_names_are_exported_where_the_other_statistics_are():
    from oai_analysis_2_amd import ops
    check_reexported(("MarginalResult", "marginal_test"))
    assert callable(ops.cluster_prepare) and callable(ops.cluster_t)
