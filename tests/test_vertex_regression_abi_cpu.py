"""CPU: the entry points of the vertex-wise design columns (include/oai_hip.h: oai_regression_vx_prepare, oai_regression_vx_t,
oai_regression_vx_f and their size functions) are declared, exported by the built library and bound in _lib.SIGNATURES, the header states
the contract word for word, and every entry point refuses bad arguments with a status and a message -- no GPU is touched before the
checks."""
import ctypes as C

import pytest

from abi_cases import BIG, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_regression_vx_prepare_workspace_bytes", "oai_regression_vx_prepare", "oai_regression_vx_t_workspace_bytes", "oai_regression_vx_t",
       "oai_regression_vx_f_workspace_bytes", "oai_regression_vx_f")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    assert len(_lib.SIGNATURES["oai_regression_vx_f"][1]) == len(_lib.SIGNATURES["oai_regression_vx_t"][1]) + 1
    section = _section(raw, "Vertex-wise design columns")
    section = section[:section.index("oai_regression_vx_f(")]
    for words in ("tests/vertex_regression_ref.py", "csrc/group_regression_vx.hip",
                  "[ vertex nuisance (s_n) | global nuisance (q_g) | global interest (k_g) |", "vertex interest (s_i) ]", "IN THIS ORDER",
                  "S = s_n + s_i in {1, 2}", "part of\n * the bit contract",
                  "m_i  = my_i && mw_0i (&& mw_1i)", "n_dropped = sum (my_i && !m_i)", "wbar_s = (sum_{m_i} (double)w_si) / (double)n",
                  "THE COMPLETED VALUE", "a centred missing entry is exactly 0.0", "a select, not a subtraction", "With n = 0 every wc is 0.0",
                  "KNEE j OF ROW pi TAKES THE WHOLE\n * DESIGN ROW perm[pi][j]", "WC[s][perm[pi][j]][v]", "UNDER THE IDENTITY ROW",
                  "the exact complete-case fit", "only the null distribution sees the mean-imputed entries",
                  "fma(prod, m ? 1.0 : 0.0, M)", "There is no unmasked fast path", "THE SAME BITS",
                  "n_dropped int32 [n_verts]", "WC float64 [S][n_knees][n_verts]", "Freedman and Lane", "NOT pinned", "ASCENDING KNEE INDEX",
                  "PIVOT RULE"):
        assert words in section, words


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_size_functions_return_0_for_refused_shapes(lib):
    prep, size_t, size_f = lib.oai_regression_vx_prepare_workspace_bytes, lib.oai_regression_vx_t_workspace_bytes, lib.oai_regression_vx_f_workspace_bytes
    assert prep(1, 10, 1) == 0 and prep((1 << 24) + 1, 10, 1) == 0 and prep(4, 0, 1) == 0 and prep(4, (1 << 31) - 1, 1) == 0
    assert prep(4, 10, 0) == 0 and prep(4, 10, 3) == 0 and prep(4, 10, -1) == 0
    # the block of "Cohort regression", then n_dropped, the effective mask and S planes of float64, each on a multiple of 256 bytes
    head = lib.oai_regression_prepare_workspace_bytes(200, 30002)
    for S in (1, 2):
        assert prep(200, 30002, S) == head + (30002 * 4 + 255) // 256 * 256 + (200 * 30002 + 255) // 256 * 256 + (S * 200 * 30002 * 8 + 255) // 256 * 256
    for size in (size_t, size_f):
        assert size(0, 10, 4, 2, 1) == 0 and size(-1, 10, 4, 2, 1) == 0 and size((1 << 20) + 1, 10, 4, 2, 1) == 0
        assert size(4, 0, 4, 2, 1) == 0 and size(4, -1, 4, 2, 1) == 0 and size(4, (1 << 31) - 1, 4, 2, 1) == 0
        assert size(4, 10, 1, 2, 1) == 0 and size(4, 10, (1 << 24) + 1, 2, 1) == 0
        assert size(4, 10, 4, 0, 1) == 0 and size(4, 10, 4, 7, 1) == 0
        assert size(4, 10, 4, 2, 0) == 0 and size(4, 10, 4, 2, 3) == 0 and size(4, 10, 4, 1, 2) == 0
        assert size(64, 30000, 200, 4, 1) >= 64 * 30000 * 8 + 64 * 200 * 10 * 8          # the tile and the table of the 3 global columns
        assert size(1, 1, 2, 1, 1) > 0 and size(1 << 20, 3, 2, 6, 2) > 0
    for shape in ((1, 1, 2, 1, 1), (4, 10, 4, 2, 1), (17, 257, 33, 5, 2), (1000, 30002, 200, 6, 2)):
        assert size_t(*shape) == size_f(*shape) > 0, shape


def test_prepare_argument_checks(lib):
    d = (C.c_float * 16)()                                                # a host buffer: every call below must fail before it is read
    call = lib.oai_regression_vx_prepare
    #             y, mask, w, wmask, nuisance, knees, verts, s_n, s_i, q_g, centre, prepared, bytes, stream
    who = b"oai_regression_vx_prepare"
    _refused(lib, call(None, None, d, None, d, 4, 10, 1, 0, 1, 1, d, BIG, None), who, b"null")
    _refused(lib, call(d, None, None, None, d, 4, 10, 1, 0, 1, 1, d, BIG, None), who, b"null")
    _refused(lib, call(d, None, d, None, None, 4, 10, 1, 0, 1, 1, d, BIG, None), who, b"null")
    _refused(lib, call(d, None, d, None, d, 4, 10, 1, 0, 1, 1, None, BIG, None), who, b"null")
    _refused(lib, call(d, None, d, None, d, 1, 10, 1, 0, 1, 1, d, BIG, None), who, b"knees", b"got 1")
    _refused(lib, call(d, None, d, None, d, 4, 0, 1, 0, 1, 1, d, BIG, None), who, b"vertices")
    for sn, si in ((0, 0), (3, 0), (2, 1), (-1, 1), (1, 2), (0, -1)):
        _refused(lib, call(d, None, d, None, d, 4, 10, sn, si, 1, 1, d, BIG, None), who, b"per-vertex columns", b"s_n = %d, s_i = %d" % (sn, si))
    _refused(lib, call(d, None, d, None, d, 4, 10, 1, 0, 5, 1, d, BIG, None), who, b"nuisance columns", b"1 + 5")
    _refused(lib, call(d, None, d, None, d, 4, 10, 2, 0, 4, 1, d, BIG, None), who, b"nuisance columns", b"2 + 4")
    _refused(lib, call(d, None, d, None, d, 4, 10, 1, 0, -1, 1, d, BIG, None), who, b"nuisance columns")
    _refused(lib, call(d, None, d, None, d, 4, 10, 1, 0, 1, 2, d, BIG, None), who, b"centre")
    _refused(lib, call(d, None, d, None, d, 4, 10, 1, 0, 1, 1, d, 16, None), who, b"workspace")
    _refused(lib, call(d, None, d, None, d, 4, 10, 1, 1, 1, 1, d, lib.oai_regression_vx_prepare_workspace_bytes(4, 10, 1), None), who, b"workspace")


def test_t_and_f_argument_checks(lib):
    d = (C.c_float * 16)()

    def t(prepared=d, pbytes=BIG, design=d, perm=d, knees=4, verts=10, p=2, sn=1, si=0, p0=0, p1=2, ws=d, wbytes=BIG):
        return lib.oai_regression_vx_t(prepared, pbytes, design, perm, knees, verts, p, sn, si, p0, p1, ws, wbytes, None, None)

    def f(prepared=d, pbytes=BIG, design=d, perm=d, knees=4, verts=10, p=2, sn=1, si=0, k=1, p0=0, p1=2, ws=d, wbytes=BIG):
        return lib.oai_regression_vx_f(prepared, pbytes, design, perm, knees, verts, p, sn, si, k, p0, p1, ws, wbytes, None, None)

    for call, who in ((t, b"oai_regression_vx_t"), (f, b"oai_regression_vx_f")):
        _refused(lib, call(prepared=None), who, b"null")
        _refused(lib, call(design=None), who, b"null")
        _refused(lib, call(perm=None), who, b"null")
        _refused(lib, call(ws=None), who, b"null")
        _refused(lib, call(knees=1), who, b"knees", b"got 1")
        _refused(lib, call(knees=(1 << 24) + 1), who, b"knees")
        _refused(lib, call(verts=0), who, b"vertices")
        _refused(lib, call(verts=-1), who, b"vertices")
        _refused(lib, call(p=0), who, b"columns", b"got 0")
        _refused(lib, call(p=7), who, b"columns", b"got 7")
        for sn, si in ((0, 0), (3, 0), (2, 1), (1, 2), (-1, 1)):
            _refused(lib, call(p=6, sn=sn, si=si), who, b"per-vertex columns", b"s_n = %d, s_i = %d" % (sn, si))
        _refused(lib, call(p0=2, p1=2), who, b"rows", b"2, 2")
        _refused(lib, call(p0=3, p1=1), who, b"rows", b"3, 1")
        _refused(lib, call(p0=-1, p1=1), who, b"rows")
        _refused(lib, call(p1=(1 << 20) + 1), who, b"rows")
        _refused(lib, call(pbytes=16), who, b"prepared block", b"workspace")
        _refused(lib, call(pbytes=lib.oai_regression_prepare_workspace_bytes(4, 10)), who, b"prepared block")      # the block without its new arrays
        _refused(lib, call(wbytes=16), who, b"workspace")
        _refused(lib, call(wbytes=lib.oai_regression_vx_t_workspace_bytes(2, 10, 4, 2, 1) - 1), who, b"workspace")
    _refused(lib, t(p=1, sn=1, si=0), b"oai_regression_vx_t", b"no column of interest")
    _refused(lib, t(p=2, sn=2, si=0), b"oai_regression_vx_t", b"no column of interest")
    _refused(lib, f(p=3, sn=1, si=1, k=1), b"oai_regression_vx_f", b"s_i = 1", b"n_interest = 1")
    _refused(lib, f(p=3, sn=1, si=1, k=0), b"oai_regression_vx_f", b"n_interest", b"got 0")
    _refused(lib, f(k=0), b"oai_regression_vx_f", b"n_interest", b"got 0")
    _refused(lib, f(k=-1), b"oai_regression_vx_f", b"n_interest", b"got -1")
    _refused(lib, f(p=4, sn=2, k=3), b"oai_regression_vx_f", b"1 .. 2", b"got 3")
    # the lone per-vertex x has no global column at all: a null design is then what is expected, and the next check is reached
    _refused(lib, lib.oai_regression_vx_t(d, BIG, None, d, 4, 10, 1, 0, 1, 0, 2, d, 16, None, None), b"oai_regression_vx_t", b"workspace")


def test_the_new_arguments_are_where_the_other_statistics_are():
    import inspect
    import oai_analysis_2_amd as pkg
    from oai_analysis_2_amd import ops, stats
    for name in ("regression_test", "f_test", "anova_test"):
        assert getattr(pkg, name) is getattr(stats, name)
        assert inspect.signature(getattr(stats, name)).parameters["vertex_covariates"].default is None
    assert callable(stats.LongitudinalCohort.first_visit) and pkg.LongitudinalCohort is stats.LongitudinalCohort
    for name in ("regression_vx_prepare", "regression_vx_t", "regression_vx_f", "RegressionVxPrepared"):
        assert hasattr(ops, name)
