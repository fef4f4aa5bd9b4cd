"""CPU: the cohort-PCA entry points of the C ABI (include/oai_hip.h, "Cohort PCA") are declared, exported by the built library and bound
in _lib.SIGNATURES, the header states the definitions word for word, and every entry point refuses bad arguments with a status and a
message that names the argument -- on host buffers, so no GPU is touched before the checks."""
import ctypes as C
import os
import re

import pytest

from abi_cases import ROOT, check_reexported, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_cohort_whiten", "oai_rows_cross", "oai_rows_cross_workspace_bytes", "oai_rows_combine")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    section = " ".join(_section(raw, "Cohort PCA (csrc/cohort_pca.hip").replace("\n *", " ").split())
    for words in ("tests/cohort_pca_ref.py", "csrc/cohort_pca.hip",
                  "Y: float32 [N][V], knee-major.",
                  "M: uint8 mask, may be null. Validity is as everywhere else: the mask is non-zero and the value is not NaN.",
                  "mean: float64 [V].",
                  "rw: float64 [V], the root weights, sqrt(area in mm^2). The host takes the square root with np.sqrt, so the device takes no "
                  "square root.",
                  "Whitening. a_iv = ((double)Y_iv - mean_v) * rw_v is one subtraction followed by one product.",
                  "Where the entry is missing or rw_v == 0, a_iv is exactly 0.0 by a select, never by a product.",
                  "A vertex with no valid knee has a NaN mean and must not leak.",
                  "Ordered dot. C_ij = sum over v of a_iv * b_jv. The order is the contract:",
                  "The vertex axis is cut into chunks of 512 consecutive vertices. The last chunk is short.",
                  "Inside a chunk, the terms are added in ascending v into one accumulator that starts at 0.0. It is a product, then an add, "
                  "with no FMA.",
                  "The chunk sums are then added in ascending chunk index into one accumulator that starts at 0.0.",
                  "The float64 product is commutative, so C of (A, A) is symmetric to the bit.",
                  "The vector fp64 MFMA is deliberately not used. Its internal summation order cannot be restated in numpy.",
                  "Ordered combine. R_cv = sum over i of k_ci * a_iv, summed over ascending i into one accumulator, product then add.",
                  "norm2_i = sum over v of a_iv^2 in the ordered-dot order",
                  "it computes only the tiles on or above the diagonal and mirrors them",
                  "Walk: one workgroup per 64 x 64 output tile walks all chunks, no workspace.",
                  "a finish kernel adds the chunk sums in ascending chunk index",
                  "Both forms give the same bits by construction.",
                  "Mean imputation", "n_missing and n_excluded", "No leave-one-out member scores.", "No choice of K and no parallel analysis.",
                  "eigh on the host.", "Degenerate (equal) eigenvalues leave their modes defined only up to rotation.", "No fp64 MFMA path.",
                  "No thresholds."):
        assert words in section, words


def test_the_kernels_limits_are_the_ones_the_python_layer_and_the_tests_name():
    from oai_analysis_2_amd import ops
    src = open(os.path.join(ROOT, "oai_analysis_2_amd", "csrc", "cohort_pca.hip")).read()
    shared = open(os.path.join(ROOT, "oai_analysis_2_amd", "csrc", "cohort.h")).read()
    assert re.search(rf"constexpr int kDotChunk = {ops.DOT_CHUNK};", shared)
    assert re.search(rf"constexpr int kTile = {ops.CROSS_TILE};", src) and re.search(r"constexpr int kOwn = 4;", src)
    assert re.search(rf"constexpr int kSplitMaxTiles = {ops.CROSS_SPLIT_MAX_TILES};", src)
    assert "#pragma clang fp contract(off)" in src and "__builtin_amdgcn_mfma" not in src


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_cohort_whiten_argument_checks(lib):
    d = (C.c_double * 64)()                                               # a host buffer: every call below must fail before it is read
    call = lib.oai_cohort_whiten
    #    values mask mean rw N V out norm2 stream
    _refused(lib, call(None, None, d, d, 4, 10, d, None, None), b"oai_cohort_whiten", b"values_dev", b"null")
    _refused(lib, call(d, None, None, d, 4, 10, d, None, None), b"oai_cohort_whiten", b"mean_dev", b"null")
    _refused(lib, call(d, d, d, None, 4, 10, d, d, None), b"root_weight_dev", b"null")
    _refused(lib, call(d, None, d, d, 4, 10, None, d, None), b"out_dev", b"null")
    _refused(lib, call(d, None, d, d, 0, 10, d, None, None), b"oai_cohort_whiten", b"n_knees", b"got 0, 10")
    _refused(lib, call(d, None, d, d, (1 << 24) + 1, 10, d, None, None), b"n_knees", b"16777217")
    _refused(lib, call(d, None, d, d, 4, 0, d, None, None), b"n_verts", b"got 4, 0")
    _refused(lib, call(d, None, d, d, 4, (1 << 31) - 1, d, None, None), b"n_verts", b"2147483647")
    _refused(lib, call(d, None, d, d, 4, -3, d, None, None), b"n_verts", b"-3")


def test_rows_cross_argument_checks(lib):
    d = (C.c_double * 64)()
    call, size = lib.oai_rows_cross, lib.oai_rows_cross_workspace_bytes
    #    a n_a b n_b V out workspace bytes stream
    _refused(lib, call(None, 4, d, 4, 10, d, None, 0, None), b"oai_rows_cross", b"a_dev", b"null")
    _refused(lib, call(d, 4, None, 4, 10, d, None, 0, None), b"oai_rows_cross", b"b_dev", b"null")
    _refused(lib, call(d, 4, d, 4, 10, None, None, 0, None), b"out_dev", b"null")
    _refused(lib, call(d, 0, d, 4, 10, d, None, 0, None), b"oai_rows_cross", b"n_a", b"got 0")
    _refused(lib, call(d, (1 << 20) + 1, d, 4, 10, d, None, 0, None), b"n_a", b"1048577")
    _refused(lib, call(d, 4, d, 0, 10, d, None, 0, None), b"oai_rows_cross", b"n_b", b"got 0")
    _refused(lib, call(d, 4, d, (1 << 20) + 1, 10, d, None, 0, None), b"n_b", b"1048577")
    _refused(lib, call(d, 4, d, 4, 0, d, None, 0, None), b"n_verts", b"got 0")
    _refused(lib, call(d, 4, d, 4, (1 << 31) - 1, d, None, 0, None), b"n_verts", b"2147483647")
    # the split form: 2 x 3 tiles, 3 chunks of 64 x 64 doubles each
    need = 2 * 3 * 3 * 64 * 64 * 8
    assert size(65, 130, 1025) == need and size(4, 4, 512) == 64 * 64 * 8 and size(4, 4, 513) == 2 * 64 * 64 * 8
    assert size(0, 4, 10) == 0 and size(4, 4, 0) == 0 and size(4, (1 << 20) + 1, 10) == 0
    assert size(16 * 64, 16 * 64, 10) == 256 * 64 * 64 * 8 and size(16 * 64 + 1, 16 * 64, 10) == 0      # more than 256 tiles: it walks
    _refused(lib, call(d, 65, d, 130, 1025, d, d, need - 1, None), b"oai_rows_cross", b"workspace", str(need - 1).encode(), str(need).encode())
    _refused(lib, call(d, 4, d, 4, 10, d, d, 0, None), b"oai_rows_cross", b"workspace")


def test_rows_combine_argument_checks(lib):
    d = (C.c_double * 64)()
    call = lib.oai_rows_combine
    #    coef rows n_out n_rows V out stream
    _refused(lib, call(None, d, 2, 4, 10, d, None), b"oai_rows_combine", b"coef_dev", b"null")
    _refused(lib, call(d, None, 2, 4, 10, d, None), b"oai_rows_combine", b"rows_dev", b"null")
    _refused(lib, call(d, d, 2, 4, 10, None, None), b"out_dev", b"null")
    _refused(lib, call(d, d, 0, 4, 10, d, None), b"oai_rows_combine", b"n_out", b"got 0")
    _refused(lib, call(d, d, (1 << 20) + 1, 4, 10, d, None), b"n_out", b"1048577")
    _refused(lib, call(d, d, 2, 0, 10, d, None), b"oai_rows_combine", b"n_rows", b"got 0")
    _refused(lib, call(d, d, 2, (1 << 20) + 1, 10, d, None), b"n_rows", b"1048577")
    _refused(lib, call(d, d, 2, 4, 0, d, None), b"n_verts", b"got 0")
    _refused(lib, call(d, d, 2, 4, -1, d, None), b"n_verts", b"-1")


def test_the_names_are_exported_where_the_other_statistics_are():
    from oai_analysis_2_amd import dask_processing, ops, stats
    check_reexported(("ThicknessPCA", "PCAScores"))
    for name in ("fit", "transform", "member_scores", "reconstruct", "image", "save", "load"):
        assert callable(getattr(stats.ThicknessPCA, name))
    assert callable(stats.ThicknessCohort.pca) and callable(dask_processing.pca_stream)
    for name in ("cohort_whiten", "rows_cross", "rows_cross_workspace", "rows_combine"):
        assert callable(getattr(ops, name))
    assert (ops.DOT_CHUNK, ops.CROSS_TILE, ops.CROSS_SPLIT_MAX_TILES) == (512, 64, 256) and stats.PCA_DROP == 1e-12
