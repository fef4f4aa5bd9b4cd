"""CPU: the rank-transform entry points of the C ABI (include/oai_hip.h, "Rank transform") are declared, exported by the built library and
bound in _lib.SIGNATURES, the header states the definitions word for word, and every entry point refuses bad arguments with a status and
a message that names the argument -- on host buffers, so no GPU is touched before the checks."""
import ctypes as C
import re

import pytest

from abi_cases import check_reexported, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_column_ranks", "oai_rank_sums", "oai_rank_scores")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)                      # a #define counts outside the comments only
    for name, value in (("OAI_RANK_PLAIN", 0), ("OAI_RANK_SIGNED", 1), ("OAI_SCORE_RANK", 0), ("OAI_SCORE_CENTRED", 1), ("OAI_SCORE_NORMAL", 2)):
        assert re.search(rf"#define {name} {value}\b", text), name
    section = " ".join(_section(raw, "Rank transform (csrc/rank_transform.hip").replace("\n *", " ").split())
    for words in ("tests/rank_transform_ref.py", "csrc/rank_transform.hip",
                  "An entry is valid iff its mask is non-zero (every entry, with a null mask) and its value is not NaN.",
                  "In signed mode the value must also be != 0.0f: scipy's zero_method=\"wilcox\" drops zeros before ranking.",
                  "The key is y in plain mode and fabsf(y) in signed mode.",
                  "Comparison is float < and ==, so -0.0 ties +0.0, and +-inf are ordinary values.",
                  "less_i = #{j: k_j < k_i}", "equal_i = #{j: k_j == k_i} (i itself included)", "twice_rank_i = 2*less_i + equal_i + 1",
                  "twice the midrank of scipy.stats.rankdata(method=\"average\")", "In signed mode the result is negated where y < 0.",
                  "0 where the entry is not valid", "n_valid_dev int32 [n_verts]",
                  "tie_term_dev int64 [n_verts] = sum over valid i of (equal_i^2 - 1), which equals the sum over tie groups of (t^3 - t)",
                  "Kruskal-Wallis and the asymptotic variances use",
                  "Everything is an integer count, so the result does not depend on launch geometry or on the order anything ran in",
                  "1 <= n_knees <= 2^22, so a midrank is exact in float32", "A HOST ARRAY", "1 <= n_groups <= 16",
                  "refused before any launch", "sum of |twice_rank|", "group 0 is the negative entries and group 1 the positive ones",
                  "OAI_SCORE_RANK: 0.5 * twice_rank, sign kept. Exact.", "OAI_SCORE_CENTRED: 0.5 * twice_rank - 0.5 * (n_valid + 1). Exact.",
                  "OAI_SCORE_NORMAL: Phi^-1((r - c) / (n_valid - 2c + 1)) with r = 0.5 * |twice_rank|",
                  "Blom 3/8 (the default of the Python layer), Tukey 1/3, Bliss-Rankit 1/2, van der Waerden 0",
                  "as recalled from PALM's -inormal and is pinned to no implementation", "q = min(p, 1 - p)", "x = -sqrt(-2 ln q)",
                  "2.5 (q - 1/2) when q > 0.2", "u = (F - q) / phi(x), x <- x - u / (1 + x u / 2)", "four Halley steps",
                  "held to a tolerance, not to the bit"):
        assert words in section, words


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_column_ranks_argument_checks(lib):
    d = (C.c_float * 16)()                                                # a host buffer: every call below must fail before it is read
    call = lib.oai_column_ranks
    #    values mask N V mode twice_rank n_valid tie_term stream
    _refused(lib, call(None, None, 4, 10, 0, d, d, d, None), b"oai_column_ranks", b"values_dev", b"null")
    _refused(lib, call(d, None, 4, 10, 0, None, d, d, None), b"oai_column_ranks", b"twice_rank_dev", b"null")
    _refused(lib, call(d, None, 4, 10, 0, d, None, d, None), b"n_valid_dev", b"null")
    _refused(lib, call(d, None, 4, 10, 0, d, d, None, None), b"tie_term_dev", b"null")
    _refused(lib, call(d, None, 0, 10, 0, d, d, d, None), b"oai_column_ranks", b"n_knees", b"got 0")
    _refused(lib, call(d, d, (1 << 22) + 1, 10, 1, d, d, d, None), b"n_knees", b"4194305")
    _refused(lib, call(d, None, 4, 0, 0, d, d, d, None), b"n_verts", b"4, 0")
    _refused(lib, call(d, None, 4, -3, 0, d, d, d, None), b"n_verts", b"-3")
    _refused(lib, call(d, None, 4, 10, 2, d, d, d, None), b"oai_column_ranks", b"mode", b"got 2")
    _refused(lib, call(d, d, 4, 10, -1, d, d, d, None), b"mode", b"got -1")


def test_rank_sums_argument_checks(lib):
    d = (C.c_int * 16)()
    labels = (C.c_ubyte * 4)(0, 1, 2, 1)
    call = lib.oai_rank_sums
    #    twice_rank labels N V G n_g twice_sum stream
    _refused(lib, call(None, labels, 4, 10, 3, d, d, None), b"oai_rank_sums", b"twice_rank_dev", b"null")
    _refused(lib, call(d, labels, 4, 10, 3, None, d, None), b"oai_rank_sums", b"n_g_dev", b"null")
    _refused(lib, call(d, labels, 4, 10, 3, d, None, None), b"twice_sum_g_dev", b"null")
    _refused(lib, call(d, labels, 0, 10, 3, d, d, None), b"oai_rank_sums", b"n_knees", b"got 0")
    _refused(lib, call(d, labels, (1 << 22) + 1, 10, 3, d, d, None), b"n_knees", b"4194305")
    _refused(lib, call(d, labels, 4, 0, 3, d, d, None), b"n_verts")
    _refused(lib, call(d, labels, 4, 10, 0, d, d, None), b"oai_rank_sums", b"n_groups", b"got 0")
    _refused(lib, call(d, labels, 4, 10, 17, d, d, None), b"n_groups", b"got 17")
    _refused(lib, call(d, None, 4, 10, 3, d, d, None), b"oai_rank_sums", b"labels_host", b"n_groups = 2", b"got 3")
    _refused(lib, call(d, None, 4, 10, 1, d, d, None), b"labels_host", b"got 1")
    _refused(lib, call(d, labels, 4, 10, 2, d, d, None), b"oai_rank_sums", b"labels_host[2] = 2", b"n_groups = 2")


def test_rank_scores_argument_checks(lib):
    d = (C.c_int * 16)()
    call = lib.oai_rank_scores
    #    twice_rank n_valid N V kind c score mask stream
    _refused(lib, call(None, d, 4, 10, 0, 0.375, d, d, None), b"oai_rank_scores", b"twice_rank_dev", b"null")
    _refused(lib, call(d, None, 4, 10, 0, 0.375, d, d, None), b"n_valid_dev", b"null")
    _refused(lib, call(d, d, 4, 10, 0, 0.375, None, d, None), b"oai_rank_scores", b"score_dev", b"null")
    _refused(lib, call(d, d, 4, 10, 0, 0.375, d, None, None), b"mask_dev", b"null")
    _refused(lib, call(d, d, 0, 10, 0, 0.375, d, d, None), b"oai_rank_scores", b"n_knees", b"got 0")
    _refused(lib, call(d, d, (1 << 22) + 1, 10, 0, 0.375, d, d, None), b"n_knees", b"4194305")
    _refused(lib, call(d, d, 4, 0, 0, 0.375, d, d, None), b"n_verts")
    _refused(lib, call(d, d, 4, 10, 3, 0.375, d, d, None), b"oai_rank_scores", b"kind", b"got 3")
    _refused(lib, call(d, d, 4, 10, -1, 0.375, d, d, None), b"kind", b"got -1")
    _refused(lib, call(d, d, 4, 10, 2, -0.01, d, d, None), b"oai_rank_scores", b"c must lie in [0, 1/2]", b"-0.01")
    _refused(lib, call(d, d, 4, 10, 2, 0.51, d, d, None), b"c must lie", b"0.51")
    _refused(lib, call(d, d, 4, 10, 2, float("nan"), d, d, None), b"c must lie")


def test_the_names_are_exported_where_the_other_statistics_are():
    from oai_analysis_2_amd import ops, stats
    check_reexported(("Ranking", "RankSumResult", "SignedRankResult", "KruskalResult", "SpearmanResult", "rank_sum_test", "signed_rank_test", "kruskal_test",
                 "spearman_test"))
    for name in ("ranked", "difference"):
        assert callable(getattr(stats.ThicknessCohort, name))
    for name in ("column_ranks", "rank_sums", "rank_scores"):
        assert callable(getattr(ops, name))
    assert ops.SCORE_KINDS == {"rank": 0, "centred": 1, "normal": 2} and (ops.OAI_RANK_PLAIN, ops.OAI_RANK_SIGNED) == (0, 1)
