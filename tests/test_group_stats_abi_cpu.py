"""CPU: the cohort-statistics entry points of the C ABI (include/oai_hip.h: oai_group_prepare, oai_permutation_t, oai_permutation_reduce,
oai_graph_clusters) are exported by the built library and refuse bad arguments with a status and a message -- no GPU is touched before
the checks."""
import ctypes as C

import pytest

from abi_cases import BIG, check_symbols, refused as _refused, section as _section
from oai_analysis_2_amd import _lib

NEW = ("oai_group_prepare_workspace_bytes", "oai_group_prepare", "oai_permutation_t_workspace_bytes", "oai_permutation_t",
       "oai_permutation_reduce_workspace_bytes", "oai_permutation_reduce", "oai_graph_clusters_workspace_bytes", "oai_graph_clusters")


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    raw = check_symbols(NEW)
    # the header states the order contract and names its restatement
    section = _section(raw, "Cohort statistics")
    for words in ("tests/group_stats_ref.py", "ASCENDING KNEE INDEX", "ss  = (Q1 - S1*S1/n1) + (Q2 - S2*S2/n2)", "sp2 = ss / (n - 2)",
                  "t   = (S1/n1 - S2/n2) / sqrt(sp2 * (1.0/n1 + 1.0/n2))", "var = (Q - Sf*Sf/n) / (n - 1)", "t   = (Sf/n) / sqrt(var/n)"):
        assert words in section, words


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_group_prepare_argument_checks(lib):
    d = (C.c_float * 16)()                                                # a host buffer: every call below must fail before it is read
    size = lib.oai_group_prepare_workspace_bytes
    assert size(1, 10) == 0 and size(-1, 10) == 0 and size(4, 0) == 0 and size(4, -1) == 0 and size((1 << 24) + 1, 10) == 0
    assert size(200, 30000) >= 2 * 200 * 30000 * 8 + 4 * 30000 * 8 + 30000 * 4
    _refused(lib, lib.oai_group_prepare(None, d, 4, 10, 1, d, BIG, None), b"oai_group_prepare", b"null")
    _refused(lib, lib.oai_group_prepare(d, d, 4, 10, 1, None, BIG, None), b"null")
    _refused(lib, lib.oai_group_prepare(d, None, 1, 10, 1, d, BIG, None), b"oai_group_prepare", b"knees", b"got 1")
    _refused(lib, lib.oai_group_prepare(d, None, -3, 10, 1, d, BIG, None), b"got -3")
    _refused(lib, lib.oai_group_prepare(d, None, 4, -10, 1, d, BIG, None), b"-10")
    _refused(lib, lib.oai_group_prepare(d, None, 4, 10, 2, d, BIG, None), b"centre", b"got 2")
    _refused(lib, lib.oai_group_prepare(d, None, 4, 10, 1, d, 16, None), b"oai_group_prepare", b"workspace")


def test_permutation_t_argument_checks(lib):
    d = (C.c_float * 16)()
    size = lib.oai_permutation_t_workspace_bytes
    assert size(0, 10) == 0 and size(-1, 10) == 0 and size(4, 0) == 0 and size((1 << 20) + 1, 10) == 0
    assert size(64, 30000) >= 64 * 30000 * 8
    call = lib.oai_permutation_t
    _refused(lib, call(None, BIG, d, d, 4, 10, 0, 2, 0, d, BIG, None), b"oai_permutation_t", b"null")
    _refused(lib, call(d, BIG, d, None, 4, 10, 0, 2, 0, d, BIG, None), b"null")
    _refused(lib, call(d, BIG, d, d, 4, 10, 0, 2, 0, None, BIG, None), b"null")
    _refused(lib, call(d, BIG, None, d, 1, 10, 0, 2, 0, d, BIG, None), b"knees", b"got 1")
    _refused(lib, call(d, BIG, None, d, 4, -1, 0, 2, 0, d, BIG, None), b"vertices")
    _refused(lib, call(d, BIG, None, d, 4, 10, 2, 2, 0, d, BIG, None), b"rows", b"2, 2")
    _refused(lib, call(d, BIG, None, d, 4, 10, 3, 1, 0, d, BIG, None), b"rows", b"3, 1")
    _refused(lib, call(d, BIG, None, d, 4, 10, -1, 1, 0, d, BIG, None), b"rows")
    _refused(lib, call(d, BIG, None, d, 4, 10, 0, 2, 2, d, BIG, None), b"mode", b"got 2")
    _refused(lib, call(d, BIG, None, d, 4, 10, 0, 2, -1, d, BIG, None), b"mode", b"got -1")
    _refused(lib, call(d, 16, None, d, 4, 10, 0, 2, 0, d, BIG, None), b"prepared block", b"workspace")
    _refused(lib, call(d, BIG, None, d, 4, 10, 0, 2, 0, d, 16, None), b"oai_permutation_t", b"workspace")


def test_permutation_reduce_argument_checks(lib):
    d = (C.c_float * 16)()
    size = lib.oai_permutation_reduce_workspace_bytes
    assert size(0, 10) == 0 and size(4, 0) == 0 and size(4, -1) == 0 and size(64, 30000) >= 64 * 8
    call = lib.oai_permutation_reduce
    _refused(lib, call(None, 10, 0, 2, d, BIG, d, d, d, None), b"oai_permutation_reduce", b"null")
    _refused(lib, call(d, 10, 0, 2, None, BIG, d, d, d, None), b"null")
    _refused(lib, call(d, 10, 0, 2, d, BIG, None, d, d, None), b"null")
    _refused(lib, call(d, 10, 0, 2, d, BIG, d, None, d, None), b"null")
    _refused(lib, call(d, 10, 0, 2, d, BIG, d, d, None, None), b"null")
    _refused(lib, call(d, -1, 0, 2, d, BIG, d, d, d, None), b"vertices", b"-1")
    _refused(lib, call(d, 10, 2, 2, d, BIG, d, d, d, None), b"rows")
    _refused(lib, call(d, 10, -1, 2, d, BIG, d, d, d, None), b"rows")
    _refused(lib, call(d, 30000, 0, 64, d, 16, d, d, d, None), b"oai_permutation_reduce", b"workspace")


def test_graph_clusters_argument_checks(lib):
    d = (C.c_float * 16)()
    size = lib.oai_graph_clusters_workspace_bytes
    assert size(0, 10) == 0 and size(4, 0) == 0 and size(-4, 10) == 0 and size(64, 30000) >= 2 * 64 * 30000 * 4
    call = lib.oai_graph_clusters
    _refused(lib, call(None, 2, 10, d, d, 18, 2.0, d, BIG, d, None, None, None), b"oai_graph_clusters", b"null")
    _refused(lib, call(d, 2, 10, None, d, 18, 2.0, d, BIG, d, None, None, None), b"null")
    _refused(lib, call(d, 2, 10, d, None, 18, 2.0, d, BIG, d, None, None, None), b"null")
    _refused(lib, call(d, 2, 10, d, d, 18, 2.0, None, BIG, d, None, None, None), b"null")
    _refused(lib, call(d, 2, 10, d, d, 18, 2.0, d, BIG, None, None, None, None), b"null")
    _refused(lib, call(d, 0, 10, d, d, 18, 2.0, d, BIG, d, None, None, None), b"rows", b"got 0")
    _refused(lib, call(d, 2, -10, d, d, 18, 2.0, d, BIG, d, None, None, None), b"vertices", b"-10")
    _refused(lib, call(d, 2, 10, d, d, -18, 2.0, d, BIG, d, None, None, None), b"negative", b"-18")
    _refused(lib, call(d, 2, 10, d, d, 18, 0.0, d, BIG, d, None, None, None), b"threshold")
    _refused(lib, call(d, 2, 10, d, d, 18, -2.0, d, BIG, d, None, None, None), b"threshold")
    _refused(lib, call(d, 2, 10, d, d, 18, float("nan"), d, BIG, d, None, None, None), b"threshold")
    _refused(lib, call(d, 2, 3000, d, d, 18, 2.0, d, 16, d, None, None, None), b"oai_graph_clusters", b"workspace")


def test_the_python_wrappers_refuse_before_the_library():
    import numpy as np
    from oai_analysis_2_amd import stats
    with pytest.raises(ValueError, match="0 / 1"):
        stats.label_permutations([0, 1, 2, 1], 10)
    with pytest.raises(ValueError, match="one label per knee"):
        stats.label_permutations([0, 1, 0, 1], 10, blocks=[0, 1])
    with pytest.raises(ValueError, match=">= 1"):
        stats.sign_flips(4, 0)
    assert stats.default_batch(100, 1000, True) % 16 == 0 or stats.default_batch(100, 1000, True) == 1000
    assert np.array_equal(stats.pack_bits([[1, 0, 1]]), [[5]])


def test_a_result_hands_its_maps_to_the_atlas_image():
    import numpy as np
    from oai_analysis_2_amd import stats

    class Atlas:
        def image(self, vector, kind):
            return kind, vector

    v = np.array([1.0, np.nan, -2.0])
    res = stats.PermutationResult("TC", v, v, v, v, v, v + 1, v, 10, False)
    kind, vec = res.image(Atlas(), "p_fwer")
    assert kind == "TC" and vec.dtype == np.float32 and np.array_equal(vec, (v + 1).astype(np.float32), equal_nan=True)
    with pytest.raises(ValueError, match="without a cluster threshold"):
        res.image(Atlas(), "cluster_label")
    with pytest.raises(ValueError, match="no image"):
        res.image(Atlas(), "n1")


def test_the_results_keep_their_field_names_and_defaults():
    """``PermutationResult`` and ``RegressionResult`` share the cluster and TFCE fields through one base: the public names, their
    defaults, the order of the fields that may be given by position, and the two refusals of ``image`` are what they were."""
    import dataclasses
    import numpy as np
    from oai_analysis_2_amd import stats

    shared = {"cluster_threshold": None, "cluster_label": None, "clusters": [], "max_extent": None, "tfce": None, "p_tfce": None,
              "p_tfce_uncorrected": None, "max_tfce": None, "tfce_clipped": 0, "tfce_settings": None}
    own = {stats.PermutationResult: ("kind", "t", "n1", "n2", "mean_difference", "p_uncorrected", "p_fwer", "max_abs", "n_permutations", "exact"),
           stats.RegressionResult: ("kind", "t", "n", "dof", "slope", "partial_r", "p_uncorrected", "p_fwer", "max_abs", "n_permutations", "exact")}
    images = {stats.PermutationResult: {"t", "p_fwer", "p_uncorrected", "mean_difference", "cluster_label", "tfce", "p_tfce"},
              stats.RegressionResult: {"t", "slope", "partial_r", "p_fwer", "p_uncorrected", "n", "cluster_label", "tfce", "p_tfce"}}

    class Atlas:
        def image(self, vector, kind):
            return kind, vector

    v = np.array([1.0, np.nan, -2.0])
    for cls, names in own.items():
        fields = {f.name: f for f in dataclasses.fields(cls)}
        assert set(fields) == set(names) | set(shared), cls.__name__
        assert [f.name for f in dataclasses.fields(cls) if f.name in names] == list(names)
        for name in names:                                                 # the test's own fields: required
            assert fields[name].default is dataclasses.MISSING and fields[name].default_factory is dataclasses.MISSING, name
        by_position = cls(*([v] * (len(names) - 2)), 10, False)            # and positional, in this order
        assert by_position.kind is v and by_position.n_permutations == 10 and by_position.exact is False
        for name, default in shared.items():
            assert getattr(by_position, name) == default, name
        assert by_position.clusters is not cls(*([v] * (len(names) - 2)), 10, False).clusters       # a list of its own
        by_keyword = cls(**{name: v for name in names}, **{name: 7 for name in shared})
        assert all(getattr(by_keyword, name) == 7 for name in shared)
        res = cls(**{name: v for name in names[1:]}, kind="FC")
        for what in images[cls]:
            if what in shared:
                with pytest.raises(ValueError, match="the test ran without tfce" if "tfce" in what else "the test ran without a cluster threshold"):
                    res.image(Atlas(), what)
            else:
                assert res.image(Atlas(), what)[0] == "FC"
        for what in (set(names) | set(shared)) - images[cls]:
            with pytest.raises(ValueError, match="no image"):
                res.image(Atlas(), what)
