"""CPU: the numpy restatement of the cohort regression (tests/group_regression_ref.py; include/oai_hip.h, "Cohort regression") against
independent code -- scipy.stats.linregress, the pooled scipy.stats.ttest_ind, the restated two-sample t of tests/group_stats_ref.py and
np.linalg.lstsq on each vertex's valid knees -- and the host side of oai_analysis_2_amd.stats.regression_test: the index permutations and
every refusal.  The gate is rtol 1e-10 (atol 1e-12 for values near zero); the measured maxima are printed."""
import math

import numpy as np
import pytest
import scipy.stats

import group_regression_ref as rref
import group_stats_ref as gref

N, V = 40, 50
RTOL = 1e-10


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-2)))


def _data(seed, missing=0.1):
    rng = np.random.default_rng(seed)
    age = rng.uniform(45, 80, N)
    sex = (rng.random(N) < 0.5).astype(np.float64)
    x = rng.normal(0, 1, N) + 0.02 * age
    Y = (2.0 + 0.3 * rng.normal(size=(N, V)) + 0.01 * (age - 60)[:, None] + 0.1 * x[:, None] * rng.random(V)[None, :]).astype(np.float32)
    mask = rng.random((N, V)) >= missing if missing else None
    return Y, mask, x, age, sex


def _observed(Y, mask, x, covariates, intercept):
    Z, D, scale = rref.design_columns(x, covariates, intercept)
    prep = rref.prepare(Y, mask, Z, centre=intercept)
    t, slope = rref.regression_t(prep, mask, D, np.arange(len(x))[None, :], with_slope=True)
    return prep, t[0], slope / scale


def _ols(y, X):
    """(t, beta) of the last column of X by np.linalg.lstsq."""
    beta, *_ = np.linalg.lstsq(X, y, rcond=None)
    res = y - X @ beta
    s2 = res @ res / (len(y) - X.shape[1])
    return beta[-1] / math.sqrt(s2 * np.linalg.inv(X.T @ X)[-1, -1]), beta[-1]


def test_one_regressor_and_an_intercept_equal_linregress():
    Y, _, x, _, _ = _data(1, missing=0)
    _, t, slope = _observed(Y, None, x, None, True)
    want = [scipy.stats.linregress(x, Y[:, v].astype(np.float64)) for v in range(V)]
    want_t, want_slope = np.array([w.slope / w.stderr for w in want]), np.array([w.slope for w in want])
    print("linregress: t", _rel(t, want_t), "slope", _rel(slope, want_slope))
    assert np.allclose(t, want_t, rtol=RTOL, atol=1e-12) and np.allclose(slope, want_slope, rtol=RTOL, atol=1e-12)


def test_a_dummy_regressor_equals_the_pooled_two_sample_t():
    Y, mask, _, _, _ = _data(2)
    g = np.arange(N) % 2 == 0
    mask[:, 7] = ~g                                                        # the dummy is constant among the valid knees: no t
    mask[:, 8] = False
    mask[:3, 8] = True                                                     # n = 3 = p + 1
    _, t, slope = _observed(Y, mask, g.astype(np.float64), None, True)
    y = Y.astype(np.float64)
    want = np.array([scipy.stats.ttest_ind(y[g & mask[:, v], v], y[~g & mask[:, v], v], equal_var=True).statistic if v != 7 else np.nan
                     for v in range(V)])
    assert np.isnan(t[7]) and np.isnan(slope[7]) and not np.isnan(np.delete(t, 7)).any()
    keep = np.arange(V) != 7
    two = gref.permutation_t(gref.prepare(Y, mask), mask, g[None, :], gref.TWO_SAMPLE)[0]
    both = keep & (np.arange(V) != 8)                                      # that t asks for two knees on either side
    assert np.isnan(two[8]) and not np.isnan(two[both]).any()
    print("ttest_ind:", _rel(t[keep], want[keep]), "group_stats_ref:", _rel(t[both], two[both]))
    assert np.allclose(t[keep], want[keep], rtol=RTOL, atol=1e-12) and np.allclose(t[both], two[both], rtol=RTOL, atol=1e-12)
    means = np.array([y[g & mask[:, v], v].mean() - y[~g & mask[:, v], v].mean() for v in np.nonzero(keep)[0]])
    assert np.allclose(slope[keep], means, rtol=RTOL, atol=1e-12)


@pytest.mark.parametrize("intercept", [True, False], ids=["intercept", "no_intercept"])
def test_covariates_and_missing_entries_equal_least_squares_on_the_valid_knees(intercept):
    Y, mask, x, age, sex = _data(3)
    cov = np.stack([age, sex], axis=1)
    prep, t, slope = _observed(Y, mask, x, cov, intercept)
    assert prep["ok"].all() and (prep["n"] == mask.sum(axis=0)).all() and (prep["n"] < N).any()
    X = np.concatenate(([np.ones((N, 1))] if intercept else []) + [cov, x[:, None]], axis=1)
    want = np.array([_ols(Y[mask[:, v], v].astype(np.float64), X[mask[:, v]]) for v in range(V)])
    print("lstsq: t", _rel(t, want[:, 0]), "slope", _rel(slope, want[:, 1]))
    assert np.allclose(t, want[:, 0], rtol=RTOL, atol=1e-12) and np.allclose(slope, want[:, 1], rtol=RTOL, atol=1e-12)


def test_a_permuted_row_is_the_observed_statistic_of_the_permuted_design():
    Y, mask, x, age, sex = _data(4)
    Z, D, _ = rref.design_columns(x, np.stack([age, sex], axis=1), True)
    prep = rref.prepare(Y, mask, Z)
    rng = np.random.default_rng(5)
    perm = np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(3)])
    t = rref.regression_t(prep, mask, D, perm)
    for r in range(len(perm)):
        alone = rref.regression_t(prep, mask, D[perm[r]], np.arange(N)[None, :])[0]
        assert np.array_equal(t[r], alone, equal_nan=True) and not np.isnan(alone).any()
    assert not np.array_equal(t[0], t[1])
    wild = perm.copy()
    wild[1, :3], wild[1, 3] = -7, N + 5                                     # out of range: clamped to 0 and N - 1
    clamped = perm.copy()
    clamped[1, :3], clamped[1, 3] = 0, N - 1
    assert np.array_equal(rref.regression_t(prep, mask, D, wild), rref.regression_t(prep, mask, D, clamped), equal_nan=True)


def test_index_permutations():
    from oai_analysis_2_amd import stats
    every = stats.index_permutations(4, 100)
    assert every.exact and every.index.shape == (24, 4) and every.index.dtype == np.int32
    assert every.index.tolist() == sorted(every.index.tolist()) and every.index[0].tolist() == [0, 1, 2, 3]
    assert len({tuple(r) for r in every.index.tolist()}) == 24
    blocks = np.array([0, 1, 0, 1, 1])
    within = stats.index_permutations(5, 12, blocks=blocks)
    assert within.exact and len(within) == 12 and len({tuple(r) for r in within.index.tolist()}) == 12
    assert (blocks[within.index] == blocks[None, :]).all() and within.index[0].tolist() == list(range(5))
    assert not stats.index_permutations(5, 11, blocks=blocks).exact
    blocks = np.arange(30) % 3
    a, b, c = (stats.index_permutations(30, 50, seed=s, blocks=blocks) for s in (7, 7, 8))
    assert not a.exact and a.index.shape == (50, 30) and np.array_equal(a.index, b.index) and not np.array_equal(a.index, c.index)
    assert np.array_equal(a.index[0], np.arange(30)) and (np.sort(a.index, axis=1) == np.arange(30)[None, :]).all()
    assert (blocks[a.index] == blocks[None, :]).all() and (a.index[1:] != np.arange(30)[None, :]).any(axis=1).all()
    rng = np.random.Generator(np.random.PCG64(3))
    assert np.array_equal(stats.index_permutations(6, 9, seed=3).index[1:], rng.permuted(np.tile(np.arange(6, dtype=np.int32), (8, 1)), axis=1))
    with pytest.raises(ValueError, match="one label per knee"):
        stats.index_permutations(5, 10, blocks=[0, 1])
    with pytest.raises(ValueError, match=">= 1"):
        stats.index_permutations(5, 0)


class _NoDevice:
    """Stands for a cohort of ten knees; anything but its length would be a launch."""
    kind = "FC"

    def __len__(self):
        return 10

    def __getattr__(self, name):
        raise AssertionError(f"regression_test touched cohort.{name} before it refused")


def test_regression_test_refuses_before_any_launch():
    from oai_analysis_2_amd import stats
    cohort, rng = _NoDevice(), np.random.default_rng(0)
    x, cov = rng.normal(size=10), rng.normal(size=(10, 2))
    for kwargs, words in (
            (dict(x=np.full(10, 3.0)), "x is constant"),
            (dict(x=x, covariates=np.stack([cov[:, 0], np.ones(10)], axis=1)), "covariate 1 is constant"),
            (dict(x=x, covariates=np.stack([cov[:, 0], 2 * x + 1], axis=1)), "full column rank"),
            (dict(x=x, covariates=np.stack([cov[:, 0], cov[:, 1], cov[:, 0] - 3 * cov[:, 1]], axis=1)), "full column rank"),
            (dict(x=x, covariates=rng.normal(size=(10, 5))), "at most 6"),
            (dict(x=x, covariates=rng.normal(size=(10, 5)), intercept=False, permutations=np.arange(9)[None, :]), r"\[P, 10\]"),
            (dict(x=x[:9]), "one entry per knee"),
            (dict(x=x, covariates=cov[:9]), "covariates must be"),
            (dict(x=np.where(np.arange(10) == 4, np.nan, x)), "NaN"),
            (dict(x=x, covariates=np.where(np.arange(20).reshape(10, 2) == 5, np.inf, cov)), "NaN"),
            (dict(x=x, permutations=np.stack([np.arange(10)[::-1], np.arange(10)])), "row 0"),
            (dict(x=x, permutations=np.stack([np.arange(10), np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 8])])), "must be a permutation"),
            (dict(x=x, permutations=np.stack([np.arange(10), np.arange(10) + 1])), "must be a permutation"),
            (dict(x=x, blocks=[0, 1]), "one label per knee")):
        with pytest.raises(ValueError, match=words):
            stats.regression_test(cohort, **kwargs)
    with pytest.raises(ValueError, match="full column rank"):                 # two dummies that add up to the intercept
        stats.regression_test(cohort, x, covariates=np.stack([np.arange(10) % 2, 1 - np.arange(10) % 2], axis=1))
    stats._design_columns(x, np.stack([np.arange(10) % 2, 1 - np.arange(10) % 2], axis=1), False, 10)        # fine without one
    assert stats.regression_batch(30002, 200, 4, 100000, False) % 16 == 0 and stats.regression_batch(100, 40, 4, 7, True) == 7


def test_the_one_regressor_builder_is_the_design_matrix_of_one_column():
    """``_design_columns`` is ``_design_matrix`` of one column called "x": its three outputs are the bits of the restated multi-column
    builder (tests/group_f_ref.py) over 2 to 13 knees, 0 to 5 covariates and both intercept settings, and what it refuses it refuses in
    the words that the callers of the earlier one-column builder match on."""
    import group_f_ref as fref
    from oai_analysis_2_amd import stats
    rng, accepted = np.random.default_rng(11), 0
    for n in range(2, 14):
        for c in range(6):
            for intercept in (True, False):
                x, cov = rng.normal(size=n), (60 + 8 * rng.normal(size=(n, c)) if c else None)
                if c + 1 + int(intercept) > min(n, 6):                    # more columns than knees, or than six: refused
                    with pytest.raises(ValueError, match="at most 6" if c + 1 + int(intercept) > 6 else "full column rank"):
                        stats._design_columns(x, cov, intercept, n)
                    continue
                (Z, D, scale), (Zr, Dr, scales) = stats._design_columns(x, cov, intercept, n), fref.design_matrix(x[:, None], cov, intercept)
                assert np.array_equal(Z, Zr) and np.array_equal(D, Dr) and scales.shape == (1,) and scale == scales[0] and isinstance(scale, float)
                assert Z.shape == (n, c + int(intercept)) and D.shape == (n, c + int(intercept) + 1) and D.flags.c_contiguous and Z.flags.c_contiguous
                accepted += 1
    assert accepted == 112
    i = np.arange(10)
    x, cov = rng.normal(size=10), rng.normal(size=(10, 2))
    for args, words in (
            ((np.full(10, 3.0), None, True), "x is constant"),
            ((x, np.stack([cov[:, 0], np.ones(10)], axis=1), True), "covariate 1 is constant"),
            ((x, np.stack([cov[:, 0], 2 * x + 1], axis=1), True), "full column rank"),                       # collinear given the intercept
            ((x, np.stack([cov[:, 0], 3 * x], axis=1), False), "full column rank"),                          # collinear without one
            ((x, np.stack([i % 2, 1 - i % 2], axis=1).astype(np.float64), True), "full column rank"),        # two dummies add up to it
            ((x, rng.normal(size=(10, 5)), True), "at most 6"),                                              # seven columns
            ((np.where(i == 4, np.nan, x), None, True), "NaN"),
            ((x, np.where(np.arange(20).reshape(10, 2) == 5, np.inf, cov), True), "NaN"),
            ((x[:9], None, True), "one entry per knee"),
            ((x[:, None], None, True), "one entry per knee"),
            ((x, cov[:9], True), "covariates must be")):
        with pytest.raises(ValueError, match=words):
            stats._design_columns(*args, 10)


def test_a_result_hands_its_maps_to_the_atlas_image():
    from oai_analysis_2_amd import stats

    class Atlas:
        def image(self, vector, kind):
            return kind, vector

    v = np.array([1.0, np.nan, -2.0])
    res = stats.RegressionResult("TC", v, v, v, v + 2, v, v, v + 1, v, 10, False)
    for what, want in (("slope", v + 2), ("p_fwer", v + 1), ("n", v), ("partial_r", v)):
        kind, vec = res.image(Atlas(), what)
        assert kind == "TC" and vec.dtype == np.float32 and np.array_equal(vec, want.astype(np.float32), equal_nan=True)
    with pytest.raises(ValueError, match="without a cluster threshold"):
        res.image(Atlas(), "cluster_label")
    with pytest.raises(ValueError, match="no image"):
        res.image(Atlas(), "dof")
