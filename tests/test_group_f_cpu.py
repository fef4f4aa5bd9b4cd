"""CPU: the numpy restatement of the cohort F test (tests/group_f_ref.py; include/oai_hip.h, "Cohort F test") against independent code --
scipy.stats.f_oneway and two np.linalg.lstsq fits (reduced and full model) on each vertex's valid knees, and the restated t of
tests/group_regression_ref.py for one tested column -- and the host side of oai_analysis_2_amd.stats.f_test and anova_test: the design
construction and every refusal.  The gate is rtol 1e-10 (atol 1e-12 for values near zero), that of test_group_regression_cpu.py; the
measured maxima are printed."""
import numpy as np
import pytest
import scipy.stats

import group_f_ref as fref
import group_regression_ref as rref

N, V = 40, 50
RTOL = 1e-10


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-2)))


def _data(seed, levels, missing=0.1):
    rng = np.random.default_rng(seed)
    groups = np.arange(N) % levels
    rng.shuffle(groups)
    age = rng.uniform(45, 80, N)
    shift = rng.normal(0.0, 0.2, (levels, V))
    Y = (2.0 + 0.3 * rng.normal(size=(N, V)) + 0.01 * (age - 60)[:, None] + shift[groups]).astype(np.float32)
    mask = rng.random((N, V)) >= missing if missing else None
    return Y, mask, groups, age


def _observed(Y, mask, X, covariates, intercept, perm=None):
    Z, D, scales = fref.design_matrix(X, covariates, intercept)
    prep = fref.prepare(Y, mask, Z if Z.shape[1] else None, centre=intercept)
    rows = np.arange(len(Y))[None, :] if perm is None else perm
    F, coef = fref.regression_f(prep, mask, D, rows, len(scales), with_coef=True)
    return prep, F, coef / scales[:, None]


def _rss(y, X):
    if X.shape[1] == 0:
        return float(y @ y), np.zeros(0)
    beta, *_ = np.linalg.lstsq(X, y, rcond=None)
    res = y - X @ beta
    return float(res @ res), beta


def _lstsq_f(y, reduced, full):
    """(F, the coefficients of the columns that ``full`` has beyond ``reduced``) from two least-squares fits."""
    k = full.shape[1] - reduced.shape[1]
    rss0, _ = _rss(y, reduced)
    rss1, beta = _rss(y, full)
    return (rss0 - rss1) / k / (rss1 / (len(y) - full.shape[1])), beta[-k:]


@pytest.mark.parametrize("levels", [3, 5])
def test_a_one_way_layout_equals_f_oneway(levels):
    Y, mask, groups, _ = _data(levels, levels)
    _, dummies = fref.anova_dummies(groups)
    prep, F, coef = _observed(Y, mask, dummies, None, True)
    y = Y.astype(np.float64)
    want = np.array([scipy.stats.f_oneway(*[y[(groups == g) & mask[:, v], v] for g in range(levels)]).statistic for v in range(V)])
    assert prep["ok"].all() and (prep["n"] < N).any() and not np.isnan(F).any()
    print(f"f_oneway, {levels} levels: F", _rel(F[0], want))
    assert np.allclose(F[0], want, rtol=RTOL, atol=1e-12)
    means = np.array([[y[(groups == g) & mask[:, v], v].mean() for v in range(V)] for g in range(levels)])
    assert np.allclose(coef, means[1:] - means[:1], rtol=RTOL, atol=1e-12)              # without covariates: differences of the means


@pytest.mark.parametrize("levels, n_cov", [(3, 1), (3, 2), (5, 1)])
def test_covariates_equal_two_least_squares_fits_on_the_valid_knees(levels, n_cov):
    Y, mask, groups, age = _data(10 + levels + n_cov, levels)
    rng = np.random.default_rng(levels)
    cov = np.stack([age, (rng.random(N) < 0.5).astype(np.float64)][:n_cov], axis=1)
    _, dummies = fref.anova_dummies(groups)
    _, F, coef = _observed(Y, mask, dummies, cov, True)
    reduced = np.concatenate([np.ones((N, 1)), cov], axis=1)
    full = np.concatenate([reduced, dummies], axis=1)
    want = [_lstsq_f(Y[mask[:, v], v].astype(np.float64), reduced[mask[:, v]], full[mask[:, v]]) for v in range(V)]
    want_f, want_coef = np.array([w[0] for w in want]), np.stack([w[1] for w in want], axis=1)
    print(f"lstsq, {levels} levels, {n_cov} covariates: F", _rel(F[0], want_f), "coefficients", _rel(coef, want_coef))
    assert np.allclose(F[0], want_f, rtol=RTOL, atol=1e-12) and np.allclose(coef, want_coef, rtol=RTOL, atol=1e-12)


def test_continuous_columns_without_an_intercept_and_nothing_else_in_the_model():
    """k = p: no nuisance column, no intercept -- the reduced model is empty and its residual sum of squares is sum y^2."""
    Y, mask, _, age = _data(21, 3)
    rng = np.random.default_rng(22)
    X = np.stack([age, rng.normal(size=N) + 1.0, rng.normal(size=N)], axis=1)
    prep, F, coef = _observed(Y, mask, X, None, False)
    assert (prep["Q"] > 0).all()
    want = [_lstsq_f(Y[mask[:, v], v].astype(np.float64), np.zeros((int(mask[:, v].sum()), 0)), X[mask[:, v]]) for v in range(V)]
    want_f, want_coef = np.array([w[0] for w in want]), np.stack([w[1] for w in want], axis=1)
    print("lstsq, k = p = 3: F", _rel(F[0], want_f), "coefficients", _rel(coef, want_coef))
    assert np.allclose(F[0], want_f, rtol=RTOL, atol=1e-12) and np.allclose(coef, want_coef, rtol=RTOL, atol=1e-12)


@pytest.mark.parametrize("intercept", [True, False], ids=["intercept", "no_intercept"])
def test_one_tested_column_is_the_square_of_the_restated_t(intercept):
    Y, mask, _, age = _data(31, 3)
    rng = np.random.default_rng(32)
    x = rng.normal(size=N) + 0.02 * age
    perm = np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(4)])
    _, F, coef = _observed(Y, mask, x, age, intercept, perm)
    Z, D, scale = rref.design_columns(x, age, intercept)
    t, slope = rref.regression_t(rref.prepare(Y, mask, Z, centre=intercept), mask, D, perm, with_slope=True)
    assert not np.isnan(t).any()
    print("k = 1: F against t*t", float(np.max(np.abs(F - t * t) / (t * t))), "coefficient", _rel(coef[0], slope / scale))
    assert np.allclose(F, t * t, rtol=1e-12, atol=0) and np.allclose(coef[0], slope / scale, rtol=1e-12, atol=0)


def test_another_reference_level_changes_the_coefficients_and_not_f():
    Y, mask, groups, age = _data(41, 4)
    rng = np.random.default_rng(42)
    perm = np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(3)])
    relabelled = np.array([3, 0, 2, 1])[groups]                               # level 1 becomes the smallest label: the reference
    _, F, coef = _observed(Y, mask, fref.anova_dummies(groups)[1], age, True, perm)
    _, F2, coef2 = _observed(Y, mask, fref.anova_dummies(relabelled)[1], age, True, perm)
    print("relabelled levels: F", _rel(F2, F))
    assert np.allclose(F2, F, rtol=RTOL, atol=1e-12) and not np.isnan(F).any()
    # old level g is new level (3, 0, 2, 1)[g]; old coefficients are differences from old level 0 = new level 3
    assert np.allclose(coef2[2], -coef[0], rtol=1e-8, atol=1e-12) and np.allclose(coef2[1], coef[1] - coef[0], rtol=1e-8, atol=1e-12)
    assert not np.allclose(coef2, coef)


def test_corner_cases_of_the_restatement():
    """dof 0 and dof 1, a constant vertex, a level without a valid knee (always, and under one permutation only), clamped indices."""
    levels = 3
    Y, mask, groups, _ = _data(51, levels)
    _, dummies = fref.anova_dummies(groups)
    p = levels
    Y[:, 4] = 0.0
    mask[:, 4] = True
    mask[:, 1] = False
    mask[:, 2] = np.arange(N) < p
    mask[:, 3] = np.arange(N) < p + 1
    mask[:, 5] = groups != 2                                                 # level 2 has no valid knee: its dummy is 0 among them
    few = np.nonzero(groups != 2)[0][:p + 2]
    few = np.concatenate([few[:-1], np.nonzero(groups == 2)[0][:1]])          # one knee of level 2 among the few valid ones
    mask[:, 6] = np.isin(np.arange(N), few)
    rng = np.random.default_rng(52)
    perm = np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(3)])
    others = np.nonzero(groups != 2)[0]
    row = perm[2].copy()                                                     # row 2 hands the few valid knees design rows of levels 0 and 1
    row[few] = others[:len(few)]
    row[np.setdiff1d(np.arange(N), few)] = np.setdiff1d(np.arange(N), others[:len(few)])
    perm[2] = row
    wild, clamped = perm.copy(), perm.copy()
    wild[1, 0], wild[1, N - 1], clamped[1, 0], clamped[1, N - 1] = -5, N + 3, 0, N - 1
    Z, D, scales = fref.design_matrix(dummies, None, True)
    prep = fref.prepare(Y, mask, Z)
    F, coef = fref.regression_f(prep, mask, D, wild, 2, with_coef=True)
    assert np.array_equal(F, fref.regression_f(prep, mask, D, clamped, 2), equal_nan=True)
    assert np.isnan(F[:, 1]).all() and prep["n"][1] == 0
    assert np.isnan(F[:, 2]).all() and prep["n"][2] == p and np.isnan(coef[:, 2]).all()
    assert not np.isnan(F[0, 3]) and prep["n"][3] == p + 1
    assert np.isnan(F[:, 4]).all() and prep["Q"][4] == 0.0 and prep["ok"][4] == 1
    assert np.isnan(F[0, 5]) and np.isnan(coef[:, 5]).all() and prep["ok"][5] == 1 and prep["n"][5] > p + 1
    assert not np.isnan(F[0, 6]) and np.isnan(F[2, 6]) and not np.isnan(F[3, 6])
    assert not np.isnan(F[:, 7:]).any() and (F[~np.isnan(F)] >= 0.0).all()


def test_the_design_of_f_test_and_anova_test_is_the_restated_one():
    from oai_analysis_2_amd import stats
    rng = np.random.default_rng(61)
    X, cov = rng.normal(size=(12, 3)) + 2.0, rng.normal(size=(12, 2)) + 5.0
    for covariates, intercept in ((cov, True), (cov, False), (None, True), (None, False), (cov[:, 0], True)):
        got, want = stats._design_matrix(X, covariates, intercept, 12), fref.design_matrix(X, covariates, intercept)
        for g, w in zip(got, want):
            assert g.dtype == np.float64 and np.array_equal(g, w)
        q = (0 if covariates is None else np.asarray(covariates).reshape(12, -1).shape[1]) + int(intercept)
        assert got[0].shape == (12, q) and got[1].shape == (12, q + 3) and got[2].shape == (3,) and got[1].flags.c_contiguous
        assert np.allclose((got[1][:, int(intercept):] ** 2).sum(axis=0), 1.0)
        if intercept:
            assert (got[1][:, 0] == 1.0).all() and np.allclose(got[1][:, 1:].sum(axis=0), 0.0, atol=1e-12)
    one = stats._design_matrix(X[:, 0], None, True, 12)                       # [N] is one tested column
    assert one[1].shape == (12, 2) and np.array_equal(one[1], fref.design_matrix(X[:, :1], None, True)[1])
    groups = np.array([7, 3, 3, 9, 7, 9, 3, 7, 9, 3, 7, 9])
    levels, where = stats._anova_levels(groups, 12, 1)
    want_levels, dummies = fref.anova_dummies(groups)
    assert levels.tolist() == [3, 7, 9] == want_levels.tolist() and np.array_equal(levels[where], groups)
    assert np.array_equal(np.stack([(where == g).astype(np.float64) for g in (1, 2)], axis=1), dummies)
    assert np.array_equal(stats._anova_levels(groups.astype(np.float64), 12, 0)[1], where)      # whole numbers in a float array are labels


class _NoDevice:
    """Stands for a cohort of ten knees; anything but its length would be a launch."""
    kind = "FC"

    def __len__(self):
        return 10

    def __getattr__(self, name):
        raise AssertionError(f"the test touched cohort.{name} before it refused")


def test_f_test_refuses_before_any_launch():
    from oai_analysis_2_amd import stats
    cohort, rng = _NoDevice(), np.random.default_rng(0)
    X, cov = rng.normal(size=(10, 2)), rng.normal(size=(10, 2))
    i = np.arange(10)
    for kwargs, words in (
            (dict(X=np.stack([X[:, 0], np.full(10, 3.0)], axis=1)), "X column 1 is constant"),
            (dict(X=X, covariates=np.stack([np.ones(10), cov[:, 0]], axis=1)), "covariate 0 is constant"),
            (dict(X=np.where(np.arange(20).reshape(10, 2) == 5, np.nan, X)), "X column 1 holds a NaN"),
            (dict(X=X, covariates=np.where(np.arange(20).reshape(10, 2) == 4, np.inf, cov)), "covariate 0 holds a NaN or an infinity"),
            (dict(X=rng.normal(size=(10, 4)), covariates=cov), "7 columns.*at most 6"),
            (dict(X=rng.normal(size=(10, 6))), "7 columns.*at most 6"),
            (dict(X=np.stack([X[:, 0], X[:, 1], 2 * X[:, 0] - X[:, 1] + 1], axis=1)), "full column rank.*X column 2"),
            (dict(X=np.stack([X[:, 0], 3 * cov[:, 1] + 2], axis=1), covariates=cov), "full column rank.*X column 1"),
            (dict(X=np.stack([i % 2, 1 - i % 2], axis=1).astype(np.float64)), "full column rank.*X column 1"),
            (dict(X=X[:9]), r"X must be \[10\]"),
            (dict(X=np.zeros((10, 0))), r"X must be \[10\]"),
            (dict(X=X, covariates=cov[:9]), "covariates must be"),
            (dict(X=X, permutations=np.stack([np.arange(10)[::-1], np.arange(10)])), "row 0"),
            (dict(X=X, permutations=np.stack([np.arange(10), np.arange(10) + 1])), "must be a permutation"),
            (dict(X=X, blocks=[0, 1]), "one label per knee"),
            (dict(X=X, tfce="yes"), "tfce must be")):
        with pytest.raises(ValueError, match=words):
            stats.f_test(cohort, **kwargs)
    stats._design_matrix(np.stack([i % 2, 1 - i % 2], axis=1).astype(np.float64), None, False, 10)     # two dummies are fine without an intercept
    with pytest.raises(ValueError, match="full column rank.*X column 5"):                                # more columns than knees
        stats._design_matrix(rng.normal(size=(5, 6)), None, False, 5)


def test_anova_test_refuses_before_any_launch():
    from oai_analysis_2_amd import stats
    cohort, rng = _NoDevice(), np.random.default_rng(1)
    i = np.arange(10)
    for kwargs, words in (
            (dict(groups=np.full(10, 2)), "single level"),
            (dict(groups=np.where(i == 9, 2, i % 2)), "level 2 has 1 knee"),
            (dict(groups=i % 2 + 0.5), "integer labels"),
            (dict(groups=np.array(list("aabbaabbab"))), "integer labels"),
            (dict(groups=np.where(i == 3, np.nan, i % 2)), "integer labels"),
            (dict(groups=i % 7), "7 levels.*at most 6"),
            (dict(groups=i % 4, covariates=rng.normal(size=(10, 3))), "4 levels and 3 covariates make a design of 7 columns"),
            (dict(groups=i % 3, covariates=rng.normal(size=(10, 4))), "at most 6"),
            (dict(groups=(i % 3)[:9]), "one label per knee"),
            (dict(groups=i % 2, covariates=(i % 2).astype(np.float64)), "full column rank.*the dummy of level 1"),
            (dict(groups=i % 2, covariates=np.where(i == 2, np.nan, rng.normal(size=10))), "covariate 0 holds a NaN"),
            (dict(groups=i % 2, permutations=np.stack([np.arange(10)[::-1], np.arange(10)])), "row 0")):
        with pytest.raises(ValueError, match=words):
            stats.anova_test(cohort, **kwargs)


def test_an_f_result_hands_its_maps_to_the_atlas_image():
    from oai_analysis_2_amd import stats

    class Atlas:
        def image(self, vector, kind):
            return kind, vector

    v = np.array([1.0, np.nan, 2.0])
    res = stats.FResult(kind="TC", f=v, n=v + 3, dof1=2, dof2=v, coefficients=np.stack([v, v]), partial_eta2=v + 2, p_uncorrected=v, p_fwer=v + 1,
                        max_f=v, n_permutations=10, exact=False)
    assert res.levels is None and res.group_n is None and res.group_mean is None and res.clusters == [] and res.tfce is None
    assert stats.FResult.IMAGES == ("f", "partial_eta2", "p_fwer", "p_uncorrected", "n", "cluster_label", "tfce", "p_tfce")
    for what, want in (("f", v), ("p_fwer", v + 1), ("n", v + 3), ("partial_eta2", v + 2)):
        kind, vec = res.image(Atlas(), what)
        assert kind == "TC" and vec.dtype == np.float32 and np.array_equal(vec, want.astype(np.float32), equal_nan=True)
    with pytest.raises(ValueError, match="without a cluster threshold"):
        res.image(Atlas(), "cluster_label")
    with pytest.raises(ValueError, match="without tfce"):
        res.image(Atlas(), "p_tfce")
    with pytest.raises(ValueError, match="no image"):
        res.image(Atlas(), "t")
    assert "FResult" in stats._SurfaceResult.image.__doc__ and "partial_eta2" in stats._SurfaceResult.image.__doc__
