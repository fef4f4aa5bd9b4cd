"""CPU: the numpy restatement of the bootstrap kernels (tests/bootstrap_ref.py) against independent code -- scipy.stats.bootstrap with its
draws replayed, np.quantile, np.std -- and the host-side resampling of oai_analysis_2_amd.stats.  No GPU is touched.

Measured on the shapes below (N = 23 and 11 + 14 knees, B = 999, level 0.9, five vertices), largest relative difference to scipy: one-sample
mean percentile 2.5e-16, BCa 5.0e-16; two-sample difference percentile 2.2e-14, BCa 1.4e-13 (a limit close to zero); paired slope
percentile 1.0e-14; standard error 1.1e-15.  Gate: 1e-10 relative.  se against np.std(ddof=1): 0 measured (along axis 0 numpy adds row
by row, the same order); the gate is B * 2^-52 = 2.2e-13, the bound of a sequential sum of B non-negative terms against any other order
of the same sum, so that a pairwise numpy passes as well."""
import numpy as np
import pytest
import scipy.stats

import bootstrap_ref as bref

B, LEVEL, SEED, V = 999, 0.9, 11, 5
GATE = 1e-10


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(np.asarray(want))))


def _one_sample():
    rng = np.random.default_rng(1)
    return (2.0 + 0.4 * rng.normal(size=(23, V))).astype(np.float32)


def _two_sample():
    rng = np.random.default_rng(2)
    g = np.array([0] * 11 + [1] * 14)
    rng.shuffle(g)
    Y = (2.0 + 0.4 * rng.normal(size=(25, V)) + 0.3 * g[:, None]).astype(np.float32)
    return Y, g


def _scipy(data, statistic, method, **kw):
    return [scipy.stats.bootstrap(tuple(d[:, v].astype(np.float64) if d.ndim == 2 else d for d in data), statistic, n_resamples=B,
                                  confidence_level=LEVEL, method=method, vectorized=True, random_state=np.random.default_rng(SEED), **kw)
            for v in range(V)]


def _limits(results):
    return (np.array([r.confidence_interval.low for r in results]), np.array([r.confidence_interval.high for r in results]),
            np.array([r.standard_error for r in results]))


@pytest.mark.parametrize("method", ["percentile", "bca"])
def test_one_sample_mean_equals_scipy_with_its_draws_replayed(method):
    Y = _one_sample()
    counts = bref.counts(23, B, SEED)
    ours = bref.ci(Y, None, counts, LEVEL, method)
    low, high, se = _limits(_scipy((Y,), lambda a, axis: np.mean(a, axis=axis), "BCa" if method == "bca" else "percentile"))
    worst = max(_rel(ours["lower"], low), _rel(ours["upper"], high))
    print(f"one-sample mean {method}: limits {worst:.3g}, se {_rel(ours['se'], se):.3g}")
    assert worst <= GATE and _rel(ours["se"], se) <= GATE
    assert (ours["n_finite"] == B).all() and (ours["n"] == 23).all()


@pytest.mark.parametrize("method", ["percentile", "bca"])
def test_two_sample_difference_equals_scipy_with_its_draws_replayed(method):
    """scipy draws the first sample's B resamples, then the second's, from one generator: the blocks in ascending label.  BCa holds the
    per-stratum acceleration."""
    Y, g = _two_sample()
    counts = bref.counts(25, B, SEED, blocks=g)
    ours = bref.ci(Y, None, counts, LEVEL, method, groups=g)
    low, high, se = _limits(_scipy((Y[g == 0], Y[g == 1]), lambda a, b, axis: np.mean(b, axis=axis) - np.mean(a, axis=axis),
                                   "BCa" if method == "bca" else "percentile"))
    worst = max(_rel(ours["lower"], low), _rel(ours["upper"], high))
    print(f"two-sample difference {method}: limits {worst:.3g}, se {_rel(ours['se'], se):.3g}")
    assert worst <= GATE and _rel(ours["se"], se) <= GATE
    y = Y.astype(np.float64)
    assert _rel(ours["estimate"], y[g == 1].mean(axis=0) - y[g == 0].mean(axis=0)) <= GATE


def test_paired_slope_equals_scipy_with_its_draws_replayed():
    Y = _one_sample()
    x = np.random.default_rng(3).normal(size=23)
    Y = (Y + 0.2 * x[:, None]).astype(np.float32)

    def slope(xs, ys, axis):
        xc, yc = xs - xs.mean(axis=axis, keepdims=True), ys - ys.mean(axis=axis, keepdims=True)
        return (xc * yc).sum(axis=axis) / (xc * xc).sum(axis=axis)
    counts = bref.counts(23, B, SEED)
    ours = bref.ci(Y, None, counts, LEVEL, "percentile", x=x)
    low, high, se = _limits(_scipy((x, Y), slope, "percentile", paired=True))
    worst = max(_rel(ours["lower"], low), _rel(ours["upper"], high))
    print(f"paired slope percentile: limits {worst:.3g}, se {_rel(ours['se'], se):.3g}")
    assert worst <= GATE and _rel(ours["se"], se) <= GATE


def test_basic_reflects_the_percentile_limits_and_the_band_contains_the_estimate():
    Y = _one_sample()
    counts = bref.counts(23, 199, SEED)
    pct, basic = bref.ci(Y, None, counts, LEVEL, "percentile", simultaneous=True), bref.ci(Y, None, counts, LEVEL, "basic")
    assert np.array_equal(basic["lower"], 2.0 * pct["estimate"] - pct["upper"]) and np.array_equal(basic["upper"], 2.0 * pct["estimate"] - pct["lower"])
    assert pct["sup"][0] == 0.0 and pct["critical"] == np.quantile(pct["sup"][1:], LEVEL) and pct["critical"] > 0
    # the share of resamples that leave the band anywhere is 1 - level, by construction of the critical value
    assert abs((pct["sup"][1:] > pct["critical"]).mean() - (1 - LEVEL)) <= 1.0 / 199
    assert (pct["lower_simultaneous"] < pct["estimate"]).all() and (pct["upper_simultaneous"] > pct["estimate"]).all()


def _quantile_tile(rng, R, V):
    t = rng.normal(size=(R, V))
    t[:, 0] = np.round(t[:, 0])                                            # heavy ties
    if V > 1:
        t[:, 1] = 3.25                                                     # all equal
    if V > 2:
        t[:, 2] = rng.choice([0.0, -0.0, 1.0, -1.0], size=R)                # signed zeros
    if V > 3:
        t[:, 3] = rng.choice([np.inf, -np.inf, 0.5, 2.0], size=R)
    return t


@pytest.mark.parametrize("R", [1, 2, 3, 64, 257, 1000])
def test_column_quantiles_restated_equal_np_quantile(R):
    rng = np.random.default_rng(R)
    t = _quantile_tile(rng, R, 9)
    probs = np.array([0.0, 1.0, 0.5, 1.0 / 3.0])
    got, count = bref.column_quantiles(t, probs)
    with np.errstate(all="ignore"):
        want = np.quantile(t, probs, axis=0, method="linear")
    assert (count == R).all()
    assert np.array_equal(got, want, equal_nan=True)                       # == everywhere (a NaN where numpy has one: inf - inf)
    plain = (want != 0) & ~np.isnan(want)
    assert np.array_equal(got[plain].view(np.int64), want[plain].view(np.int64))
    # NaN entries are left out, an all-NaN column and a bad probability give NaN, probabilities may differ per vertex
    t2 = t.copy()
    t2[::2, 4] = np.nan
    t2[:, 5] = np.nan
    per_vertex = np.tile(probs[:2, None], (1, 9))
    per_vertex[0, 6], per_vertex[1, 6], per_vertex[0, 7], per_vertex[1, 7] = 0.25, np.nan, -0.1, 1.5
    got2, count2 = bref.column_quantiles(t2, per_vertex)
    kept = t2[:, 4][~np.isnan(t2[:, 4])]
    assert count2[4] == len(kept) and count2[5] == 0 and np.isnan(got2[:, 5]).all()
    if len(kept):
        assert np.array_equal(got2[:, 4], np.quantile(kept, probs[:2]))
    assert got2[0, 6] == np.quantile(t2[:, 6], 0.25) and np.isnan(got2[1, 6]) and np.isnan(got2[:, 7]).all()


def test_negative_zero_sorts_before_positive_zero():
    x = np.array([-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1e-300, np.inf])
    assert (np.diff(bref.keys(x).astype(object)) > 0).all()
    # _lerp adds a zero product, so the sign of a zero result is +: the one place where the bits may differ from np.quantile's
    got, _ = bref.column_quantiles(np.array([[0.0], [-0.0], [0.0], [-0.0]]), np.array([0.0, 1.0]))
    assert (got == 0.0).all()


def test_se_against_numpy_std():
    rng = np.random.default_rng(5)
    tile = 2.0 + 0.1 * rng.normal(size=(B + 1, 40))
    mom = bref.moments(tile)
    want = np.std(tile[1:], axis=0, ddof=1)
    worst = _rel(mom["se"], want)
    print(f"se against np.std(ddof=1): {worst:.3g}")
    assert worst <= B * 2.0 ** -52
    assert np.allclose(mom["mean"], tile[1:].mean(axis=0), rtol=B * 2.0 ** -52, atol=0)
    assert np.array_equal(mom["below"], (tile[1:] < tile[0]).sum(axis=0)) and (mom["equal"] == 0).all()
    tile[3, 0], tile[4, 0], tile[5, 1] = np.nan, np.inf, tile[0, 1]
    again = bref.moments(tile)
    assert again["n_finite"][0] == B - 2 and again["equal"][1] == 1
    assert np.isnan(bref.moments(tile[:2])["se"]).all() and np.isnan(bref.moments(tile[:1])["mean"]).all()


def test_acceleration_single_stratum_is_the_textbook_one():
    rng = np.random.default_rng(8)
    Y = rng.gamma(2.0, 1.0, size=(17, 6)).astype(np.float32)
    jack, _, _ = bref.coef(Y, None, np.ones((17, 1)), 1 - np.eye(17, dtype=np.int64))
    y = Y.astype(np.float64)
    loo = (y.sum(axis=0)[None, :] - y) / 16.0
    assert np.allclose(jack, loo, rtol=1e-13, atol=0)
    d = loo.mean(axis=0)[None, :] - loo
    want = (d ** 3).sum(axis=0) / (6.0 * ((d ** 2).sum(axis=0)) ** 1.5)
    assert np.allclose(bref.acceleration(jack, None, np.zeros(17, np.int64), 1), want, rtol=1e-10, atol=0)


def test_bootstrap_counts():
    from oai_analysis_2_amd import stats
    blocks = np.array([2, 0, 2, 2, 0, 7, 7, 0, 2, 7, 7])
    c = stats.bootstrap_counts(11, 50, seed=3, blocks=blocks).counts
    assert c.dtype == np.uint16 and c.shape == (51, 11) and (c[0] == 1).all()
    for lab in np.unique(blocks):
        assert (c[:, blocks == lab].sum(axis=1) == (blocks == lab).sum()).all()          # knees are resampled within a block only
    assert np.array_equal(c, stats.bootstrap_counts(11, 50, seed=3, blocks=blocks).counts)
    assert not np.array_equal(c, stats.bootstrap_counts(11, 50, seed=4, blocks=blocks).counts)
    assert np.array_equal(c, bref.counts(11, 50, seed=3, blocks=blocks))
    plain = stats.bootstrap_counts(23, B, seed=SEED).counts
    assert (plain.sum(axis=1) == 23).all() and np.array_equal(plain, bref.counts(23, B, SEED))
    draws = np.random.default_rng(SEED).integers(0, 23, (B, 23))
    assert np.array_equal(plain[1:], np.stack([np.bincount(d, minlength=23) for d in draws]))
    with pytest.raises(ValueError, match="n_bootstrap"):
        stats.bootstrap_counts(5, 0)
    with pytest.raises(ValueError, match="65535"):                          # rows handed over are held to the 16 bits as well
        stats._count_rows(np.array([[1, 1], [70000, 0]]), None, 2)
    with pytest.raises(ValueError, match="all ones"):
        stats._count_rows(np.array([[2, 0], [1, 1]]), None, 2)
