"""CPU: the restatement of the rank transform (tests/rank_transform_ref.py) is held to scipy per column, on random float32 data with heavy
ties, and to the header's counting definition to the element; the host helpers of oai_analysis_2_amd.stats that the rank tests use are
held to scipy as well.  No GPU is touched."""
import numpy as np
import pytest
import scipy.special
import scipy.stats

import rank_transform_ref as rref


def _data(seed, N, V, levels=6, missing=0.15):
    """float32 [N, V] drawn from a few levels (heavy ties) with signs, exact zeros and a mask."""
    rng = np.random.default_rng(seed)
    y = rng.integers(-levels, levels + 1, size=(N, V)).astype(np.float32) * np.float32(0.25)
    y[:, V // 2:] += rng.normal(0.0, 1.0, size=(N, V - V // 2)).astype(np.float32)          # the right half is (almost surely) tie-free
    mask = rng.random((N, V)) >= missing
    return y, mask


def test_the_counting_definition_equals_rankdata_to_the_element():
    y, mask = _data(1, 23, 12)
    y[3, 0], y[4, 0] = -0.0, 0.0
    y[5, 1], y[6, 1], y[7, 1] = np.inf, -np.inf, np.nan
    for m in (None, mask):
        for signed in (False, True):
            twice, n_valid, tie = rref.column_ranks(y, m, signed)
            counted, counted_tie = rref.counted_ranks(y, m, signed)
            assert np.array_equal(twice, counted), (m is not None, signed)
            assert np.array_equal(tie, counted_tie), "sum (equal_i^2 - 1) == sum (t^3 - t)"
            assert np.array_equal(n_valid, (twice != 0).sum(axis=0))
    twice, _, _ = rref.column_ranks(y, None, False)
    assert twice[3, 0] == twice[4, 0], "-0.0 ties +0.0"
    assert twice[7, 1] == 0 and twice[5, 1] == 2 * 22 and twice[6, 1] == 2, "NaN is missing; the infinities are the extreme ranks"


def test_u1_equals_scipys_mann_whitney_statistic():
    y, mask = _data(2, 31, 16)
    g = np.arange(31) % 3 == 0
    u1, n1, n2 = rref.mann_whitney_u1(y, mask, g)
    for v in range(y.shape[1]):
        a, b = y[g & mask[:, v], v], y[~g & mask[:, v], v]
        assert (n1[v], n2[v]) == (len(a), len(b))
        assert u1[v] == scipy.stats.mannwhitneyu(a, b).statistic, v


def test_w_equals_scipys_wilcoxon_statistic():
    y, mask = _data(3, 29, 16)
    w_plus, w_minus, n = rref.signed_rank_w(y, mask)
    for v in range(y.shape[1]):
        d = y[mask[:, v], v].astype(np.float64)
        assert n[v] == np.count_nonzero(d)
        assert min(w_plus[v], w_minus[v]) == scipy.stats.wilcoxon(d, zero_method="wilcox", method="approx").statistic, v
        assert w_plus[v] + w_minus[v] == n[v] * (n[v] + 1) / 2


def test_h_equals_scipys_kruskal():
    y, mask = _data(4, 37, 16)
    where = np.arange(37) % 4
    h = rref.kruskal_h(y, mask, where, 4)
    for v in range(y.shape[1]):
        want = scipy.stats.kruskal(*[y[(where == g) & mask[:, v], v] for g in range(4)]).statistic
        assert abs(h[v] - want) <= 1e-12 * abs(want), (v, h[v], want)
    y[:, 0], mask[:, 0] = 1.0, True                                       # every value ties
    mask[where == 2, 1] = False                                           # a level without a knee
    h = rref.kruskal_h(y, mask, where, 4)
    assert np.isnan(h[0]) and np.isnan(h[1]) and np.isfinite(h[2:]).all()


def test_pearson_of_the_midranks_equals_scipys_spearman():
    y, _ = _data(5, 41, 16)
    x = np.random.default_rng(50).integers(0, 5, size=41).astype(np.float64)
    twice, _, _ = rref.column_ranks(y)
    rx = scipy.stats.rankdata(x)
    for v in range(y.shape[1]):
        got = np.corrcoef(0.5 * twice[:, v], rx)[0, 1]
        assert abs(got - scipy.stats.spearmanr(y[:, v], x).statistic) <= 1e-12, v


def test_blom_scores_of_a_tie_free_column_are_symmetric_and_sum_to_zero():
    """Within 1e-12, which is a statement about float64 and not about the code: the probability p of a rank above the middle lies near 1,
    where float64 resolves 2^-53, so its score carries 2^-53 / phi(x) and no mirror image of its partner's -- 2.7e-13 at the extreme
    ranks of n = 4096.  Over a column those errors add up to about n * 2^-53 * (the range of x): 1.2e-13 at n = 200, 8e-13 at n = 1000
    and 3e-12 at n = 4096, so the sum is held to 1e-12 up to n = 1000 and the symmetry at every n."""
    rng = np.random.default_rng(6)
    for n in (1, 2, 7, 200, 1000, 4096):
        y = rng.permutation(n).astype(np.float32)[:, None]
        twice, n_valid, tie = rref.column_ranks(y)
        assert tie[0] == 0 and n_valid[0] == n
        for name, c in rref.CONSTANTS.items():
            score, mask = rref.rank_scores(twice, n_valid, "normal", c)
            s = np.sort(score[:, 0])
            assert mask.all() and np.abs(s + s[::-1]).max() <= 1e-12, (n, name)
            assert n > 1000 or abs(s.sum()) <= 1e-12, (n, name)
    score, _ = rref.rank_scores(twice, n_valid, "normal", 0.375)
    r = np.arange(1, 4097, dtype=np.float64)
    assert np.array_equal(np.sort(score[:, 0]), scipy.special.ndtri((r - 0.375) / (4096 + 0.25)))


def test_rank_and_centred_scores_and_the_mask():
    y, mask = _data(7, 19, 8)
    for signed in (False, True):
        twice, n_valid, _ = rref.column_ranks(y, mask, signed)
        rank, m = rref.rank_scores(twice, n_valid, "rank")
        centred, _ = rref.rank_scores(twice, n_valid, "centred")
        assert np.array_equal(m != 0, rref.valid_entries(y, mask, signed))
        assert np.array_equal(rank, 0.5 * twice) and (rank[m == 0] == 0).all()
        if not signed:
            sums = (centred * m).sum(axis=0)
            assert np.abs(sums).max() == 0.0, "centred midranks sum to zero exactly"


def test_rank_sums_by_label_and_by_sign():
    y, mask = _data(8, 33, 8)
    twice, n_valid, _ = rref.column_ranks(y, mask, signed=True)
    for G in (1, 2, 3, 16):
        labels = np.arange(33) % G
        n_g, sums = rref.rank_sums(twice, labels, G)
        assert np.array_equal(n_g.sum(axis=0), n_valid) and np.array_equal(sums.sum(axis=0), np.abs(twice.astype(np.int64)).sum(axis=0))
    n_g, sums = rref.rank_sums(twice, None, 2)
    assert np.array_equal(n_g[0], (twice < 0).sum(axis=0)) and np.array_equal(sums[1], np.where(twice > 0, twice, 0).sum(axis=0))


def test_the_host_midranks_of_the_package_equal_rankdata():
    from oai_analysis_2_amd import stats
    rng = np.random.default_rng(9)
    for n in (1, 2, 50):
        x = rng.integers(0, 6, size=n).astype(np.float64)
        assert np.array_equal(stats._midranks(x), scipy.stats.rankdata(x))
    with pytest.raises(ValueError):
        stats._midranks([1.0, np.nan])
    assert stats.rank_constant("blom") == 0.375 and stats.rank_constant("tukey") == 1.0 / 3.0 and stats.rank_constant(0.5) == 0.5
    assert stats.rank_constant("rankit") == 0.5 and stats.rank_constant("waerden") == 0.0
    for bad in ("bloom", -0.1, 0.6):
        with pytest.raises(ValueError):
            stats.rank_constant(bad)
