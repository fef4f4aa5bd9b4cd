"""CPU: (i) the numpy restatement of the cohort statistics (tests/group_stats_ref.py) against scipy's per-vertex tests -- the
restatement is what the GPU tests hold the kernels to, to the bit, so it is itself held to an independent implementation here; (ii) the
labelling generators of oai_analysis_2_amd.stats.

The bound of (i): on float32-rounded N(2, 0.5) data with 10 % of the entries masked, the cases below measure a largest relative difference
of the observed t to scipy's of 2.2e-12 (two-sample) and 4.4e-16 (one-sample) at N = 400, V = 2000, and 1.6e-13 and 7.5e-16 at N = 8;
the gate is 1e-10 for N <= 400."""
import math

import numpy as np
import pytest
import scipy.stats

import group_stats_ref as gref

RTOL = 1e-10


def _data(N, V, seed):
    rng = np.random.default_rng([seed, N, V])
    Y = rng.normal(2.0, 0.5, size=(N, V)).astype(np.float32)
    mask = rng.random((N, V)) >= 0.1
    groups = np.arange(N) % 2 == 0
    return Y, mask, groups


@pytest.mark.parametrize("N,V", [(8, 500), (33, 300), (400, 2000)])
def test_the_restated_two_sample_t_is_scipys_pooled_t(N, V):
    Y, mask, groups = _data(N, V, 1)
    prep = gref.prepare(Y, mask, centre=True)
    t = gref.permutation_t(prep, mask, groups[None, :], gref.TWO_SAMPLE)[0]
    y = np.where(mask, Y.astype(np.float64), np.nan)
    want = scipy.stats.ttest_ind(y[groups], y[~groups], axis=0, equal_var=True, nan_policy="omit").statistic
    want = np.ma.filled(want, np.nan).astype(np.float64)
    n1, n2 = mask[groups].sum(axis=0), mask[~groups].sum(axis=0)
    ok = (n1 >= 2) & (n2 >= 2)
    assert ok.sum() > 0.5 * V and not np.isnan(t[ok]).any()
    assert np.isnan(t[~ok]).all()
    rel = np.abs(t[ok] - want[ok]) / np.abs(want[ok])
    print(f"N={N} V={V}: largest relative difference to scipy.stats.ttest_ind {rel.max():.3g}")
    assert rel.max() <= RTOL
    # the descriptive side: n, mean, std
    assert np.array_equal(prep["n"], mask.sum(axis=0))
    some = prep["n"] >= 2
    assert np.allclose(prep["mean"][some], np.nanmean(y, axis=0)[some], rtol=1e-12, atol=0)
    assert np.allclose(prep["std"][some], np.nanstd(y, axis=0, ddof=1)[some], rtol=1e-10, atol=0)


@pytest.mark.parametrize("N,V", [(8, 500), (33, 300), (400, 2000)])
def test_the_restated_one_sample_t_is_scipys(N, V):
    Y, mask, _ = _data(N, V, 2)
    Y = (Y - np.float32(1.9)).astype(np.float32)                         # paired differences: a mean near zero, either sign
    prep = gref.prepare(Y, mask, centre=False)
    flips = np.zeros((2, N), bool)
    flips[1, ::3] = True
    t = gref.permutation_t(prep, mask, flips, gref.ONE_SAMPLE)
    y = np.where(mask, Y.astype(np.float64), np.nan)
    for row in range(2):
        signed = np.where(flips[row][:, None], -y, y)
        want = np.ma.filled(scipy.stats.ttest_1samp(signed, 0.0, axis=0, nan_policy="omit").statistic, np.nan).astype(np.float64)
        ok = mask.sum(axis=0) >= 2
        assert ok.sum() > 0.5 * V and not np.isnan(t[row][ok]).any()
        rel = np.abs(t[row][ok] - want[ok]) / np.abs(want[ok])
        print(f"N={N} V={V} row {row}: largest relative difference to scipy.stats.ttest_1samp {rel.max():.3g}")
        assert rel.max() <= RTOL


def test_the_restatement_marks_what_has_no_t():
    Y = np.array([[1, 5, 0, 2], [2, 5, 0, 9], [3, 5, 0, 4], [5, 5, 0, 1], [4, 5, 0, 7]], np.float32)
    mask = np.ones_like(Y, bool)
    mask[:, 3] = [1, 0, 0, 1, 1]                                          # vertex 3: group 1 keeps one knee
    groups = np.array([1, 1, 1, 0, 0], bool)
    prep = gref.prepare(Y, mask)
    t = gref.permutation_t(prep, mask, groups[None, :], gref.TWO_SAMPLE)[0]
    assert np.isfinite(t[0]) and np.isnan(t[1:]).all()                    # constant, constant, n1 = 1
    empty = gref.prepare(Y, np.zeros_like(mask))
    assert (empty["n"] == 0).all() and np.isnan(empty["mean"]).all() and np.isnan(empty["std"]).all() and (empty["C"] == 0).all()
    max_abs, exceed = gref.reduce_tiles(np.array([[1.0, np.nan, -3.0], [-2.0, 1.0, np.nan], [np.nan, np.nan, np.nan]]))
    assert max_abs.tolist() == [3.0, 2.0, 0.0] and exceed.tolist() == [2, 0, 1]


def test_the_restated_clusters_on_a_path():
    n = 12
    off = np.concatenate([[0], np.cumsum([1] + [2] * (n - 2) + [1])])
    nbr = np.concatenate([[1]] + [[i - 1, i + 1] for i in range(1, n - 1)] + [[n - 2]])
    v = np.array([3, 3, 2, 3, np.nan, 3, -3, -3, 0, 3, 2.0, -2.0])
    label, size, extent = gref.clusters(v[None, :], off, nbr, 2.0)
    assert label[0].tolist() == [0, 0, -1, 3, -1, 5, 6, 6, -1, 9, -1, -1]
    assert size[0].tolist() == [2, 2, 0, 1, 0, 1, 2, 2, 0, 1, 0, 0] and extent.tolist() == [2]


# ---- the generators ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [31, 32, 33])
def test_bit_packing_round_trips(N):
    from oai_analysis_2_amd import stats
    rows = np.random.default_rng(N).random((5, N)) < 0.5
    rows[0, -1], rows[1, -1] = True, False
    bits = stats.pack_bits(rows)
    assert bits.dtype == np.uint32 and bits.shape == (5, (N + 31) // 32)
    assert np.array_equal(bits, gref.pack_bits(rows))                     # the package's packing is the restatement's (written with shifts)
    assert np.array_equal(stats.unpack_bits(bits, N), rows) and np.array_equal(gref.unpack_bits(bits, N), rows)
    for p, i in ((0, 0), (2, N - 1), (4, N // 2)):
        assert bool((bits[p, i // 32] >> np.uint32(i % 32)) & np.uint32(1)) == bool(rows[p, i])


def test_label_permutations_keep_row_0_the_group_sizes_and_the_blocks():
    from oai_analysis_2_amd import stats
    rng = np.random.default_rng(5)
    groups = rng.random(45) < 0.4
    blocks = np.arange(45) % 3
    perms = stats.label_permutations(groups, 500, seed=3, blocks=blocks)
    rows = perms.rows()
    assert len(perms) == 500 and not perms.exact and rows.shape == (500, 45)
    assert np.array_equal(rows[0], groups)
    for b in range(3):
        assert (rows[:, blocks == b].sum(axis=1) == groups[blocks == b].sum()).all()
    assert len(np.unique(rows, axis=0)) > 400                            # draws, not copies
    again = stats.label_permutations(groups, 500, seed=3, blocks=blocks)
    assert np.array_equal(again.bits, perms.bits)
    assert not np.array_equal(stats.label_permutations(groups, 500, seed=4, blocks=blocks).bits, perms.bits)
    free = stats.label_permutations(groups, 200, seed=3).rows()
    assert (free.sum(axis=1) == groups.sum()).all()
    assert any((free[:, blocks == 0].sum(axis=1) != groups[blocks == 0].sum()))      # without blocks the labels do cross them


def test_small_designs_are_enumerated_exactly():
    from oai_analysis_2_amd import stats
    groups = np.array([1, 1, 1, 1, 0, 0, 0, 0])
    perms = stats.label_permutations(groups, 10000)
    rows = perms.rows()
    assert perms.exact and len(perms) == math.comb(8, 4) == 70
    assert np.array_equal(rows[0], groups.astype(bool)) and (rows.sum(axis=1) == 4).all() and len(np.unique(rows, axis=0)) == 70
    assert not stats.label_permutations(groups, 69).exact and len(stats.label_permutations(groups, 69)) == 69
    blocked = stats.label_permutations(groups, 10000, blocks=[0, 0, 1, 1, 0, 0, 1, 1])
    assert blocked.exact and len(blocked) == math.comb(4, 2) ** 2 and len(np.unique(blocked.rows(), axis=0)) == 36
    flips = stats.sign_flips(6, 10000)
    assert flips.exact and len(flips) == 64 and len(np.unique(flips.rows(), axis=0)) == 64 and not flips.rows()[0].any()
    drawn = stats.sign_flips(40, 300, seed=1)
    assert not drawn.exact and len(drawn) == 300 and not drawn.rows()[0].any() and 0.4 < drawn.rows()[1:].mean() < 0.6


def test_default_batch_fits_the_budget():
    from oai_analysis_2_amd import stats
    assert stats.default_batch(30000, 10000, False) == (256 << 20) // (30000 * 8) // 16 * 16
    assert stats.default_batch(30000, 10000, True) == (256 << 20) // (30000 * 16) // 16 * 16
    assert stats.default_batch(30000, 7, False) == 7 and stats.default_batch(10 ** 9, 100, True) == 16
