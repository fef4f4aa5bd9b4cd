"""GPU: the rank-transform kernels (csrc/rank_transform.hip) against their restatement through scipy (tests/rank_transform_ref.py) --
ranks, valid counts, tie terms, rank sums and the rank and centred scores to the element -- and ThicknessCohort.ranked and the four rank
tests of oai_analysis_2_amd.stats end to end on a small sphere against scipy's own tests per vertex.

The normal score is the one output held to a tolerance: the device erfc, exp and log are not numpy's.  Measured on an MI355X over every
(n, twice_rank) with n <= 4096, the four named constants, and the extreme ranks of n = 2^22 (scripts/rank_transform_timing.py --error;
profiles/rank_transform.md): the largest |device - scipy.special.ndtri| is NORMAL_MEASURED = 1.33e-15; the gate NORMAL_GATE = 2.13e-14 is
16 times that.  Three Halley steps leave 4e-6, four leave this, a fifth changes nothing: the iteration has converged."""
import functools

import numpy as np
import pytest
import scipy.special
import scipy.stats
import torch

import rank_transform_ref as rref
from cohort_cases import cohort as _cohort, dev, icosphere, same_bits, sphere_atlas

pytestmark = pytest.mark.gpu

OWN = 16                                          # csrc/rank_transform.hip, kOwn: own rows per lane; a block owns 4 * OWN rows
VERTS = (1, 63, 65, 257, 600)                     # both sides of a wave (64) and of a block's vertices, several blocks
KNEES = (1, 2, OWN - 1, OWN, OWN + 1, 2 * OWN + 5, 65, 257)
NORMAL_MEASURED = 1.3322676295501878e-15          # 6 * 2^-52, the same for each of the four constants; 8.9e-16 at n = 2^22
NORMAL_GATE = 16 * NORMAL_MEASURED                # 2.13e-14
PLANTED = {"empty": 0, "single": 1, "equal": 2, "distinct": 3, "zeros_pair": 4, "extremes": 5, "nan": 6, "all_zero": 7, "some_zero": 8,
           "across_signs": 9}


@functools.lru_cache(maxsize=None)
def _case(N, V, masked):
    """(Y, mask) -- half the columns drawn from eight levels, so that large tie groups straddle row groups, half continuous -- with the
    header's corner cases planted where the shape has room (V >= 63)."""
    rng = np.random.default_rng([N, V, int(masked), 5])
    Y = rng.normal(0.0, 1.0, size=(N, V)).astype(np.float32)
    levels = np.array([-2.0, -0.75, -0.5, 0.0, 0.25, 0.5, 0.75, 3.0], np.float32)
    Y[:, ::2] = levels[rng.integers(0, 8, size=(N, (V + 1) // 2))]
    mask = rng.random((N, V)) >= 0.15 if masked else None
    if V >= 63:
        at = PLANTED
        if masked:
            mask[:, [at[k] for k in ("equal", "distinct", "zeros_pair", "extremes", "all_zero", "some_zero", "across_signs")]] = True
            mask[:, at["empty"]] = False
            mask[:, at["single"]] = np.arange(N) == N // 2
        else:
            Y[:, at["empty"]] = np.nan
            Y[np.arange(N) != N // 2, at["single"]] = np.nan
        Y[:, at["equal"]] = 1.25
        Y[:, at["distinct"]] = rng.permutation(N).astype(np.float32) - np.float32(N // 2)
        Y[:, at["zeros_pair"]] = np.arange(1, N + 1, dtype=np.float32) * np.where(np.arange(N) % 2 == 0, -1, 1)
        Y[:2, at["zeros_pair"]] = (-0.0, 0.0)[:min(N, 2)]
        Y[:4, at["extremes"]] = np.array([1e-45, -1e-45, np.inf, -np.inf], np.float32)[:min(N, 4)]
        Y[N // 2, at["nan"]] = np.nan
        Y[:, at["all_zero"]] = 0.0
        Y[::3, at["some_zero"]] = 0.0
        Y[:2, at["across_signs"]] = (-1.5, 1.5)[:min(N, 2)]
    for a in (Y, mask):
        if a is not None:
            a.setflags(write=False)
    return Y, mask


@functools.lru_cache(maxsize=None)
def _reference(N, V, masked, signed):
    got = rref.column_ranks(*_case(N, V, masked), signed)
    for a in got:
        a.setflags(write=False)
    return got


def _ranks_into_sentinels(y_d, m_d, signed):
    """oai_column_ranks through the one call path, into buffers pre-filled with a sentinel: every element must be written."""
    from oai_analysis_2_amd import _lib
    N, V = y_d.shape
    tr = torch.full((N, V), -77, dtype=torch.int32, device="cuda")
    n = torch.full((V,), -77, dtype=torch.int32, device="cuda")
    tie = torch.full((V,), -77, dtype=torch.int64, device="cuda")
    _lib.call("oai_column_ranks", y_d.data_ptr(), None if m_d is None else m_d.data_ptr(), N, V, int(signed), tr.data_ptr(), n.data_ptr(),
              tie.data_ptr(), _lib.STREAM, device=y_d.device)
    return tr, n, tie


@pytest.mark.parametrize("signed", [False, True], ids=["plain", "signed"])
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "no_mask"])
def test_ranks_counts_and_tie_terms_equal_the_restatement_to_the_element(masked, signed):
    from oai_analysis_2_amd import ops
    for N in KNEES:
        for V in VERTS:
            Y, mask = _case(N, V, masked)
            tr_ref, n_ref, tie_ref = _reference(N, V, masked, signed)
            y_d, m_d = dev(Y), None if mask is None else dev(mask.astype(np.uint8))
            where = f"N={N} V={V}"
            tr, n, tie = _ranks_into_sentinels(y_d, m_d, signed)
            same_bits(tr, tr_ref, f"{where} twice_rank")
            same_bits(n, n_ref, f"{where} n_valid")
            same_bits(tie, tie_ref, f"{where} tie_term")
            again = ops.column_ranks(y_d, m_d, signed=signed)              # two runs are identical
            assert torch.equal(again.twice_rank, tr) and torch.equal(again.n_valid, n) and torch.equal(again.tie_term, tie), where
            if V >= 63:                                                    # on the restatement: what was planted is really there
                at = PLANTED
                assert n_ref[at["empty"]] == 0 and (tr_ref[:, at["empty"]] == 0).all()
                assert n_ref[at["single"]] == 1 and tr_ref[N // 2, at["single"]] in (2, -2, 0)
                assert (np.abs(tr_ref[:, at["equal"]]) == N + 1).all() and tie_ref[at["equal"]] == N ** 3 - N
                assert n_ref[at["all_zero"]] == (0 if signed else N)
                if N >= 2:
                    pair = tr_ref[:2, at["zeros_pair"]]
                    assert (pair == 0).all() if signed else pair[0] == pair[1] != 0          # -0.0 ties +0.0
                    assert abs(tr_ref[0, at["across_signs"]]) == abs(tr_ref[1, at["across_signs"]]) or not signed
                if signed and N >= 2:
                    assert tr_ref[0, at["across_signs"]] < 0 < tr_ref[1, at["across_signs"]]
                if not signed and N >= 4:
                    assert tr_ref[2, at["extremes"]] == 2 * n_ref[at["extremes"]] and tr_ref[3, at["extremes"]] == 2
                    assert tie_ref[at["distinct"]] == 0
                if not masked:
                    assert tr_ref[N // 2, at["nan"]] == 0 and (signed or n_ref[at["nan"]] == N - 1)      # NaN under a null mask is missing


SUM_SHAPES = ((1, 65), (OWN + 1, 63), (65, 257), (257, 600), (1030, 65))   # 1030: past the 1024 labels that one launch carries


@pytest.mark.parametrize("shape", SUM_SHAPES, ids=lambda s: f"N{s[0]}_V{s[1]}")
def test_rank_sums_equal_the_restatement_to_the_element(shape):
    from oai_analysis_2_amd import _lib, ops
    N, V = shape
    Y, mask = _case(N, V, True)
    for signed in (False, True):
        tr_ref, _, _ = _reference(N, V, True, signed)
        tr = ops.column_ranks(dev(Y), dev(mask.astype(np.uint8)), signed=signed).twice_rank
        same_bits(tr, tr_ref, f"N={N} V={V} twice_rank")
        cases = [(G, np.random.default_rng([N, V, G]).integers(0, G, size=N).astype(np.uint8)) for G in (1, 2, 3, 16)] + [(2, None)]
        for G, labels in cases:
            n_ref, sum_ref = rref.rank_sums(tr_ref, labels, G)
            n_g = torch.full((G, V), -77, dtype=torch.int32, device="cuda")
            sums = torch.full((G, V), -77, dtype=torch.int64, device="cuda")
            _lib.call("oai_rank_sums", tr.data_ptr(), None if labels is None else labels.ctypes.data, N, V, G, n_g.data_ptr(), sums.data_ptr(),
                      _lib.STREAM, device=tr.device)
            what = f"N={N} V={V} signed={signed} G={G} labels={'sign' if labels is None else 'given'}"
            same_bits(n_g, n_ref, what + " n_g")
            same_bits(sums, sum_ref, what + " twice_sum_g")
            got = ops.rank_sums(tr, labels, G)
            assert torch.equal(got[0], n_g) and torch.equal(got[1], sums), what
    with pytest.raises(ValueError):
        ops.rank_sums(tr, np.full(N, 3), 3)
    with pytest.raises(ValueError):
        ops.rank_sums(tr, None, 3)


def test_rank_and_centred_scores_are_bit_equal_and_normal_scores_lie_within_the_gate():
    from oai_analysis_2_amd import ops
    worst = 0.0
    for N, V in ((1, 63), (OWN + 1, 65), (65, 257), (257, 600)):
        Y, mask = _case(N, V, True)
        for signed in (False, True):
            tr_ref, n_ref, _ = _reference(N, V, True, signed)
            ranks = ops.column_ranks(dev(Y), dev(mask.astype(np.uint8)), signed=signed)
            for kind in ("rank", "centred"):
                score, m = ops.rank_scores(ranks.twice_rank, ranks.n_valid, kind)
                want, want_m = rref.rank_scores(tr_ref, n_ref, kind)
                same_bits(score, want, f"N={N} V={V} signed={signed} {kind}")
                same_bits(m, want_m, f"N={N} V={V} signed={signed} {kind} mask")
            for name, c in rref.CONSTANTS.items():
                score, m = ops.rank_scores(ranks.twice_rank, ranks.n_valid, "normal", c)
                want, want_m = rref.rank_scores(tr_ref, n_ref, "normal", c)
                same_bits(m, want_m, f"N={N} V={V} signed={signed} normal mask")
                worst = max(worst, float(np.abs(score.cpu().numpy() - want).max()))
    print(f"largest |device - ndtri| on the planted cases: {worst:.3e} (gate {NORMAL_GATE:.3e})")
    assert worst <= NORMAL_GATE


def _every_rank(n_lo, n_hi):
    """twice_rank int32 [2 n_hi - 1, n_hi - n_lo + 1] and n_valid: column k holds every twice_rank 2 .. 2 n of n = n_lo + k, 0 below."""
    n = np.arange(n_lo, n_hi + 1, dtype=np.int32)
    tr = np.arange(2, 2 * n_hi + 1, dtype=np.int32)[:, None] * np.ones((1, len(n)), np.int32)
    return np.where(tr <= 2 * n[None, :], tr, 0).astype(np.int32), n


def test_normal_scores_of_every_rank_lie_within_the_gate_of_scipys_ndtri():
    """Every (n, twice_rank) with n <= 256, n = 1000 and n = 4096 whole, and the extreme ranks of n = 2^22, for the four named
    constants; scripts/rank_transform_timing.py --error measures every n <= 4096."""
    from oai_analysis_2_amd import ops
    big = 1 << 22
    cases = [_every_rank(1, 256), _every_rank(1000, 1000), _every_rank(4096, 4096),
             (np.array([2, 3, 4, 2 * big - 2, 2 * big - 1, 2 * big, -2, -2 * big], np.int32)[:, None], np.array([big], np.int32))]
    worst = 0.0
    for tr, n in cases:
        tr_d, n_d = dev(tr), dev(n)
        for name, c in rref.CONSTANTS.items():
            score, _ = ops.rank_scores(tr_d, n_d, "normal", c)
            want, _ = rref.rank_scores(tr, n, "normal", c)
            got = score.cpu().numpy()
            assert np.isfinite(got).all(), name
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"largest |device - ndtri|: {worst:.3e} (measured {NORMAL_MEASURED:.3e}, gate {NORMAL_GATE:.3e})")
    assert worst <= NORMAL_GATE


# ---- end to end on the icosphere -------------------------------------------------------------------------------------------------------
N_E2E = 24


@functools.lru_cache(maxsize=None)
def _e2e(missing):
    """(Y, Yb, mask, maskb): N_E2E knees on the 642 vertices, quantised to 1/8 so that ties (and zero differences) occur."""
    rng = np.random.default_rng([11, int(missing)])
    V = len(icosphere()[0])
    Y = (np.rint(8.0 * rng.normal(2.0, 0.5, size=(N_E2E, V))) / 8.0).astype(np.float32)
    Yb = (Y + np.rint(4.0 * rng.normal(0.1, 0.4, size=(N_E2E, V))) / 4.0).astype(np.float32)
    mask = rng.random((N_E2E, V)) >= 0.1 if missing else np.ones((N_E2E, V), bool)
    maskb = rng.random((N_E2E, V)) >= 0.1 if missing else np.ones((N_E2E, V), bool)
    for a in (Y, Yb, mask, maskb):
        a.setflags(write=False)
    return Y, Yb, mask, maskb


def test_ranked_leaves_the_original_untouched_and_carries_the_settings_over():
    from oai_analysis_2_amd import stats
    Y, _, mask, _ = _e2e(True)
    atlas = sphere_atlas()
    cohort = _cohort(atlas, Y, mask=mask, chunk=7)
    cohort.ids = [f"knee{i}" for i in range(N_E2E)]
    cohort.smoothing, cohort.change = "a smoothing", "a change"           # any object: they are carried, not read
    before_values, before_mask = cohort.values.clone(), cohort.mask.clone()
    tr_ref, n_ref, tie_ref = rref.column_ranks(Y, mask)
    for method, kind, signed in (("rank", "rank", False), ("centred", "centred", False), ("inormal", "normal", False), ("signed", "rank", True),
                                 ("signed_inormal", "normal", True)):
        ranked = cohort.ranked(method)
        assert torch.equal(cohort.values, before_values) and torch.equal(cohort.mask, before_mask) and cohort.ranking is None
        assert ranked.ids == cohort.ids and ranked.ids is not cohort.ids and ranked.smoothing == "a smoothing" and ranked.change == "a change"
        assert ranked.ranking.method == method and ranked.ranking.c == (0.375 if kind == "normal" else None)
        tr, n, tie = rref.column_ranks(Y, mask, signed)
        want, want_mask = rref.rank_scores(tr, n, kind, 0.375)
        same_bits(ranked.mask, want_mask, f"{method} mask")
        same_bits(ranked.ranking.n_valid, n, f"{method} n_valid")
        same_bits(ranked.ranking.tie_term, tie, f"{method} tie_term")
        got = ranked.values.cpu().numpy()
        assert got.dtype == np.float32
        if kind != "normal":
            assert np.array_equal(got, want.astype(np.float32)), method
        else:                                                              # every entry within one float32 ulp of the float32 of scipy's value
            w32 = want.astype(np.float32)
            ulp = np.maximum(np.spacing(np.abs(w32)), np.spacing(np.abs(got)))
            assert (np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= ulp).all(), method
        with pytest.raises(ValueError, match="already ranked"):
            ranked.ranked()
    assert cohort.ranked("inormal", c="rankit").ranking.c == 0.5 and cohort.ranked("inormal", c=0.25).ranking.c == 0.25
    with pytest.raises(ValueError):
        cohort.ranked("ranks")
    with pytest.raises(ValueError):
        cohort.ranked("inormal", c=0.75)


def test_difference_matches_rows_by_id_as_paired_test_does():
    from oai_analysis_2_amd import stats
    Y, Yb, mask, maskb = _e2e(True)
    atlas = sphere_atlas()
    a = _cohort(atlas, Y, mask=mask, chunk=7)
    order = np.random.default_rng(13).permutation(N_E2E)
    b = _cohort(atlas, Yb[order], mask=maskb[order], chunk=7)
    b.ids = [int(i) for i in order]                                       # row k of b is knee order[k]
    diff = a.difference(b)
    both = mask & maskb
    assert diff.ids == a.ids and diff.ranking is None
    assert np.array_equal(diff.values.cpu().numpy(), np.where(both, Y - Yb, np.float32(0.0)).astype(np.float32))
    assert np.array_equal(diff.mask.cpu().numpy() != 0, both)
    paired = stats.paired_test(a, b, n_permutations=32, seed=2)
    alone = stats.one_sample_test(diff, n_permutations=32, seed=2)
    for name in ("t", "mean_difference", "n1", "p_fwer"):
        same_bits(getattr(alone, name), getattr(paired, name), f"one_sample_test(a.difference(b)) against paired_test(a, b): {name}")
    with pytest.raises(ValueError, match="rank"):
        a.ranked().difference(b)
    b.ids[0] = "another knee"
    with pytest.raises(ValueError, match="same ids"):
        a.difference(b)


def _pearson(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("missing", [False, True], ids=["complete", "missing"])
def test_the_four_rank_tests_give_the_classical_statistics_per_vertex(missing):
    from oai_analysis_2_amd import stats
    Y, Yb, mask, maskb = _e2e(missing)
    V = Y.shape[1]
    atlas = sphere_atlas()
    a, b = _cohort(atlas, Y, mask=mask, chunk=7), _cohort(atlas, Yb, mask=maskb, chunk=7)
    groups = (np.arange(N_E2E) % 3 == 0).astype(np.int64)
    levels = np.arange(N_E2E) % 3 + 5
    x = np.random.default_rng(12).integers(0, 7, size=N_E2E).astype(np.float64)
    P = 64

    # rank sum: U, and the test itself is two_sample_test of the ranked cohort
    res = stats.rank_sum_test(a, groups, n_permutations=P, seed=3)
    direct = stats.two_sample_test(a.ranked(), groups, n_permutations=P, seed=3)
    for name in ("t", "p_uncorrected", "p_fwer"):
        same_bits(getattr(res.test, name), getattr(direct, name), f"rank_sum_test .test.{name}")
    u_ref, n1_ref, n2_ref = rref.mann_whitney_u1(Y, mask, groups == 1)
    assert np.array_equal(res.u1, u_ref) and np.array_equal(res.n1, n1_ref) and np.array_equal(res.n2, n2_ref)
    assert np.array_equal(res.tie_term, rref.column_ranks(Y, mask)[2])
    if not missing:
        for v in range(V):
            assert res.u1[v] == scipy.stats.mannwhitneyu(Y[groups == 1, v], Y[groups == 0, v]).statistic, v
        assert np.array_equal(res.auc, res.u1 / (8.0 * 16.0))
    inormal = stats.rank_sum_test(a, groups, scores="inormal", n_permutations=P, seed=3)
    assert np.array_equal(inormal.u1, res.u1)
    same_bits(inormal.test.t, stats.two_sample_test(a.ranked("inormal"), groups, n_permutations=P, seed=3).t, "rank_sum_test inormal t")

    # signed rank: W of a - b, through difference() or not
    res = stats.signed_rank_test(a, b, n_permutations=P, seed=4)
    diff = a.difference(b)
    same = stats.signed_rank_test(diff, n_permutations=P, seed=4)
    for name in ("w_plus", "w_minus", "n_nonzero", "rank_biserial"):
        same_bits(getattr(res, name), getattr(same, name), f"signed_rank_test {name}")
    same_bits(res.test.t, same.test.t, "signed_rank_test .test.t")
    same_bits(res.test.t, stats.one_sample_test(diff.ranked("signed"), n_permutations=P, seed=4).t, "signed_rank_test against one_sample_test")
    both = mask & maskb
    d = np.where(both, Y - Yb, np.float32(0.0)).astype(np.float32)
    assert np.array_equal(diff.values.cpu().numpy(), d) and np.array_equal(diff.mask.cpu().numpy() != 0, both)
    wp, wm, nz = rref.signed_rank_w(d, both)
    assert np.array_equal(res.w_plus, wp) and np.array_equal(res.w_minus, wm) and np.array_equal(res.n_nonzero, nz)
    assert (d == 0)[both].any(), "the case holds zero differences"
    for v in range(V):
        dv = d[both[:, v], v].astype(np.float64)
        assert min(res.w_plus[v], res.w_minus[v]) == scipy.stats.wilcoxon(dv, zero_method="wilcox", method="approx").statistic, v
    assert np.allclose(res.rank_biserial, (wp - wm) / (wp + wm), rtol=0, atol=1e-15)

    # Kruskal-Wallis: H
    res = stats.kruskal_test(a, levels, n_permutations=P, seed=5)
    same_bits(res.test.f, stats.anova_test(a.ranked(), levels, n_permutations=P, seed=5).f, "kruskal_test .test.f")
    assert np.array_equal(res.levels, [5, 6, 7])
    h_ref = rref.kruskal_h(Y, mask, levels - 5, 3)
    assert np.array_equal(np.isnan(res.h), np.isnan(h_ref)) and np.all(np.abs(res.h - h_ref)[~np.isnan(h_ref)] <= 1e-12 * np.abs(h_ref)[~np.isnan(h_ref)])
    for v in range(V):
        want = scipy.stats.kruskal(*[Y[(levels == g) & mask[:, v], v] for g in (5, 6, 7)]).statistic
        assert abs(res.h[v] - want) <= 1e-12 * abs(want), (v, res.h[v], want)

    # Spearman: rho
    res = stats.spearman_test(a, x, n_permutations=P, seed=6)
    rx = scipy.stats.rankdata(x)
    same_bits(res.test.t, stats.regression_test(a.ranked(), rx, n_permutations=P, seed=6).t, "spearman_test .test.t")
    tr, _, _ = rref.column_ranks(Y, mask)
    for v in range(V):
        ok = mask[:, v]
        assert abs(res.rho[v] - _pearson(0.5 * tr[ok, v], rx[ok])) <= 1e-12, v      # the rank regression over the valid knees
        if not missing:
            assert abs(res.rho[v] - scipy.stats.spearmanr(Y[:, v], x).statistic) <= 1e-12, v
