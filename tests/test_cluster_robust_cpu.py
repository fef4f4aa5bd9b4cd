"""CPU: the numpy restatement of the cluster-robust regression (tests/cluster_robust_ref.py; include/oai_hip.h, "Cluster-robust
regression") against independent code -- numpy's least squares and the explicit sandwich --, the identities the definition implies, the
calibration that motivates it, and the host side of ``stats.marginal_test``.  The fixtures (tests/cluster_robust_cases.py) are also those
of tests/test_cluster_robust_gpu.py, which holds the device to the restatement bit for bit."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import cluster_robust_ref as cref
import group_regression_ref as rref
import group_stats_ref as gref
from cluster_robust_cases import COLUMNS, KINDS, VERTS, case, counts_of, reference

LSTSQ_GATE = 1e-10                                # relative: the project's gate for a pin to numpy's least squares


def planted_cases_occur(block, t, counts, p):
    """On the restatement: every corner that ``hostile_case`` plants under a mask is really there."""
    at, S = cref.PLANTED, len(counts)
    assert block["G"][at["cluster_missing"]] == S - 1 and block["G"][0] == S
    assert block["G"][at["one_cluster"]] == 1 and block["okc"][at["one_cluster"]] == 0 and np.isnan(t[:, at["one_cluster"]]).all()
    assert block["okc"][at["rank"]] == 0 and np.isnan(t[:, at["rank"]]).all()
    if p in (2, 4) and block["n"][at["rank"]] > p:                          # (p = 6: the constant column is a nuisance one, so ok is 0 too)
        assert block["ok"][at["rank"]] == 1 and block["G"][at["rank"]] >= 2       # the null model is fine there: it is M that loses its rank


def test_at_least_half_the_vertices_of_every_case_have_a_t_and_the_planted_corners_occur():
    """The condition on the GPU test's cases, so that NaN-equality cannot hide a failure."""
    for kind in KINDS:
        for p in COLUMNS:
            for V in VERTS:
                for masked in (False, True):
                    block, t, slope0, se0 = reference(kind, V, p, masked)
                    finite = np.isfinite(t).all(axis=0)
                    assert 2 * int(finite.sum()) >= V, (kind, p, V, masked, int(finite.sum()))
                    assert np.array_equal(np.isfinite(slope0), np.isfinite(t[0])) and np.array_equal(np.isfinite(se0), np.isfinite(t[0]))
                    if masked and V >= 8:
                        planted_cases_occur(block, t, counts_of(kind, p), p)
                    if not masked:
                        assert finite.all() and (block["G"] == len(counts_of(kind, p))).all()


def _relative(a, b):
    both = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "the NaN positions differ"
    return float((np.abs(a - b)[both] / np.abs(b)[both]).max())


@pytest.mark.parametrize("p", (2, 4))
def test_the_restatement_agrees_with_lstsq_and_the_explicit_sandwich(p):
    """Row 0 and rebuilt y* rows of an unbalanced masked case against the dense route; measured here: 1.3e-12 relative at p = 2 and 1.2e-13 at p = 4."""
    Y, mask, D, offsets, flips = case("five", 63, p, True)
    _, t, _, _ = reference("five", 63, p, True)
    dense = cref.dense_t(Y, mask, D, offsets, flips[:6], centre=True)
    worst = _relative(t[:6], dense)
    print(f"p = {p}: restatement against lstsq + sandwich, largest relative distance {worst:.3g} (row 0: {_relative(t[:1], dense[:1]):.3g})")
    assert worst <= LSTSQ_GATE


def test_the_scores_of_a_row_sum_to_zero():
    """sum_s k_s = M a = e_p and sum_s u_s = a . b, so sum_s e_s = a . b - beta_p = 0 up to rounding -- for every flip row."""
    block, _, _, _ = reference("five", 63, 4, True)
    _, _, _, _, flips = case("five", 63, 4, True)
    ok = block["okc"] != 0
    for row in (flips[0], flips[2]):
        e = cref.scores(block, row)[:, ok]
        ratio = np.abs(e.sum(axis=0)) / np.abs(e).sum(axis=0)
        print(f"|sum of scores| / sum |score|: largest {ratio.max():.3g}")
        assert ratio.max() < 1e-12


def test_with_one_row_per_cluster_the_variance_is_whites_hc0_times_c():
    p = 4
    Y, _, D, offsets, _ = case("singletons", 65, p, False)
    block, _, slope0, se0 = reference("singletons", 65, p, False)
    N = len(Y)
    y = Y.astype(np.float64) - Y.astype(np.float64).mean(axis=0)
    beta = np.linalg.lstsq(D, y, rcond=None)[0]
    e = y - D @ beta
    bread = np.linalg.inv(D.T @ D)
    hc0 = np.array([(bread @ (D.T * e[:, v] ** 2) @ D @ bread)[-1, -1] for v in range(65)])
    c = (N / (N - 1)) * ((N - 1) / (N - p))
    assert np.array_equal(block["c"], np.full(65, c))
    assert np.abs(se0 ** 2 - c * hc0).max() <= LSTSQ_GATE * (c * hc0).max() and np.allclose(slope0, beta[-1], rtol=LSTSQ_GATE, atol=0)


def test_flipping_every_sign_leaves_abs_t_unchanged_to_the_bit():
    for kind, p in (("five", 4), ("word", 6), ("two", 1)):
        _, t, _, _ = reference(kind, 65, p, True)
        _, _, _, _, flips = case(kind, 65, p, True)
        assert not flips[0].any() and flips[1].all()
        assert np.array_equal(np.abs(t[1]).view(np.int64), np.abs(t[0]).view(np.int64)) and np.isfinite(t[0]).sum() >= 33


def test_the_order_of_the_clusters_changes_the_result_within_rounding_only():
    """Not to the bit: the order IS the contract."""
    p = 4
    Y, mask, D, offsets, flips = case("five", 65, p, True)
    _, t, _, _ = reference("five", 65, p, True)
    counts = counts_of("five", p)
    off = cref.clamp_offsets(offsets, len(Y))
    new = [3, 0, 4, 2, 1]
    rows = np.concatenate([np.arange(off[s], off[s + 1]) for s in new])
    offsets2 = np.concatenate([[0], np.cumsum([counts[s] for s in new])]).astype(np.int32)
    block2 = cref.prepare(Y[rows], mask[rows], D[rows], offsets2, centre=True)
    t2 = cref.cluster_t(block2, flips[:, new])
    worst = _relative(t2, t)
    print(f"clusters reordered: largest relative distance {worst:.3g}")
    assert worst <= LSTSQ_GATE


def test_the_packed_flip_rows_of_three_clusters_are_all_eight():
    from oai_analysis_2_amd import stats
    perms = stats.sign_flips(3, 10000, seed=0)
    assert perms.exact and len(perms) == 8 and not perms.rows()[0].any() and len({tuple(r) for r in perms.rows().tolist()}) == 8
    assert not stats.sign_flips(24, 500, seed=0).exact


# ---- the calibration that motivates the test -------------------------------------------------------------------------------------------------
CAL_SUBJECTS, CAL_VISITS, CAL_SIMS, CAL_RESAMPLES, CAL_SEED = 24, 4, 200, 200, 7


@functools.lru_cache(maxsize=None)
def calibration():
    """24 subjects x 4 visits, random intercept sd 0.3, noise sd 0.1, a between-subject group with NO effect; every simulation is one
    vertex.  Returns the rejections at p <= 0.05 of free permutation of the rows (the restated oai_regression_t) and of the wild cluster
    bootstrap (the restated oai_cluster_t), out of CAL_SIMS."""
    rng = np.random.default_rng(CAL_SEED)
    S, k, V, P = CAL_SUBJECTS, CAL_VISITS, CAL_SIMS, CAL_RESAMPLES
    N = S * k
    owner = np.repeat(np.arange(S), k)
    group = (np.arange(S) % 2).astype(np.float64)[owner]
    Y = (2.0 + 0.3 * rng.normal(size=(S, V))[owner] + 0.1 * rng.normal(size=(N, V))).astype(np.float32)
    Z, D, _ = rref.design_columns(group, None, True)
    index = np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(P - 1)])
    naive = rref.regression_t(rref.prepare(Y, None, Z), None, D, index)
    flips = rng.integers(0, 2, size=(P, S)).astype(bool)
    flips[0] = False
    offsets = np.arange(0, N + 1, k).astype(np.int32)
    robust = cref.cluster_t(cref.prepare(Y, None, D, offsets), flips)
    return tuple(int((gref.reduce_tiles(t)[1] / float(P) <= 0.05).sum()) for t in (naive, robust))


def test_free_permutation_of_clustered_rows_rejects_far_too_often_and_the_cluster_bootstrap_does_not():
    naive, robust = calibration()
    print(f"no effect, {CAL_SUBJECTS} subjects x {CAL_VISITS} visits, {CAL_SIMS} simulations, {CAL_RESAMPLES} resamples: free permutation of rows "
          f"rejects {naive} times at p <= 0.05, the wild cluster bootstrap {robust} times")
    assert naive > robust


# ---- the host side ---------------------------------------------------------------------------------------------------------------------
def _cpu_cohort(N, V, kind="FC"):
    """A cohort that lives on the host (its rows are set directly): enough for everything that is refused before a launch."""
    import torch
    from oai_analysis_2_amd import stats
    atlas = SimpleNamespace(inner={kind: SimpleNamespace(verts=np.zeros((V, 3), np.float32))}, device="cpu", image=None)
    cohort = stats.ThicknessCohort(atlas, kind)
    cohort._values = torch.from_numpy(np.random.default_rng(5).normal(2.0, 0.3, (N, V)).astype(np.float32))
    cohort._mask = torch.ones((N, V), dtype=torch.uint8)
    cohort.ids = list(range(N))
    return cohort


def _cpu_visits(subjects, years, V=12):
    from oai_analysis_2_amd import stats
    visits = stats.LongitudinalCohort.__new__(stats.LongitudinalCohort)
    visits.rows = _cpu_cohort(len(subjects), V)
    visits._subject, visits._years, visits._label = list(subjects), [float(y) for y in years], [None] * len(subjects)
    visits._seen = set(zip(visits._subject, visits._years))
    return visits


def test_years_and_per_row_follow_the_rows():
    visits = _cpu_visits(["b", "a", "b", "c", "a"], [0, 0, 1, 0, 2.5])
    assert visits.subjects == ["b", "a", "c"]
    assert visits.years.dtype == np.float64 and visits.years.tolist() == [0.0, 0.0, 1.0, 0.0, 2.5]
    assert visits.per_row([10, 20, 30]).tolist() == [10, 20, 10, 30, 20]
    assert visits.per_row({"a": 1.5, "b": 2.5, "c": 3.5, "z": 9.0}).tolist() == [2.5, 1.5, 2.5, 3.5, 1.5]
    assert visits.per_row(np.arange(6).reshape(3, 2)).tolist() == [[0, 1], [2, 3], [0, 1], [4, 5], [2, 3]]
    with pytest.raises(ValueError, match="one entry per subject"):
        visits.per_row([1, 2])
    with pytest.raises(ValueError, match="one entry per subject"):
        visits.per_row(3.0)
    with pytest.raises(ValueError, match="no value for subject 'c'"):
        visits.per_row({"a": 1, "b": 2})


def test_cluster_rows_orders_the_rows_cluster_major():
    from oai_analysis_2_amd import stats
    names, order, offsets = stats.cluster_rows(["b", "a", "b", "c", "a"])
    assert names == ["b", "a", "c"] and order.tolist() == [0, 2, 1, 4, 3] and offsets.tolist() == [0, 2, 4, 5] and offsets.dtype == np.int32


def test_marginal_test_refuses_before_any_launch():
    from oai_analysis_2_amd import stats
    subjects = [s for s in range(5) for _ in range(2)]
    visits = _cpu_visits(subjects, [0, 1] * 5)
    N, rng = 10, np.random.default_rng(0)
    x, cov = rng.normal(size=N), rng.normal(size=(N, 2))
    nan = x.copy()
    nan[3] = np.nan
    for target, kwargs, words in (
            (visits.rows, dict(x=x), "needs clusters="),
            (visits.rows, dict(x=x, clusters=subjects[:-1]), r"one label per row of the cohort \(10\), got 9"),
            (visits, dict(x=x, clusters=subjects + [7]), r"one label per row of the cohort \(10\), got 11"),
            (visits, dict(x=x, clusters=["same"] * N), "at least two clusters, got 1"),
            (visits, dict(x=nan), "NaN or an infinity"),
            (visits, dict(x=x, covariates=np.where(np.arange(N)[:, None] == 2, np.inf, cov)), "NaN or an infinity"),
            (visits, dict(x=x[:-1]), "x must hold one entry per knee"),
            (visits, dict(x=np.full(N, 2.0)), "x is constant"),
            (visits, dict(x=x, covariates=np.ones(N)), "covariate 0 is constant"),
            (visits, dict(x=x, covariates=np.stack([cov[:, 0], 2 * cov[:, 0] + 1], axis=1)), "full column rank"),
            (visits, dict(x=x, covariates=rng.normal(size=(N, 5))), "7 columns"),
            (visits, dict(x=x, flips=np.ones((4, 5), bool)), "row 0 of the flips must flip nothing"),
            (visits, dict(x=x, flips=np.zeros((4, 6), bool)), r"one bit per cluster \(5\)"),
            (visits, dict(x=x, cluster_threshold=-1.0), "cluster_threshold must be > 0"),
            (visits, dict(x=x, tfce="yes"), "tfce")):
        with pytest.raises(ValueError, match=words):
            stats.marginal_test(target, **kwargs)


def test_a_marginal_result_hands_its_maps_to_the_atlas_image():
    from oai_analysis_2_amd import stats
    V = 12
    vec = np.arange(V, dtype=np.float64)
    res = stats.MarginalResult(kind="FC", t=vec, slope=vec + 1, se=vec + 2, n=np.full(V, 9, np.int32), n_clusters=np.full(V, 4, np.int32),
                               dof=np.full(V, 3, np.int64), p_uncorrected=vec / V, p_fwer=vec / V, max_abs=np.ones(8), n_bootstrap=8, exact=True)
    atlas = SimpleNamespace(image=lambda v, kind: (kind, np.asarray(v).reshape(3, 4)))
    for what in ("t", "slope", "se", "p_fwer", "p_uncorrected", "n", "n_clusters"):
        kind, img = res.image(atlas, what)
        assert kind == "FC" and img.dtype == np.float32 and np.array_equal(img.reshape(-1), np.asarray(getattr(res, what), np.float32))
    with pytest.raises(ValueError, match="without tfce"):
        res.image(atlas, "tfce")
    with pytest.raises(ValueError, match="no image of"):
        res.image(atlas, "partial_r")
