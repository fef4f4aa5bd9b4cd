"""GPU: the cohort-regression kernels (csrc/group_regression.hip) against their numpy restatement (tests/group_regression_ref.py) --
prepared block, t tile, slope, max |t| and the exceedance counts to the bit -- and oai_analysis_2_amd.stats.regression_test end to end on
a small sphere.  Every float64 is the result of IEEE add / subtract / multiply / divide / sqrt in a stated order, so equality is exact."""
import functools

import numpy as np
import pytest
import torch

import group_regression_ref as rref
import group_stats_ref as gref
from cohort_cases import bare_atlas, cohort as _cohort, design, icosphere, knees as _knees, rows as _rows, same_bits, sphere_atlas

pytestmark = pytest.mark.gpu

COLUMNS = (1, 2, 4, 6)                            # p: no nuisance column at all; the intercept alone; two sizes of the kernels' rows per thread
VERTS = (1, 63, 65, 257, 600)                     # both sides of a wave (64) and of a block's 256 vertices, several blocks


def _rows_per_thread(p, masked):                  # csrc/group_regression.hip, rows_per_thread
    return {1: 16, 2: 8, 4: 2, 6: 1}[p] if masked else {1: 16, 2: 16, 4: 8, 6: 8}[p]


def _batch(p, masked):
    """One full row group and a ragged one."""
    r = _rows_per_thread(p, masked)
    return r + max(1, r // 4)


PLANTED = {"empty": 1, "dof0": 2, "dof1": 3, "constant": 4, "nuisance": 5, "x_sometimes": 6}


@functools.lru_cache(maxsize=None)
def _case(N, V, p, masked):
    """(Y, mask, design, perm) with the header's corner cases planted where the shape has room (V >= 8, and for the last two N >= 31)."""
    rng = np.random.default_rng([N, V, p, int(masked)])
    D = design(N, p, rng)
    Y = (2.0 + 0.5 * rng.normal(size=(N, V)) + 0.3 * D[:, -1:] * rng.random(V)[None, :]).astype(np.float32)
    mask = rng.random((N, V)) >= 0.1 if masked else None
    P = max(_rows(_batch(p, masked)))
    perm = np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(P - 1)]).astype(np.int32)
    perm[1, 0], perm[1, N - 1] = -5, N + 3                                # out of range: clamped to knee 0 and knee N - 1
    if V >= 8:
        Y[:, PLANTED["constant"]] = 0.0                                   # exactly constant: every residual is 0.0, s2 == 0
        if masked:
            mask[:, PLANTED["constant"]] = True
            mask[:, PLANTED["empty"]] = False
            for name, keep in (("dof0", p), ("dof1", p + 1)):
                mask[:, PLANTED[name]] = np.arange(N) < keep
            if N >= 31 and p in (4, 6):
                mask[:, PLANTED["nuisance"]] = D[:, 1] == 1.0             # the sex dummy is constant among the valid knees
            if N >= 31 and p in (2, 4):
                few = p + 2
                mask[:, PLANTED["x_sometimes"]] = np.arange(N) < few      # few valid knees; row 3 hands them design rows whose x is 0
                zeros = np.nonzero(D[:, -1] == 0.0)[0][:few]
                rest = np.setdiff1d(np.arange(N), zeros)
                perm[3, :few], perm[3, few:] = zeros, rng.permutation(rest)
    for a in (Y, mask, D, perm):
        if a is not None:
            a.setflags(write=False)
    return Y, mask, D, perm


@functools.lru_cache(maxsize=None)
def _reference(N, V, p, masked):
    Y, mask, D, perm = _case(N, V, p, masked)
    prep = rref.prepare(Y, mask, D[:, :-1] if p > 1 else None, centre=p > 1)
    t, slope = rref.regression_t(prep, mask, D, perm, with_slope=True)
    t.setflags(write=False)
    return prep, t, slope


def _prepare_device(Y, mask, D):
    from oai_analysis_2_amd import ops
    p = D.shape[1]
    return ops.regression_prepare(torch.from_numpy(np.array(Y)).cuda(), None if mask is None else torch.from_numpy(mask.astype(np.uint8)).cuda(),
                                  torch.from_numpy(np.ascontiguousarray(D[:, :-1])).cuda() if p > 1 else None, centre=p > 1)


def _device(prep, D, perm, batch):
    from oai_analysis_2_amd import ops
    P, V = perm.shape[0], prep.n_verts
    design, index = torch.from_numpy(np.array(D)).cuda(), torch.from_numpy(np.array(perm)).cuda()
    t0 = torch.full((V,), 7.0, dtype=torch.float64, device="cuda")
    slope0 = torch.full((V,), 7.0, dtype=torch.float64, device="cuda")
    max_abs = torch.full((P,), -1.0, dtype=torch.float64, device="cuda")
    exceed = torch.full((V,), -5, dtype=torch.int64, device="cuda")            # garbage: the first batch must start it
    tiles = []
    for p0 in range(0, P, batch):
        p1 = min(p0 + batch, P)
        tile = ops.regression_t(prep, design, index, p0, p1, slope0=slope0)    # later batches must leave slope0 alone
        ops.permutation_reduce(tile, p0, t0, max_abs, exceed)
        tiles.append(tile.clone())
    return torch.cat(tiles), slope0, t0, max_abs, exceed


def _planted_cases_occur(N, V, p, ref, t_ref):
    """On the restatement: every corner case that was planted is really there."""
    at = PLANTED
    assert np.isnan(t_ref[:, at["constant"]]).all() and ref["Q"][at["constant"]] == 0.0 and ref["ok"][at["constant"]] == 1
    assert np.isnan(t_ref[:, at["empty"]]).all() and ref["n"][at["empty"]] == 0 and np.isnan(ref["mean"][at["empty"]]) and ref["ok"][at["empty"]] == 0
    if N > p:
        assert ref["n"][at["dof0"]] == p and ref["ok"][at["dof0"]] == 0 and np.isnan(t_ref[:, at["dof0"]]).all()
    if N >= 7:
        assert ref["n"][at["dof1"]] == p + 1 and ref["ok"][at["dof1"]] == 1 and not np.isnan(t_ref[0, at["dof1"]])
    if N >= 31 and p in (4, 6):
        assert ref["ok"][at["nuisance"]] == 0 and ref["n"][at["nuisance"]] >= p + 1 and np.isnan(t_ref[:, at["nuisance"]]).all()
    if N >= 31 and p in (2, 4):
        col = t_ref[:, at["x_sometimes"]]
        assert ref["ok"][at["x_sometimes"]] == 1 and not np.isnan(col[0]) and np.isnan(col[3]) and not np.isnan(col).all()


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "no_mask"])
@pytest.mark.parametrize("p", COLUMNS)
def test_prepared_block_t_slope_max_and_exceed_equal_the_restatement_to_the_bit(p, masked):
    batch = _batch(p, masked)
    for N in _knees(p):
        for V in VERTS:
            Y, mask, D, perm = _case(N, V, p, masked)
            ref, t_ref, slope_ref = _reference(N, V, p, masked)
            prep = _prepare_device(Y, mask, D)
            for name in ("R", "Q", "mean", "n", "ok"):
                same_bits(getattr(prep, name), ref[name], f"N={N} V={V} prepare.{name}")
            for P in _rows(_batch(p, masked)):
                t, slope0, t0, max_abs, exceed = _device(prep, D, perm[:P], batch)
                where = f"N={N} V={V} P={P}"
                same_bits(t, t_ref[:P], f"{where} t")
                same_bits(slope0, slope_ref, f"{where} slope0")
                same_bits(t0, t_ref[0], f"{where} t0")
                want_max, want_exceed = gref.reduce_tiles(t_ref[:P])
                same_bits(max_abs, want_max, f"{where} max_abs")
                same_bits(exceed, want_exceed, f"{where} exceed")
            assert not np.isnan(t_ref[:, 0]).any() or N < 31                    # an ordinary vertex has a t in every row
            clamped = np.array(perm[1])
            clamped[0], clamped[N - 1] = 0, N - 1
            assert perm[1].min() < 0 and perm[1].max() >= N
            assert np.array_equal(t_ref[1], rref.regression_t(ref, mask, D, clamped[None, :])[0], equal_nan=True)
            if masked and V >= 8:
                _planted_cases_occur(N, V, p, ref, t_ref)


@pytest.mark.parametrize("p", COLUMNS)
def test_no_mask_gives_the_bits_of_a_mask_of_all_ones(p):
    N, V = 33, 257
    Y, _, D, perm = _case(N, V, p, False)
    ref, t_ref, slope_ref = _reference(N, V, p, False)
    ones = np.ones((N, V), bool)
    bare, full = _prepare_device(Y, None, D), _prepare_device(Y, ones, D)
    assert bare.mask is None and full.mask is not None and (ref["n"] == N).all()
    for name in ("R", "Q", "mean", "n", "ok"):
        same_bits(getattr(full, name), ref[name], f"prepare.{name} (all ones)")
    for prep, batch, what in ((bare, _batch(p, False), "no mask"), (full, _batch(p, True), "all ones")):      # two kernels, two row groupings
        t, slope0, _, max_abs, exceed = _device(prep, D, perm, batch)
        same_bits(t, t_ref, f"t ({what})")
        same_bits(slope0, slope_ref, f"slope0 ({what})")
        same_bits(max_abs, gref.reduce_tiles(t_ref)[0], f"max_abs ({what})")
        same_bits(exceed, gref.reduce_tiles(t_ref)[1], f"exceed ({what})")


# ---- the public interface --------------------------------------------------------------------------------------------------------------
def test_exhaustive_counts_lie_in_scipys_band():
    """N = 6, a dummy x of 3 + 3, the intercept alone, V = 65, all 720 permutations.  Each of the 20 labellings occurs 3! 3! = 36 times,
    and a labelling and its complement tie up to rounding, so an exact count against an independent implementation is not defined: the
    device count must lie between 36 times scipy's counts with the comparison tightened and loosened by 1e-9 relative."""
    import itertools
    import scipy.stats
    from oai_analysis_2_amd import stats
    rng = np.random.default_rng(6)
    Y = rng.normal(2.0, 0.5, size=(6, 65)).astype(np.float32)
    x = np.array([1, 0, 1, 1, 0, 0], np.float64)
    res = stats.regression_test(_cohort(bare_atlas(65), Y, chunk=7), x, n_permutations=10000, batch=100)
    assert res.exact and res.n_permutations == 720 and (res.n == 6).all() and (res.dof == 4).all()
    y = Y.astype(np.float64)
    labellings = [np.isin(np.arange(6), c) for c in itertools.combinations(range(6), 3)]
    a = np.abs(np.stack([scipy.stats.ttest_ind(y[r], y[~r], axis=0, equal_var=True).statistic for r in labellings]))
    observed = scipy.stats.ttest_ind(y[x == 1], y[x == 0], axis=0, equal_var=True).statistic
    assert len(labellings) == 20 and np.abs(res.t - observed).max() < 1e-10
    count = np.rint(res.p_uncorrected * 720).astype(np.int64)
    low, high = (a >= np.abs(observed) * (1 + 1e-9)).sum(axis=0), (a >= np.abs(observed) * (1 - 1e-9)).sum(axis=0)
    print("exceed", count.tolist(), "band width", (36 * (high - low)).tolist())
    assert (36 * low <= count).all() and (count <= 36 * high).all() and (count >= 36).all()
    assert np.allclose(res.slope, y[x == 1].mean(axis=0) - y[x == 0].mean(axis=0), rtol=1e-10, atol=1e-13)


N_E2E, P_E2E, T_CLUSTER = 40, 400, 6.0


@functools.lru_cache(maxsize=None)
def _painted(effect):
    """40 knees on the sphere: 2 mm + 0.1 mm noise + 0.02 mm per year of age over 60 everywhere, and ``effect`` mm per unit of a
    continuous x on the cap z > 0.8.  The covariates are age and a sex dummy."""
    verts, _ = icosphere()
    cap = verts[:, 2] > 0.8
    rng = np.random.default_rng(2025)
    age = rng.uniform(45, 80, N_E2E)
    sex = (rng.random(N_E2E) < 0.5).astype(np.float64)
    x = rng.normal(0.0, 1.0, N_E2E)
    Y = 2.0 + 0.1 * rng.normal(size=(N_E2E, len(verts))) + 0.02 * (age - 60)[:, None]
    Y[:, cap] += effect * x[:, None]
    return Y.astype(np.float32), x, np.stack([age, sex], axis=1), cap


def _restated(Y, mask, x, cov, index):
    Z, D, scale = rref.design_columns(x, cov, True)
    t, slope = rref.regression_t(rref.prepare(Y, mask, Z), mask, D, index, with_slope=True)
    return t, slope / scale


FIELDS = ("t", "n", "dof", "slope", "partial_r", "p_uncorrected", "p_fwer", "max_abs", "cluster_label", "max_extent")


def test_regression_end_to_end_finds_the_painted_cap_and_is_reproducible():
    from oai_analysis_2_amd import mesh_processing as mp, stats
    Y, x, cov, cap = _painted(0.5)
    atlas = sphere_atlas()
    kwargs = dict(covariates=cov, n_permutations=P_E2E, cluster_threshold=T_CLUSTER, seed=1)
    res = stats.regression_test(_cohort(atlas, Y, chunk=7), x, batch=96, **kwargs)
    assert res.n_permutations == P_E2E and not res.exact and res.max_abs.shape == (P_E2E,) and res.max_extent.shape == (P_E2E,)
    assert (res.n == N_E2E).all() and (res.dof == N_E2E - 4).all()
    big = max(res.clusters, key=lambda c: c.extent)
    members = res.cluster_label == big.label
    assert big.sign == 1 and members[cap].all() and big.extent == members.sum() >= cap.sum()
    assert big.p_cluster == 1.0 / P_E2E                                    # the smallest value P permutations can give
    area, _ = mp.mesh_areas(atlas.inner["FC"])
    assert big.area == pytest.approx(area[members].sum(), rel=1e-12) and res.max_extent[0] == big.extent
    assert (res.p_fwer[cap] == 1.0 / P_E2E).all() and (np.abs(res.slope[cap] - 0.5) < 0.15).all()
    assert np.array_equal(res.partial_r, res.t / np.sqrt(res.t * res.t + res.dof)) and (res.partial_r[cap] > 0.9).all()
    # the device against the restatement through the public interface, batches and all
    perms = stats.index_permutations(N_E2E, P_E2E, seed=1)
    t_ref, slope_ref = _restated(Y, None, x, cov, perms.index)
    same_bits(res.t, t_ref[0], "t")
    same_bits(res.max_abs, gref.reduce_tiles(t_ref)[0], "max_abs")
    assert np.array_equal(np.rint(res.p_uncorrected * P_E2E).astype(np.int64), gref.reduce_tiles(t_ref)[1])
    assert np.allclose(res.slope, slope_ref, rtol=1e-14, atol=0)           # un-scaled on the host: one division
    # a second run on the same input: the same bits in every field
    again = stats.regression_test(_cohort(atlas, Y, chunk=7), x, batch=96, **kwargs)
    for name in FIELDS:
        same_bits(getattr(again, name), getattr(res, name), name)
    assert again.clusters == res.clusters
    # another batch size changes nothing either, nor do the rows handed over instead of drawn
    for other, what in ((stats.regression_test(_cohort(atlas, Y, chunk=7), x, **kwargs), "default batch"),
                        (stats.regression_test(_cohort(atlas, Y, chunk=7), x, batch=37, covariates=cov, cluster_threshold=T_CLUSTER, permutations=perms.index), "batch 37")):
        for name in FIELDS:
            same_bits(getattr(other, name), getattr(res, name), f"{name} ({what})")
        assert other.clusters == res.clusters


def test_without_an_effect_the_corrected_p_is_the_rank_of_the_observed_maximum():
    from oai_analysis_2_amd import stats
    Y, x, cov, _ = _painted(0.0)
    res = stats.regression_test(_cohort(sphere_atlas(), Y, chunk=7), x, covariates=cov, n_permutations=P_E2E, seed=2, batch=64)
    assert not np.isnan(res.t).any() and res.cluster_label is None and res.clusters == []
    assert (res.p_fwer >= res.p_uncorrected).all()
    assert res.p_fwer.min() == (res.max_abs >= res.max_abs[0]).sum() / P_E2E
    assert res.max_abs[0] == np.abs(res.t).max()


def test_what_the_cohort_calls_missing_reaches_the_kernel_as_missing():
    from oai_analysis_2_amd import stats
    from oai_analysis_2_amd.thickness import KneeThickness
    rng = np.random.default_rng(12)
    N, V = 12, 70
    Y = (2.0 + 0.3 * rng.normal(size=(N, V))).astype(np.float32)
    Y[rng.random((N, V)) < 0.1] = np.nan
    Y[:, 9] = np.nan
    Y[:3, 9] = 2.0, 2.5, 1.5                                                # three knees for three columns: no t
    x, age = rng.normal(size=N), rng.uniform(45, 80, N)
    knees = [KneeThickness(Y[i], Y[i]) for i in range(N)]
    knees[4] = KneeThickness(Y[4], Y[4], errors={"FC": "no surface"})       # every entry of this knee is missing
    cohort = stats.ThicknessCohort.from_stream(enumerate(knees), bare_atlas(V), "FC")
    mask = ~np.isnan(Y)
    mask[4] = False
    assert np.array_equal(cohort.mask.cpu().numpy() != 0, mask)
    res = stats.regression_test(cohort, x, covariates=age, n_permutations=50, seed=4, batch=16)
    assert np.array_equal(res.n, mask.sum(axis=0)) and res.n[9] == 3 and np.isnan(res.t[9]) and np.isnan(res.p_fwer[9]) and np.isnan(res.slope[9])
    t_ref, slope_ref = _restated(np.where(mask, Y, 0).astype(np.float32), mask, x, age, stats.index_permutations(N, 50, seed=4).index)
    same_bits(res.t, t_ref[0], "t")
    same_bits(res.max_abs, gref.reduce_tiles(t_ref)[0], "max_abs")
    assert np.allclose(res.slope, slope_ref, rtol=1e-14, atol=0, equal_nan=True) and not np.isnan(np.delete(res.t, 9)).any()
