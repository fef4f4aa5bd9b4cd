"""GPU: the kernels of the vertex-wise design columns (csrc/group_regression_vx.hip) against their numpy restatement
(tests/vertex_regression_ref.py) -- the prepared block with n_dropped, the effective mask and the completed columns, the t and F tiles,
row 0's coefficients, the max statistic and the exceedance counts to the bit --, and oai_analysis_2_amd.stats.regression_test / f_test with
``vertex_covariates`` end to end on a small sphere.  Every float64 is the result of IEEE add / subtract / multiply / divide / sqrt in a
stated order, so equality is exact.  The fixtures are tests/vertex_regression_cases.py's; tests/test_vertex_regression_cpu.py asserts that
their corner cases occur."""
import dataclasses

import numpy as np
import pytest
import torch

import group_f_ref as fref
import group_regression_ref as rref
import group_stats_ref as gref
import vertex_regression_ref as vref
from cohort_cases import cohort as _cohort, dev, restated_fields, same_bits, same_result, sphere_atlas
from vertex_regression_cases import (COMBOS, CONFOUND_ADJUSTED, CONFOUND_N, CONFOUND_P, CONFOUND_UNADJUSTED_CAP, VERTS, batch_rows, case, confound,
                                     confound_restated, knees, planted_cases_occur, reference, row_counts)

pytestmark = pytest.mark.gpu

PREPARED = ("R", "Q", "mean", "n", "ok", "n_dropped", "m", "WC")


def _prepare_device(Y, mask, W, wmask, nuisance, s_i, centre):
    from oai_analysis_2_amd import ops
    return ops.regression_vx_prepare(dev(Y), dev(mask, np.uint8), dev(W), dev(wmask, np.uint8),
                                     dev(nuisance) if nuisance is not None and nuisance.shape[1] else None, n_vertex_interest=s_i, centre=centre)


def _device(prep, D, perm, k, batch):
    """The tile of every row in batches of ``batch``, row 0's coefficient(s), and the running reduction: k = 0 the t kernel, else F."""
    from oai_analysis_2_amd import ops
    P, V = perm.shape[0], prep.n_verts
    design, index = (dev(D) if D.shape[1] else None), dev(perm)
    first = torch.full((V,), 7.0, dtype=torch.float64, device="cuda")
    out0 = torch.full((V,) if k == 0 else (k, V), 7.0, dtype=torch.float64, device="cuda")
    max_abs = torch.full((P,), -1.0, dtype=torch.float64, device="cuda")
    exceed = torch.full((V,), -5, dtype=torch.int64, device="cuda")            # garbage: the first batch must start it
    tiles = []
    for p0 in range(0, P, batch):
        p1 = min(p0 + batch, P)                                                # later batches must leave out0 alone
        tile = ops.regression_vx_t(prep, design, index, p0, p1, slope0=out0) if k == 0 else ops.regression_vx_f(prep, design, index, p0, p1, k, coef0=out0)
        ops.permutation_reduce(tile, p0, first, max_abs, exceed)
        tiles.append(tile.clone())
    return torch.cat(tiles), out0, first, max_abs, exceed


def _check(prep, D, perm, k, batch, tile_ref, out0_ref, where):
    for P in sorted(set(min(P, len(perm)) for P in where[1])):
        tile, out0, first, max_abs, exceed = _device(prep, D, perm[:P], k, batch)
        what = f"{where[0]} P={P} {'t' if k == 0 else 'F'}"
        same_bits(tile, tile_ref[:P], f"{what} tile")
        same_bits(out0, out0_ref, f"{what} row 0's coefficients")
        same_bits(first, tile_ref[0], f"{what} row 0")
        want_max, want_exceed = gref.reduce_tiles(tile_ref[:P])
        same_bits(max_abs, want_max, f"{what} max")
        same_bits(exceed, want_exceed, f"{what} exceed")


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "p%d_sn%d_si%d" % c[:3])
def test_prepared_block_tiles_coefficients_max_and_exceed_equal_the_restatement_to_the_bit(combo):
    p, s_n, s_i, k, intercept = combo
    S = s_n + s_i
    batch, rows = batch_rows(p, S), row_counts(p, S)
    for N in knees(p):
        for V in VERTS:
            Y, mask, W, wmask, D, perm = case(N, V, combo)
            ref_t, t_ref, slope_ref, ref_f, F_ref, coef_ref = reference(N, V, combo)
            pg = D.shape[1]
            for kk, ref, tile_ref, out0_ref in ((0, ref_t, t_ref, slope_ref), (k, ref_f, F_ref, coef_ref)):
                if ref is None:
                    continue
                q_g = pg - (kk if kk else (0 if s_i else 1))
                prep = _prepare_device(Y, mask, W, wmask, D[:, :q_g], s_i, intercept)
                for name in PREPARED:
                    same_bits(getattr(prep, name), ref[name], f"N={N} V={V} k={kk} prepared {name}")
                _check(prep, D, perm, kk, batch, tile_ref, out0_ref, (f"N={N} V={V}", rows))
            if V >= 8:
                planted_cases_occur(N, V, combo)
            clamped = np.array(perm[1])
            clamped[0], clamped[N - 1] = 0, N - 1
            assert np.array_equal(t_ref[1], vref.regression_t(ref_t, D, clamped[None, :], s_n, s_i)[0], equal_nan=True)


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "p%d_sn%d_si%d" % c[:3])
def test_null_masks_give_the_bits_of_masks_of_all_ones(combo):
    p, s_n, s_i, k, intercept = combo
    N, V = 33, 257
    Y, _, W, _, D, perm = case(N, V, combo)
    q_g = D.shape[1] - (0 if s_i else 1)
    ref = vref.prepare(Y, None, W, None, D[:, :q_g] if q_g else None, s_n, centre=intercept)
    t_ref, slope_ref = vref.regression_t(ref, D, perm, s_n, s_i, with_slope=True)
    assert (ref["n"] == N).all() and (ref["n_dropped"] == 0).all() and (ref["m"] == 1).all()
    ones, wones = np.ones((N, V), bool), np.ones(W.shape, bool)
    for mask, wmask, what in ((None, None, "null masks"), (ones, wones, "all ones"), (None, wones, "null mask"), (ones, None, "null wmask")):
        prep = _prepare_device(Y, mask, W, wmask, D[:, :q_g], s_i, intercept)
        for name in PREPARED:
            same_bits(getattr(prep, name), ref[name], f"{what}: prepared {name}")
        _check(prep, D, perm, 0, batch_rows(p, s_n + s_i), t_ref, slope_ref, (what, (len(perm),)))


def test_the_wrappers_refuse_what_the_kernels_would():
    from oai_analysis_2_amd import ops
    combo = COMBOS[3]                                                          # [w | 1, d1, d2]
    Y, mask, W, wmask, D, perm = case(31, 65, combo)
    prep = _prepare_device(Y, mask, W, wmask, D[:, :1], 0, True)               # one global nuisance column: F of the two dummies
    design, index = dev(D), dev(perm)
    for kwargs, words in ((dict(n_interest=0), "n_interest must be 1 .. 4"), (dict(n_interest=5), "n_interest must be 1 .. 4"),
                          (dict(n_interest=1), r"design must be float64 \[31, 2 .. 2\]"), (dict(n_interest=2, p0=3, p1=3), "are not rows"),
                          (dict(n_interest=2, coef0=torch.empty((1, 65), dtype=torch.float64, device="cuda")), r"coef0 must be float64 \[2, 65\]"),
                          (dict(n_interest=2, workspace=torch.empty(16, dtype=torch.uint8, device="cuda")), "workspace")):
        args = dict(p0=0, p1=4)
        args.update(kwargs)
        with pytest.raises((ValueError, RuntimeError), match=words):
            ops.regression_vx_f(prep, design, index, **args)
    with pytest.raises(ValueError, match=r"design must be float64 \[31, 2 .. 2\]"):
        ops.regression_vx_t(prep, design, index, 0, 4)                         # the t of that block tests ONE column after the intercept
    with pytest.raises(ValueError, match="perm must be int32"):
        ops.regression_vx_t(prep, design[:, :2].contiguous(), index[:, :-1], 0, 4)
    as_x = _prepare_device(Y, mask, W, wmask, D[:, :1], 1, True)
    with pytest.raises(ValueError, match="regression_vx_t tests"):
        ops.regression_vx_f(as_x, design, index, 0, 4, 1)
    for kwargs, words in ((dict(vertex_columns=dev(W)[0]), r"vertex_columns must be float32 \[1 .. 2, 31, 65\]"),
                          (dict(vertex_columns=torch.zeros((3, 31, 65), device="cuda")), "vertex_columns must be float32"),
                          (dict(vertex_mask=dev(wmask, np.uint8)[:, :-1]), "vertex_mask must have the shape"),
                          (dict(n_vertex_interest=2), "n_vertex_interest must be 0 or 1"),
                          (dict(nuisance=dev(np.ones((31, 6)))), r"nuisance must be float64 \[31, 1 .. 4\]")):
        args = dict(values=dev(Y), mask=dev(mask, np.uint8), vertex_columns=dev(W), vertex_mask=dev(wmask, np.uint8))
        args.update(kwargs)
        with pytest.raises((ValueError, RuntimeError), match=words):
            ops.regression_vx_prepare(**args)


# ---- the public interface --------------------------------------------------------------------------------------------------------------
T_CLUSTER = 2.5


def _map_cohort(atlas, base, wmask, reverse):
    """The baseline maps as a cohort; ``reverse``: its rows in the opposite order, so that only the ids can match them to the rates."""
    from oai_analysis_2_amd import stats
    cohort = stats.ThicknessCohort(atlas, "FC", chunk=5)
    for i in (range(len(base) - 1, -1, -1) if reverse else range(len(base))):
        cohort.add_vector(base[i], i, wmask[i])
    return cohort


def test_regression_and_f_test_with_a_vertex_covariate_end_to_end_equal_the_restatement_and_remove_the_confound():
    from oai_analysis_2_amd import stats
    rate, mask, base, wmask, group, cap = confound()
    atlas = sphere_atlas()
    index = stats.index_permutations(CONFOUND_N, CONFOUND_P, seed=1).index
    kwargs = dict(n_permutations=CONFOUND_P, seed=1, cluster_threshold=T_CLUSTER, tfce=True)
    cohort = _cohort(atlas, rate, mask=mask, chunk=7)                      # ids 0 .. N - 1 in row order
    res = stats.regression_test(cohort, group, vertex_covariates=_map_cohort(atlas, base, wmask, reverse=True), batch=48, **kwargs)
    # regression_test against the restatement, field by field
    Z, D, scale = rref.design_columns(group, None, True)
    prep = vref.prepare(rate, mask, base[None], wmask[None], Z, 1)
    t, slope = vref.regression_t(prep, D, index, 1, 0, with_slope=True)
    want, max_abs = restated_fields(t, CONFOUND_P, atlas, T_CLUSTER)
    dof = prep["n"].astype(np.int64) - 3
    with np.errstate(invalid="ignore", divide="ignore"):
        partial_r = t[0] / np.sqrt(t[0] * t[0] + dof.astype(np.float64))
    want.update(t=t[0], n=prep["n"], dof=dof, slope=slope / scale, partial_r=partial_r, max_abs=max_abs, n_dropped=prep["n_dropped"])
    same_result(res, want, "regression_test against the restatement", extra=("n_dropped",))
    assert np.array_equal(res.n, (mask & wmask).sum(axis=0)) and np.array_equal(res.n_dropped, (mask & ~wmask).sum(axis=0)) and res.n_dropped.max() > 0
    # the confound demonstration's counts: the unadjusted test finds the cap, the adjusted one finds nothing
    plain = stats.regression_test(cohort, group, n_permutations=CONFOUND_P, seed=1, batch=48)
    assert plain.n_dropped is None
    same_bits(plain.p_fwer, confound_restated(False, index)[1], "unadjusted p_fwer")
    assert int((plain.p_fwer[cap] <= 0.05).sum()) == CONFOUND_UNADJUSTED_CAP and int((res.p_fwer <= 0.05).sum()) == CONFOUND_ADJUSTED
    # the same maps as an [N, V] array with NaN for a missing entry, another batch size, the rows handed over: the same bits in every field
    fields = {f.name: getattr(res, f.name) for f in dataclasses.fields(res)}
    fields["n_dropped"] = res.n_dropped
    as_array = np.where(wmask, base, np.float32(np.nan))
    for other, what in ((stats.regression_test(cohort, group, vertex_covariates=as_array, **kwargs), "an array, default batch"),
                        (stats.regression_test(cohort, group, vertex_covariates=[torch.from_numpy(as_array).cuda()], cluster_threshold=T_CLUSTER,
                                               tfce=True, batch=37, permutations=index), "a tensor in a list, batch 37")):
        same_result(other, fields, what, extra=("n_dropped",))
    # f_test of the same column
    fres = stats.f_test(cohort, group, vertex_covariates=_map_cohort(atlas, base, wmask, reverse=False), batch=48, **kwargs)
    Zf, Df, scales = fref.design_matrix(group, None, True)
    F, coef = vref.regression_f(vref.prepare(rate, mask, base[None], wmask[None], Zf, 1), Df, index, 1, 1, with_coef=True)
    want, max_f = restated_fields(F, CONFOUND_P, atlas, T_CLUSTER)
    with np.errstate(invalid="ignore", divide="ignore"):
        eta2 = F[0] / (F[0] + dof.astype(np.float64))
    want.update(f=F[0], n=prep["n"], dof1=1, dof2=dof, coefficients=coef / scales[:, None], partial_eta2=eta2, max_f=max_f, n_dropped=prep["n_dropped"],
                levels=None, group_n=None, group_mean=None)
    same_result(fres, want, "f_test against the restatement", extra=("n_dropped",))
    assert np.allclose(fres.f, res.t ** 2, rtol=1e-10, atol=0, equal_nan=True) and int((fres.p_fwer <= 0.05).sum()) == 0
    # anova_test takes the argument too: its F is f_test's
    ares = stats.anova_test(cohort, group.astype(np.int64), vertex_covariates=as_array, n_permutations=CONFOUND_P, seed=1, batch=48)
    same_bits(ares.f, fres.f, "anova_test f")
    same_bits(ares.n_dropped, fres.n_dropped, "anova_test n_dropped")
    assert ares.group_n.sum(axis=0).tolist() == mask.sum(axis=0).tolist()      # the descriptive side counts the knees with a value


def test_a_map_as_x_end_to_end_equals_the_restatement():
    from oai_analysis_2_amd import stats
    rate, mask, base, wmask, group, cap = confound()
    atlas = sphere_atlas()
    P = 60
    index = stats.index_permutations(CONFOUND_N, P, seed=2).index
    cohort = _cohort(atlas, rate, mask=mask, chunk=7)
    res = stats.regression_test(cohort, _map_cohort(atlas, base, wmask, reverse=True), covariates=group, n_permutations=P, seed=2, batch=16)
    _, D, _ = fref.design_matrix(group, None, True)                        # [1, group scaled]: every global column is nuisance
    prep = vref.prepare(rate, mask, base[None], wmask[None], D, 0)
    t, slope = vref.regression_t(prep, D, index, 0, 1, with_slope=True)
    max_abs, exceed = gref.reduce_tiles(t)
    same_bits(res.t, t[0], "t")
    same_bits(res.slope, slope, "slope: per unit of the map, not rescaled")
    same_bits(res.max_abs, max_abs, "max_abs")
    same_bits(res.p_fwer, stats._p_values(t[0], max_abs, exceed, P)[1], "p_fwer")
    same_bits(res.n_dropped, prep["n_dropped"], "n_dropped")
    assert np.array_equal(res.dof, prep["n"].astype(np.int64) - 3)
    assert abs(np.nanmedian(res.slope) + 0.05) < 0.02                      # the rate was made as -0.05 mm / year per mm of baseline
    # with a second map beside it as a nuisance column
    smooth = (0.5 * base + 0.5 * np.roll(base, 1, axis=1)).astype(np.float32)
    both = stats.regression_test(cohort, np.where(wmask, base, np.float32(np.nan)), vertex_covariates=smooth, n_permutations=P, seed=2, batch=16)
    Z = np.ones((CONFOUND_N, 1))
    prep2 = vref.prepare(rate, mask, np.stack([smooth, base]), np.stack([np.ones_like(wmask), wmask]), Z, 1)
    same_bits(both.t, vref.regression_t(prep2, Z, index, 1, 1)[0], "t beside a nuisance map")


def test_vertex_covariates_none_is_the_call_without_the_argument():
    from oai_analysis_2_amd import stats
    rate, mask, base, wmask, group, cap = confound()
    atlas = sphere_atlas()
    cohort = _cohort(atlas, rate, mask=mask, chunk=7)
    age = np.random.default_rng(3).uniform(45, 80, CONFOUND_N)
    for call, args in ((stats.regression_test, (group,)), (stats.f_test, (np.stack([group, age ** 2], axis=1),)), (stats.anova_test, (group.astype(np.int64),))):
        kwargs = dict(covariates=age, n_permutations=40, seed=5, batch=16, cluster_threshold=T_CLUSTER, tfce=True)
        a, b = call(cohort, *args, **kwargs), call(cohort, *args, vertex_covariates=None, **kwargs)
        assert a.n_dropped is None and b.n_dropped is None
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, np.ndarray):
                same_bits(y, x, f"{call.__name__}: {f.name}")
            else:
                assert x == y, f.name


def test_first_visit_is_each_subjects_earliest_row():
    from oai_analysis_2_amd import stats
    atlas = sphere_atlas()
    V = len(atlas.inner["FC"].verts)
    rng = np.random.default_rng(9)
    subjects = ["c", "a", "b", "a", "c", "b", "a", "d"]
    years = [2.0, 1.0, 0.5, 0.0, 1.0, 3.0, 4.0, 7.0]
    maps = rng.normal(2.0, 0.3, (len(subjects), V)).astype(np.float32)
    valid = rng.random(maps.shape) >= 0.2
    visits = stats.LongitudinalCohort(atlas, "FC", chunk=3)
    for row, s, y, ok in zip(maps, subjects, years, valid):
        visits.add_vector(row, s, y, valid=ok)
    first = visits.first_visit()
    picked = [4, 3, 2, 7]                                                   # c at 1.0, a at 0.0, b at 0.5, d at 7.0: in order of first appearance
    assert first.ids == ["c", "a", "b", "d"] == visits.subjects == visits.change("rate").ids and first.kind == "FC"
    same_bits(first.mask, valid[picked].astype(np.uint8), "mask")
    same_bits(first.values, np.where(valid[picked], maps[picked], np.float32(0)), "values")
    with pytest.raises(ValueError, match="no visit"):
        stats.LongitudinalCohort(atlas, "FC").first_visit()
