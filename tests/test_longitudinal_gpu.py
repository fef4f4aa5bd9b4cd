"""GPU: the longitudinal line fit (csrc/visit_slopes.hip) against its numpy restatement (tests/visit_slopes_ref.py), to the bit -- every
float64 is the result of IEEE add, multiply, divide and sqrt in a stated order -- and ``LongitudinalCohort`` / ``one_sample_test`` of
oai_analysis_2_amd.stats end to end on a small sphere."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import group_stats_ref as gref
import visit_slopes_ref as vref
from cohort_cases import dev, icosphere, same_bits, sphere_atlas

pytestmark = pytest.mark.gpu


COUNTS = {1: (6,), 5: vref.HOSTILE_COUNTS}


@functools.lru_cache(maxsize=None)
def _case(S, V, with_mask=True):
    case = vref.hostile_case(100 * S + V, V, COUNTS[S], with_mask)
    for a in case:
        if a is not None:
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _want(S, V, with_mask=True, min_visits=2, min_span=0.0):
    return vref.fit(*_case(S, V, with_mask), min_visits=min_visits, min_span=min_span)


def _run(case, **kwargs):
    from oai_analysis_2_amd import ops
    Y, mask, offsets, rows, times, tref = case
    return ops.visit_slopes(dev(Y), dev(offsets), dev(rows), dev(times), dev(tref), mask=dev(mask), **kwargs)


def _check(got, want, where, names=vref.OUTPUTS):
    for name in names:
        same_bits(getattr(got, name), want[name], f"{where} {name}")


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("V", [1, 63, 65, 257])
def test_the_fit_equals_the_restatement_to_the_bit(V, S):
    want = _want(S, V)
    got = _run(_case(S, V))
    _check(got, want, f"S={S} V={V}")
    out = {name: getattr(got, name).cpu().numpy() for name in vref.OUTPUTS}
    assert np.isfinite(out["rate"]).all() and np.abs(out["avg"]).max() <= 4.0 and np.abs(out["fit_ref"]).max() < 100.0     # no garbage
    missing = out["mask"] == 0
    for name in ("rate", "avg", "fit_ref", "resid_sd"):
        assert (out[name][missing] == 0).all() and not np.signbit(out[name][missing]).any(), name
    assert np.array_equal(np.isnan(out["resid_sd"]), (out["mask"] == 1) & (out["n"] == 2))
    if S == 5:
        # the empty run, the single visit and the two visits at one time have no fit anywhere; the 40 visits have one everywhere
        assert (out["n"][0] == 0).all() and (out["n"][1] <= 1).all() and (out["mask"][:3] == 0).all() and out["mask"][3].all()
        assert (out["n"][3] > 8).all()                                     # beyond the slots that the kernel holds in registers
    assert out["n"][-1, 0] == 0 and out["mask"][-1, 0] == 0                # a vertex with no valid visit
    if V >= 2:
        assert out["n"][-1, V - 1] == 1 and out["mask"][-1, V - 1] == 0    # and one with exactly one


def test_without_a_mask_and_with_every_output_null_in_turn():
    S, V = 5, 65
    got = _run(_case(S, V, False))
    _check(got, _want(S, V, False), "no mask")
    assert (got.n.cpu().numpy()[3] == 38).all()                            # 40 slots, one of row -1 and one of row n_rows
    want = _want(S, V)
    for absent in vref.OUTPUTS:
        names = tuple(n for n in vref.OUTPUTS if n != absent)
        got = _run(_case(S, V), want=names)
        assert getattr(got, absent) is None
        _check(got, want, f"without {absent}", names)
    for alone in vref.OUTPUTS:
        _check(_run(_case(S, V), want=(alone,)), want, "alone", (alone,))


def test_min_visits_and_min_span_flip_the_expected_entries():
    S, V = 5, 257
    base = _want(S, V)
    for kwargs in (dict(min_visits=3), dict(min_span=2.5), dict(min_visits=4, min_span=1.0)):
        want = _want(S, V, True, kwargs.get("min_visits", 2), kwargs.get("min_span", 0.0))
        flipped = (base["mask"] == 1) & (want["mask"] == 0)
        assert flipped.any() and not ((base["mask"] == 0) & (want["mask"] == 1)).any(), kwargs
        if "min_span" not in kwargs:
            assert np.array_equal(flipped, (base["mask"] == 1) & (base["n"] < kwargs["min_visits"]))
        _check(_run(_case(S, V), **kwargs), want, str(kwargs))


def test_rows_out_of_range_read_as_missing_and_the_last_offset_is_clamped():
    S, V = 5, 63
    Y, mask, offsets, rows, times, tref = _case(S, V)
    E, R = len(rows), len(Y)
    assert (rows == -1).sum() == 1 and (rows == R).sum() == 1 and offsets[-1] > E
    # the same fit with those two slots' rows in range but masked out entirely, and the last offset at the slot count
    rows2, offsets2, mask2 = rows.copy(), offsets.copy(), np.concatenate([mask, np.zeros((1, V), np.uint8)])
    rows2[(rows == -1) | (rows == R)] = R
    offsets2[-1] = E
    Y2 = np.concatenate([Y, np.full((1, V), np.nan, np.float32)])
    want = vref.fit(Y2, mask2, offsets2, rows2, times, tref)
    _check(_run((Y, mask, offsets, rows, times, tref)), want, "hostile")
    _check(_run((Y2, mask2, offsets2, rows2, times, tref)), want, "tame")
    # offsets below 0, beyond the end and inverted
    wild = np.array([-5, 3, 2, 44, 10 ** 6, 7], np.int32)
    _check(_run((Y, mask, wild, rows, times, tref)), vref.fit(Y, mask, wild, rows, times, tref), "wild offsets")


def test_two_launches_give_identical_bits_and_no_visit_at_all_is_a_count_of_zero():
    from oai_analysis_2_amd import ops
    first, second = _run(_case(5, 257)), _run(_case(5, 257))
    for name in vref.OUTPUTS:
        same_bits(getattr(second, name), getattr(first, name).cpu().numpy(), name)
    Y = torch.ones((2, 3), dtype=torch.float32, device="cuda")
    none = ops.visit_slopes(Y, dev(np.zeros(4, np.int32)), dev(np.zeros(0, np.int32)), dev(np.zeros(0)), dev(np.zeros(3)))
    assert none.n.shape == (3, 3) and not none.n.any() and not none.mask.any() and not none.rate.any()


def test_the_wrapper_refuses_what_the_kernel_would():
    from oai_analysis_2_amd import ops
    Y, mask, offsets, rows, times, tref = (dev(a) for a in _case(1, 63))
    for kwargs, match in ((dict(min_visits=1), "min_visits"), (dict(min_span=-1.0), "min_span"), (dict(min_span=float("nan")), "min_span"),
                          (dict(want=()), "want"), (dict(want=("rate", "slope")), "want"), (dict(mask=mask[:, :5]), "mask must have")):
        with pytest.raises(ValueError, match=match):
            ops.visit_slopes(Y, offsets, rows, times, tref, **kwargs)
    with pytest.raises(ValueError, match="offsets must hold"):
        ops.visit_slopes(Y, offsets, rows, times[:-1], tref)
    with pytest.raises(ValueError, match="offsets must hold"):
        ops.visit_slopes(Y, offsets, rows, times, torch.cat([tref, tref]))
    with pytest.raises(Exception, match="float32"):
        ops.visit_slopes(Y.double(), offsets, rows, times, tref)
    with pytest.raises(Exception, match="float64"):
        ops.visit_slopes(Y, offsets, rows, times.float(), tref)


# ---- the public interface --------------------------------------------------------------------------------------------------------------
N_SUBJECTS, LOSS = 12, 0.08
LABELS = {year: f"V{k:02d}" for k, year in enumerate(vref.OAI_VISIT_YEARS)}


@functools.lru_cache(maxsize=None)
def _study():
    """Twelve subjects on the sphere with baseline, the one-year visit and up to three more: 2.5 mm + 0.05 mm noise, a loss of 0.08 mm a
    year on the cap z > 0.7, 10 % of the entries missing (NaN).  The rows come visit by visit, so a subject's rows are apart.  Returns
    (Y float32 [R, V], subject, nominal years, label, jittered years, cap)."""
    verts, _ = icosphere(2)
    cap = verts[:, 2] > 0.7
    rng = np.random.default_rng(12)
    later = np.array(vref.OAI_VISIT_YEARS[2:])
    visits = [(f"knee{s:02d}", year) for s in range(N_SUBJECTS) for year in [0.0, 1.0] + sorted(rng.choice(later, rng.integers(0, 4), replace=False))]
    visits.sort(key=lambda p: p[1])                                        # stable: visit by visit, subjects in order within one
    subject, nominal = [p[0] for p in visits], np.array([p[1] for p in visits])
    jittered = nominal + rng.uniform(-0.08, 0.08, len(nominal))
    Y = 2.5 + 0.05 * rng.normal(size=(len(visits), len(verts)))
    Y[:, cap] -= LOSS * jittered[:, None]
    Y = Y.astype(np.float32)
    Y[rng.random(Y.shape) < 0.1] = np.nan
    Y.setflags(write=False)
    return Y, subject, nominal, [LABELS[y] for y in nominal], jittered, cap


def _longitudinal(years, **kwargs):
    from oai_analysis_2_amd import stats
    Y, subject, _, label, _, _ = _study()
    cohort = stats.LongitudinalCohort(sphere_atlas(level=2), "FC", chunk=7, **kwargs)
    for row, s, y, lab in zip(Y, subject, years, label):
        cohort.add_vector(np.array(row), s, y, visit=lab)                  # a copy: the cached study is read-only
    return cohort


@functools.lru_cache(maxsize=None)
def _restated(min_visits=2, min_span=0.0):
    from oai_analysis_2_amd import stats
    Y, subject, _, _, jittered, _ = _study()
    table = stats.visit_table(subject, jittered)
    return table, vref.fit(np.nan_to_num(Y), ~np.isnan(Y), table.offsets, table.rows, table.times, table.reference_time, min_visits, min_span)


def test_change_is_the_restatement_rounded_once():
    from oai_analysis_2_amd import stats
    Y, subject, _, _, jittered, cap = _study()
    visits = _longitudinal(jittered)
    table, fitted = _restated()
    assert visits.subjects == table.subjects == [f"knee{s:02d}" for s in range(N_SUBJECTS)] and len(visits) == len(Y)
    assert [len(visits.visits_of(s)) for s in visits.subjects] == np.diff(table.offsets).tolist() and 2 <= np.diff(table.offsets).min()
    assert np.diff(table.offsets).max() == 5 and visits.visits_of("knee00")[0][1] == "V00"
    _check(visits.trajectories(), fitted, "trajectories")
    graph = visits.rows.surface_graph()
    for measure in ("rate", "avg", "pc1", "spc"):
        want, want_m = vref.measure(fitted, measure)
        got = visits.change(measure)
        same_bits(got.mask, want_m, measure + " mask")
        same_bits(got.values, want, measure + " values")
        assert got.ids == table.subjects and got.kind == "FC" and got.atlas is visits.atlas and len(got) == N_SUBJECTS
        assert got.change == stats.Change(measure, 2, 0.0, "first") and got.smoothing is None and got._graph is graph
    with pytest.raises(dataclasses.FrozenInstanceError):
        got.change.measure = "rate"
    # the loss is where it was painted
    rate, rate_m = vref.measure(fitted, "rate")
    assert np.median(rate[:, cap][rate_m[:, cap] != 0]) < -0.5 * LOSS and abs(np.median(rate[:, ~cap][rate_m[:, ~cap] != 0])) < 0.2 * LOSS
    # stricter settings and another reference time
    _, strict = _restated(3, 2.5)
    got = visits.change("rate", min_visits=3, min_span_years=2.5)
    same_bits(got.mask, vref.measure(strict, "rate")[1], "strict mask")
    same_bits(got.values, vref.measure(strict, "rate")[0], "strict values")
    assert got.change == stats.Change("rate", 3, 2.5, "first") and strict["mask"].sum() < fitted["mask"].sum()
    table4 = stats.visit_table(subject, jittered, reference=4.0)
    at4 = vref.fit(np.nan_to_num(Y), ~np.isnan(Y), table4.offsets, table4.rows, table4.times, table4.reference_time)
    got = visits.change("pc1", reference=4.0)
    same_bits(got.values, vref.measure(at4, "pc1")[0], "pc1 at four years")
    assert got.change.reference == 4.0 and visits.change("pc1", reference={s: 4.0 for s in table.subjects}).change.reference == "per subject"
    with pytest.raises(ValueError, match="measure must be"):
        visits.change("slope")
    with pytest.raises(ValueError, match="already has a visit"):
        visits.add_vector(np.array(Y[0]), subject[0], jittered[0])
    assert len(visits) == len(Y) == len(visits.rows)                       # a refused row leaves nothing behind


def test_from_cohorts_per_row_add_and_at_visit():
    from oai_analysis_2_amd import stats
    Y, subject, nominal, label, _, _ = _study()
    atlas = sphere_atlas(level=2)
    by_row = _longitudinal(nominal)
    per_visit = {}
    for year in sorted(set(nominal.tolist())):
        per_visit[year] = stats.ThicknessCohort(atlas, "FC", chunk=5)
        for i in np.nonzero(nominal == year)[0]:
            per_visit[year].add_vector(np.array(Y[i]), subject[i])
    joined = stats.LongitudinalCohort.from_cohorts(per_visit)
    assert joined.subjects == by_row.subjects and joined.rows.ids == by_row.rows.ids == list(zip(subject, nominal.tolist()))
    assert torch.equal(joined.rows.values, by_row.rows.values) and torch.equal(joined.rows.mask, by_row.rows.mask)
    same_bits(joined.change("rate").values, by_row.change("rate").values.cpu().numpy(), "rate of the joined cohorts")
    # one visit as a cohort: by label and by years, rows matched by subject
    for key in ("V04", 2.5):
        picked = np.nonzero(nominal == 2.5)[0]
        assert 0 < len(picked) < N_SUBJECTS
        visit = by_row.at_visit(key)
        assert visit.ids == [subject[i] for i in picked] and isinstance(visit, stats.ThicknessCohort)
        same_bits(visit.values, np.nan_to_num(Y[picked]), f"at_visit({key!r})")
        same_bits(visit.mask, (~np.isnan(Y[picked])).astype(np.uint8), f"at_visit({key!r}) mask")
    assert joined.at_visit(1.0).ids == by_row.subjects                     # no labels there: by years
    with pytest.raises(ValueError, match="no row"):
        by_row.at_visit("V99")
    # follow-up against baseline through the existing paired test; the follow-up handed over in another order
    base, follow = by_row.at_visit("V00"), by_row.at_visit("V01")
    order = np.random.default_rng(5).permutation(N_SUBJECTS)
    shuffled = stats.ThicknessCohort(atlas, "FC")
    for i in order:
        shuffled.add_vector(follow.values[i], follow.ids[i], follow.mask[i])
    res, res_shuffled = (stats.paired_test(f, base, n_permutations=64, seed=2) for f in (follow, shuffled))
    assert subject[:2 * N_SUBJECTS] == 2 * by_row.subjects                 # the baseline rows come first, then the one-year rows
    diff = Y[N_SUBJECTS:2 * N_SUBJECTS] - Y[:N_SUBJECTS]
    assert np.array_equal(res.n1, (~np.isnan(diff)).sum(axis=0)) and np.array_equal(res_shuffled.n1, res.n1)
    assert np.allclose(res.mean_difference, np.nanmean(diff.astype(np.float64), axis=0), rtol=1e-12, atol=1e-15)


def test_one_sample_test_is_the_paired_test_against_zeros_and_the_restatement():
    from oai_analysis_2_amd import stats
    _, _, _, _, jittered, cap = _study()
    rate = _longitudinal(jittered).change("rate")
    zeros = stats.ThicknessCohort(rate.atlas, "FC")
    for s in rate.ids:
        zeros.add_vector(np.zeros(rate.n_verts, np.float32), s)
    kwargs = dict(n_permutations=5000, cluster_threshold=3.0, tfce=stats.TFCE(extent="vertices"))
    res, paired = stats.one_sample_test(rate, **kwargs), stats.paired_test(rate, zeros, **kwargs)
    assert res.exact and res.n_permutations == 1 << N_SUBJECTS             # all 2^12 sign vectors, each once
    for f in dataclasses.fields(res):
        a, b = getattr(res, f.name), getattr(paired, f.name)
        if isinstance(a, np.ndarray):
            same_bits(a, b, f.name)
        else:
            assert a == b, f.name
    # against the restatement of the t on the restated rates
    _, fitted = _restated()
    want, want_m = vref.measure(fitted, "rate")
    flips = stats.sign_flips(N_SUBJECTS, 5000)
    t_ref = gref.permutation_t(gref.prepare(want, want_m, centre=False), want_m, flips.rows(), gref.ONE_SAMPLE)
    max_abs, exceed = gref.reduce_tiles(t_ref)
    same_bits(res.t, t_ref[0], "t")
    same_bits(res.max_abs, max_abs, "max_abs")
    valid = ~np.isnan(t_ref[0])
    p_fwer = np.where(valid, (max_abs[None, :] >= np.abs(np.where(valid, t_ref[0], 0.0))[:, None]).sum(axis=1) / float(len(flips)), np.nan)
    same_bits(res.p_fwer, p_fwer, "p_fwer")
    assert np.array_equal(np.rint(res.p_uncorrected[valid] * len(flips)).astype(np.int64), exceed[valid])
    assert np.array_equal(res.n1, want_m.sum(axis=0).astype(np.int32)) and (res.mean_difference[cap] < -0.5 * LOSS).all()
    assert (res.t[cap] < 0).all() and np.nanmedian(res.p_fwer[cap]) < 0.05 < np.nanmedian(res.p_fwer[~cap])
    with pytest.raises(ValueError, match="at least two"):
        stats.one_sample_test(stats.ThicknessCohort(rate.atlas, "FC"))


def test_the_other_tests_take_the_rate_cohort_unchanged():
    from oai_analysis_2_amd import stats
    _, _, _, _, jittered, _ = _study()
    visits = _longitudinal(jittered)
    rate = visits.change("rate")
    _, fitted = _restated()
    want, want_m = vref.measure(fitted, "rate")
    groups = np.arange(N_SUBJECTS) % 2 == 0
    res = stats.two_sample_test(rate, groups, n_permutations=50, seed=4)
    t_ref = gref.permutation_t(gref.prepare(want, want_m), want_m, stats.label_permutations(groups, 50, seed=4).rows(), gref.TWO_SAMPLE)
    same_bits(res.t, t_ref[0], "two-sample t of the rates")
    reg = stats.regression_test(rate, np.linspace(45.0, 79.0, N_SUBJECTS), n_permutations=50, seed=4)
    assert reg.t.shape == (rate.n_verts,) and np.isfinite(reg.t[want_m.sum(axis=0) >= 4]).all()
    # smoothing before the fit and after it: both run, both keep their settings, and they differ where entries are missing
    before = visits.smoothed(sweeps=2).change("rate")
    after = rate.smoothed(sweeps=2)
    assert before.smoothing.sweeps == after.smoothing.sweeps == 2 and before.change == after.change == rate.change
    assert before.ids == after.ids == rate.ids and not torch.equal(before.values, after.values)
