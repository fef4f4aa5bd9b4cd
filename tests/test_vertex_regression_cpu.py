"""CPU: the numpy restatement of the vertex-wise design columns (tests/vertex_regression_ref.py; include/oai_hip.h, "Vertex-wise design
columns") against independent code -- numpy's least squares on the complete cases for the identity row, an explicitly dealt design for
the permuted rows, the existing restatements where the map is the same number at every vertex -- and the host side of
oai_analysis_2_amd.stats: the refusals that need no device.  The gate is rtol 1e-10 (atol 1e-12 for values near zero), that of
test_group_regression_cpu.py and test_group_f_cpu.py; the measured distances are printed (``-s``) and recorded in
profiles/vertex_covariates.md.  The fixtures are those of tests/test_vertex_regression_gpu.py (tests/vertex_regression_cases.py), and the
corner cases they plant are asserted on the restatement here, so that the bit comparison on the device cannot pass vacuously."""
from types import SimpleNamespace

import numpy as np
import pytest

import group_f_ref as fref
import group_regression_ref as rref
import vertex_regression_ref as vref
from vertex_regression_cases import (COMBOS, CONFOUND_ADJUSTED, CONFOUND_N, CONFOUND_P, CONFOUND_UNADJUSTED_CAP, PLANTED, case, confound, confound_restated,
                                     knees, planted_cases_occur, reference)

RTOL, ATOL = 1e-10, 1e-12


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "p%d_sn%d_si%d" % c[:3])
def test_every_planted_corner_occurs_on_the_restatement(combo):
    for N in knees(combo[0]):
        planted_cases_occur(N, 65, combo)


# ---- against least squares -------------------------------------------------------------------------------------------------------------
def _gap(got, want):
    """The largest distance in units of the gate, over entries where both exist; NaN positions must agree."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ"
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / (ATOL + RTOL * np.abs(want[ok])), initial=0.0)) * RTOL


def _completed(W, wmask, m):
    """Independent of the restatement: a valid entry as it is, a missing one on the mean over the complete cases (uncentred: with an
    intercept in the model, centring changes no statistic)."""
    w = W.astype(np.float64)
    out = np.empty_like(w)
    for s in range(len(w)):
        for v in range(w.shape[2]):
            cc = m[:, v]
            out[s, :, v] = np.where(wmask[s, :, v], w[s, :, v], w[s, cc, v].mean() if cc.any() else 0.0)
    return out


def _fit(X, y, k):
    """(t of the last column, F of the last k, their coefficients, dof) by numpy's least squares; NaN where there is no fit."""
    n, p = X.shape
    norm = np.sqrt((X * X).sum(axis=0))
    if n - p < 1 or not (norm > 0).all() or np.linalg.matrix_rank(X / norm[None, :], tol=1e-5) < p:
        return np.nan, np.nan, np.full(k, np.nan), n - p
    beta = np.linalg.lstsq(X, y, rcond=None)[0]
    rss = float(((y - X @ beta) ** 2).sum())
    s2 = rss / (n - p)
    if not s2 > 1e-20:
        return np.nan, np.nan, np.full(k, np.nan), n - p
    t = beta[-1] / np.sqrt(s2 * np.linalg.inv(X.T @ X)[-1, -1])
    q = p - k
    rss0 = float((y ** 2).sum()) if q == 0 else float(((y - X[:, :q] @ np.linalg.lstsq(X[:, :q], y, rcond=None)[0]) ** 2).sum())
    return t, ((rss0 - rss) / k) / s2, beta[q:], n - p


def _dealt(wfull, D, s_n, s_i, idx, v):
    """The design at vertex v whose knee j holds the whole design row idx[j]."""
    S = s_n + s_i
    return np.concatenate([wfull[:s_n, idx, v].T, D[idx], wfull[S - s_i:S, idx, v].T], axis=1)


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "p%d_sn%d_si%d" % c[:3])
def test_rows_equal_least_squares_on_the_dealt_design(combo):
    """Row 0: the complete-case fit with the design built from the raw maps (t, F, slope, coef, n, dof).  Permuted rows: y residualised on
    the nuisance columns by least squares, then refitted on the explicitly dealt design, completed values included (t, F)."""
    p, s_n, s_i, k, intercept = combo
    N, V = 31, 65
    Y, mask, W, wmask, D, perm = case(N, V, combo)
    prep, t, slope, prep_f, F, coef = reference(N, V, combo)
    m = mask & wmask.all(axis=0)
    wfull, y = _completed(W, wmask, m), Y.astype(np.float64)
    idx = np.clip(perm.astype(np.int64), 0, N - 1)
    kk = max(k, 1)
    rows = range(min(len(perm), 6))
    want_t, want_F = np.full((len(rows), V), np.nan), np.full((len(rows), V), np.nan)
    want_slope, want_coef, want_dof = np.full(V, np.nan), np.full((kk, V), np.nan), np.zeros(V, np.int64)
    for v in range(V):
        cc = np.nonzero(m[:, v])[0]
        X0 = _dealt(wfull, D, s_n, s_i, np.arange(N), v)
        for kind, q in (("t", p - 1), ("f", p - kk)):
            if kind == "f" and not k:
                continue
            Zc = X0[cc, :q]
            r = y[cc, v] - (Zc @ np.linalg.lstsq(Zc, y[cc, v], rcond=None)[0] if q and len(cc) else 0.0)
            for row in rows:
                Xp = _dealt(wfull, D, s_n, s_i, idx[row], v)[cc]
                # Freedman-Lane refits the residuals; on the identity row that is the fit of y itself, which is what is asked there
                tt, ff, beta, dof = _fit(Xp, y[cc, v] if row == 0 else r, 1 if kind == "t" else kk)
                if kind == "t":
                    want_t[row, v] = tt
                    if row == 0:
                        want_slope[v], want_dof[v] = beta[-1], dof
                else:
                    want_F[row, v] = ff
                    if row == 0:
                        want_coef[:, v] = beta
    known = [PLANTED[name] for name in ("constant_y",)]                  # no residual variance: the reference fit has rounding noise there
    keep = np.setdiff1d(np.arange(V), known)
    assert np.array_equal(prep["n"].astype(np.int64) - p, want_dof) and np.array_equal(prep["n"], m.sum(axis=0))
    gaps = {"t": _gap(t[:len(rows)][:, keep], want_t[:, keep]), "slope": _gap(slope[keep], want_slope[keep])}
    if k:
        gaps.update(F=_gap(F[:len(rows)][:, keep], want_F[:, keep]), coef=_gap(coef[:, keep], want_coef[:, keep]))
    print(f"(p, s_n, s_i) = {combo[:3]}: largest relative distance from least squares " + ", ".join(f"{a} {b:.2e}" for a, b in gaps.items()))
    assert all(g <= RTOL for g in gaps.values()), gaps


@pytest.mark.parametrize("as_x", [False, True], ids=["nuisance", "as_x"])
def test_a_map_that_is_one_number_per_knee_gives_the_t_of_the_existing_restatement(as_x):
    N, V, P = 33, 40, 12
    rng = np.random.default_rng([7, int(as_x)])
    c, x, cov = rng.normal(2.5, 0.4, N).astype(np.float32), rng.normal(size=N), 60 + 8 * rng.normal(size=N)
    Y = (2.0 + 0.5 * rng.normal(size=(N, V)) + 0.2 * x[:, None]).astype(np.float32)
    perm = np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(P - 1)])
    W = np.broadcast_to(c[None, :, None], (1, N, V))
    if as_x:                                                              # [1, cov | map] against [1, cov, c]
        Dg = np.stack([np.ones(N), cov], axis=1)
        got = vref.regression_t(vref.prepare(Y, None, W, None, Dg, 0), Dg, perm, 0, 1)
        full = np.concatenate([Dg, c.astype(np.float64)[:, None]], axis=1)
    else:                                                                 # [map | 1, x] against [1, c, x]
        Dg = np.stack([np.ones(N), x], axis=1)
        got = vref.regression_t(vref.prepare(Y, None, W, None, Dg[:, :1], 1), Dg, perm, 1, 0)
        full = np.stack([np.ones(N), c.astype(np.float64), x], axis=1)
    want = rref.regression_t(rref.prepare(Y, None, full[:, :-1]), None, full, perm)
    gap = _gap(got, want)
    print(f"a map constant over the vertices ({'x' if as_x else 'nuisance'}): largest relative distance from the global column's t {gap:.2e}")
    assert not np.isnan(want).any() and gap <= RTOL


@pytest.mark.parametrize("combo", [c for c in COMBOS if c[3]], ids=lambda c: "p%d_sn%d_si%d" % c[:3])
def test_one_tested_column_is_the_square_of_t(combo):
    p, s_n, s_i, _, intercept = combo
    N, V = 31, 65
    Y, mask, W, wmask, D, perm = case(N, V, combo)
    prep, t = reference(N, V, combo)[:2]
    F = vref.regression_f(prep, D, perm, s_n, 1)                          # the prepared block of t has the q of k = 1
    gap = _gap(F, t * t)
    print(f"(p, s_n, s_i) = {combo[:3]}, k = 1: largest relative distance of F from t * t {gap:.2e}")
    assert gap <= RTOL


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "p%d_sn%d_si%d" % c[:3])
def test_under_the_identity_no_completed_value_reaches_a_sum(combo):
    """Poisoned missing entries of w change no bit of anything; other (finite) completed values change no bit of the identity row."""
    p, s_n, s_i, k, intercept = combo
    N, V = 31, 65
    Y, mask, W, wmask, D, perm = case(N, V, combo)
    prep, t, slope = reference(N, V, combo)[:3]
    q_t = D.shape[1] - (0 if s_i else 1)
    poisoned = vref.prepare(Y, mask, np.where(wmask, W, np.float32(np.nan)), wmask, D[:, :q_t] if q_t else None, s_n, centre=intercept)
    for name, want in prep.items():
        assert np.array_equal(poisoned[name], want, equal_nan=True), name
    other = dict(prep)
    other["WC"] = np.where(wmask, prep["WC"], 1e30)
    t0, slope0 = vref.regression_t(other, D, perm[:1], s_n, s_i, with_slope=True)
    assert np.array_equal(t0, t[:1], equal_nan=True) and np.array_equal(slope0, slope, equal_nan=True)
    assert not np.array_equal(vref.regression_t(other, D, perm[:4], s_n, s_i), t[:4], equal_nan=True)      # the null rows do read them


def test_baseline_at_the_vertex_removes_a_group_effect_that_is_regression_to_the_mean():
    from oai_analysis_2_amd import stats
    cap = confound()[-1]
    index = stats.index_permutations(CONFOUND_N, CONFOUND_P, seed=1).index
    (_, plain), (_, adjusted) = confound_restated(False, index), confound_restated(True, index)
    found = int((plain[cap] <= 0.05).sum())
    print(f"unadjusted: {found} of {int(cap.sum())} cap vertices with p_fwer <= 0.05 ({int((plain[~cap] <= 0.05).sum())} outside); adjusted for baseline "
          f"at the vertex: {int((adjusted <= 0.05).sum())} anywhere, smallest p_fwer {np.nanmin(adjusted):.3f}")
    assert found == CONFOUND_UNADJUSTED_CAP and found > 0 and int((adjusted <= 0.05).sum()) == CONFOUND_ADJUSTED == 0


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def _cpu_cohort(N, V, kind="FC", ids=None, device="cpu"):
    """A cohort that lives on the host (its rows are set directly: ``add_vector`` uploads): enough for everything that is refused before
    a launch."""
    import torch
    from oai_analysis_2_amd import stats
    atlas = SimpleNamespace(inner={kind: SimpleNamespace(verts=np.zeros((V, 3), np.float32))}, device=device, image=None)
    cohort = stats.ThicknessCohort(atlas, kind)
    cohort._values = torch.from_numpy(np.random.default_rng(5).normal(2.0, 0.3, (N, V)).astype(np.float32)).to(device)
    cohort._mask = torch.ones((N, V), dtype=torch.uint8, device=device)
    cohort.ids = list(range(N)) if ids is None else list(ids)
    return cohort


def test_the_wrappers_refuse_before_any_launch():
    from oai_analysis_2_amd import stats
    N, V = 10, 12
    cohort, rng = _cpu_cohort(N, V), np.random.default_rng(0)
    x, cov, maps = rng.normal(size=N), rng.normal(size=(N, 3)), rng.normal(size=(3, N, V)).astype(np.float32)
    for kwargs, words in (
            (dict(x=x, vertex_covariates=_cpu_cohort(N, V, ids=list(range(1, N + 1)))), "vertex_covariates needs the same ids"),
            (dict(x=x, vertex_covariates=_cpu_cohort(N, V, ids=[0] * N)), "vertex_covariates needs the same ids"),
            (dict(x=x, vertex_covariates=_cpu_cohort(N - 1, V)), "vertex_covariates needs the same ids"),
            (dict(x=x, vertex_covariates=_cpu_cohort(N, V, kind="TC")), "vertex_covariates must hold the same cartilage of the same atlas"),
            (dict(x=x, vertex_covariates=_cpu_cohort(N, V + 1)), "vertex_covariates must hold the same cartilage of the same atlas"),
            (dict(x=x, vertex_covariates=_cpu_cohort(0, V, device="meta")), "vertex_covariates must hold .* on the same GPU"),
            (dict(x=x, vertex_covariates=[maps[0], _cpu_cohort(N, V, kind="TC")]), r"vertex_covariates\[1\] must hold the same cartilage"),
            (dict(x=x, vertex_covariates=maps[0][:, :-1]), r"vertex_covariates must be a ThicknessCohort or \[10, 12\]"),
            (dict(x=x, vertex_covariates=list(maps)), "vertex_covariates: at most 2 per-vertex columns"),
            (dict(x=maps[0], vertex_covariates=[maps[1], maps[2]]), "vertex_covariates: at most 2 per-vertex columns"),
            (dict(x=maps[0][:, :-1]), r"x must be a ThicknessCohort or \[10, 12\]"),
            (dict(x=x, covariates=cov, vertex_covariates=[maps[0], maps[1]]), "7 columns.*vertex_covariates.*at most 6"),
            (dict(x=maps[0], covariates=np.concatenate([cov, cov[:, :1] ** 2], axis=1), vertex_covariates=maps[1]), "7 columns.*at most 6"),
            (dict(x=np.full(N, 3.0), vertex_covariates=maps[0]), "x is constant"),
            (dict(x=x, vertex_covariates=maps[0], permutations=np.stack([np.arange(N)[::-1], np.arange(N)])), "row 0")):
        with pytest.raises(ValueError, match=words):
            stats.regression_test(cohort, **kwargs)
    X = rng.normal(size=(N, 2))
    for call, kwargs, words in (
            (stats.f_test, dict(X=_cpu_cohort(N, V)), r"a map .* is tested with regression_test\(cohort, x=map\)"),
            (stats.f_test, dict(X=maps[0]), r"a map .* is tested with regression_test\(cohort, x=map\)"),
            (stats.anova_test, dict(groups=maps[0]), r"a map .* is tested with regression_test\(cohort, x=map\)"),
            (stats.anova_test, dict(groups=_cpu_cohort(N, V)), r"a map .* is tested with regression_test\(cohort, x=map\)"),
            (stats.f_test, dict(X=X, vertex_covariates=list(maps)), "vertex_covariates: at most 2 per-vertex columns"),
            (stats.f_test, dict(X=X, covariates=cov[:, :2], vertex_covariates=[maps[0], maps[1]]), "7 columns.*at most 6"),
            (stats.f_test, dict(X=X, vertex_covariates=_cpu_cohort(N, V, kind="TC")), "vertex_covariates must hold the same cartilage"),
            (stats.anova_test, dict(groups=np.arange(N) % 5, covariates=cov[:, 0], vertex_covariates=maps[0]), "7 columns.*at most 6"),
            (stats.anova_test, dict(groups=np.arange(N) % 2, vertex_covariates=_cpu_cohort(N, V, ids=list("abcdefghij"))), "needs the same ids")):
        with pytest.raises(ValueError, match=words):
            call(cohort, **kwargs)


def test_results_carry_n_dropped_as_none_unless_a_map_is_used():
    import dataclasses
    from oai_analysis_2_amd import stats
    for cls in (stats.RegressionResult, stats.FResult):
        assert cls.n_dropped is None and "n_dropped" not in [f.name for f in dataclasses.fields(cls)]
