"""CPU: the numpy restatement of the normative deviation (tests/normative_ref.py; include/oai_hip.h, "Normative deviation") against
independent refits -- every knee scored against ``np.linalg.lstsq`` on the knees actually used, which for loo = 1 means a fit WITHOUT
the knee -- its ties to known quantities, and the host side of ``stats.NormativeModel``: design, p-value ranks, refusals and the file.

The gate of the refits is 1e-10 on |z - z_refit| / max(1, |z_refit|), the gate the regression tests use.  Measured on the inputs below
(N = 24, V = 65, p = 3 with the covariates centred, mask density 0.8): 8.5e-14 with the mask and 2.3e-14 without for loo = 1, 5.1e-14 and
5.5e-15 for loo = 0 (profiles/normative.md)."""
import numpy as np
import pytest
from scipy import stats as scipy_stats

import normative_ref as nref

N, V, P = 24, 65, 3
GATE = 1e-10


def _plain(with_mask):
    rng = np.random.default_rng(2024)
    age = rng.normal(60.0, 9.0, N)
    sex = (np.arange(N) % 2).astype(np.float64)
    Z = np.stack([np.ones(N), age - age.mean(), sex - sex.mean()], axis=1)
    Y = (2.4 + 0.3 * rng.normal(size=(N, V))).astype(np.float32)
    mask = (rng.random((N, V)) < 0.8).astype(np.uint8) if with_mask else None
    return Y, mask, Z


def _refit_z(Y, mask, Z, loo):
    """z of every (knee, vertex) from scratch: lstsq on the knees used, the textbook prediction-interval t of the knee against it."""
    y = Y.astype(np.float64)
    m = np.ones(Y.shape, bool) if mask is None else mask != 0
    out = np.full(Y.shape, np.nan)
    for v in range(Y.shape[1]):
        for k in range(Y.shape[0]):
            if not m[k, v]:
                continue
            used = m[:, v].copy()
            if loo:
                used[k] = False
            A, b = Z[used], y[used, v]
            gamma = np.linalg.lstsq(A, b, rcond=None)[0]
            r = b - A @ gamma
            dof = used.sum() - Z.shape[1]
            s2 = (r @ r) / dof
            lev = Z[k] @ np.linalg.solve(A.T @ A, Z[k])
            out[k, v] = (y[k, v] - Z[k] @ gamma) / np.sqrt(s2 * (1.0 + lev))
    return out


@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("loo", [0, 1])
def test_the_restatement_equals_independent_refits(loo, with_mask):
    Y, mask, Z = _plain(with_mask)
    model = nref.fit(Y, mask, Z)
    z, diff = nref.score(model, Y, mask, Z, loo)
    want = _refit_z(Y, mask, Z, loo)
    valid = np.ones(Y.shape, bool) if mask is None else mask != 0
    assert np.isfinite(z[valid]).all() and np.isnan(z[~valid]).all() and np.isfinite(diff[valid]).all()     # finite wherever the mask is set
    err = np.abs(z[valid] - want[valid]) / np.maximum(1.0, np.abs(want[valid]))
    print(f"loo={loo} mask={with_mask}: max |z - z_refit| / max(1, |z_refit|) = {err.max():.3e}")
    assert err.max() <= GATE
    assert model["ok"].all() and np.array_equal(model["n"], valid.sum(axis=0))
    # the coefficients and the residual sum of squares are the refit's too
    for v in (0, V - 1):
        used = valid[:, v]
        gamma = np.linalg.lstsq(Z[used], Y[used, v].astype(np.float64), rcond=None)[0]
        assert np.allclose(model["gamma"][:, v], gamma, rtol=1e-10, atol=1e-12)
        r = Y[used, v].astype(np.float64) - Z[used] @ gamma
        assert np.isclose(model["rss"][v], r @ r, rtol=1e-10)


def test_a_null_mask_gives_the_bits_of_a_mask_of_ones():
    Y, _, Z = _plain(False)
    a, b = nref.fit(Y, None, Z), nref.fit(Y, np.ones(Y.shape, np.uint8), Z)
    for name in ("gamma", "L", "rss", "n", "ok"):
        assert np.array_equal(a[name], b[name]), name
    for loo in (0, 1):
        za, zb = nref.score(a, Y, None, Z, loo)[0], nref.score(b, Y, np.ones(Y.shape, np.uint8), Z, loo)[0]
        assert np.array_equal(za, zb)


def test_with_the_intercept_alone_loo_is_the_one_sample_t_of_the_others():
    Y, _, _ = _plain(False)
    Z = np.ones((N, 1))
    z = nref.score(nref.fit(Y, None, Z), Y, None, Z, 1)[0]
    y = Y.astype(np.float64)
    for k in (0, 7, N - 1):
        others = np.delete(y, k, axis=0)
        # (y_k - mean_-k) / (sd_-k sqrt(1 + 1 / (N - 1)))
        want = (y[k] - others.mean(axis=0)) / (others.std(axis=0, ddof=1) * np.sqrt(1.0 + 1.0 / (N - 1)))
        assert np.allclose(z[k], want, rtol=1e-10, atol=1e-12)
        # scipy's one-sample t of the others against the value, rearranged: t = (mean_-k - y_k) / (sd_-k / sqrt(N - 1))
        t = scipy_stats.ttest_1samp(others, y[k], axis=0).statistic
        assert np.allclose(z[k], -t / np.sqrt(N - 1.0) / np.sqrt(1.0 + 1.0 / (N - 1)), rtol=1e-10, atol=1e-12)


def test_the_hostile_case_holds_every_reason_for_a_nan():
    for p in (1, 3, 6):
        for n in (p + 2, 24):
            Y, mask, Z = nref.hostile_case(5, 65, n, p)
            found = nref.nan_classes(Y, mask, Z)
            assert found["nothing"] >= 1 and found["loo_dof"] >= 1 and found["s2"] >= 1 and found["pivot"] >= 1, (p, n, found)
            assert p == 1 or (found["den"] >= 1 and found["pivot_alone"] >= 1), (p, n, found)


def test_the_summary_of_a_tile():
    tile = np.array([[0.5, -3.0, np.nan, 3.0, 2.5, -2.0], [np.nan] * 6, [0.0, 0.0, np.nan, -0.0, 0.0, 0.0]])
    w = np.array([1, 10, 100, 1000, 10000, 100000], np.int64)
    stats, counts = nref.summary(tile, 2.0, w)
    assert stats[0].tolist() == [3.0, -3.0, 3.0] and counts[0].tolist() == [5, 1, 1, 10, 2, 11000]      # the tie of |z| = 3 goes to vertex 1
    assert stats[1][0] == 0.0 and np.isnan(stats[1][1:]).all() and counts[1].tolist() == [0, -1, 0, 0, 0, 0]
    assert stats[2][0] == 0.0 and counts[2].tolist() == [5, 0, 0, 0, 0, 0]


def test_p_value_ranks():
    from oai_analysis_2_amd import stats
    ref = np.array([1.0, 4.0, 2.0, 2.0, 8.0])
    # a new knee: against all five
    assert stats._rank_p(np.array([9.0, 8.0, 2.0, 0.5]), ref, False).tolist() == [1 / 6, 2 / 6, 5 / 6, 1.0]
    # a member: itself left out, N' = 4
    assert stats._rank_p(ref, ref, True).tolist() == [1.0, 2 / 5, 4 / 5, 4 / 5, 1 / 5]
    for member in (False, True):
        assert np.array_equal(stats._rank_p(ref, ref, member), nref.rank_p(ref, ref, member))
    assert stats._rank_p(np.array([3], np.int64), np.array([1, 3, 5], np.int64), False).tolist() == [3 / 4]


def test_the_design_is_centred_on_the_reference_and_refuses_by_name():
    from oai_analysis_2_amd import stats
    rng = np.random.default_rng(3)
    age, bmi = rng.normal(60, 9, N), rng.normal(28, 4, N)
    cov = np.stack([age, bmi], axis=1)
    design, means, scales, names = stats._normative_design(cov, True, N, ["age", "bmi"])
    assert design.shape == (N, 3) and (design[:, 0] == 1).all() and names == ["age", "bmi"]
    assert np.allclose(means, cov.mean(axis=0), rtol=1e-15) and np.allclose((design[:, 1:] ** 2).sum(axis=0), 1.0)
    assert np.allclose(design[:, 1:].sum(axis=0), 0.0, atol=1e-12)
    assert np.array_equal(stats._design_rows(cov[:5], True, means, scales), design[:5])          # a new knee is treated as the reference was
    only, m0, s0, n0 = stats._normative_design(None, True, N)
    assert only.shape == (N, 1) and (only == 1).all() and len(m0) == len(s0) == len(n0) == 0
    flat, m1, _, _ = stats._normative_design(cov, False, N)
    assert flat.shape == (N, 2) and (m1 == 0).all()
    with pytest.raises(ValueError, match="needs the intercept"):
        stats._normative_design(None, False, N)
    bad = cov.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="bmi holds a NaN"):
        stats._normative_design(bad, True, N, ["age", "bmi"])
    with pytest.raises(ValueError, match="age is constant"):
        stats._normative_design(np.stack([np.full(N, 60.0), bmi], axis=1), True, N, ["age", "bmi"])
    with pytest.raises(ValueError, match="twice is a combination"):
        stats._normative_design(np.stack([age, bmi, 2 * age - bmi], axis=1), True, N, ["age", "bmi", "twice"])
    with pytest.raises(ValueError, match="at most 6"):
        stats._normative_design(rng.normal(size=(N, 6)), True, N)
    with pytest.raises(ValueError, match="covariates must be"):
        stats._normative_design(cov[:-1], True, N)
    with pytest.raises(ValueError, match="one entry per covariate"):
        stats._normative_design(cov, True, N, ["age"])


def test_the_model_file_round_trip(tmp_path):
    from oai_analysis_2_amd import stats
    Y, mask, Z = _plain(True)
    fitted = nref.fit(Y, mask, Z)
    state = {name: fitted[name] for name in ("gamma", "L", "rss", "n", "ok")}
    state.update(means=np.array([60.5, 0.5]), scales=np.array([40.0, 2.4]), names=np.asarray(["age", "sex"], dtype=np.str_), intercept=np.asarray(True),
                 kind=np.asarray("FC"), n_knees=np.asarray(N, np.int64), ref_z_threshold=np.array([2.0, 2.5]),
                 ref_max_abs=np.random.default_rng(1).random((2, N)), ref_max_extent=np.arange(2 * N, dtype=np.int32).reshape(2, N),
                 ref_area_below=np.arange(2 * N, dtype=np.int64).reshape(2, N) << 20)
    path = tmp_path / "model.npz"
    stats.NormativeModel.write_state(path, state)
    back = stats.NormativeModel.read_state(path)
    assert set(back) == set(state)
    for name, want in state.items():
        assert back[name].dtype == np.asarray(want).dtype and np.array_equal(back[name], want), name
    assert str(back["kind"]) == "FC" and bool(back["intercept"]) and [str(n) for n in back["names"]] == ["age", "sex"]
