"""CPU: the numpy restatement of the cohort PCA (tests/cohort_pca_ref.py, which the device must equal to the bit) against independent
implementations -- np.linalg.svd of an independently whitened matrix and sklearn.decomposition.PCA -- and the rules of the contract that
need no GPU: the symmetry of G, the component-drop rule, the sign rule, min_valid, and the save / load round trip of stats.ThicknessPCA.

The gate is GATE = 1e-10, the house gate for library comparisons.  Measured with this file on these shapes (N, V) = (40, 1100) and
(130, 1025), with and without 5-10 % missing entries, random positive weights (the largest over the cases; every test prints its own):
    singular values against np.linalg.svd        1.6e-15 relative
    modes, 1 - |dot| with svd's right vectors     2.9e-15
    orthonormality of the root-weighted modes     2.3e-13 (7.6e-15 with missing entries; the same under the weighted inner product)
    scores against A V of the svd                 5.7e-14 of the largest singular value
    sklearn explained variance                    2.3e-15 relative
    sklearn scores                                1.0e-13 absolute (scores up to 73)
    sklearn transform of new knees                6.0e-14 absolute
The comparisons with the svd take six components, two of them in the noise; sklearn's take the four planted ones, whose eigenvalues are
well apart (with the two noise components, whose eigenvalues nearly coincide, the scores differ by 1.6e-11: the conditioning of the
question, not an error of either side)."""
import os
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest

import cohort_pca_ref as pref

GATE = 1e-10
SHAPES = ((40, 1100), (130, 1025))
K = 6


def _case(N, V, missing, seed=0):
    """(Y float32 [N, V], mask or None, weights [V]): four planted smooth modes of distinct amplitudes over noise."""
    rng = np.random.default_rng([N, V, int(missing), seed])
    t = np.linspace(0.0, 1.0, V)
    shapes = np.stack([np.sin(np.pi * (k + 1) * t + 0.3 * k) for k in range(4)])
    amp = np.array([1.0, 0.6, 0.35, 0.2])
    Y = (2.5 + (rng.normal(size=(N, 4)) * amp) @ shapes + 0.05 * rng.normal(size=(N, V))).astype(np.float32)
    mask = None
    if missing:
        mask = rng.random((N, V)) >= rng.uniform(0.05, 0.10)
        Y[~mask & (rng.random((N, V)) < 0.5)] = np.nan                  # half of the missing entries are NaN as well
    return Y, mask, rng.uniform(0.2, 1.8, size=V)


def _independent_whitened(Y, mask, weights):
    ok = ~np.isnan(Y) if mask is None else mask & ~np.isnan(Y)
    y = np.where(ok, Y.astype(np.float64), np.nan)
    return np.where(ok, y - np.nanmean(y, axis=0)[None, :], 0.0) * np.sqrt(weights)[None, :]


@pytest.mark.parametrize("missing", (False, True))
@pytest.mark.parametrize("N,V", SHAPES)
def test_fit_against_svd_of_the_whitened_matrix(N, V, missing):
    Y, mask, w = _case(N, V, missing)
    got = pref.fit(Y, mask, w, n_components=K)
    A = _independent_whitened(Y, mask, w)
    _, s, Vt = np.linalg.svd(A, full_matrices=False)
    e_s = np.abs(got.singular_values - s[:K]).max() / s[0]
    e_modes = (1.0 - np.abs((got.modes_w * Vt[:K]).sum(axis=1))).max()
    e_orth = np.abs(got.modes_w @ got.modes_w.T - np.eye(K)).max()
    e_area = np.abs((got.modes_mm * w[None, :]) @ got.modes_mm.T - np.eye(K)).max()
    e_scores = np.abs(np.abs(got.scores) - np.abs(A @ Vt[:K].T)).max() / s[0]
    e_ratio = np.abs(got.explained_variance_ratio - s[:K] ** 2 / (s ** 2).sum()).max()
    print(f"N={N} V={V} missing={missing}: singular {e_s:.2e} modes {e_modes:.2e} orthonormal {e_orth:.2e} area-orthonormal {e_area:.2e} "
          f"scores {e_scores:.2e} ratio {e_ratio:.2e}")
    assert got.singular_values.shape == (K,) and got.modes_mm.shape == (K, V) and got.scores.shape == (N, K) and got.n_excluded == 0
    assert max(e_s, e_modes, e_orth, e_area, e_scores, e_ratio) <= GATE
    assert np.array_equal(got.explained_variance, got.singular_values ** 2 / (N - 1)) or \
        np.abs(got.explained_variance - got.singular_values ** 2 / (N - 1)).max() <= GATE * got.explained_variance[0]
    assert (np.diff(got.singular_values) <= 0).all()


@pytest.mark.parametrize("N,V", SHAPES)
def test_uniform_weights_against_sklearn(N, V):
    sklearn_pca = pytest.importorskip("sklearn.decomposition").PCA
    Y, _, _ = _case(N, V, False)
    new, _, _ = _case(7, V, False, seed=1)
    got = pref.fit(Y, None, np.ones(V), n_components=4)                    # the four planted modes: distinct amplitudes, well separated
    want = sklearn_pca(n_components=4, svd_solver="full").fit(Y.astype(np.float64))
    sign = np.sign((got.modes_mm * want.components_).sum(axis=1))
    e_var = (np.abs(got.explained_variance - want.explained_variance_) / want.explained_variance_).max()
    e_ratio = np.abs(got.explained_variance_ratio - want.explained_variance_ratio_).max()
    e_scores = np.abs(got.scores * sign[None, :] - want.transform(Y.astype(np.float64))).max()
    e_new = np.abs(pref.transform(got, new, None).scores * sign[None, :] - want.transform(new.astype(np.float64))).max()
    print(f"N={N} V={V}: explained variance {e_var:.2e} relative, ratio {e_ratio:.2e}, scores {e_scores:.2e} absolute (largest "
          f"{np.abs(got.scores).max():.3g}), new knees {e_new:.2e}")
    assert max(e_var, e_ratio, e_scores, e_new) <= GATE


@pytest.mark.parametrize("missing", (False, True))
def test_gram_matrix_is_symmetric_to_the_bit_and_its_diagonal_is_norm2(missing):
    Y, mask, w = _case(40, 1100, missing)
    got = pref.fit(Y, mask, w, n_components=2)
    assert np.array_equal(got.G, got.G.T)
    assert np.array_equal(got.G.diagonal(), pref.norm2(got.A))
    swapped = pref.ordered_dot(got.A[:7], got.A[5:])
    assert np.array_equal(swapped, pref.ordered_dot(got.A[5:], got.A[:7]).T)


def test_the_order_of_the_dot_is_not_the_left_to_right_one():
    """Terms spread over many decades: the chunked sum differs from one accumulator over all vertices, so the tests that hold the
    device to ordered_dot hold it to the chunking too."""
    rng = np.random.default_rng(3)
    a = (rng.normal(size=(3, 1537)) * 10.0 ** rng.integers(-8, 8, size=(3, 1537)))
    plain = np.zeros((3, 3))
    for v in range(a.shape[1]):
        plain = plain + a[:, v, None] * a[None, :, v]
    assert not np.array_equal(pref.ordered_dot(a, a), plain)
    assert np.allclose(pref.ordered_dot(a, a), plain, rtol=1e-9)


def test_rank_deficient_cohort_drops_components():
    """N = 5 with two identical knees: centring takes one dimension and the duplicate another, so three components are kept whatever is
    asked for, and the dropped eigenvalues are below 1e-12 of the first (or not positive)."""
    rng = np.random.default_rng(5)
    Y = rng.normal(2.0, 0.5, size=(5, 1025)).astype(np.float32)
    Y[3] = Y[1]
    got = pref.fit(Y, None, np.ones(1025), n_components=10)
    lam = np.linalg.eigvalsh(got.G)[::-1]
    assert got.singular_values.shape == (3,) and got.modes_mm.shape == (3, 1025) and got.scores.shape == (5, 3)
    assert (lam[:3] > pref.DROP * lam[0]).all() and (lam[3:] <= pref.DROP * lam[0]).all()
    assert np.isfinite(got.scores).all() and np.abs(got.scores[3] - got.scores[1]).max() <= GATE * np.abs(got.scores).max()
    assert pref.fit(Y, None, np.ones(1025), n_components=2).singular_values.shape == (2,)
    with pytest.raises(ValueError, match="no variance"):
        pref.fit(np.ones((4, 30), np.float32), None, np.ones(30), n_components=2)


def test_sign_rule():
    R = np.array([[0.1, -0.7, 0.7, 0.2], [0.3, 0.5, -0.9, 0.9], [-0.2, 0.1, 0.0, -0.1]])
    U = np.arange(12, dtype=np.float64).reshape(4, 3) + 1.0
    got_R, got_U = pref.sign_modes(R, U)
    assert np.array_equal(got_R[0], -R[0]) and np.array_equal(got_U[:, 0], -U[:, 0])        # a tie of |value|: the lowest vertex, -0.7, decides
    assert np.array_equal(got_R[1], -R[1]) and np.array_equal(got_U[:, 1], -U[:, 1])        # the tie again: -0.9 comes first
    assert np.array_equal(got_R[2], -R[2]) and np.array_equal(got_U[:, 2], -U[:, 2])
    again_R, again_U = pref.sign_modes(got_R, got_U)
    assert np.array_equal(again_R, got_R) and np.array_equal(again_U, got_U)
    Y, mask, w = _case(40, 1100, True)
    got = pref.fit(Y, mask, w, n_components=K)
    for c in range(K):
        assert got.modes_w[c, int(np.argmax(np.abs(got.modes_w[c])))] > 0.0
    assert np.abs(got.A @ got.modes_w.T - got.scores).max() <= GATE * np.abs(got.scores).max()   # the knees' signs followed the modes'


def test_min_valid_and_a_column_without_a_valid_knee():
    Y, mask, w = _case(40, 1100, True)
    mask = mask.copy()
    mask[:, 7] = False                                                     # no valid knee: the mean is NaN
    mask[:, 11] = np.arange(40) == 3                                       # one valid knee
    mask[:, 13] = np.arange(40) < 4                                        # four
    w = w.copy()
    w[17] = 0.0                                                            # a weight of zero is not an exclusion
    got = pref.fit(Y, mask, w, n_components=K, min_valid=2)
    assert got.n_excluded == 2 and np.isnan(got.mean[7]) and (got.rw[[7, 11, 17]] == 0.0).all() and got.rw[13] > 0.0
    assert np.isnan(got.modes_mm[:, [7, 11, 17]]).all() and np.isfinite(np.delete(got.modes_mm, [7, 11, 17], axis=1)).all()
    for a in (got.G, got.A, got.scores, got.singular_values, got.explained_variance_ratio, got.modes_w):
        assert np.isfinite(a).all()
    assert (got.A[:, [7, 11, 17]] == 0.0).all()
    assert pref.fit(Y, mask, w, n_components=K, min_valid=5).n_excluded == 3
    rec = pref.transform(got, Y[:3], mask[:3])
    assert np.isfinite(rec.scores).all() and np.isfinite(rec.q).all()
    assert np.array_equal(rec.n_missing, (~(mask[:3] & ~np.isnan(Y[:3])) & (got.rw != 0.0)[None, :]).sum(axis=1))
    assert np.abs(rec.scores - got.scores[:3]).max() <= GATE * np.abs(got.scores).max()


def test_member_record_and_q_is_the_squared_residual():
    Y, mask, w = _case(40, 1100, True)
    got = pref.fit(Y, mask, w, n_components=K)
    t2, q, q_fraction = pref.score_record(got.scores, got.G.diagonal(), got.explained_variance)
    resid = got.A - got.scores @ got.modes_w
    assert np.abs(q - (resid * resid).sum(axis=1)).max() <= GATE * got.G.diagonal().max()
    assert ((q_fraction > 0.0) & (q_fraction < 1.0)).all()
    assert abs(t2.sum() - (40 - 1) * K) <= GATE * 40 * K                    # the members' T2 sum to (N - 1) K: the scores' sample covariance is diag


def test_save_and_load_round_trip():
    torch = pytest.importorskip("torch")
    from oai_analysis_2_amd import mesh_processing as mp
    from oai_analysis_2_amd import stats
    V = 12
    verts = np.random.default_rng(0).normal(size=(V, 3)).astype(np.float32)
    faces = np.array([[i, (i + 1) % V, (i + 2) % V] for i in range(V)], np.int32)
    atlas = SimpleNamespace(inner={"FC": mp.Mesh(verts, faces)}, device=torch.device("cpu"), image=lambda vec, kind: np.asarray(vec).reshape(3, 4))
    rng = np.random.default_rng(1)
    Y = rng.normal(2.0, 0.4, size=(9, V)).astype(np.float32)
    mask = rng.random((9, V)) > 0.1
    mask[:, 5] = False
    got = pref.fit(Y, mask, rng.uniform(0.5, 1.5, V), n_components=3)
    surface = stats.ThicknessCohort(atlas, "FC")
    model = stats.ThicknessPCA(surface, got.mean, got.rw, got.rw ** 2, got.modes_w, got.singular_values, got.explained_variance,
                               got.explained_variance_ratio, 9, got.n_excluded, 2)
    assert np.array_equal(model.modes_mm, got.modes_mm, equal_nan=True) and model.n_components == 3
    assert model.image(atlas, mode=1).shape == (3, 4)
    with pytest.raises(ValueError, match="no mode"):
        model.image(atlas, mode=3)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "pca.npz")
        model.save(path)
        with np.load(path, allow_pickle=False) as f:
            assert "scores" not in f.files and "values" not in f.files
        back = stats.ThicknessPCA.load(path, atlas)
        other = SimpleNamespace(inner={"FC": mp.Mesh(verts[:-1], faces[:3] % (V - 1))}, device=torch.device("cpu"))
        with pytest.raises(ValueError, match="vertices"):
            stats.ThicknessPCA.load(path, other)
    for name in ("mean", "root_weights", "weights", "modes_w", "modes_mm", "singular_values", "explained_variance", "explained_variance_ratio"):
        assert np.array_equal(getattr(back, name), getattr(model, name), equal_nan=True), name
    assert (back.kind, back.n_knees, back.n_excluded, back.min_valid) == ("FC", 9, got.n_excluded, 2)
    assert back.scores is None
    with pytest.raises(ValueError, match="loaded model"):
        back.member_scores()
