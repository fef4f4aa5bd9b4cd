"""CPU: the numpy restatement of surface smoothing (tests/graph_smooth_ref.py) against its own loop form, a scipy sparse matrix power, the
lattice calibration behind ``stats.sweeps_for_fwhm`` and a constant field under a mask; and the host helpers of oai_analysis_2_amd.stats."""
import math

import numpy as np
import pytest

import graph_smooth_ref as sref
from cohort_cases import same_bits
from oai_analysis_2_amd import stats
from oai_analysis_2_amd.stats import surface_edge_d2, surface_edge_weights, surface_step_variance, sweeps_for_fwhm


def _sphere_graph(level=1):
    verts, faces = sref.icosphere(level)
    off, nbr = sref.face_adjacency(len(verts), faces)
    return verts, off, nbr


def test_the_vectorised_restatement_equals_the_loop_form_to_the_bit():
    verts, off, nbr = _sphere_graph(1)
    V = len(verts)
    assert V == 42
    rng = np.random.default_rng(5)
    x = rng.normal(2.0, 0.5, (3, V))
    mask = (rng.random((3, V)) > 0.3).astype(np.uint8)
    x[mask == 0] = np.nan                                                  # what lies under a 0 mask must not matter
    w = rng.uniform(0.0, 2.0, len(nbr))
    w[rng.random(len(nbr)) < 0.1] = 0.0
    sw = rng.uniform(0.0, 2.0, V)
    sw[::5] = 0.0
    for fill in (False, True):
        for K in (1, 3):
            for self_weight in (None, sw):
                got, got_m = sref.smooth(x, mask, off, nbr, w, self_weight, K, fill)
                want, want_m = sref.smooth_loop(x, mask, off, nbr, w, self_weight, K, fill)
                same_bits(got_m, want_m, f"mask fill={fill} K={K}")
                same_bits(got, want, f"values fill={fill} K={K}")
                assert not np.isnan(got).any()
                if not fill:
                    assert not (got_m & ~mask.astype(bool)).any()
    filled = sref.smooth(x, mask, off, nbr, np.ones(len(nbr)), None, 3, True)[1]
    assert filled.sum() > mask.sum()


def test_with_nothing_missing_it_is_a_power_of_the_row_normalised_matrix():
    from scipy import sparse
    verts, off, nbr = _sphere_graph(2)
    V = len(verts)
    w = surface_edge_weights(verts, off, nbr, 0.3)
    owner = np.repeat(np.arange(V), np.diff(off))
    W = sparse.csr_matrix((w, (owner, nbr)), shape=(V, V)) + sparse.identity(V, format="csr")
    A = sparse.diags(1.0 / np.asarray(W.sum(axis=1)).ravel()) @ W
    x = np.random.default_rng(6).normal(2.0, 0.5, (4, V))
    want = x.T.copy()
    for K in (1, 2, 6):
        want = x.T.copy()
        for _ in range(K):
            want = A @ want
        got, m = sref.smooth(x, None, off, nbr, w, None, K, False)
        assert m.all()
        np.testing.assert_allclose(got, want.T, rtol=1e-12, atol=0.0)


def test_on_a_lattice_the_second_moment_of_the_impulse_response_is_k_times_the_step_variance():
    n, K = 15, 5
    verts, off, nbr = sref.triangular_lattice(n)
    centre = (n // 2) * n + n // 2
    w = surface_edge_weights(verts, off, nbr, 0.8)
    d2 = surface_edge_d2(verts, off, nbr)
    np.testing.assert_allclose(d2, 1.0, rtol=1e-14)
    s = surface_step_variance(off, nbr, w, d2)
    x = np.zeros((1, n * n))
    x[0, centre] = 1.0
    got, m = sref.smooth(x, None, off, nbr, w, None, K, False)
    r2 = ((verts - verts[centre]) ** 2).sum(axis=1)
    assert abs(got[0].sum() - 1.0) < 1e-14
    assert np.count_nonzero(got[0]) == 1 + 3 * K * (K + 1) == 91
    moment = float((got[0] * r2).sum())
    print(f"second moment {moment!r}, K * s {K * s[centre]!r}, relative difference {abs(moment - K * s[centre]) / (K * s[centre]):.2e}")
    np.testing.assert_allclose(moment, K * s[centre], rtol=1e-12)
    # so the calibration asks for K sweeps when it is given the FWHM of that second moment
    fwhm = math.sqrt(8.0 * math.log(2.0) * K * s[centre] / 2.0)
    assert sweeps_for_fwhm(fwhm, s[centre]) == K


def test_a_constant_field_stays_constant_where_it_is_valid():
    verts, off, nbr = _sphere_graph(2)
    V = len(verts)
    rng = np.random.default_rng(7)
    mask = (rng.random((5, V)) > 0.3).astype(np.uint8)
    w = surface_edge_weights(verts, off, nbr, 0.25)
    maxdeg = int(np.diff(off).max())
    for K in (1, 4, 9):
        got, m = sref.smooth(np.full((5, V), 2.37), mask, off, nbr, w, None, K, False)
        assert np.array_equal(m, mask)                                     # keep mode, positive self weight: nothing drops out, nothing appears
        valid = m != 0
        bound = K * (maxdeg + 2) * 2.0 ** -52                              # K weighted averages of at most maxdeg + 1 terms and a division
        assert np.abs(got[valid] / 2.37 - 1.0).max() <= bound
        assert (got[~valid] == 0).all()


def test_edge_weights_are_the_stated_gaussian_of_the_edge_length():
    verts, off, nbr = _sphere_graph(1)
    V = len(verts)
    sigma = 0.4
    w = surface_edge_weights(verts, off, nbr, sigma)
    d2 = surface_edge_d2(verts, off, nbr)
    assert w.dtype == np.float64 and w.shape == nbr.shape == d2.shape
    v = verts.astype(np.float64)
    for i in range(V):
        for e in range(off[i], off[i + 1]):
            dx, dy, dz = (v[nbr[e]] - v[i]).tolist()
            want_d2 = dx * dx + dy * dy + dz * dz
            assert d2[e] == want_d2 and w[e] == np.exp(-want_d2 / (2 * sigma ** 2))
    s = surface_step_variance(off, nbr, w, d2)
    for i in (0, 17, V - 1):
        sl = slice(off[i], off[i + 1])
        np.testing.assert_allclose(s[i], (w[sl] * d2[sl]).sum() / (1.0 + w[sl].sum()), rtol=1e-15)
    assert abs(stats.mean_edge_length(verts, off, nbr) - np.sqrt(d2).mean()) < 1e-15
    # the clamping of the kernel: a slot that is never read and a neighbour out of range weigh nothing
    off2, nbr2 = off.copy(), np.concatenate([nbr, [5]]).astype(np.int32)
    nbr2[3] = V + 7
    w2 = surface_edge_weights(verts, off2, nbr2, sigma)
    assert w2[3] == 0.0 and w2[-1] == 0.0 and np.array_equal(np.delete(w2, [3, len(nbr)]), np.delete(w, 3))
    with pytest.raises(ValueError, match="sigma_step"):
        surface_edge_weights(verts, off, nbr, 0.0)


def test_sweeps_for_fwhm():
    s = np.array([0.0, 0.4, 0.5, 0.6])                                      # vertex 0 has no neighbour: the mean is 0.5
    ks = [sweeps_for_fwhm(f, s) for f in (0.01, 0.5, 1.0, 2.0, 3.0, 5.0, 8.0, 20.0)]
    assert ks[0] == 1 and ks == sorted(ks) and ks[-1] > ks[1]
    sigma2 = (5.0 / math.sqrt(8.0 * math.log(2.0))) ** 2
    assert sweeps_for_fwhm(5.0, s) == round(2.0 * sigma2 / 0.5) == sweeps_for_fwhm(5.0, 0.5)
    assert sweeps_for_fwhm(5.0, s, has_neighbour=[True, True, True, True]) == round(2.0 * sigma2 / 0.375)
    # round half to even: 2 sigma^2 / s = 2.5 and 3.5
    for ratio, want in ((2.5, 2), (3.5, 4)):
        fwhm = math.sqrt(8.0 * math.log(2.0) * ratio * 0.5 / 2.0)
        got = sweeps_for_fwhm(fwhm, 0.5)
        assert got in (want, round(ratio + 1e-9), round(ratio - 1e-9))     # the square root may land either side of the half
    with pytest.raises(ValueError, match="larger sigma_step"):
        sweeps_for_fwhm(200.0, s)
    with pytest.raises(ValueError, match="fwhm_mm"):
        sweeps_for_fwhm(0.0, s)
    with pytest.raises(ValueError, match="step variance"):
        sweeps_for_fwhm(5.0, np.zeros(4))


def test_the_smoother_refuses_bad_settings_before_it_looks_at_the_atlas():
    """The atlas is None: a refusal that came after the first look at it would be another error."""
    for kwargs, match in ((dict(), "exactly one"), (dict(fwhm_mm=5.0, sweeps=3), "exactly one"), (dict(fwhm_mm=5.0, missing="drop"), "missing"),
                          (dict(fwhm_mm=-1.0), "fwhm_mm"), (dict(fwhm_mm=float("nan")), "fwhm_mm"), (dict(sweeps=0), "sweeps"),
                          (dict(sweeps=4097), "sweeps"), (dict(sweeps=3, sigma_step=0.0), "sigma_step")):
        with pytest.raises(ValueError, match=match):
            stats.SurfaceSmoother(None, "FC", **kwargs)
    settings = stats.Smoothing(5.0, 4.9, 70, 0.6, "keep")
    with pytest.raises(Exception):
        settings.sweeps = 3                                                # frozen
    assert stats.smoothing_batch(30002, 1000) == (256 << 20) // (30002 * 27) == 331 and stats.smoothing_batch(30002, 200) == 200 and stats.smoothing_batch(30002, 7) == 7
    assert stats.smoothing_batch(1 << 30, 5) == 1
