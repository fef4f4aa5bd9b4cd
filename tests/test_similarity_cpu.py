"""CPU: the numpy restatement of csrc/similarity.hip (tests/similarity_ref.py) held to independent code -- scipy's and torch's filters,
np.histogram2d, np.corrcoef -- and to what LNCC and mutual information must read on images whose likeness is known; the argument checks
of the four entry points, which run before anything touches a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import similarity_ref as sr
from oai_analysis_2_amd import _lib, ops, qc

SHAPE = (12, 40, 70)
SIGMAS = (1.0, 4.0)


@functools.lru_cache(maxsize=None)
def field(seed=0, shape=SHAPE):
    """A smooth field plus noise in [0, 1], float32: structure at the scale of the window and texture below it."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    smooth = 0.5 + 0.2 * np.sin(0.31 * x + 0.4) * np.cos(0.23 * y) + 0.15 * np.sin(0.5 * z + 0.17 * x)
    a = np.clip(smooth + 0.1 * rng.standard_normal(shape), 0.0, 1.0).astype(np.float32)
    a.setflags(write=False)
    return a


def mean_lncc(a, b, sigma):
    taps, radius = sr.gaussian_taps(sigma)
    cc = sr.lncc_map(a, b, taps, radius)
    s = sr.lncc_stats(cc)
    assert s[0] == cc.size and s[1] == 0
    assert abs(s[2] / s[0] - cc.mean()) <= 1e-12                 # the ordered sum is a sum
    return s[2] / s[0]


def test_gaussian_taps():
    for fn in (sr.gaussian_taps, ops.gaussian_taps):
        w, r = fn(4.0)
        assert r == 8 and w.shape == (17,) and w.dtype == np.float64 and abs(w.sum() - 1.0) <= 1e-15 and np.array_equal(w, w[::-1])
        assert abs(w[8] / w[4] - np.exp(0.5)) <= 1e-14           # exp(-16 / 32) four samples out
        assert fn(1.0)[1] == 2 and fn(16.0)[1] == 32 and fn(0.7)[1] == 1
        for sigma in (0.0, -1.0):
            w, r = fn(sigma)
            assert r == 0 and w.tolist() == [1.0]
    for sigma in (0.3, 1.0, 2.5, 4.0, 16.0):
        assert np.array_equal(sr.gaussian_taps(sigma)[0], ops.gaussian_taps(sigma)[0])


@pytest.mark.parametrize("sigma", SIGMAS)
def test_filter_equals_scipy_and_torch(sigma):
    import torch
    import torch.nn.functional as F
    from scipy import ndimage
    taps, radius = sr.gaussian_taps(sigma)
    v = field().astype(np.float64)
    worst = 0.0
    for axis in range(3):
        got = sr.filter_axis(v, taps, radius, axis)
        want = ndimage.correlate1d(v, taps, axis=axis, mode="mirror")
        worst = max(worst, float(np.abs(got - want).max()))
    got = sr.filter3(v, taps, radius)
    t = torch.from_numpy(v)[None, None]
    t = F.pad(t, (radius,) * 6, mode="reflect")
    k = torch.from_numpy(taps)
    for shape in ((1, 1, 1, 1, -1), (1, 1, 1, -1, 1), (1, 1, -1, 1, 1)):
        t = F.conv3d(t, k.reshape(shape))
    worst3 = float(np.abs(got - t[0, 0].numpy()).max())
    print("sigma", sigma, "largest difference per axis against scipy", worst, "of the three passes against torch", worst3)
    assert worst <= 1e-13 and worst3 <= 1e-13


def test_filter_refuses_an_axis_not_longer_than_the_radius():
    taps, radius = sr.gaussian_taps(4.0)
    with pytest.raises(ValueError):
        sr.filter_axis(np.zeros((8, 9, 9)), taps, radius, 0)


def test_lncc_reads_what_it_should():
    a = field()
    noise = np.random.default_rng(5).uniform(0, 1, SHAPE).astype(np.float32)
    shifted = np.roll(a, 3, axis=2)
    got = {}
    for sigma in SIGMAS:
        same, affine, shift, indep = (mean_lncc(a, b, sigma) for b in (a, (0.5 * a + 0.25).astype(np.float32), shifted, noise))
        print("sigma", sigma, "self", same, "affine", affine, "shifted by 3", shift, "independent noise", indep)
        assert 0.99 < same <= 1.0 and affine > 0.99
        assert abs(indep) < 0.01
        got[sigma] = shift
    assert got[1.0] < 0.8 and got[4.0] < 0.9 and got[4.0] > got[1.0]


@pytest.mark.parametrize("bins", [2, 32, 64])
def test_binning_equals_histogram2d_on_in_range_data(bins):
    rng = np.random.default_rng(bins)
    a, b = (rng.uniform(0, 1, 50_000).astype(np.float32) for _ in range(2))
    a[:4], b[:4] = [0.0, 1.0, 0.5, 0.25], [1.0, 0.0, 0.5, 0.75]
    got = sr.joint_histogram(a, b, bins)
    want = np.histogram2d(a, b, bins=bins, range=((0, 1), (0, 1)))[0].astype(np.int64)
    differing = int((got[:-1].reshape(bins, bins) != want).sum())
    print("bins", bins, "cells differing from np.histogram2d", differing)
    assert differing == 0 and got[-1] == 0 and got.sum() == a.size


def test_binning_of_nan_and_out_of_range_values():
    a = np.array([np.nan, 0.5, np.inf, -3.0, 7.0, 0.1, 1.0, 0.0, 0.3], np.float32)
    b = np.array([0.5, np.nan, 0.5, 0.5, 0.5, -np.inf, 2.0, -1.0, 0.9], np.float32)
    h = sr.joint_histogram(a, b, 4)
    t = h[:-1].reshape(4, 4)
    assert h[-1] == 4 and t.sum() == 5                            # NaN and Inf are skipped, finite values outside are clamped
    assert t[0, 2] == 1 and t[3, 2] == 1 and t[3, 3] == 1 and t[0, 0] == 1 and t[1, 3] == 1
    mask = np.array([0, 1, 1, 1, 0, 0, 1, 1, 0], np.uint8)
    h = sr.joint_histogram(a, b, 4, mask=mask)
    assert h[-1] == 2 and h[:-1].sum() == 3 and h.sum() == mask.sum()
    # a range other than [0, 1]
    assert sr.bin_of(np.array([-1.0, 0.0, 0.99, 1.0, 2.9, 3.0, 9.0], np.float32), -1.0, 3.0, 4).tolist() == [0, 1, 1, 2, 3, 3, 3]


def test_mutual_information_of_known_pairs():
    a = field()
    ent = sr.entropies(sr.joint_histogram(a, a, 64), 64)
    mi, nmi = sr.mi_nmi(ent)
    print("self: entropies", ent.tolist(), "mi", mi, "nmi", nmi)
    assert ent[0] == a.size and nmi == 2.0 and abs(mi - ent[1]) <= 1e-12
    rng = np.random.default_rng(11)
    u, v = (rng.uniform(0, 1, 400_000).astype(np.float32) for _ in range(2))
    ent = sr.entropies(sr.joint_histogram(u, v, 64), 64)
    mi, nmi = sr.mi_nmi(ent)
    print("independent: entropies", ent.tolist(), "mi", mi, "nmi", nmi)
    assert 1.0 <= nmi < 1.01 and mi >= -1e-12
    for b in (np.roll(a, 3, axis=2), (0.5 * a + 0.25).astype(np.float32), np.zeros_like(a)):
        assert sr.mi_nmi(sr.entropies(sr.joint_histogram(a, b, 64), 64))[0] >= -1e-12
    # against a plain restatement of the definition
    h = sr.joint_histogram(a, np.roll(a, 1, axis=1), 32)
    p = h[:-1].reshape(32, 32) / h[:-1].sum()
    H = lambda q: float(-(q[q > 0] * np.log(q[q > 0])).sum())
    assert np.allclose(sr.entropies(h, 32)[1:], [H(p.sum(1)), H(p.sum(0)), H(p)], rtol=0, atol=1e-12)
    # an empty table, and a single occupied cell
    assert np.isnan(sr.entropies(np.zeros(17, np.int64), 4)[1:]).all() and sr.entropies(np.zeros(17, np.int64), 4)[0] == 0
    one = np.zeros(17, np.int64)
    one[5] = 1234
    assert sr.entropies(one, 4).tolist() == [1234.0, 0.0, 0.0, 0.0]


def test_ncc_equals_corrcoef():
    a = field()
    for b in (np.roll(a, 3, axis=2), (0.5 * a + 0.25).astype(np.float32), field(3)):
        stats = sr.moments_stats(a, b)
        r, mse = sr.ncc_mse(stats)
        want = np.corrcoef(a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64))[0, 1]
        assert abs(r - want) <= 1e-12 and stats[0] == a.size and stats[1] == 0
        assert abs(mse - np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)) <= 1e-12
        assert qc.ncc_from_moments(stats) == (r, mse)
    planted = a.copy()
    planted[0, 0, :3] = [np.nan, np.inf, -np.inf]
    mask = (np.random.default_rng(2).uniform(size=SHAPE) < 0.5).astype(np.uint8)
    mask[0, 0, :2] = 1
    mask[0, 0, 2] = 0
    stats = sr.moments_stats(planted, a, mask)
    assert stats[1] == 2 and stats[0] == mask.sum() - 2


def test_the_record_from_the_device_slots():
    a, b = field(), np.roll(field(), 2, axis=1)
    taps, radius = sr.gaussian_taps(4.0)
    cc = sr.lncc_map(a, b, taps, radius)
    ent = sr.entropies(sr.joint_histogram(a, b, 64), 64)
    slots = np.concatenate([sr.moments_stats(a, b), sr.lncc_stats(cc), ent])
    rec = qc.similarity_from_stats(slots, 4.0, 64)
    assert rec.n == a.size and rec.nonfinite == 0 and rec.sigma == 4.0 and rec.bins == 64 and rec.cc_map is None
    assert abs(rec.lncc - cc.mean()) <= 1e-12 and abs(rec.lncc_std - cc.std()) <= 1e-9 and (rec.lncc_min, rec.lncc_max) == (cc.min(), cc.max())
    assert (rec.mi, rec.nmi) == sr.mi_nmi(ent) and (rec.entropy_a, rec.entropy_b, rec.entropy_joint) == tuple(ent[1:])
    assert (rec.ncc, rec.mse) == sr.ncc_mse(slots[:8])


def test_signatures_have_the_new_names():
    for name in ("oai_image_moments_workspace_bytes", "oai_image_moments", "oai_joint_histogram", "oai_histogram_entropies",
                 "oai_lncc_workspace_bytes", "oai_lncc"):
        assert name in _lib.SIGNATURES, name
    for name in ("image_moments", "joint_histogram", "histogram_entropies", "lncc", "gaussian_taps"):
        assert callable(getattr(ops, name))


def test_argument_checks_run_without_a_gpu():
    """Bad arguments come back as a non-zero status with a message -- no GPU is touched before the checks."""
    lib = _lib.load()
    dummy = (C.c_float * 8)()
    p = C.cast(dummy, C.c_void_p)
    unit = (C.c_float * 2)(0.0, 1.0)

    def refused(rc, word):
        msg = lib.oai_last_error()
        assert rc != 0 and word in msg, (rc, msg)

    refused(lib.oai_image_moments(None, None, 8, None, None, 0, None, None), b"null")
    refused(lib.oai_image_moments(p, None, 8, None, p, 1 << 20, p, None), b"null")
    refused(lib.oai_image_moments(p, p, -1, None, p, 1 << 20, p, None), b"negative")
    refused(lib.oai_image_moments(p, p, 8, None, p, 8, p, None), b"workspace")
    assert lib.oai_image_moments_workspace_bytes(0) == 0 and lib.oai_image_moments_workspace_bytes(80 * 192 * 192) == 2048 * 8 * 8

    refused(lib.oai_joint_histogram(None, None, 8, unit, unit, 64, None, None, None), b"null")
    refused(lib.oai_joint_histogram(p, p, 8, None, unit, 64, None, p, None), b"null")
    refused(lib.oai_joint_histogram(p, p, 8, unit, unit, 0, None, p, None), b"bins")
    refused(lib.oai_joint_histogram(p, p, 8, unit, unit, 129, None, p, None), b"bins")
    refused(lib.oai_joint_histogram(p, p, 8, (C.c_float * 2)(1.0, 1.0), unit, 64, None, p, None), b"hi > lo")
    refused(lib.oai_joint_histogram(p, p, 8, unit, (C.c_float * 2)(1.0, 0.0), 64, None, p, None), b"hi > lo")
    refused(lib.oai_joint_histogram(p, p, 8, unit, (C.c_float * 2)(0.0, float("nan")), 64, None, p, None), b"hi > lo")

    refused(lib.oai_histogram_entropies(None, 64, None, None), b"null")
    refused(lib.oai_histogram_entropies(p, 0, p, None), b"bins")
    refused(lib.oai_histogram_entropies(p, 129, p, None), b"bins")

    taps = (C.c_double * 67)(*([1.0 / 67] * 67))
    big = 1 << 40
    refused(lib.oai_lncc(None, None, 9, 9, 9, taps, 8, 1e-5, None, None, None, 0, None, None), b"null")
    refused(lib.oai_lncc(p, p, 9, 9, 9, None, 8, 1e-5, None, None, p, big, p, None), b"null")
    refused(lib.oai_lncc(p, p, 40, 40, 40, taps, 33, 1e-5, None, None, p, big, p, None), b"radius")
    refused(lib.oai_lncc(p, p, 40, 40, 40, taps, -1, 1e-5, None, None, p, big, p, None), b"radius")
    for shape in ((8, 9, 9), (9, 8, 9), (9, 9, 8), (0, 9, 9)):
        refused(lib.oai_lncc(p, p, *shape, taps, 8, 1e-5, None, None, p, big, p, None), b"longer than the radius")
    refused(lib.oai_lncc(p, p, 9, 9, 9, taps, 8, 1e-5, None, None, p, 64, p, None), b"workspace")
    refused(lib.oai_lncc(p, p, 9, 9, 9, taps, 8, float("nan"), None, None, p, big, p, None), b"eps")
    assert lib.oai_lncc_workspace_bytes(0, 9, 9) == 0 and lib.oai_lncc_workspace_bytes(80, 192, 192) >= 2 * 5 * 8 * 80 * 192 * 192
