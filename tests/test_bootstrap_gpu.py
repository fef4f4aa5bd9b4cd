"""GPU: the bootstrap kernels (csrc/bootstrap.hip) against their numpy restatement (tests/bootstrap_ref.py) -- coefficient tiles, moments,
quantiles, sup-t and acceleration to the bit -- and oai_analysis_2_amd.stats.bootstrap_ci end to end on a small sphere.  Every float64 is
the result of IEEE add / subtract / multiply / divide / sqrt / floor in a stated order, so equality is exact."""
import functools

import numpy as np
import pytest
import torch

import bootstrap_ref as bref
from cohort_cases import bare_atlas, cohort as _cohort, design, dev, icosphere, knees as _knees, same_bits, sphere_atlas

pytestmark = pytest.mark.gpu

COLUMNS = (1, 2, 4, 6)
VERTS = (1, 63, 65, 257, 600)                     # both sides of a wave (64) and of a block's 256 vertices, several blocks
PLANTED = {"empty": 1, "exact": 2, "unseen": 3, "constant": 4, "dummy": 5}


def _rows_per_thread(p, masked):                  # csrc/bootstrap.hip, rows_per_thread
    return {1: 8, 2: 4, 4: 4, 6: 2}[p] if masked else {1: 16, 2: 16, 4: 8, 6: 8}[p]


def _rows(p, masked):
    """1, 2, one row group minus one, one plus one, two groups + 5."""
    r = _rows_per_thread(p, masked)
    return tuple(sorted({n for n in (1, 2, r - 1, r + 1, 2 * r + 5) if n >= 1}))


@functools.lru_cache(maxsize=None)
def _case(N, V, p, masked):
    """(Y, mask, design, counts) with the header's corner cases planted where the shape has room (V >= 8)."""
    rng = np.random.default_rng([N, V, p, int(masked), 77])
    D = design(N, p, rng)
    Y = (2.0 + 0.5 * rng.normal(size=(N, V)) + 0.3 * D[:, -1:] * rng.random(V)[None, :]).astype(np.float32)
    mask = rng.random((N, V)) >= 0.1 if masked else None
    R = max(_rows(p, masked))
    counts = np.concatenate([np.ones((1, N), np.int64), rng.multinomial(N, np.full(N, 1.0 / N), size=R - 1)]).astype(np.uint16)
    few = min(p + 1, N)
    counts[1, :few] = 0                                                   # row 1 never draws the first p + 1 knees
    counts[2, 0] = 65535                                                  # the largest count
    if V >= 8:
        Y[:, PLANTED["constant"]] = 0.0
        if masked:
            mask[:, PLANTED["constant"]] = True
            mask[:, PLANTED["empty"]] = False
            mask[:, PLANTED["exact"]] = np.arange(N) < p                  # exactly p valid knees
            mask[:, PLANTED["unseen"]] = np.arange(N) < few               # row 1 has count 0 on every valid knee
            if N >= 31 and p in (4, 6):
                mask[:, PLANTED["dummy"]] = D[:, 1] == 1.0                # the sex dummy is constant among the valid knees
    for a in (Y, mask, D, counts):
        if a is not None:
            a.setflags(write=False)
    return Y, mask, D, counts


@functools.lru_cache(maxsize=None)
def _reference(N, V, p, masked):
    Y, mask, D, counts = _case(N, V, p, masked)
    theta, n, ok = bref.coef(Y, mask, D, counts)
    theta.setflags(write=False)
    return theta, n, ok


def _spans(V):
    return tuple(sorted({(0, V), (1, V - 1) if V >= 3 else (0, V), (V // 2, V // 2 + 1)}))


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "no_mask"])
@pytest.mark.parametrize("p", COLUMNS)
def test_coefficient_tile_n_and_ok_equal_the_restatement_to_the_bit(p, masked):
    from oai_analysis_2_amd import ops
    for N in _knees(p):
        for V in VERTS:
            Y, mask, D, counts = _case(N, V, p, masked)
            theta, n_ref, ok_ref = _reference(N, V, p, masked)
            y_d, m_d, d_d, c_d = dev(Y), None if mask is None else dev(mask.astype(np.uint8)), dev(D), dev(counts)
            where = f"N={N} V={V}"
            for R in _rows(p, masked):
                n = torch.full((V,), -7, dtype=torch.int32, device="cuda")
                ok = torch.full((V,), -7, dtype=torch.int32, device="cuda")
                tile = ops.bootstrap_coef(y_d, d_d, c_d, 0, R, mask=m_d, n=n, ok=ok)
                same_bits(tile, theta[:R], f"{where} R={R} theta")
                same_bits(n, n_ref, f"{where} R={R} n")
                same_bits(ok, ok_ref, f"{where} R={R} ok")
            R = counts.shape[0]
            for v0, v1 in _spans(V):
                n = torch.full((V,), -7, dtype=torch.int32, device="cuda")
                tile = ops.bootstrap_coef(y_d, d_d, c_d, 0, R, mask=m_d, v0=v0, v1=v1, n=n)
                same_bits(tile, np.ascontiguousarray(theta[:, v0:v1]), f"{where} span [{v0}, {v1}) theta")
                want = np.full(V, -7, np.int32)
                want[v0:v1] = n_ref[v0:v1]
                same_bits(n, want, f"{where} span [{v0}, {v1}) n")        # nothing outside the span is written
            if R > 4:                                                      # a batch that does not start at row 0 leaves n alone
                n = torch.full((V,), -7, dtype=torch.int32, device="cuda")
                tile = ops.bootstrap_coef(y_d, d_d, c_d, 3, R, mask=m_d, n=n)
                same_bits(tile, np.ascontiguousarray(theta[3:]), f"{where} rows [3, {R}) theta")
                assert (n == -7).all()
            # on the restatement: what was planted is really there
            assert (n_ref == (N if not masked else mask.sum(axis=0))).all()
            if V >= 8:
                at = PLANTED
                assert (theta[:, at["constant"]] == 0.0).all() or np.isnan(theta[:, at["constant"]]).any()
                if masked:
                    assert np.isnan(theta[:, at["empty"]]).all() and n_ref[at["empty"]] == 0 and ok_ref[at["empty"]] == 0
                    assert n_ref[at["exact"]] == p
                    if R > 1:
                        assert np.isnan(theta[1, at["unseen"]]) and n_ref[at["unseen"]] == min(p + 1, N)
                    if N >= 31 and p in (4, 6):
                        assert np.isnan(theta[:, at["dummy"]]).all() and ok_ref[at["dummy"]] == 0 and n_ref[at["dummy"]] >= p + 1
            if N >= 31:
                assert not np.isnan(theta[0, 0]) and not np.isnan(theta[:, 0]).all()
            if R > 2:
                assert counts[2, 0] == 65535


@pytest.mark.parametrize("p", COLUMNS)
def test_no_mask_gives_the_bits_of_a_mask_of_all_ones(p):
    from oai_analysis_2_amd import ops
    N, V = 33, 257
    Y, _, D, counts = _case(N, V, p, False)
    theta, n_ref, ok_ref = _reference(N, V, p, False)
    y_d, d_d, c_d = dev(Y), dev(D), dev(counts)
    ones = torch.ones((N, V), dtype=torch.uint8, device="cuda")
    for m_d, what in ((None, "no mask"), (ones, "all ones")):              # two kernels, two row groupings
        n, ok = torch.zeros(V, dtype=torch.int32, device="cuda"), torch.zeros(V, dtype=torch.int32, device="cuda")
        same_bits(ops.bootstrap_coef(y_d, d_d, c_d, 0, counts.shape[0], mask=m_d, n=n, ok=ok), theta, f"theta ({what})")
        same_bits(n, n_ref, f"n ({what})")
        same_bits(ok, ok_ref, f"ok ({what})")
    assert (n_ref == N).all() and not np.isnan(theta[0]).any()


# ---- order statistics --------------------------------------------------------------------------------------------------------------------
ROWS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)       # both sides of a wave and of a block's 256 threads; several strides of a block
QVERTS = (1, 65, 600)


def _replicates(R, V, seed):
    """A tile with heavy ties, an all-equal column, signed zeros, infinities, NaN entries and an all-NaN column where V has room."""
    rng = np.random.default_rng([R, V, seed])
    t = 2.0 + 0.3 * rng.normal(size=(R, V))
    t[:, 0] = np.round(3 * t[:, 0])
    if V > 8:
        t[:, 1] = 3.25
        t[:, 2] = rng.choice([0.0, -0.0, 1.0, -1.0], size=R)
        t[:, 3] = rng.choice([np.inf, -np.inf, 0.5, 2.0], size=R)
        t[rng.random(R) < 0.5, 4] = np.nan
        t[:, 5] = np.nan
        t[:, 6] = 2.5                                                      # every replicate equals the observed value: se == 0
        t[rng.random(R) < 0.1, 7] = np.inf
    return t


def _probabilities(n):
    """0 and 1 belong to every call; then a probability on an integer virtual index, and one at interpolation weight 0.5 with its
    neighbour just below."""
    if n < 2:
        return [np.array([0.0, 1.0, 0.5, 0.3])]
    k = (n - 1) // 3
    half = (k + 0.5) / (n - 1)
    return [np.array([0.0, 1.0, k / (n - 1), 0.05]), np.array([half, np.nextafter(half, 0.0), 0.95, 1.0 / 3.0])]


@pytest.mark.parametrize("V", QVERTS)
def test_column_quantiles_equal_the_restatement_to_the_bit(V):
    from oai_analysis_2_amd import ops
    for R in ROWS:
        t = _replicates(R, V, 1)
        t_d = dev(t)
        for first in (0, 1):
            for probs in _probabilities(R - first):
                want, count = bref.column_quantiles(t, probs, first)
                got, n = ops.column_quantiles(t_d, probs, first_row=first)
                same_bits(got, want, f"R={R} V={V} first={first} shared")
                same_bits(n, count, f"R={R} V={V} first={first} count")
        rng = np.random.default_rng([R, V])
        per_vertex = rng.random((4, V))
        per_vertex[0, 0], per_vertex[1, 0], per_vertex[2, 0], per_vertex[3, 0] = np.nan, -0.25, 1.0, 0.0
        per_vertex[:, V // 2] = [1.5, 0.5, np.nan, 1.0]
        want, count = bref.column_quantiles(t, per_vertex, 1)
        got, n = ops.column_quantiles(t_d, dev(per_vertex), first_row=1)
        same_bits(got, want, f"R={R} V={V} per vertex")
        same_bits(n, count, f"R={R} V={V} per vertex count")
        assert np.isnan(want[0 if V > 1 else 2, V // 2]) and (V <= 8 or (np.isnan(want[:2, 0]).all() and count[5] == 0 and np.isnan(want[:, 5]).all()))
    # against numpy itself, where the column has neither a NaN nor opposite infinities
    t = _replicates(257, V, 2)
    probs = np.array([0.0, 0.05, 0.5, 1.0])
    got = ops.column_quantiles(dev(t), probs)[0].cpu().numpy()
    clean = ~np.isnan(t).any(axis=0) & ~np.isinf(t).any(axis=0)
    assert clean.sum() >= min(V, V - 5) and np.array_equal(got[:, clean], np.quantile(t[:, clean], probs, axis=0))


@pytest.mark.parametrize("V", QVERTS)
def test_moments_and_sup_equal_the_restatement_to_the_bit(V):
    from oai_analysis_2_amd import ops
    for R in ROWS:
        t = _replicates(R, V, 3)
        t_d = dev(t)
        want = bref.moments(t)
        got = ops.bootstrap_moments(t_d)
        for name in ("n_finite", "mean", "se", "below", "equal"):
            same_bits(getattr(got, name), want[name], f"R={R} V={V} {name}")
        if V > 8 and R > 2:
            assert want["se"][6] == 0.0 and want["equal"][6] == R - 1 and want["n_finite"][5] == 0 and np.isnan(want["se"][5])
        running = np.random.default_rng(R).random(R) * (np.arange(R) % 2)          # a running maximum that some rows exceed and some do not
        sup = dev(running)
        ops.bootstrap_sup(t_d, got.se, sup)
        same_bits(sup, bref.sup(t, want["se"], running), f"R={R} V={V} sup")
        half = V // 2                                                              # two spans fold to the whole
        if half:
            sup2 = torch.zeros(R, dtype=torch.float64, device="cuda")
            for a, b in ((0, half), (half, V)):
                ops.bootstrap_sup(t_d[:, a:b].contiguous(), got.se[a:b].contiguous(), sup2)
            same_bits(sup2, bref.sup(t, want["se"], np.zeros(R)), f"R={R} V={V} sup over two spans")


@pytest.mark.parametrize("V", QVERTS)
def test_acceleration_equals_the_restatement_to_the_bit(V):
    from oai_analysis_2_amd import ops
    for N in (2, 7, 33, 65):
        rng = np.random.default_rng([N, V, 4])
        jack = 2.0 + 0.2 * rng.normal(size=(N, V))
        strata = (np.arange(N) >= max(N // 3, 1)).astype(np.int32)                 # two strata of unequal size
        mask = rng.random((N, V)) >= 0.15
        if V > 8:
            mask[:, 1] = strata == 0                                               # valid in one stratum only
            mask[:, 2] = False
            jack[:, 3] = 1.5                                                       # no spread: the denominator is 0
            jack[N // 2, 4], mask[N // 2, 4] = np.nan, True                        # a NaN on a valid knee
            jack[N // 2, 5], mask[N // 2, 5] = np.nan, False                       # a NaN on a missing one does not count
        for m, S, what in ((mask, 2, "masked"), (None, 2, "no mask"), (mask, 1, "one stratum of two labels"), (None, 3, "an empty stratum")):
            want = bref.acceleration(jack, m, strata, S)
            got = ops.jackknife_acceleration(dev(jack), dev(strata), S, mask=None if m is None else dev(m.astype(np.uint8)))
            same_bits(got, want, f"N={N} V={V} {what}")
        want = bref.acceleration(jack, mask, strata, 2)
        if V > 8:
            assert np.isnan(want[2]) and np.isnan(want[3]) and np.isnan(want[4]) and (N < 7 or not np.isnan(want[5]))
            assert N < 7 or not np.isnan(want[1])
            a, b = 3, V - 2                                                        # a span inside the cohort's vertices
            got = ops.jackknife_acceleration(dev(np.ascontiguousarray(jack[:, a:b])), dev(strata), 2, mask=dev(mask.astype(np.uint8)), v0=a)
            same_bits(got, want[a:b], f"N={N} V={V} span")


# ---- the public interface --------------------------------------------------------------------------------------------------------------
N_E2E, B_E2E, LEVEL = 24, 199, 0.9
FIELDS = ("estimate", "se", "lower", "upper", "n", "n_finite", "z0", "acceleration", "sup", "lower_simultaneous", "upper_simultaneous")


def _image(vec, kind):
    """Stands for the atlas' rasteriser."""
    return np.asarray(vec, np.float32).reshape(1, -1)


@functools.lru_cache(maxsize=None)
def _painted():
    """24 knees on the sphere: 2 mm + 0.1 mm noise, 0.3 mm more in group 1 and 0.2 mm per unit of x on the cap z > 0.8; 3 % of the entries
    and one whole vertex are missing."""
    verts, _ = icosphere()
    cap = verts[:, 2] > 0.8
    rng = np.random.default_rng(2026)
    groups = np.array([3] * 10 + [8] * 14)
    rng.shuffle(groups)
    x, age = rng.normal(size=N_E2E), rng.uniform(45, 80, N_E2E)
    Y = 2.0 + 0.1 * rng.normal(size=(N_E2E, len(verts)))
    Y[:, cap] += 0.3 * (groups == 8)[:, None] + 0.2 * x[:, None]
    Y = Y.astype(np.float32)
    Y[rng.random(Y.shape) < 0.03] = np.nan
    Y[:, 17] = np.nan
    return Y, groups, x, age, cap


def _check(res, want, what):
    for name in FIELDS:
        if name in want:
            same_bits(getattr(res, name), want[name], f"{what} {name}")
        else:
            assert getattr(res, name) is None, (what, name)
    assert res.critical == want.get("critical")


@pytest.mark.parametrize("method", ["percentile", "basic", "bca"])
def test_bootstrap_ci_equals_the_restatement_to_the_bit(method):
    from oai_analysis_2_amd import stats
    Y, groups, x, age, cap = _painted()
    atlas = sphere_atlas(image=_image)
    cohort = _cohort(atlas, Y, chunk=7)
    mask = cohort.mask.cpu().numpy() != 0
    values = cohort.values.cpu().numpy()
    assert np.array_equal(mask, ~np.isnan(Y))
    for what, kw in (("mean", {}), ("difference", dict(groups=groups, covariates=age)), ("slope", dict(x=x, covariates=age))):
        res = stats.bootstrap_ci(cohort, n_bootstrap=B_E2E, level=LEVEL, method=method, simultaneous=True, seed=5, batch=100, **kw)
        assert res.what == what and res.kind == "FC" and res.n_bootstrap == B_E2E and res.method == method and res.level == LEVEL
        labels = bref.design_of(N_E2E, **kw)[2]
        counts = stats.bootstrap_counts(N_E2E, B_E2E, seed=5, blocks=labels).counts
        want = bref.ci(values, mask, counts, LEVEL, method, simultaneous=True, **kw)
        _check(res, want, f"{method} {what}")
        assert np.array_equal(res.n, mask.sum(axis=0)) and np.isnan(res.estimate[17]) and np.isnan(res.lower[17])
        ordinary = np.delete(np.arange(len(cap)), 17)
        assert (res.lower[ordinary] <= res.upper[ordinary]).all() and (res.se[ordinary] > 0).all()
        assert (res.lower_simultaneous[ordinary] < res.lower[ordinary]).mean() > 0.9        # the band is wider than the pointwise interval
        if what == "difference":
            assert (res.n_finite == B_E2E).sum() >= len(cap) - 5                            # stratified: no group is ever drawn empty
        for name in stats.BootstrapResult.IMAGES:
            if method != "bca" and name in ("z0", "acceleration"):
                with pytest.raises(ValueError, match="bca"):
                    res.image(atlas, name)
            else:
                assert res.image(atlas, name).dtype == np.float32 and res.image(atlas, name).size == len(cap)
        with pytest.raises(ValueError, match="no image"):
            res.image(atlas, "t")
        # another span size, the default one, and a second run: the same bits in every field
        for other, note in ((stats.bootstrap_ci(cohort, n_bootstrap=B_E2E, level=LEVEL, method=method, simultaneous=True, seed=5, batch=257, **kw), "span 257"),
                            (stats.bootstrap_ci(cohort, n_bootstrap=B_E2E, level=LEVEL, method=method, simultaneous=True, seed=5, **kw), "default span"),
                            (stats.bootstrap_ci(cohort, level=LEVEL, method=method, simultaneous=True, counts=counts, batch=100, **kw), "again, rows handed over")):
            _check(other, want, f"{method} {what} ({note})")


def test_a_vertex_permutation_of_the_cohort_permutes_the_result():
    from oai_analysis_2_amd import stats
    Y, groups, _, age, _ = _painted()
    order = np.random.default_rng(9).permutation(Y.shape[1])
    bare = bare_atlas(Y.shape[1])
    kw = dict(groups=groups, covariates=age, n_bootstrap=B_E2E, level=LEVEL, method="bca", simultaneous=True, seed=5, batch=200)
    res, moved = stats.bootstrap_ci(_cohort(bare, Y, chunk=7), **kw), stats.bootstrap_ci(_cohort(bare, Y[:, order], chunk=7), **kw)
    for name in FIELDS:
        a, b = getattr(res, name), getattr(moved, name)
        same_bits(b, a if name == "sup" else a[order], name)
    assert moved.critical == res.critical


def test_without_simultaneous_or_bca_their_fields_are_absent_and_bad_arguments_are_refused():
    from oai_analysis_2_amd import stats
    Y, groups, x, _, _ = _painted()
    atlas = sphere_atlas(image=_image)
    cohort = _cohort(atlas, Y, chunk=7)
    res = stats.bootstrap_ci(cohort, n_bootstrap=20)
    assert res.z0 is None and res.acceleration is None and res.sup is None and res.critical is None and res.lower_simultaneous is None
    with pytest.raises(ValueError, match="simultaneous"):
        res.image(atlas, "lower_simultaneous")
    with pytest.raises(ValueError, match="bca"):
        res.image(atlas, "z0")
    for kw, words in ((dict(method="studentized"), "method"), (dict(level=1.0), "level"), (dict(x=x, groups=groups), "not both"),
                      (dict(covariates=x), "intercept alone"), (dict(groups=np.arange(N_E2E)), "two labels"),
                      (dict(x=np.ones(N_E2E)), "x is constant"), (dict(x=x, covariates=np.stack([x, 2 * x], axis=1)), "rank"),
                      (dict(batch=0), "batch"), (dict(counts=np.ones((1, N_E2E), int)), "counts")):
        with pytest.raises(ValueError, match=words):
            stats.bootstrap_ci(cohort, n_bootstrap=20, **kw)
