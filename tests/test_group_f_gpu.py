"""GPU: the F kernel of the cohort regression (csrc/group_regression.hip, oai_regression_f) against its numpy restatement
(tests/group_f_ref.py) -- F tile, the coefficients of row 0, max F and the exceedance counts to the bit --, against the t kernel for one
tested column, and oai_analysis_2_amd.stats.anova_test end to end on a small sphere.  Every float64 is the result of IEEE add / subtract /
multiply / divide / sqrt in a stated order, so equality is exact."""
import functools

import numpy as np
import pytest
import torch

import graph_tfce_ref as tref
import group_f_ref as fref
import group_regression_ref as rref
import group_stats_ref as gref
from cohort_cases import cohort as _cohort, icosphere, rows as _rows, same_bits, same_result, sphere_atlas, sphere_graph

pytestmark = pytest.mark.gpu

# (p, k): k = p without an intercept (the cell means of two levels); one-way layouts of 3 and 5 levels; a 3-level factor with a covariate;
# a 4-level factor with two covariates.  With a mask these are R = 8, 2, 2, 1, 1 rows per thread, without one R = 16, 8, 8, 8, 8.
SHAPES = ((2, 2), (3, 2), (4, 2), (5, 4), (6, 3))
VERTS = (1, 63, 65, 257, 600)                     # both sides of a wave (64) and of a block's 256 vertices, several blocks


def _knees(p):
    return (p + 1, 31, 65)


def _rows_per_thread(p, masked):                  # csrc/group_regression.hip, rows_per_thread
    return {2: 8, 3: 2, 4: 2, 5: 1, 6: 1}[p] if masked else {2: 16, 3: 8, 4: 8, 5: 8, 6: 8}[p]


def _batch(p, masked):
    """One full row group and a ragged one."""
    r = _rows_per_thread(p, masked)
    return r + max(1, r // 4)


def _levels(p, k):
    return k if p == k else k + 1


def _design(N, p, k, rng):
    """([N, p] with the k columns of interest last, the level of every knee).  (2, 2): the 0 / 1 indicators of two levels and no
    intercept.  Otherwise: the intercept, p - k - 1 continuous covariates, and a 0 / 1 dummy for every level after the first."""
    level = np.arange(N) % _levels(p, k)
    if p == k:
        cols = [(level == g).astype(np.float64) for g in range(k)]
    else:
        cols = [np.ones(N)] + [60 + 8 * rng.normal(0.0, 1.0, N) for _ in range(p - k - 1)] + [(level == g).astype(np.float64) for g in range(1, k + 1)]
    return np.ascontiguousarray(np.stack(cols, axis=1)), level


PLANTED = {"empty": 1, "dof0": 2, "dof1": 3, "constant": 4, "level_missing": 5, "level_sometimes": 6}
PLANTED_ROW = 3                                   # the row that takes the last level away from vertex "level_sometimes"


@functools.lru_cache(maxsize=None)
def _case(N, V, p, k, masked):
    """(Y, mask, design, perm) with the header's corner cases planted where the shape has room (V >= 8, and for the last two N >= 31)."""
    rng = np.random.default_rng([N, V, p, k, int(masked)])
    D, level = _design(N, p, k, rng)
    Y = (2.0 + 0.5 * rng.normal(size=(N, V)) + 0.3 * (level[:, None] == 1) * rng.random(V)[None, :]).astype(np.float32)
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
            if N >= 31:
                last = _levels(p, k) - 1
                mask[:, PLANTED["level_missing"]] = level != last         # the last dummy is 0 on every valid knee: a pivot of M is refused
                few = 4 * (last + 1)
                mask[:, PLANTED["level_sometimes"]] = np.arange(N) < few  # few valid knees; one row hands them design rows without the last level
                others = np.nonzero(level != last)[0][:few]
                rest = np.setdiff1d(np.arange(N), others)
                perm[PLANTED_ROW, :few], perm[PLANTED_ROW, few:] = others, rng.permutation(rest)
    for a in (Y, mask, D, perm):
        if a is not None:
            a.setflags(write=False)
    return Y, mask, D, perm


def _prepare_ref(Y, mask, D, k):
    q = D.shape[1] - k
    return rref.prepare(Y, mask, D[:, :q] if q else None, centre=q > 0)


@functools.lru_cache(maxsize=None)
def _reference(N, V, p, k, masked):
    Y, mask, D, perm = _case(N, V, p, k, masked)
    prep = _prepare_ref(Y, mask, D, k)
    F, coef = fref.regression_f(prep, mask, D, perm, k, with_coef=True)
    F.setflags(write=False)
    return prep, F, coef


def _prepare_device(Y, mask, D, k):
    from oai_analysis_2_amd import ops
    q = D.shape[1] - k
    return ops.regression_prepare(torch.from_numpy(np.array(Y)).cuda(), None if mask is None else torch.from_numpy(mask.astype(np.uint8)).cuda(),
                                  torch.from_numpy(np.ascontiguousarray(D[:, :q])).cuda() if q else None, centre=q > 0)


def _device(prep, D, perm, k, batch):
    from oai_analysis_2_amd import ops
    P, V = perm.shape[0], prep.n_verts
    design, index = torch.from_numpy(np.array(D)).cuda(), torch.from_numpy(np.array(perm)).cuda()
    f0 = torch.full((V,), 7.0, dtype=torch.float64, device="cuda")
    coef0 = torch.full((k, V), 7.0, dtype=torch.float64, device="cuda")
    max_f = torch.full((P,), -1.0, dtype=torch.float64, device="cuda")
    exceed = torch.full((V,), -5, dtype=torch.int64, device="cuda")            # garbage: the first batch must start it
    tiles = []
    for p0 in range(0, P, batch):
        p1 = min(p0 + batch, P)
        tile = ops.regression_f(prep, design, index, p0, p1, k, coef0=coef0)   # later batches must leave coef0 alone
        ops.permutation_reduce(tile, p0, f0, max_f, exceed)
        tiles.append(tile.clone())
    return torch.cat(tiles), coef0, f0, max_f, exceed


def _planted_cases_occur(N, V, p, k, ref, F_ref, coef_ref):
    """On the restatement: every corner case that was planted is really there."""
    at = PLANTED
    assert np.isnan(F_ref[:, at["constant"]]).all() and ref["Q"][at["constant"]] == 0.0 and ref["ok"][at["constant"]] == 1
    assert np.isnan(F_ref[:, at["empty"]]).all() and ref["n"][at["empty"]] == 0 and ref["ok"][at["empty"]] == 0
    if N > p:
        assert ref["n"][at["dof0"]] == p and np.isnan(F_ref[:, at["dof0"]]).all() and np.isnan(coef_ref[:, at["dof0"]]).all()
        assert ref["ok"][at["dof0"]] == (1 if k >= 2 else 0)               # prepare's own rule lets it pass: the kernel's dof >= 1 refuses it
    assert ref["n"][at["dof1"]] == p + 1 and ref["ok"][at["dof1"]] == 1 and not np.isnan(F_ref[0, at["dof1"]])
    assert not np.isnan(coef_ref[:, at["dof1"]]).any()
    if N >= 31:
        assert ref["ok"][at["level_missing"]] == 1 and ref["n"][at["level_missing"]] >= p + 1
        assert np.isnan(F_ref[0, at["level_missing"]]) and np.isnan(coef_ref[:, at["level_missing"]]).all()
        col = F_ref[:, at["level_sometimes"]]
        assert ref["ok"][at["level_sometimes"]] == 1 and not np.isnan(col[0]) and np.isnan(col[PLANTED_ROW]) and not np.isnan(col[PLANTED_ROW + 1:]).all()


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "no_mask"])
@pytest.mark.parametrize("p, k", SHAPES)
def test_f_coefficients_max_and_exceed_equal_the_restatement_to_the_bit(p, k, masked):
    batch = _batch(p, masked)
    for N in _knees(p):
        for V in VERTS:
            Y, mask, D, perm = _case(N, V, p, k, masked)
            ref, F_ref, coef_ref = _reference(N, V, p, k, masked)
            prep = _prepare_device(Y, mask, D, k)
            for P in _rows(_batch(p, masked)):
                F, coef0, f0, max_f, exceed = _device(prep, D, perm[:P], k, batch)
                where = f"N={N} V={V} P={P}"
                same_bits(F, F_ref[:P], f"{where} F")
                same_bits(coef0, coef_ref, f"{where} coef0")
                same_bits(f0, F_ref[0], f"{where} f0")
                want_max, want_exceed = gref.reduce_tiles(F_ref[:P])
                same_bits(max_f, want_max, f"{where} max_f")
                same_bits(exceed, want_exceed, f"{where} exceed")
            assert (F_ref[~np.isnan(F_ref)] >= 0.0).all()
            assert not np.isnan(F_ref[:, 0]).any() or N < 31                    # an ordinary vertex has an F in every row
            clamped = np.array(perm[1])
            clamped[0], clamped[N - 1] = 0, N - 1
            assert perm[1].min() < 0 and perm[1].max() >= N
            assert np.array_equal(F_ref[1], fref.regression_f(ref, mask, D, clamped[None, :], k)[0], equal_nan=True)
            if masked and V >= 8:
                _planted_cases_occur(N, V, p, k, ref, F_ref, coef_ref)


@pytest.mark.parametrize("p, k", SHAPES)
def test_no_mask_gives_the_bits_of_a_mask_of_all_ones(p, k):
    N, V = 33, 257
    Y, _, D, perm = _case(N, V, p, k, False)
    ref, F_ref, coef_ref = _reference(N, V, p, k, False)
    bare, full = _prepare_device(Y, None, D, k), _prepare_device(Y, np.ones((N, V), bool), D, k)
    assert bare.mask is None and full.mask is not None and (ref["n"] == N).all()
    for prep, batch, what in ((bare, _batch(p, False), "no mask"), (full, _batch(p, True), "all ones")):      # two kernels, two row groupings
        F, coef0, _, max_f, exceed = _device(prep, D, perm, k, batch)
        same_bits(F, F_ref, f"F ({what})")
        same_bits(coef0, coef_ref, f"coef0 ({what})")
        same_bits(max_f, gref.reduce_tiles(F_ref)[0], f"max_f ({what})")
        same_bits(exceed, gref.reduce_tiles(F_ref)[1], f"exceed ({what})")


# ---- one tested column: the F kernel against the t kernel ------------------------------------------------------------------------------
K1_N, K1_V, K1_P, K1_SEED = 33, 257, 40, 11
NEAR = 1e-9


@functools.lru_cache(maxsize=None)
def _k1_case(p):
    rng = np.random.default_rng([K1_SEED, p])
    i = np.arange(K1_N)
    cols = {2: [np.ones(K1_N)], 4: [np.ones(K1_N), (i % 2).astype(np.float64), 60 + 8 * rng.normal(size=K1_N)]}[p] + [rng.normal(size=K1_N)]
    D = np.ascontiguousarray(np.stack(cols, axis=1))
    Y = (2.0 + 0.5 * rng.normal(size=(K1_N, K1_V)) + 0.3 * D[:, -1:] * rng.random(K1_V)[None, :]).astype(np.float32)
    mask = rng.random((K1_N, K1_V)) >= 0.1
    perm = np.stack([np.arange(K1_N)] + [rng.permutation(K1_N) for _ in range(K1_P - 1)]).astype(np.int32)
    return Y, mask, D, perm


def _no_near_ties(values, axis):
    """No two entries along ``axis`` lie within NEAR relative of each other."""
    s = np.sort(values, axis=axis)
    lo, hi = np.take(s, range(0, s.shape[axis] - 1), axis=axis), np.take(s, range(1, s.shape[axis]), axis=axis)
    return bool(((hi - lo) > NEAR * hi).all())


@pytest.mark.parametrize("p", [2, 4])
def test_one_tested_column_agrees_with_the_t_kernel(p):
    from oai_analysis_2_amd import ops
    Y, mask, D, perm = _k1_case(p)
    t_ref = rref.regression_t(rref.prepare(Y, mask, D[:, :-1]), mask, D, perm)
    # the fixture is free of near-ties, so that the ranks below are defined beyond the rounding that separates F from t * t
    assert not np.isnan(t_ref).any() and _no_near_ties(np.abs(t_ref), 0) and _no_near_ties(np.abs(t_ref).max(axis=1), 0)
    prep = _prepare_device(Y, mask, D, 1)
    design, index = torch.from_numpy(D).cuda(), torch.from_numpy(perm).cuda()
    out = {}
    for name in ("t", "f"):
        first, max_abs = torch.empty(K1_V, dtype=torch.float64, device="cuda"), torch.empty(K1_P, dtype=torch.float64, device="cuda")
        exceed, row0 = torch.empty(K1_V, dtype=torch.int64, device="cuda"), torch.empty((1, K1_V), dtype=torch.float64, device="cuda")
        tiles = []
        for p0 in range(0, K1_P, 16):
            p1 = min(p0 + 16, K1_P)
            tile = (ops.regression_t(prep, design, index, p0, p1, slope0=row0[0]) if name == "t" else
                    ops.regression_f(prep, design, index, p0, p1, 1, coef0=row0))
            ops.permutation_reduce(tile, p0, first, max_abs, exceed)
            tiles.append(tile.clone())
        out[name] = [x.cpu().numpy() for x in (torch.cat(tiles), max_abs, exceed, row0[0])]
    (t, t_max, t_exceed, slope), (F, f_max, f_exceed, coef) = out["t"], out["f"]
    same_bits(t, t_ref, "t")
    rel = float(np.max(np.abs(F - t * t) / (t * t)))
    print(f"p = {p}: max relative distance of F from t * t {rel:.3g}")
    assert np.allclose(F, t * t, rtol=1e-12, atol=0) and np.allclose(coef, slope, rtol=1e-12, atol=0)
    assert np.array_equal(f_exceed, t_exceed) and np.array_equal(np.argsort(f_max), np.argsort(t_max))
    assert np.allclose(f_max, t_max * t_max, rtol=1e-12, atol=0)


def test_the_wrapper_refuses_what_the_kernel_would():
    from oai_analysis_2_amd import ops
    Y, mask, D, perm = _k1_case(4)
    prep = _prepare_device(Y, mask, D, 2)                                      # two nuisance columns
    design, index = torch.from_numpy(D).cuda(), torch.from_numpy(perm).cuda()
    for kwargs, words in ((dict(n_interest=0), "n_interest must be 1 .. 4"), (dict(n_interest=5), "n_interest must be 1 .. 4"),
                          (dict(n_interest=1), r"design must be float64 \[33, 3 .. 3\]"), (dict(n_interest=3), r"design must be float64 \[33, 5 .. 5\]"),
                          (dict(n_interest=2, p0=3, p1=3), "are not rows"), (dict(n_interest=2, p1=K1_P + 1), "are not rows"),
                          (dict(n_interest=2, coef0=torch.empty((1, K1_V), dtype=torch.float64, device="cuda")), r"coef0 must be float64 \[2, 257\]"),
                          (dict(n_interest=2, workspace=torch.empty(16, dtype=torch.uint8, device="cuda")), "workspace")):
        args = dict(p0=0, p1=4)
        args.update(kwargs)
        with pytest.raises((ValueError, RuntimeError), match=words):
            ops.regression_f(prep, design, index, **args)
    with pytest.raises(ValueError, match="perm must be int32"):
        ops.regression_f(prep, design, index[:, :-1], 0, 4, 2)


# ---- the public interface --------------------------------------------------------------------------------------------------------------
def _image(vec, kind):
    """Stands for the atlas' rasteriser."""
    return np.broadcast_to(np.asarray(vec, np.float32)[:12].reshape(3, 4), (3, 4))


N_E2E, P_E2E, F_CLUSTER = 24, 200, 8.0
LABELS = (2, 4, 9)                                                         # the labels of the three groups


@functools.lru_cache(maxsize=None)
def _painted(effect):
    """Three groups of 8 knees on the sphere: 2 mm + 0.2 mm noise + 0.01 mm per year of age over 60 everywhere; on the cap z > 0.8 the
    group labelled 4 is ``effect`` mm thicker and the group labelled 9 ``effect`` mm thinner than the group labelled 2.  10 % missing."""
    verts, _ = icosphere()
    cap, far = verts[:, 2] > 0.8, verts[:, 2] < 0.5
    rng = np.random.default_rng(2027)                                     # a draw without a family-wise false positive far from the cap (5 % have one)
    member = np.arange(N_E2E) % 3
    rng.shuffle(member)
    groups = np.asarray(LABELS)[member]
    age = rng.uniform(45, 80, N_E2E)
    Y = 2.0 + 0.2 * rng.normal(size=(N_E2E, len(verts))) + 0.01 * (age - 60)[:, None]
    Y[np.ix_(member == 1, cap)] += effect
    Y[np.ix_(member == 2, cap)] -= effect
    mask = rng.random(Y.shape) >= 0.1
    return np.where(mask, Y, 0.0).astype(np.float32), mask, groups, age, cap, far


def _restated(Y, mask, groups, age, index, threshold, atlas):
    """Every field of the FResult from the restatements: the F tile of tests/group_f_ref.py, the clusters of tests/group_stats_ref.py, the
    TFCE of tests/graph_tfce_ref.py, and the host's own ``_p_values`` and cluster bookkeeping on them."""
    from oai_analysis_2_amd import mesh_processing as mp, stats
    levels, dummies = fref.anova_dummies(groups)
    Z, D, scales = fref.design_matrix(dummies, age, True)
    prep = fref.prepare(Y, mask, Z)
    k, p, P = dummies.shape[1], D.shape[1], len(index)
    F, coef = fref.regression_f(prep, mask, D, index, k, with_coef=True)
    max_f, exceed = gref.reduce_tiles(F)
    p_unc, p_fwer = stats._p_values(F[0], max_f, exceed, P)
    dof2 = prep["n"].astype(np.int64) - p
    with np.errstate(invalid="ignore", divide="ignore"):
        eta2 = (k * F[0]) / (k * F[0] + dof2.astype(np.float64))
    off, nbr = sphere_graph()
    area = mp.mesh_areas(atlas.inner["FC"])[0]
    label, size, extent = gref.clusters(F, off, nbr, threshold)
    found = []
    for lab in np.unique(label[0][label[0] >= 0]):
        members = np.nonzero(label[0] == lab)[0]
        found.append(stats.Cluster(int(lab), 1, int(size[0][lab]), float(np.cumsum(area[members])[-1]), float((extent >= size[0][lab]).sum()) / float(P)))
    enhanced, clipped = tref.tfce(F, off, nbr, dh=0.1, E=1.0, H=2.0, weights=np.rint(area * 2 ** 20).astype(np.int64), unit=2.0 ** -20)
    max_tfce, tfce_exceed = gref.reduce_tiles(enhanced)
    p_tfce_unc, p_tfce = stats._p_values(enhanced[0], max_tfce, tfce_exceed, P)
    sides = [gref.prepare(Y[groups == lab], mask[groups == lab]) for lab in levels]
    return dict(f=F[0], n=prep["n"], dof1=k, dof2=dof2, coefficients=coef / scales[:, None], partial_eta2=eta2, p_uncorrected=p_unc, p_fwer=p_fwer,
                max_f=max_f, n_permutations=P, exact=False, levels=levels, group_n=np.stack([s["n"] for s in sides]),
                group_mean=np.stack([s["mean"] for s in sides]), cluster_threshold=threshold, cluster_label=label[0], clusters=found, max_extent=extent,
                tfce=enhanced[0], p_tfce=p_tfce, p_tfce_uncorrected=p_tfce_unc, max_tfce=max_tfce, tfce_clipped=int(np.count_nonzero(clipped)),
                tfce_settings=stats.TFCE(), kind="FC")


def test_anova_end_to_end_finds_the_painted_cap_and_equals_the_restatement():
    import dataclasses
    from oai_analysis_2_amd import stats
    Y, mask, groups, age, cap, far = _painted(0.3)
    atlas = sphere_atlas(image=_image)
    kwargs = dict(covariates=age, n_permutations=P_E2E, cluster_threshold=F_CLUSTER, seed=1, tfce=True)
    res = stats.anova_test(_cohort(atlas, Y, mask=mask, chunk=7), groups, batch=48, **kwargs)
    assert isinstance(res, stats.FResult) and res.n_permutations == P_E2E and not res.exact and res.dof1 == 2 and res.levels.tolist() == [2, 4, 9]
    want = _restated(Y, mask, groups, age, stats.index_permutations(N_E2E, P_E2E, seed=1).index, F_CLUSTER, atlas)
    same_result(res, want, "against the restatement")
    # what was painted is found: the corrected p inside the cap and nowhere at distance; the coefficients are differences from level 2
    assert (res.p_fwer[cap] <= 0.05).any() and not (res.p_fwer[far] <= 0.05).any() and not np.isnan(res.f).any()
    assert (res.p_tfce[cap] <= 0.05).any() and not (res.p_tfce[far] <= 0.05).any()
    assert all(c.sign == 1 for c in res.clusters) and res.clusters and res.max_f[0] == res.f.max()
    print(f"cap vertices (of {cap.sum()}) with p_fwer <= 0.05: {int((res.p_fwer[cap] <= 0.05).sum())}, p_tfce <= 0.05: {int((res.p_tfce[cap] <= 0.05).sum())}; "
          f"max F {res.f.max():.1f}, clipped {res.tfce_clipped}")
    assert np.abs(np.median(res.coefficients[0][cap]) - 0.3) < 0.1 and np.abs(np.median(res.coefficients[1][cap]) + 0.3) < 0.1
    # the descriptive side against plain numpy on the valid knees
    y = Y.astype(np.float64)
    for g, lab in enumerate(res.levels):
        rows = groups == lab
        assert np.array_equal(res.group_n[g], mask[rows].sum(axis=0)) and res.group_n.dtype == np.int32
        assert np.allclose(res.group_mean[g], (y[rows] * mask[rows]).sum(axis=0) / mask[rows].sum(axis=0), rtol=1e-13, atol=0)
    assert np.array_equal(res.n, res.group_n.sum(axis=0)) and np.array_equal(res.dof2, res.n.astype(np.int64) - 4)
    assert res.image(atlas, "f").shape == atlas.image(np.zeros(len(cap)), "FC").shape and res.image(atlas, "partial_eta2").dtype == np.float32
    # a linear score over the groups sees a weaker effect than the F: the painted means are not monotone in the label
    score = stats.regression_test(_cohort(atlas, Y, mask=mask, chunk=7), np.searchsorted(res.levels, groups).astype(np.float64), covariates=age,
                                  n_permutations=P_E2E, seed=1, batch=48)
    assert np.median(score.t[cap] ** 2) < np.median(res.f[cap])
    # a second run, another batch size and the rows handed over instead of drawn: the same bits in every field
    fields = {f.name: getattr(res, f.name) for f in dataclasses.fields(res)}
    perms = stats.index_permutations(N_E2E, P_E2E, seed=1)
    for other, what in ((stats.anova_test(_cohort(atlas, Y, mask=mask, chunk=7), groups, batch=48, **kwargs), "again"),
                        (stats.anova_test(_cohort(atlas, Y, mask=mask, chunk=7), groups, **kwargs), "default batch"),
                        (stats.anova_test(_cohort(atlas, Y, mask=mask, chunk=7), groups, covariates=age, cluster_threshold=F_CLUSTER, tfce=True, batch=37,
                                          permutations=perms.index), "batch 37")):
        same_result(other, fields, what)
    # f_test on the same dummies is the same test, without the descriptive side
    plain = stats.f_test(_cohort(atlas, Y, mask=mask, chunk=7), fref.anova_dummies(groups)[1], covariates=age, n_permutations=P_E2E, seed=1, batch=48)
    for name in ("f", "coefficients", "partial_eta2", "p_fwer", "p_uncorrected", "max_f", "n", "dof2"):
        same_bits(getattr(plain, name), getattr(res, name), f"f_test: {name}")
    assert plain.levels is None and plain.group_n is None and plain.group_mean is None and plain.tfce is None and plain.cluster_label is None


def test_without_an_effect_the_corrected_p_is_the_rank_of_the_observed_maximum():
    from oai_analysis_2_amd import stats
    Y, mask, groups, age, _, _ = _painted(0.0)
    res = stats.anova_test(_cohort(sphere_atlas(image=_image), Y, mask=mask, chunk=7), groups, covariates=age, n_permutations=P_E2E, seed=2, batch=64)
    assert not np.isnan(res.f).any() and res.cluster_label is None and res.clusters == [] and res.tfce is None
    assert (res.p_fwer >= res.p_uncorrected).all()
    assert res.p_fwer.min() == (res.max_f >= res.max_f[0]).sum() / P_E2E
    assert res.max_f[0] == res.f.max() and (res.f >= 0).all()
