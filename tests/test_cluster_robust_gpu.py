"""GPU: the cluster-robust kernels (csrc/cluster_robust.hip) against their numpy restatement (tests/cluster_robust_ref.py) -- the cluster
block, the t tile, slope0, se0, max |t| and the exceedance counts to the bit -- and oai_analysis_2_amd.stats.marginal_test end to end on a
small sphere.  Every float64 is the result of IEEE add / subtract / multiply / divide / sqrt in a stated order, so equality is exact.  The
fixtures are tests/cluster_robust_cases.py's; the check that at least half the vertices of every case have a finite t is
tests/test_cluster_robust_cpu.py's."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import cluster_robust_ref as cref
import group_regression_ref as rref
import group_stats_ref as gref
from cluster_robust_cases import COLUMNS, KINDS, VERTS, case, reference, rows_per_thread
from cohort_cases import bare_atlas, cohort as _cohort, dev, icosphere, restated_fields, same_bits, same_result, sphere_atlas

pytestmark = pytest.mark.gpu

BLOCK = ("R", "Q", "mean", "n", "ok", "H", "K", "U", "L", "c", "G", "okc")


def _prepare_device(Y, mask, D, offsets, centre):
    from oai_analysis_2_amd import ops
    return ops.cluster_prepare(dev(Y), dev(mask, np.uint8), dev(D), dev(offsets), centre=centre)


def _device(prep, flips, batch):
    """The tile of every flip row in batches of ``batch``, row 0's slope and standard error, and the running reduction."""
    from oai_analysis_2_amd import ops, stats
    P, V = flips.shape[0], prep.n_verts
    bits = dev(stats.pack_bits(flips).view(np.int32))
    t0, slope0, se0 = (torch.full((V,), 7.0, dtype=torch.float64, device="cuda") for _ in range(3))
    max_abs = torch.full((P,), -1.0, dtype=torch.float64, device="cuda")
    exceed = torch.full((V,), -5, dtype=torch.int64, device="cuda")            # garbage: the first batch must start it
    tiles = []
    for p0 in range(0, P, batch):
        p1 = min(p0 + batch, P)
        tile = ops.cluster_t(prep, bits, p0, p1, slope0=slope0, se0=se0)       # later batches must leave slope0 and se0 alone
        ops.permutation_reduce(tile, p0, t0, max_abs, exceed)
        tiles.append(tile.clone())
    return torch.cat(tiles), slope0, se0, t0, max_abs, exceed


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", COLUMNS)
def test_cluster_block_t_slope_se_max_and_exceed_equal_the_restatement_to_the_bit(p, kind):
    r = rows_per_thread(p)
    for V in VERTS:
        for masked in (True, False):
            Y, mask, D, offsets, flips = case(kind, V, p, masked)
            ref, t_ref, slope_ref, se_ref = reference(kind, V, p, masked)
            assert 2 * int(np.isfinite(t_ref).all(axis=0).sum()) >= V
            prep = _prepare_device(Y, mask, D, offsets, centre=p > 1)
            where = f"{kind} p={p} V={V} {'masked' if masked else 'no mask'}"
            for name in BLOCK:
                same_bits(getattr(prep, name), ref[name], f"{where} block.{name}")
            # one fewer and one more rows than a thread owns; then every row in batches that start in the middle of a row group
            for P, batch in ((r - 1, r - 1), (r + 1, r + 1), (len(flips), r + max(1, r // 4))):
                t, slope0, se0, t0, max_abs, exceed = _device(prep, flips[:P], batch)
                what = f"{where} P={P}"
                same_bits(t, t_ref[:P], f"{what} t")
                same_bits(slope0, slope_ref, f"{what} slope0")
                same_bits(se0, se_ref, f"{what} se0")
                same_bits(t0, t_ref[0], f"{what} t0")
                want_max, want_exceed = gref.reduce_tiles(t_ref[:P])
                same_bits(max_abs, want_max, f"{what} max_abs")
                same_bits(exceed, want_exceed, f"{what} exceed")


@pytest.mark.parametrize("p", COLUMNS)
def test_no_mask_gives_the_bits_of_a_mask_of_all_ones(p):
    V = 257
    Y, _, D, offsets, flips = case("word", V, p, False)
    ref, t_ref, slope_ref, se_ref = reference("word", V, p, False)
    bare = _prepare_device(Y, None, D, offsets, centre=p > 1)
    full = _prepare_device(Y, np.ones(Y.shape, bool), D, offsets, centre=p > 1)
    assert bare.mask is None and full.mask is not None and (ref["n"] == len(Y)).all()
    for prep, what in ((bare, "no mask"), (full, "all ones")):             # two prepare kernels, one t kernel
        for name in BLOCK:
            same_bits(getattr(prep, name), ref[name], f"block.{name} ({what})")
        t, slope0, se0, _, max_abs, exceed = _device(prep, flips, len(flips))
        same_bits(t, t_ref, f"t ({what})")
        same_bits(slope0, slope_ref, f"slope0 ({what})")
        same_bits(se0, se_ref, f"se0 ({what})")
        same_bits(max_abs, gref.reduce_tiles(t_ref)[0], f"max_abs ({what})")
        same_bits(exceed, gref.reduce_tiles(t_ref)[1], f"exceed ({what})")


def test_the_wrappers_refuse_what_the_library_would():
    from oai_analysis_2_amd import _lib, ops, stats
    Y, mask, D, offsets, flips = case("five", 65, 2, True)
    prep = _prepare_device(Y, mask, D, offsets, True)
    bits = dev(stats.pack_bits(flips).view(np.int32))
    with pytest.raises(ValueError, match="offsets must hold"):
        ops.cluster_prepare(dev(Y), None, dev(D), dev(offsets[:2]))
    with pytest.raises(ValueError, match=r"design must be float64 \[11, 1 .. 6\]"):
        ops.cluster_prepare(dev(Y), None, dev(D[:-1]), dev(offsets))
    with pytest.raises(ValueError, match="mask must have the values' shape"):
        ops.cluster_prepare(dev(Y), dev(mask[:, :-1], np.uint8), dev(D), dev(offsets))
    with pytest.raises(ValueError, match="are not rows of"):
        ops.cluster_t(prep, bits, 0, len(flips) + 1)
    with pytest.raises(ValueError, match="packed flip rows of the 5 clusters"):
        ops.cluster_t(prep, torch.cat([bits, bits], dim=1), 0, 2)
    with pytest.raises(ValueError, match=r"se0 must be float64 \[65\]"):
        ops.cluster_t(prep, bits, 0, 2, se0=torch.zeros(64, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="workspace must be a uint8 buffer"):
        ops.cluster_t(prep, bits, 0, 2, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.OaiError, match="must live on the GPU"):
        ops.cluster_prepare(torch.from_numpy(np.array(Y)), None, dev(D), dev(offsets))


# ---- the public interface --------------------------------------------------------------------------------------------------------------
E2E_SUBJECTS, E2E_P, T_CLUSTER = 20, 200, 3.0


@functools.lru_cache(maxsize=None)
def _painted_visits():
    """20 subjects with 2 .. 5 visits each on the sphere, rows in visit-major order (so the subjects' rows are NOT contiguous): 2 mm, a
    random intercept per subject (sd 0.05 mm), 0.05 mm noise, a loss of 0.01 mm / year everywhere and of 0.10 mm / year more on the cap
    z > 0.8 in group 1; a twentieth of the entries missing."""
    verts, _ = icosphere()
    cap = verts[:, 2] > 0.8
    rng = np.random.default_rng(2026)
    S, V = E2E_SUBJECTS, len(verts)
    n_visits = 2 + ((np.arange(S) // 2) % 4)
    group = (np.arange(S) % 2).astype(np.float64)
    intercept = 0.05 * rng.normal(size=(S, V))
    rows = [(s, k) for k in range(5) for s in range(S) if k < n_visits[s]]
    subject = np.array([s for s, _ in rows])
    years = np.array([k + 0.25 * (s % 3) for s, k in rows], np.float64)
    Y = 2.0 + intercept[subject] + 0.05 * rng.normal(size=(len(rows), V)) - 0.01 * years[:, None]
    Y[:, cap] -= 0.10 * (years * group[subject])[:, None]
    mask = rng.random(Y.shape) >= 0.05
    return Y.astype(np.float32), mask, subject, years, group, cap


def _restated_marginal(Y, mask, labels, x, cov, flips):
    from oai_analysis_2_amd import stats
    _, order, offsets = stats.cluster_rows(labels)
    _, D, scale = rref.design_columns(x, cov, True)
    block = cref.prepare(Y[order], mask[order], D[order], offsets, centre=True)
    t, slope0, se0 = cref.cluster_t(block, flips, with_row0=True)
    return block, t, slope0 / scale, se0 / scale


def _want(block, t, slope, se, atlas):
    want, max_abs = restated_fields(t, E2E_P, atlas, T_CLUSTER)
    want["n_bootstrap"] = want.pop("n_permutations")
    want.update(t=t[0], slope=slope, se=se, n=block["n"], n_clusters=block["G"], dof=block["G"].astype(np.int64) - 1, max_abs=max_abs)
    return want


def test_marginal_test_on_visits_and_on_paired_knees_end_to_end_equals_the_restatement():
    from oai_analysis_2_amd import stats
    Y, mask, subject, years, group, cap = _painted_visits()
    atlas = sphere_atlas()
    visits = stats.LongitudinalCohort(atlas, "FC", chunk=7)
    for i in range(len(Y)):
        visits.add_vector(Y[i], f"s{subject[i]:02d}", years[i], valid=mask[i])
    g = visits.per_row(group)                                              # per subject, in the order of ``subjects`` = s00, s01, ...
    assert np.array_equal(g, group[subject]) and np.array_equal(visits.years, years)
    x, cov = visits.years * g, np.stack([visits.years, g], axis=1)
    flips = stats.sign_flips(E2E_SUBJECTS, E2E_P, seed=3)
    kwargs = dict(covariates=cov, n_bootstrap=E2E_P, seed=3, cluster_threshold=T_CLUSTER, tfce=True)
    res = stats.marginal_test(visits, x, batch=48, **kwargs)
    block, t, slope, se = _restated_marginal(Y, mask, list(subject), x, cov, flips.rows())
    same_result(res, _want(block, t, slope, se, atlas), "marginal_test on visits against the restatement")
    assert not res.exact and res.n_bootstrap == E2E_P and (res.n_clusters[~np.isnan(res.t)] >= 2).all()
    # the painted loss: found at every cap vertex on its own, at most of them family-wise (the null of max |t| has a long tail at S = 20)
    assert (res.t[cap] < -T_CLUSTER).all() and (res.p_uncorrected[cap] <= 0.01).all() and np.median(res.p_fwer[cap]) == 1.0 / E2E_P
    assert (np.abs(res.slope[cap] + 0.10) < 0.04).all() and not (res.p_fwer[~cap] <= 0.05).any()
    big = min(res.clusters, key=lambda c: (c.sign, -c.extent))
    assert big.sign == -1 and (res.cluster_label[cap] == big.label).all() and big.p_cluster == 1.0 / E2E_P
    # the default batch, and the flips handed over: the same bits in every field
    fields = {f.name: getattr(res, f.name) for f in dataclasses.fields(res)}
    for other, what in ((stats.marginal_test(visits, x, **kwargs), "default batch"),
                        (stats.marginal_test(visits, x, covariates=cov, cluster_threshold=T_CLUSTER, tfce=True, flips=flips.rows(), batch=37), "flips, batch 37")):
        same_result(other, fields, what)
    # a plain cohort of paired knees: the two earliest rows of every subject as its left and right knee, clusters= by subject
    first = [i for i in range(len(Y)) if years[i] < 2.0]
    knees = _cohort(atlas, Y[first], mask=mask[first], chunk=7)
    labels = [int(subject[i]) for i in first]
    side = np.array([years[i] >= 1.0 for i in first], np.float64)
    xk = side * group[subject[first]]
    covk = np.stack([side, group[subject[first]]], axis=1)
    resk = stats.marginal_test(knees, xk, covariates=covk, clusters=labels, n_bootstrap=E2E_P, seed=3, cluster_threshold=T_CLUSTER, tfce=True, batch=64)
    blockk, tk, slopek, sek = _restated_marginal(Y[first], mask[first], labels, xk, covk, flips.rows())
    same_result(resk, _want(blockk, tk, slopek, sek, atlas), "marginal_test on paired knees against the restatement")
    assert (resk.n_clusters <= E2E_SUBJECTS).all() and resk.n_clusters.max() == E2E_SUBJECTS and resk.n.max() <= 2 * E2E_SUBJECTS


def test_exact_enumeration_of_three_clusters_runs_eight_rows():
    from oai_analysis_2_amd import stats
    Y, mask, D, offsets, _ = case("five", 65, 2, False)
    cohort = _cohort(bare_atlas(65), Y[:6], chunk=7)
    res = stats.marginal_test(cohort, D[:6, -1], clusters=["a", "b", "b", "b", "c", "a"], n_bootstrap=1000)
    assert res.exact and res.n_bootstrap == 8 and res.max_abs.shape == (8,) and (res.n_clusters == 3).all() and (res.dof == 2).all()
    block, t, slope, se = _restated_marginal(Y[:6], np.ones((6, 65), bool), ["a", "b", "b", "b", "c", "a"], D[:6, -1], None, stats.sign_flips(3, 1000).rows())
    same_bits(res.t, t[0], "t")
    same_bits(res.max_abs, gref.reduce_tiles(t)[0], "max_abs")
    assert np.isfinite(res.t).all()
