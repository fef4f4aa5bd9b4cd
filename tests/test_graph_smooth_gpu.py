"""GPU: surface smoothing (csrc/graph_smooth.hip) against its numpy restatement (tests/graph_smooth_ref.py), to the bit -- every float64 is
the result of IEEE multiply, add and divide in a stated order -- and ``ThicknessCohort.smoothed`` / ``SurfaceSmoother`` of
oai_analysis_2_amd.stats end to end on a small sphere."""
import functools

import numpy as np
import pytest
import torch

import graph_smooth_ref as sref
import group_stats_ref as gref
from cohort_cases import cohort as _cohort, dev, icosphere, same_bits, sphere_atlas, sphere_graph

pytestmark = pytest.mark.gpu

GARBAGE = np.array([np.nan, np.inf, 1e300])         # written under every 0 mask bit of the input: none of it may show in the output


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(offsets, neighbours) on the host; the sphere's are those of ``mesh_processing.vertex_adjacency_device``."""
    if name == "path_3000":
        return sref.path_graph(3000)
    if name == "star_700":                            # a hub whose degree exceeds any unroll and any wave
        return sref.star_graph(700)
    if name == "odd_40":
        # isolated vertices (0, 13, 39), a vertex among its own neighbours, one neighbour out of range, one negative, and a last offset
        # beyond the neighbour count: the kernel clamps the one and ignores the others
        rng = np.random.default_rng(40)
        lists = [[] if i in (0, 13, 39) else rng.choice(40, rng.integers(1, 9), replace=False).tolist() for i in range(40)]
        lists[5] = [5, 7, 41, 2]
        lists[6] = [-1, 8]
        off, nbr = sref.from_lists(lists)
        off[-1] += 5
        return off, nbr
    if name == "hostile_40":                          # odd_40's faults and a first offset below 0: the graph that the cluster and TFCE tests use
        off, nbr = gref.hostile_graph()
        assert off[0] < 0 and off[-1] > len(nbr) and (nbr < 0).any() and (nbr >= len(off) - 1).any() and 5 in nbr[off[5]:off[6]]
        return off, nbr
    return sphere_graph()


@functools.lru_cache(maxsize=None)
def _case(graph, R):
    """(values with garbage under the mask, clean values, mask, edge weights, self weights): 30 % missing at random; with five rows or
    more, row 1 is entirely missing and row 2 has one valid vertex; asymmetric edge weights and self weights, both with exact zeros."""
    off, nbr = _graph(graph)
    V = len(off) - 1
    rng = np.random.default_rng(1000 * R + V)
    clean = rng.normal(2.0, 0.5, (R, V))
    mask = (rng.random((R, V)) > 0.3).astype(np.uint8)
    if R >= 5:
        mask[1] = 0
        mask[2] = 0
        mask[2, V // 3] = 1
    dirty = np.where(mask != 0, clean, GARBAGE[np.arange(R * V).reshape(R, V) % 3])
    w = rng.uniform(0.0, 2.0, len(nbr))
    w[rng.random(len(nbr)) < 0.1] = 0.0
    sw = rng.uniform(0.0, 2.0, V)
    sw[rng.random(V) < 0.2] = 0.0
    for a in (dirty, clean, mask, w, sw):
        a.setflags(write=False)
    return dirty, clean, mask, w, sw


@pytest.mark.parametrize("R", [1, 5, 17, 33])
@pytest.mark.parametrize("graph", ["path_3000", "star_700", "odd_40", "hostile_40", "icosphere"])
def test_smoothing_equals_the_restatement_to_the_bit(graph, R):
    from oai_analysis_2_amd import ops
    off, nbr = _graph(graph)
    dirty, clean, mask, w, sw = _case(graph, R)
    off_d, nbr_d, w_d, sw_d = dev(off), dev(nbr), dev(w), dev(sw)
    dirty_d, clean_d, mask_d = dev(dirty), dev(clean), dev(mask)
    dropped = 0
    for K in (1, 2, 7):                               # both parities of the ping-pong
        for fill in (False, True):
            where = f"{graph} R={R} K={K} fill={fill}"
            want, want_m = sref.smooth(dirty, mask, off, nbr, w, sw, K, fill)
            got, got_m = ops.graph_smooth(dirty_d, off_d, nbr_d, w_d, mask=mask_d, self_weights=sw_d, sweeps=K, fill=fill)
            same_bits(got_m, want_m, where + " mask")
            same_bits(got, want, where + " values")
            out = got.cpu().numpy()
            assert np.isfinite(out).all() and np.abs(out).max() < 10.0, where          # nothing of what lay under a 0 mask bit
            assert (out[want_m == 0] == 0).all() and not np.signbit(out[want_m == 0]).any(), where
            if not fill:
                assert not (want_m & (1 - mask)).any()
                dropped += int((mask & (1 - want_m)).sum())                             # valid, self weight 0, no valid neighbour that weighs
    assert dropped > 0 or graph not in ("path_3000", "star_700"), f"{graph} R={R}: no valid entry dropped out"
    # null self weights; null mask (on the clean values: everything is valid); both
    for mask_h, mask_t, values_h, values_t, sw_h, sw_t in ((mask, mask_d, dirty, dirty_d, None, None), (None, None, clean, clean_d, sw, sw_d),
                                                           (None, None, clean, clean_d, None, None)):
        for fill in (False, True):
            want, want_m = sref.smooth(values_h, mask_h, off, nbr, w, sw_h, 2, fill)
            got, got_m = ops.graph_smooth(values_t, off_d, nbr_d, w_d, mask=mask_t, self_weights=sw_t, sweeps=2, fill=fill)
            where = f"{graph} R={R} mask={'yes' if mask_h is not None else 'null'} self={'yes' if sw_h is not None else 'null'} fill={fill}"
            same_bits(got_m, want_m, where + " mask")
            same_bits(got, want, where + " values")


def test_a_valid_nan_propagates_and_an_invalid_one_does_not():
    from oai_analysis_2_amd import ops
    off, nbr = sref.path_graph(9)
    x = np.arange(9, dtype=np.float64)[None, :].repeat(2, axis=0)
    x[:, 4] = np.nan
    mask = np.ones((2, 9), np.uint8)
    mask[1, 4] = 0
    w = np.ones(len(nbr))
    want, want_m = sref.smooth(x, mask, off, nbr, w, None, 2, False)
    got, got_m = ops.graph_smooth(dev(x), dev(off), dev(nbr), dev(w), mask=dev(mask), sweeps=2)
    same_bits(got, want, "values")
    same_bits(got_m, want_m, "mask")
    assert np.isnan(want[0, 2:7]).all() and not np.isnan(want[0, :2]).any() and not np.isnan(want[1]).any() and want_m[1, 4] == 0


def test_fill_grows_the_valid_set_by_one_ring_per_sweep():
    from oai_analysis_2_amd import ops
    off, nbr = sref.path_graph(101)
    x = np.full((1, 101), np.nan)
    x[0, 50] = 3.0
    mask = np.zeros((1, 101), np.uint8)
    mask[0, 50] = 1
    args = (dev(x), dev(off), dev(nbr), dev(np.ones(len(nbr))))
    filled, filled_m = ops.graph_smooth(*args, mask=dev(mask), sweeps=7, fill=True)
    kept, kept_m = ops.graph_smooth(*args, mask=dev(mask), sweeps=7, fill=False)
    assert int(filled_m.sum()) == 15 and filled_m[0, 43:58].all() and int(kept_m.sum()) == 1 and kept_m[0, 50] == 1
    assert kept[0, 50] == 3.0 and (filled[0, 43:58] == 3.0).all() and float(filled.abs().sum()) == 45.0
    same_bits(filled, sref.smooth(x, mask, off, nbr, np.ones(len(nbr)), None, 7, True)[0], "filled")


def test_in_place_row_by_row_and_twice_give_the_same_bits():
    from oai_analysis_2_amd import ops
    off, nbr = _graph("icosphere")
    dirty, _, mask, w, sw = _case("icosphere", 17)
    off_d, nbr_d, w_d, sw_d = dev(off), dev(nbr), dev(w), dev(sw)
    for fill in (False, True):
        kwargs = dict(self_weights=sw_d, sweeps=3, fill=fill)
        ref, ref_m = ops.graph_smooth(dev(dirty), off_d, nbr_d, w_d, mask=dev(mask), **kwargs)
        ref, ref_m = ref.cpu().numpy(), ref_m.cpu().numpy()
        again, again_m = ops.graph_smooth(dev(dirty), off_d, nbr_d, w_d, mask=dev(mask), **kwargs)
        same_bits(again, ref, "second run")
        same_bits(again_m, ref_m, "second run mask")
        values_d, mask_d = dev(dirty), dev(mask)
        got, got_m = ops.graph_smooth(values_d, off_d, nbr_d, w_d, mask=mask_d, out=values_d, out_mask=mask_d, **kwargs)
        assert got.data_ptr() == values_d.data_ptr() and got_m.data_ptr() == mask_d.data_ptr()
        same_bits(values_d, ref, "in place")
        same_bits(mask_d, ref_m, "in place mask")
        values_d, mask_d = dev(dirty), dev(mask)
        for r in range(len(dirty)):                                        # every row as a tile of its own
            got, got_m = ops.graph_smooth(values_d[r:r + 1], off_d, nbr_d, w_d, mask=mask_d[r:r + 1], **kwargs)
            same_bits(got, ref[r:r + 1], f"row {r} alone")
            same_bits(got_m, ref_m[r:r + 1], f"row {r} alone, mask")


def test_atlas_scale_path():
    """The one case above toy size: R * V = 480 032 elements on a path as long as the atlas mesh has vertices."""
    from oai_analysis_2_amd import ops
    V, R, K = 30002, 16, 4
    off, nbr = sref.path_graph(V)
    rng = np.random.default_rng(30002)
    x = rng.normal(2.0, 0.5, (R, V))
    mask = (rng.random((R, V)) > 0.3).astype(np.uint8)
    x[mask == 0] = np.nan
    w = rng.uniform(0.0, 2.0, len(nbr))
    for fill in (False, True):
        want, want_m = sref.smooth(x, mask, off, nbr, w, None, K, fill)
        got, got_m = ops.graph_smooth(dev(x), dev(off), dev(nbr), dev(w), mask=dev(mask), sweeps=K, fill=fill)
        same_bits(got_m, want_m, f"fill={fill} mask")
        same_bits(got, want, f"fill={fill} values")


def test_the_wrapper_refuses_what_the_kernel_would():
    from oai_analysis_2_amd import ops
    off, nbr = (dev(a) for a in sref.path_graph(10))
    tile = torch.zeros((2, 10), dtype=torch.float64, device="cuda")
    w = torch.ones(18, dtype=torch.float64, device="cuda")
    for kwargs, match in ((dict(sweeps=0), "sweeps"), (dict(sweeps=4097), "sweeps"),
                          (dict(self_weights=torch.zeros(9, dtype=torch.float64, device="cuda")), "self_weights must be"),
                          (dict(mask=torch.zeros((2, 9), dtype=torch.uint8, device="cuda")), "mask must have"),
                          (dict(out=torch.zeros((2, 9), dtype=torch.float64, device="cuda")), "out must be"),
                          (dict(out_mask=torch.zeros((2, 10), dtype=torch.int32, device="cuda")), "out_mask must be")):
        with pytest.raises(ValueError, match=match):
            ops.graph_smooth(tile, off, nbr, w, **kwargs)
    with pytest.raises(ValueError, match="edge_weights must be"):
        ops.graph_smooth(tile, off, nbr, w[:17])
    with pytest.raises(Exception, match="float64"):
        ops.graph_smooth(tile.float(), off, nbr, w)


# ---- the public interface --------------------------------------------------------------------------------------------------------------
N_E2E, FWHM_E2E = 24, 15.0


@functools.lru_cache(maxsize=None)
def _knees():
    """24 float32 knees on the sphere with 10 % of the entries missing (NaN)."""
    V = len(icosphere()[0])
    rng = np.random.default_rng(2025)
    Y = (2.0 + 0.3 * rng.normal(size=(N_E2E, V))).astype(np.float32)
    Y[rng.random((N_E2E, V)) < 0.1] = np.nan
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def _restated(missing):
    """(float32 values with 0 where missing, uint8 mask, sweeps) of the restatement, with the host helpers' weights and sweep count."""
    from oai_analysis_2_amd import stats
    off, nbr = _graph("icosphere")
    verts = icosphere()[0] * np.float32(40.0)
    sigma_step = stats.mean_edge_length(verts, off, nbr)
    w = stats.surface_edge_weights(verts, off, nbr, sigma_step)
    s = stats.surface_step_variance(off, nbr, w, stats.surface_edge_d2(verts, off, nbr))
    K = stats.sweeps_for_fwhm(FWHM_E2E, s)
    Y = _knees()
    x, m = sref.smooth(np.nan_to_num(Y.astype(np.float64)), ~np.isnan(Y), off, nbr, w, None, K, missing == "fill")
    return x.astype(np.float32), m, K, sigma_step, float(s.mean())


def test_a_smoothed_cohort_is_the_restatement_and_the_tests_take_it():
    from oai_analysis_2_amd import stats
    atlas, Y = sphere_atlas(scale=40.0), _knees()
    cohort = _cohort(atlas, Y, [f"knee-{i}" for i in range(len(Y))])
    before, before_m = cohort.values.clone(), cohort.mask.clone()
    for missing in ("keep", "fill"):
        want, want_m, K, sigma_step, s_mean = _restated(missing)
        assert K >= 2
        smooth = cohort.smoothed(fwhm_mm=FWHM_E2E, missing=missing)
        same_bits(smooth.mask, want_m, f"{missing} mask")
        same_bits(smooth.values, want, f"{missing} values")
        assert smooth.ids == cohort.ids and smooth.kind == "FC" and smooth.atlas is atlas and len(smooth) == N_E2E
        assert smooth.smoothing == stats.Smoothing(FWHM_E2E, np.sqrt(8 * np.log(2) * K * s_mean / 2), K, sigma_step, missing)
        assert smooth.smoothing.sweeps == K and abs(smooth.smoothing.achieved_fwhm_mm / FWHM_E2E - 1) < 0.25 and cohort.smoothing is None
        assert torch.equal(cohort.values, before) and torch.equal(cohort.mask, before_m)
        assert smooth.surface_graph()[0].data_ptr() == cohort.surface_graph()[0].data_ptr()
        if missing == "keep":
            assert np.array_equal(want_m != 0, ~np.isnan(Y))
        else:
            assert want_m.all()
    # batches of seven knees: the same bits
    want, want_m, K, _, _ = _restated("keep")
    assert stats.smoothing_batch(cohort.n_verts, N_E2E, 7 * cohort.n_verts * stats._SMOOTH_BYTES) == 7
    small = cohort.smoothed(fwhm_mm=FWHM_E2E, batch=7)
    same_bits(small.values, want, "batches of seven, values")
    same_bits(small.mask, want_m, "batches of seven, mask")
    # the smoothed cohort goes into the test as it is
    smooth = cohort.smoothed(sweeps=K)
    same_bits(smooth.values, want, "by sweeps")
    assert smooth.smoothing.fwhm_mm is None and smooth.smoothing.sweeps == K
    groups = np.arange(N_E2E) < N_E2E // 2
    res = stats.two_sample_test(smooth, groups, n_permutations=50, seed=4)
    t_ref = gref.permutation_t(gref.prepare(want, want_m), want_m, stats.label_permutations(groups, 50, seed=4).rows(), gref.TWO_SAMPLE)
    same_bits(res.t, t_ref[0], "t of the smoothed cohort")
    # smoothing does what it is for: the noise per vertex falls
    assert smooth.summary()["std"].mean() < 0.7 * cohort.summary()["std"].mean()


def test_the_smoother_on_vectors_matrices_and_an_impulse():
    from oai_analysis_2_amd import stats
    atlas, Y = sphere_atlas(scale=40.0), _knees()
    want, want_m, K, sigma_step, _ = _restated("keep")
    smoother = stats.SurfaceSmoother(atlas, "FC", FWHM_E2E)
    assert smoother.sweeps == K and smoother.sigma_step == sigma_step and smoother.fwhm_mm == FWHM_E2E
    one = smoother(Y[3])                                                   # one numpy vector with NaNs: NaN at the same places in keep mode
    assert isinstance(one, np.ndarray) and one.dtype == np.float32 and one.shape == Y[3].shape
    assert np.array_equal(np.isnan(one), np.isnan(Y[3]))
    same_bits(np.nan_to_num(one), want[3], "one vector")
    many = smoother(torch.from_numpy(Y.astype(np.float64)).cuda())        # a float64 device matrix: not rounded to float32
    assert isinstance(many, torch.Tensor) and many.is_cuda and many.dtype == torch.float64 and tuple(many.shape) == Y.shape
    assert np.array_equal(np.isnan(many.cpu().numpy()), np.isnan(Y))
    same_bits(np.nan_to_num(many.cpu().numpy()).astype(np.float32), want, "matrix")
    valid = np.ones(Y.shape[1], np.uint8)
    valid[:100] = 0
    assert np.isnan(smoother(Y[3], valid=valid)[:100]).all()
    filler = stats.SurfaceSmoother(atlas, "FC", sweeps=K, missing="fill")
    assert not np.isnan(filler(Y[3])).any() and filler.fwhm_mm is None and filler.achieved_fwhm_mm > 0
    for v in (0, 345):
        kernel = smoother.impulse(v)
        assert kernel.dtype == np.float64 and kernel.shape == (Y.shape[1],) and abs(kernel.sum() - 1.0) < 1e-12
        assert kernel[v] > 0 and 1 < np.count_nonzero(kernel) < len(kernel) and (kernel >= 0).all()
    with pytest.raises(ValueError, match="vertex"):
        smoother.impulse(len(valid))
    with pytest.raises(ValueError, match="field must be"):
        smoother(Y[3][:-1])
