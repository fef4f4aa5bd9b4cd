"""GPU: the normative deviation (csrc/normative.hip) against its numpy restatement (tests/normative_ref.py), to the bit -- every float64 is
the result of IEEE add, subtract, multiply, divide and sqrt in a stated order, every count and area an integer -- and
``stats.NormativeModel`` / ``dask_processing.deviation_stream`` end to end on the small sphere of the longitudinal tests."""
import functools

import numpy as np
import pytest
import torch

import normative_ref as nref
from cohort_cases import dev, icosphere, same_bits, sphere_atlas

pytestmark = pytest.mark.gpu

MODEL = ("gamma", "L", "rss", "n", "ok")
Z0 = 1.5


@functools.lru_cache(maxsize=None)
def _case(V, N, p, with_mask=True):
    case = nref.hostile_case(1000 * p + 10 * N + V, V, N, p, with_mask)
    for a in case:
        if a is not None:
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _want(V, N, p, with_mask=True):
    """The restatement of a case, once: the model, (z, diff) of the reference's own rows for both loo values, their summaries."""
    Y, mask, Z = _case(V, N, p, with_mask)
    model = nref.fit(Y, mask, Z)
    scored = {loo: nref.score(model, Y, mask, Z, loo) for loo in (0, 1)}
    weight = (np.arange(V, dtype=np.int64) * 7919) % 1000 + 1
    return model, scored, {loo: nref.summary(scored[loo][0], Z0, weight) for loo in (0, 1)}, weight


def _fit(V, N, p, with_mask=True):
    from oai_analysis_2_amd import ops
    Y, mask, Z = _case(V, N, p, with_mask)
    return ops.normative_fit(dev(Y), dev(Z), dev(mask))


@pytest.mark.parametrize("p", [1, 3, 6])
@pytest.mark.parametrize("V", [1, 63, 65, 257])
def test_fit_score_and_summary_equal_the_restatement_to_the_bit(V, p):
    from oai_analysis_2_amd import ops
    for N in (p + 2, 24):
        Y, mask, Z = _case(V, N, p)
        model, scored, summaries, weight = _want(V, N, p)
        got = _fit(V, N, p)
        for name in MODEL:
            same_bits(getattr(got, name), model[name], f"V={V} N={N} p={p} {name}")
        for loo in (0, 1):
            diff = torch.empty((N, V), dtype=torch.float64, device="cuda")
            z = ops.normative_score(got, dev(Y), dev(Z), dev(mask), loo=bool(loo), diff=diff)
            same_bits(z, scored[loo][0], f"V={V} N={N} p={p} loo={loo} z")
            same_bits(diff, scored[loo][1], f"V={V} N={N} p={p} loo={loo} diff")
            stats, counts = ops.deviation_summary(z, Z0, dev(weight))
            same_bits(stats, summaries[loo][0], f"V={V} N={N} p={p} loo={loo} stats")
            same_bits(counts, summaries[loo][1], f"V={V} N={N} p={p} loo={loo} counts")
        if V >= 63:
            # every reason for a NaN is there, by the restatement alone (p = 1 admits no lone design direction)
            found = nref.nan_classes(Y, mask, Z)
            assert found["nothing"] >= 1 and found["loo_dof"] >= 1 and found["s2"] >= 1 and found["pivot"] >= 1, found
            assert p == 1 or (found["den"] >= 1 and found["pivot_alone"] >= 1), found
            valid = ~np.isnan(scored[0][0])
            assert valid.any() and np.abs(scored[0][0][valid]).max() < 1e6                      # and the rest is no garbage (3e38 lies under the mask)


@pytest.mark.parametrize("p", [1, 3, 6])
def test_without_a_mask_and_a_null_mask_is_a_mask_of_ones(p):
    from oai_analysis_2_amd import ops
    V, N = 65, 24
    Y, _, Z = _case(V, N, p, False)
    model, scored, _, _ = _want(V, N, p, False)
    ones = torch.ones((N, V), dtype=torch.uint8, device="cuda")
    bare, masked = ops.normative_fit(dev(Y), dev(Z)), ops.normative_fit(dev(Y), dev(Z), ones)
    for name in MODEL:
        same_bits(getattr(bare, name), model[name], f"no mask {name}")
        same_bits(getattr(masked, name), model[name], f"ones {name}")
    for loo in (0, 1):
        same_bits(ops.normative_score(bare, dev(Y), dev(Z), loo=bool(loo)), scored[loo][0], f"no mask loo={loo}")
        same_bits(ops.normative_score(masked, dev(Y), dev(Z), ones, loo=bool(loo)), scored[loo][0], f"ones loo={loo}")


@pytest.mark.parametrize("loo", [0, 1])
def test_row_groups_with_a_ragged_last_group(loo):
    from oai_analysis_2_amd import ops
    V, N, p = 257, 24, 3
    R = ops.NORMATIVE_SCORE_ROWS
    assert R + 1 <= N
    Y, mask, Z = _case(V, N, p)
    _, scored, _, _ = _want(V, N, p)
    model = _fit(V, N, p)
    for rows in (1, R, R + 1):
        # without diff, into a caller's workspace that is larger than needed and filled with a pattern: nothing is written past the tile
        ws = torch.full((rows * V * 8 + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
        z = ops.normative_score(model, dev(Y[:rows]), dev(Z[:rows]), dev(mask[:rows]), loo=bool(loo), workspace=ws)
        same_bits(z, scored[loo][0][:rows], f"rows={rows} loo={loo}")
        assert bool((ws[rows * V * 8:] == 0xAB).all())
    # rows taken from the middle: the design row and the values of a row travel together
    some = [5, 2, 23, 0, 11, 7, 7, 19, 3, 14]
    z = ops.normative_score(model, dev(Y[some]), dev(Z[some]), dev(mask[some]), loo=bool(loo))
    same_bits(z, scored[loo][0][some], f"picked rows loo={loo}")


def test_two_runs_give_identical_bits():
    from oai_analysis_2_amd import ops
    V, N, p = 257, 24, 6
    Y, mask, Z = _case(V, N, p)
    _, _, _, weight = _want(V, N, p)
    runs = []
    for _ in range(2):
        model = _fit(V, N, p)
        z = ops.normative_score(model, dev(Y), dev(Z), dev(mask), loo=True)
        runs.append([getattr(model, name).cpu().numpy() for name in MODEL] + [z.cpu().numpy()] + [t.cpu().numpy() for t in ops.deviation_summary(z, Z0, dev(weight))])
    for a, b in zip(*runs):
        same_bits(a, b, "second run")


def test_the_summary_breaks_ties_towards_the_smallest_vertex_and_spans_many_blocks():
    from oai_analysis_2_amd import ops
    V = 5000                                                               # five partial records per row
    rng = np.random.default_rng(9)
    tile = rng.normal(size=(4, V))
    tile[0, [4100, 77, 2600]] = [-6.0, 6.0, 6.0]                           # a tie of |z| across blocks and signs: vertex 77
    tile[1] = np.nan                                                       # a row without a score
    tile[2, rng.random(V) < 0.3] = np.nan
    tile[3] = 0.0
    weight = rng.integers(0, 1 << 21, V).astype(np.int64)
    for w in (weight, None):
        want = nref.summary(tile, 2.0, w)
        stats, counts = ops.deviation_summary(dev(tile), 2.0, dev(w))
        same_bits(stats, want[0], "stats")
        same_bits(counts, want[1], "counts")
    assert want[1][0, 1] == 77 and want[1][1, 1] == -1 and want[1][3, 1] == 0


def test_the_wrappers_refuse_what_the_kernels_would():
    from oai_analysis_2_amd import ops
    V, N, p = 63, 24, 3
    Y, mask, Z = (dev(a) for a in _case(V, N, p))
    model = ops.normative_fit(Y, Z, mask)
    with pytest.raises(ValueError, match="design must be"):
        ops.normative_fit(Y, Z[:-1], mask)
    with pytest.raises(ValueError, match="design must be"):
        ops.normative_fit(Y, torch.cat([Z, Z, Z], dim=1), mask)
    with pytest.raises(ValueError, match="mask must have"):
        ops.normative_fit(Y, Z, mask[:, :5])
    with pytest.raises(ValueError, match="design_rows must be"):
        ops.normative_score(model, Y[:4], Z[:4, :2])
    with pytest.raises(ValueError, match="values must be"):
        ops.normative_score(model, Y[:, :5], Z)
    with pytest.raises(ValueError, match="z_threshold"):
        ops.deviation_summary(torch.zeros((2, V), dtype=torch.float64, device="cuda"), 0.0)
    with pytest.raises(ValueError, match="weights must be"):
        ops.deviation_summary(torch.zeros((2, V), dtype=torch.float64, device="cuda"), 2.0, torch.ones(V - 1, dtype=torch.int64, device="cuda"))
    with pytest.raises(Exception, match="float32"):
        ops.normative_fit(Y.double(), Z, mask)


# ---- the public interface --------------------------------------------------------------------------------------------------------------
N_REF, PATCH_MM = 30, 0.6


def _image(vector, kind):
    """Stands for the atlas' rasteriser."""
    return kind, vector


@functools.lru_cache(maxsize=None)
def _study():
    """Thirty reference knees on the sphere: 2.5 mm, less 0.01 mm per year of age above 60, 0.1 mm of noise, 5 % of the entries missing
    (NaN); and one new knee of 70 years with the model's expectation, 0.05 mm of noise and a painted patch of -0.6 mm on the cap z > 0.8.
    Returns (Y float32 [N, V], covariates [N, 2], the new knee float32 [V], its covariates [2], cap)."""
    verts, _ = icosphere(2)
    rng = np.random.default_rng(21)
    age, sex = rng.normal(60.0, 9.0, N_REF), (np.arange(N_REF) % 2).astype(np.float64)
    Y = 2.5 - 0.01 * (age[:, None] - 60.0) + 0.1 * rng.normal(size=(N_REF, len(verts)))
    Y = Y.astype(np.float32)
    Y[rng.random(Y.shape) < 0.05] = np.nan
    cap = verts[:, 2] > 0.8
    knee = 2.5 - 0.01 * (70.0 - 60.0) + 0.05 * rng.normal(size=len(verts))
    knee[cap] -= PATCH_MM
    Y.setflags(write=False)
    return Y, np.stack([age, sex], axis=1), knee.astype(np.float32), np.array([70.0, 1.0]), cap


def _reference_cohort():
    from oai_analysis_2_amd import stats
    Y = _study()[0]
    cohort = stats.ThicknessCohort(sphere_atlas(level=2, image=_image), "FC", chunk=7)
    for i, row in enumerate(Y):
        cohort.add_vector(np.array(row), f"ref{i:02d}")
    return cohort


def test_a_painted_patch_is_found_scored_and_ranked(tmp_path):
    from oai_analysis_2_amd import dask_processing, stats
    from oai_analysis_2_amd.thickness import KneeThickness
    Y, cov, knee, knee_cov, cap = _study()
    cohort = _reference_cohort()
    model = stats.NormativeModel.fit(cohort, cov, names=["age", "sex"])
    # the restatement of everything, from the same design
    design = stats._design_rows(cov, True, model.means, model.scales)
    same_bits(np.ascontiguousarray(model.design), design, "design")
    mask = (~np.isnan(Y)).astype(np.uint8)
    fitted = nref.fit(np.nan_to_num(Y), mask, design)
    for name in MODEL:
        same_bits(getattr(model.block, name), fitted[name], name)
    areas = stats.tfce_weights(cohort.vertex_areas())

    # the members themselves
    members = model.loo(return_maps=True)
    z_loo, diff_loo = nref.score(fitted, np.nan_to_num(Y), mask, design, 1)
    same_bits(members.z, z_loo, "loo z")
    same_bits(members.diff_mm, diff_loo, "loo diff")
    stats_loo, counts_loo = nref.summary(z_loo, 2.0, areas)
    same_bits(members.max_abs, np.ascontiguousarray(stats_loo[:, 0]), "loo max_abs")
    assert np.array_equal(members.n_below, counts_loo[:, 2]) and np.array_equal(members.max_vertex, counts_loo[:, 1])
    assert members.ids == cohort.ids and members.loo and len(members) == N_REF and (members.dof == fitted["n"].astype(np.int64) - 3 - 1).all()
    same_bits(members.p_max, nref.rank_p(stats_loo[:, 0], stats_loo[:, 0], member=True), "loo p_max")
    assert members.p_max.min() == 1.0 / N_REF and members.p_max.max() == 1.0
    bare = model.loo()
    assert bare.z is None and np.array_equal(bare.max_abs, members.max_abs) and np.array_equal(bare.max_extent, members.max_extent)
    # a healthy reference: nobody's map is far out
    assert 2.0 < np.median(members.max_abs) < 5.0 and members.max_extent.max() < cap.sum()

    # the new knee
    res = model.deviation(knee, covariates=knee_cov, return_maps=True)
    row = model.rows(knee_cov, 1)
    z_new, diff_new = nref.score(fitted, knee[None, :], None, row, 0)
    same_bits(res.z, z_new, "z")
    same_bits(res.diff_mm, diff_new, "diff")
    stats_new, counts_new = nref.summary(z_new, 2.0, areas)
    below = z_new[0] < -2.0
    assert (below[cap]).all() and below.sum() < cap.sum() + 6              # the patch, and next to nothing else
    assert res.n_below[0] == counts_new[0, 2] == below.sum() and res.n_valid[0] == len(knee)
    assert res.area_below_mm2[0] == float(areas[below].sum()) * 2.0 ** -20 and int(counts_new[0, 3]) == int(areas[below].sum())
    assert abs(res.area_below_mm2[0] - cohort.vertex_areas()[below].sum()) < 1e-3
    same_bits(res.max_abs, np.ascontiguousarray(stats_new[:, 0]), "max_abs")
    assert cap[res.max_vertex[0]] and res.max_z[0] < 5.0 and res.min_z[0] == -res.max_abs[0]
    assert np.nanmedian(res.diff_mm[0][cap]) < -0.5 * PATCH_MM and abs(np.nanmedian(res.diff_mm[0][~cap])) < 0.05
    # the patch is the largest cluster, and the p-values are the host rank formula against the members' statistics
    found = res.clusters(0)
    largest = max(found, key=lambda c: c.extent)
    assert largest.sign == -1 and largest.extent == res.max_extent[0] >= cap.sum() and cap[largest.label]
    assert set(np.nonzero(cap)[0]) <= set(np.nonzero(below)[0])
    same_bits(res.p_max, nref.rank_p(stats_new[:, 0], stats_loo[:, 0]), "p_max")
    same_bits(res.p_extent, nref.rank_p(res.max_extent, members.max_extent), "p_extent")
    same_bits(res.p_area_below, nref.rank_p(counts_new[:, 3], counts_loo[:, 3]), "p_area_below")
    assert res.p_max[0] == res.p_extent[0] == res.p_area_below[0] == 1.0 / (N_REF + 1) and largest.p_cluster == 1.0 / (N_REF + 1)
    valid = ~np.isnan(res.z)
    assert np.array_equal(np.isnan(res.p_uncorrected), ~valid) and (res.p_uncorrected[0][cap] < 0.05).all()
    assert res.image(model.atlas, "z")[0] == "FC" and not res.loo and res.ids == [0]
    # the expected map at the knee's covariates is what the deviation was taken from
    expected = model.predict(knee_cov)
    assert expected.shape == (1, len(knee)) and np.allclose(knee.astype(np.float64) - expected[0], res.diff_mm[0], rtol=0, atol=1e-12)

    # the stream yields the same numbers, cartilage by cartilage
    stream = [(7, KneeThickness(fc=knee, tc=np.zeros(3, np.float32))), (9, KneeThickness(fc=knee, tc=np.zeros(3, np.float32), errors={"FC": "no mesh"}))]
    out = list(dask_processing.deviation_stream(stream, {"FC": model}, {7: knee_cov, 9: knee_cov}))
    assert [i for i, _ in out] == [7, 9] and set(out[0][1]) == {"FC"}
    first, failed = out[0][1]["FC"], out[1][1]["FC"]
    for name in ("max_abs", "area_below_mm2", "n_below", "max_extent", "p_max", "p_extent", "p_area_below", "max_vertex"):
        assert np.array_equal(getattr(first, name), getattr(res, name)), name
    assert first.ids == [7] and failed.n_valid[0] == 0 and failed.max_abs[0] == 0.0 and failed.p_max[0] == 1.0 and failed.max_vertex[0] == -1

    # a model that was saved scores the knee as the fitted one does, and says what it cannot do
    path = tmp_path / "fc.npz"
    model.save(path)
    loaded = stats.NormativeModel.load(path, sphere_atlas(level=2, image=_image))
    again = loaded.deviation(knee, covariates=knee_cov)
    for name in ("max_abs", "area_below_mm2", "max_extent", "p_max", "p_extent", "p_area_below"):
        assert np.array_equal(getattr(again, name), getattr(res, name)), name
    with pytest.raises(ValueError, match="without the reference's statistics"):
        loaded.deviation(knee, covariates=knee_cov, z_threshold=3.0)
    with pytest.raises(ValueError, match="loo needs the model that was fitted"):
        loaded.loo()
    with pytest.raises(ValueError, match="covariates must hold"):
        model.deviation(knee)
    with pytest.raises(ValueError, match="too small"):
        few = stats.ThicknessCohort(sphere_atlas(level=2, image=_image), "FC")
        for i in range(4):
            few.add_vector(np.array(Y[i]), i)
        stats.NormativeModel.fit(few, cov[:4])
