"""GPU: the cohort-statistics kernels (csrc/group_stats.hip) against their numpy restatement (tests/group_stats_ref.py) -- prepare, t
tile, max |t| and the exceedance counts to the bit, clusters to the element -- and oai_analysis_2_amd.stats end to end on a small
sphere.  Every float64 is the result of IEEE add / subtract / multiply / divide / sqrt in a stated order, so equality is exact."""
import functools

import numpy as np
import pytest
import torch

import group_stats_ref as gref
from cohort_cases import bare_atlas, cohort as _cohort, dev, icosphere, painted, path_graph, same_bits, sphere_atlas

pytestmark = pytest.mark.gpu

KNEES = (2, 4, 31, 33, 65, 130)                   # both sides of a label word (32), one, two and four words and a ragged last one
VERTS = (1, 63, 65, 257, 1500)                    # both sides of a wave (64) and of a block's 256 vertices, several blocks
BATCH = 20                                        # labellings per launch: one full row group of 16 and a ragged one of 4
ROWS = (1, 2, BATCH - 1, BATCH + 1, 2 * BATCH + 5)


@functools.lru_cache(maxsize=None)
def _case(N, V, two_sample, with_mask=True):
    """(Y, mask, rows): values with the corner cases of the header -- an emptied vertex, constant vertices, a vertex that keeps four
    knees (so that n1 = 1 in some labellings only) -- and labellings that include a lone knee and everybody."""
    rng = np.random.default_rng([N, V, int(two_sample)])
    Y = rng.normal(2.0 if two_sample else 0.1, 0.5, size=(N, V)).astype(np.float32)
    mask = rng.random((N, V)) >= 0.1
    if V >= 2:
        Y[:, 1] = 0.0                             # constant: sp2 == 0 exactly
        mask[:, 1] = True
    if V >= 3:
        Y[:, 2] = 1.5                             # constant, and the mean need not be exact
    if V >= 4:
        mask[:, 3] = False
        mask[:4, 3] = True                        # four knees left: n1 = 1 (or n2 = 1) in some labellings, 2 + 2 in others
    if V >= 5:
        mask[:, V - 1] = False                    # nobody: n = 0
    rows = rng.random((max(ROWS), N)) < 0.5
    rows[1] = False
    rows[1, 0] = True                             # group 1 is one knee
    if max(ROWS) > 2:
        rows[2] = True                            # group 2 is empty
    for a in (Y, mask, rows):
        a.setflags(write=False)
    return Y, (mask if with_mask else None), rows


@functools.lru_cache(maxsize=None)
def _reference(N, V, two_sample, with_mask=True):
    Y, mask, rows = _case(N, V, two_sample, with_mask)
    prep = gref.prepare(Y, mask, centre=two_sample)
    t = gref.permutation_t(prep, mask, rows, gref.TWO_SAMPLE if two_sample else gref.ONE_SAMPLE)
    t.setflags(write=False)
    return prep, t


def _device(Y, mask, rows, two_sample, batch):
    from oai_analysis_2_amd import ops
    P, V = rows.shape[0], Y.shape[1]
    prep = ops.group_prepare(torch.from_numpy(Y).cuda(), None if mask is None else torch.from_numpy(mask.astype(np.uint8)).cuda(), centre=two_sample)
    bits = torch.from_numpy(gref.pack_bits(rows).view(np.int32)).cuda()
    t0 = torch.full((V,), 7.0, dtype=torch.float64, device="cuda")
    max_abs = torch.full((P,), -1.0, dtype=torch.float64, device="cuda")
    exceed = torch.full((V,), -5, dtype=torch.int64, device="cuda")            # garbage: the first batch must start it
    tiles = []
    for p0 in range(0, P, batch):
        p1 = min(p0 + batch, P)
        tile = ops.permutation_t(prep, bits, p0, p1, ops.STATS_TWO_SAMPLE if two_sample else ops.STATS_ONE_SAMPLE)
        ops.permutation_reduce(tile, p0, t0, max_abs, exceed)
        tiles.append(tile)
    return prep, torch.cat(tiles), t0, max_abs, exceed


@pytest.mark.parametrize("two_sample", [True, False], ids=["two_sample", "one_sample"])
@pytest.mark.parametrize("N", KNEES)
def test_prepare_t_max_and_exceed_equal_the_restatement_to_the_bit(N, two_sample):
    for V in VERTS:
        Y, mask, rows = _case(N, V, two_sample)
        ref, t_ref = _reference(N, V, two_sample)
        for P in ROWS:
            prep, t, t0, max_abs, exceed = _device(Y, mask, rows[:P], two_sample, BATCH)
            where = f"N={N} V={V} P={P}"
            if P == ROWS[0]:
                for name in ("n", "mean", "std", "S", "Q", "C", "Qm"):
                    same_bits(getattr(prep, name), ref[name], f"{where} prepare.{name}")
            same_bits(t, t_ref[:P], f"{where} t")
            same_bits(t0, t_ref[0], f"{where} t0")
            want_max, want_exceed = gref.reduce_tiles(t_ref[:P])
            same_bits(max_abs, want_max, f"{where} max_abs")
            same_bits(exceed, want_exceed, f"{where} exceed")
        if two_sample and V >= 5 and N >= 4:                               # the corner cases are really there
            assert np.isnan(t_ref[:, 1]).all() and np.isnan(t_ref[:, V - 1]).all() and ref["n"][V - 1] == 0 and np.isnan(ref["mean"][V - 1])
            assert np.isnan(t_ref[1]).all() and np.isnan(t_ref[2]).all()
            if N >= 31:
                valid3 = ~np.isnan(t_ref[:, 3])
                assert valid3.any() and (~valid3).any()


def test_without_a_mask_every_entry_counts():
    N, V = 33, 257
    Y, _, rows = _case(N, V, True, False)
    ref, t_ref = _reference(N, V, True, False)
    prep, t, _, max_abs, exceed = _device(Y, None, rows, True, BATCH)
    assert (ref["n"] == N).all()
    same_bits(prep.C, ref["C"], "C")
    same_bits(t, t_ref, "t")
    same_bits(max_abs, gref.reduce_tiles(t_ref)[0], "max_abs")
    same_bits(exceed, gref.reduce_tiles(t_ref)[1], "exceed")


# ---- clusters --------------------------------------------------------------------------------------------------------------------------
def _hand_tile(V, t0, seed):
    """Rows written by hand: 0 a mix (runs, values exactly at +-t0, a NaN that splits a run, adjacent opposite signs, lone vertices),
    1 nothing above the threshold, 2 / 3 one component of either sign over everything, 4 every other vertex, 5 noise."""
    rng = np.random.default_rng(seed)
    tile = np.zeros((6, V))
    row = tile[0]
    row[:] = np.where(rng.random(V) < 0.5, 1.0, -1.0) * t0 * 0.5
    row[10:40] = t0 + 1.0
    row[25] = np.nan                               # splits the run 10..39
    row[40:60] = -t0 - 1.0                         # touches the positive run: must not join it
    row[70], row[71] = t0, -t0                     # exactly at the threshold: outside
    row[80] = t0 + 0.5                             # alone
    row[90] = -np.inf
    row[V - 1] = np.nextafter(t0, np.inf)
    row[V // 2:V // 2 + V // 4] = t0 * 3
    tile[1] = rng.uniform(-t0, t0, V)
    tile[2] = t0 + 1.0 + rng.random(V)
    tile[3] = -tile[2]
    tile[4] = np.where(np.arange(V) % 2 == 0, t0 + 1.0, -t0 - 1.0)
    tile[5] = rng.normal(0.0, 1.5 * t0, V)
    return tile


@pytest.mark.parametrize("graph", ["path_3000", "icosphere"])
def test_clusters_equal_the_restatement_to_the_element(graph):
    from oai_analysis_2_amd import mesh_processing as mp, ops
    t0 = 2.5
    if graph == "path_3000":
        V = 3000
        off, nbr = path_graph(V)
        off_d, nbr_d = torch.from_numpy(off).cuda(), torch.from_numpy(nbr).cuda()
    else:
        verts, faces = icosphere()
        V = len(verts)
        off_d, nbr_d = mp.vertex_adjacency_device(V, dev(faces))
        off, nbr = off_d.cpu().numpy(), nbr_d.cpu().numpy()
        assert np.array_equal(off, mp.vertex_adjacency(V, faces)[0]) and np.array_equal(nbr, mp.vertex_adjacency(V, faces)[1])
    tile = _hand_tile(V, t0, 11)
    label, size, extent = gref.clusters(tile, off, nbr, t0)
    assert extent[1] == 0 and extent[2] == V and extent[3] == V and (label[2] == 0).all() and (label[1] == -1).all()
    if graph == "path_3000":
        assert extent[4] == 1 and label[0, 24] == 10 and label[0, 26] == 26 and label[0, 40] == 40 and label[0, 70] == -1 and label[0, 71] == -1
        assert label[0, V - 1] == V - 1 and size[0, 80] == 1 and size[0, 24] == 15 and size[0, 26] == 14 and size[0, 45] == 20
    tile_d = torch.from_numpy(tile).cuda()
    ext, lab0, size0 = ops.graph_clusters(tile_d, off_d, nbr_d, t0, return_labels=True)
    same_bits(ext, extent, "max_extent")
    same_bits(lab0, label[0], "label of row 0")
    same_bits(size0, size[0], "size of row 0")
    assert ops.graph_clusters(tile_d, off_d, nbr_d, t0).cpu().numpy().tolist() == extent.tolist()       # without the label outputs
    for r in range(1, len(tile)):                                          # every other row's labels: the row as a tile of its own
        e, lab, siz = ops.graph_clusters(tile_d[r:r + 1], off_d, nbr_d, t0, return_labels=True)
        same_bits(e, extent[r:r + 1], f"max_extent of row {r}")
        same_bits(lab, label[r], f"label of row {r}")
        same_bits(siz, size[r], f"size of row {r}")


def test_clusters_read_a_hostile_graph_as_the_restatement_reads_it():
    """Offsets below 0 and beyond the neighbour count, neighbours below 0 and at or above V, a vertex among its own neighbours: the kernel
    clamps the first and ignores the others, as csrc/csr_graph.h states once for every graph kernel."""
    from oai_analysis_2_amd import ops
    off, nbr = gref.hostile_graph()
    V = len(off) - 1
    assert off[0] < 0 and off[V] > len(nbr) and (nbr < 0).any() and (nbr >= V).any() and 5 in nbr[off[5]:off[6]]
    t0 = 1.0
    tile = np.random.default_rng(5).normal(0.0, 2.0, (6, V))
    tile[0, 7], tile[1, :] = np.nan, np.abs(tile[1]) + 2 * t0              # row 1: every vertex in the positive set
    label, size, extent = gref.clusters(tile, off, nbr, t0)
    assert 1 < extent[1] < V - 2 and size[1, 0] == 1 and size[1, V - 1] == 1 and len(np.unique(label[1])) > 3
    off_d, nbr_d, tile_d = torch.from_numpy(off).cuda(), torch.from_numpy(nbr).cuda(), torch.from_numpy(tile).cuda()
    same_bits(ops.graph_clusters(tile_d, off_d, nbr_d, t0), extent, "max_extent")
    for r in range(len(tile)):
        e, lab, siz = ops.graph_clusters(tile_d[r:r + 1], off_d, nbr_d, t0, return_labels=True)
        same_bits(e, extent[r:r + 1], f"max_extent of row {r}")
        same_bits(lab, label[r], f"label of row {r}")
        same_bits(siz, size[r], f"size of row {r}")


# ---- the public interface --------------------------------------------------------------------------------------------------------------
N_E2E, P_E2E, T_CLUSTER = 24, 500, 6.0


def test_exhaustive_counts_lie_in_scipys_band():
    """N = 8 (4 + 4), V = 65, all 70 labellings.  A labelling and its complement tie up to rounding, so an exact count against an
    independent implementation is not defined: the device count must lie between scipy's counts with the comparison tightened and
    loosened by 1e-9 relative."""
    import scipy.stats
    from oai_analysis_2_amd import stats
    rng = np.random.default_rng(8)
    Y = rng.normal(2.0, 0.5, size=(8, 65)).astype(np.float32)
    groups = np.array([1, 0, 1, 1, 0, 0, 1, 0])
    res = stats.two_sample_test(_cohort(bare_atlas(65), Y), groups, n_permutations=10000, batch=32)
    assert res.exact and res.n_permutations == 70 and (res.n1 == 4).all() and (res.n2 == 4).all()
    rows = stats.label_permutations(groups, 10000).rows()
    y = Y.astype(np.float64)
    a = np.abs(np.stack([scipy.stats.ttest_ind(y[r], y[~r], axis=0, equal_var=True).statistic for r in rows]))
    assert np.abs(res.t - scipy.stats.ttest_ind(y[rows[0]], y[~rows[0]], axis=0).statistic).max() < 1e-10
    count = np.rint(res.p_uncorrected * 70).astype(np.int64)
    low, high = (a >= a[0] * (1 + 1e-9)).sum(axis=0), (a >= a[0] * (1 - 1e-9)).sum(axis=0)
    print("exceed", count.tolist(), "band width", (high - low).tolist())
    assert (low <= count).all() and (count <= high).all() and (count >= 1).all()
    assert np.allclose(res.mean_difference, y[rows[0]].mean(axis=0) - y[~rows[0]].mean(axis=0), rtol=1e-12, atol=1e-15)


def test_two_sample_end_to_end_finds_the_painted_cap_and_is_reproducible():
    from oai_analysis_2_amd import mesh_processing as mp, stats
    Y, groups, cap = painted(0.5, N_E2E)
    atlas = sphere_atlas()
    res = stats.two_sample_test(_cohort(atlas, Y), groups, n_permutations=P_E2E, cluster_threshold=T_CLUSTER, seed=1, batch=96)
    assert res.n_permutations == P_E2E and not res.exact and res.max_abs.shape == (P_E2E,) and res.max_extent.shape == (P_E2E,)
    big = max(res.clusters, key=lambda c: c.extent)
    members = res.cluster_label == big.label
    assert big.sign == 1 and members[cap].all() and big.extent == members.sum() >= cap.sum()
    assert big.p_cluster == 1.0 / P_E2E                                    # the smallest value P labellings can give
    area, _ = mp.mesh_areas(atlas.inner["FC"])
    assert big.area == pytest.approx(area[members].sum(), rel=1e-12) and 0 < big.area < 4 * np.pi * 400 * 0.2
    assert (res.p_fwer[cap] == 1.0 / P_E2E).all() and (res.mean_difference[cap] > 0.3).all()
    assert res.max_extent[0] == big.extent and [c.label for c in res.clusters] == sorted(c.label for c in res.clusters)
    # the device against the restatement through the public interface, batches and all
    perms = stats.label_permutations(groups, P_E2E, seed=1)
    t_ref = gref.permutation_t(gref.prepare(Y, None), None, perms.rows(), gref.TWO_SAMPLE)
    same_bits(res.t, t_ref[0], "t")
    same_bits(res.max_abs, gref.reduce_tiles(t_ref)[0], "max_abs")
    assert np.array_equal(np.rint(res.p_uncorrected * P_E2E).astype(np.int64), gref.reduce_tiles(t_ref)[1])
    # a second run on the same input: the same bits in every field
    again = stats.two_sample_test(_cohort(atlas, Y), groups, n_permutations=P_E2E, cluster_threshold=T_CLUSTER, seed=1, batch=96)
    for name in ("t", "n1", "n2", "mean_difference", "p_uncorrected", "p_fwer", "max_abs", "cluster_label", "max_extent"):
        same_bits(getattr(again, name), getattr(res, name), name)
    assert again.clusters == res.clusters
    # another batch size changes nothing either
    other = stats.two_sample_test(_cohort(atlas, Y), groups, n_permutations=P_E2E, cluster_threshold=T_CLUSTER, seed=1)
    for name in ("t", "p_uncorrected", "p_fwer", "max_abs", "cluster_label", "max_extent"):
        same_bits(getattr(other, name), getattr(res, name), name + " (default batch)")


def test_without_an_effect_the_corrected_p_is_the_rank_of_the_observed_maximum():
    from oai_analysis_2_amd import stats
    Y, groups, _ = painted(0.0, N_E2E)
    res = stats.two_sample_test(_cohort(sphere_atlas(), Y), groups, n_permutations=P_E2E, seed=2, batch=64)
    assert not np.isnan(res.t).any() and res.cluster_label is None and res.clusters == []
    assert (res.p_fwer >= res.p_uncorrected).all()
    assert res.p_fwer.min() == (res.max_abs >= res.max_abs[0]).sum() / P_E2E
    assert res.max_abs[0] == np.abs(res.t).max()


def test_paired_test_matches_rows_by_id_and_finds_the_cap():
    """A cohort against itself shifted by 0.5 mm on the cap -- with fresh 0.1 mm noise, as a constant difference has no variance and so
    no t -- and handed over in another order: ids match the rows."""
    from oai_analysis_2_amd import stats
    Y, _, cap = painted(0.0, N_E2E)
    atlas = sphere_atlas()
    rng = np.random.default_rng(77)
    follow = (Y + 0.1 * rng.normal(size=Y.shape)).astype(np.float32)
    follow[:, cap] += np.float32(0.5)
    follow[3, 5] = np.nan                                                  # a missing value on one side: the pair is missing
    ids = [f"knee{i:02d}" for i in range(N_E2E)]
    order = rng.permutation(N_E2E)
    a, b = _cohort(atlas, follow[order], [ids[i] for i in order]), _cohort(atlas, Y, ids)
    res = stats.paired_test(a, b, n_permutations=P_E2E, cluster_threshold=T_CLUSTER, seed=3, batch=80)
    assert res.n1[5] == N_E2E - 1 and (np.delete(res.n1, 5) == N_E2E).all() and np.array_equal(res.n1, res.n2)
    big = max(res.clusters, key=lambda c: c.extent)
    members = res.cluster_label == big.label
    assert big.sign == 1 and members[cap].all() and big.p_cluster == 1.0 / P_E2E
    assert (res.mean_difference[cap] > 0.4).all() and np.abs(res.mean_difference[~cap]).max() < 0.15
    # the restatement on the differences in a's order
    diff = follow[order] - Y[order]
    mask = ~np.isnan(diff)
    flips = stats.sign_flips(N_E2E, P_E2E, seed=3)
    t_ref = gref.permutation_t(gref.prepare(np.where(mask, diff, 0).astype(np.float32), mask, centre=False), mask, flips.rows(), gref.ONE_SAMPLE)
    same_bits(res.t, t_ref[0], "t")
    same_bits(res.max_abs, gref.reduce_tiles(t_ref)[0], "max_abs")
    with pytest.raises(ValueError, match="same ids"):
        stats.paired_test(a, _cohort(atlas, Y, ["x"] + ids[1:]), n_permutations=10)


def test_the_cohort_masks_what_is_missing():
    from oai_analysis_2_amd import stats
    from oai_analysis_2_amd.thickness import KneeThickness
    atlas = bare_atlas(6)
    vec = np.array([1, 2, np.nan, 4, 5, 6], np.float32)
    cover = np.array([1, 1, 1, 0, 1, 1], np.uint8)
    knees = [KneeThickness(vec, vec, coverage={"FC": cover}), KneeThickness(torch.from_numpy(vec + 1).cuda(), vec, coverage={"FC": torch.from_numpy(cover).cuda()}),
             KneeThickness(np.full(6, np.nan, np.float32), vec, errors={"FC": "no surface"})]
    plain = stats.ThicknessCohort.from_stream(enumerate(knees), atlas, "FC")
    assert plain.ids == [0, 1, 2] and plain.mask.cpu().numpy().tolist() == [[1, 1, 0, 1, 1, 1], [1, 1, 0, 1, 1, 1], [0] * 6]
    covered = stats.ThicknessCohort.from_stream(enumerate(knees), atlas, "FC", use_coverage=True)
    assert covered.mask.cpu().numpy().tolist() == [[1, 1, 0, 0, 1, 1], [1, 1, 0, 0, 1, 1], [0] * 6]
    s = covered.summary()
    assert s["n"].tolist() == [2, 2, 0, 0, 2, 2] and s["mean"][0] == 1.5 and np.isnan(s["mean"][2]) and s["std"][0] == np.sqrt(0.5)
