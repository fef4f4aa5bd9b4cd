"""What the tests of the cohort-statistics stack share (test_group_*, test_graph_*, test_bootstrap_*, test_rank_transform_*,
test_cohort_pca_*, test_vertex_regression_*, test_cluster_robust_*, test_longitudinal_*, test_normative_*): the comparator behind every
"equal to the bit", the sphere, the atlas and cohort stand-ins, and the restated fields that several result classes have in common.  No
tests and no fixtures; nothing here that only one file uses.  A helper that mirrors one kernel's constants (``_rows_per_thread``) stays
beside the tests of that kernel."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np
import torch

import graph_smooth_ref as sref
import graph_tfce_ref as tref
import group_stats_ref as gref
from graph_smooth_ref import path_graph  # noqa: F401  (the path 0 - 1 - ... - n-1 as (offsets, neighbours), for the tests to import from here)


def same_bits(got, want, what):
    """``got`` (a tensor is downloaded) has the dtype, the shape and the bits of ``want``.  Floats of either width: NaN at the same places
    (whatever the payload) and the same bit pattern everywhere else, so -0.0 is not +0.0.  Anything else: equal elements."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
        as_int = np.int64 if got.dtype == np.float64 else np.int32
        got, want = np.where(np.isnan(got), 0, got).view(as_int), np.where(np.isnan(want), 0, want).view(as_int)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} differ, first at {bad[0].tolist()}"


def same_result(got, want: dict, what, extra=()):
    """Every field of the result dataclass ``got`` against the dict ``want``, whose keys are exactly the fields and ``extra`` (attributes
    that are not fields): arrays to the bit, everything else equal and of the same type."""
    fields = {f.name for f in dataclasses.fields(got)} | set(extra)
    assert fields == set(want), (what, fields ^ set(want))
    for name, b in want.items():
        a = getattr(got, name)
        if isinstance(b, np.ndarray):
            same_bits(a, b, f"{what}: {name}")
        else:
            assert a == b and type(a) is type(b), f"{what}: {name}: {a!r} != {b!r}"


def dev(a, dtype=None):
    """A numpy array on the GPU, cast to ``dtype`` if one is given; None stays None.  Always a C-contiguous copy: the cached cases are
    read-only, and the kernels take dense rows."""
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


@functools.lru_cache(maxsize=None)
def icosphere(level=3):
    """(verts float32 [n, 3] on the unit sphere, faces int32 [m, 3]), read-only: 162 vertices at level 2, 642 and 1280 faces at level 3."""
    verts, faces = sref.icosphere(level)
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


@functools.lru_cache(maxsize=None)
def sphere_graph(level=3):
    """(offsets, neighbours) of the icosphere on the host, as ``mesh_processing.vertex_adjacency_device`` builds them."""
    from oai_analysis_2_amd import mesh_processing as mp
    verts, faces = icosphere(level)
    off_d, nbr_d = mp.vertex_adjacency_device(len(verts), dev(faces))
    return off_d.cpu().numpy(), nbr_d.cpu().numpy()


def sphere_atlas(level=3, scale=20.0, image=None):
    """What the statistics read of an atlas: the icosphere of radius ``scale`` mm as the femoral cartilage's inner surface, on GPU 0;
    ``image`` stands for the atlas' rasteriser where a test asks for one."""
    from oai_analysis_2_amd import mesh_processing as mp
    verts, faces = icosphere(level)
    atlas = SimpleNamespace(inner={"FC": mp.Mesh(verts * np.float32(scale), np.array(faces))}, device=torch.device("cuda", 0))
    if image is not None:
        atlas.image = image
    return atlas


def bare_atlas(V):
    """An atlas of V vertices and no faces: for the tests that need no surface."""
    from oai_analysis_2_amd import mesh_processing as mp
    return SimpleNamespace(inner={"FC": mp.Mesh(np.zeros((V, 3), np.float32), np.zeros((0, 3), np.int32))}, device=torch.device("cuda", 0))


def cohort(atlas, Y, ids=None, mask=None, chunk=5):
    """The rows of Y as a ThicknessCohort that grows in several steps of ``chunk`` rows."""
    from oai_analysis_2_amd import stats
    out = stats.ThicknessCohort(atlas, "FC", chunk=chunk)
    for i, row in enumerate(Y):
        out.add_vector(row, None if ids is None else ids[i], None if mask is None else mask[i])
    return out


def knees(p):
    """Cohort sizes for p design columns: the fewest that leave a degree of freedom, and both sides of 32 and of a wave."""
    return tuple(sorted({p + 1, 7, 31, 33, 65}))


def rows(batch):
    """Permutation rows for a launch of ``batch`` rows: 1, 2, both sides of one launch, and two launches and a ragged third."""
    return (1, 2, batch - 1, batch + 1, 2 * batch + 5)


def design(N, p, rng):
    """[N, p] with x last.  p = 1: a continuous x alone (no intercept).  p = 2: intercept and a dummy x.  p = 4: intercept, a sex dummy,
    age, a dummy x.  p = 6: intercept, a sex dummy, three continuous covariates, a continuous x."""
    i = np.arange(N)
    sex, dummy = (i % 2).astype(np.float64), ((i // 2) % 2).astype(np.float64)
    cont = lambda: rng.normal(0.0, 1.0, N)
    cols = {1: [cont()], 2: [np.ones(N), dummy], 4: [np.ones(N), sex, 60 + 8 * cont(), dummy],
            6: [np.ones(N), sex, 60 + 8 * cont(), 27 + 4 * cont(), cont(), cont()]}[p]
    return np.ascontiguousarray(np.stack(cols, axis=1))


@functools.lru_cache(maxsize=None)
def painted(offset, n):
    """(Y, groups, cap): n float32 knees on the sphere: 2 mm + 0.1 mm noise, and ``offset`` mm more on the cap z > 0.8 for group 1 (the
    first half).  The two-sample and the TFCE tests share it; the other ``_painted`` have designs of their own."""
    verts, _ = icosphere()
    cap = verts[:, 2] > 0.8
    rng = np.random.default_rng(2024)
    Y = (2.0 + 0.1 * rng.normal(size=(n, len(verts)))).astype(np.float32)
    groups = np.arange(n) < n // 2
    Y[np.ix_(groups, cap)] += np.float32(offset)
    return Y, groups, cap


def restated_fields(tile, P, atlas, threshold):
    """The fields that every permutation result shares, from the restatements of the reduce, the clusters and the TFCE and the host's own
    bookkeeping, and max |statistic| per row beside them."""
    from oai_analysis_2_amd import mesh_processing as mp, stats
    max_abs, exceed = gref.reduce_tiles(tile)
    p_unc, p_fwer = stats._p_values(tile[0], max_abs, exceed, P)
    off, nbr = sphere_graph()
    area = mp.mesh_areas(atlas.inner["FC"])[0]
    label, size, extent = gref.clusters(tile, off, nbr, threshold)
    found = []
    for lab in np.unique(label[0][label[0] >= 0]):
        members = np.nonzero(label[0] == lab)[0]
        found.append(stats.Cluster(int(lab), 1 if tile[0][lab] > 0 else -1, int(size[0][lab]), float(np.cumsum(area[members])[-1]),
                                   float((extent >= size[0][lab]).sum()) / float(P)))
    enhanced, clipped = tref.tfce(tile, off, nbr, dh=0.1, E=1.0, H=2.0, weights=np.rint(area * 2 ** 20).astype(np.int64), unit=2.0 ** -20)
    max_tfce, tfce_exceed = gref.reduce_tiles(enhanced)
    p_tfce_unc, p_tfce = stats._p_values(enhanced[0], max_tfce, tfce_exceed, P)
    return dict(p_uncorrected=p_unc, p_fwer=p_fwer, n_permutations=P, exact=False, cluster_threshold=threshold, cluster_label=label[0], clusters=found,
                max_extent=extent, tfce=enhanced[0], p_tfce=p_tfce, p_tfce_uncorrected=p_tfce_unc, max_tfce=max_tfce,
                tfce_clipped=int(np.count_nonzero(clipped)), tfce_settings=stats.TFCE(), kind="FC"), max_abs
