"""GPU: the three morphometry primitives against their numpy restatement (tests/morphometry_ref.py), to the bit: oai_mesh_areas,
oai_point_footprint(_grid) and oai_region_stats.  Every quantity is an integer or an fp64 result of IEEE add / mul / compare / min /
max; the one exception is the sqrt of a face area, which the project already holds to numpy's bits (oai_lncc)."""
import functools

import numpy as np
import pytest
import torch

import morphometry_ref as mref
import ordered_reduce_ref as oref

pytestmark = pytest.mark.gpu

EMPTY_FACES = np.zeros((0, 3), np.int32)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype == np.float64
    return a.view(np.int64)


# ---- oai_mesh_areas ----------------------------------------------------------------------------------------------------------------
def _strip(m, seed=0):
    """A strip of m triangles between two jittered rows of vertices: face k = (k, k + 1, k + 2), alternate faces turned round."""
    rng = np.random.default_rng([seed, m])
    k = np.arange(m + 2)
    verts = np.stack([0.5 * k, (k % 2).astype(np.float64), np.zeros(m + 2)], axis=1) + rng.normal(scale=0.1, size=(m + 2, 3))
    faces = np.stack([k[:-2], k[1:-1], k[2:]], axis=1)
    faces[1::2] = faces[1::2, ::-1]
    return verts.astype(np.float32), faces.astype(np.int32)


def _fan(m=300):
    """m faces around the hub, vertex 0: the rim's radii run over six decades, so the face areas span twelve, and the hub's sum depends
    on the order in which they are added."""
    k = np.arange(m + 1)
    r = 10.0 ** (-3.0 + 6.0 * k / m)
    ang = 2 * np.pi * k / (m + 1)
    rim = np.stack([r * np.cos(ang), r * np.sin(ang), 0.01 * r * np.sin(5 * ang)], axis=1)
    verts = np.concatenate([np.zeros((1, 3)), rim]).astype(np.float32)
    faces = np.stack([np.zeros(m, np.int64), 1 + k[:-1], 2 + k[:-1]], axis=1).astype(np.int32)
    return verts, faces


def _sphere_mesh():
    from oai_analysis_2_amd import mesh_processing as mp
    z, y, x = np.mgrid[0:24, 0:24, 0:24].astype(np.float32)
    vol = 1.0 / (1.0 + np.exp(np.sqrt((x - 11.3) ** 2 + (y - 12.1) ** 2 + (z - 11.7) ** 2) - 8.0))
    return mp.marching_cubes(vol.astype(np.float32), 0.5, (0.36, 0.37, 0.7))


def _odd():
    """One unreferenced vertex (3), a face that names a vertex twice, and a repeated face."""
    verts = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [9, 9, 9], [1, 1, 5]], np.float32)
    return verts, np.array([[0, 1, 2], [4, 4, 1], [2, 1, 4], [0, 1, 2]], np.int32)


MESHES = {"one_face": lambda: (np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], np.float32), np.array([[0, 1, 2]], np.int32)),
          "strip_255": lambda: _strip(255), "strip_256": lambda: _strip(256), "strip_257": lambda: _strip(257), "strip_1025": lambda: _strip(1025),
          "fan_300": _fan, "odd": _odd, "sphere_24": _sphere_mesh}


@pytest.mark.parametrize("name", list(MESHES))
def test_mesh_areas_equal_the_restatement_to_the_bit(name):
    from oai_analysis_2_amd import mesh_processing as mp
    verts, faces = MESHES[name]()
    va, fa = mp.mesh_areas(mp.Mesh(verts, faces))
    ref_va, ref_fa = mref.mesh_areas(verts, faces)
    assert va.dtype == fa.dtype == np.float64 and va.shape == (len(verts),) and fa.shape == (len(faces),)
    print(name, "verts", len(verts), "faces", len(faces), "face areas differing", int((_bits(fa) != _bits(ref_fa)).sum()),
          "vertex areas differing", int((_bits(va) != _bits(ref_va)).sum()), "surface", float(fa.sum()))
    assert np.array_equal(_bits(fa), _bits(ref_fa))
    assert np.array_equal(_bits(va), _bits(ref_va))
    va2, fa2 = mp.mesh_areas(mp.Mesh(verts, faces))
    assert np.array_equal(_bits(va2), _bits(va)) and np.array_equal(_bits(fa2), _bits(fa))            # twice: the same bits
    dev = mp._mesh_areas_dev(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda())         # the resident form, face areas not asked for
    assert dev.is_cuda and np.array_equal(_bits(dev), _bits(va))
    if name == "one_face":
        assert fa.tolist() == [6.0] and va.tolist() == [2.0, 2.0, 2.0]
    if name == "fan_300":
        assert fa.max() / fa.min() > 1e11
        down = mref.vertex_areas(len(verts), faces, ref_fa, descending=True)
        assert down[0] != ref_va[0]                              # the hub's sum is order-dependent: an unordered implementation shows
        assert va[0] == ref_va[0]
    if name == "odd":
        assert va[3] == 0.0 and fa[1] == 0.0 and fa[0] == fa[3] == 6.0
        assert va[4] == (fa[1] + fa[1] + fa[2]) / 3.0            # the degenerate face counts twice at the vertex it names twice
    if name == "sphere_24":
        assert len(faces) > 1000 and np.bincount(faces.reshape(-1), minlength=len(verts)).min() >= 3
        assert abs(va.sum() - fa.sum()) <= len(faces) * np.finfo(np.float64).eps * fa.sum()


def test_mesh_areas_of_nothing():
    from oai_analysis_2_amd import mesh_processing as mp
    va, fa = mp.mesh_areas(mp.Mesh(np.ones((5, 3), np.float32), EMPTY_FACES))
    assert va.tolist() == [0.0] * 5 and fa.shape == (0,)
    va, fa = mp.mesh_areas(mp.Mesh(np.zeros((0, 3), np.float32), EMPTY_FACES))
    assert va.shape == (0,) and fa.shape == (0,)


# ---- oai_point_footprint -------------------------------------------------------------------------------------------------------------
def _case(seed, n_src, n_tgt, box, far=0):
    """tests/test_thickness_map_gpu.py::_case, the Distance array only."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(0, box, size=(n_src, 3)).astype(np.float32)
    tgt = rng.uniform(-0.2 * box, 1.2 * box, size=(n_tgt, 3)).astype(np.float32)
    if far:
        tgt = np.concatenate([tgt, rng.uniform(-30 * box, 30 * box, size=(far, 3)).astype(np.float32)])
    return src, tgt, rng.uniform(0.5, 4.0, n_src).astype(np.float32)


def _serial_means(src, vals, tgt, radius):
    """float32(fp64 sum in ascending source index / count) where count > 0: what the brute-force map_attributes stores."""
    from thickness_map_ref import pairwise_d2
    out = np.full(len(tgt), np.nan, np.float32)
    v = vals.astype(np.float64)
    for a in range(0, len(tgt), 512):
        inside = pairwise_d2(tgt[a:a + 512], src) <= float(radius) * float(radius)
        sums = np.cumsum(np.where(inside, v[None, :], 0.0), axis=1)[:, -1]              # cumsum adds one by one, in index order
        cnt = inside.sum(axis=1)
        out[a:a + 512] = np.where(cnt > 0, sums / np.maximum(cnt, 1), np.nan).astype(np.float32)
    return out


@pytest.mark.parametrize("seed,n_src,n_tgt,box,radius,far", [
    (0, 4000, 3000, 10.0, 1.0, 40),        # dense overlap: ~17 source points per footprint
    (1, 300, 2000, 40.0, 1.0, 40),         # sparse: most targets fall back to the closest point
    (2, 2500, 2500, 12.0, 2.5, 0),         # a larger radius
    (3, 1, 50, 1.0, 1.0, 10)])             # one source point
def test_point_footprint_grid_brute_and_restatement_agree(seed, n_src, n_tgt, box, radius, far):
    from oai_analysis_2_amd import mesh_processing as mp
    src, tgt, vals = _case(seed, n_src, n_tgt, box, far)
    ref_count, ref_d2, ref_j = mref.point_footprint(src, tgt, radius)
    s, t = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    grid = (src.min(axis=0).astype(np.float64), src.max(axis=0).astype(np.float64))
    for form in (grid, None, grid):                                                     # grid, brute force, and the grid again: the same bits
        count, d2, j = mp._point_footprint_dev(s, t, radius, form)
        count, d2, j = count.cpu().numpy(), d2.cpu().numpy(), j.cpu().numpy()
        assert count.dtype == np.int32 and j.dtype == np.int32
        print("grid" if form else "brute", "count differing", int((count != ref_count).sum()), "nearest_j", int((j != ref_j).sum()),
              "nearest_d2", int((_bits(d2) != _bits(ref_d2)).sum()), "uncovered", int((count == 0).sum()), "of", len(tgt))
        assert np.array_equal(count, ref_count) and np.array_equal(j, ref_j) and np.array_equal(_bits(d2), _bits(ref_d2))     # no element excluded
    assert (ref_count == 0).any() and (n_src == 1 or (ref_count > 0).any())
    # the public form: the distance is the square root
    c2, dist, j2 = mp.point_footprint(tgt, src, radius=radius)
    assert np.array_equal(c2, ref_count) and np.array_equal(j2, ref_j) and np.array_equal(_bits(dist), _bits(np.sqrt(ref_d2)))
    # consistency with the unchanged map_attributes on the same inputs
    source, target = mp.Mesh(src, EMPTY_FACES, {"Distance": vals}), mp.Mesh(tgt, EMPTY_FACES)
    brute = mp.map_attributes(source, target, radius=radius, broad_phase=False).point_data["Distance"]
    binned = mp.map_attributes(source, target, radius=radius, broad_phase=True).point_data["Distance"]
    none = ref_count == 0
    for got in (brute, binned):
        assert np.array_equal(got[none].view(np.int32), vals[ref_j[none]].view(np.int32))           # the fallback took the nearest point's value
    mean = _serial_means(src, vals, tgt, radius)
    assert np.array_equal(brute[~none].view(np.int32), mean[~none].view(np.int32))                   # float32(mean), in the brute force's own order
    # (the grid form adds cell by cell: the same fp64 terms in another order, so within one float32 ulp, as test_thickness_map_gpu.py has it)
    assert (np.abs(binned[~none].astype(np.float64) - mean[~none].astype(np.float64)) <= np.spacing(np.abs(mean[~none])).astype(np.float64)).all()


def test_point_footprint_without_source_points_raises():
    from oai_analysis_2_amd import mesh_processing as mp
    with pytest.raises(ValueError):
        mp._point_footprint_dev(torch.zeros((0, 3), device="cuda"), torch.zeros((4, 3), device="cuda"))


# ---- oai_region_stats ----------------------------------------------------------------------------------------------------------------
REGION_SIZES = oref.ORDER_SIZES[:6]        # 1, 63, 64, 65, 1025, 1024 * 257 + 3: partial waves, two blocks, the finish in runs, the grid stride


@functools.lru_cache(maxsize=None)
def _region_case(n, R):
    """Weights exp(U(-20, 20)), labels over -1 .. R with one label of [0, R) never drawn when R > 1, NaN and +-inf among the values, a
    random covered mask; with them the restated rows, computed once."""
    rng = np.random.default_rng([11, n, R])
    values = rng.normal(2.0, 1.0, n).astype(np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        values[rng.uniform(size=n) < 0.03] = bad
    weights = np.exp(rng.uniform(-20.0, 20.0, n))
    labels = rng.integers(-1, R + 1, n).astype(np.int32)
    empty = 1 if R > 1 else None
    if empty is not None:
        labels[labels == empty] = 0
    covered = (rng.uniform(size=n) < 0.7).astype(np.uint8)
    want = {"full": mref.region_stats(values, weights, labels, covered, R)}
    if n * R < 1 << 22:                    # the null-pointer forms at every size and R but the largest product: the restatement is a numpy loop
        want.update(no_mask=mref.region_stats(values, weights, labels, None, R), no_labels=mref.region_stats(values, weights, None, covered, R))
    for a in (values, weights, labels, covered, *want.values()):
        a.setflags(write=False)
    return values, weights, labels, covered, want, empty


@pytest.mark.parametrize("R", [1, 3, 64])
@pytest.mark.parametrize("n", REGION_SIZES)
def test_region_stats_equal_the_restatement_to_the_bit(n, R):
    from oai_analysis_2_amd import ops
    values, weights, labels, covered, want, empty = _region_case(n, R)
    v, w, l, c = (torch.from_numpy(np.array(a)).cuda() for a in (values, weights, labels, covered))
    for form, args in (("full", (l, c)), ("no_mask", (l, None)), ("no_labels", (None, c)), ("full", (l, c))):      # and the first again: the same bits
        if form not in want:
            continue
        got = ops.region_stats(v, w, *args, n_regions=R)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (R, 12)
        bad = _bits(got) != _bits(want[form])
        print(n, R, form, "slots differing", int(bad.sum()), "of", bad.size, np.argwhere(bad)[:4].tolist())
        assert not bad.any()
    full = want["full"]
    if empty is not None:
        assert np.array_equal(full[empty], mref.REGION_CLEAR)                        # an empty region: zeros, +inf, -inf
    if "no_labels" in want:
        assert np.array_equal(want["no_labels"][1:], np.tile(mref.REGION_CLEAR, (R - 1, 1)))
    assert full[:, 0].sum() == ((labels >= 0) & (labels < R)).sum()
    if n >= 1025 and R == 3:                                                          # the order shows: the serial sum is another number
        m = (labels == 0) & (covered != 0) & np.isfinite(values)
        assert float(np.add.accumulate(weights[m])[-1]) != full[0, 5]
    # a slice of a larger buffer as the output, as ThicknessAtlas.measure uses it
    buf = torch.zeros((R + 2, 12), dtype=torch.float64, device="cuda")
    ops.region_stats(v, w, l, c, n_regions=R, out=buf[1:R + 1])
    assert np.array_equal(_bits(buf[1:R + 1]), _bits(full)) and not buf[0].any() and not buf[R + 1].any()


def test_region_stats_of_nothing_and_bad_arguments():
    from oai_analysis_2_amd import ops
    none = ops.region_stats(torch.zeros(0, device="cuda"), torch.zeros(0, dtype=torch.float64, device="cuda"), n_regions=2)
    assert np.array_equal(none.cpu().numpy(), np.tile(mref.REGION_CLEAR, (2, 1)))
    v, w = torch.zeros(4, device="cuda"), torch.ones(4, dtype=torch.float64, device="cuda")
    for R in (0, 65):
        with pytest.raises(ValueError):
            ops.region_stats(v, w, n_regions=R)
    with pytest.raises(ValueError):
        ops.region_stats(v, w[:3])
