"""GPU: mesh QC (csrc/mesh_quality.hip; mesh_processing.mesh_topology / mesh_geometry / mesh_self_intersections, qc.mesh_quality /
split_quality, ThicknessAtlas.measure(..., mesh_qc=True)) against tests/mesh_quality_ref.py: every integer to the element, every fp64
figure to the bit."""
import dataclasses

import numpy as np
import pytest
import torch

import mesh_quality_ref as mref
from oai_analysis_2_amd.mesh_processing import Mesh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mp():
    from oai_analysis_2_amd import _lib, mesh_processing
    _lib.load()
    return mesh_processing


@pytest.fixture(scope="module")
def qc(mp):
    from oai_analysis_2_amd import qc
    return qc


def _topology(mp, verts, faces, side=None):
    """(record int64 [16], edge_class) from the device, unchecked, and compared with the restatement."""
    f = mp._dev(faces, np.int32, (3,))
    s = None if side is None else mp._dev(side, np.int8)
    cls, rec = mp._mesh_topology_dev(f, len(verts), s)
    rec, cls = rec.cpu().numpy(), cls.cpu().numpy()
    want_rec, want_cls = mref.topology(faces, len(verts), side)
    print(dict(zip(mref.TOPO, rec)))
    assert np.array_equal(rec, want_rec), (dict(zip(mref.TOPO, rec)), dict(zip(mref.TOPO, want_rec)))
    assert cls.dtype == np.uint8 and np.array_equal(cls, want_cls)
    return dict(zip(mref.TOPO, (int(x) for x in rec))), cls


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


# ---- topology ------------------------------------------------------------------------------------------------------------------------
def test_sphere_two_spheres_and_torus(mp, qc):
    v, f = mref.uv_sphere()
    assert v.shape == (362, 3) and f.shape == (720, 3)
    t, cls = _topology(mp, v, f)
    assert t["euler_characteristic"] == 2 and t["edges"] == t["manifold_edges"] == 1080 and t["boundary_loops"] == 0
    assert (cls != 0).sum() == 1080
    q = qc.mesh_quality(Mesh(v, f))
    assert q.closed and q.components == 1 and q.genus_sum == 0 and q.intersecting_pairs == 0 and q.intersecting_faces == 0
    assert q.volume_mm3 == abs(q.geometry["signed_volume"]) and 0.97 * 4.18879 < q.volume_mm3 < 4.18879          # inscribed in the unit ball
    v2, f2 = mref.two_spheres()
    t, _ = _topology(mp, v2, f2)
    assert t["euler_characteristic"] == 4 and t["faces"] == 1440
    q2 = qc.mesh_quality(Mesh(v2, f2), self_intersections=False)
    assert q2.closed and q2.components == 2 and q2.genus_sum == 0 and q2.intersecting_pairs is None and q2.intersecting_faces is None
    tv, tf = mref.torus()
    t, _ = _topology(mp, tv, tf)
    assert t["euler_characteristic"] == 0 and t["boundary_edges"] == t["misoriented_edges"] == t["non_manifold_edges"] == 0
    q3 = qc.mesh_quality(Mesh(tv, tf), self_intersections=False)
    assert q3.closed and q3.components == 1 and q3.genus_sum == 1


def test_defects_are_classified(mp):
    v, f = mref.uv_sphere()
    f = np.array(f)
    # two faces with no common vertex removed: two holes of three edges
    a, b = 100, 400
    assert not set(f[a]) & set(f[b])
    t, _ = _topology(mp, v, np.delete(f, [a, b], axis=0))
    assert t["boundary_edges"] == 6 and t["boundary_loops"] == 2 and t["euler_characteristic"] == 0
    # one face flipped: its three edges run the same way as their neighbours'
    g = f.copy()
    g[a] = g[a][::-1]
    t, _ = _topology(mp, v, g)
    assert t["misoriented_edges"] == 3 and t["boundary_edges"] == 0 and t["non_manifold_edges"] == 0
    # a fin glued on an existing edge: that edge carries three faces, the fin's other two are boundary
    fin_v = np.concatenate([v, [[0.0, 0.0, 2.0]]]).astype(np.float32)
    t, cls = _topology(mp, fin_v, np.concatenate([f, [[f[a][0], f[a][1], len(v)]]]).astype(np.int32))
    assert t["non_manifold_edges"] == 1 and t["boundary_edges"] == 2 and t["boundary_loops"] == 1
    # a duplicated face: its three edges carry three faces each
    t, _ = _topology(mp, v, np.concatenate([f, f[a:a + 1]]))
    assert t["non_manifold_edges"] == 3 and t["boundary_edges"] == 0
    # a degenerate face and a vertex nothing names
    t, cls = _topology(mp, fin_v, np.concatenate([f, [[5, 5, 9]]]).astype(np.int32))
    assert t["degenerate_faces"] == 1 and t["referenced_vertices"] == 362 and t["euler_characteristic"] == 2 and not cls[-1].any()
    # an index outside the mesh is counted, reads nothing, and raises in the checked form
    bad = np.concatenate([f, [[0, 1, 362]], [[-1, 2, 3]]]).astype(np.int32)
    t, cls = _topology(mp, v, bad)
    assert t["bad_faces"] == 2 and t["euler_characteristic"] == 2 and not cls[-2:].any()
    with pytest.raises(ValueError, match="2 face"):
        mp.mesh_topology(Mesh(v, bad))
    with pytest.raises(ValueError, match="2 face"):
        mp.mesh_geometry(Mesh(v, bad))


@pytest.mark.parametrize("n_faces", [0, 255, 256, 257, 300])
def test_a_fan_of_high_valence_and_the_block_boundaries(mp, n_faces):
    v, f = mref.fan(n_faces)
    t, cls = _topology(mp, v, f)
    assert t["faces"] == n_faces and t["edges"] == (2 * n_faces + 1 if n_faces else 0) and t["boundary_loops"] == (1 if n_faces else 0)
    assert t["euler_characteristic"] == (1 if n_faces else 0)
    geo = mp._mesh_geometry_dev(mp._dev(v, np.float32, (3,)), mp._dev(f, np.int32, (3,)), mp._dev(cls, np.uint8, (3,))).cpu().numpy()
    assert np.array_equal(_bits(geo), _bits(mref.geometry(v, f, cls)))
    if not n_faces:
        assert not geo.any()


def test_the_interface_of_a_side_vector(mp):
    v, f = mref.uv_sphere()
    for island, edges, loops in ((False, 24, 1), (True, 48, 2)):
        side = mref.equator_side(f, v, island)
        t, cls = _topology(mp, v, f, side)
        assert t["interface_edges"] == edges and t["interface_loops"] == loops and ((cls & 16) != 0).sum() == edges
        assert t["faces_inner"] + t["faces_outer"] == 720 and t["faces_unassigned"] == 0
        rec, cls_host = mp.mesh_topology(Mesh(v, f), side)
        assert rec == t and np.array_equal(cls_host, cls)
        geo = mp.mesh_geometry(Mesh(v, f), side)
        want = mref.geometry(v, f, cls)
        assert all(_bits(geo[k]) == _bits(want[i]) for i, k in enumerate(mp.GEOMETRY_FIELDS))
        assert geo["interface_length"] > 0.0 and geo["boundary_length"] == 0.0
    assert abs(mp.mesh_geometry(Mesh(v, f), mref.equator_side(f, v))["interface_length"] - 48 * np.sin(np.pi / 24)) < 1e-5   # the 24-gon of the equator


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def test_the_cube_is_exact(mp):
    v, f = mref.cube()
    g = mp.mesh_geometry(Mesh(v, f))
    assert g["area"] == 24.0 and g["signed_volume"] == 8.0 and g["edges"] == 18.0 and g["faces"] == 12.0
    assert g["min_edge"] == 2.0 and g["max_edge"] == np.sqrt(8.0) and g["min_face_area"] == g["max_face_area"] == 2.0
    assert mp.mesh_geometry(Mesh(v, f[:, ::-1].copy()))["signed_volume"] == -8.0
    moved = mp.mesh_geometry(Mesh(v, f), origin=(3.3, -1.7, 0.9))["signed_volume"]
    assert abs(moved - 8.0) <= 1e-12 * 8.0
    t, _ = mp.mesh_topology(Mesh(v, f))
    assert t["euler_characteristic"] == 2 and t["boundary_edges"] == t["misoriented_edges"] == 0


def test_geometry_bits_on_the_spheres(mp):
    for (v, f), origin, q_min in ((mref.uv_sphere(), None, 0.1), (mref.two_spheres(), (0.3, -2.0, 5.0), 0.5)):
        _, cls = mref.topology(f, len(v))
        got = mp._mesh_geometry_dev(mp._dev(v, np.float32, (3,)), mp._dev(f, np.int32, (3,)), mp._dev(cls, np.uint8, (3,)), origin, q_min).cpu().numpy()
        want = mref.geometry(v, f, cls, (0.0, 0.0, 0.0) if origin is None else origin, q_min)
        print(got)
        assert np.array_equal(_bits(got), _bits(want))
        assert got[11] > 0 if q_min == 0.5 else got[11] == 0                     # the polar slivers fall below 0.5, none below 0.1


def test_quality_of_an_equilateral_and_of_a_flat_face(mp):
    v = np.array([[0, 0, 0], [2, 0, 0], [1, np.sqrt(3.0), 0], [4, 0, 0]], np.float32)
    # q is stationary at the equilateral triangle: float32's rounding of sqrt 3 moves it by its square only
    g = mp.mesh_geometry(Mesh(v, np.array([[0, 1, 2]], np.int32)))
    assert abs(g["min_quality"] - 1.0) <= 1e-12 and g["mean_quality"] == g["min_quality"] and g["low_quality_faces"] == 0.0
    g = mp.mesh_geometry(Mesh(v, np.array([[0, 1, 3]], np.int32)))             # three points on a line
    assert g["min_quality"] == 0.0 and g["area"] == 0.0 and g["low_quality_faces"] == 1.0
    g = mp.mesh_geometry(Mesh(v, np.array([[0, 1, 2], [1, 1, 1]], np.int32)))  # all three corners the same point: the denominator is 0
    assert g["min_quality"] == 0.0 and g["faces"] == 2.0 and g["edges"] == 3.0


# ---- self-intersections --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brute():
    v, f = mref.two_spheres()
    pairs, flag = mref.self_intersections(v, f)
    flag.setflags(write=False)
    return pairs, flag


def test_two_spheres_equal_the_brute_force_under_every_grid(mp, brute):
    v, f = mref.two_spheres()
    pairs, flag = brute
    assert pairs == 124
    vd, fd = mp._dev(v, np.float32, (3,)), mp._dev(f, np.int32, (3,))
    seen = []
    for cell, cap in ((None, None), (0.05, 400 * len(f)), (100.0, None)):          # default, tiny, one cell for the whole mesh
        fl, rec = mp._mesh_self_intersections_dev(vd, fd, cell, cap)
        fl, rec = fl.cpu().numpy(), rec.cpu().numpy()
        print(cell, rec)
        assert rec[0] == pairs and rec[1] == flag.sum() and rec[3] == 0 and np.array_equal(fl, flag)
        seen.append((fl.tobytes(), rec[:2].tobytes(), int(rec[2])))
    assert seen[0][:2] == seen[1][:2] == seen[2][:2]
    assert seen[2][2] == len(f) and seen[0][2] <= 8 * len(f) < seen[1][2]
    again = mp._mesh_self_intersections_dev(vd, fd)
    assert again[0].cpu().numpy().tobytes() == seen[0][0] and again[1].cpu().numpy()[:2].tobytes() == seen[0][1]     # two runs, equal bytes
    rec, fl = mp.mesh_self_intersections(Mesh(v, f))
    assert rec["pairs"] == 124 and rec["flagged_faces"] == flag.sum() and np.array_equal(fl, flag)
    rec, fl = mp.mesh_self_intersections(Mesh(*mref.uv_sphere()))
    assert rec["pairs"] == 0 and rec["flagged_faces"] == 0 and not fl.any()


def test_an_undersized_workspace_overflows_and_flags_nothing(mp):
    v, f = mref.two_spheres()
    vd, fd = mp._dev(v, np.float32, (3,)), mp._dev(f, np.int32, (3,))
    fl, rec = mp._mesh_self_intersections_dev(vd, fd, 0.05, 2 * len(f))
    rec = rec.cpu().numpy()
    assert rec[3] == 1 and rec[2] > 2 * len(f) and rec[0] == 0 and rec[1] == 0 and not fl.cpu().numpy().any()
    with pytest.raises(Exception, match="overflow"):
        mp.mesh_self_intersections(Mesh(v, f), cell_size=0.05, max_entries=2 * len(f))


def test_the_predicate_on_two_triangles(mp):
    pts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [.5, .5, -1], [.5, .5, 1], [3, 3, 0]], np.float32)
    rec, fl = mp.mesh_self_intersections(Mesh(pts, np.array([[0, 1, 2], [3, 4, 5]], np.int32)))
    assert rec["pairs"] == 1 and rec["flagged_faces"] == 2 and fl.tolist() == [1, 1]
    assert mref.self_intersections(pts, [[0, 1, 2], [3, 4, 5]])[0] == 1
    # the second triangle names the first one's vertex 0 as its far corner: its edge still passes through the first, but faces that
    # share a vertex index are skipped; with a copy of that vertex under an index of its own the pair counts again
    rec, fl = mp.mesh_self_intersections(Mesh(pts, np.array([[0, 1, 2], [3, 4, 0]], np.int32)))
    assert rec["pairs"] == 0 and not fl.any()
    copy = np.concatenate([pts, pts[:1]])
    rec, fl = mp.mesh_self_intersections(Mesh(copy, np.array([[0, 1, 2], [3, 4, 6]], np.int32)))
    assert rec["pairs"] == 1 and fl.tolist() == [1, 1]
    # coplanar overlap, and an edge that only touches the other triangle's plane
    flat = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [.5, .5, 0], [3, .5, 0], [.5, 3, 0], [.5, .5, 0], [.5, .5, 1], [3, 3, 1]], np.float32)
    rec, fl = mp.mesh_self_intersections(Mesh(flat, np.array([[0, 1, 2], [3, 4, 5]], np.int32)))
    assert rec["pairs"] == 0
    rec, fl = mp.mesh_self_intersections(Mesh(flat, np.array([[0, 1, 2], [6, 7, 8]], np.int32)))
    assert rec["pairs"] == 0


def test_a_large_triangle_across_many_cells_counts_each_pair_once(mp):
    # 20 x 20 small upright triangles standing on a lattice, pierced by one large horizontal triangle that covers some of them
    small_v, small_f = [], []
    for i in range(20):
        for j in range(20):
            b = len(small_v)
            x, y = 0.5 * i, 0.5 * j
            small_v += [(x, y, -0.1), (x + 0.2, y, -0.1), (x + 0.1, y + 0.05, 0.2)]
            small_f.append((b, b + 1, b + 2))
    n = len(small_v)
    v = np.array(small_v + [(-1.0, -1.0, 0.0), (12.0, -1.0, 0.013), (-1.0, 12.0, 0.007)], np.float32)
    f = np.array(small_f + [(n, n + 1, n + 2)], np.int32)
    pairs, flag = mref.self_intersections(v, f)
    assert 100 < pairs < 400 and flag[-1] == 1 and flag.sum() == pairs + 1      # every pair is (a small one, the large one)
    vd, fd = mp._dev(v, np.float32, (3,)), mp._dev(f, np.int32, (3,))
    for cell, cap in ((None, None), (0.3, 200000), (0.11, 2000000)):
        fl, rec = mp._mesh_self_intersections_dev(vd, fd, cell, cap)
        rec = rec.cpu().numpy()
        print(cell, rec)
        assert rec[3] == 0 and rec[0] == pairs and np.array_equal(fl.cpu().numpy(), flag)
    assert rec[2] > 1000                                                        # the large triangle alone spans > 1000 cells of the finest grid


# ---- the stage -----------------------------------------------------------------------------------------------------------------------
def _same_quality(a, b):
    return dataclasses.asdict(a) == dataclasses.asdict(b)


@pytest.fixture(scope="module")
def stage():
    from test_morphometry_stage_gpu import MIN_CELLS, _cap, _slab
    from oai_analysis_2_amd.thickness import ThicknessAtlas
    atlas = ThicknessAtlas(_slab(1.5), _cap(), image_shape=(96, 128), min_cells=MIN_CELLS)
    maps = {"FC": torch.from_numpy(_slab(1.5).array).cuda(), "TC": torch.from_numpy(_cap().array).cuda(), "none": torch.zeros((8, 8, 8), device="cuda")}
    return atlas, maps, MIN_CELLS


def test_measure_fills_the_record_of_the_split_it_measured_on(mp, stage):
    from oai_analysis_2_amd import qc
    atlas, maps, min_cells = stage
    plain = atlas.measure(maps["FC"], maps["TC"])
    knee = atlas.measure(maps["FC"], maps["TC"], mesh_qc=True)
    assert plain.mesh_qc is None and set(knee.mesh_qc) == {"FC", "TC"} and knee.errors == {}
    for kind in ("FC", "TC"):
        assert np.array_equal(knee[kind].view(np.int32), plain[kind].view(np.int32))                  # the flag changes no bit of the thickness
        sq = knee.mesh_qc[kind]
        direct = qc.split_quality(mp._resident_split(maps[kind], atlas.spacing[kind], kind, min_cells[kind]))
        assert isinstance(sq, qc.SplitQuality) and _same_quality(sq, direct)
        print(kind, sq)
        assert sq.inner.faces + sq.outer.faces + sq.unassigned_faces == sq.whole.faces > 0
        assert sq.interface_edges == sq.whole.topology["interface_edges"] > 0 and sq.interface_loops >= 1 and sq.interface_length > 0.0
        assert sq.inner.topology["boundary_edges"] >= sq.interface_edges and not sq.inner.closed
        assert sq.whole.intersecting_pairs is not None and sq.whole.geometry["area"] > 0.0
    cap = knee.mesh_qc["TC"].whole
    assert cap.closed and cap.components == 1 and cap.genus_sum == 0 and cap.volume_mm3 > 0.0
    # the enclosed volume against the voxel count of the map it came from: the same set up to the half-voxel surface layer
    voxels = float((maps["TC"] > 0.5).sum().item())
    assert abs(cap.volume_mm3 - voxels) < 0.5 * cap.geometry["area"]
    # a cartilage that raised has no record; the other one is intact
    half = atlas.measure(maps["none"], maps["TC"], mesh_qc=True)
    assert set(half.mesh_qc) == {"TC"} and "FC" in half.errors and _same_quality(half.mesh_qc["TC"], knee.mesh_qc["TC"])


def test_pipeline_and_stream_carry_the_record(stage):
    from test_morphometry_stage_gpu import _small_pipe
    from oai_analysis_2_amd.dask_processing import thickness_stream
    from oai_analysis_2_amd.image import Image
    from oai_analysis_2_amd.pipeline import VolumeResult
    from oai_analysis_2_amd.synth import make_unet_state_dict, make_volume
    atlas, maps, _ = stage
    tiny = torch.zeros(1, device="cuda")
    direct = atlas.measure(maps["none"], maps["TC"], mesh_qc=True)
    got = list(thickness_stream(iter([(3, VolumeResult(tiny, tiny, tiny, maps["none"], maps["TC"]))]), atlas, mesh_qc=True))
    assert got[0][0] == 3 and set(got[0][1].mesh_qc) == {"TC"} and _same_quality(got[0][1].mesh_qc["TC"], direct.mesh_qc["TC"])
    off = list(thickness_stream(iter([(3, VolumeResult(tiny, tiny, tiny, maps["none"], maps["TC"]))]), atlas))
    assert off[0][1].mesh_qc is None and np.array_equal(off[0][1].tc.view(np.int32), got[0][1].tc.view(np.int32))
    pipe, shape = _small_pipe(make_unet_state_dict(1, width_div=2))
    vol = make_volume(9, shape)
    meta = Image(vol, [0.36, 0.37, 0.7], [1.0, 2.0, 3.0])
    v = torch.from_numpy(vol).cuda()
    plain = pipe.run(v, meta, thickness=atlas)
    on = pipe.run(v, meta, thickness=atlas, mesh_qc=True)
    ref = atlas.measure(on.fc_atlas, on.tc_atlas, spacing_xyz=pipe.atlas.spacing, mesh_qc=True)
    assert plain.thickness.mesh_qc is None and on.thickness.mesh_qc is not None and set(on.thickness.mesh_qc) == set(ref.mesh_qc)
    assert all(_same_quality(on.thickness.mesh_qc[k], ref.mesh_qc[k]) for k in ref.mesh_qc) and on.thickness.errors == plain.thickness.errors
    for kind in ("FC", "TC"):
        assert np.array_equal(on.thickness[kind].view(np.int32), plain.thickness[kind].view(np.int32))
