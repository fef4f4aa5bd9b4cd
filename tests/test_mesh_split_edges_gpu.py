"""GPU: the device inner / outer split (csrc/mesh_split.hip) against its restatement (tests/mesh_split_ref.py) on the small meshes of
tests/mesh_split_cases.py, which tests/test_mesh_split_edges_cpu.py shows to be decided in fp64 and to reach the edges of the file:
sizes around a wave, the workgroup and the cumulative-sum tile, every ending of the Lloyd loop, the best-of-init rule, both
orientations, side 0, hand-picked draws, the empty-cluster error, the second pass of the min / max reduction, the sequential column
sum, and get_vtk_sub_mesh on hand-made side arrays.  The three entry points are driven through _lib.call, as
mesh_processing._split_dev drives them, so that the draws, n_init and max_iter can be chosen.  Every face is compared."""
import ctypes as C

import numpy as np
import pytest

import mesh_split_cases as mc
import mesh_split_ref as sref

pytestmark = pytest.mark.gpu

MESH_TYPE = {"FC": 0, "TC": 1}
N_INITS, MAX_ITERS = (1, 5), (1, 2, 300)
CASES = {c.name: c for c in mc.cases()}


class Features:
    """oai_mesh_split_features on a mesh, with a workspace for five inits; kmeans() may then be called any number of times"""

    def __init__(self, verts, faces, mesh_type):
        import torch
        from oai_analysis_2_amd import _lib
        self.lib, self.kind, self.dev = _lib, MESH_TYPE[mesh_type], torch.device("cuda", 0)
        self.v = torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(self.dev)
        self.f = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(self.dev)
        self.nv, self.nf = len(verts), len(faces)
        self.ws = _lib.workspace("oai_mesh_split", self.dev, self.nv, self.nf, self.kind, 5)
        self.cent = torch.empty((self.nf, 3), dtype=torch.float64, device=self.dev)
        self.nrm = torch.empty((self.nf, 3), dtype=torch.float64, device=self.dev)
        self.counts = (C.c_longlong * 3)()
        _lib.call("oai_mesh_split_features", self.v.data_ptr(), self.nv, self.f.data_ptr(), self.nf, self.kind, self.ws.data_ptr(), self.ws.numel(),
                  self.cent.data_ptr(), self.nrm.data_ptr(), self.counts, _lib.STREAM, device=self.dev)
        self.sizes = list(self.counts)[:3 if mesh_type == "FC" else 1]

    def stats(self):
        """What the features call left at the head of the workspace: the column sums of the centroids, then their least and greatest
        and the vertices' (struct Stats: double csum[3], cmin[3], cmax[3], float vmin[3], vmax[3]).  This follows the carve order of
        csrc/mesh_split.hip: Stats is the first thing carve() takes from the workspace."""
        head = self.ws[:96].cpu().numpy()
        d, f = head[:72].view(np.float64), head[72:].view(np.float32)
        return d[0:3], d[3:6], d[6:9], f[0:3], f[3:6]

    def kmeans(self, n_init, max_iter, slab_draws=None):
        """(side, n_iter per slab) of oai_mesh_split_kmeans; the draws RandomState(5)'s, as the product's, unless given"""
        import torch
        first, uni = [], []
        for s, n in enumerate(self.sizes):
            f, u = slab_draws[s] if slab_draws is not None else sref.draws(int(n), n_init)
            first += [int(x) for x in f]
            uni += [float(x) for x in np.asarray(u, np.float64).reshape(-1)]
        assert len(first) == len(self.sizes) * n_init
        side = torch.full((self.nf,), 77, dtype=torch.int8, device=self.dev)
        n_iter = (C.c_int * 3)()
        self.lib.call("oai_mesh_split_kmeans", self.nf, self.kind, self.ws.data_ptr(), self.ws.numel(), self.nrm.data_ptr(), n_init, max_iter,
                      self.counts, (C.c_longlong * len(first))(*first), (C.c_double * len(uni))(*uni), side.data_ptr(), n_iter, self.lib.STREAM,
                      device=self.dev)
        return side.cpu().numpy(), np.array(list(n_iter)[:len(self.sizes)])


def _check_features(feat, verts, faces, mesh_type):
    cent, nrm = feat.cent.cpu().numpy(), feat.nrm.cpu().numpy()
    assert np.array_equal(cent.view(np.uint64), sref.cell_centroids(verts, faces).view(np.uint64))
    assert np.array_equal(nrm.view(np.uint64), sref.cell_normals(verts, faces).view(np.uint64))
    masks = sref.features(verts, faces, mesh_type)[1]
    assert feat.sizes == masks.sum(axis=1).tolist()


@pytest.mark.parametrize("name", list(CASES))
def test_sides_and_iterations_are_the_restatement_on_every_face(name):
    case = CASES[name]
    feat = Features(case.verts, case.faces, case.mesh_type)
    _check_features(feat, case.verts, case.faces, case.mesh_type)
    for n_init in N_INITS:
        for max_iter in MAX_ITERS:
            want_side, want_iter, _ = sref.split_sides_draws(case.verts, case.faces, case.mesh_type, n_init, max_iter)
            side, n_iter = feat.kmeans(n_init, max_iter)
            what = f"{name} n_init={n_init} max_iter={max_iter}"
            assert np.array_equal(n_iter, want_iter), what
            assert np.array_equal(side, want_side), f"{what}: {int((side != want_side).sum())} of {len(side)} faces differ"


@pytest.mark.parametrize("name", mc.HAND_DRAW_MESHES)
def test_hand_picked_draws_and_the_empty_cluster_error(name):
    from oai_analysis_2_amd._lib import OaiError
    case = CASES[name]
    feat = Features(case.verts, case.faces, case.mesh_type)
    for kind in ("clip", "zero", "last"):
        draws = mc.hand_draws(kind, feat.sizes)
        want_side, want_iter, _ = sref.split_sides_draws(case.verts, case.faces, case.mesh_type, 1, 300, draws)
        side, n_iter = feat.kmeans(1, 300, draws)
        assert np.array_equal(n_iter, want_iter) and np.array_equal(side, want_side), f"{name} {kind}"
    with pytest.raises(OaiError, match="became empty"):
        feat.kmeans(1, 300, mc.hand_draws("empty", feat.sizes))
    want_side, want_iter, _ = sref.split_sides_draws(case.verts, case.faces, case.mesh_type, 1, 300)
    side, n_iter = feat.kmeans(1, 300)                               # the call after the error is an ordinary one
    assert np.array_equal(n_iter, want_iter) and np.array_equal(side, want_side)


@pytest.mark.parametrize("mesh_type", ["FC", "TC"])
def test_extremes_past_the_first_stride_of_the_min_max_reduction(mesh_type):
    case = mc.big_case(mesh_type)
    feat = Features(case.verts, case.faces, mesh_type)
    _check_features(feat, case.verts, case.faces, mesh_type)
    c = sref.cell_centroids(case.verts, case.faces)
    csum, cmin, cmax, vmin, vmax = feat.stats()
    assert np.array_equal(cmin, c.min(axis=0)) and np.array_equal(cmax, c.max(axis=0))
    assert np.array_equal(vmin, case.verts.min(axis=0)) and np.array_equal(vmax, case.verts.max(axis=0))
    assert np.array_equal(csum.view(np.uint64), np.add.accumulate(c, axis=0)[-1].view(np.uint64))
    want_side, want_iter, _ = sref.split_sides_draws(case.verts, case.faces, mesh_type)
    side, n_iter = feat.kmeans(5 if mesh_type == "FC" else 1, 300)
    assert np.array_equal(n_iter, want_iter) and np.array_equal(side, want_side)


@pytest.mark.parametrize("n", mc.SUM_SIZES)
def test_column_sum_is_numpys_row_after_row(n):
    verts, faces = mc.cut(600 + n, n, True)
    feat = Features(verts, faces, "TC")
    c = sref.cell_centroids(verts, faces)
    want = np.add.accumulate(c, axis=0)[-1]
    if n >= 4095:                                                    # the order of the sum shows in its bits: numpy's pairwise sum differs
        assert not np.array_equal(want, np.ascontiguousarray(c.T).sum(axis=1))
    assert np.array_equal(feat.stats()[0].view(np.uint64), want.view(np.uint64))


def test_faces_that_index_past_the_vertices_are_an_error_and_the_next_call_succeeds():
    from oai_analysis_2_amd._lib import OaiError
    verts, faces = mc.bad_indices(420)
    with pytest.raises(OaiError, match="indexes outside"):
        Features(verts, faces, "FC")
    with pytest.raises(OaiError, match="indexes outside"):
        Features(verts, faces, "TC")
    case = CASES["sheets-fc-513"]
    feat = Features(case.verts, case.faces, "FC")
    _check_features(feat, case.verts, case.faces, "FC")
    want_side, want_iter, _ = sref.split_sides_draws(case.verts, case.faces, "FC")
    side, n_iter = feat.kmeans(5, 300)
    assert np.array_equal(n_iter, want_iter) and np.array_equal(side, want_side)


def test_three_repeats_give_identical_bytes():
    case = CASES["sheets-fc-4097"]
    runs = []
    for _ in range(3):
        feat = Features(case.verts, case.faces, "FC")
        side, n_iter = feat.kmeans(5, 300)
        runs.append((side.tobytes(), n_iter.tobytes(), feat.cent.cpu().numpy().tobytes(), feat.nrm.cpu().numpy().tobytes(),
                     feat.ws[:96].cpu().numpy().tobytes()))
    assert runs[1] == runs[0] and runs[2] == runs[0]


# ---- oai_mesh_submesh on hand-made side arrays ---------------------------------------------------------------------------------------
def _sub_mesh_device(verts, faces, side, which):
    import torch
    from oai_analysis_2_amd import _lib
    dev = torch.device("cuda", 0)
    nv, nf = len(verts), len(faces)
    v, f, s = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (verts, faces, side))
    ws = _lib.workspace("oai_mesh_submesh", dev, nv, nf)
    vo = torch.full((nv, 3), np.nan, dtype=torch.float32, device=dev)
    fo = torch.full((nf, 3), -7, dtype=torch.int32, device=dev)
    io = torch.full((nf,), -7, dtype=torch.int32, device=dev)
    n_v, n_f = C.c_longlong(-1), C.c_longlong(-1)
    _lib.call("oai_mesh_submesh", v.data_ptr(), nv, f.data_ptr(), nf, s.data_ptr(), int(which), ws.data_ptr(), ws.numel(), vo.data_ptr(),
              fo.data_ptr(), io.data_ptr(), C.byref(n_v), C.byref(n_f), _lib.STREAM, device=dev)
    return vo[:n_v.value].cpu().numpy(), fo[:n_f.value].cpu().numpy(), io[:n_f.value].cpu().numpy(), n_v.value, n_f.value


def _check_sub_mesh(verts, faces, side, which):
    want_list = np.flatnonzero(side == which)
    v, f, lst, n_v, n_f = _sub_mesh_device(verts, faces, side, which)
    what = f"{len(faces)} faces, which={which}"
    assert n_f == len(want_list), what
    assert np.array_equal(lst, want_list), what
    if len(want_list) == 0:
        assert n_v == 0, what
        return
    want_v, want_f = sref.sub_mesh(verts, faces, want_list)
    assert n_v == len(want_v), what
    assert np.array_equal(v.view(np.uint32), want_v.view(np.uint32)), what
    assert np.array_equal(f, want_f), what


SIDE_VALUES = np.array([-1, 1, 0, 5, -128], np.int8)


@pytest.mark.parametrize("n_faces", [1, 255, 256, 257, 70000])
def test_sub_mesh_of_a_hand_made_side_array(n_faces):
    """random faces (some repeat a vertex) on more vertices than they use, every side value in the array, every value asked for"""
    rng = np.random.default_rng(n_faces)
    n_verts = max(3, n_faces // 2 + 40)
    verts = rng.normal(size=(n_verts + 25, 3)).astype(np.float32)           # the last 25 vertices: in no face at all
    faces = rng.integers(0, n_verts, (n_faces, 3)).astype(np.int32)
    faces[::7, 1] = faces[::7, 0]                                            # faces (v, v, w)
    side = SIDE_VALUES[rng.integers(0, len(SIDE_VALUES), n_faces)]
    for which in SIDE_VALUES:
        _check_sub_mesh(verts, faces, side, int(which))
    _check_sub_mesh(verts, faces, np.full(n_faces, 1, np.int8), 1)           # all selected
    _check_sub_mesh(verts, faces, np.full(n_faces, 1, np.int8), -1)          # none selected: counts 0, 0
    _check_sub_mesh(verts, faces, np.full(n_faces, -128, np.int8), -128)


@pytest.mark.parametrize("n_faces", [257, 70000])
def test_sub_mesh_of_a_fan_round_one_vertex(n_faces):
    """vertex 3 is in every face, as its first, second or third corner: every selected face bids for its first use"""
    rng = np.random.default_rng(n_faces + 1)
    verts = rng.normal(size=(n_faces + 10, 3)).astype(np.float32)
    rim = 4 + np.arange(n_faces)
    faces = np.stack([np.full(n_faces, 3), rim, rim + 1], axis=1).astype(np.int32)
    faces = np.stack([np.roll(row, k) for row, k in zip(faces, rng.integers(0, 3, n_faces))])
    side = SIDE_VALUES[rng.integers(0, 2, n_faces)]
    for which in (-1, 1, 0):
        _check_sub_mesh(verts, faces, side, which)
    _check_sub_mesh(verts, faces, np.full(n_faces, -1, np.int8), -1)
