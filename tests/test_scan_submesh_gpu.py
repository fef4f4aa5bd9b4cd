"""GPU: the shared exclusive scan (csrc/mesh.hip, oai::exclusive_scan_i32) probed through oai_mesh_submesh at its block and level
boundaries.  oai_mesh_submesh scans the n_faces + 1 flags ``side == which`` (the compacted face list must be np.flatnonzero of them) and
then the 3 m + 1 first-use flags (the vertex numbering); the host get_sub_mesh is the reference, bit for bit.

The mesh is a triangle strip: n_faces + 2 random float32 vertices, face i = (i, i + 1, i + 2).  Sizes, in 1024-element scan blocks:
  1, 2                      one partial block
  1023, 1024, 1025          n + 1 = 1024 (one full block), 1025 (a second block of one element), 1026
  2047, 2048                the same one block later
  1024*64 - 1, 1024*64      n + 1 = 65536 / 65537 flags: 64 / 65 block sums, round64(nb) on its own boundary (the scratch carving)
  2^20 - 1, 2^20, 2^20 + 1  n + 1 = 2^20 flags is the last size of two levels; from n = 2^20 on there are three (1025 block sums, then 2),
                            and at n = 2^20 both level 1 and level 2 end in a block of one element
  2^20 + 1025               three levels, every level with a ragged tail
The second scan runs over 3 m + 1 elements and so reaches three levels from m = 349 526 selected faces on."""
import functools

import numpy as np
import pytest
import torch

from oai_analysis_2_amd import mesh_processing as mp

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 1023, 1024, 1025, 2047, 2048, 1024 * 64 - 1, 1024 * 64, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 1025]
PATTERNS = ["all", "none", "first", "last", "alternating", "bernoulli", "block_ends"]


def _selection(pattern, n):
    sel = np.zeros(n, bool)
    if pattern == "all":
        sel[:] = True
    elif pattern == "first":
        sel[0] = True
    elif pattern == "last":
        sel[-1] = True
    elif pattern == "alternating":
        sel[::2] = True
    elif pattern == "bernoulli":
        sel = np.random.default_rng(n).random(n) < 0.5
    elif pattern == "block_ends":                              # one face per 1024-block, at the block's last position
        sel[1023::1024] = True
    return sel


@functools.lru_cache(maxsize=1)                                # the sizes run one after the other: one strip at a time on the device
def _strip(n_faces):
    verts = np.random.default_rng(1000 + n_faces % 997).random((n_faces + 2, 3), dtype=np.float32)
    faces = (np.arange(n_faces, dtype=np.int32)[:, None] + np.arange(3, dtype=np.int32)[None, :]).astype(np.int32)
    return mp.Mesh(verts, faces), torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n_faces", SIZES)
def test_sub_mesh_of_a_strip_equals_get_sub_mesh(n_faces, pattern):
    mesh, verts, faces = _strip(n_faces)
    sel = _selection(pattern, n_faces)
    assert pattern != "none" or not sel.any()
    face_list = np.flatnonzero(sel)
    m = len(face_list)
    side = torch.from_numpy(np.where(sel, 1, -1).astype(np.int8)).cuda()
    v, f, io = mp._sub_mesh_dev(mp.DeviceSplit(verts, faces, side, None, None, None), 1)
    assert io.dtype == torch.int32 and f.dtype == torch.int32 and v.dtype == torch.float32
    assert int(io.shape[0]) == int(f.shape[0]) == m                               # n_faces_out
    assert m > 0 or pattern != "all"
    if m == 0:                                                                   # the early return: nothing selected, no vertex used
        assert int(v.shape[0]) == 0
        return
    want = mp.get_sub_mesh(mesh, face_list)
    assert int(v.shape[0]) == len(want.verts)                                     # n_verts_out
    assert np.array_equal(io.cpu().numpy(), face_list)
    assert np.array_equal(f.cpu().numpy(), want.faces)
    assert v.cpu().numpy().tobytes() == want.verts.tobytes()
