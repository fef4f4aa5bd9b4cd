"""GPU: the shared exclusive scan (csrc/mesh.hip) under its two volume users at and just past 2^20 elements, where it takes its third
level: mp.marching_cubes against oracle.mesh.marching_cubes and mp.cuberille_device against tests/cuberille_ref.py, faces and float32
vertices bit for bit.

  marching cubes  64 x 128 x 128   n = 2^20: 1024 block sums, level 2 is exactly one full block
                  65 x 128 x 128   n = 2^20 + 16384: 1040 block sums, three levels
  cuberille       64 x 128 x 128   scans n + 1 = 2^20 + 1: three levels, levels 1 and 2 both end in a block of one element
                  8 x 8 x 16       n + 1 = 1025: two blocks, the second of one element
(1024*64 - 1 and 1024*64 elements, round64(nb) on its boundary, are no volume product with every axis >= 2 that is worth a mesh of its
own: tests/test_scan_submesh_gpu.py has them.)

The input is a seeded sparse field: uniform noise below the level, and with probability DENSITY a voxel above it, so that every part of
the scan carries counts.  Before anything is compared the reference's own per-voxel counts must show that (``_assert_loads_the_scan``):
the first 1024-block and the last are non-zero, and every level-2 block (2^20 elements) holds at least 100 non-zero level-1 blocks.
Two of these cannot hold as stated and are asserted in the form the kernels allow: a cell of the last z plane has no triangle and the
last voxel owns no edge, so "the last block" is the last one that can hold a count; and the level-2 tail of 65 x 128 x 128 has 16 level-1
blocks (of cuberille's 2^20 + 1: the one closing element), so there "at least 100" is "all that can be non-zero".

DENSITY = 0.02 at the large shapes: about 121 000 vertices and 161 000 triangles from marching cubes, 157 000 vertices and 247 000
triangles from cuberille, and all but a handful of the level-1 blocks non-zero.  Host reference times, measured: oracle.mesh.marching_cubes
0.2 s per large shape, cuberille_ref.cuberille with the projection 1.3 s at 64 x 128 x 128 -- far below the ten seconds at which the
density would have had to come down."""
import numpy as np
import pytest

import cuberille_ref as ref
from oai_analysis_2_amd import mesh_processing as mp
from oai_analysis_2_amd.image import Image
from oracle import mesh as om

pytestmark = pytest.mark.gpu

DENSITY = 0.02
LEVEL = 0.5


def sparse_field(shape, density, seed):
    """Noise in [0, 0.4) and, with probability ``density``, a voxel in [0.6, 1); the first and the last voxel pairs planted above the level."""
    rng = np.random.default_rng(seed)
    v = rng.random(shape, dtype=np.float32) * np.float32(0.4)
    hot = rng.random(shape) < density
    hot.reshape(-1)[[0, -2]] = True                                # an x edge out of voxel 0 and one into the last voxel
    hot.reshape(-1)[[1, -1]] = False
    v[hot] = np.float32(0.6) + rng.random(int(hot.sum()), dtype=np.float32) * np.float32(0.4)
    return v


def _assert_loads_the_scan(counts, last_possible=None):
    """``counts``: what the scan adds up, per element.  ``last_possible``: the last element that can be non-zero at all."""
    counts = np.asarray(counts).reshape(-1)
    n = counts.size
    last_possible = n - 1 if last_possible is None else last_possible
    nb = -(-n // 1024)
    live = np.add.reduceat(counts, np.arange(0, n, 1024)) > 0
    assert live.shape == (nb,)
    assert live[0] and live[last_possible // 1024], "the first and the last 1024-block must carry counts"
    for b2 in range(-(-nb // 1024)):                               # level-2 blocks: 1024 level-1 blocks = 2^20 elements
        lo, hi = b2 * 1024, min((b2 + 1) * 1024, nb, last_possible // 1024 + 1)
        if hi > lo:
            assert live[lo:hi].sum() >= min(100, hi - lo), (b2, int(live[lo:hi].sum()), hi - lo)


def _mc_counts(vol, iso):
    """Per voxel: the vertices it owns and the triangles of the cell whose lowest corner it is, from the oracle's own conventions."""
    D, H, W = vol.shape
    ins = vol > np.float32(iso)
    vcount = np.zeros((D, H, W), np.int64)
    vcount[:, :, :-1] += ins[:, :, :-1] != ins[:, :, 1:]
    vcount[:, :-1, :] += ins[:, :-1, :] != ins[:, 1:, :]
    vcount[:-1, :, :] += ins[:-1, :, :] != ins[1:, :, :]
    case = np.zeros((D - 1, H - 1, W - 1), np.int32)
    for c in range(8):
        cx, cy, cz = om.corner_offset(c)
        case |= ins[cz:D - 1 + cz, cy:H - 1 + cy, cx:W - 1 + cx].astype(np.int32) << c
    ntri = (om.mc_table() >= 0).sum(axis=1) // 3
    tcount = np.zeros((D, H, W), np.int64)
    tcount[:-1, :-1, :-1] = ntri[case]
    return vcount, tcount


@pytest.mark.parametrize("shape", [(64, 128, 128), (65, 128, 128)])
def test_marching_cubes_at_three_scan_levels(shape):
    """DENSITY 0.02; oracle.mesh.marching_cubes takes about 0.2 s on the host at either shape."""
    D, H, W = shape
    vol = sparse_field(shape, DENSITY, seed=D)
    rv, rf = om.marching_cubes(vol, LEVEL, (0.36, 0.37, 0.7))
    vcount, tcount = _mc_counts(vol, LEVEL)
    assert vcount.sum() == len(rv) and tcount.sum() == len(rf)
    _assert_loads_the_scan(vcount, last_possible=D * H * W - 2)                                   # the last voxel owns no edge
    _assert_loads_the_scan(tcount, last_possible=((D - 2) * H + (H - 2)) * W + (W - 2))           # the last cell
    gv, gf = mp.marching_cubes(vol, LEVEL, (0.36, 0.37, 0.7))
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and gv.shape == rv.shape and gf.shape == rf.shape
    assert np.array_equal(gf, rf)
    assert gv.tobytes() == rv.tobytes()


@pytest.mark.parametrize("shape,density", [((64, 128, 128), DENSITY), ((8, 8, 16), 0.2)])
def test_cuberille_at_three_scan_levels(shape, density):
    """DENSITY 0.02 at 64 x 128 x 128 (0.2 at 8 x 8 x 16: two blocks need no sparseness); tests/cuberille_ref.cuberille with the
    projection takes about 1.3 s on the host at the large shape."""
    D, H, W = shape
    n = D * H * W
    vol = sparse_field(shape, density, seed=100 + D)
    vol.reshape(-1)[[0, -1]] = np.float32(0.9)                       # an inside voxel at either end: both have outside neighbours
    want = ref.cuberille(vol, LEVEL, spacing=(0.36, 0.37, 0.7))
    _, lattice, pairs = ref.faces_and_lattice(vol, LEVEL)
    fcount = np.bincount(pairs[:, 0], minlength=n)                   # quads per voxel: the first scan, over these and a closing 0
    assert fcount.sum() * 2 == len(want["faces"]) and len(lattice) == len(want["verts"])
    _assert_loads_the_scan(np.append(fcount, 0), last_possible=n - 1)
    v, f, k = mp.cuberille_device(Image(vol, (0.36, 0.37, 0.7)), LEVEL)
    v, f, k = v.cpu().numpy(), f.cpu().numpy(), k.cpu().numpy()
    assert f.dtype == np.int32 and np.array_equal(f, want["faces"])
    assert v.dtype == np.float32 and v.tobytes() == want["verts"].tobytes()
    assert np.array_equal(k, want["steps"])
