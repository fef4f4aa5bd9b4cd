"""CPU: the live-block list of option "one_launch" (csrc/unet.hip: block_list_host / block_list_kernel), as the host-only entry point oai_unet_block_list
gives it, against the pieces of every tile's own cover from oai_unet_cover_stats.  No GPU and no handle."""
import ctypes as C
import os

import numpy as np
import pytest

from oai_analysis_2_amd import _lib
from oai_analysis_2_amd.segmentation.engine import tile_grid

OWN = {"dc8": 9, "dc7": 10, "dc5": 12, "dc4": 13, "dc2": 15}
SHAPES = ((8, 8), (16, 4), (4, 16))                 # (TY, TX) of a main block, an x-strip block, a y-strip block; 4 z slices each
CUS = 256                                           # compute units of an MI355X: the size gate of the option

# (volume, tile, overlap, crop): the ragged geometries of tests/test_own_cover_gpu.py and the benchmark's
GEOMETRIES = {"A": ((28, 66, 154), (24, 40, 64), (6, 4, 8), (6, 4, 8)),
              "B": ((40, 72, 104), (16, 32, 48), (4, 4, 8), (4, 4, 8)),
              "bench": ((160, 384, 384), (32, 128, 128), (8, 16, 16), (8, 16, 16))}


def pieces(geometry, layer):
    shape, tile, ovl, crop = geometry
    n = tile_grid(shape, tile, ovl)[2]
    stats, rows = (C.c_double * 3)(), (C.c_int * (24 * n))()
    assert _lib.load().oai_unet_cover_stats(*shape, _lib.int3(tile), _lib.int3(ovl), _lib.int3(crop), n, layer, stats, rows, n) == 0
    return np.array(rows, dtype=np.int64).reshape(n, 4, 2, 3)[:, 1:]          # [tile][shape][lo / hi][z y x]


def block_list(geometry, layer, batch, tile_begin, n):
    shape, tile, ovl, crop = geometry
    lib, count, off = _lib.load(), C.c_int(), C.c_longlong()
    args = (*shape, _lib.int3(tile), _lib.int3(ovl), _lib.int3(crop), batch, tile_begin, n, layer)
    assert lib.oai_unet_block_list(*args, None, 0, C.byref(count), C.byref(off)) == 0, lib.oai_last_error()
    words = (C.c_uint * max(1, count.value))()
    assert lib.oai_unet_block_list(*args, words, count.value, C.byref(count), None) == 0, lib.oai_last_error()
    w = np.array(words, dtype=np.int64)[:count.value]
    return np.stack([w >> 20, (w >> 18) & 3, (w >> 12) & 63, (w >> 6) & 63, w & 63], axis=1), off.value      # tile, shape, bz, by, bx


def live_blocks(piece, s):
    """(bz, by, bx) of the blocks of shape s that hold a voxel of the piece, counted from the piece's corner (x rounded down to even)."""
    lo, hi = piece
    if (hi <= lo).any():
        return []
    ty, tx = SHAPES[s]
    org, ext = (lo[0], lo[1], lo[2] & ~1), (4, ty, tx)
    nb = [-(-(hi[i] - org[i]) // ext[i]) for i in range(3)]
    out = []
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                b = (bz, by, bx)
                blo = [max(lo[i], org[i] + b[i] * ext[i]) for i in range(3)]
                bhi = [min(hi[i], org[i] + (b[i] + 1) * ext[i]) for i in range(3)]
                assert all(h > l for l, h in zip(blo, bhi)), "a block of the grid that misses its piece"
                out.append(b)
    return out


def batches(n, batch):
    return [(t, min(batch, n - t)) for t in range(0, n, batch)]


@pytest.mark.parametrize("batch", ["n", 6, 1])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_list_is_every_live_block_once_in_order(geo, batch):
    g = GEOMETRIES[geo]
    ntiles = tile_grid(*g[:3])[2]
    b = ntiles if batch == "n" else batch
    for name, layer in OWN.items():
        pc, total = pieces(g, layer), 0
        for t0, n in batches(ntiles, b)[:: 1 if geo != "bench" or b != 1 else 7]:      # (the benchmark's 160 single-tile batches: every seventh)
            got, _ = block_list(g, layer, b, t0, n)
            want = [(t, s, *blk) for s in range(3) for t in range(n) for blk in live_blocks(pc[t0 + t][s], s)]
            # the list in the order asked for -- mains (tile-major, a tile's blocks as its launch numbers them: bx fastest), x strips, y strips --
            # which makes it the set of live blocks, each once, none dead, and its length the sum of the tiles' block counts
            assert len(got) == len(want), (name, t0)
            total += len(got)
            if not want:                                                                # (a batch of tiles whose kept centre lies outside the image)
                continue
            assert np.array_equal(got, np.array(want, dtype=np.int64)), (name, t0)
            assert len(set(map(tuple, got))) == len(got)
            assert (np.diff(got[:, 1]) >= 0).all()                                      # mains before x strips before y strips
        assert total > 0


@pytest.mark.parametrize("ncb", [1, 2, 4])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_xcd_shares_of_the_live_blocks_differ_by_at_most_one_deal(geo, ncb):
    """xcd_block_id over the list index: workgroup w of the grid (rounded up to whole deals of G ids to each of 8 XCDs) runs on XCD w % 8 and takes id
    ((w // 8 // G) * 8 + w % 8) * G + w // 8 % G; ids >= the live count are padding."""
    g, G = GEOMETRIES[geo], 32
    ntiles = tile_grid(*g[:3])[2]
    for layer in OWN.values():
        nblocks = len(block_list(g, layer, ntiles, 0, ntiles)[0]) * ncb
        w = np.arange(-(-nblocks // (8 * G)) * 8 * G)
        ids = ((w // 8 // G) * 8 + w % 8) * G + (w // 8) % G
        assert np.array_equal(np.sort(ids[ids < nblocks]), np.arange(nblocks))          # every live id exactly once
        share = np.bincount(w[ids < nblocks] % 8, minlength=8)
        assert share.max() - share.min() <= G, share


def test_the_pinned_small_batches_stay_under_the_size_gate():
    """tests/test_unet_gpu.py counts the timed launches of batches of 9 tiles of a 24 x 72 x 72 volume: no own-cover layer of such a batch has as many
    live blocks as the device has CUs, so without the force bit they keep their three launches."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segment_small.npz"))
    patch, ovl = tuple(int(v) for v in z["patch"]), tuple(int(v) for v in z["overlap"])
    g = ((24, 72, 72), patch[::-1], ovl[::-1], (ovl[2], ovl[0], ovl[1]))
    ntiles = tile_grid(*g[:3])[2]
    for name, layer in OWN.items():
        counts = [len(block_list(g, layer, 9, t0, n)[0]) for t0, n in batches(ntiles, 9)]
        print(f"{name}: live blocks per batch of 9 tiles {counts}")
        assert max(counts) < CUS and sum(counts) > 0
    bench = GEOMETRIES["bench"]
    assert all(len(block_list(bench, layer, 160, 0, 160)[0]) >= 1000 for layer in OWN.values())      # ... and the benchmark's batch is far above it


def test_workspace_offsets_and_bad_arguments():
    lib, g = _lib.load(), GEOMETRIES["A"]
    offs = [block_list(g, layer, 36, 0, 36)[1] for layer in OWN.values()]
    table = 33 * 4096 * 6 * 4                                                           # the box table comes first: 18 + 3 x 5 rows of 4096 tiles
    assert offs[0] == table and all(b > a and b % 256 == 0 for a, b in zip(offs, offs[1:]))
    assert offs[1] - offs[0] >= 4 * len(block_list(g, OWN["dc2"], 36, 0, 36)[0])         # every layer has the room of the longest list (dc2's)
    n, t, o = C.c_int(), _lib.int3(g[1]), _lib.int3(g[2])
    assert lib.oai_unet_block_list(*g[0], t, o, o, 36, 0, 36, 16, None, 0, C.byref(n), None) != 0 and b"layer" in lib.oai_last_error()
    assert lib.oai_unet_block_list(*g[0], t, o, o, 36, 30, 36, 9, None, 0, C.byref(n), None) != 0      # tiles 30..65 of 36
    assert lib.oai_unet_block_list(*g[0], t, o, o, 6, 0, 7, 9, None, 0, C.byref(n), None) != 0         # more tiles than the batch
    assert lib.oai_unet_block_list(*g[0], t, o, o, 36, 0, 36, 9, (C.c_uint * 1)(), 1, C.byref(n), None) != 0 and n.value > 1
