"""CPU: the per-tile cover of option "own_cover" (csrc/unet.hip: tile_cover), counted by the host-only entry point oai_unet_cover_stats with the
functions the launcher and the device table use.  No GPU and no handle."""
import ctypes as C

import numpy as np
import pytest

from oai_analysis_2_amd import _lib
from oai_analysis_2_amd.segmentation.engine import tile_grid

DC9, DC8, DC7, DC6, DC5, DC4, DC3, DC2 = 8, 9, 10, 11, 12, 13, 14, 15
OWN = {"dc8": DC8, "dc7": DC7, "dc5": DC5, "dc4": DC4, "dc2": DC2}

# (volume, tile, overlap, crop, batch): the benchmark volume as one batch of 160 and the two ragged geometries of tests/test_own_cover_gpu.py
BENCH = ((160, 384, 384), (32, 128, 128), (8, 16, 16), (8, 16, 16), 160)
GEOMETRIES = {"bench": BENCH,
              "A": ((28, 66, 154), (24, 40, 64), (6, 4, 8), (6, 4, 8), 36),
              "B": ((40, 72, 104), (16, 32, 48), (4, 4, 8), (4, 4, 8), 45)}


def cover_stats(geometry, layer, batch=None):
    shape, tile, ovl, crop, b = geometry
    n = tile_grid(shape, tile, ovl)[2]
    stats, pieces = (C.c_double * 3)(), (C.c_int * (24 * n))()
    rc = _lib.load().oai_unet_cover_stats(*shape, _lib.int3(tile), _lib.int3(ovl), _lib.int3(crop), batch or b, layer, stats, pieces, n)
    assert rc == 0, _lib.load().oai_last_error()
    return list(stats), np.array(pieces, dtype=np.int64).reshape(n, 4, 2, 3)


def _voxels(box):
    ext = box[1] - box[0]
    return 0 if (ext <= 0).any() else int(ext.prod())


@pytest.mark.parametrize("layer", sorted(OWN))
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_pieces_partition_every_tile_box(geo, layer):
    """The three pieces of every tile are disjoint, lie inside the tile's box and add up to it -- for every batch size too: the pieces are the tile's own."""
    stats, rows = cover_stats(GEOMETRIES[geo], OWN[layer])
    assert np.array_equal(rows, cover_stats(GEOMETRIES[geo], OWN[layer], batch=5)[1])
    live = 0
    for box, *pieces in rows:
        if _voxels(box) == 0:
            assert all(_voxels(p) == 0 for p in pieces)
            continue
        live += 1
        seen = np.zeros(tuple(box[1] - box[0]), dtype=np.int32)
        for p in pieces:
            if _voxels(p) == 0:
                continue
            assert (p[0] >= box[0]).all() and (p[1] <= box[1]).all()
            lo, hi = p[0] - box[0], p[1] - box[0]
            seen[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] += 1
        assert (seen == 1).all()
        main, xs, ys = pieces
        assert _voxels(main) > 0                                                        # a live tile always has main blocks
        if _voxels(xs):                                                                 # strips: a remainder of <= 4 behind whole main blocks, x start even
            assert xs[0][2] % 2 == 0 and 0 < xs[1][2] - xs[0][2] <= 4 and (xs[0][2] - (box[0][2] & ~1)) % 8 == 0 and xs[0][2] > box[0][2]
        if _voxels(ys):
            assert 0 < ys[1][1] - ys[0][1] <= 4 and (ys[0][1] - box[0][1]) % 8 == 0 and ys[0][1] > box[0][1] and ys[1][2] == main[1][2]
    assert live > 0 and stats[0] == sum(_voxels(r[0]) for r in rows)


@pytest.mark.parametrize("batch", [None, 1, 7])
@pytest.mark.parametrize("layer", sorted(OWN) + ["dc9", "dc6", "dc3"])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_own_cover_executes_no_more_than_the_union_and_no_less_than_needed(geo, layer, batch):
    need, union, own = cover_stats(GEOMETRIES[geo], {**OWN, "dc9": DC9, "dc6": DC6, "dc3": DC3}[layer], batch)[0]
    assert 0 < need <= own <= union


# the table of the issue that introduced the option (benchmark geometry, one batch of 160): needed, executed with the union's placement, and the least
# reduction own cover must bring (margins under the derived 12.1 / 10.7 / 3.6 / 3.6 / 2.0 %)
TABLE = {"dc8": ("9.78e5", "1.294e6", 0.10), "dc7": ("8.22e5", "9.585e5", 0.09), "dc5": ("4.129e6", "4.372e6", 0.03),
         "dc4": ("3.115e6", "3.592e6", 0.03), "dc2": ("2.125e7", "2.280e7", 0.015)}
UP_TABLE = {"dc6": ("8.22e5", "9.544e5"), "dc3": ("3.115e6", "3.695e6")}


def _digits(value, printed):
    """`value` rounds to the printed figure, at the figure's own number of digits."""
    mant = printed.split("e")[0]
    decimals = len(mant.split(".")[1]) if "." in mant else 0
    m, e = f"{value:.{decimals}e}".split("e")
    return float(m) == float(mant) and int(e) == int(printed.split("e")[1])


@pytest.mark.parametrize("layer", sorted(TABLE))
def test_benchmark_geometry_reproduces_the_table_and_the_reduction(layer):
    need, union, own = cover_stats(BENCH, OWN[layer])[0]
    print(f"{layer}: needed {need:.4e}  union {union:.4e} ({100 * (1 - need / union):.1f} % waste)  own {own:.4e}  change {100 * (own / union - 1):.1f} %")
    printed_need, printed_union, least = TABLE[layer]
    assert _digits(need, printed_need), (need, printed_need)
    assert _digits(union, printed_union), (union, printed_union)
    assert 1.0 - own / union >= least, (own, union)


@pytest.mark.parametrize("layer", sorted(UP_TABLE))
def test_benchmark_geometry_reproduces_the_up_conv_rows(layer):
    need, union, own = cover_stats(BENCH, {"dc6": DC6, "dc3": DC3}[layer])[0]
    print(f"{layer}: needed rows {need:.4e}  union {union:.4e} ({100 * (1 - need / union):.1f} % dead)  own {own:.4e} ({100 * (1 - need / own):.1f} % dead)")
    assert _digits(need, UP_TABLE[layer][0]) and _digits(union, UP_TABLE[layer][1]), (need, union)
    assert 1.0 - need / own < 0.01                                                     # own box: only the last workgroup of a tile has dead rows


def test_bad_arguments_are_reported():
    lib = _lib.load()
    stats = (C.c_double * 3)()
    t, o = _lib.int3((32, 128, 128)), _lib.int3((8, 16, 16))
    assert lib.oai_unet_cover_stats(160, 384, 384, t, o, o, 160, 16, stats, None, 0) != 0 and b"layer" in lib.oai_last_error()      # dc1 has whole boxes
    assert lib.oai_unet_cover_stats(160, 384, 384, t, o, o, 0, DC8, stats, None, 0) != 0
    assert lib.oai_unet_cover_stats(160, 384, 384, t, None, o, 160, DC8, stats, None, 0) != 0
    assert lib.oai_unet_cover_stats(160, 384, 384, t, o, o, 160, DC8, stats, (C.c_int * 24)(), 1) != 0                                # 160 tiles, not 1
