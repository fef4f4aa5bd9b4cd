"""GPU: option "own_cover" (blocks of the trimmed decoder convs on every tile's own cover, up-conv rows of every tile's own input box) changes no bit.
Ragged geometries whose decoder boxes have odd x origins, both strip shapes, remainders above and below the strip limit, boxes narrower than one main
block and partial z blocks (counted on the CPU: tests/test_own_cover_cpu.py)."""
import pytest
import torch

from oai_analysis_2_amd.synth import make_unet_state_dict, make_volume

pytestmark = pytest.mark.gpu

# name -> (volume, tile, overlap, crop, number of tiles)
GEOMETRIES = {"A": ((28, 66, 154), (24, 40, 64), (6, 4, 8), (6, 4, 8), 36),
              "A-crop-of-the-batching-test": ((28, 66, 154), (24, 40, 64), (6, 4, 8), (6, 8, 4), 36),
              "B": ((40, 72, 104), (16, 32, 48), (4, 4, 8), (4, 4, 8), 45)}


@pytest.fixture(scope="module")
def eng():
    from oai_analysis_2_amd.segmentation.engine import UNetEngine
    return UNetEngine(make_unet_state_dict(seed=50, width_div=1), precision="fp16x3")


@pytest.fixture(scope="module")
def volumes():
    return {}


def _setup(eng, volumes, geo, wino, own):
    shape, tile, ovl, crop, n = GEOMETRIES[geo]
    if geo not in volumes:
        volumes[geo] = torch.from_numpy(make_volume(200, shape)).cuda()
    eng.set_option("winograd", wino)
    eng.set_option("own_cover", own)
    v = volumes[geo]
    seg = lambda batch, rng=None: eng.segment_tiles(v, tile, ovl, rng, 2, batch, crop)
    st = lambda b: eng.stitch(b, shape, tile, ovl, crop)
    return seg, st, n


@pytest.mark.parametrize("wino", [19, 51])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_own_cover_equals_the_union_cover(eng, volumes, geo, wino):
    seg, st, n = _setup(eng, volumes, geo, wino, 0)
    ref = st(seg(n))
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
    seg, st, n = _setup(eng, volumes, geo, wino, 1)
    try:
        for batch in (n, 6):
            assert torch.equal(st(seg(batch)), ref), batch
    finally:
        eng.set_option("winograd", 19)


@pytest.mark.parametrize("wino", [19, 51])
@pytest.mark.parametrize("geo", ["A", "B"])
def test_own_cover_does_not_depend_on_the_batch_or_the_tile_range(eng, volumes, geo, wino):
    seg, st, n = _setup(eng, volumes, geo, wino, 1)
    try:
        ref = st(seg(n))
        for batch in (1, 5):
            assert torch.equal(st(seg(batch)), ref), batch
        whole = seg(n)
        whole[5:19] = seg(7, (5, 19))
        assert torch.equal(st(whole), ref)
    finally:
        eng.set_option("winograd", 19)


def test_forward_tiles_is_unchanged_by_the_option(eng):
    """oai_unet_forward_tiles has no box table: the option must not reach it."""
    import numpy as np
    x = torch.from_numpy(np.stack([make_volume(s, (24, 40, 64)) for s in (7, 8, 9)]))[:, None].cuda()
    eng.set_option("own_cover", 0)
    ref = eng.forward_tiles(x)
    eng.set_option("own_cover", 1)
    assert torch.equal(eng.forward_tiles(x), ref) and torch.isfinite(ref).all()
