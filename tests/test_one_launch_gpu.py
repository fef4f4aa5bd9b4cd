"""GPU: option "one_launch" (an own-cover layer as ONE launch over the batch's live-block list: conv3_wino_list2 / conv3_wino_list1) changes no bit.
The geometries of tests/test_own_cover_gpu.py: odd x origins, both strip shapes, partial z blocks, boxes narrower than one main block.  Their batches are
below the option's size gate, so the tests set the force bit (one_launch = 7: both kernel families, forced)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oai_analysis_2_amd import _lib
from oai_analysis_2_amd.synth import make_unet_state_dict, make_volume

pytestmark = pytest.mark.gpu

# name -> (volume, tile, overlap, crop, number of tiles)
GEOMETRIES = {"A": ((28, 66, 154), (24, 40, 64), (6, 4, 8), (6, 4, 8), 36),
              "B": ((40, 72, 104), (16, 32, 48), (4, 4, 8), (4, 4, 8), 45)}
OWN = {"dc8": 9, "dc7": 10, "dc5": 12, "dc4": 13, "dc2": 15}


@pytest.fixture(scope="module")
def eng():
    from oai_analysis_2_amd.segmentation.engine import UNetEngine
    e = UNetEngine(make_unet_state_dict(seed=50, width_div=1), precision="fp16x3")
    yield e
    e.set_option("winograd", 19)
    e.set_option("one_launch", 1)


@pytest.fixture(scope="module")
def volumes():
    return {}


@pytest.fixture(scope="module")
def references():
    return {}


def _setup(eng, volumes, geo, wino, one):
    shape, tile, ovl, crop, n = GEOMETRIES[geo]
    if geo not in volumes:
        volumes[geo] = torch.from_numpy(make_volume(200, shape)).cuda()
    eng.set_option("winograd", wino)
    eng.set_option("one_launch", one)
    v = volumes[geo]
    seg = lambda batch, rng=None: eng.segment_tiles(v, tile, ovl, rng, 2, batch, crop)
    st = lambda b: eng.stitch(b, shape, tile, ovl, crop)
    return seg, st, n


def _reference(eng, volumes, references, geo, wino):
    """the stitched logits, the range flag and the census of one_launch = 0 (three launches per layer), computed once per geometry and tap form"""
    if (geo, wino) not in references:
        seg, st, n = _setup(eng, volumes, geo, wino, 0)
        seg(n)                                                       # (calibrates on the first call)
        eng.range_flag(), eng.census(reset=True)
        ref = st(seg(n))
        assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
        references[(geo, wino)] = (ref, eng.range_flag(), eng.census(reset=True), eng.act_exponents())
    return references[(geo, wino)]


@pytest.mark.parametrize("wino", [19, 51])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_one_launch_equals_three_launches(eng, volumes, references, geo, wino):
    ref, flag, census, exps = _reference(eng, volumes, references, geo, wino)
    seg, st, n = _setup(eng, volumes, geo, wino, 7)
    got = st(seg(n))
    assert torch.equal(got, ref)
    assert eng.range_flag() == flag and eng.census(reset=True) == census and eng.act_exponents() == exps
    for batch in (6, 1, 5):
        assert torch.equal(st(seg(batch)), ref), batch
    whole = seg(n)
    whole[5:19] = seg(7, (5, 19))
    assert torch.equal(st(whole), ref)
    assert eng.range_flag() == flag and eng.census(reset=True) == census


@pytest.mark.parametrize("bits", [1, 2])
def test_each_family_alone_equals_three_launches(eng, volumes, references, bits):
    ref = _reference(eng, volumes, references, "A", 19)[0]
    seg, st, n = _setup(eng, volumes, "A", 19, 4 | bits)
    assert torch.equal(st(seg(n)), ref)
    assert torch.equal(st(seg(5)), ref)


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_device_list_is_the_host_list(eng, volumes, geo):
    """What block_list_kernel left in the workspace for the last batch of a call, against oai_unet_block_list."""
    shape, tile, ovl, crop, n = GEOMETRIES[geo]
    seg, st, n = _setup(eng, volumes, geo, 19, 7)
    lib = _lib.load()
    for batch, end in ((n, n), (7, 20)):                             # (tiles [14, 20) are live in both geometries; a dead batch builds no list)
        seg(batch, (0, end))
        torch.cuda.synchronize()
        t0 = (end - 1) // batch * batch                              # the call's last batch
        for name, layer in OWN.items():
            count, off = C.c_int(), C.c_longlong()
            args = (*shape, _lib.int3(tile), _lib.int3(ovl), _lib.int3(crop), batch, t0, end - t0, layer)
            assert lib.oai_unet_block_list(*args, None, 0, C.byref(count), C.byref(off)) == 0
            words = (C.c_uint * count.value)()
            assert lib.oai_unet_block_list(*args, words, count.value, C.byref(count), None) == 0 and count.value > 0
            dev = eng._ws[off.value:off.value + 4 * count.value].cpu().numpy().view(np.uint32)
            assert np.array_equal(dev, np.array(words, dtype=np.uint32)), (name, batch)


def test_a_forced_run_records_fewer_launches_and_the_same_result(eng, volumes, references):
    ref = _reference(eng, volumes, references, "A", 19)[0]
    counts = {}
    for one in (0, 7):
        seg, st, n = _setup(eng, volumes, "A", 19, one)
        eng.profile(True)
        try:
            got = st(seg(n))
            counts[one] = eng.profile_read()[1]
        finally:
            eng.profile(False)
        assert torch.equal(got, ref), one
    print(f"timed launches: {counts}")
    assert 0 < counts[7] < counts[0] <= counts[7] + 2 * len(OWN)     # five layers, at most three launches each become one


def test_forward_tiles_is_unchanged_by_the_option(eng):
    """oai_unet_forward_tiles has no box table and no own cover: the option must not reach it."""
    x = torch.from_numpy(np.stack([make_volume(s, (24, 40, 64)) for s in (7, 8, 9)]))[:, None].cuda()
    eng.set_option("one_launch", 0)
    ref = eng.forward_tiles(x)
    eng.set_option("one_launch", 7)
    assert torch.equal(eng.forward_tiles(x), ref) and torch.isfinite(ref).all()
