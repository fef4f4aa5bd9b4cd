"""GPU: the three ICON tallUNet2 nets against a float64 run of oracle.icon.tall_unet2, in units of the fp32 oracle's own distance from
it (tests/unet_truth_ref.py).  tests/test_icon_gpu.py gates the same outputs at 1e-4 of their maximum, about 100 x the oracle's fp32
noise.  The project holds no truth multiple for these fp32 MFMA nets: sum|e| and rms are gated at the ceiling multiple 3.5 per output
channel, over all voxels and over the regions ``shell`` (fewer than 2 voxels from a face) and ``interior``; max|e| at 8 x the oracle's
largest error of the case.  DESIGN.md section 1a records what was measured."""
import pytest
import torch

import unet_truth_ref as ut
from oai_analysis_2_amd.synth import make_icon_state_dict, make_volume
from oracle import icon as oicon

pytestmark = pytest.mark.gpu

SHAPES = [(17, 33, 21), (33, 45, 37)]           # odd axes = crop + edges; the second reaches the MFMA up-conv
PREFIXES = (oicon.U1, oicon.U2, oicon.U3)


@pytest.fixture(scope="module")
def icon_truth():
    cache = {}
    sd = make_icon_state_dict(1)

    def get(shape):
        if shape not in cache:
            a, b = torch.from_numpy(make_volume(1, shape)), torch.from_numpy(make_volume(2, shape))
            reg = ut.regions(shape)
            nets = []
            for pre in PREFIXES:
                truth = ut.truth_tall_unet2(a[None, None], b[None, None], sd, pre)[0].numpy()
                ref32 = oicon.tall_unet2(a[None, None], b[None, None], sd, pre)[0].numpy()
                for arr in (truth, ref32):
                    arr.setflags(write=False)
                nets.append((truth, ref32))
            cache[shape] = dict(a=a, b=b, nets=nets, regions={"shell": reg["shell"], "interior": reg["interior"]})
        return sd, cache[shape]
    return get


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=["17x33x21", "33x45x37"])
def test_tall_unet2_against_float64(icon_truth, shape, which):
    from oai_analysis_2_amd.registration import IconEngine
    sd, case = icon_truth(shape)
    truth, ref32 = case["nets"][which]
    assert truth.dtype.itemsize == 8 and truth.shape == (3, *shape)
    eng = IconEngine(sd, net_shape=(40, 48, 48))
    got = eng.unet(which, case["a"], case["b"]).cpu().numpy()
    table = ut.grade(got, truth, ref32, True, case["regions"])
    tag = f"icon net {which} {'x'.join(map(str, shape))} f32"
    print(ut.report(tag, table))
    bad = ut.violations(table, ut.K_CEILING)
    assert not bad, f"{tag}: (channel, region, statistic, multiple of the oracle's fp32 error, limit) {bad}"
