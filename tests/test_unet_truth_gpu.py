"""GPU: the segmentation U-Net's logits against a float64 run of the oracle, in units of the fp32 oracle's own distance from it
(tests/unet_truth_ref.py) -- at the small ragged shapes where kernels go wrong: strips beside the main blocks, border tiles anchored at
their own trimmed box, the shell of the shared encoder pass, a ragged last batch, and the kernel forms that are not the default.

Limits (DESIGN.md section 1a holds the measured table): per class, over all kept voxels and over every region of at least 2000 voxels,
sum|g - t| and rms(g - t) at most 1.2 x the oracle's for f32 and 2.2 x for fp16x3 / bf16x6; max|g - t| at most 8 x the oracle's
largest error of the case.  The 1e-4 gates of the other files let a whole lost split term through (tests/test_unet_truth_cpu.py)."""
import numpy as np
import pytest
import torch

import unet_truth_ref as ut
from oai_analysis_2_amd.synth import make_unet_state_dict, make_volume, make_volume_windowed
from oracle import seg as oseg

pytestmark = pytest.mark.gpu

K = {"f32": ut.K_F32, "bf16x6": ut.K_SPLIT, "fp16x3": ut.K_SPLIT}

# Two forms measured above 2.2 x and take the next multiple, the ceiling 3.5 -- as arithmetic, not as a defect:
#   * fp16x3 with "winograd" 0 (every layer in the direct form): 2.20-2.41 x in every region of (16,24,40).  The same 2.30-2.36 x comes out of all four
#     direct kernels (tap pairs or 32x32x16 taps, the 8-wave 128-cout kernel or not, split-resident activations or fp32 ones), so it belongs to the direct
#     summation -- one running fp32 sum over K = 27 Cin and three passes (only the exact-fp32 kernels accumulate in two levels), chains three times the
#     Winograd form's -- not to a kernel; with the 128-cout layers alone in Winograd form ("winograd" 1) it is 1.70-1.77 x; the project's own
#     full-size record has the direct form 1.4-1.7 x the Winograd form's distance from the reference (4.42 / 4.21 against 3.12 / 2.41).
#   * bf16x6 (six passes into one running sum, direct form only): 2.42-2.71 x at (8,16,24), 3.03-3.43 x at the two larger shapes, in every region -- what
#     the single-running-sum fp32 kernel measured (2.9-3.5 x) before its two-level accumulation.
# Such a case must also stay UNIFORM: every graded region within 20 % of the case's own whole-tile multiple, so that nothing local hides under the ceiling.
ARITHMETIC = {("fp16x3", "winograd=0"), ("bf16x6", "default")}


def _network(name, width_div=1):
    if name == "bn":
        return make_unet_state_dict(seed=5, bn=True, width_div=width_div)
    sd = make_unet_state_dict(seed=5, width_div=width_div)
    if name == "dc":                                        # DC-heavy activations, as synth.make_fullsize_case("dc")
        sd = {k: (v + 1.0 if k.endswith(".0.bias") else v) for k, v in sd.items()}
    return sd


@pytest.fixture(scope="module")
def tile_truth():
    """(network, input, shape, width_div) -> the case: three tiles, their float64 logits and the fp32 oracle's, made once and shared by
    every precision and kernel form."""
    cache = {}

    def get(net, inp, shape, width_div=1):
        key = (net, inp, tuple(shape), width_div)
        if key not in cache:
            sd = _network(net, width_div)
            make = make_volume_windowed if inp == "win" else make_volume
            x = torch.from_numpy(np.stack([make(s, shape) for s in (1, 2, 3)]))[:, None]
            truth = ut.truth_forward(x, sd).numpy().swapaxes(0, 1)                      # [C, B, d, h, w]
            ref32 = oseg.unet_forward(x, sd).numpy().swapaxes(0, 1)
            for a in (truth, ref32):
                a.setflags(write=False)
            cache[key] = dict(sd=sd, x=x, truth=truth, ref32=ref32, regions=ut.regions(shape))
        return cache[key]
    return get


def _engine(sd, precision, opts=None):
    from oai_analysis_2_amd.segmentation.engine import UNetEngine
    eng = UNetEngine(sd, precision=precision)
    for name, value in (opts or {}).items():
        eng.set_option(name, value)
    return eng


def _after_run(eng, precision):
    if precision == "fp16x3":
        assert eng.range_flag() == 0
        assert eng.calibration_status() == "calibrated"


def _check(tag, got, case, mask, precision, form="default"):
    table = ut.grade(got, case["truth"], case["ref32"], mask, case["regions"])
    print(ut.report(tag, table))
    k = K[precision]
    if (precision, form) in ARITHMETIC:
        k = ut.K_CEILING
        for (c, region), row in ((key, row) for key, row in table.items() if key != "ref_max"):
            if row["n"] >= ut.MIN_REGION:
                for s in (0, 1):
                    whole = table[(c, "all")]["ratio"][s]
                    assert 0.8 * whole <= row["ratio"][s] <= 1.2 * whole, f"{tag}: class {c} {region} {ut.STATS[s]} x{row['ratio'][s]:.2f} against x{whole:.2f} over the tile"
    bad = ut.violations(table, k)
    assert not bad, f"{tag}: (class, region, statistic, multiple of the oracle's fp32 error, limit) {bad}"


def _run_tiles(tile_truth, net, inp, shape, precision, opts=None, width_div=1):
    case = tile_truth(net, inp, shape, width_div)
    eng = _engine(case["sd"], precision, opts)
    got = eng.forward_tiles(case["x"].cuda()).cpu().numpy().swapaxes(0, 1)
    _after_run(eng, precision)
    form = ",".join(f"{k}={v}" for k, v in (opts or {}).items()) or "default"
    _check(f"tiles {net}/{inp} w/{width_div} {'x'.join(map(str, shape))} {precision} {form}", got, case, True, precision, form)


@pytest.mark.parametrize("precision", ["f32", "bf16x6", "fp16x3"])
@pytest.mark.parametrize("shape", [(8, 16, 24), (16, 24, 40), (24, 40, 16)])
def test_whole_tiles_base_network(tile_truth, shape, precision):
    """Reference width, spatial sizes that need every strip shape, three tiles per call."""
    _run_tiles(tile_truth, "base", "plain", shape, precision)


@pytest.mark.parametrize("precision", ["f32", "fp16x3"])
@pytest.mark.parametrize("net,inp", [("bn", "plain"), ("dc", "plain"), ("base", "win")])
def test_whole_tiles_other_networks_and_inputs(tile_truth, net, inp, precision):
    """The BN network, the DC-heavy network (every conv bias + 1.0: where the Winograd input transform's d1 + d2 / d0 - d2 cancel) and an
    intensity-windowed input with 5 % of the voxels at exactly 0 and at exactly 1."""
    _run_tiles(tile_truth, net, inp, (16, 24, 40), precision)


@pytest.mark.parametrize("precision,opts", [("fp16x3", {"winograd": 0}), ("fp16x3", {"winograd": 3}), ("fp16x3", {"winograd": 51}),
                                            ("fp16x3", {"m16": 0}), ("fp16x3", {"wide": 2}), ("f32", {"winograd_f32": 0})],
                         ids=["fp16x3-winograd0", "fp16x3-winograd3", "fp16x3-winograd51", "fp16x3-m16_0", "fp16x3-wide2", "f32-winograd_f32_0"])
def test_whole_tiles_other_kernel_forms(tile_truth, precision, opts):
    """Forms with other rounding points or other kernels than the default: the direct form everywhere, Winograd on 32x32x16 taps, the
    64-cout layer in Winograd form too, the direct kernel on 32x32x16 taps, the 8-wave kernel forced, the exact-fp32 direct form."""
    _run_tiles(tile_truth, "base", "plain", (16, 24, 40), precision, opts)


@pytest.mark.parametrize("precision", ["f32", "fp16x3"])
def test_whole_tiles_half_width(tile_truth, precision):
    """width_div=2: channel counts that are no multiple of the production K chunks."""
    _run_tiles(tile_truth, "base", "plain", (16, 24, 40), precision, width_div=2)


# ---- whole volumes: segment_tiles (trimmed border boxes, batch 5 = a ragged last batch) + stitch ---------------------------------------

VOLUMES = {"9x20x38": ((9, 20, 38), (16, 32, 32), (4, 8, 8)),         # 12 tiles, all border tiles, through the shared encoder pass
           "13x37x35": ((13, 37, 35), (16, 32, 32), (4, 8, 8)),       # 18 tiles, the same
           "12x30x33": ((12, 30, 33), (16, 32, 32), (3, 5, 6))}       # 8 tiles, no shared pass, odd trimmed-box anchors


@pytest.fixture(scope="module")
def volume_truth():
    cache = {}

    def get(name):
        if name not in cache:
            shape, tile, ovl = VOLUMES[name]
            sd = make_unet_state_dict(seed=7)
            vol = make_volume(3, shape)
            truth, ref32, kept, g = ut.truth_segment(vol, sd, tile, ovl)
            for a in (truth, ref32, kept):
                a.setflags(write=False)
            cache[name] = dict(sd=sd, vol=vol, truth=truth, ref32=ref32, kept=kept, regions=ut.regions(shape, g), n_tiles=g["n_tiles"])
        return cache[name]
    return get


@pytest.mark.parametrize("precision", ["f32", "fp16x3"])
@pytest.mark.parametrize("name", sorted(VOLUMES))
def test_volumes(volume_truth, name, precision):
    shape, tile, ovl = VOLUMES[name]
    case = volume_truth(name)
    assert case["n_tiles"] == {"9x20x38": 12, "13x37x35": 18, "12x30x33": 8}[name] and case["n_tiles"] % 5 != 0
    crop = ut.crop_of(ovl)
    eng = _engine(case["sd"], precision)
    blocks = eng.segment_tiles(torch.from_numpy(case["vol"]).cuda(), tile, ovl, out_mode=2, batch=5, crop_zyx=crop)
    got = eng.stitch(blocks, shape, tile, ovl, crop).cpu().numpy()
    _after_run(eng, precision)
    assert got.shape == case["truth"].shape
    assert not got[:, ~case["kept"]].any()                                 # the zeroed frame is exactly 0
    assert np.isfinite(got).all()
    _check(f"volume {name} tile {'x'.join(map(str, tile))} ovl {'x'.join(map(str, ovl))} {precision}", got, case, case["kept"], precision)
