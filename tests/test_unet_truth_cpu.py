"""CPU: the float64-relative gate of tests/unet_truth_ref.py bites where the suite's 1e-4 gates do not -- shown without a GPU.

A "mutant" is the float64 forward of the oracle with some weights rounded to a few bits: exact arithmetic on a slightly wrong network,
the signature of a kernel that loses a low split term or rounds a transform at the wrong place.
  ec3 / 12 bits: the first quarter of ec3's output channels keep 12 significant bits -- a whole lost low split term on those channels;
  dc2 / 16 bits: the first quarter of dc2's output channels keep 16.
Both stay below ``max|d| / max|truth| < 1e-4`` (what test_forward_tiles_ragged_shapes_vs_oracle and its kin assert) and both fail the
sum and rms limits of the new gate by a wide margin; the ec3 mutant fails the pointwise limit too.  Tile (8,16,24), reference width,
the inputs of the GPU cases.  Networks: the base one and the DC-heavy one (every conv bias + 1.0).  (On the BN network at this tile
the ec3 mutant moves the logits by 1.02e-4 of their maximum -- at the old gate, not under it -- so it shows nothing about that gate.)
"""
import numpy as np
import pytest
import torch

import unet_truth_ref as ut
from oai_analysis_2_amd.synth import make_unet_state_dict, make_volume
from oracle import seg as oseg

SHAPE = (8, 16, 24)
MUTANTS = {"ec3_12bit": ("ec3.0.weight", 12, 0),       # Conv3d weight [cout, cin, 3,3,3]
           "dc2_16bit": ("dc2.0.weight", 16, 1)}       # ConvTranspose3d weight [cin, cout, 3,3,3]


def _round_bits(w: torch.Tensor, bits: int) -> torch.Tensor:
    """``w`` rounded to ``bits`` significant bits (round to nearest)."""
    m, e = torch.frexp(w.double())
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e).to(w.dtype)


def _mutate(sd, which):
    key, bits, cout_axis = MUTANTS[which]
    w = sd[key].clone()
    q = w.shape[cout_axis] // 4
    sel = (slice(0, q),) if cout_axis == 0 else (slice(None), slice(0, q))
    w[sel] = _round_bits(w[sel], bits)
    assert not torch.equal(w, sd[key])
    out = dict(sd)
    out[key] = w
    return out


def _network(name):
    sd = make_unet_state_dict(seed=5)
    if name == "dc":
        sd = {k: (v + 1.0 if k.endswith(".0.bias") else v) for k, v in sd.items()}
    return sd


@pytest.fixture(scope="module", params=["base", "dc"])
def case(request):
    sd = _network(request.param)
    x = torch.from_numpy(np.stack([make_volume(s, SHAPE) for s in (1, 2, 3)]))[:, None]
    truth = ut.truth_forward(x, sd).numpy().swapaxes(0, 1)                 # [C, B, d, h, w]
    ref32 = oseg.unet_forward(x, sd).numpy().swapaxes(0, 1)
    return dict(name=request.param, sd=sd, x=x, truth=truth, ref32=ref32, regions=ut.regions(SHAPE))


def test_the_fp32_oracle_passes_with_ratio_one(case):
    table = ut.grade(case["ref32"], case["truth"], case["ref32"], True, case["regions"])
    print(ut.report(f"{case['name']} oracle-fp32", table))
    rel = table["ref_max"] / np.abs(case["truth"]).max()
    print(f"[truth] {case['name']}: the oracle's own fp32 noise: max {table['ref_max']:.2e} = {rel:.2e} of max|logit|")
    assert 1e-8 < rel < 1e-5                                               # fp32 noise of an 18-layer network, and not zero: truth really is float64
    assert all(row["ratio"] == (1.0, 1.0, 1.0) for key, row in table.items() if key != "ref_max")
    assert ut.violations(table, ut.K_F32) == []
    assert set(case["regions"]) == {"shell", "interior", "x_even", "x_odd"}
    assert all(table[(c, r)]["n"] >= ut.MIN_REGION for c in (0, 1) for r in case["regions"])      # every region of this tile is graded in full


@pytest.mark.parametrize("which", sorted(MUTANTS))
def test_mutants_fail_the_truth_gate_and_pass_the_old_one(case, which):
    got = ut.truth_forward(case["x"], _mutate(case["sd"], which)).numpy().swapaxes(0, 1)
    table = ut.grade(got, case["truth"], case["ref32"], True, case["regions"])
    old = ut.old_gate(got, case["truth"], True)
    print(ut.report(f"{case['name']} {which}", table))
    print(f"[truth] {case['name']} {which}: max|d| / max|truth| = {old:.2e} (the 1e-4 gate lets it through)")
    assert old < 1e-4
    for k in (ut.K_F32, ut.K_SPLIT, ut.K_CEILING):                        # not even the ceiling multiple lets a mutant through
        bad = ut.violations(table, k)
        for c in (0, 1):
            for region in ("all", *case["regions"]):
                assert (c, region, "l1", table[(c, region)]["ratio"][0], k) in bad
                assert (c, region, "rms", table[(c, region)]["ratio"][1], k) in bad
    if which == "ec3_12bit":
        point = [v for v in ut.violations(table, ut.K_SPLIT) if v[2] == "max"]
        assert {(c, r) for c, r, *_ in point} >= {(0, "all"), (1, "all")}
        assert all(m > ut.K_POINT for *_, m, _lim in point)


def test_regions_of_a_volume_and_the_kept_mask():
    """Geometry only (a width_div=8 network keeps it instant): ``kept`` is what assemble leaves outside its zeroed frame, truth and the
    fp32 run are zero off it, the regions are the ones named, and low | high covers a two-tile axis."""
    sd = make_unet_state_dict(seed=7, width_div=8)
    vol, tile, ovl = make_volume(3, (12, 30, 33)), (16, 32, 32), (3, 5, 6)
    truth, ref32, kept, g = ut.truth_segment(vol, sd, tile, ovl)
    cz, cy, cx = ut.crop_of(ovl)
    assert (cz, cy, cx) == (3, 6, 5) and g["n_tiles"] == 8
    want = np.zeros(vol.shape, bool)
    want[cz:-cz, cy:-cy, cx:-cx] = True
    assert np.array_equal(kept, want)
    assert truth.dtype == np.float64 and truth.shape == (2, *vol.shape)
    assert not truth[:, ~kept].any() and not ref32[:, ~kept].any() and np.abs(truth[:, kept]).min() > 0
    fc, tc, lf, lt = oseg.segment(vol, sd, tile[::-1], ovl[::-1], return_logits=True)     # the oracle's own whole-volume run, unframed logits
    assert np.array_equal(ref32[0][kept], lf[kept]) and np.array_equal(ref32[1][kept], lt[kept])
    reg = ut.regions(vol.shape, g)
    assert set(reg) == {"x_even", "x_odd", "seam", "low", "high"}
    assert np.array_equal(reg["x_even"], ~reg["x_odd"]) and reg["x_even"][0, 0, 0] and reg["x_odd"][0, 0, 1]
    assert (reg["low"] | reg["high"]).all()                                 # grid 2 x 2 x 2: every tile touches a face
    seam = np.zeros(vol.shape, bool)
    seam[9:11] = True                                                       # effective tile (10, 22, 20): block boundaries at z 10, y 22, x 20
    seam[:, 21:23] = True
    seam[:, :, 19:21] = True
    assert np.array_equal(reg["seam"], seam)
    table = ut.grade(ref32, truth, ref32, kept, reg)
    assert table[(0, "all")]["n"] == int(kept.sum()) == 6 * 18 * 23 and ut.violations(table, ut.K_F32) == []
