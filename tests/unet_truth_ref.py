"""Float64 truth for the two networks of the hot path and the statistics that grade a result against it.

The oracle (oracle/seg.py, oracle/icon.py) is pure torch, so the same functions run in float64 once every floating tensor of the
state dict is cast: the same algorithm without fp32 rounding.  A result ``g`` (a HIP kernel's, or a deliberately damaged forward) is
graded by its distance from that run ``t`` IN UNITS OF the fp32 oracle's own distance ``r - t`` on the same machine: sum|e|,
sqrt(mean e^2) and max|e| per class and per named region.  A gate of the form ``max|g - r| / max|r| < 1e-4`` sits about 100 times
above fp32 noise; these ratios sit at it.

Limits: sum and rms at most 1.2 x the oracle's for exact fp32 products, 2.2 x for the split formats
(fp16x3, bf16x6), in every region of at least MIN_REGION voxels; max|g - t| at most 8 x the oracle's largest error of the whole case.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import icon as oicon, seg as oseg

torch.set_num_threads(min(16, torch.get_num_threads()))

K_F32 = 1.2          # sum|e| and rms multiple of the exact-fp32 path (tests/test_fullsize_gpu.py holds the same against float64)
K_SPLIT = 2.2        # ... of fp16x3 / bf16x6
K_CEILING = 3.5      # what the single-running-sum fp32 kernel measured and the project judged too noisy: nothing is gated above it
K_POINT = 8.0        # max|g - t| against the oracle's largest error of the case
MIN_REGION = 2000    # smaller regions get the pointwise gate only: a sum over a few hundred voxels is not a statistic
STATS = ("l1", "rms", "max")


def _double_sd(sd):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}


@torch.no_grad()
def truth_forward(x: torch.Tensor, sd) -> torch.Tensor:
    """oracle.seg.unet_forward in float64: [B,1,d,h,w] -> float64 logits [B,C,d,h,w]."""
    return oseg.unet_forward(x.double(), _double_sd(sd))


@torch.no_grad()
def truth_tall_unet2(a: torch.Tensor, b: torch.Tensor, sd, prefix: str = "", apply_bn=None, pad_front=None) -> torch.Tensor:
    """oracle.icon.tall_unet2 in float64 (whether BatchNorm applies is decided from the whole checkpoint, as in the fp32 run)."""
    if apply_bn is None and oicon.OPTIONS["apply_bn"] is None:
        apply_bn = oicon.infer_apply_bn(sd)
    return oicon.tall_unet2(a.double(), b.double(), _double_sd(sd), prefix, apply_bn=apply_bn, pad_front=pad_front)


def crop_of(ovl_zyx: Sequence[int]) -> Tuple[int, int, int]:
    """The frame Partition.assemble zeroes, in z,y,x: it indexes crop_size as (x,y,z) and puts [0] on numpy axis 1 (oracle.seg.assemble)."""
    oz, oy, ox = (int(v) for v in ovl_zyx)
    return (oz, ox, oy)


@torch.no_grad()
def truth_segment(vol: np.ndarray, sd, tile_zyx: Sequence[int], ovl_zyx: Sequence[int], batch: int = 4):
    """(truth, ref32, kept, geometry) of a whole volume: logits [C,D,H,W] float64 as ``assemble`` keeps them -- tiles cut by
    oracle.seg.partition, the network per tile, centres stitched, the frame zeroed -- from the float64 run and from the fp32 oracle,
    and the boolean [D,H,W] mask of the voxels outside the zeroed frame (all of them inside the image)."""
    patch_xyz, ovl_xyz = tuple(tile_zyx)[::-1], tuple(ovl_zyx)[::-1]
    tiles, g = oseg.partition(np.asarray(vol), patch_xyz, ovl_xyz)
    tiles_t = torch.from_numpy(np.ascontiguousarray(tiles))
    sd64 = _double_sd(sd)
    t64 = torch.cat([oseg.unet_forward(tiles_t[s:s + batch].double(), sd64) for s in range(0, len(tiles_t), batch)]).numpy()
    r32 = torch.cat([oseg.unet_forward(tiles_t[s:s + batch], sd) for s in range(0, len(tiles_t), batch)]).numpy()
    n_cls = t64.shape[1]
    truth = np.stack([oseg.assemble(t64[:, c], g, crop_size_xyz=ovl_xyz) for c in range(n_cls)])
    ref32 = np.stack([oseg.assemble(r32[:, c], g, crop_size_xyz=ovl_xyz) for c in range(n_cls)])
    kept = oseg.assemble(np.ones((len(tiles_t), *g["tile"]), np.float64), g, crop_size_xyz=ovl_xyz) > 0.5
    return truth, ref32, kept, g


def regions(shape_zyx: Sequence[int], geometry: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """Named boolean masks of shape ``shape_zyx``.

    A whole tile (``geometry`` None): ``shell`` (fewer than 2 voxels from a tile face), ``interior``, ``x_even`` / ``x_odd`` (the
    Winograd form computes x pairs).  A volume (``geometry`` = oracle.seg.tile_geometry): ``x_even`` / ``x_odd`` in volume
    coordinates, ``seam`` (within 1 voxel of a boundary between two kept-centre blocks), ``low`` / ``high`` (voxels whose tile
    touches a low / high face of the volume)."""
    shape = tuple(int(v) for v in shape_zyx)
    idx = np.indices(shape)
    out = {"x_even": idx[2] % 2 == 0, "x_odd": idx[2] % 2 == 1}
    if geometry is None:
        shell = np.zeros(shape, bool)
        for a, n in enumerate(shape):
            shell |= (idx[a] < 2) | (idx[a] >= n - 2)
        out.update(shell=shell, interior=~shell)
        return out
    eff, grid = geometry["effective"], geometry["grid"]
    seam, low, high = (np.zeros(shape, bool) for _ in range(3))
    for a in range(3):
        e, n = int(eff[a]), int(grid[a])
        for b in range(e, min(n * e, shape[a]), e):           # kept block i covers [i e, (i + 1) e): its boundaries inside the image
            seam |= (idx[a] == b - 1) | (idx[a] == b)
        low |= idx[a] < e
        high |= idx[a] >= (n - 1) * e
    out.update(seam=seam, low=low, high=high)
    return out


def _stats(e: np.ndarray) -> Tuple[float, float, float]:
    if e.size == 0:
        return 0.0, 0.0, 0.0
    a = np.abs(e)
    return float(a.sum()), float(np.sqrt(np.mean(e * e))), float(a.max())


def grade(got, truth, ref32, mask, regions: Dict[str, np.ndarray]):
    """``got``, ``truth``, ``ref32``: [C, ...]; ``mask`` and every region: boolean, broadcastable to the trailing axes.  Returns
    {(class, region): {"n", "got": (sum|e|, rms, max|e|), "ref": the same of ref32, "ratio": got / ref}} with the region "all" =
    every voxel of ``mask``, and under the key "ref_max" the oracle's largest error over the whole case (all classes)."""
    got, truth, ref32 = (np.asarray(v, np.float64) for v in (got, truth, ref32))
    assert got.shape == truth.shape == ref32.shape
    mask = np.broadcast_to(np.asarray(mask, bool), truth.shape[1:])
    table = {}
    named = {"all": np.ones(truth.shape[1:], bool), **regions}
    for c in range(truth.shape[0]):
        eg, er = got[c] - truth[c], ref32[c] - truth[c]
        for name, reg in named.items():
            sel = mask & np.broadcast_to(reg, mask.shape)
            sg, sr = _stats(eg[sel]), _stats(er[sel])
            table[(c, name)] = dict(n=int(sel.sum()), got=sg, ref=sr,
                                    ratio=tuple(a / b if b > 0 else (0.0 if a == 0 else float("inf")) for a, b in zip(sg, sr)))
    table["ref_max"] = max(table[(c, "all")]["ref"][2] for c in range(truth.shape[0]))
    return table


def violations(table, k: float, k_point: float = K_POINT, min_region: int = MIN_REGION):
    """The gates of section 4 on a ``grade`` table: list of (class, region, statistic, measured multiple, limit); empty = passes."""
    bad = []
    ref_max = table["ref_max"]
    for key, row in table.items():
        if key == "ref_max" or row["n"] == 0:
            continue
        c, name = key
        if name == "all" or row["n"] >= min_region:
            for s in (0, 1):
                if not row["got"][s] <= k * row["ref"][s]:
                    bad.append((c, name, STATS[s], row["ratio"][s], k))
        if not row["got"][2] <= k_point * ref_max:
            bad.append((c, name, "max", row["got"][2] / ref_max if ref_max > 0 else float("inf"), k_point))
    return bad


def old_gate(got, truth, mask) -> float:
    """max|got - truth| / max|truth| over ``mask``: the figure the 1e-4 gates of the rest of the suite look at."""
    got, truth = np.asarray(got, np.float64), np.asarray(truth, np.float64)
    sel = np.broadcast_to(np.asarray(mask, bool), truth.shape[1:])
    return float(np.abs(got - truth)[:, sel].max() / np.abs(truth[:, sel]).max())


def report(tag: str, table) -> str:
    """One line per class and region: n, the three figures of ``got``, their multiples of the oracle's; the pointwise figure also as
    a multiple of the case's ``ref_max`` (what the pointwise gate reads)."""
    lines = []
    ref_max = table["ref_max"]
    for key, row in table.items():
        if key == "ref_max":
            continue
        c, name = key
        g, q = row["got"], row["ratio"]
        lines.append(f"[truth] {tag} | class {c} | {name:8s} | n {row['n']:7d} | L1 {g[0]:.3e} x{q[0]:5.2f} | rms {g[1]:.3e} x{q[1]:5.2f} | "
                     f"max {g[2]:.3e} x{q[2]:5.2f} | max/ref_max x{(g[2] / ref_max if ref_max > 0 else 0.0):5.2f}")
    return "\n".join(lines)
