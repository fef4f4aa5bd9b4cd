"""Registration QC on the device: was this knee registered badly?

The chain computes ``phi``, pulls the probability maps and pushes the atlas meshes through it, and never looks at it.  A fold in
``phi`` (a negative Jacobian determinant) tears the warped maps and the pushed meshes, and downstream that is a thickness number like
any other.  ``registration_qc`` returns, per knee, a small record:

    jacobian          ``PhiJacobian``: the fold count and fraction (what ICON / GradICON evaluations report beside Dice, the quantity of
                      ``icon_registration.losses.flips``), min / max / mean / std of det J, optionally the map
    volume_scale      det J is taken in network voxels; ``det * volume_scale`` is the local patient mm^3 per atlas mm^3
    dice              of the warped FC / TC maps against the atlas' own maps (the reference's acceptance test is a Dice-like budget)
    cartilage_voxels, cartilage_mm3      the patient-grid mask counts, and the volumes they stand for

Kernels: csrc/phi_jacobian.hip (include/oai_hip.h, "Registration QC").  The fold definition is restated from ``flips`` as recalled
and unpinned, like the resample: icon_registration and ITK are absent.  No threshold and no pass / fail policy is built in: the
record is data.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops
from .image import as_image

KINDS = ("FC", "TC")
THRESHOLD = 0.5          # the segmentation's rule: a voxel is cartilage when its probability is > 0.5


@dataclass
class PhiJacobian:
    """det J of phi over the (D-1)(H-1)(W-1) backward-difference cells, in network voxels.  A cell whose determinant is not finite
    (a NaN or Inf in phi) is counted in ``nonfinite`` and left out of every other figure."""
    cells: int
    folds: int                   # cells with det < 0
    nonfinite: int
    fold_fraction: float         # folds / cells
    det_min: float               # NaN when no cell is finite, like the two below
    det_max: float
    det_mean: float              # from the device's two fp64 sums, on the host in fp64
    det_std: float               # population standard deviation
    det_map: Optional[torch.Tensor] = None       # float32 [D-1,H-1,W-1] on the device (return_map=True only)


@dataclass
class RegistrationQC:
    """Every part whose inputs were absent is None."""
    jacobian: PhiJacobian
    volume_scale: Optional[float] = None                              # |det A_out| * |det A_in| of the physical point affines around phi
    dice: Optional[Dict[str, float]] = None                           # 2 |A and B| / (|A| + |B|), NaN when both sets are empty
    overlap_counts: Optional[Dict[str, Tuple[int, int, int, int]]] = None      # per cartilage: |warped|, |atlas|, |both|, non-finite positions
    cartilage_voxels: Optional[Dict[str, int]] = None                 # patient grid: voxels with probability > 0.5
    cartilage_mm3: Optional[Dict[str, float]] = None                  # ... times the patient voxel volume


def jacobian_from_stats(stats, det_map: Optional[torch.Tensor] = None) -> PhiJacobian:
    """The record of the seven doubles of ``ops.phi_jacobian`` (already on the host)."""
    s = [float(v) for v in stats]
    cells, folds, bad = int(s[0]), int(s[1]), int(s[2])
    finite = cells - bad
    if finite > 0:
        mean = s[5] / finite
        std = math.sqrt(max(s[6] / finite - mean * mean, 0.0))
        lo, hi = s[3], s[4]
    else:
        mean = std = lo = hi = float("nan")
    return PhiJacobian(cells, folds, bad, folds / cells if cells else float("nan"), lo, hi, mean, std, det_map)


def volume_scale(image_A, image_B, net_shape) -> float:
    """``|det A_out| * |det A_in|`` of ``mesh_point_affines(image_A, image_B, net_shape, "physical", "physical")`` in fp64: an atlas
    point p goes to ``A_out (x + u(x)) + b`` with ``x = A_in p + b'``, so the local volume change in physical units is
    ``det J * det A_out * det A_in``.  The absolute values keep a flipped direction matrix from turning every cell into a "fold": a
    fold is a property of phi in network space."""
    from .mesh_processing import mesh_point_affines
    (A_in, _), (A_out, _) = mesh_point_affines(image_A, image_B, tuple(int(v) for v in net_shape), "physical", "physical")
    return float(abs(np.linalg.det(np.asarray(A_out, np.float64))) * abs(np.linalg.det(np.asarray(A_in, np.float64))))


def dice_from_counts(n_a: int, n_b: int, n_both: int) -> float:
    return 2.0 * n_both / (n_a + n_b) if (n_a + n_b) else float("nan")


class QCReference:
    """The atlas' own FC and TC probability maps on the device, uploaded once: what the warped maps of every knee are compared with.
    Each an ``Image``, an array or a [z,y,x] device tensor, as ``thickness.ThicknessAtlas`` takes them."""

    def __init__(self, atlas_fc, atlas_tc):
        from .mesh_processing import _probmap_dev
        self.maps: Dict[str, torch.Tensor] = {kind: _probmap_dev(m)[0].contiguous() for kind, m in zip(KINDS, (atlas_fc, atlas_tc))}
        self.device = self.maps["FC"].device

    def __getitem__(self, kind: str) -> torch.Tensor:
        return self.maps[kind]


def registration_qc(result_or_phi, image_A=None, image_B=None, reference: Optional[QCReference] = None, return_map: bool = False) -> RegistrationQC:
    """The QC record of one registration: of a ``pipeline.VolumeResult`` (its phi, its patient-grid and warped maps, ``meta_A`` /
    ``meta_B`` unless ``image_A`` / ``image_B`` are given), or of a bare ``phi`` (float32 [3,D,H,W], array or device tensor: the
    Jacobian, and the volume scale when both images are given).  ``reference``: the atlas' own maps, for Dice.  Parts whose inputs are
    absent are None.  Every kernel is queued on the current stream first; ONE download of the few dozen result bytes follows, the only
    synchronisation."""
    is_result = hasattr(result_or_phi, "phi") and hasattr(result_or_phi, "fc_atlas")
    phi = result_or_phi.phi if is_result else result_or_phi
    if not torch.is_tensor(phi):
        phi = torch.from_numpy(np.ascontiguousarray(phi)).cuda()
    phi = ops._chk(phi, "phi")
    if is_result:
        image_A = result_or_phi.meta_A if image_A is None else image_A
        image_B = getattr(result_or_phi, "meta_B", None) if image_B is None else image_B
    with torch.cuda.device(phi.device):
        jobs = []                                       # (part, kind, a, b), one oai_mask_overlap each
        if is_result:
            jobs += [("patient", kind, getattr(result_or_phi, kind.lower()), None) for kind in KINDS]
            if reference is not None:
                jobs += [("dice", kind, getattr(result_or_phi, kind.lower() + "_atlas"), reference[kind]) for kind in KINDS]
        buf = torch.empty(7 + 4 * len(jobs), dtype=torch.int64, device=phi.device)          # one buffer, one download
        got = ops.phi_jacobian(phi, return_map=return_map, out=buf[:7].view(torch.float64))
        det_map = got[1] if return_map else None
        for i, (_, _, a, b) in enumerate(jobs):
            ops.mask_overlap(a, b, THRESHOLD, out=buf[7 + 4 * i:11 + 4 * i])
        host = buf.cpu().numpy()
    qc = RegistrationQC(jacobian_from_stats(host[:7].view(np.float64), det_map))
    if image_A is not None and image_B is not None:
        qc.volume_scale = volume_scale(image_A, image_B, phi.shape[1:])
    for i, (part, kind, _, _) in enumerate(jobs):
        n_a, n_b, n_both, n_bad = (int(v) for v in host[7 + 4 * i:11 + 4 * i])
        if part == "patient":
            if qc.cartilage_voxels is None:
                qc.cartilage_voxels = {}
            qc.cartilage_voxels[kind] = n_a
            if image_A is not None:
                if qc.cartilage_mm3 is None:
                    qc.cartilage_mm3 = {}
                qc.cartilage_mm3[kind] = n_a * float(np.prod(as_image(image_A).spacing))
        else:
            if qc.dice is None:
                qc.dice, qc.overlap_counts = {}, {}
            qc.dice[kind] = dice_from_counts(n_a, n_b, n_both)
            qc.overlap_counts[kind] = (n_a, n_b, n_both, n_bad)
    return qc
