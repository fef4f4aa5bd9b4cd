"""Registration QC on the device: was this knee registered badly?

The chain computes ``phi``, pulls the probability maps and pushes the atlas meshes through it, and never looks at it.  A fold in
``phi`` (a negative Jacobian determinant) tears the warped maps and the pushed meshes, and downstream that is a thickness number like
any other.  ``registration_qc`` returns, per knee, a small record:

    jacobian          ``PhiJacobian``: the fold count and fraction (what ICON / GradICON evaluations report beside Dice, the quantity of
                      ``icon_registration.losses.flips``), min / max / mean / std of det J, optionally the map
    volume_scale      det J is taken in network voxels; ``det * volume_scale`` is the local patient mm^3 per atlas mm^3
    dice              of the warped FC / TC maps against the atlas' own maps (the reference's acceptance test is a Dice-like budget)
    cartilage_voxels, cartilage_mm3      the patient-grid mask counts, and the volumes they stand for

    surface           per cartilage a ``SurfaceDistance``: how far, in millimetres, the warped cartilage surface lies from the atlas' own
                      (ASSD, Hausdorff, HD95) -- only with ``QCReference(..., surface=True)``.  Cartilage is a sheet two to four voxels
                      thick: a one-voxel error halves the Dice and is harmless to the thickness map, a three-voxel error breaks it,
                      and only a distance tells the two apart.

``surface_distance`` and ``segmentation_qc`` give the same figures for any two masks, e.g. a segmentation against a manual one.  The
surface rule (``A ^ binary_erosion(A)``, 6-connectivity) and the pooled percentile are MedPy's on scipy, checked against scipy on the
CPU; ``assd`` is the mean over the pooled distances, and ``mean_ab`` / ``mean_ba`` are there for the mean of the two directed means.

Kernels: csrc/phi_jacobian.hip, csrc/edt.hip (include/oai_hip.h, "Registration QC", "Surface-distance QC").  The fold definition is restated from ``flips`` as recalled
and unpinned, like the resample: icon_registration and ITK are absent.  No threshold and no pass / fail policy is built in: the
record is data.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

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
class SurfaceDistance:
    """The distances between the surfaces of two masks A and B, in the units of the spacing.  d(A->B) is, for every surface voxel of A,
    the distance to the nearest surface voxel of B.  With an empty surface everything but the counts is NaN."""
    n_a: int                     # surface voxels of A
    n_b: int
    mean_ab: float               # mean d(A->B)
    mean_ba: float
    assd: float                  # (sum d(A->B) + sum d(B->A)) / (n_a + n_b)
    hausdorff: float             # max(max d(A->B), max d(B->A))
    percentiles: Dict[float, float]      # np.percentile of the pooled distances (MedPy's hd95 for 95)

    @property
    def hd95(self) -> float:
        return self.percentiles[95.0]


@dataclass
class SegmentationQC:
    """A segmentation against a reference one: Dice, the counts |A|, |B|, |A and B|, non-finite positions, and the surface distances."""
    dice: float
    counts: Tuple[int, int, int, int]
    surface: SurfaceDistance


@dataclass
class RegistrationQC:
    """Every part whose inputs were absent is None."""
    jacobian: PhiJacobian
    volume_scale: Optional[float] = None                              # |det A_out| * |det A_in| of the physical point affines around phi
    dice: Optional[Dict[str, float]] = None                           # 2 |A and B| / (|A| + |B|), NaN when both sets are empty
    overlap_counts: Optional[Dict[str, Tuple[int, int, int, int]]] = None      # per cartilage: |warped|, |atlas|, |both|, non-finite positions
    cartilage_voxels: Optional[Dict[str, int]] = None                 # patient grid: voxels with probability > 0.5
    cartilage_mm3: Optional[Dict[str, float]] = None                  # ... times the patient voxel volume
    surface: Optional[Dict[str, SurfaceDistance]] = None              # warped surface against the atlas' own (QCReference(surface=True))


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


def surface_distance_from_stats(stats, percentiles: Sequence[float]) -> SurfaceDistance:
    """The record of the eight doubles of ``ops.surface_distance`` (already on the host)."""
    s = [float(v) for v in stats]
    n_a, n_b = int(s[0]), int(s[1])
    nan = float("nan")
    if n_a == 0 or n_b == 0:
        return SurfaceDistance(n_a, n_b, nan, nan, nan, nan, {float(q): nan for q in percentiles})
    return SurfaceDistance(n_a, n_b, s[2] / n_a, s[3] / n_b, (s[2] + s[3]) / (n_a + n_b), max(s[4], s[5]),
                           {float(q): s[6 + i] for i, q in enumerate(percentiles)})


def _surface_and_map(vol: torch.Tensor, spacing_xyz, threshold: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(the surface of the set ``> threshold`` as a uint8 mask, the float32 distance map to it): one oai_mask_surface, one oai_edt."""
    surf = ops.mask_surface(vol, threshold, "surface")
    return surf, ops.distance_transform(surf, spacing_xyz)


def _map_with_spacing(m, spacing_xyz):
    """(float32 [z,y,x] device volume, spacing): ``spacing_xyz`` describes a tensor or a bare array, an Image keeps its own."""
    from .image import Image
    from .mesh_processing import _probmap_dev
    if isinstance(m, np.ndarray) and spacing_xyz is not None:
        m = Image(m, spacing_xyz)
    return _probmap_dev(m, spacing_xyz)[:2]


def _two_volumes(a, b, spacing_xyz):
    """Both maps on the device with ONE spacing: ``spacing_xyz`` describes tensors and arrays, an Image brings its own."""
    (va, sa), (vb, sb) = _map_with_spacing(a, spacing_xyz), _map_with_spacing(b, spacing_xyz)
    if va.shape != vb.shape or va.device != vb.device:
        raise ValueError(f"the two maps must share one grid and one GPU, got {tuple(va.shape)} on {va.device} and {tuple(vb.shape)} on {vb.device}")
    if not np.array_equal(sa, sb):
        raise ValueError(f"the two maps must share one spacing, got {sa} and {sb}")
    return va.contiguous(), vb.contiguous(), sa


def _queue_surface_distance(va, vb, spacing, threshold, percentiles, out):
    with torch.cuda.device(va.device):
        surf_a, to_a = _surface_and_map(va, spacing, threshold)
        surf_b, to_b = _surface_and_map(vb, spacing, threshold)
        return ops.surface_distance(surf_a, to_b, surf_b, to_a, percentiles, out=out)


def surface_distance(a, b, spacing_xyz=None, threshold: float = 0.5, percentiles: Sequence[float] = (95.0,)) -> SurfaceDistance:
    """The surface distances of the sets ``> threshold`` of two maps on one grid (each an ``Image``, an array or a [z,y,x] device
    tensor; ``spacing_xyz`` goes with arrays and tensors, unit otherwise): two surfaces, two distance transforms, one
    ``ops.surface_distance``, one download."""
    va, vb, spacing = _two_volumes(a, b, spacing_xyz)
    percentiles = tuple(float(q) for q in percentiles)
    return surface_distance_from_stats(_queue_surface_distance(va, vb, spacing, threshold, percentiles, None).cpu().numpy(), percentiles)


def segmentation_qc(pred, truth, spacing_xyz=None, threshold: float = 0.5) -> SegmentationQC:
    """A segmentation against a manual one, both as maps on one grid (see ``surface_distance``): Dice from ``ops.mask_overlap`` and the
    surface distances, queued together and downloaded once."""
    va, vb, spacing = _two_volumes(pred, truth, spacing_xyz)
    with torch.cuda.device(va.device):
        buf = torch.empty(12, dtype=torch.int64, device=va.device)
        ops.mask_overlap(va, vb, threshold, out=buf[:4])
        _queue_surface_distance(va, vb, spacing, threshold, (95.0,), buf[4:].view(torch.float64))
        host = buf.cpu().numpy()
    counts = tuple(int(v) for v in host[:4])
    return SegmentationQC(dice_from_counts(*counts[:3]), counts, surface_distance_from_stats(host[4:].view(np.float64), (95.0,)))


class QCReference:
    """The atlas' own FC and TC probability maps on the device, uploaded once: what the warped maps of every knee are compared with.
    Each an ``Image``, an array or a [z,y,x] device tensor, as ``thickness.ThicknessAtlas`` takes them.  ``surface=True`` also keeps,
    per cartilage, the atlas surface mask and the distance map to it (computed here, once) and the spacing they are measured in: the
    Images' own, or ``spacing_xyz`` for tensors and bare arrays; a tensor is refused without it."""

    def __init__(self, atlas_fc, atlas_tc, surface: bool = False, spacing_xyz=None):
        got = {kind: _map_with_spacing(m, spacing_xyz) for kind, m in zip(KINDS, (atlas_fc, atlas_tc))}
        self.maps: Dict[str, torch.Tensor] = {kind: g[0].contiguous() for kind, g in got.items()}
        self.device = self.maps["FC"].device
        self.spacing_xyz: Optional[np.ndarray] = None
        self.surfaces: Optional[Dict[str, torch.Tensor]] = None       # uint8 [z,y,x]: the atlas surface per cartilage
        self.distance_maps: Optional[Dict[str, torch.Tensor]] = None  # float32 [z,y,x]: the distance to it
        if surface:
            if spacing_xyz is None and any(torch.is_tensor(m) for m in (atlas_fc, atlas_tc)):
                raise ValueError("QCReference(surface=True): a tensor has no spacing of its own, give spacing_xyz")
            if not np.array_equal(got["FC"][1], got["TC"][1]) or self.maps["FC"].shape != self.maps["TC"].shape:
                raise ValueError("QCReference(surface=True): the two atlas maps must share one grid and one spacing")
            self.spacing_xyz = got["FC"][1]
            with torch.cuda.device(self.device):
                pairs = {kind: _surface_and_map(self.maps[kind], self.spacing_xyz, THRESHOLD) for kind in KINDS}
            self.surfaces = {kind: p[0] for kind, p in pairs.items()}
            self.distance_maps = {kind: p[1] for kind, p in pairs.items()}

    def __getitem__(self, kind: str) -> torch.Tensor:
        return self.maps[kind]


def registration_qc(result_or_phi, image_A=None, image_B=None, reference: Optional[QCReference] = None, return_map: bool = False) -> RegistrationQC:
    """The QC record of one registration: of a ``pipeline.VolumeResult`` (its phi, its patient-grid and warped maps, ``meta_A`` /
    ``meta_B`` unless ``image_A`` / ``image_B`` are given), or of a bare ``phi`` (float32 [3,D,H,W], array or device tensor: the
    Jacobian, and the volume scale when both images are given).  ``reference``: the atlas' own maps, for Dice; built with
    ``surface=True``, also for the surface distances of the warped maps (per cartilage one oai_mask_surface, one oai_edt and one
    oai_surface_distance more).  Parts whose inputs are absent are None.  Every kernel is queued on the current stream first; ONE download of the few dozen result bytes follows, the only
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
        kinds_s = KINDS if is_result and reference is not None and reference.surfaces is not None else ()
        at_s = 7 + 4 * len(jobs)                        # eight doubles per cartilage behind the counts
        buf = torch.empty(at_s + 8 * len(kinds_s), dtype=torch.int64, device=phi.device)     # one buffer, one download
        got = ops.phi_jacobian(phi, return_map=return_map, out=buf[:7].view(torch.float64))
        det_map = got[1] if return_map else None
        for i, (_, _, a, b) in enumerate(jobs):
            ops.mask_overlap(a, b, THRESHOLD, out=buf[7 + 4 * i:11 + 4 * i])
        for i, kind in enumerate(kinds_s):
            warped = ops._chk(getattr(result_or_phi, kind.lower() + "_atlas"), kind)
            if warped.shape != reference.surfaces[kind].shape:
                raise ValueError(f"the warped {kind} map {tuple(warped.shape)} is not on the reference's grid {tuple(reference.surfaces[kind].shape)}")
            surf, to_warped = _surface_and_map(warped, reference.spacing_xyz, THRESHOLD)
            ops.surface_distance(surf, reference.distance_maps[kind], reference.surfaces[kind], to_warped, (95.0,),
                                 out=buf[at_s + 8 * i:at_s + 8 * i + 8].view(torch.float64))
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
    if kinds_s:
        qc.surface = {kind: surface_distance_from_stats(host[at_s + 8 * i:at_s + 8 * i + 8].view(np.float64), (95.0,))
                      for i, kind in enumerate(kinds_s)}
    return qc
