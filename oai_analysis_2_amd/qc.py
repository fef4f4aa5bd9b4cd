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

    similarity        per stage an ``ImageSimilarity``: how alike the patient IMAGE and the atlas image are on the network grid, "before"
                      and "after" the warp through phi (and within a few millimetres of the atlas cartilage: "before_roi" / "after_roi")
                      -- LNCC, what the registration was trained to maximise; NCC and MSE; mutual information, what the atlas was built
                      under.  Only with ``QCReference(..., image=atlas)`` and a patient image.  Every other figure here goes through the
                      segmentation; these do not.

``segmentation_shape`` needs nothing to compare with: per map a ``SegmentationShape`` -- the connected pieces of the cartilage mask,
the share of the largest, what sits in islands, the closed cavities, the voxels of uncertain probability.  A failed segmentation
(cartilage in several pieces, a blob in the muscle, a sheet full of holes) shows there and nowhere else.  Two labelling calls per
map (the set under ``connectivity``, its complement under the dual connectivity) and two overlap counts, queued and downloaded once;
``clean_segmentation`` drops the islands on the device; ``VolumePipeline.run(seg_qc=True)`` returns the records of the patient-grid
maps in ``VolumeResult.seg_qc``.  The labelling is ``scipy.ndimage.label``'s to the element, checked against scipy on the CPU.

``local_thickness`` checks the one figure the pipeline exists to produce without any of the stages that produce it: per map a
``LocalThickness`` -- at every voxel of the cartilage the diameter of the largest ball that contains it and stays inside (Hildebrand
and Ruegsegger's local thickness), then mean / median / p95 over the set and over its surface voxels.  No mesh, no smoothing, no
inner/outer split, no atlas, no phi: where the k-means split mislabels a patch the mesh-based thickness is the distance of a surface
to itself or across the joint, and only a disagreement with this figure shows it.  ``VolumePipeline.run(thickness_qc=True)`` returns
the records of the patient-grid maps in ``VolumeResult.thickness_qc``.

``mesh_quality`` / ``split_quality`` check the stage in between: the surface that the mesh-based thickness is measured on, after marching
cubes, the region filter, 150 smoothing sweeps and the k-means split -- is it closed and consistently oriented, does it fold through
itself, how many pieces, how long and how ragged is the inner / outer interface, what volume does it enclose (``MeshQuality``,
``SplitQuality``).  ``ThicknessAtlas.measure(..., mesh_qc=True)`` returns the records of the very split the distance was taken on in
``KneeThickness.mesh_qc``.

``image_similarity`` gives the same record for any two images on one grid.  ``surface_distance`` and ``segmentation_qc`` give the same figures for any two masks, e.g. a segmentation against a manual one.  The
surface rule (``A ^ binary_erosion(A)``, 6-connectivity) and the pooled percentile are MedPy's on scipy, checked against scipy on the
CPU; ``assd`` is the mean over the pooled distances, and ``mean_ab`` / ``mean_ba`` are there for the mean of the two directed means.

Kernels: csrc/phi_jacobian.hip, csrc/edt.hip, csrc/similarity.hip, csrc/components.hip, csrc/local_thickness.hip, csrc/mesh_quality.hip
(include/oai_hip.h, "Registration QC", "Surface-distance QC", "Image-similarity QC", "Segmentation-shape QC", "Thickness QC", "Mesh quality").  ICON's LNCC form (a Gaussian window of 4 sigma + 1 samples, sigma = 4, eps = 1e-5) is restated as recalled and unpinned.  The fold definition is restated from ``flips`` as recalled
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
from .registration import NET_SHAPE

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
class ImageSimilarity:
    """How alike two images on one grid are.  A position takes part when the mask admits it and both values are finite (``n``;
    ``nonfinite`` counts the admitted positions left out); with no such position every figure is NaN."""
    n: int
    nonfinite: int
    ncc: float                   # Pearson's r from the device's fp64 moments, on the host in fp64
    mse: float                   # mean (a - b)^2
    lncc: float                  # mean cc under a Gaussian window of ``sigma`` voxels; the network's similarity loss is 1 - lncc
    lncc_std: float              # population standard deviation of cc
    lncc_min: float
    lncc_max: float
    mi: float                    # H_A + H_B - H_AB, natural logarithm
    nmi: float                   # (H_A + H_B) / H_AB, Studholme's form: 2 for identical images, 1 for independent ones
    entropy_a: float
    entropy_b: float
    entropy_joint: float
    sigma: float
    bins: int
    cc_map: Optional[torch.Tensor] = None        # float64 [z,y,x] on the device (return_map=True only)


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
    # Optional[Dict[str, ImageSimilarity]]: "before" / "after" the warp (and "*_roi"), the patient image against the atlas'
    # (QCReference(image=)).  A plain attribute and not a dataclass field: dataclasses.asdict and fields of the record stay the parts
    # that go through phi and the segmentation, which earlier tests pin by name; the images' record is read as ``qc.similarity``.
    similarity = None


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


SIGMA, BINS = 4.0, 64        # registration_qc's window (ICON's sigma for the knee model, as recalled) and histogram
SIMILARITY_SLOTS = 18        # doubles per comparison in the downloaded buffer: 8 moments, 6 of the LNCC, 4 of the entropies


def ncc_from_moments(stats) -> Tuple[float, float]:
    """(Pearson's r, mean squared error) of the eight doubles of ``ops.image_moments``; r is NaN when an image is constant."""
    n, _, sa, sb, saa, sbb, sab, sdd = (float(v) for v in stats)
    if n <= 0:
        return float("nan"), float("nan")
    cov, va, vb = sab / n - (sa / n) * (sb / n), saa / n - (sa / n) ** 2, sbb / n - (sb / n) ** 2
    return (cov / math.sqrt(va * vb) if va > 0 and vb > 0 else float("nan")), sdd / n


def similarity_from_stats(stats, sigma: float, bins: int, cc_map: Optional[torch.Tensor] = None) -> ImageSimilarity:
    """The record of the 18 doubles that ``_queue_similarity`` leaves (already on the host)."""
    s = [float(v) for v in stats]
    mom, lc, (_, ha, hb, hab) = s[:8], s[8:14], s[14:18]
    ncc, mse = ncc_from_moments(mom)
    if lc[0] > 0:
        mean = lc[2] / lc[0]
        std = math.sqrt(max(lc[3] / lc[0] - mean * mean, 0.0))
    else:
        mean = std = float("nan")
    return ImageSimilarity(int(mom[0]), int(mom[1]), ncc, mse, mean, std, lc[4], lc[5], ha + hb - hab,
                           (ha + hb) / hab if hab > 0 else float("nan"), ha, hb, hab, float(sigma), int(bins), cc_map)


def _result_slots(device, layout):
    """The ONE buffer behind "queue everything, then ONE download": ``layout`` is the ordered list of ``(key, n_slots, dtype)``, dtype
    torch.int64 or torch.float64 (both eight bytes: one int64 buffer holds them all).  Returns ``(views, download)``: the device views by
    key, each of its dtype, for the kernels to write into; ``download()`` copies the buffer to the host once -- the only synchronisation
    -- and returns the host views by the same keys.  The layout is written here and nowhere else."""
    spans, at = {}, 0
    for key, n_slots, dtype in layout:
        spans[key] = (at, at + n_slots, dtype)
        at += n_slots
    buf = torch.empty(at, dtype=torch.int64, device=device)

    def download():
        host = buf.cpu().numpy()
        return {key: host[lo:hi].view(np.float64 if dtype == torch.float64 else np.int64) for key, (lo, hi, dtype) in spans.items()}
    return {key: buf[lo:hi] if dtype == torch.int64 else buf[lo:hi].view(dtype) for key, (lo, hi, dtype) in spans.items()}, download


def _image_dev(m) -> torch.Tensor:
    """An image -- an ``Image``, an array or a [z,y,x] device tensor -- as a contiguous float32 device volume (its geometry is not used)."""
    return _map_with_spacing(m, None)[0].contiguous()


def _queue_similarity(a, b, sigma, bins, value_range, mask, return_map, out):
    """One comparison queued on the current stream: four launches' worth of kernels, results into ``out`` (float64 [18])."""
    ops.image_moments(a, b, mask, out=out[:8])
    got = ops.lncc(a, b, sigma, mask=mask, return_map=return_map, out=out[8:14])
    hist = ops.joint_histogram(a, b, bins, value_range, value_range, mask)
    ops.histogram_entropies(hist, bins, out=out[14:18])
    return got[1] if return_map else None


def image_similarity(a, b, sigma: float = 4.0, bins: int = 64, value_range=(0.0, 1.0), mask=None, return_map: bool = False) -> ImageSimilarity:
    """The similarity record of two images on one grid (each an ``Image``, an array or a [z,y,x] device tensor, as ``surface_distance``
    takes them; ``mask``: uint8 / bool on the same grid, non-zero = takes part).  The images are expected windowed to ``value_range``,
    as the pipeline's are to [0, 1]; values outside it fall into the histogram's end bins.  Everything is queued, then ONE download."""
    va, vb = _image_dev(a), _image_dev(b)
    if va.shape != vb.shape or va.device != vb.device:
        raise ValueError(f"the two images must share one grid and one GPU, got {tuple(va.shape)} on {va.device} and {tuple(vb.shape)} on {vb.device}")
    if mask is not None:
        if not torch.is_tensor(mask):
            mask = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0).view(np.uint8)).to(va.device)
        elif mask.dtype == torch.bool:
            mask = mask.to(torch.uint8)
    with torch.cuda.device(va.device):
        views, download = _result_slots(va.device, [("similarity", SIMILARITY_SLOTS, torch.float64)])
        cc_map = _queue_similarity(va, vb, sigma, bins, value_range, mask, return_map, views["similarity"])
        host = download()
    return similarity_from_stats(host["similarity"], sigma, bins, cc_map)


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
        views, download = _result_slots(va.device, [("counts", 4, torch.int64), ("surface", 8, torch.float64)])
        ops.mask_overlap(va, vb, threshold, out=views["counts"])
        _queue_surface_distance(va, vb, spacing, threshold, (95.0,), views["surface"])
        host = download()
    counts = tuple(int(v) for v in host["counts"])
    return SegmentationQC(dice_from_counts(*counts[:3]), counts, surface_distance_from_stats(host["surface"], (95.0,)))


class QCReference:
    """The atlas' own FC and TC probability maps on the device, uploaded once: what the warped maps of every knee are compared with.
    Each an ``Image``, an array or a [z,y,x] device tensor, as ``thickness.ThicknessAtlas`` takes them.  ``surface=True`` also keeps,
    per cartilage, the atlas surface mask and the distance map to it (computed here, once) and the spacing they are measured in: the
    Images' own, or ``spacing_xyz`` for tensors and bare arrays; a tensor is refused without it.  ``image``: the atlas image, for the
    image similarity -- uploaded and resized once to ``net_shape``, the very tensor the registration network is fed (``image_net``).
    ``roi_mm``: also the uint8 mask ``roi`` on the network grid of the voxels within that many millimetres of the atlas cartilage (both
    maps resized to ``net_shape``, the set where either is > 0.5, its distance transform under the network grid's spacing = atlas
    spacing x atlas size / network size per axis); needs a spacing, as ``surface=True`` does."""

    def __init__(self, atlas_fc, atlas_tc, surface: bool = False, spacing_xyz=None, image=None, net_shape=NET_SHAPE, roi_mm: Optional[float] = None):
        got = {kind: _map_with_spacing(m, spacing_xyz) for kind, m in zip(KINDS, (atlas_fc, atlas_tc))}
        self.maps: Dict[str, torch.Tensor] = {kind: g[0].contiguous() for kind, g in got.items()}
        self.device = self.maps["FC"].device
        self.spacing_xyz: Optional[np.ndarray] = None
        self.surfaces: Optional[Dict[str, torch.Tensor]] = None       # uint8 [z,y,x]: the atlas surface per cartilage
        self.distance_maps: Optional[Dict[str, torch.Tensor]] = None  # float32 [z,y,x]: the distance to it
        self.net_shape = tuple(int(v) for v in net_shape)
        self.image_net: Optional[torch.Tensor] = None                 # float32 net_shape: the atlas image as the registration network sees it
        self.roi: Optional[torch.Tensor] = None                       # uint8 net_shape: within roi_mm of the atlas cartilage
        self.roi_mm = None if roi_mm is None else float(roi_mm)
        if surface or roi_mm is not None:
            what = "surface=True" if surface else "roi_mm"
            if spacing_xyz is None and any(torch.is_tensor(m) for m in (atlas_fc, atlas_tc)):
                raise ValueError(f"QCReference({what}): a tensor has no spacing of its own, give spacing_xyz")
            if not np.array_equal(got["FC"][1], got["TC"][1]) or self.maps["FC"].shape != self.maps["TC"].shape:
                raise ValueError(f"QCReference({what}): the two atlas maps must share one grid and one spacing")
            self.spacing_xyz = got["FC"][1]
        if image is not None:
            vol = _map_with_spacing(image, spacing_xyz)[0].contiguous()
            if vol.device != self.device:
                raise ValueError(f"the atlas image ({vol.device}) and the atlas maps ({self.device}) must live on one GPU")
            with torch.cuda.device(self.device):                      # what VolumePipeline.register feeds the network
                self.image_net = ops.resize_trilinear(vol[None], self.net_shape)[0]
        if roi_mm is not None:
            if not self.roi_mm >= 0.0:
                raise ValueError(f"roi_mm must be >= 0, got {roi_mm}")
            with torch.cuda.device(self.device):
                # the cartilage on the network grid, and the distance to it in that grid's millimetres: existing kernels only
                # (torch's comparisons and the logical or are plumbing, once per atlas)
                net = {kind: ops.resize_trilinear(self.maps[kind][None], self.net_shape)[0] for kind in KINDS}
                cartilage = ((net["FC"] > THRESHOLD) | (net["TC"] > THRESHOLD)).to(torch.uint8)
                size_xyz = np.asarray(self.maps["FC"].shape[::-1], np.float64)
                self.roi_spacing_xyz = self.spacing_xyz * size_xyz / np.asarray(self.net_shape[::-1], np.float64)
                self.roi = (ops.distance_transform(cartilage, self.roi_spacing_xyz) <= self.roi_mm).to(torch.uint8)
        if surface:
            with torch.cuda.device(self.device):
                pairs = {kind: _surface_and_map(self.maps[kind], self.spacing_xyz, THRESHOLD) for kind in KINDS}
            self.surfaces = {kind: p[0] for kind, p in pairs.items()}
            self.distance_maps = {kind: p[1] for kind, p in pairs.items()}

    def __getitem__(self, kind: str) -> torch.Tensor:
        return self.maps[kind]


def _similarity_jobs(result, phi, reference, patient_image):
    """The comparisons of one registration, [(key, image, atlas image, mask or None)]; the warp is queued here.  Empty unless the
    reference has an image and a patient image is there."""
    if reference is None or reference.image_net is None:
        return []
    if patient_image is None:
        patient_image = getattr(result, "image_net", None)
    if patient_image is None:
        return []
    net = reference.net_shape
    if tuple(phi.shape[1:]) != net:
        raise ValueError(f"phi {tuple(phi.shape[1:])} is not on the reference's network grid {net}")
    A = _image_dev(patient_image)
    if A.device != phi.device or reference.image_net.device != phi.device:
        raise ValueError("the patient image, phi and the reference must live on one GPU")
    if tuple(A.shape) != net:
        A = ops.resize_trilinear(A[None], net)[0]           # as VolumePipeline.register resizes it
    warped = ops.grid_sample3d(A[None], phi)[0]             # A o phi: the patient image on the atlas' grid
    jobs = [("before", A, reference.image_net, None), ("after", warped, reference.image_net, None)]
    if reference.roi is not None:
        jobs += [("before_roi", A, reference.image_net, reference.roi), ("after_roi", warped, reference.image_net, reference.roi)]
    return jobs


def registration_qc(result_or_phi, image_A=None, image_B=None, reference: Optional[QCReference] = None, return_map: bool = False,
                    patient_image=None) -> RegistrationQC:
    """The QC record of one registration: of a ``pipeline.VolumeResult`` (its phi, its patient-grid and warped maps, ``meta_A`` /
    ``meta_B`` unless ``image_A`` / ``image_B`` are given), or of a bare ``phi`` (float32 [3,D,H,W], array or device tensor: the
    Jacobian, and the volume scale when both images are given).  ``patient_image`` (or the result's ``image_net``) with a reference built
    with ``image=``: the image similarity before and after the warp ``grid_sample3d(A_net, phi)`` -- the warp the registration itself
    applies to the patient image -- against the atlas image on the network grid; a full-size image is resized as the pipeline resizes it.  ``reference``: the atlas' own maps, for Dice; built with
    ``surface=True``, also for the surface distances of the warped maps (per cartilage one oai_mask_surface, one oai_edt and one
    oai_surface_distance more).  Parts whose inputs are absent are None.  Every kernel is queued on the current stream first; ONE download of the few dozen result bytes follows, the only
    synchronisation."""
    is_result = hasattr(result_or_phi, "phi") and hasattr(result_or_phi, "fc_atlas")
    phi = result_or_phi.phi if is_result else result_or_phi
    if not torch.is_tensor(phi):
        phi = torch.from_numpy(np.ascontiguousarray(phi)).cuda()
    phi = ops.check_tensor(phi, "phi")
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
        sims = _similarity_jobs(result_or_phi if is_result else None, phi, reference, patient_image)      # (key, a, b, mask)
        views, download = _result_slots(phi.device,                                                      # one buffer, one download
                                        [("jacobian", 7, torch.float64)]
                                        + [((part, kind), 4, torch.int64) for part, kind, _, _ in jobs]
                                        + [(("surface", kind), 8, torch.float64) for kind in kinds_s]
                                        + [(("similarity", key), SIMILARITY_SLOTS, torch.float64) for key, _, _, _ in sims])
        got = ops.phi_jacobian(phi, return_map=return_map, out=views["jacobian"])
        det_map = got[1] if return_map else None
        for part, kind, a, b in jobs:
            ops.mask_overlap(a, b, THRESHOLD, out=views[part, kind])
        for kind in kinds_s:
            warped = ops.check_tensor(getattr(result_or_phi, kind.lower() + "_atlas"), kind)
            if warped.shape != reference.surfaces[kind].shape:
                raise ValueError(f"the warped {kind} map {tuple(warped.shape)} is not on the reference's grid {tuple(reference.surfaces[kind].shape)}")
            surf, to_warped = _surface_and_map(warped, reference.spacing_xyz, THRESHOLD)
            ops.surface_distance(surf, reference.distance_maps[kind], reference.surfaces[kind], to_warped, (95.0,), out=views["surface", kind])
        for key, a, b, mask in sims:
            _queue_similarity(a, b, SIGMA, BINS, (0.0, 1.0), mask, False, views["similarity", key])
        host = download()
    qc = RegistrationQC(jacobian_from_stats(host["jacobian"], det_map))
    if sims:
        qc.similarity = {key: similarity_from_stats(host["similarity", key], SIGMA, BINS) for key, _, _, _ in sims}
    if image_A is not None and image_B is not None:
        qc.volume_scale = volume_scale(image_A, image_B, phi.shape[1:])
    for part, kind, _, _ in jobs:
        n_a, n_b, n_both, n_bad = (int(v) for v in host[part, kind])
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
        qc.surface = {kind: surface_distance_from_stats(host["surface", kind], (95.0,)) for kind in kinds_s}
    return qc


# ---- segmentation-shape QC (include/oai_hip.h, "Segmentation-shape QC"; csrc/components.hip) ---------------------------------------------
@dataclass
class SegmentationShape:
    """The shape of one segmentation map, with nothing to compare it with: the connected components of the set ``> threshold`` under
    ``connectivity``, and the closed cavities -- the components of its complement, under the dual connectivity (6 for 18 and 26, 26 for
    6), that do not touch the border of the volume.  All counts are exact."""
    voxels: int                  # voxels of the set
    mm3: Optional[float]         # ... times the voxel volume (None without a spacing)
    components: int
    largest_voxels: int
    largest_fraction: float      # largest_voxels / voxels, NaN for an empty set
    islands: int                 # components - 1, at least 0
    island_voxels: int           # voxels - largest_voxels
    small_components: int        # components below min_voxels
    small_voxels: int
    border_components: int       # components with a voxel on the border of the volume
    cavities: int
    cavity_voxels: int           # with a 6-connected background: binary_fill_holes(set).sum() - set.sum()
    uncertain_voxels: int        # |p > band[0]| - |p > band[1]|: voxels the network was not sure about
    nonfinite: int               # non-finite values of the map (in no set)
    connectivity: int
    min_voxels: int


SHAPE_SLOTS = 2 * ops.SUMMARY_SLOTS + 8      # int64 per map in the downloaded buffer: two labelling summaries, two overlap counts
_SHAPE_PARTS = (("set", ops.SUMMARY_SLOTS), ("complement", ops.SUMMARY_SLOTS), ("over_low", 4), ("over_high", 4))
assert sum(n for _, n in _SHAPE_PARTS) == SHAPE_SLOTS


def _shape_layout(key):
    return [((key, part), n, torch.int64) for part, n in _SHAPE_PARTS]


def dual_connectivity(connectivity: int) -> int:
    """The connectivity of the background that goes with a foreground connectivity (the digital Jordan theorem needs the pair)."""
    if connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity}")
    return 26 if connectivity == 6 else 6


def shape_from_summaries(fg, bg, n_over_lo: int, n_over_hi: int, connectivity: int, min_voxels: int,
                         voxel_mm3: Optional[float] = None) -> SegmentationShape:
    """The record of the summary of the set, the summary of its complement under the dual connectivity and the two band counts (already
    on the host)."""
    voxels, k, largest = int(fg[1]), int(fg[2]), int(fg[3])
    return SegmentationShape(voxels, None if voxel_mm3 is None else voxels * float(voxel_mm3), k, largest,
                             largest / voxels if voxels else float("nan"), max(k - 1, 0), voxels - largest, int(fg[6]), int(fg[7]), int(fg[8]),
                             int(bg[2]) - int(bg[8]), int(bg[1]) - int(bg[9]), int(n_over_lo) - int(n_over_hi), int(fg[10]),
                             int(connectivity), int(min_voxels))


def _queue_shape(vol: torch.Tensor, threshold, connectivity, min_voxels, band, views, key) -> None:
    """One map queued on the current stream, results into the views of ``_shape_layout(key)``: nothing is returned to the host here."""
    ops.label_components(vol, threshold, connectivity, False, min_voxels, return_labels=False, out=views[key, "set"])
    ops.label_components(vol, threshold, dual_connectivity(connectivity), True, 0, return_labels=False, out=views[key, "complement"])
    ops.mask_overlap(vol, None, float(band[0]), out=views[key, "over_low"])
    ops.mask_overlap(vol, None, float(band[1]), out=views[key, "over_high"])


def _shape_from_host(host, key, connectivity, min_voxels, spacing) -> SegmentationShape:
    return shape_from_summaries(host[key, "set"], host[key, "complement"], host[key, "over_low"][0], host[key, "over_high"][0],
                                connectivity, min_voxels, None if spacing is None else float(np.prod(np.asarray(spacing, np.float64))))


def _check_shape_args(connectivity, min_voxels, band) -> None:
    dual_connectivity(connectivity)
    if int(min_voxels) < 0:
        raise ValueError(f"min_voxels must be >= 0, got {min_voxels}")
    if len(band) != 2 or not float(band[0]) <= float(band[1]):
        raise ValueError(f"band must be (low, high) with low <= high, got {band!r}")


def segmentation_shapes(maps: Dict[str, object], spacing_xyz=None, threshold: float = 0.5, connectivity: int = 26, min_voxels: int = 0,
                        band=(0.1, 0.9)) -> Dict[str, SegmentationShape]:
    """``segmentation_shape`` of several maps on one GPU, all queued before the ONE download."""
    _check_shape_args(connectivity, min_voxels, band)
    got = {key: _map_with_spacing(m, spacing_xyz) for key, m in maps.items()}
    vols = {key: g[0].contiguous() for key, g in got.items()}
    spacing = {key: (None if spacing_xyz is None and (torch.is_tensor(maps[key]) or isinstance(maps[key], np.ndarray)) else g[1])
               for key, g in got.items()}
    if not vols:
        return {}
    device = next(iter(vols.values())).device
    if any(v.device != device for v in vols.values()):
        raise ValueError("the maps must live on one GPU")
    with torch.cuda.device(device):
        views, download = _result_slots(device, [slot for key in vols for slot in _shape_layout(key)])
        for key, vol in vols.items():
            _queue_shape(vol, threshold, connectivity, min_voxels, band, views, key)
        host = download()
    return {key: _shape_from_host(host, key, connectivity, min_voxels, spacing[key]) for key in vols}


def segmentation_shape(map, spacing_xyz=None, threshold: float = 0.5, connectivity: int = 26, min_voxels: int = 0,
                       band=(0.1, 0.9)) -> SegmentationShape:
    """The shape record of one probability map (an ``Image``, an array or a [z,y,x] device tensor, as ``surface_distance`` takes them;
    ``spacing_xyz`` goes with arrays and tensors, and without it ``mm3`` is None): two ``ops.label_components`` -- the set ``> threshold``
    under ``connectivity``, its complement under the dual connectivity -- and two ``ops.mask_overlap`` for the band of uncertain
    probabilities, queued into one int64 buffer; ONE download, the only synchronisation.  No threshold for "bad" is built in: the
    record is data."""
    return segmentation_shapes({"map": map}, spacing_xyz, threshold, connectivity, min_voxels, band)["map"]


def clean_segmentation(map, keep_largest: bool = True, min_voxels: int = 0, threshold: float = 0.5, connectivity: int = 26) -> torch.Tensor:
    """The map as a float32 device tensor with the voxels of dropped components set to 0.  ``keep_largest``: only the largest
    component of the set ``> threshold`` stays (on a tie the one that comes first in raster order: the summary's label); otherwise every
    component of at least ``min_voxels`` voxels stays.  Voxels that are not in the set are left as they are.  One labelling call; the
    choice is made on the device from the per-voxel sizes and the summary (the element-wise ``torch.where`` is plumbing): no host round
    trip and no synchronisation."""
    if int(min_voxels) < 0:
        raise ValueError(f"min_voxels must be >= 0, got {min_voxels}")
    vol = _image_dev(map)
    with torch.cuda.device(vol.device):
        summary, labels, sizes = ops.label_components(vol, threshold, connectivity, False, int(min_voxels), return_labels=bool(keep_largest),
                                                      return_sizes=not keep_largest)
        drop = (labels != 0) & (labels != summary[4].to(torch.int32)) if keep_largest else (sizes != 0) & (sizes < int(min_voxels))
        return torch.where(drop, torch.zeros((), dtype=vol.dtype, device=vol.device), vol)


def result_segmentation_shapes(result, **kwargs) -> Dict[str, SegmentationShape]:
    """``{"FC": ..., "TC": ...}``: the shape records of the patient-grid maps ``fc`` / ``tc`` of a ``pipeline.VolumeResult``, with the
    spacing of its ``meta_A`` (``mm3`` is None without one).  Both maps are queued before the one download."""
    meta = getattr(result, "meta_A", None)
    spacing = None if meta is None else np.asarray(as_image(meta).spacing, np.float64)
    return segmentation_shapes({kind: getattr(result, kind.lower()) for kind in KINDS}, spacing, **kwargs)


# ---- thickness QC (include/oai_hip.h, "Thickness QC"; csrc/local_thickness.hip) ----------------------------------------------------------
@dataclass
class LocalThickness:
    """The local thickness of the set ``> threshold`` of one map, in the units of the spacing: at a voxel the diameter of the largest
    ball that contains the voxel and stays inside the set (Hildebrand and Ruegsegger).  No mesh, no inner/outer split, no atlas and no
    phi take part.  ``radius`` "voxel": the balls' radii are the exact distances of the voxel centres to the nearest voxel outside the
    set, so a slab of t voxels along an axis of spacing s reads 2 ceil(t / 2) s, between t s and (t + 1) s; "mesh": their distances to
    the raw marching-cubes surface of the map, sub-voxel.  Without a centre (an empty set, or a set that fills the volume and has no
    complement to measure to) every statistic is NaN and the counts stay."""
    voxels: int                  # voxels of the set
    mm3: Optional[float]         # ... times the voxel volume (None without a spacing)
    mean: float                  # over the voxels of the set, from the device's two fp64 sums, on the host in fp64
    std: float                   # population standard deviation
    median: float                # np.percentile of the float32 map on the set, 50
    p95: float
    max: float
    surface_mean: float          # the same map on the set's surface voxels (mask_surface "surface"): area-like weighting, closer to
    surface_median: float        # what the mesh thickness averages over
    capped_centres: int          # centres whose window was above max_window_voxels: not 0 = the map is a lower bound
    work: int                    # voxel tests done
    radius: str                  # "voxel" | "mesh"
    thickness_map: Optional[torch.Tensor] = None     # float32 [z,y,x] on the device (return_map=True only)


THICKNESS_RADII = ("voxel", "mesh")
_THICKNESS_PARTS = (("scatter", ops.THICKNESS_SLOTS, torch.int64), ("set", ops.STATS_SLOTS, torch.float64),
                    ("surface", ops.STATS_SLOTS, torch.float64))


def _thickness_layout(key):
    return [((key, part), n, dtype) for part, n, dtype in _THICKNESS_PARTS]


def thickness_from_stats(scatter, over_set, over_surface, radius: str, voxel_mm3: Optional[float] = None,
                         thickness_map: Optional[torch.Tensor] = None) -> LocalThickness:
    """The record of the four integers of ``ops.local_thickness`` and the eight doubles of ``ops.masked_stats`` over the set and over
    its surface (already on the host)."""
    centres, work, capped = int(scatter[0]), int(scatter[1]), int(scatter[2])
    s, f = [float(v) for v in over_set], [float(v) for v in over_surface]
    voxels, nan = int(s[0]), float("nan")
    if centres > 0 and voxels > 0:
        mean = s[1] / voxels
        std = 0.0 if s[3] == s[4] else math.sqrt(max(s[2] / voxels - mean * mean, 0.0))       # min == max: one value, whatever the sums rounded to
        figures = (mean, std, s[5], s[6], s[4], f[1] / f[0] if f[0] > 0 else nan, f[5])
    else:
        figures = (nan,) * 7
    return LocalThickness(voxels, None if voxel_mm3 is None else voxels * float(voxel_mm3), *figures, capped, work, radius, thickness_map)


def mesh_radius_points(vol: torch.Tensor, spacing_xyz, threshold: float = 0.5):
    """(idx int64 [n,3] (z,y,x) of the set's voxels, their centres float32 [n,3] (x,y,z) in physical units, verts, faces of the raw
    marching cubes of the map at the threshold): what ``radius="mesh"`` measures from and to.  ``torch.nonzero`` is plumbing."""
    from .mesh_processing import _marching_cubes_dev
    idx = torch.nonzero(ops.mask_surface(vol, threshold, "set"))
    pts = (idx.flip(1).to(torch.float32) * torch.tensor([float(v) for v in spacing_xyz], dtype=torch.float32, device=vol.device)).contiguous()
    verts, faces = _marching_cubes_dev(vol, threshold, spacing_xyz)
    return idx, pts, verts, faces


def _radius_field(vol: torch.Tensor, spacing_xyz, threshold: float, radius: str) -> torch.Tensor:
    """The float64 squared-radius field of the set ``> threshold``: zero outside the set."""
    if radius == "voxel":       # the EDT to the complement is zero on the complement itself, and +inf everywhere when there is none
        return ops.distance_transform(ops.mask_surface(vol, threshold, "complement"), spacing_xyz, return_squared=True)[1]
    from .mesh_processing import _distance_dev
    idx, pts, verts, faces = mesh_radius_points(vol, spacing_xyz, threshold)
    rsq = torch.zeros(tuple(vol.shape), dtype=torch.float64, device=vol.device)
    if int(idx.shape[0]) and int(faces.shape[0]):
        d = _distance_dev(pts, verts, faces).to(torch.float64)
        rsq[idx[:, 0], idx[:, 1], idx[:, 2]] = d * d
    return rsq


def _queue_thickness(vol: torch.Tensor, spacing_xyz, threshold, radius, max_window_voxels, views, key) -> torch.Tensor:
    """One map queued on the current stream, results into the views of ``_thickness_layout(key)``; returns the device map."""
    rsq = _radius_field(vol, spacing_xyz, threshold, radius)
    thick = ops.local_thickness(rsq, spacing_xyz, max_window_voxels, out=views[key, "scatter"])
    ops.masked_stats(thick, ops.mask_surface(vol, threshold, "set"), (50.0, 95.0), out=views[key, "set"])
    ops.masked_stats(thick, ops.mask_surface(vol, threshold, "surface"), (50.0,), out=views[key, "surface"])
    return thick


def local_thicknesses(maps: Dict[str, object], spacing_xyz=None, threshold: float = 0.5, radius: str = "voxel", return_map: bool = False,
                      max_window_voxels: int = ops.MAX_WINDOW_VOXELS) -> Dict[str, LocalThickness]:
    """``local_thickness`` of several maps on one GPU, all queued before the ONE download."""
    if radius not in THICKNESS_RADII:
        raise ValueError(f"radius must be one of {THICKNESS_RADII}, got {radius!r}")
    if int(max_window_voxels) <= 0:
        raise ValueError(f"max_window_voxels must be > 0, got {max_window_voxels}")
    got = {key: _map_with_spacing(m, spacing_xyz) for key, m in maps.items()}
    vols = {key: g[0].contiguous() for key, g in got.items()}
    if not vols:
        return {}
    has_spacing = {key: not (spacing_xyz is None and (torch.is_tensor(maps[key]) or isinstance(maps[key], np.ndarray))) for key in vols}
    device = next(iter(vols.values())).device
    if any(v.device != device for v in vols.values()):
        raise ValueError("the maps must live on one GPU")
    with torch.cuda.device(device):
        views, download = _result_slots(device, [slot for key in vols for slot in _thickness_layout(key)])
        thick = {key: _queue_thickness(vol, got[key][1], threshold, radius, int(max_window_voxels), views, key) for key, vol in vols.items()}
        host = download()
    return {key: thickness_from_stats(host[key, "scatter"], host[key, "set"], host[key, "surface"], radius,
                                      float(np.prod(got[key][1])) if has_spacing[key] else None, thick[key] if return_map else None)
            for key in vols}


def local_thickness(map, spacing_xyz=None, threshold: float = 0.5, radius: str = "voxel", return_map: bool = False,
                    max_window_voxels: int = ops.MAX_WINDOW_VOXELS) -> LocalThickness:
    """The local-thickness record of one probability map (an ``Image``, an array or a [z,y,x] device tensor, as ``surface_distance``
    takes them; ``spacing_xyz`` goes with arrays and tensors: unit without it, and ``mm3`` is None): the squared-radius field of the set
    ``> threshold`` (``radius`` "voxel": one ``ops.mask_surface`` and one ``ops.distance_transform`` of the complement; "mesh": the
    point-to-mesh distance of the set's voxel centres to the raw marching cubes of the map, which reads the mesh's size back), one
    ``ops.local_thickness`` and two ``ops.masked_stats`` -- over the set and over its surface voxels -- queued into one buffer; ONE
    download.  ``capped_centres`` not 0: centres above ``max_window_voxels`` were left out and the figures are lower bounds.  No
    threshold for "bad" is built in: the record is data, to be put beside the mesh-based thickness."""
    return local_thicknesses({"map": map}, spacing_xyz, threshold, radius, return_map, max_window_voxels)["map"]


def result_local_thicknesses(result, **kwargs) -> Dict[str, LocalThickness]:
    """``{"FC": ..., "TC": ...}``: the local-thickness records of the patient-grid maps ``fc`` / ``tc`` of a ``pipeline.VolumeResult``,
    with the spacing of its ``meta_A`` (unit, and ``mm3`` None, without one).  Both maps are queued before the one download."""
    meta = getattr(result, "meta_A", None)
    spacing = None if meta is None else np.asarray(as_image(meta).spacing, np.float64)
    return local_thicknesses({kind: getattr(result, kind.lower()) for kind in KINDS}, spacing, **kwargs)


# ---- mesh QC: the surface the mesh-based thickness is measured on (csrc/mesh_quality.hip) -------------------------------------------------
@dataclass
class MeshQuality:
    """Topology and geometry of one triangle mesh (include/oai_hip.h, "Mesh quality").  ``topology``: the integer record of
    mesh_processing.mesh_topology by name (mesh_processing.TOPOLOGY_FIELDS), ``geometry``: the fp64 record of mesh_geometry
    (GEOMETRY_FIELDS; lengths, areas and the volume in the units of the vertices -- mm, mm2, mm3 for the pipeline's meshes).
    ``components``: connected components of the face graph (mesh_components_device) less the vertices that no face with edges names;
    exact on a mesh without degenerate faces.  ``intersecting_pairs`` /
    ``intersecting_faces``: pairs of faces without a common vertex of which one's edge properly pierces the other, and the faces in such
    pairs; None when not requested.  Folds between faces that share a vertex, coplanar overlap and mere touching are not seen."""
    topology: Dict[str, int]
    geometry: Dict[str, float]
    components: int
    intersecting_pairs: Optional[int] = None
    intersecting_faces: Optional[int] = None

    @property
    def faces(self) -> int:
        return self.topology["faces"]

    @property
    def closed(self) -> bool:
        """A closed, consistently oriented 2-manifold as far as edges tell: no boundary, misoriented or non-manifold edge, no degenerate face."""
        t = self.topology
        return not (t["boundary_edges"] or t["misoriented_edges"] or t["non_manifold_edges"] or t["degenerate_faces"])

    @property
    def volume_mm3(self) -> Optional[float]:
        """|signed volume| of a closed mesh; None when it is not closed (the sum then depends on the origin)."""
        return abs(self.geometry["signed_volume"]) if self.closed else None

    @property
    def genus_sum(self) -> Optional[float]:
        """The genera of a closed mesh's components added up: chi = 2 components - 2 genus_sum.  None when it is not closed."""
        return (2 * self.components - self.topology["euler_characteristic"]) / 2 if self.closed else None


@dataclass
class SplitQuality:
    """The mesh QC of an inner / outer split: the whole mesh (with the interface figures of its ``side``), each sub-mesh, and from the
    whole mesh's record the faces in neither sub-mesh and the inner / outer interface -- its edges, its loops (connected components of
    the interface-edge graph: one per sheet when the split is clean, more when a patch is mislabelled) and its length."""
    whole: MeshQuality
    inner: MeshQuality
    outer: MeshQuality
    unassigned_faces: int
    interface_edges: int
    interface_loops: int
    interface_length: float


_MQ_INTS = 16 + 4 + 1                     # topology record, intersection record, component roots
_MQ_ROW = _MQ_INTS + 16                   # ... and the geometry record, its float64 bits carried as int64


def _queue_mesh_quality(v: torch.Tensor, f: torch.Tensor, side: Optional[torch.Tensor], self_intersections: bool, q_min: float, row: torch.Tensor) -> None:
    """Everything of one mesh into its int64 row of the caller's buffer, nothing downloaded besides what the grid parameters and the
    component rounds read back."""
    from . import mesh_processing as mp
    n = int(v.shape[0])
    cls, _ = mp._mesh_topology_dev(f, n, side, out=row[0:16])
    if self_intersections:
        mp._mesh_self_intersections_dev(v, f, out=row[16:20])
    else:
        row[16:20] = -1
    if n:
        label = mp.mesh_components_device(f, n)
        roots = (label == torch.arange(n, dtype=torch.int32, device=v.device)).sum()
        row[20] = torch.clamp(roots - (n - row[2]), min=0)       # a vertex that no face names is a component of its own there: left out
    else:
        row[20] = 0
    geo = torch.empty(16, dtype=torch.float64, device=v.device)
    mp._mesh_geometry_dev(v, f, cls, None, q_min, out=geo)
    row[_MQ_INTS:] = geo.view(torch.int64)


def _mesh_quality_from_host(row: np.ndarray) -> MeshQuality:
    from . import mesh_processing as mp
    si = None if row[16] < 0 else row[16:20]
    mp.check_mesh_records(topology=row[0:16], intersections=si)
    topo = {k: int(row[i]) for i, k in enumerate(mp.TOPOLOGY_FIELDS)}
    g = row[_MQ_INTS:].view(np.float64)
    geo = {k: float(g[i]) for i, k in enumerate(mp.GEOMETRY_FIELDS)}
    return MeshQuality(topo, geo, int(row[20]), None if si is None else int(si[0]), None if si is None else int(si[1]))


def _mesh_qualities(meshes, self_intersections: bool, q_min: float):
    """[(verts, faces, side or None)] device tensors -> [MeshQuality]: all queued, one download."""
    dev = meshes[0][0].device
    with torch.cuda.device(dev):
        rows = torch.zeros((len(meshes), _MQ_ROW), dtype=torch.int64, device=dev)
        for (v, f, side), row in zip(meshes, rows):
            _queue_mesh_quality(v, f, side, self_intersections, q_min, row)
        host = rows.cpu().numpy()
    return [_mesh_quality_from_host(r) for r in host]


def mesh_quality(mesh, side=None, self_intersections: bool = True, q_min: float = 0.1) -> MeshQuality:
    """The MeshQuality of a ``mesh_processing.Mesh``: is it closed and consistently oriented, how many pieces, what area and volume,
    how ragged are its triangles, does it fold through itself.  ``side``: int8 per face (-1 / 0 / +1) for the interface figures.
    No threshold
    and no pass / fail policy.  Raises ValueError on a face index outside the vertices."""
    from . import _lib, mesh_processing as mp
    _lib.load()
    v, f = mp._dev(mesh.verts, np.float32, (3,)), mp._dev(mesh.faces, np.int32, (3,))
    s = None if side is None else mp._dev(side, np.int8, device=f.device)
    return _mesh_qualities([(v, f, s)], self_intersections, q_min)[0]


def split_quality(split, self_intersections: bool = True, q_min: float = 0.1) -> SplitQuality:
    """The SplitQuality of a ``mesh_processing.DeviceSplit`` -- the mesh after marching cubes, the region filter, smoothing and the
    k-means split, as the distance will see it: the whole mesh with ``split.side``, and each sub-mesh of ``_sub_mesh_dev``.  Queued on
    the current stream, one download of the records at the end."""
    from . import mesh_processing as mp
    with torch.cuda.device(split.verts.device):
        (iv, if_, _), (ov, of, _) = mp._sub_mesh_dev(split, -1), mp._sub_mesh_dev(split, 1)
        whole, inner, outer = _mesh_qualities([(split.verts, split.faces, split.side), (iv, if_, None), (ov, of, None)], self_intersections, q_min)
    return SplitQuality(whole, inner, outer, whole.topology["faces_unassigned"], whole.topology["interface_edges"],
                        whole.topology["interface_loops"], whole.geometry["interface_length"])
