"""The per-knee thickness stage: what the reference's task graph ends in (dask_processing.py:46-189: ... -> get_thickness x2) and what
its demo notebook goes on to (FullDemo.ipynb: map_attributes onto the atlas inner meshes, project_thickness), as one device-resident
step behind ``VolumeResult.fc_atlas`` / ``tc_atlas``, plus a thickness IMAGE on a fixed grid.

    ThicknessAtlas(atlas_fc, atlas_tc)      once per process: the atlas inner meshes (resident map_attributes targets), their 2-D
                                            projection in mesh point order, and its raster (csrc/thickness_image.hip)
    atlas.measure(fc_atlas, tc_atlas)       per knee: marching cubes -> large regions -> edge graph -> smoothing -> device split ->
                                            inner / outer sub-mesh -> distance inner -> outer -> map_attributes onto the atlas inner
                                            vertices; one float32 vector per cartilage comes back
    atlas.measure(.., phi=, image_A=)       the same in PATIENT millimetres: both sub-meshes are pushed through phi (atlas -> patient,
                                            csrc/mesh_transform.hip) before the distance is taken; map_attributes still runs on the
                                            atlas-space inner vertices, which is what puts every knee on the atlas' vertices
    atlas.measure(fc, tc, phi=, image_A=, space="patient_grid")
                                            NATIVE thickness: the mesh is extracted, split and measured on the patient-grid maps
                                            themselves (no resample blur, the patient's own millimetres), then its inner vertices are
                                            pulled to the atlas through the inverse of phi (csrc/phi_inverse.hip) for map_attributes
    atlas.measure(.., morphometry=True)     also the figures a study tabulates, per cartilage and region (KneeThickness.morphometry): bone
                                            area, covered and denuded area, area-weighted mean thickness -- vertex areas of the atlas
                                            inner mesh as weights, covered where map_attributes found a source point inside its radius
                                            (csrc/morphometry.hip; morphometry_rows(knee) flattens a knee for a cohort table)
    atlas.image(thickness, kind)            per knee: one gather through the raster; the same pixel is the same atlas location in
                                            every knee, because map_attributes puts every knee on the atlas' vertices

The inner / outer split of the atlas and of every knee is the DEVICE split (mesh_processing.split_mesh(on_device=True): scikit-learn
>= 1.4's KMeans restated in fp64); it is the only split that keeps the stage resident.  The default host split of split_mesh runs the
installed sklearn and may label differently under an older version.

The atlas-space distance is what the reference measures, and it carries the registration's local stretch: a knee that had to be
stretched 10 % to fit the atlas reads 10 % thick.  The iso-surface extracted on the atlas grid is {x_B : p(phi(x_B)) = 0.5}; its image
under phi is the patient's own iso-surface, to interpolation accuracy, so the distance between the pushed sub-meshes is the patient's.
The push is restated from ITK's documented composite-transform behaviour and unpinned (ITK is absent), like the resample.

The host-side rules of the raster are exact, without thresholds (fc_cut, fc_face_skip, tc_face_skip below).
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import mesh_processing as mp
from . import ops
from .image import Image, as_image

KINDS = ("FC", "TC")
_TC_SPLIT_Z = 50.0                  # project_thickness: the plateaus are split at z < 50 (raw coordinate units)


# ---- host rules of the raster (numpy only) ----------------------------------------------------------------------------------------
def wrap_angle(a):
    """a folded once into (-pi, pi] (for |a| <= 3 pi)."""
    a = np.asarray(a, dtype=np.float64)
    a = np.where(a > np.pi, a - 2 * np.pi, a)
    return np.where(a <= -np.pi, a + 2 * np.pi, a)


def fc_cut(angle) -> float:
    """The rotation that takes atan2's cut out of the femoral arc: the femoral surface is an arc, and nothing says the cut at +-pi lies
    outside it.  The angles are sorted and the largest empty gap found (the gap that wraps from the last angle round to the first
    included; the first of equal gaps); the returned ``cut`` in (-pi, pi] is such that ``u = wrap_angle(angle - cut)`` has its own
    +-pi seam in the middle of that gap, i.e. the middle of the gap is the angle ``cut + pi``.  u is then contiguous over the arc (its
    extent is 2 pi minus the gap), and ``wrap_angle(u + cut)`` is the raw angle again."""
    a = np.sort(np.asarray(angle, dtype=np.float64)[np.isfinite(angle)])
    if len(a) == 0:
        raise ValueError("fc_cut: no finite angle")
    gaps = np.append(np.diff(a), a[0] + 2 * np.pi - a[-1])
    k = int(np.argmax(gaps))
    return float(wrap_angle(a[k] + 0.5 * gaps[k] - np.pi))


def fc_face_skip(u, faces) -> np.ndarray:
    """Faces with an edge whose |du| > pi after the rotation: only a surface that closes the full circle has one (it would be drawn
    across the whole image)."""
    t = np.asarray(u, dtype=np.float64)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    return (np.abs(t[:, 0] - t[:, 1]) > np.pi) | (np.abs(t[:, 1] - t[:, 2]) > np.pi) | (np.abs(t[:, 2] - t[:, 0]) > np.pi)


def tc_face_skip(z, faces) -> np.ndarray:
    """Faces whose three vertices are not on the same side of z = 50, project_thickness's plateau split: the two plateaus are
    projected separately, a face between them means nothing in the image."""
    side = (np.asarray(z, dtype=np.float32) >= _TC_SPLIT_Z)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    return (side[:, 0] != side[:, 1]) | (side[:, 1] != side[:, 2])


def tc_point_order(z) -> np.ndarray:
    """project_thickness(TC) returns the right plateau (z >= 50) first, each plateau in point order: row k of its output is mesh
    point ``tc_point_order(z)[k]``."""
    z = np.asarray(z, dtype=np.float32)
    return np.concatenate([np.nonzero(z >= _TC_SPLIT_Z)[0], np.nonzero(z < _TC_SPLIT_Z)[0]])


def _frame_of(atlas_image) -> Tuple[np.ndarray, np.ndarray]:
    """(origin, direction) of the atlas grid, from an Image (or anything as_image takes)."""
    img = as_image(atlas_image)
    return img.origin.copy(), img.direction.copy()


# ---- morphometry records (host arithmetic on the twelve slots of oai_region_stats) ------------------------------------------------------
@dataclass
class RegionMorphometry:
    """The cartilage over one region of the atlas inner (subchondral bone) surface of one knee, derived on the host from the twelve fp64
    slots of ``ops.region_stats`` (include/oai_hip.h, "Cartilage morphometry") with w = the vertex areas and t = the thickness vector:

    ``area_mm2``               sum w over the region's vertices: the bone area (tAB)
    ``covered_mm2``            sum w over its covered vertices (cAB); ``denuded_mm2`` = area - covered (dAB), ``denuded_fraction`` = denuded / area
    ``mean_thickness_covered`` sum w t / sum w over the measured vertices (covered and finite): ThCcAB
    ``mean_thickness_total``   sum w t / area: denuded bone counts as thickness 0 (ThCtAB)
    ``std``                    area-weighted population standard deviation over the measured vertices; exactly 0 when min == max
    ``min`` / ``max``          over the measured vertices
    ``vertex_mean`` / ``vertex_std``  the unweighted figures over the measured vertices, for comparison: they weigh the surface by sampling density
    ``n_vertices`` / ``n_covered`` / ``n_measured``  the three counts

    ``space`` is the KneeThickness' ("atlas": mm2 on the atlas mesh; "patient" / "patient_grid": on the atlas mesh pushed through phi,
    the patient's own mm2); ``cover`` the coverage rule: "footprint" (covered exactly where map_attributes took the mean: a source
    point within the atlas' radius) or a distance in mm (covered where the closest source point is at most that far).  An empty
    region, and a cartilage that could not be measured, have NaN figures; nothing raises."""
    kind: str
    region: str
    space: str
    cover: Union[str, float]
    n_vertices: int
    n_covered: int
    n_measured: int
    area_mm2: float
    covered_mm2: float
    denuded_mm2: float
    denuded_fraction: float
    mean_thickness_covered: float
    mean_thickness_total: float
    std: float
    min: float
    max: float
    vertex_mean: float
    vertex_std: float

    @classmethod
    def from_slots(cls, kind: str, region: str, slots, space: str = "atlas", cover: Union[str, float] = "footprint",
                   failed: bool = False) -> "RegionMorphometry":
        """``slots``: the region's row of ``ops.region_stats``.  ``failed``: the cartilage could not be measured -- the area and the vertex
        count are kept, every other figure is NaN and the other counts 0."""
        s = [float(v) for v in slots]
        nan = float("nan")
        area = s[3]
        if failed:
            return cls(kind, region, space, cover, int(s[0]), 0, 0, area, *([nan] * 10))
        covered = s[4]
        denuded = area - covered
        mean_c = mean_t = std = lo = hi = v_mean = v_std = nan
        if s[0] > 0:
            mean_t = s[6] / area if area > 0 else nan
        if s[2] > 0:
            lo, hi = s[8], s[9]
            mean_c = s[6] / s[5] if s[5] > 0 else nan
            v_mean = s[10] / s[2]
            if lo == hi:                                           # one value, whatever the sums rounded to
                std = v_std = 0.0
            else:
                std = math.sqrt(max(s[7] / s[5] - mean_c * mean_c, 0.0)) if s[5] > 0 else nan
                v_std = math.sqrt(max(s[11] / s[2] - v_mean * v_mean, 0.0))
        return cls(kind, region, space, cover, int(s[0]), int(s[1]), int(s[2]), area, covered, denuded, denuded / area if area > 0 else nan,
                   mean_c, mean_t, std, lo, hi, v_mean, v_std)


@dataclass
class CartilageMorphometry:
    """One cartilage of one knee: ``all`` = the whole atlas inner surface, ``regions`` = one record per named region of
    ``ThicknessAtlas.regions[kind]`` in label order (a vertex labelled -1 is in ``all`` only)."""
    kind: str
    all: RegionMorphometry
    regions: Dict[str, RegionMorphometry] = field(default_factory=dict)

    def __getitem__(self, region: str) -> RegionMorphometry:
        return self.all if region == "all" else self.regions[region]


def morphometry_rows(knee) -> List[dict]:
    """A knee's morphometry as plain dicts, one per cartilage and region ("all" first): kind, region and every field of
    RegionMorphometry.  ``knee``: a KneeThickness or its ``morphometry`` dict.  A cohort table is
    ``[dict(row, knee=i) for i, k in knees for row in morphometry_rows(k)]``."""
    morph = knee.morphometry if isinstance(knee, KneeThickness) else knee
    return [asdict(r) for kind in KINDS if kind in morph for r in (morph[kind].all, *morph[kind].regions.values())]


@dataclass
class KneeThickness:
    """Cartilage thickness of one knee on the atlas inner vertices: float32 [n_fc], [n_tc] (numpy, or device tensors with
    ``keep_on_device``).  A cartilage that could not be measured is all NaN and has its reason in ``errors["FC"]`` / ``errors["TC"]``.
    ``space``: "atlas" = distances taken on the atlas grid (the reference's), "patient" = on the meshes pushed through phi, the patient's
    own millimetres; then ``outside[kind]`` counts the pushed vertices (inner and outer) that fell outside phi's buffer and moved by the
    affines alone.  "patient_grid" = distances taken on the mesh of the patient-grid maps, whose inner vertices were pulled to the atlas
    through the inverse of phi: ``outside[kind]`` counts the pulled vertices whose preimage lies outside phi's buffer, ``unconverged[kind]``
    those the solver could not place (inside a fold of phi), which moved by the affines alone.
    ``morphometry`` ({"FC": CartilageMorphometry, "TC": ...}) and ``coverage`` (per cartilage a uint8 vector on the atlas vertices, 1 where
    the vertex is covered under the rule used; numpy or device like the vectors) are filled by ``measure(..., morphometry=)`` only."""
    fc: Union[np.ndarray, torch.Tensor]
    tc: Union[np.ndarray, torch.Tensor]
    errors: Dict[str, str] = field(default_factory=dict)
    space: str = "atlas"
    outside: Dict[str, int] = field(default_factory=dict)
    unconverged: Dict[str, int] = field(default_factory=dict)
    morphometry: Dict[str, CartilageMorphometry] = field(default_factory=dict)
    coverage: Dict[str, Union[np.ndarray, torch.Tensor]] = field(default_factory=dict)
    mesh_qc: Optional[Dict[str, object]] = None          # {"FC": qc.SplitQuality, "TC": ...} with measure(..., mesh_qc=True)

    def __getitem__(self, kind: str):
        return {"FC": self.fc, "TC": self.tc}[kind]


class ThicknessAtlas:
    """Everything about the atlas that is the same for every knee, built once per process from the atlas' own FC and TC probability
    maps (FullDemo.ipynb reads atlas_fc.nii.gz / atlas_tc.nii.gz): each an ``Image``, an array, or a [z,y,x] device tensor with
    ``spacing_xyz``.

    ``inner[kind]``      the atlas inner mesh (host ``Mesh``); its vertices stay on the device as the map_attributes targets
    ``uv[kind]``         float64 [n,2], the 2-D projection in MESH POINT ORDER: vertex i of ``inner[kind]`` owns ``uv[kind][i]``.
                         FC: (angle rotated by ``cut``, z); TC: project_thickness's (x, y) put back from its right-plateau-first order
    ``point_order[kind]`` row k of project_thickness's output is mesh point ``point_order[kind][k]`` (FC: the identity)
    ``raster[kind]``     the ThicknessRaster of ``image_shape``; ``cut`` = the FC rotation: pixel column i is the raw angle
                         ``wrap_angle(lo[0] + (i + 0.5) * step[0] + cut)``
    ``projection_errors[kind]``  a projection that does not exist (project_thickness's ValueError: a tibial atlas with an empty
                         plateau): ``measure`` works all the same, ``image`` / ``scatter`` of that cartilage raise it.

    Both the atlas and every knee are split on the device (sklearn >= 1.4 semantics, see mesh_processing.split_mesh): the only split
    that keeps the stage resident.  ``min_cells`` (an int, or one per cartilage) is get_mesh's region filter, used for the atlas and
    for every knee; ``radius`` is map_attributes'.  ``image_shape`` (H, W) is an API default, not a tuned number.

    ``atlas_image``: the atlas grid's geometry (an Image; only its origin and direction are used) for patient-space ``measure``.  Maps
    given as Images carry their own; a tensor or an array has none, and patient space then needs this argument here or at ``measure``."""

    def __init__(self, atlas_fc, atlas_tc, spacing_xyz=None, image_shape: Tuple[int, int] = (256, 256), min_cells=3000, radius: float = 1.0,
                 atlas_image=None):
        self.image_shape = (int(image_shape[0]), int(image_shape[1]))
        self.min_cells = {k: int(min_cells[k] if isinstance(min_cells, dict) else min_cells) for k in KINDS}
        self.radius = float(radius)
        self.inner: Dict[str, mp.Mesh] = {}
        self.uv: Dict[str, np.ndarray] = {}
        self.point_order: Dict[str, np.ndarray] = {}
        self.raster: Dict[str, mp.ThicknessRaster] = {}
        self.projection_errors: Dict[str, str] = {}
        self.cut = 0.0
        self._targets: Dict[str, torch.Tensor] = {}
        self._scatter: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}
        self.spacing: Dict[str, np.ndarray] = {}            # each map's own (x, y, z) spacing: measure's default for that cartilage
        self.frame: Dict[str, Optional[Tuple[np.ndarray, np.ndarray]]] = {}     # each map's (origin, direction); None: built from a bare tensor or array
        self.shape: Dict[str, Tuple[int, int, int]] = {}    # each map's (z, y, x) shape: the atlas grid, for "patient_grid"
        self.device = None
        self.regions: Dict[str, Tuple[np.ndarray, Tuple[str, ...]]] = {}       # per cartilage (int32 label per inner vertex, region names): set_regions
        self._region_labels: Dict[str, torch.Tensor] = {}                      # the labels on the device, and the atlas-space vertex areas:
        self._area: Dict[str, torch.Tensor] = {}                               # both made at the first summary that needs them
        for kind, probmap in zip(KINDS, (atlas_fc, atlas_tc)):
            vol, sp, origin, direction = mp._probmap_dev(probmap, spacing_xyz)
            self.spacing[kind] = sp
            self.shape[kind] = tuple(int(v) for v in vol.shape)
            if atlas_image is not None:
                self.frame[kind] = _frame_of(atlas_image)
            else:
                self.frame[kind] = None if isinstance(probmap, (torch.Tensor, np.ndarray)) else (origin, direction)
            if self.device is None:
                self.device = vol.device
            iv, if_, _ = mp._sub_mesh_dev(mp._resident_split(vol, sp, kind, self.min_cells[kind]), -1)
            if iv.shape[0] == 0:
                raise ValueError(f"ThicknessAtlas: the atlas {kind} map has no inner surface")
            self._targets[kind] = iv
            self.inner[kind] = mp.Mesh(iv.cpu().numpy(), if_.cpu().numpy())
            self._set_default_regions(kind)
            try:
                self._project(kind)
            except ValueError as e:
                self.projection_errors[kind] = str(e)

    def _project(self, kind: str) -> None:
        mesh = self.inner[kind]
        n = len(mesh.verts)
        x, y, _ = mp.project_thickness(mp.Mesh(mesh.verts, mesh.faces, {"Distance": np.zeros(n, np.float32)}), kind)
        uv = np.empty((n, 2), dtype=np.float64)
        if kind == "FC":
            order = np.arange(n)
            self.cut = fc_cut(x)
            uv[:, 0], uv[:, 1] = wrap_angle(x - self.cut), y
            skip = fc_face_skip(uv[:, 0], mesh.faces)
        else:
            order = tc_point_order(mesh.verts[:, 2])
            uv[order, 0], uv[order, 1] = x, y
            skip = tc_face_skip(mesh.verts[:, 2], mesh.faces)
        self._scatter[kind], self.point_order[kind], self.uv[kind] = (x, y), order, uv
        with torch.cuda.device(self.device):
            self.raster[kind] = mp.thickness_image_build(uv, mesh.faces, skip, self.image_shape)

    def n_points(self, kind: str) -> int:
        return len(self.inner[kind].verts)

    # ---- regions of the morphometry ------------------------------------------------------------------------------------------------
    def _set_default_regions(self, kind: str) -> None:
        """No anatomy is invented: FC has no named region (the whole surface is reported as "all" in any case); TC has the two plateaus of
        project_thickness's own split at z = 50 (a NaN z is in neither)."""
        if kind == "FC":
            self.set_regions(kind, np.full(self.n_points(kind), -1, np.int32), ())
        else:
            z = self.inner[kind].verts[:, 2]
            self.set_regions(kind, np.where(z < _TC_SPLIT_Z, 0, np.where(z >= _TC_SPLIT_Z, 1, -1)), ("z_lt_50", "z_ge_50"))

    def set_regions(self, kind: str, labels, names: Sequence[str]) -> None:
        """The regions ``measure(..., morphometry=)`` reports for one cartilage besides "all": an integer label per atlas inner vertex
        (vertex i of ``inner[kind]``; -1, or anything outside [0, len(names)): in no region) and the name of each label.  At most 64."""
        if kind not in KINDS:
            raise KeyError(f"kind must be one of {KINDS}, got {kind!r}")
        labels, names = np.asarray(labels), tuple(str(n) for n in names)
        if labels.shape != (self.n_points(kind),) or not np.issubdtype(labels.dtype, np.integer):
            raise ValueError(f"set_regions: labels must be {self.n_points(kind)} integers (one per inner vertex of the atlas {kind} mesh), "
                             f"got {labels.dtype} {labels.shape}")
        if len(names) > ops.MAX_REGIONS or len(set(names)) != len(names) or "all" in names:
            raise ValueError(f"set_regions: at most {ops.MAX_REGIONS} distinct names other than 'all', got {names}")
        self.regions[kind] = (np.where((labels >= 0) & (labels < len(names)), labels, -1).astype(np.int32), names)
        self._region_labels.pop(kind, None)

    def regions_from_image(self, kind: str, label_image, names: Optional[Sequence[str]] = None) -> None:
        """Regions painted on the 2-D thickness image: ``label_image`` is an [H, W] integer image on the grid of ``image`` (``image_shape``),
        and vertex i takes the label of the pixel that holds ``uv[kind][i]`` (pixel (j, i) spans [lo + i step, lo + (i + 1) step) per
        axis; the last pixel includes its upper edge).  Negative labels mean no region; ``names`` default to "label_0", "label_1", ..."""
        r = self._raster(kind)
        img = np.asarray(label_image)
        if img.shape != self.image_shape or not np.issubdtype(img.dtype, np.integer):
            raise ValueError(f"regions_from_image: label_image must be an integer image of shape {self.image_shape}, got {img.dtype} {img.shape}")
        H, W = self.image_shape
        uv = self.uv[kind]
        fin = np.isfinite(uv).all(axis=1)
        col = np.clip(np.floor((np.where(fin, uv[:, 0], r.lo[0]) - r.lo[0]) / r.step[0]), 0, W - 1).astype(np.int64)
        row = np.clip(np.floor((np.where(fin, uv[:, 1], r.lo[1]) - r.lo[1]) / r.step[1]), 0, H - 1).astype(np.int64)
        labels = np.where(fin, img[row, col], -1).astype(np.int64)
        if names is None:
            names = [f"label_{k}" for k in range(int(labels.max()) + 1)]
        self.set_regions(kind, labels, names)

    def _atlas_area(self, kind: str) -> torch.Tensor:
        """The vertex areas of the atlas inner mesh (float64 [n] on the device), computed at the first summary that needs them."""
        if kind not in self._area:
            with torch.cuda.device(self.device):
                self._area[kind] = mp._mesh_areas_dev(self._targets[kind], mp._dev(self.inner[kind].faces, np.int32, (3,), device=self.device))
        return self._area[kind]

    def _patient_area(self, kind: str, phi: torch.Tensor, image_A: Image, image_B: Image) -> torch.Tensor:
        """The vertex areas of the atlas inner mesh with its vertices pushed through phi: the patient's own mm2."""
        p2n, n2o = mp.mesh_point_affines(image_A, image_B, phi.shape[1:])
        pushed = mp._transform_points_dev(self._targets[kind], phi, p2n, n2o)
        return mp._mesh_areas_dev(pushed, mp._dev(self.inner[kind].faces, np.int32, (3,), device=self.device))

    def _queue_stats(self, kind: str, vec: torch.Tensor, weights: torch.Tensor, covered: Optional[torch.Tensor], rows: torch.Tensor) -> None:
        """Both region_stats calls of one cartilage into its rows of the knee's buffer: row 0 = the whole surface, then the named regions."""
        ops.region_stats(vec, weights, None, covered, 1, out=rows[:1])
        labels, names = self.regions[kind]
        if names:
            if kind not in self._region_labels:
                self._region_labels[kind] = mp._dev(labels, np.int32, device=self.device)
            ops.region_stats(vec, weights, self._region_labels[kind], covered, len(names), out=rows[1:])

    def _map(self, kind: str, src: torch.Tensor, faces: torch.Tensor, dist: torch.Tensor, foot: Optional[dict]) -> torch.Tensor:
        """map_attributes of one knee's inner vertices onto the atlas'; with ``foot`` also the footprint query on the same sources,
        targets and grid (count, nearest squared distance)."""
        lo, hi, _ = mp.mesh_grid_params_device(src, faces)
        vec = mp._map_attributes_dev(src, dist.reshape(1, -1), self._targets[kind], self.radius, grid=(lo, hi))[0]
        if foot is not None:
            foot[kind] = mp._point_footprint_dev(src, self._targets[kind], self.radius, grid=(lo, hi))[:2]
        return vec

    # ---- per knee -----------------------------------------------------------------------------------------------------------------
    def _split(self, vol: torch.Tensor, spacing, kind: str, mesh_qc: Optional[dict]):
        """The resident split of one map, with its SplitQuality queued into ``mesh_qc`` when that is asked for: the record is of the very
        split the distance is then taken on."""
        sp = mp._resident_split(vol, spacing, kind, self.min_cells[kind])
        if mesh_qc is not None:
            from . import qc
            mesh_qc[kind] = qc.split_quality(sp, **mesh_qc["options"])
        return sp

    def _measure_one(self, vol: torch.Tensor, spacing, kind: str, foot: Optional[dict] = None, mesh_qc: Optional[dict] = None) -> torch.Tensor:
        iv, if_, dist = mp._thickness_from_split(self._split(vol, spacing, kind, mesh_qc))
        if iv.shape[0] == 0:
            raise ValueError("map_attributes: the source mesh has no points")
        return self._map(kind, iv, if_, dist, foot)

    def _measure_one_patient(self, vol: torch.Tensor, spacing, kind: str, phi: torch.Tensor, image_A: Image, frame,
                             foot: Optional[dict] = None, mesh_qc: Optional[dict] = None) -> Tuple[torch.Tensor, int]:
        """_measure_one with both sub-meshes pushed through phi before the distance: (vector, pushed vertices outside phi's buffer)."""
        sp = self._split(vol, spacing, kind, mesh_qc)
        (iv, if_, _), (ov, of, _) = mp._sub_mesh_dev(sp, -1), mp._sub_mesh_dev(sp, 1)
        image_B = Image(np.broadcast_to(np.zeros((), np.float32), tuple(vol.shape)), spacing, *frame)       # the grid of the maps, no voxels
        p2n, n2o = mp.mesh_point_affines(image_A, image_B, phi.shape[1:])
        (piv, in_i), (pov, in_o) = (mp._transform_points_dev(v, phi, p2n, n2o, return_inside=True) for v in (iv, ov))
        dist = mp._distance_dev(piv, pov, of)                   # (the grid parameters are the pushed outer mesh's)
        if iv.shape[0] == 0:
            raise ValueError("map_attributes: the source mesh has no points")
        vec = self._map(kind, iv, if_, dist, foot)              # sources stay in atlas space: vertex correspondence across knees
        return vec, sum(int(m.numel()) - int(np.count_nonzero(m.cpu().numpy())) for m in (in_i, in_o))

    def _measure_one_patient_grid(self, vol: torch.Tensor, spacing, kind: str, phi: torch.Tensor, image_A: Image, frame,
                                  foot: Optional[dict] = None, mesh_qc: Optional[dict] = None) -> Tuple[torch.Tensor, int, int]:
        """_measure_one on a patient-grid map, with the inner vertices pulled to the atlas through the inverse of phi as map_attributes'
        sources: (vector, pulled vertices whose preimage lies outside phi's buffer, vertices that did not converge)."""
        iv, if_, dist = mp._thickness_from_split(self._split(vol, spacing, kind, mesh_qc))
        if iv.shape[0] == 0:
            raise ValueError("map_attributes: the source mesh has no points")
        image_B = Image(np.broadcast_to(np.zeros((), np.float32), self.shape[kind]), self.spacing[kind], *frame)     # the atlas grid, no voxels
        p2n, n2o = mp.mesh_point_affines(image_A, image_B, phi.shape[1:], inverse=True)
        piv, status = mp._inverse_points_dev(iv, phi, p2n, n2o, return_status=True)
        vec = self._map(kind, piv, if_, dist, foot)
        counts = np.bincount(status.cpu().numpy(), minlength=3)
        return vec, int(counts[2]), int(counts[0])

    def measure(self, fc_atlas: torch.Tensor, tc_atlas: torch.Tensor, spacing_xyz=None, keep_on_device: bool = False, phi=None, image_A=None,
                atlas_image=None, space: Optional[str] = None, morphometry: Union[bool, float] = False, mesh_qc: bool = False) -> KneeThickness:
        """Thickness of one knee on the atlas inner vertices, from the two [z,y,x] float32 device tensors of a ``VolumeResult``
        (``spacing_xyz``: the atlas grid's, default the spacing of the map this atlas was built from).  Everything stays on the device, on the
        current stream, until the two vectors; only the inner -> outer distance is computed.  Per cartilage, bit for bit,

            map_attributes(get_thickness_mesh(Image(map.cpu(), spacing), kind, min_cells=.., on_device=True)[0], atlas.inner[kind]).point_data["Distance"]

        ``phi`` (float32 [3,D,H,W], VolumeResult.phi) with ``image_A`` (the patient image's geometry, VolumeResult.meta_A): the distance
        in PATIENT space (``space == "patient"``).  The inner and outer sub-meshes are pushed through phi to the patient's "spacing"
        coordinates and the distance taken between the pushed meshes; map_attributes keeps the atlas-space inner vertices as its
        sources.  The atlas side of phi is the grid of the maps: their shape, ``spacing_xyz``, and the origin and direction of the
        Image the atlas was built from, or of ``atlas_image`` (here or at construction; required for an atlas built from bare
        tensors or arrays).  Per cartilage, bit for bit, with inner, outer = get_thickness_mesh(.., on_device=True) as above and
        T = lambda m: transform_mesh(m, phi, image_A, image_B):

            map_attributes(Mesh(inner.verts, inner.faces, {"Distance": point_distance(T(inner).verts, T(outer))}), atlas.inner[kind]).point_data["Distance"]

        ``outside[kind]`` counts the pushed vertices outside phi's buffer.  Unpinned, like the resample: ITK is absent.

        ``space``: None (default) = "atlas" without phi, "patient" with it, as above.  "patient_grid" (with ``phi`` and ``image_A``):
        NATIVE thickness.  The two maps are then the PATIENT-grid ``VolumeResult.fc`` / ``tc`` and ``spacing_xyz`` the patient's
        (default ``image_A``'s): the mesh is extracted, split and measured on them at native resolution, with no resample blur and in
        the patient's own millimetres; its inner vertices are then pulled to the atlas' "spacing" coordinates by the point solver
        (mesh_processing.transform_mesh(..., inverse=True): Newton on phi per vertex, exact to 1e-7 network voxels) and are
        map_attributes' sources, the atlas inner vertices its targets.  The atlas grid is the shape and spacing of the maps this
        atlas was built from with the origin and direction as for "patient".  ``outside[kind]`` counts the vertices whose preimage
        lies outside phi's buffer, ``unconverged[kind]`` those that did not converge and moved by the affines alone.  This space is
        UNPINNED (ITK is absent, and the reference has no such step), and the inner / outer split heuristics have only ever been run
        on atlas-grid meshes: the split assumes that the patient grid has the atlas' orientation.

        A map with no region above ``min_cells``, or an FC slab of fewer than 2 faces, raises ValueError inside those functions: that
        is caught PER CARTILAGE, the vector filled with NaN and the message kept in ``errors`` -- one bad knee must not end a cohort.
        Nothing else is caught.

        ``morphometry``: True, or a coverage distance in mm -- the knee's vectors reduced to the figures a study tabulates, in
        ``KneeThickness.morphometry`` (per cartilage a CartilageMorphometry: the whole surface and every region of ``regions[kind]``), and the
        coverage itself in ``KneeThickness.coverage``.  map_attributes never says "no cartilage here": a vertex with no source point
        inside the radius takes the value of the closest one, however far.  So a footprint query (mesh_processing.point_footprint) runs on
        the same sources, targets and grid as the map_attributes call beside it, and a vertex is COVERED exactly when map_attributes took
        the mean there (True: a source point within ``radius``), or when the closest source point is at most ``morphometry`` mm away (a
        float).  The weights are vertex areas (mesh_processing.mesh_areas) of the atlas inner mesh: in space "atlas" its own, computed
        once at the first summary; in "patient" and "patient_grid" those of its vertices pushed through this knee's phi, the patient's
        own mm2 as the thickness is the patient's mm.  The twelve-slot rows of both cartilages come down in one download.  A cartilage
        in ``errors`` gets all-NaN figures and the atlas-space area.  "Denuded" here means: no inner-surface vertex of the warped patient
        cartilage within the radius of the atlas bone surface -- that includes registration error; no pass / fail policy is built in,
        and the figures are unpinned (the reference has no such step).  False (default): nothing more is launched, no bit changes.

        ``mesh_qc``: True -- per cartilage a ``qc.SplitQuality`` in ``KneeThickness.mesh_qc``: topology, geometry and self-intersections
        of the very mesh and split the distance was then taken on (in every space: the mesh of the maps given, before any push or pull
        through phi), so that a thickness figure that is off can be traced to a surface that is open, folded, or split into patches.  A
        cartilage in ``errors`` has no record.  No threshold and no pass / fail policy.  False (default): nothing more is launched, no
        bit changes, and ``mesh_qc`` is None."""
        if morphometry is not False and morphometry is not True:
            if isinstance(morphometry, bool) or not isinstance(morphometry, (int, float)) or not morphometry >= 0:
                raise ValueError(f"morphometry must be False, True or a coverage distance >= 0 in mm, got {morphometry!r}")
        if space not in (None, "atlas", "patient", "patient_grid"):
            raise ValueError(f"space must be None, 'atlas', 'patient' or 'patient_grid', got {space!r}")
        if (phi is None) != (image_A is None):
            raise ValueError(f"patient-space thickness needs both phi and image_A: {'image_A' if image_A is None else 'phi'} is missing")
        patient = phi is not None
        if space is not None and (space != "atlas") != patient:
            raise ValueError(f"space={space!r} " + ("takes no phi" if patient else "needs phi and image_A"))
        native = space == "patient_grid"
        if patient:
            frames = {k: _frame_of(atlas_image) if atlas_image is not None else self.frame[k] for k in KINDS}
            missing = [k for k in KINDS if frames[k] is None]
            if missing:
                raise ValueError(f"patient-space thickness needs atlas_image: the atlas {'/'.join(missing)} map was a bare tensor or array, which has no origin "
                                 "or direction (pass atlas_image= here or to ThicknessAtlas)")
            image_A = as_image(image_A)
            with torch.cuda.device(self.device):
                phi = mp._dev(phi, np.float32, device=self.device)
            if phi.dim() != 4 or phi.shape[0] != 3:
                raise ValueError(f"phi must be [3,D,H,W], got {tuple(phi.shape)}")
        out, errors, outside, unconverged = {}, {}, {}, {}
        foot = None if morphometry is False else {}               # per cartilage (count, nearest squared distance) of the footprint query
        weights = {}
        mqc = {"options": {}} if mesh_qc else None
        for kind, vol in zip(KINDS, (fc_atlas, tc_atlas)):
            default = image_A.spacing if native else self.spacing[kind]
            sp = default if spacing_xyz is None else np.asarray(spacing_xyz, dtype=np.float64).reshape(3)
            with torch.cuda.device(self.device):
                vol_d = mp._probmap_dev(vol, sp)[0]
                try:
                    if native:
                        out[kind], outside[kind], unconverged[kind] = self._measure_one_patient_grid(vol_d, sp, kind, phi, image_A, frames[kind], foot, mqc)
                    elif patient:
                        out[kind], outside[kind] = self._measure_one_patient(vol_d, sp, kind, phi, image_A, frames[kind], foot, mqc)
                    else:
                        out[kind] = self._measure_one(vol_d, sp, kind, foot, mqc)
                except ValueError as e:
                    errors[kind] = str(e)
                    out[kind] = torch.full((self.n_points(kind),), float("nan"), dtype=torch.float32, device=self.device)
                if foot is not None:
                    if kind in errors or not patient:
                        weights[kind] = self._atlas_area(kind)
                    else:                                          # the atlas side of phi: the atlas grid ("patient": the grid of the maps, which is it)
                        grid_B = (self.shape[kind], self.spacing[kind]) if native else (tuple(vol_d.shape), sp)
                        image_B = Image(np.broadcast_to(np.zeros((), np.float32), grid_B[0]), grid_B[1], *frames[kind])
                        weights[kind] = self._patient_area(kind, phi, image_A, image_B)
        space = "patient_grid" if native else "patient" if patient else "atlas"
        morph, coverage = {}, {}
        if foot is not None:
            morph, coverage = self._summarise(out, errors, foot, weights, space, "footprint" if morphometry is True else float(morphometry))
            if not keep_on_device:
                coverage = {k: v.cpu().numpy() for k, v in coverage.items()}
        if not keep_on_device:
            out = {k: v.cpu().numpy() for k, v in out.items()}
        if mqc is not None:
            mqc = {k: mqc[k] for k in KINDS if k in mqc and k not in errors}
        return KneeThickness(out["FC"], out["TC"], errors, space, outside, unconverged, morph, coverage, mqc)

    def _summarise(self, out, errors, foot, weights, space: str, cover) -> Tuple[Dict[str, CartilageMorphometry], Dict[str, torch.Tensor]]:
        """The region sums of both cartilages queued into one buffer, one download, the records derived on the host."""
        n_rows = {k: 1 + len(self.regions[k][1]) for k in KINDS}
        with torch.cuda.device(self.device):
            rows = torch.empty((sum(n_rows.values()), ops.REGION_SLOTS), dtype=torch.float64, device=self.device)
            coverage, first = {}, 0
            for kind in KINDS:
                if kind in errors:
                    coverage[kind] = torch.zeros(self.n_points(kind), dtype=torch.uint8, device=self.device)
                else:
                    count, d2 = foot[kind]
                    coverage[kind] = (count > 0 if cover == "footprint" else d2 <= float(cover) * float(cover)).to(torch.uint8)
                self._queue_stats(kind, out[kind], weights[kind], coverage[kind], rows[first:first + n_rows[kind]])
                first += n_rows[kind]
            host = rows.cpu().numpy()
        morph, first = {}, 0
        for kind in KINDS:
            make = lambda name, row: RegionMorphometry.from_slots(kind, name, host[row], space, cover, failed=kind in errors)
            morph[kind] = CartilageMorphometry(kind, make("all", first), {name: make(name, first + 1 + k) for k, name in enumerate(self.regions[kind][1])})
            first += n_rows[kind]
        return morph, coverage

    def _raster(self, kind: str) -> mp.ThicknessRaster:
        if kind not in KINDS:
            raise KeyError(f"kind must be one of {KINDS}, got {kind!r}")
        if kind in self.projection_errors:
            raise ValueError(f"the atlas {kind} mesh has no 2-D projection: {self.projection_errors[kind]}")
        return self.raster[kind]

    def image(self, thickness, kind: Optional[str] = None):
        """The thickness image of one cartilage: float32 [H,W] for a vector [n], [K,H,W] for [K,n] (K knees at once); NaN where no
        face of the atlas mesh owns the pixel, and NaN spreads from NaN vertices.  An array gives an array, a device tensor a device
        tensor.  A ``KneeThickness`` gives {"FC": image, "TC": image}."""
        if isinstance(thickness, KneeThickness):
            return {k: self.image(thickness[k], k) for k in KINDS}
        with torch.cuda.device(self.device):
            return mp.thickness_image(self._raster(kind), thickness)

    def scatter(self, kind: str) -> Tuple[np.ndarray, np.ndarray]:
        """(x, y) exactly as ``project_thickness(mapped mesh, kind)`` returns them for any knee mapped onto this atlas (FC: the raw
        angle; TC: the right plateau first): the notebook's plt.scatter coordinates, computed once."""
        self._raster(kind)
        return self._scatter[kind]
