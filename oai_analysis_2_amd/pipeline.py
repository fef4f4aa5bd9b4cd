"""The per-volume hot path, device resident end to end:

    DESS volume (fp32, [z,y,x]) --segment--> FC/TC probability maps --+
                                --register--> phi (atlas -> patient) --+--> FC/TC on the atlas grid

i.e. AnalysisObject.segment + AnalysisObject.register + the two ``deform_probmap`` calls of the
reference's pipeline (test/test_all.py:54-58, dask_processing.py:46-125), without any host round trip.
Used by bench.py, the cohort driver and the multi-GPU sharding.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import TYPE_CHECKING, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .image import Image
from .registration import IconEngine, _meta_only, resample_affines
from .segmentation.engine import UNetEngine, tile_grid

if TYPE_CHECKING:
    from .qc import QCReference, RegistrationQC
    from .thickness import KneeThickness, ThicknessAtlas

TILE_ZYX = (32, 128, 128)        # patch_size (128,128,32) in x,y,z (a2)
OVERLAP_ZYX = (8, 16, 16)        # overlap_size (16,16,8) in x,y,z (analysis_object.py:23)
CROP_ZYX = (8, 16, 16)           # assemble's frame: crop_size[2], [0], [1]


@dataclass
class VolumeResult:
    fc: torch.Tensor             # [z,y,x] probability map, patient grid
    tc: torch.Tensor
    phi: torch.Tensor            # [3,D,H,W] dense map, network grid, [0,1] units
    fc_atlas: torch.Tensor       # FC pulled onto the atlas grid through phi
    tc_atlas: torch.Tensor
    overflow: Optional[torch.Tensor] = None    # int32[1] on the device: the fp16 range flag of THIS volume's segmentation
    #                                            (None with exact arithmetic).  Non-zero = the maps are invalid: repeat in fp32.
    repeated_f32: bool = False   # the fp16x3 run overflowed and these are the results of the fp32 repeat
    meta_A: Optional[Image] = None    # the patient image's geometry (metadata only, no voxel array): with phi, what takes atlas points to patient points
    meta_B: Optional[Image] = None    # the atlas image's geometry (metadata only): the other side of phi
    image_net: Optional[torch.Tensor] = None       # the patient image at network resolution, as the registration saw it (run(..., qc=QCReference(image=)) only)
    qc: Optional["RegistrationQC"] = None          # registration QC: folds and det J of phi, Dice, cartilage volume (run(..., qc=...) only)
    thickness: Optional["KneeThickness"] = None    # cartilage thickness on the atlas inner vertices (run(..., thickness=atlas) only)
    # Optional[Dict[str, qc.SegmentationShape]]: the shape record of the patient-grid maps ``fc`` / ``tc`` (run(..., seg_qc=True) only).  A
    # plain attribute and not a dataclass field, like RegistrationQC.similarity: the fields of the result stay the ones earlier tests pin.
    seg_qc = None
    # Optional[Dict[str, qc.LocalThickness]]: the mesh-free local thickness of the same maps (run(..., thickness_qc=True | "mesh") only); a
    # plain attribute for the same reason
    thickness_qc = None


class VolumePipeline:
    """Range guard of the default fp16x3 arithmetic (|activation| <= 65504): every entry point that returns results either
    checks the flag of its own volume and repeats that volume in exact fp32 (``check=True``, the default: one stream
    synchronisation AFTER everything of the volume is queued), or hands the flag snapshot back in ``VolumeResult.overflow`` for a
    caller that pipelines volumes and checks at download time (``check=False``: CohortRunner, bench.py).  Never silent."""

    def __init__(self, unet: UNetEngine, icon: IconEngine, atlas: Image, tile_zyx=TILE_ZYX, overlap_zyx=OVERLAP_ZYX,
                 crop_zyx=CROP_ZYX, batch: Optional[int] = None):
        self.unet, self.icon, self.atlas = unet, icon, atlas
        self.tile_zyx, self.overlap_zyx, self.crop_zyx, self.batch = tuple(tile_zyx), tuple(overlap_zyx), tuple(crop_zyx), batch
        self.atlas_dev = torch.from_numpy(np.ascontiguousarray(atlas.array, dtype=np.float32)).to(unet.device)
        self._atlas_net = None
        self._atlas_meta = _meta_only(atlas)
        self._side = None
        self.overlap_registration = True          # registration underneath the segmentation (+1.5 %); False serialises

    # ---- stages ---------------------------------------------------------------------------------------------------------------
    def segment(self, vol: torch.Tensor, out_mode: int = 0, tile_range: Optional[Tuple[int, int]] = None):
        blocks = self.unet.segment_tiles(vol, self.tile_zyx, self.overlap_zyx, tile_range, out_mode, self.batch, self.crop_zyx)
        if tile_range is not None:
            return blocks
        return self.unet.stitch(blocks, vol.shape, self.tile_zyx, self.overlap_zyx, self.crop_zyx)

    def _flag_snapshot(self) -> Optional[torch.Tensor]:
        """Queue (no sync) a copy-and-clear of the fp16 range flag behind the segment calls queued so far."""
        if self.unet.precision != "fp16x3":
            return None
        flag = torch.zeros(1, dtype=torch.int32, device=self.unet.device)
        self.unet.range_overflow_snapshot(flag)
        return flag

    def register(self, vol: torch.Tensor) -> torch.Tensor:
        """phi_AB with A = patient volume (fixed), B = atlas (moving): registration.py:22-27."""
        A = ops.resize_trilinear(vol[None], self.icon.net_shape)[0]
        if self._atlas_net is None:      # the atlas is the same for every volume: resize it once
            self._atlas_net = ops.resize_trilinear(self.atlas_dev[None], self.icon.net_shape)[0]
        return self.icon.phi(A, self._atlas_net)

    def resample(self, maps: torch.Tensor, phi: torch.Tensor, meta_A: Image, z_range: Optional[Tuple[int, int]] = None):
        """Both maps pulled onto the atlas grid through phi (ONE launch reads the displacement once for all maps);
        ``z_range`` = only atlas slices [z0, z1) (the z-slab shard of SURVEY 8e).  Returns [n_maps, z, y, x]."""
        b2n, n2a = resample_affines(meta_A, self.atlas, self.icon.net_shape)
        shape = tuple(self.atlas.array.shape)
        if z_range is not None:
            z0, z1 = int(z_range[0]), int(z_range[1])
            if not 0 <= z0 <= z1 <= shape[0]:
                raise ValueError("z_range outside the atlas grid")
            A1, b1 = b2n
            b2n = (A1, b1 + A1[:, 2] * float(z0))          # index_B = index_slab + (0, 0, z0) in ITK's x,y,z order
            shape = (z1 - z0, shape[1], shape[2])
        return ops.resample_maps_through_phi(maps, phi, b2n, n2a, shape)

    # ---- one volume, one GPU --------------------------------------------------------------------------------------------------
    def run(self, vol: torch.Tensor, meta_A: Image, check: bool = True, thickness: Optional["ThicknessAtlas"] = None,
            thickness_space: str = "atlas", qc=None, seg_qc: bool = False, thickness_qc=False, morphometry=False,
            mesh_qc: bool = False) -> VolumeResult:
        """``thickness``: a thickness.ThicknessAtlas -- the volume's cartilage thickness on the atlas inner vertices is measured from
        ``fc_atlas`` / ``tc_atlas`` (after the range check and the fp32 repeat, if any) and returned in ``VolumeResult.thickness``.
        None (default): nothing more is launched.  ``thickness_space``: "atlas" (default) = the distance on the atlas grid, as the
        reference takes it; "patient" = on the meshes pushed through this volume's phi, in the patient's own millimetres
        (ThicknessAtlas.measure(..., phi=, image_A=)); "patient_grid" = native thickness: the mesh is taken from the patient-grid maps
        ``fc`` / ``tc`` and its inner vertices pulled to the atlas through the inverse of phi (ThicknessAtlas.measure(..., space="patient_grid")).
        ``morphometry``: True or a coverage distance in mm, with ``thickness`` -- the knee's area-weighted regional thickness, covered and
        denuded area in ``VolumeResult.thickness.morphometry`` (ThicknessAtlas.measure(..., morphometry=)).  False (default): nothing more is
        launched.
        ``mesh_qc``: True, with ``thickness`` -- per cartilage the qc.SplitQuality of the mesh and split the thickness was measured on
        (topology, volume, self-intersections, the inner / outer interface) in ``VolumeResult.thickness.mesh_qc``
        (ThicknessAtlas.measure(..., mesh_qc=True)).  False (default): nothing more is launched and no bit changes.
        ``qc``: True, or a qc.QCReference (the atlas' own maps, for Dice) -- the registration QC record of the volume
        (qc.registration_qc: folds and det J of phi, volume scale, cartilage volume) in ``VolumeResult.qc``, computed where the thickness
        is: after the range check and the fp32 repeat.  A few small launches and one more synchronisation.  None (default): nothing more
        is launched and no bit changes.  A reference built with ``image=`` (the atlas image) adds the image similarity before and after
        the warp (``qc.similarity``) and leaves the patient image at network resolution in ``VolumeResult.image_net``.
        ``seg_qc``: True -- the reference-free shape record of the patient-grid maps (qc.segmentation_shapes: components, islands,
        cavities of ``fc`` and ``tc`` with ``meta_A``'s spacing) as ``{"FC": ..., "TC": ...}`` in ``VolumeResult.seg_qc``, computed where ``qc``
        is; both cartilages are queued before the one download.  False (default): nothing more is launched and no bit changes.
        ``thickness_qc``: True (or "voxel"), or "mesh" -- the mesh-free local thickness of the patient-grid maps (qc.local_thicknesses with
        that ``radius``: the largest inscribed ball per voxel, mean / median / p95 per cartilage, with ``meta_A``'s spacing) as ``{"FC": ...,
        "TC": ...}`` in ``VolumeResult.thickness_qc``, queued where ``seg_qc`` is; an independent figure to put beside ``thickness``.
        False (default): nothing more is launched and no bit changes."""
        if thickness_qc not in (False, True, "voxel", "mesh"):
            raise ValueError(f"thickness_qc must be False, True, 'voxel' or 'mesh', got {thickness_qc!r}")
        if qc is not None and qc is not True and not hasattr(qc, "maps"):
            raise ValueError(f"qc must be None, True or a qc.QCReference, got {qc!r}")
        if thickness_space not in ("atlas", "patient", "patient_grid"):
            raise ValueError(f"thickness_space must be 'atlas', 'patient' or 'patient_grid', got {thickness_space!r}")
        res = self._run_overlapped(vol, meta_A) if self.overlap_registration else self._run_serial(vol, meta_A)
        if check and res.overflow is not None:
            raised = bool(int(res.overflow.item()))
            self.unet.note_volume_flag(raised)              # (a calibration FILE that keeps missing the data is dropped after three volumes in a row)
            if raised:
                res = self.rerun_f32(vol, meta_A)
        if thickness is not None:
            if thickness_space == "patient_grid":
                res.thickness = thickness.measure(res.fc, res.tc, spacing_xyz=res.meta_A.spacing, phi=res.phi, image_A=res.meta_A, space="patient_grid",
                                                  morphometry=morphometry, mesh_qc=mesh_qc)
            else:
                push = dict(phi=res.phi, image_A=res.meta_A) if thickness_space == "patient" else {}
                res.thickness = thickness.measure(res.fc_atlas, res.tc_atlas, spacing_xyz=self.atlas.spacing, morphometry=morphometry, mesh_qc=mesh_qc,
                                                  **push)
        if qc is not None:
            from .qc import registration_qc
            if qc is not True and getattr(qc, "image_net", None) is not None:      # the image similarity needs the image, not only the maps
                res.image_net = ops.resize_trilinear(vol[None], self.icon.net_shape)[0]
            res.qc = registration_qc(res, reference=None if qc is True else qc)
        if seg_qc:
            from .qc import result_segmentation_shapes
            res.seg_qc = result_segmentation_shapes(res)
        if thickness_qc:
            from .qc import result_local_thicknesses
            res.thickness_qc = result_local_thicknesses(res, radius="mesh" if thickness_qc == "mesh" else "voxel")
        return res

    def rerun_f32(self, vol: torch.Tensor, meta_A: Image, sharded_group="none") -> VolumeResult:
        """The volume left fp16x3's calibrated range window (range flag: overflow or a layer far quieter than at calibration): repeat
        it with exact fp32 MFMA arithmetic (what Segmenter3DInPatchClassWise does)."""
        print("WARNING: activations outside the fp16x3 range window, repeating the volume in fp32")
        prev = self.unet.precision
        self.unet.set_precision("f32")
        try:
            res = self.run(vol, meta_A, check=False) if sharded_group == "none" else self.run_sharded(vol, meta_A, sharded_group, check=False)
        finally:
            self.unet.set_precision(prev)
        res.repeated_f32 = True
        return res

    def _run_serial(self, vol: torch.Tensor, meta_A: Image) -> VolumeResult:
        maps = self.segment(vol)
        flag = self._flag_snapshot()
        phi = self.register(vol)
        atlas_maps = self.resample(maps, phi, meta_A)
        return VolumeResult(maps[0], maps[1], phi, atlas_maps[0], atlas_maps[1], flag, meta_A=_meta_only(meta_A), meta_B=self._atlas_meta)

    def _run_overlapped(self, vol: torch.Tensor, meta_A: Image) -> VolumeResult:
        """Registration needs only the image, not its segmentation: its small, launch- and latency-bound kernels (a few dozen
        workgroups at the deep ICON levels) run on a side stream underneath the segmentation's MFMA kernels; the resample joins."""
        main = torch.cuda.current_stream()
        if self._side is None or self._side.priority != main.priority:
            self._side = torch.cuda.Stream(device=self.unet.device, priority=main.priority)      # (the compute stream's own priority: under a high-priority caller -- CohortRunner -- a default-priority side stream would starve)
        self._side.wait_stream(main)                                    # vol (and the atlas) are ready
        with torch.cuda.stream(self._side):
            phi = self.register(vol)
            phi.record_stream(main)
        maps = self.segment(vol)
        flag = self._flag_snapshot()
        main.wait_stream(self._side)
        atlas_maps = self.resample(maps, phi, meta_A)
        return VolumeResult(maps[0], maps[1], phi, atlas_maps[0], atlas_maps[1], flag, meta_A=_meta_only(meta_A), meta_B=self._atlas_meta)

    # ---- one volume, all ranks of a group (single-volume latency mode) ---------------------------------------------
    def segment_sharded(self, vol: torch.Tensor, group=None) -> torch.Tensor:
        """One volume split over the ranks of ``group`` at tile granularity: every rank runs the U-Net on
        its contiguous tile range, ONE all_gather (RCCL) gives every rank all kept-centre blocks, then stitch."""
        from . import parallel
        _, _, n_tiles = tile_grid(vol.shape, self.tile_zyx, self.overlap_zyx)
        costs = self.unet.tile_costs(vol.shape, self.tile_zyx, self.overlap_zyx, self.crop_zyx)     # border tiles are cheaper: balance the work
        eff, _, _ = tile_grid(vol.shape, self.tile_zyx, self.overlap_zyx)
        # the kernels write this rank's blocks straight into its slot of the gather buffer, the collective runs in place, and the stitch
        # reads the (ragged: 19-23 tiles per rank) buffer through a table: no copy on either side of the all_gather
        gathered = parallel.segment_tile_sharded(
            lambda rng, out: self.unet.segment_tiles(vol, self.tile_zyx, self.overlap_zyx, rng, 0, self.batch, self.crop_zyx, out=out),
            n_tiles, group, costs, block_shape=(self.unet.n_classes, *eff), dtype=torch.float32, device=self.unet.device)
        return self.unet.stitch(gathered, vol.shape, self.tile_zyx, self.overlap_zyx, self.crop_zyx)

    def run_sharded(self, vol: Optional[torch.Tensor], meta_A: Image, group=None, src: int = 0, check: bool = True) -> VolumeResult:
        """``vol`` is needed on rank ``src`` only (others may pass None): broadcast -> tile-sharded segmentation + all_gather ->
        registration replicated (0.1 TFLOP: cheaper than communicating) -> both resamples sharded by atlas z-slab + all_gather.
        The fp16 range flag is all_reduce(MAX)ed: either every rank keeps the result or every rank repeats in fp32.
        Registration QC (``run(..., qc=...)``) is out of scope here: call qc.registration_qc on the result."""
        from . import parallel
        import torch.distributed as dist
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        rank = dist.get_rank(group) if dist.is_initialized() else 0
        vol = parallel.broadcast_volume(vol, meta_A.array.shape, self.unet.device, src, group)
        # The replicated registration needs only the image: like _run_overlapped, it goes on the side stream UNDERNEATH the sharded
        # segmentation and joins before the resample.  At 8 ranks the segmentation is ~21 ms per rank, so 4.85 ms of ICON + warp
        # kernels in front of or behind it would be ~20 % of the single-volume latency.
        main = torch.cuda.current_stream()
        phi = None
        if self.overlap_registration:
            if self._side is None or self._side.priority != main.priority:
                self._side = torch.cuda.Stream(device=self.unet.device, priority=main.priority)      # (the compute stream's own priority: under a high-priority caller -- CohortRunner -- a default-priority side stream would starve)
            self._side.wait_stream(main)                                # the broadcast volume is ready
            with torch.cuda.stream(self._side):
                phi = self.register(vol)
                phi.record_stream(main)
        maps = self.segment_sharded(vol, group)
        # the range flag of the WHOLE volume: the raw state (overflow bit + per-layer maxima) is MAX-reduced over the ranks and the
        # LOW bit evaluated from that -- a rank whose tile range is all quiet background must not force every rank into the fp32
        # repeat on its own subset's census; after the reduction every rank holds the same verdict
        flag = None
        if self.unet.precision == "fp16x3":
            state = torch.zeros(self.unet.RANGE_STATE_WORDS, dtype=torch.int32, device=self.unet.device)
            self.unet.range_state_snapshot(state)
            parallel.any_rank(state, group)
            flag = self.unet.range_flag_from_state(state)
        if phi is None:
            phi = self.register(vol)
        else:
            main.wait_stream(self._side)
        nz = self.atlas.array.shape[0]
        local = self.resample(maps, phi, meta_A, parallel.slab_range_for_rank(nz, rank, world))
        atlas_maps = parallel.gather_slabs(local, nz, group)
        res = VolumeResult(maps[0], maps[1], phi, atlas_maps[0], atlas_maps[1], flag, meta_A=_meta_only(meta_A), meta_B=self._atlas_meta)
        if check and flag is not None:
            raised = bool(int(flag.item()))                 # (the same verdict on every rank: the state was MAX-reduced)
            self.unet.note_volume_flag(raised)
            if raised:
                return self.rerun_f32(vol, meta_A, sharded_group=group)
        return res
