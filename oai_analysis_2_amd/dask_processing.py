"""The task bodies of the reference's ``oai_analysis/dask_processing.py`` with PERSISTENT per-process workers.

The reference wraps these functions in ``dask.delayed`` and, inside every task, rebuilds its model
(``pretrained_models.OAI_knees_gradICON_model()`` at :77, ``Segmenter3DInPatchClassWise(...)`` at :170), moves it to the GPU, runs one
volume and deletes it again.  Here the same names take the same arguments and return the same things, but the engines behind them are
built ONCE per process (``get_worker``) and stay resident in HBM; ``process_cohort`` is the driver that replaces the task graph: every
rank pulls the next volume from one shared queue (``parallel.VolumeQueue``) and streams it through its GPU (``cohort.CohortRunner``:
upload of i+1, compute of i, download of i-1 overlap).

    image_normalize          :10-26    percentile window -> [0,1] (device kernel, oai_image_normalize)
    readimage                :29-43    itk.imread(path, itk.F)    (NIfTI via io_nifti)
    register_images_delayed  :46-92    read A, B; normalise A; ICON register_pair -> (phi_AB, image_A, image_B)
    deform_probmap_delayed   :95-111   ITK resample of a probability map through phi_AB onto image_B's grid
    get_thickness            :114-122  inner cartilage surface with per-point thickness
    segment_method           :125-189  read; normalise; Segmenter3DInPatchClassWise.segment -> (FC, TC) probability maps
"""
from __future__ import annotations

import os
from typing import Iterable, Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .image import Image, as_image


def image_normalize(image, window_min_perc, window_max_perc, output_min, output_max) -> Image:
    """Percentile intensity window -> [output_min, output_max], like the reference; computed on the GPU."""
    img = as_image(image)
    vol = torch.from_numpy(np.array(img.array, dtype=np.float32, order="C", copy=True)).cuda()      # (a file-backed array may be read-only)
    out = ops.image_normalize(vol, window_min_perc, window_max_perc, output_min, output_max)
    return img.like(out.cpu().numpy().astype(img.array.dtype if img.array.dtype.kind == "f" else np.float32))


def readimage(image_path) -> Image:
    """dask_processing.py:29-43: ``itk.imread(path, itk.F)`` (NIfTI here; see io_nifti.py).  Images pass through unchanged."""
    if isinstance(image_path, (Image, np.ndarray)):
        return as_image(image_path)
    from .io_nifti import read_nifti
    return read_nifti(str(image_path), np.float32)


class Worker:
    """What a Dask task of the reference rebuilds per call, built once per process: the segmenter and the ICON registration engine
    with their weights resident on the GPU.  ``models_dir`` = the reference's ``models/`` directory (or $OAI_DATA_DIR)."""

    def __init__(self, models_dir: Optional[str] = None, icon_weights=None, precision: str = "fp16x3", icon_net_shape=None):
        from .analysis_object import asset_paths, data_dir
        from .registration import ICON_Registration, NET_SHAPE
        from .segmentation.segmenter import Segmenter3DInPatchClassWise
        paths = asset_paths(models_dir or data_dir())
        self.segmenter = Segmenter3DInPatchClassWise(mode="pred", config=dict(      # the literals of dask_processing.py:160-168
            ckpoint_path=paths["ckpoint_path"], training_config_file=paths["training_config_file"], device="cuda",
            batch_size=2, overlap_size=(16, 16, 8), output_prob=True, output_itk=True, precision=precision))
        self.registerer = ICON_Registration(weights=icon_weights if icon_weights is not None else paths["icon_weights"],
                                            net_shape=icon_net_shape or NET_SHAPE, verbose=False)


_WORKER: Optional[Worker] = None


def get_worker(**kwargs) -> Worker:
    """The process's worker (created on first use; pass models_dir= / icon_weights= the first time, or set $OAI_DATA_DIR)."""
    global _WORKER
    if _WORKER is None:
        _WORKER = Worker(**kwargs)
    return _WORKER


def set_worker(worker: Optional[Worker]) -> None:
    global _WORKER
    _WORKER = worker


def segment_method(image_A):
    """dask_processing.py:125-189 without the per-task model download / construction / deletion."""
    test_volume = image_normalize(readimage(image_A), 0.1, 99.9, 0, 1)
    FC_probmap, TC_probmap = get_worker().segmenter.segment(test_volume, if_output_prob_map=True, if_output_itk=True)
    return FC_probmap, TC_probmap


def register_images_delayed(image_A, image_B):
    """dask_processing.py:46-92: (phi_AB, image_A (normalised), image_B)."""
    image_A, image_B = readimage(image_A), readimage(image_B)
    # the reference casts BOTH images to itk.D (:63-73) and windows A in double; here the window (percentiles + rescale) is computed in
    # fp32 on the device and widened: values agree with the double computation to ~1e-7 (tests/test_normalize_gpu.py)
    image_B = image_B.like(image_B.array.astype(np.float64))
    image_A = image_normalize(image_A.like(image_A.array.astype(np.float64)), 0.1, 99.9, 0, 1)
    phi_AB = get_worker().registerer.register(image_A, image_B)
    return phi_AB, image_A, image_B


def deform_probmap_delayed(phi_AB, image_A, image_B, prob, image_type="FC"):
    """dask_processing.py:95-111."""
    from .registration import deform_probmap
    return deform_probmap(phi_AB, image_A, image_B, prob)


def get_thickness(warped_image, mesh_type, split_on_device: bool = False, on_device: bool = False):
    """dask_processing.py:114-122: the inner surface of the cartilage with per-point thickness ("Distance").  The reference converts the
    vtk mesh with mp.get_itk_mesh only "to make it serializable" for Dask's pickling (mesh_processing.py:57-98); there is no task graph
    to pickle for here, so the mesh is returned as mesh_processing produces it.  ``split_on_device``: the inner / outer KMeans split
    on the GPU (mesh_processing.split_mesh).  ``on_device``: the whole step resident on the GPU (mesh_processing.get_thickness_mesh)."""
    from . import mesh_processing as mp
    distance_inner, _ = mp.get_thickness_mesh(warped_image, mesh_type=mesh_type, split_on_device=split_on_device, on_device=on_device)
    return distance_inner


def process_cohort(images: Sequence, atlas_image, worker: Optional[Worker] = None, keep_on_device: bool = False) -> Iterator[Tuple[int, object]]:
    """The driver that replaces the Dask graph of DaskComputation.ipynb for the dense path: every rank of the (optional) process group
    claims volumes from ONE queue and streams them through its GPU with the resident engines: normalise -> segment + register ->
    both probability maps on the atlas grid.  Yields (index, VolumeResult) for the volumes THIS rank processed.
    ``images``: paths or Images (all ranks pass the same list; only claimed entries are read)."""
    from .cohort import CohortRunner
    from .parallel import CalibrationBoard, VolumeQueue, sync_calibration
    from .pipeline import VolumePipeline
    w = worker or get_worker()
    seg = w.segmenter
    if not seg.ready:
        seg.pred_setup()
    eng = seg.model.engine
    if eng.precision != seg.config.get("precision", "fp16x3"):
        eng.set_precision(seg.config.get("precision", "fp16x3"))
    ovl = tuple(int(v) for v in seg.config["overlap_size"])
    if eng.precision == "fp16x3" and len(images):
        # ONE calibration for the cohort: the checkpoint's sidecar if there is one, else rank 0 calibrates on volume 0 (and writes the
        # sidecar); every rank takes rank 0's exponents, so a volume's maps do not depend on which rank the queue hands it to
        eng.set_calibration_file(seg.calibration_file, write=getattr(seg, "calibration_write", False))

        def _calibrate_on_first():
            vol0 = image_normalize(readimage(images[0]), 0.1, 99.9, 0, 1)
            eng.calibrate_volume(torch.from_numpy(np.ascontiguousarray(vol0.array, dtype=np.float32)).to(eng.device),
                                 seg.tile_zyx, ovl[::-1], (ovl[2], ovl[0], ovl[1]))
        sync_calibration(eng, _calibrate_on_first)
    pipe = VolumePipeline(eng, w.registerer.register_module, readimage(atlas_image), tile_zyx=seg.tile_zyx, overlap_zyx=ovl[::-1],
                          crop_zyx=(ovl[2], ovl[0], ovl[1]))
    import torch.distributed as dist
    board = CalibrationBoard() if (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) else None
    runner = CohortRunner(pipe, keep_on_device=keep_on_device, board=board)

    class _Lazy(Sequence):                      # reads + normalises a volume when the runner asks for it (after it was claimed)
        def __len__(self_inner):
            return len(images)

        def __getitem__(self_inner, i):
            # on the runner's copy stream: the upload, the percentile kernels and the blocking .cpu() of image_normalize then wait for
            # earlier copies only, not for the volume whose compute was queued a moment ago (the overlap was lost)
            with torch.cuda.stream(runner.copy_stream):
                return image_normalize(readimage(images[i]), 0.1, 99.9, 0, 1)

    return runner.run(_Lazy(), queue=VolumeQueue(len(images)))


def thickness_stream(results: Iterable[Tuple[int, object]], thickness_atlas, keep_on_device: bool = False,
                     results_complete: bool = False, space: str = "atlas", morphometry=False, mesh_qc: bool = False) -> Iterator[Tuple[int, object]]:
    """(index, KneeThickness) for every (index, VolumeResult) of ``results`` whose ``fc_atlas`` / ``tc_atlas`` are on the device: the
    thickness stage of the reference's task graph (get_thickness x2, then the notebook's map_attributes) behind a cohort, a few hundred
    KB per knee instead of five tensors.

    Each knee's ``ThicknessAtlas.measure`` runs on ONE worker thread with a stream of its own (the library's calls release the GIL, its
    error text is thread-local), so that the stage's small kernels and count read-backs lie underneath the next volume's segmentation and
    never block the thread that queues volumes -- the idea of VolumePipeline._run_overlapped's registration stream.  The worker's stream
    never waits for an event ON THE GPU: a waiting stream parks a barrier packet at the head of an in-order hardware queue and holds
    back whatever shares that queue (cohort.CohortRunner._queue_d2h, profiles/r06_cohort.md).  ``results_complete``: the results are
    already finished on the host's side when they are handed over (CohortRunner(keep_on_device=True) synchronises each volume's event);
    otherwise an event is recorded on the consumer's current stream as each result arrives and the worker waits for it on the host.
    ``space``: "atlas" (default) = the distance on the atlas grid; "patient" = each knee's meshes pushed through its own ``phi`` with its
    ``meta_A`` (ThicknessAtlas.measure(..., phi=, image_A=): the patient's own millimetres); "patient_grid" = native thickness, measured on
    each knee's patient-grid ``fc`` / ``tc`` and carried to the atlas through the inverse of its ``phi`` (ThicknessAtlas.measure(...,
    space="patient_grid")); in both, a result without ``meta_A`` raises ValueError.
    ``morphometry``: True or a coverage distance in mm -- each knee's ``KneeThickness.morphometry`` and ``coverage`` as well
    (ThicknessAtlas.measure(..., morphometry=): area-weighted regional thickness, covered and denuded area).
    ``mesh_qc``: True -- each knee's ``KneeThickness.mesh_qc`` as well (ThicknessAtlas.measure(..., mesh_qc=True): the qc.SplitQuality of
    the mesh and split the thickness was measured on).
    At most two knees are in flight; results come in input order; the worker is gone when the generator is exhausted or closed.
    Measured (profiles/thickness_stage.md section 3): about nine tenths of the stage lie underneath the next volume, unless the runtime
    deals the worker's stream onto the compute stream's own hardware queue (one creation order in four), where it runs serially."""
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    if space not in ("atlas", "patient", "patient_grid"):
        raise ValueError(f"space must be 'atlas', 'patient' or 'patient_grid', got {space!r}")
    dev = thickness_atlas.device
    caller = torch.cuda.current_stream(dev)
    side = []                                                     # the worker's stream, created on the worker

    def job(res, ev):
        with torch.cuda.device(dev):
            if not side:
                side.append(torch.cuda.Stream(device=dev))
            if ev is not None:
                ev.synchronize()                                  # on the host, never a wait queued on the GPU
            with torch.cuda.stream(side[0]):
                res.fc_atlas.record_stream(side[0])
                res.tc_atlas.record_stream(side[0])
                push = {}
                if space != "atlas":
                    if res.meta_A is None:
                        raise ValueError(f"thickness_stream(space='{space}'): a result carries no meta_A (the patient image's geometry)")
                    res.phi.record_stream(side[0])
                    push = dict(phi=res.phi, image_A=res.meta_A)
                if space == "patient_grid":
                    res.fc.record_stream(side[0])
                    res.tc.record_stream(side[0])
                    knee = thickness_atlas.measure(res.fc, res.tc, keep_on_device=keep_on_device, space="patient_grid", morphometry=morphometry,
                                                   mesh_qc=mesh_qc, **push)
                else:
                    knee = thickness_atlas.measure(res.fc_atlas, res.tc_atlas, keep_on_device=keep_on_device, morphometry=morphometry, mesh_qc=mesh_qc, **push)
                if keep_on_device:
                    side[0].synchronize()                         # complete when handed over, like the input
                    knee.fc.record_stream(caller)
                    knee.tc.record_stream(caller)
                    for cov in knee.coverage.values():
                        cov.record_stream(caller)
            return knee

    pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="oai-thickness")
    pending: deque = deque()
    try:
        for index, res in results:
            ev = None
            if not results_complete:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
            pending.append((index, pool.submit(job, res, ev)))
            while len(pending) >= 2:                              # the newest runs while the one before it is handed out
                i, fut = pending.popleft()
                yield i, fut.result()
        while pending:
            i, fut = pending.popleft()
            yield i, fut.result()
    finally:
        pool.shutdown(wait=True, cancel_futures=True)


def qc_stream(results: Iterable[Tuple[int, object]], reference=None) -> Iterator[Tuple[int, object]]:
    """(index, qc.RegistrationQC) for every (index, VolumeResult) of ``results``: the registration QC record of each knee of a cohort
    (folds and det J of its phi, volume scale, cartilage volume; Dice against ``reference``, a qc.QCReference; the image similarity for
    results that carry ``image_net`` when the reference has the atlas image).  The results must be
    complete and on the device, as ``process_cohort(keep_on_device=True)`` hands them over.  A plain synchronous generator: a few small
    launches and one download of a few dozen bytes per knee need no worker thread."""
    from .qc import registration_qc
    for index, res in results:
        yield index, registration_qc(res, reference=reference)


def seg_qc_stream(results: Iterable[Tuple[int, object]], **kwargs) -> Iterator[Tuple[int, object]]:
    """(index, {"FC": qc.SegmentationShape, "TC": ...}) for every (index, VolumeResult) of ``results``: the reference-free shape record
    of each knee's patient-grid maps (qc.result_segmentation_shapes; ``kwargs``: threshold, connectivity, min_voxels, band).  The results
    must be complete and on the device, as for ``qc_stream``; like it a plain synchronous generator, one download per knee."""
    from .qc import result_segmentation_shapes
    for index, res in results:
        yield index, result_segmentation_shapes(res, **kwargs)


def thickness_qc_stream(results: Iterable[Tuple[int, object]], **kwargs) -> Iterator[Tuple[int, object]]:
    """(index, {"FC": qc.LocalThickness, "TC": ...}) for every (index, VolumeResult) of ``results``: the mesh-free local thickness of each
    knee's patient-grid maps (qc.result_local_thicknesses; ``kwargs``: threshold, radius, return_map, max_window_voxels), the figure to
    put beside the mesh-based thickness of a cohort.  The results must be complete and on the device, as for ``qc_stream``; like it a
    plain synchronous generator, one download per knee."""
    from .qc import result_local_thicknesses
    for index, res in results:
        yield index, result_local_thicknesses(res, **kwargs)


def deviation_stream(stream: Iterable[Tuple[int, object]], models, covariates=None, z_threshold: float = 2.0,
                     return_maps: bool = False) -> Iterator[Tuple[int, object]]:
    """(index, {"FC": stats.DeviationResult, "TC": ...}) for every (index, KneeThickness) of ``stream`` (``thickness_stream`` /
    ``process_cohort_thickness``): each knee scored against the normative model of each cartilage in ``models`` ({"FC":
    stats.NormativeModel, ...}) as it arrives.  ``covariates``: what ``covariates[index]`` gives is the knee's covariate row (a mapping or
    a sequence by index; None for models without covariates).  A cartilage that could not be measured has no score anywhere (``n_valid``
    0).  Like ``qc_stream`` a plain synchronous generator: a few small launches and one download per knee and cartilage."""
    from .stats import ThicknessCohort
    for index, knee in stream:
        row = None if covariates is None else covariates[index]
        found = {}
        for kind, model in models.items():
            one = ThicknessCohort(model.atlas, kind, use_coverage=model.surface.use_coverage, chunk=1)
            one.add(knee, index)
            found[kind] = model.deviation(one, covariates=row, z_threshold=z_threshold, return_maps=return_maps)
        yield index, found


def pca_stream(stream: Iterable[Tuple[int, object]], models) -> Iterator[Tuple[int, object]]:
    """(index, {"FC": stats.PCAScores, "TC": ...}) for every (index, KneeThickness) of ``stream`` (``thickness_stream`` /
    ``process_cohort_thickness``): each knee scored against the cohort PCA of each cartilage in ``models`` ({"FC": stats.ThicknessPCA,
    ...}) as it arrives -- its scores, T2 inside the model and the residual Q outside it.  A cartilage that could not be measured lies on
    the mean everywhere (``n_missing`` = the model's vertices, q = 0).  Like ``deviation_stream`` a plain synchronous generator: two small
    launches and one download per knee and cartilage."""
    from .stats import ThicknessCohort
    for index, knee in stream:
        found = {}
        for kind, model in models.items():
            one = ThicknessCohort(model.atlas, kind, use_coverage=model.surface.use_coverage, chunk=1)
            one.add(knee, index)
            found[kind] = model.transform(one)
        yield index, found


def process_cohort_thickness(images: Sequence, atlas_image, thickness_atlas, worker: Optional[Worker] = None,
                             space: str = "atlas", morphometry=False, mesh_qc: bool = False) -> Iterator[Tuple[int, object]]:
    """process_cohort with the thickness stage behind it: yields (index, KneeThickness) for the volumes this rank processed; the
    probability maps never leave the device.  ``space``: see thickness_stream ("patient": every knee through its own phi; "patient_grid":
    native thickness on every knee's own grid); ``morphometry``, ``mesh_qc``: see there."""
    return thickness_stream(process_cohort(images, atlas_image, worker, keep_on_device=True), thickness_atlas, results_complete=True, space=space,
                            morphometry=morphometry, mesh_qc=mesh_qc)
