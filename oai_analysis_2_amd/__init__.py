"""MI355X-native (gfx950) implementation of OAI_analysis_2's per-volume dense path.

Public surface mirrors the reference: ``AnalysisObject`` (analysis_object.py), ``segmentation.segmenter.
Segmenter3DInPatchClassWise``, ``registration.ICON_Registration``.  All compute runs in hand-written HIP
kernels behind the C ABI of ``liboai_hip.so`` (include/oai_hip.h); there is no CPU fallback.
"""
__version__ = "0.1.0"


def imread(path, dtype="float32"):
    """``itk.imread(path, itk.F)`` without ITK: NIfTI-1 (.nii / .nii.gz) -> ``image.Image`` in ITK's LPS conventions."""
    import numpy as _np
    from .io_nifti import read_nifti
    return read_nifti(path, _np.dtype(dtype) if dtype is not None else None)


def imwrite(image, path):
    """``itk.imwrite(image, path)`` without ITK (NIfTI-1; gzip when the name ends in .gz)."""
    from .image import as_image
    from .io_nifti import write_nifti
    write_nifti(path, as_image(image))


def meshread(path):
    """``itk.meshread(path)`` without ITK: a legacy VTK POLYDATA file (ASCII or BINARY) -> ``mesh_processing.Mesh``."""
    from .io_vtk import read_vtk
    return read_vtk(path)


def meshwrite(mesh, path, binary=False):
    """``itk.meshwrite(mesh, path)`` without ITK: legacy VTK POLYDATA, ASCII unless ``binary``."""
    from .io_vtk import write_vtk
    write_vtk(mesh, path, binary=binary)


def __getattr__(name):
    """``ThicknessAtlas`` / ``KneeThickness`` (thickness.py) and the cohort statistics (stats.py), imported on first use: the package itself
    imports neither torch nor the library."""
    if name in ("ThicknessAtlas", "KneeThickness"):
        from . import thickness
        return getattr(thickness, name)
    if name in ("ThicknessCohort", "PermutationResult", "two_sample_test", "paired_test", "label_permutations", "sign_flips",
                "RegressionResult", "IndexPermutations", "regression_test", "index_permutations", "FResult", "f_test", "anova_test",
                "LongitudinalCohort", "visit_table", "one_sample_test", "VisitSlopes",
                "BootstrapCounts", "BootstrapResult", "bootstrap_counts", "bootstrap_ci",
                "Ranking", "RankSumResult", "SignedRankResult", "KruskalResult", "SpearmanResult", "rank_sum_test", "signed_rank_test",
                "kruskal_test", "spearman_test", "ThicknessPCA", "PCAScores", "MarginalResult", "marginal_test"):
        from . import stats
        return getattr(stats, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
