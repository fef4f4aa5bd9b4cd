"""The reference's test_get_mesh (test/test_mesh_processing.py:12-22) the day the assets are supplied: the cuberille mesh of
``colab_case/TC_probmap.nii.gz`` against the baseline ``TC_mesh.vtk``.  Both are pooch downloads (oai_analysis/data.py:8-22) and there
is no network here, so the test SKIPS WITH A REASON unless ``OAI_DATA_DIR`` holds the extracted ``test_data/`` tarball.

The comparison is order-free on purpose: the reference compares vertex arrays row by row (atol 0.02), but the vertex order of ITK's
cuberille output cannot be confirmed offline, so this asserts the same vertex count and that every vertex lies within 0.02 of its
nearest baseline vertex and the other way round.  If it fails, try move_after_converged=False first, then the other recalled points
of DESIGN.md 1."""
import os

import numpy as np
import pytest

ROOT = os.environ.get("OAI_DATA_DIR", "")


def _files():
    from oai_analysis_2_amd.analysis_object import asset_paths
    case = asset_paths(ROOT)["test_case"]
    return os.path.join(case, "TC_probmap.nii.gz"), os.path.join(case, "TC_mesh.vtk")


def _missing():
    if not ROOT:
        return ["$OAI_DATA_DIR is not set"]
    return [f for f in _files() if not os.path.exists(f)]


pytestmark = pytest.mark.gpu


@pytest.mark.skipif(bool(_missing()), reason="real OAI assets absent (pooch downloads of oai_analysis/data.py:8-22, no network in this "
                                             "environment): set OAI_DATA_DIR to the extracted v2.0.0 tarballs; missing: %s" % _missing())
def test_get_mesh_matches_the_baseline_vtk():
    from scipy.spatial import cKDTree
    from oai_analysis_2_amd import meshread
    from oai_analysis_2_amd.io_nifti import read_nifti
    from oai_analysis_2_amd.mesh_processing import get_mesh_from_probability_map
    prob, base = _files()
    mesh = get_mesh_from_probability_map(read_nifti(prob))
    baseline = meshread(base)
    got, want = mesh.verts.astype(np.float64), np.asarray(baseline.verts, np.float64)
    d_gb = cKDTree(want).query(got)[0]
    d_bg = cKDTree(got).query(want)[0]
    print(f"[TC cuberille] {len(got)} verts vs {len(want)} baseline; max nearest distance {d_gb.max():.4f} / {d_bg.max():.4f}")
    assert len(got) == len(want)
    assert d_gb.max() <= 0.02 and d_bg.max() <= 0.02
