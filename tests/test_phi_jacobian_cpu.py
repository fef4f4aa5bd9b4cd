"""CPU: the fp64 restatement of the Jacobian determinant of phi (tests/phi_jacobian_ref.py) against analytic cases and against the
independent ``flips`` form, and the argument checks of oai_phi_jacobian / oai_mask_overlap (which touch no GPU)."""
import ctypes as C

import numpy as np
import pytest

import phi_jacobian_ref as pj


@pytest.mark.parametrize("shape", [(6, 7, 9), (80, 192, 192)])
def test_identity_reads_exactly_one(shape):
    """The displacement of the identity map is exactly zero, so every determinant is exactly 1.0 (the raw-phi form is not: float32
    identity coordinates are not equidistant)."""
    det = pj.det_ref(pj.drawn_phi(shape, 0))
    assert det.shape == tuple(n - 1 for n in shape)
    assert det.min() == 1.0 and det.max() == 1.0
    if shape == (80, 192, 192):
        raw = pj.flips_form(pj.drawn_phi(shape, 0))
        print("raw-phi form of the identity map at", shape, "reads", float(raw.min()), "..", float(raw.max()))
        assert raw.min() < 1.0 < raw.max()


def test_axis_aligned_stretch():
    """1.25 * 0.8 * 1.1 about the centre: det = 1.1 within phi_jacobian_ref.stretch_tolerance (float32 epsilon x the rebuild's magnitude)."""
    shape = (8, 16, 64)
    det = pj.det_ref(pj.stretch_phi(shape))
    tol = pj.stretch_tolerance(shape)
    print("det in", float(det.min()), "..", float(det.max()), "tolerance", tol)
    assert tol < 1e-4
    assert np.abs(det - 1.1).max() <= tol


@pytest.mark.parametrize("shape,amp", [((3, 4, 5), 0.8), ((6, 7, 9), 0.45), ((6, 7, 9), 0.8), ((9, 33, 70), 0.45)])
def test_fold_count_equals_the_flips_form(shape, amp):
    """Two definitions of a fold -- the displacement form in fp64, ICON's raw-phi cross product in fp32 -- count the same cells.  The
    comparison means something only where no determinant is within the two forms' disagreement of zero: asserted, ten times over, at
    the largest case."""
    phi = pj.drawn_phi(shape, amp)
    det, raw = pj.det_ref(phi), pj.flips_form(phi)
    disagreement, smallest = float(np.abs(det - raw).max()), float(np.abs(det).min())
    print(shape, amp, "folds", int((det < 0).sum()), "of", det.size, "flips form", int((raw < 0).sum()), "smallest |det|", smallest,
          "largest disagreement", disagreement)
    assert smallest >= (10 if shape == (9, 33, 70) else 1) * disagreement
    assert 0 < int((det < 0).sum()) < det.size
    assert np.array_equal(det < 0, raw < 0)
    assert pj.stats_ref(det)["folds"] == int((raw < 0).sum())


def test_a_planted_nan_and_inf_are_counted_apart():
    phi = pj.drawn_phi((6, 7, 9), 0.45)
    phi[0, 2, 3, 4], phi[2, 4, 2, 6] = np.nan, np.inf
    det = pj.det_ref(phi)
    s = pj.stats_ref(det)
    assert s["nonfinite"] == 8 and s["n_finite"] == det.size - 8         # each voxel sits in its own cell and in the three behind it
    assert np.isfinite([s["min"], s["max"], s["sum"], s["sum_sq"]]).all()


def test_argument_checks_of_the_qc_entry_points():
    """Bad arguments come back as a non-zero status with a message -- no GPU is touched before the checks."""
    from oai_analysis_2_amd import _lib
    lib = _lib.load()
    dummy = (C.c_float * 8)()
    assert lib.oai_phi_jacobian(None, 8, 8, 8, None, None, 0, None, None) != 0 and b"null" in lib.oai_last_error()
    assert lib.oai_phi_jacobian(dummy, 8, 8, 8, None, dummy, 1 << 20, None, None) != 0 and b"null" in lib.oai_last_error()
    for dims in ((1, 8, 8), (8, 1, 8), (8, 8, 1)):
        assert lib.oai_phi_jacobian(dummy, *dims, None, dummy, 1 << 20, dummy, None) != 0 and b"at least 2" in lib.oai_last_error()
        assert lib.oai_phi_jacobian_workspace_bytes(*dims) == 0
    need = lib.oai_phi_jacobian_workspace_bytes(8, 8, 8)
    assert need > 0 and lib.oai_phi_jacobian_workspace_bytes(80, 192, 192) > need
    assert lib.oai_phi_jacobian(dummy, 8, 8, 8, None, dummy, need - 1, dummy, None) != 0
    assert b"oai_phi_jacobian: workspace" in lib.oai_last_error()
    assert lib.oai_mask_overlap(dummy, None, 8, 0.5, dummy, 1 << 20, None, None) != 0 and b"null" in lib.oai_last_error()
    assert lib.oai_mask_overlap(None, None, 8, 0.5, dummy, 1 << 20, dummy, None) != 0 and b"null" in lib.oai_last_error()
    assert lib.oai_mask_overlap(dummy, None, -1, 0.5, dummy, 1 << 20, dummy, None) != 0 and b"negative" in lib.oai_last_error()
    need = lib.oai_mask_overlap_workspace_bytes(8)
    assert need > 0 and lib.oai_mask_overlap_workspace_bytes(0) == 0
    assert lib.oai_mask_overlap_workspace_bytes(384 * 384 * 160) == lib.oai_mask_overlap_workspace_bytes(1 << 40)      # the grid is capped
    assert lib.oai_mask_overlap(dummy, dummy, 8, 0.5, dummy, need - 1, dummy, None) != 0
    assert b"oai_mask_overlap: workspace" in lib.oai_last_error()
