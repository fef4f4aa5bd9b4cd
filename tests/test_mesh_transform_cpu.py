"""CPU: mesh_processing.mesh_point_affines -- the two affine legs around phi for mesh points -- against the exact cases and against the
leg-by-leg chain of tests/mesh_transform_ref.py, and the argument checks of oai_transform_points_through_phi (which touch no GPU)."""
import numpy as np
import pytest

import mesh_transform_ref as ref
from oai_analysis_2_amd.image import Image
from oai_analysis_2_amd.mesh_processing import mesh_point_affines
from oai_analysis_2_amd.registration import resample_affines


def _meta(shape_zyx, spacing, origin=(0.0, 0.0, 0.0), direction=None):
    return Image(np.broadcast_to(np.zeros((), np.float32), shape_zyx), spacing, origin, np.eye(3) if direction is None else direction)


def _rotated_flipped():
    """A rotation about a skew axis (Rodrigues) with the y axis flipped: det = -1."""
    k = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    d = R @ np.diag([1.0, -1.0, 1.0])
    assert np.linalg.det(d) < 0 and np.allclose(d @ d.T, np.eye(3), atol=1e-15)
    return d


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (2.0, 2.0, 2.0), (2.0, 1.0, 0.5)])
def test_exact_geometry_gives_exactly_the_diagonal_pair(spacing):
    """Identity directions, power-of-two spacings, net shape = image size: every product and sum of the composition is exact."""
    shape = (6, 10, 12)
    A = _meta(shape, [2 * s for s in spacing], [1.0, -2.5, 3.0])
    B = _meta(shape, spacing, [-4.0, 0.5, 8.0])
    (A1, b1), (A2, b2) = resample_affines(A, B, shape)
    assert np.array_equal(A1, np.eye(3)) and np.array_equal(b1, np.zeros(3)) and np.array_equal(A2, np.eye(3)) and np.array_equal(b2, np.zeros(3))
    (P, p), (Q, q) = mesh_point_affines(A, B, shape)
    assert np.array_equal(P, np.diag(1.0 / B.spacing)) and np.array_equal(p, np.zeros(3))
    assert np.array_equal(Q, np.diag(A.spacing)) and np.array_equal(q, np.zeros(3))
    (P, p), (Q, q) = mesh_point_affines(B, B, shape)                     # the same image on either side: the round trip is the identity, exactly
    pts = np.random.default_rng(0).uniform(-3, 20, size=(50, 3)).astype(np.float32).astype(np.float64)
    assert np.array_equal(ref.apply_affine((Q, q), ref.apply_affine((P, p), pts)), pts)


def test_rotated_flipped_geometry_with_zero_displacement_is_physical_A_of_the_network_point():
    net = (5, 7, 9)
    d = _rotated_flipped()
    A = _meta((11, 13, 17), [0.36, 0.37, 0.7], [10.0, -20.0, 5.0], d)
    B = _meta((8, 12, 10), [0.4, 0.35, 0.75], [0.0, -1.0, 2.0], _rotated_flipped().T)
    rng = np.random.default_rng(1)
    idx = rng.uniform(-2, 14, size=(200, 3))                             # B continuous indices, some outside the grid
    for cin in ref.COORDS:
        pts = ref._from_index(idx, B, cin)
        p2n, n2o = mesh_point_affines(A, B, net, cin, "physical")
        x = ref.apply_affine(p2n, pts)
        want, x_ref, _ = ref.point_chain_ref(pts, None, net, A, B, cin, "physical")
        assert np.abs(x - x_ref).max() < 1e-12
        got = ref.apply_affine(n2o, x)
        assert np.abs(got - ref.net_to_physical(x, A, net)).max() < 1e-12        # physical_A of the same network point
        assert np.abs(got - want).max() < 1e-12                                  # ... and the whole chain, leg by leg
        for cout in ref.COORDS:
            got = ref.apply_affine(mesh_point_affines(A, B, net, cin, cout)[1], x)
            assert np.abs(got - ref.point_chain_ref(pts, None, net, A, B, cin, cout)[0]).max() < 1e-12


def test_physical_and_spacing_forms_agree_through_index_to_physical_affine():
    net = (4, 6, 5)
    A = _meta((9, 8, 7), [0.5, 0.8, 1.1], [3.0, 2.0, -1.0], _rotated_flipped())
    B = _meta((6, 7, 8), [0.9, 0.6, 1.3], [-5.0, 4.0, 0.25], _rotated_flipped().T)
    idx = np.random.default_rng(2).uniform(-1, 9, size=(100, 3))
    P_B, o_B = B.index_to_physical_affine()
    P_A, o_A = A.index_to_physical_affine()
    sp_in, ph_in = mesh_point_affines(A, B, net, "spacing", "spacing")[0], mesh_point_affines(A, B, net, "physical", "spacing")[0]
    x = ref.apply_affine(sp_in, idx * B.spacing)
    assert np.abs(x - ref.apply_affine(ph_in, idx @ P_B.T + o_B)).max() < 1e-12        # the same index, spelled both ways
    sp_out, ph_out = mesh_point_affines(A, B, net, "spacing", "spacing")[1], mesh_point_affines(A, B, net, "spacing", "physical")[1]
    ia = ref.apply_affine(sp_out, x) / A.spacing                                      # A continuous index
    assert np.abs(ref.apply_affine(ph_out, x) - (ia @ P_A.T + o_A)).max() < 1e-12
    b2n, n2a = resample_affines(A, B, net)                                            # ... and both legs are the resample's, around the index
    assert np.abs(x - ref.apply_affine(b2n, idx)).max() < 1e-12 and np.abs(ia - ref.apply_affine(n2a, x)).max() < 1e-12


def test_unknown_coordinates_are_refused():
    img = _meta((4, 4, 4), [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="coords"):
        mesh_point_affines(img, img, (4, 4, 4), coords_in="voxel")
    with pytest.raises(ValueError, match="coords"):
        mesh_point_affines(img, img, (4, 4, 4), coords_out="index")


def test_entry_point_checks_its_arguments_before_touching_a_gpu():
    import ctypes as C
    from oai_analysis_2_amd import _lib
    lib = _lib.load()
    aff = _lib.Affine()
    dummy = (C.c_float * 8)()
    assert lib.oai_transform_points_through_phi(None, 0, None, 2, 2, 2, None, None, None, None, None) == 0              # n = 0: a no-op
    assert lib.oai_transform_points_through_phi(None, 4, None, 2, 2, 2, None, None, None, None, None) != 0 and b"null" in lib.oai_last_error()
    assert lib.oai_transform_points_through_phi(dummy, 1, dummy, 1, 2, 2, C.byref(aff), C.byref(aff), dummy, None, None) != 0
    assert b"at least 2" in lib.oai_last_error()
    assert lib.oai_transform_points_through_phi(dummy, 0, dummy, 2, 2, 1, C.byref(aff), C.byref(aff), dummy, None, None) != 0     # ... even for n = 0
    assert lib.oai_transform_points_through_phi(dummy, -1, dummy, 2, 2, 2, C.byref(aff), C.byref(aff), dummy, None, None) != 0
