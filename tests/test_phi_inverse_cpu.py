"""CPU: the numpy restatement of the inverse of phi (tests/phi_inverse_ref.py) against an analytic stretch and its own round trip, the
inverse affine pair of mesh_processing.mesh_point_affines, and the argument checks of oai_inverse_points_through_phi and oai_invert_phi
(which touch no GPU)."""
import numpy as np
import pytest

import mesh_transform_ref as mref
import phi_inverse_ref as ref
from oai_analysis_2_amd.image import Image
from oai_analysis_2_amd.mesh_processing import mesh_point_affines

# net, amplitude (x, y, z) in voxels, bound L on the row sums of |grad u| at the cell centres (the figures the GPU tests' bounds use)
FIELDS = [((3, 4, 5), (0.3, 0.25, 0.2), 0.24), ((6, 7, 9), (0.4, 0.35, 0.3), 0.28), ((12, 16, 20), (0.9, 0.8, 0.6), 0.33),
          ((8, 16, 64), (3.0, 0.8, 0.4), 1.29)]


def _meta(shape_zyx, spacing, origin=(0.0, 0.0, 0.0), direction=None):
    return Image(np.broadcast_to(np.zeros((), np.float32), shape_zyx), spacing, origin, np.eye(3) if direction is None else direction)


def _rotated_flipped():
    k = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K) @ np.diag([1.0, -1.0, 1.0])


def _stretch_phi(net, factor):
    phi = mref.identity_phi(net)
    phi[2] = (0.5 + factor * (phi[2].copy() - 0.5)).astype(np.float32)
    return phi


def test_reference_inverts_the_analytic_stretch_where_the_fixed_point_diverges():
    """x stretched 2.5 times about the centre: T(x) = 31.5 + 2.5 (x - 31.5) inside the buffer.  Newton lands on 31.5 + (y - 31.5) / 2.5;
    the plain fixed point x <- y - u(x) multiplies its error by 1.5 per step.  Bound 1e-4: that of the forward analytic test (float32
    epsilon x coordinate x the roundings of the displacement rebuild)."""
    net = (8, 16, 64)
    phi = _stretch_phi(net, 2.5)
    y = np.random.default_rng(0).uniform([-0.4, -0.4, -0.4], [63.4, 15.4, 7.4], size=(2000, 3))
    x, status, iters, resid = ref.solve_ref(phi, y)
    err = np.abs(x[:, 0] - (31.5 + (y[:, 0] - 31.5) / 2.5)).max()
    print("newton iterations max", int(iters.max()), "max error", float(err))
    assert (status == 1).all() and iters.max() <= 5 and resid.max() <= 1e-7
    assert err <= 1e-4 and np.array_equal(x[:, 1:], y[:, 1:])
    disp = mref.displacement(phi)
    xf = y.copy()
    for _ in range(30):                                                # the fixed point, on the points that start off the centre
        xf = y - ref._trilinear_clamped(disp, xf[:, 0], xf[:, 1], xf[:, 2])
    off = np.abs(y[:, 0] - 31.5) > 1.0
    assert (np.abs(ref.forward_net(phi, xf)[off] - y[off]).max(axis=1) > 1.0).all()


@pytest.mark.parametrize("net,amp,L", FIELDS)
def test_reference_round_trip_on_the_smooth_fields(net, amp, L):
    phi = ref.smooth_phi(net, amp)
    disp = mref.displacement(phi)
    assert not disp[[0, -1]].any() and not disp[:, [0, -1]].any() and not disp[:, :, [0, -1]].any()      # zero on the boundary lattice
    got_L = ref.gradient_row_sum(phi)
    print(net, "row sum of |grad u|", got_L)
    assert got_L <= L and (L < 1.0 or got_L > 1.0)                     # (the last field stretches by more than 2 somewhere)
    eye = (np.eye(3), np.zeros(3))
    size = np.array(net[::-1], np.float64)
    pts = np.random.default_rng(5).uniform(-0.5 - 0.0386 * size, size - 0.5 + 0.0386 * size, size=(5000, 3)).astype(np.float32)
    for y in (ref.lattice(net), pts.astype(np.float64)):
        x, status, iters, resid = ref.solve_ref(phi, y)
        assert (status != 0).all() and iters.max() <= 9 and resid.max() <= 1e-7
        assert np.array_equal(status == 2, ~mref.inside_buffer(x, net))
        assert np.abs(ref.forward_net(phi, x) - y).max() <= 1e-7
    out, status, _, _, x = ref.inverse_points_ref(pts, phi, eye, eye)
    back, inside, _ = mref.transform_points_ref(out.astype(np.float32), phi, eye, eye)      # the forward restatement, on the rounded points
    assert np.abs(back - pts).max() <= 4 * 2.0 ** -24 * max(net) + 2e-7 * (1 + L)
    psi, st, stats = ref.invert_phi_ref(phi)
    assert stats[:3] == (int(np.prod(net)), 0, 0) and st.all() and psi.dtype == np.float32 and psi.shape == phi.shape


def test_gradient_is_the_derivative_of_the_interpolant():
    net = (6, 7, 9)
    disp = mref.displacement(mref.random_phi(net, np.random.default_rng(2), 0.05))
    x = np.random.default_rng(3).uniform(0.1, 0.9, size=(200, 3)) + np.random.default_rng(4).integers(0, [8, 6, 5], size=(200, 3))
    d, G = ref.disp_and_gradient(disp, x)
    h = 1e-6
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        num = (ref.disp_and_gradient(disp, x + e)[0] - ref.disp_and_gradient(disp, x - e)[0]) / (2 * h)
        assert np.abs(num - G[:, :, k]).max() <= 1e-8
    low = np.array([[-0.3, 2.2, 1.5], [3.3, -0.2, 1.5], [3.3, 2.2, -0.4], [8.2, 2.2, 1.5], [3.3, 6.3, 1.5], [3.3, 2.2, 5.25]])
    G = ref.disp_and_gradient(disp, low)[1]
    for i, k in enumerate((0, 1, 2, 0, 1, 2)):                         # a clamped axis: a zero column
        assert not G[i, :, k].any() and G[i].any()


def test_inverse_affine_pair_undoes_mesh_point_affines():
    net = (5, 7, 9)
    A = _meta((11, 13, 17), [0.36, 0.37, 0.7], [10.0, -20.0, 5.0], _rotated_flipped())
    B = _meta((8, 12, 10), [0.4, 0.35, 0.75], [0.0, -1.0, 2.0], _rotated_flipped().T)
    pts = np.random.default_rng(1).uniform(-5, 15, size=(200, 3))
    for ca in mref.COORDS:                                             # the coordinates on A's side
        for cb in mref.COORDS:                                         # ... and on B's
            p2n, n2o = mesh_point_affines(A, B, net, cb, ca)
            q2n, n2q = mesh_point_affines(A, B, net, ca, cb, inverse=True)
            x = mref.apply_affine(p2n, pts)
            assert np.abs(mref.apply_affine(n2q, x) - pts).max() < 1e-12                       # net -> B undoes B -> net
            assert np.abs(mref.apply_affine(q2n, mref.apply_affine(n2o, x)) - x).max() < 1e-12    # A -> net undoes net -> A
            for got, want in ((q2n, ref.inverse_affine(n2o)), (n2q, ref.inverse_affine(p2n))):
                assert np.abs(got[0] - want[0]).max() < 1e-12 and np.abs(got[1] - want[1]).max() < 1e-12
    with pytest.raises(ValueError, match="coords"):
        mesh_point_affines(A, B, net, coords_in="voxel", inverse=True)
    fwd = mesh_point_affines(A, B, net)
    same = mesh_point_affines(A, B, net, inverse=False)
    assert all(np.array_equal(a, b) for f, s in zip(fwd, same) for a, b in zip(f, s))


def test_entry_points_check_their_arguments_before_touching_a_gpu():
    import ctypes as C
    from oai_analysis_2_amd import _lib
    lib = _lib.load()
    aff = _lib.Affine()
    dummy = (C.c_float * 24)()
    a = C.byref(aff)
    pts = lib.oai_inverse_points_through_phi
    assert pts(None, 0, None, 2, 2, 2, None, None, 30, 1e-7, None, None, None) == 0                           # n = 0: a no-op
    assert pts(None, 4, None, 2, 2, 2, None, None, 30, 1e-7, None, None, None) != 0 and b"null" in lib.oai_last_error()
    assert pts(dummy, 1, dummy, 1, 2, 2, a, a, 30, 1e-7, dummy, None, None) != 0 and b"at least 2" in lib.oai_last_error()
    assert pts(dummy, 0, dummy, 2, 2, 1, a, a, 30, 1e-7, dummy, None, None) != 0                              # ... even for n = 0
    assert pts(dummy, -1, dummy, 2, 2, 2, a, a, 30, 1e-7, dummy, None, None) != 0
    assert pts(dummy, 1, dummy, 2, 2, 2, a, a, 0, 1e-7, dummy, None, None) != 0 and b"max_iter" in lib.oai_last_error()
    assert pts(dummy, 1, dummy, 2, 2, 2, a, a, 30, 0.0, dummy, None, None) != 0 and b"tol" in lib.oai_last_error()
    assert pts(dummy, 1, dummy, 2, 2, 2, a, a, 30, float("nan"), dummy, None, None) != 0
    dense, need = lib.oai_invert_phi, lib.oai_invert_phi_workspace_bytes
    assert need(1, 4, 4) == 0 and need(2, 2, 2) > 0 and need(80, 192, 192) >= 5 * 8 * (80 * 192 * 192 // 256)
    other = (C.c_float * 24)()
    stats = (C.c_double * 6)()
    assert dense(dummy, 2, 2, 1, 30, 1e-7, other, None, dummy, 1 << 20, stats, None) != 0 and b"at least 2" in lib.oai_last_error()
    assert dense(dummy, 2, 2, 2, 0, 1e-7, other, None, dummy, 1 << 20, stats, None) != 0 and b"max_iter" in lib.oai_last_error()
    assert dense(dummy, 2, 2, 2, 30, -1.0, other, None, dummy, 1 << 20, stats, None) != 0 and b"tol" in lib.oai_last_error()
    assert dense(None, 2, 2, 2, 30, 1e-7, other, None, dummy, 1 << 20, stats, None) != 0 and b"null" in lib.oai_last_error()
    assert dense(dummy, 2, 2, 2, 30, 1e-7, dummy, None, other, 1 << 20, stats, None) != 0 and b"alias" in lib.oai_last_error()
    assert dense(dummy, 2, 2, 2, 30, 1e-7, other, None, dummy, 8, stats, None) != 0 and b"workspace" in lib.oai_last_error()
