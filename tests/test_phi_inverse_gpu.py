"""GPU: the inverse of phi (csrc/phi_inverse.hip: ops.inverse_points_through_phi, ops.invert_phi, DisplacementTransform.inverse,
mesh_processing.transform_mesh(inverse=True), ThicknessAtlas.measure(space="patient_grid")) against the fp64 restatement of
tests/phi_inverse_ref.py, round trips through the existing forward push, an analytic stretch, a folded field and the argument errors.

The smooth fields and their gradient bounds L are those of tests/test_phi_inverse_cpu.py (FIELDS), where the reference alone is shown to
converge on them.  tol is the default, 1e-7 network voxels."""
import threading

import numpy as np
import pytest
import torch

import mesh_transform_ref as mref
import phi_inverse_ref as ref
from oai_analysis_2_amd import _lib, ops
from oai_analysis_2_amd import mesh_processing as mp
from oai_analysis_2_amd.image import Image
from oai_analysis_2_amd.registration import DisplacementTransform, deform_probmap

pytestmark = pytest.mark.gpu

TOL = 1e-7
FIELDS = {(3, 4, 5): ((0.3, 0.25, 0.2), 0.24), (6, 7, 9): ((0.4, 0.35, 0.3), 0.28), (12, 16, 20): ((0.9, 0.8, 0.6), 0.33)}
NETS = sorted(FIELDS)
EYE = (np.eye(3), np.zeros(3))


def _meta(shape_zyx, spacing, origin=(0.0, 0.0, 0.0), direction=None):
    return Image(np.broadcast_to(np.zeros((), np.float32), shape_zyx), spacing, origin, np.eye(3) if direction is None else direction)


def _rotated_flipped():
    """tests/test_mesh_transform_gpu.py::_rotated_flipped: a rotation about a skew axis with the y axis flipped, det = -1."""
    k = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K) @ np.diag([1.0, -1.0, 1.0])


def _geometries():
    """tests/test_mesh_transform_gpu.py's pair: A the patient's side, B the atlas'."""
    return (_meta((11, 13, 17), [0.36, 0.37, 0.7], [10.0, -20.0, 5.0], _rotated_flipped()),
            _meta((8, 12, 10), [0.4, 0.35, 0.75], [0.0, -1.0, 2.0], _rotated_flipped().T))


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


def _draw_points(rng, n, net, p2n):
    """tests/test_mesh_transform_gpu.py::_draw_points: n float32 points whose network coordinates are uniform over the buffer widened by
    3.9 % per side, none within 1e-3 voxels of a face of the buffer."""
    Dn, Hn, Wn = net
    size = np.array([Wn, Hn, Dn], np.float64)
    x = rng.uniform(-0.5 - 0.0386 * size, size - 0.5 + 0.0386 * size, size=(n, 3))
    for face in (np.full(3, -0.5), size - 0.5):
        d = x - face
        x = np.where(np.abs(d) < 1e-3, face + np.where(d < 0, -1e-3, 1e-3), x)
    A, b = p2n
    return ((x - b) @ np.linalg.inv(A).T).astype(np.float32)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _round_trip_voxels(net, L):
    """One float32 rounding of the solved point, amplified by at most 1 + L, plus one rounding of the result; the solver's tolerance,
    amplified by at most 1 + L, twice."""
    return 4 * 2.0 ** -24 * max(net) + 2 * TOL * (1 + L)


@pytest.fixture(scope="module")
def smooth():
    """Per net: the smooth phi (host and device) and the reference's dense inverse of it, computed once and left unchanged."""
    out = {}
    for net in NETS:
        phi = ref.smooth_phi(net, FIELDS[net][0])
        x, status, iters, resid = ref.solve_ref(phi, ref.lattice(net))
        out[net] = dict(phi=phi, phi_d=_cuda(phi), x=x, status=status, iters=iters, resid=resid)
    return out


# ---- 1. points, smooth fields -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS)
def test_points_against_the_fp64_restatement_and_round_trip(net, smooth):
    rng = np.random.default_rng(200 + net[2])
    phi, phi_d, L = smooth[net]["phi"], smooth[net]["phi_d"], FIELDS[net][1]
    A, B = _geometries()
    n_out = n_all = 0
    for ca, cb in (("physical", "physical"), ("spacing", "spacing")):          # the coordinates on A's side and on B's
        q2n, n2q = mp.mesh_point_affines(A, B, net, ca, cb, inverse=True)
        p2n, n2o = mp.mesh_point_affines(A, B, net, cb, ca)
        for n in (0, 1, 63, 64, 65, 1000):
            pts = _draw_points(rng, n, net, q2n)
            want, status, iters, y, x = ref.inverse_points_ref(pts, phi, q2n, n2q)
            assert (status != 0).all()                                          # the condition of this test: the reference converges everywhere
            got, got_st = ops.inverse_points_through_phi(_cuda(pts), phi_d, q2n, n2q, return_status=True)
            assert got.shape == (n, 3) and got.dtype == torch.float32 and got_st.shape == (n,) and got_st.dtype == torch.uint8
            back = ops.transform_points_through_phi(got, phi_d, p2n, n2o).cpu().numpy()
            alone = ops.inverse_points_through_phi(_cuda(pts), phi_d, q2n, n2q)
            got, got_st = got.cpu().numpy(), got_st.cpu().numpy()
            assert np.array_equal(got_st, status)                               # the status bytes: exactly
            assert np.array_equal(_bits(alone), _bits(got))                     # without the status output: the same points
            w32 = want.astype(np.float32)
            err = np.abs(got.astype(np.float64) - w32.astype(np.float64))
            allowed = np.abs(np.spacing(w32)).astype(np.float64) + (np.abs(n2q[0]).sum(axis=1) * 4 * TOL)[None, :]
            rt = np.abs(back.astype(np.float64) - pts.astype(np.float64))
            rt_allowed = np.abs(n2o[0]).sum(axis=1) * _round_trip_voxels(net, L)
            if n:
                print(net, ca, "n", n, "outside", int((status == 2).sum()), "iterations max", int(iters.max()), "not bitwise", int((_bits(got) != _bits(w32)).sum()),
                      "max error / allowed", float((err / allowed).max()), "round trip / allowed", float((rt / rt_allowed[None, :]).max()))
            assert (err <= allowed).all()
            assert (rt <= rt_allowed[None, :]).all()
            n_out, n_all = n_out + int((status == 2).sum()), n_all + n
    assert 0.1 < n_out / n_all < 0.3                                            # about a fifth converged outside the buffer


# ---- 2. stretch ---------------------------------------------------------------------------------------------------------------------------
def test_analytic_stretch_along_x():
    """phi stretches x by 2.5 about the centre (the plain fixed point diverges): every y inside the buffer comes back as
    31.5 + (y - 31.5) / 2.5.  Bound 1e-4: float32 epsilon x coordinate x the roundings of the fp32 displacement rebuild, as in
    tests/test_mesh_transform_gpu.py::test_analytic_stretch_along_x; the numpy restatement shows 1.8e-6."""
    net = (8, 16, 64)
    phi = mref.identity_phi(net)
    phi[2] = (0.5 + 2.5 * (phi[2].copy() - 0.5)).astype(np.float32)
    y = np.random.default_rng(0).uniform([-0.4, -0.4, -0.4], [63.4, 15.4, 7.4], size=(2000, 3)).astype(np.float32)
    got, status = ops.inverse_points_through_phi(_cuda(y), _cuda(phi), EYE, EYE, return_status=True)
    got, status = got.cpu().numpy().astype(np.float64), status.cpu().numpy()
    err = np.abs(got[:, 0] - (31.5 + (y[:, 0].astype(np.float64) - 31.5) / 2.5)).max()
    _, stats = ops.invert_phi(_cuda(phi))
    print("max error", float(err), "dense: iterations max", stats.max_iterations, "mean", stats.mean_iterations, "unconverged", stats.unconverged)
    assert (status == 1).all() and stats.unconverged == 0
    assert err <= 1e-4 and np.array_equal(got[:, 1:], y[:, 1:].astype(np.float64))


# ---- 3. dense -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS)
def test_dense_inverse_is_the_point_solver_on_the_lattice(net, smooth):
    D, H, W = net
    s = smooth[net]
    phi_d, L = s["phi_d"], FIELDS[net][1]
    psi, stats, status = ops.invert_phi(phi_d, return_status=True)
    assert psi.shape == phi_d.shape and psi.dtype == torch.float32 and status.shape == net and status.dtype == torch.uint8
    lat = ref.lattice(net)
    lat_d = _cuda(lat.astype(np.float32))
    # the point solver at every lattice point, with phi's storage convention as its net_to_out: the same device function, the same bits
    to_unit = (np.diag([1.0 / (W - 1), 1.0 / (H - 1), 1.0 / (D - 1)]), np.zeros(3))
    pt, pt_st = ops.inverse_points_through_phi(lat_d, phi_d, EYE, to_unit, return_status=True)
    pt = pt.cpu().numpy()
    for c in range(3):
        assert np.array_equal(_bits(psi[2 - c]).reshape(-1), _bits(np.ascontiguousarray(pt[:, c]))), c
    st = status.cpu().numpy().reshape(-1)
    assert np.array_equal(st, pt_st.cpu().numpy()) and np.array_equal(st, s["status"])
    # the stats: recomputed from the status output and the iterations of the restatement (whose iterates are the kernel's)
    assert isinstance(stats, ops.PhiInverseStats)
    assert (stats.points, stats.unconverged, stats.outside) == (D * H * W, int((st == 0).sum()), int((st == 2).sum())) and stats.unconverged == 0
    print(net, stats, "reference residual", float(s["resid"].max()))
    assert stats.max_iterations == int(s["iters"].max()) and stats.mean_iterations == float(s["iters"].sum()) / (D * H * W)
    assert stats.max_residual <= TOL and abs(stats.max_residual - float(s["resid"].max())) <= 1e-12
    ref_psi = np.stack([(s["x"][:, 2 - ch] * (1.0 / (n - 1))).astype(np.float32).reshape(net) for ch, n in enumerate(net)])
    print("psi not bitwise the restatement's", int((_bits(psi) != _bits(ref_psi)).sum()))
    assert (np.abs(psi.cpu().numpy().astype(np.float64) - ref_psi) <= np.spacing(ref_psi)).all()
    # identical with and without the optional output, and into a caller's tensor
    psi2, stats2 = ops.invert_phi(phi_d)
    slot = torch.full_like(phi_d, float("nan"))
    psi3, stats3 = ops.invert_phi(phi_d, out=slot)
    assert psi3 is slot and stats2 == stats and stats3 == stats and np.array_equal(_bits(psi2), _bits(psi)) and np.array_equal(_bits(psi3), _bits(psi))
    # psi is a phi: the existing point push reads it, and phi after psi returns every interior lattice point.  Three float32 roundings on the
    # psi side, each at most 2^-24 (n - 1), amplified by 1 + L <= 1.5, plus the output rounding: about 5.5 such units; 8 leaves margin for the lerp
    mid = ops.transform_points_through_phi(lat_d, psi, EYE, EYE)
    back = ops.transform_points_through_phi(mid, phi_d, EYE, EYE).cpu().numpy().astype(np.float64)
    interior = ((lat > 0) & (lat < np.array([W - 1, H - 1, D - 1]))).all(axis=1)
    rt = np.abs(back - lat)[interior].max()
    print("phi(psi(lattice)) - lattice: max", float(rt), "allowed", 8 * 2.0 ** -24 * (max(net) - 1))
    assert interior.any() and rt <= 8 * 2.0 ** -24 * (max(net) - 1)
    jac = ops.phi_jacobian(psi).cpu().numpy()
    assert jac[0] == (D - 1) * (H - 1) * (W - 1) and jac[1] == 0 and jac[2] == 0          # no folds, every determinant finite


# ---- 4. folded input ------------------------------------------------------------------------------------------------------------------------
def test_folded_phi_returns_and_flags_what_it_could_not_solve():
    """random_phi(0.2) moves every lattice point by up to a fifth of the extent: heavily folded.  A point flagged 1 or 2 satisfies
    |T(x) - y| <= 2 tol, evaluated with the numpy forward restatement.  The outputs are float32, so what can be evaluated is T at the
    ROUNDED x: the rounding moves x by at most half a float32 step per axis, and T by at most (1 + G) times that, G = the largest
    row sum of the one-voxel differences of the displacement (which bound the gradient of the trilinear interpolant in every cell);
    that term is added to 2 tol.  Where the kernel's status equals the restatement's (everywhere, unless the chaotic iteration
    separates them) the restatement's own fp64 x is also held to 2 tol with nothing added."""
    net = (6, 7, 9)
    D, H, W = net
    rng = np.random.default_rng(41)
    phi = mref.random_phi(net, rng, 0.2)
    phi_d = _cuda(phi)
    disp = mref.displacement(phi)
    G = max(float(sum(np.abs(np.diff(disp[..., c], axis=ax)).max() for ax in range(3))) for c in range(3))
    pts = _draw_points(rng, 1000, net, EYE)
    got, status = ops.inverse_points_through_phi(_cuda(pts), phi_d, EYE, EYE, return_status=True)
    got, status = got.cpu().numpy(), status.cpu().numpy()
    assert np.isfinite(got).all() and np.isin(status, (0, 1, 2)).all()
    y = pts.astype(np.float64)
    x_ref, st_ref, _, _ = ref.solve_ref(phi, y)
    print("points: status counts", np.bincount(status, minlength=3).tolist(), "restatement's", np.bincount(st_ref, minlength=3).tolist(),
          "status differs at", int((status != st_ref).sum()), "gradient bound", G)
    ok = status != 0
    assert ok.any() and (~ok).any()
    x32 = got.astype(np.float64)
    resid = np.abs(ref.forward_net(phi, x32) - y)
    allowed = 2 * TOL + (1 + G) * 0.5 * np.abs(np.spacing(got)).astype(np.float64).max(axis=1, keepdims=True)
    print("flagged 1 or 2: max |T(x) - y|", float(resid[ok].max()), "allowed at most", float(allowed[ok].max()))
    assert (resid[ok] <= allowed[ok]).all()
    assert np.array_equal(status[ok] == 1, mref.inside_buffer(x32[ok], net))
    same = ok & (status == st_ref) & (_bits(got) == _bits(x_ref.astype(np.float32))).all(axis=1)
    assert (np.abs(ref.forward_net(phi, x_ref[same]) - y[same]) <= 2 * TOL).all()
    assert np.array_equal(_bits(got[~ok]), _bits(pts[~ok]))                     # flagged 0: the affine-only image, bit for bit
    A, B = _geometries()                                                        # ... also under affines that are not the identity
    q2n, n2q = mp.mesh_point_affines(A, B, net, "physical", "spacing", inverse=True)
    pts = _draw_points(rng, 500, net, q2n)
    got, status = ops.inverse_points_through_phi(_cuda(pts), phi_d, q2n, n2q, return_status=True)
    got, bad = got.cpu().numpy(), status.cpu().numpy() == 0
    want = mref.apply_affine(n2q, mref.apply_affine(q2n, pts.astype(np.float64))).astype(np.float32)
    assert bad.any() and np.isfinite(got).all() and np.array_equal(_bits(got[bad]), _bits(want[bad]))
    # dense
    psi, stats, st = ops.invert_phi(phi_d, return_status=True)
    st = st.cpu().numpy()
    print("dense:", stats, "restatement's unconverged", int((ref.solve_ref(phi, ref.lattice(net))[1] == 0).sum()))
    assert torch.isfinite(psi).all() and stats.unconverged == int((st == 0).sum()) > 0 and stats.outside == int((st == 2).sum())
    assert stats.points == D * H * W and stats.max_iterations == 30 and stats.max_residual <= TOL
    ident = mref.identity_phi(net)
    assert np.array_equal(_bits(psi)[:, st == 0], _bits(ident)[:, st == 0])     # unconverged lattice points hold their identity coordinate


# ---- 5. DisplacementTransform.inverse() -------------------------------------------------------------------------------------------------------
def test_displacement_transform_inverse(smooth):
    net = (12, 16, 20)
    D, H, W = net
    phi = smooth[net]["phi"]
    A, B = _meta(net, [1.0, 1.0, 1.0]), _meta(net, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    T = DisplacementTransform(mref.displacement(phi), A, B, phi)
    assert T.inverse_stats is None
    Ti = T.inverse()
    assert Ti.image_A is T.image_B and Ti.image_B is T.image_A and isinstance(Ti.inverse_stats, ops.PhiInverseStats)
    assert Ti.inverse_stats.points == D * H * W and Ti.inverse_stats.unconverged == 0 and Ti.inverse_stats.max_residual <= TOL
    psi, _ = ops.invert_phi(smooth[net]["phi_d"])
    assert Ti.phi.dtype == np.float32 and np.array_equal(_bits(Ti.phi), _bits(psi)) and np.array_equal(Ti.displacement, mref.displacement(Ti.phi))
    assert Ti.displacement.shape == (D, H, W, 3) and Ti.displacement.dtype == np.float64
    with pytest.raises(ValueError, match="carries no phi"):
        DisplacementTransform(mref.displacement(phi), A, B, None).inverse()
    # a mesh whose pushed vertices land on psi's lattice points (where the stored psi is not interpolated) comes back: the bound of the dense test
    lat = ref.lattice(net)
    interior = ((lat > 0) & (lat < np.array([W - 1, H - 1, D - 1]))).all(axis=1)
    verts = ops.transform_points_through_phi(_cuda(lat[interior].astype(np.float32)), psi, EYE, EYE).cpu().numpy()
    faces = np.random.default_rng(1).integers(0, len(verts), size=(50, 3)).astype(np.int32)
    m = mp.Mesh(verts, faces, {"Distance": np.arange(len(verts), dtype=np.float32)})
    back = mp.transform_mesh(mp.transform_mesh(m, T), Ti)
    rt = np.abs(back.verts.astype(np.float64) - verts.astype(np.float64)).max()
    print("transform_mesh(transform_mesh(m, T), T.inverse()) - m: max", float(rt), "allowed", 8 * 2.0 ** -24 * (max(net) - 1))
    assert rt <= 8 * 2.0 ** -24 * (max(net) - 1) and np.array_equal(back.faces, faces) and np.array_equal(back.point_data["Distance"], m.point_data["Distance"])
    # identity phi on two different grids: pulling an atlas-space image onto the patient grid through T.inverse() IS the plain resample
    A = _meta((9, 11, 13), [0.5, 0.6, 0.9], [3.0, 2.0, -1.0], _rotated_flipped())
    B = _meta((10, 12, 8), [0.7, 0.5, 1.1], [-5.0, 4.0, 0.25], _rotated_flipped().T)
    ident = mref.identity_phi(net)
    T0 = DisplacementTransform(mref.displacement(ident), A, B, ident)
    T0i = T0.inverse()
    assert np.array_equal(_bits(T0i.phi), _bits(ident)) and not T0i.displacement.any() and T0i.inverse_stats.max_iterations == 1
    img = Image(np.random.default_rng(2).uniform(size=(10, 12, 8)).astype(np.float32), B.spacing, B.origin, B.direction)     # on the atlas grid
    pulled = deform_probmap(T0i, B, A, img)
    plain = deform_probmap(DisplacementTransform(np.zeros((D, H, W, 3)), B, A, ident), B, A, img)
    assert pulled.array.shape == (9, 11, 13) and np.array_equal(pulled.array, plain.array) and pulled.array.any()


# ---- 6. transform_mesh(..., inverse=True) -----------------------------------------------------------------------------------------------------
def test_transform_mesh_inverse_round_trip_and_identity(smooth):
    net = (12, 16, 20)
    phi, L = smooth[net]["phi"], FIELDS[net][1]
    A, B = _geometries()
    rng = np.random.default_rng(9)
    for ca, cb in (("physical", "physical"), ("spacing", "physical"), ("spacing", "spacing")):
        q2n, _ = mp.mesh_point_affines(A, B, net, ca, cb, inverse=True)
        _, n2o = mp.mesh_point_affines(A, B, net, cb, ca)
        verts = _draw_points(rng, 700, net, q2n)                               # in ``ca`` coordinates on the patient's grid
        faces = rng.integers(0, 700, size=(900, 3)).astype(np.int32)
        m = mp.Mesh(verts, faces, {"Distance": rng.uniform(size=700).astype(np.float32), "vec": rng.uniform(size=(700, 2))})
        pulled = mp.transform_mesh(m, phi, A, B, coords_in=ca, coords_out=cb, inverse=True)
        assert isinstance(pulled, mp.Mesh) and pulled.verts.dtype == np.float32 and not np.array_equal(pulled.verts, verts)
        assert np.array_equal(pulled.faces, faces) and pulled.faces.dtype == np.int32
        assert sorted(pulled.point_data) == ["Distance", "vec"] and all(np.array_equal(pulled.point_data[k], m.point_data[k]) for k in m.point_data)
        via_transform = mp.transform_mesh(m, DisplacementTransform(mref.displacement(phi), A, B, phi), coords_in=ca, coords_out=cb, inverse=True)
        assert np.array_equal(_bits(via_transform.verts), _bits(pulled.verts))
        back = mp.transform_mesh(pulled, phi, A, B, coords_in=cb, coords_out=ca)
        rt = np.abs(back.verts.astype(np.float64) - verts.astype(np.float64))
        allowed = np.abs(n2o[0]).sum(axis=1) * _round_trip_voxels(net, L)
        print(ca, cb, "round trip / allowed", float((rt / allowed[None, :]).max()))
        assert (rt <= allowed[None, :]).all()
    # the identity phi on an exact geometry returns the mesh bit for bit
    net = (6, 10, 12)
    img = _meta(net, [2.0, 1.0, 0.5], [1.0, -2.5, 3.0])
    verts = rng.uniform(-4, 26, size=(300, 3)).astype(np.float32)              # inside and outside the buffer alike
    m = mp.Mesh(verts, rng.integers(0, 300, size=(500, 3)).astype(np.int32))
    ident = mref.identity_phi(net)
    for tr, kw in ((ident, dict(image_A=img, image_B=img)), (_cuda(ident), dict(image_A=img, image_B=img)),
                   (DisplacementTransform(mref.displacement(ident), img, img, ident), {})):
        out = mp.transform_mesh(m, tr, inverse=True, **kw)
        assert np.array_equal(_bits(out.verts), _bits(verts)) and np.array_equal(out.faces, m.faces)
    with pytest.raises(ValueError, match="image_A and image_B"):
        mp.transform_mesh(m, ident, inverse=True)
    with pytest.raises(ValueError, match="no phi"):
        mp.transform_mesh(m, DisplacementTransform(mref.displacement(ident), img, img, None), inverse=True)


# ---- 7. native thickness: space="patient_grid" ------------------------------------------------------------------------------------------------
_sig = lambda t: 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))
T_BOWL = 6.0
MIN_CELLS = {"FC": 3000, "TC": 100}
NO_REGION = "n_samples=0 should be >= n_clusters=2."


def _bowl(shift_x=0.0, T=T_BOWL):
    """tests/test_thickness_native_gpu.py::_bowl: a cap of a spherical shell of thickness T (TC-sized), optionally shifted along x."""
    D, H, W = 48, 96, 96
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    x = x - shift_x
    r = np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4 + (y + 30) ** 2)
    prob = _sig(2.0 * (np.abs(r - 60.0) - T / 2)) * _sig(2.0 * (np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4) - 30))
    return Image(prob.astype(np.float32), [1.0, 1.0, 1.0])


def _same_knee(a, b):
    return (np.array_equal(_bits(a.fc), _bits(b.fc)) and np.array_equal(_bits(a.tc), _bits(b.tc)) and a.errors == b.errors and a.space == b.space
            and a.outside == b.outside and a.unconverged == b.unconverged)


def _threads():
    return [t.name for t in threading.enumerate() if t.name.startswith("oai-thickness")]


@pytest.fixture(scope="module")
def atlas():
    """The stand-in atlas: the bowl for both cartilages (the femoral split fails on it or not -- either way it is recorded per knee)."""
    from oai_analysis_2_amd.thickness import ThicknessAtlas
    return ThicknessAtlas(_bowl(1.5), _bowl(1.5), image_shape=(32, 32), min_cells=MIN_CELLS["TC"])


@pytest.fixture(scope="module")
def tc_knee():
    """No FC cartilage (an empty map: its error is recorded, nothing is computed for it) and the TC bowl, on the device."""
    return torch.zeros((8, 8, 8), device="cuda"), _cuda(_bowl(0.0).array)


def test_patient_grid_thickness_identity_phi_is_the_atlas_space_thickness(atlas, tc_knee):
    fc_t, tc_t = tc_knee
    shape = tuple(tc_t.shape)
    plain = atlas.measure(fc_t, tc_t)
    assert plain.space == "atlas" and plain.unconverged == {} and plain.errors == {"FC": NO_REGION}
    assert np.isfinite(plain.tc).all() and abs(np.median(plain.tc) - T_BOWL) < 0.15 * T_BOWL
    phi, meta = _cuda(mref.identity_phi(shape)), _meta(shape, [1.0, 1.0, 1.0])
    got = atlas.measure(fc_t, tc_t, spacing_xyz=[1.0, 1.0, 1.0], phi=phi, image_A=meta, space="patient_grid")
    assert got.space == "patient_grid" and got.errors == plain.errors and got.outside == {"TC": 0} and got.unconverged == {"TC": 0}
    assert np.array_equal(_bits(got.tc), _bits(plain.tc)) and np.isnan(got.fc).all()
    by_default = atlas.measure(fc_t, tc_t, phi=phi, image_A=meta, space="patient_grid", keep_on_device=True)       # spacing: image_A's
    assert by_default.tc.is_cuda and np.array_equal(_bits(by_default.tc), _bits(got.tc))
    assert _same_knee(atlas.measure(fc_t, tc_t, space="atlas"), plain)          # the spelled-out defaults are the defaults
    pushed = atlas.measure(fc_t, tc_t, phi=phi, image_A=meta)
    assert _same_knee(atlas.measure(fc_t, tc_t, phi=phi, image_A=meta, space="patient"), pushed) and pushed.space == "patient" and pushed.unconverged == {}
    # a smooth phi on another patient grid: the vertices are pulled, not left where they are, and all of them are placed
    net = (12, 16, 20)
    warped = atlas.measure(fc_t, tc_t, phi=_cuda(ref.smooth_phi(net, FIELDS[net][0])), image_A=_meta(shape, [1.0, 1.0, 1.0], [0.5, -0.25, 0.0]),
                           space="patient_grid")
    assert warped.unconverged == {"TC": 0} and np.isfinite(warped.tc).any() and not np.array_equal(_bits(warped.tc), _bits(plain.tc))
    # argument errors
    with pytest.raises(ValueError, match="image_A is missing"):
        atlas.measure(fc_t, tc_t, phi=phi, space="patient_grid")
    with pytest.raises(ValueError, match="phi is missing"):
        atlas.measure(fc_t, tc_t, image_A=meta, space="patient_grid")
    with pytest.raises(ValueError, match="needs phi and image_A"):
        atlas.measure(fc_t, tc_t, space="patient_grid")
    with pytest.raises(ValueError, match="takes no phi"):
        atlas.measure(fc_t, tc_t, phi=phi, image_A=meta, space="atlas")
    with pytest.raises(ValueError, match="space"):
        atlas.measure(fc_t, tc_t, phi=phi, image_A=meta, space="native")


def test_patient_grid_thickness_through_the_pipeline_and_the_stream(atlas, tc_knee):
    from oai_analysis_2_amd.dask_processing import thickness_stream
    from oai_analysis_2_amd.pipeline import VolumePipeline, VolumeResult
    from oai_analysis_2_amd.registration import IconEngine
    from oai_analysis_2_amd.segmentation.engine import UNetEngine
    from oai_analysis_2_amd.synth import make_icon_state_dict, make_unet_state_dict, make_volume
    from oai_analysis_2_amd.thickness import KneeThickness
    # tests/test_thickness_native_gpu.py::_small_pipe
    shape, net = (24, 72, 72), (40, 48, 48)
    pipe = VolumePipeline(UNetEngine(make_unet_state_dict(1, width_div=2)), IconEngine(make_icon_state_dict(1, last_scale=0.1), net_shape=net),
                          Image(make_volume(10, shape), [0.4, 0.35, 0.75], [0.0, -1.0, 2.0]), tile_zyx=(16, 32, 32), overlap_zyx=(4, 8, 8),
                          crop_zyx=(4, 8, 8), batch=8)
    vol = make_volume(9, shape)
    meta = Image(vol, [0.36, 0.37, 0.7], [1.0, 2.0, 3.0])
    v = _cuda(vol)
    base = pipe.run(v, meta)
    on = pipe.run(v, meta, thickness=atlas, thickness_space="patient_grid")
    for name in ("fc", "tc", "phi", "fc_atlas", "tc_atlas"):
        assert torch.equal(getattr(on, name), getattr(base, name)), name
    assert base.thickness is None and isinstance(on.thickness, KneeThickness) and on.thickness.space == "patient_grid"
    direct = atlas.measure(on.fc, on.tc, spacing_xyz=meta.spacing, phi=on.phi, image_A=meta, space="patient_grid")
    assert _same_knee(on.thickness, direct)
    for kind in ("FC", "TC"):                                                  # (on this synthetic volume an unmeasurable cartilage is an acceptable outcome)
        vec = on.thickness[kind]
        assert (kind in on.thickness.errors and np.isnan(vec).all()) or (kind not in on.thickness.errors and kind in on.thickness.unconverged)
    # the stream: the patient-grid maps of each result, through its own phi
    fc_t, tc_t = tc_knee
    tiny = torch.zeros(1, device="cuda")
    knee_shape = tuple(tc_t.shape)
    phis = [_cuda(mref.identity_phi(knee_shape)), _cuda(ref.smooth_phi((12, 16, 20), FIELDS[(12, 16, 20)][0]))]
    metas = [_meta(knee_shape, [1.0, 1.0, 1.0]), _meta(knee_shape, [1.0, 1.0, 1.0], [0.5, -0.25, 0.0])]
    results = [(7 + i, VolumeResult(fc_t, tc_t, p, tiny, tiny, meta_A=m)) for i, (p, m) in enumerate(zip(phis, metas))]
    want = [atlas.measure(fc_t, tc_t, phi=p, image_A=m, space="patient_grid") for p, m in zip(phis, metas)]
    assert all(w.space == "patient_grid" and "TC" not in w.errors for w in want) and not np.array_equal(_bits(want[0].tc), _bits(want[1].tc))
    got = list(thickness_stream(iter(results), atlas, space="patient_grid"))
    assert [i for i, _ in got] == [7, 8] and all(_same_knee(k, w) for (_, k), w in zip(got, want))
    assert _threads() == []
    with pytest.raises(ValueError, match="meta_A"):
        list(thickness_stream(iter([(0, VolumeResult(fc_t, tc_t, phis[0], tiny, tiny))]), atlas, space="patient_grid"))
    assert _threads() == []


# ---- 8. bad arguments ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_do_not_fault():
    phi = _cuda(mref.identity_phi((4, 5, 6)))
    pts = torch.zeros((10, 3), device="cuda")
    bad = (_lib.OaiError, ValueError)
    with pytest.raises(bad):
        ops.inverse_points_through_phi(pts, phi[0], EYE, EYE)                         # rank 3
    with pytest.raises(bad):
        ops.inverse_points_through_phi(pts, phi[:2], EYE, EYE)                        # two channels
    with pytest.raises(bad):
        ops.inverse_points_through_phi(pts, phi.double(), EYE, EYE)                   # dtype
    with pytest.raises(bad):
        ops.inverse_points_through_phi(pts, phi[:, :1], EYE, EYE)                     # Dn = 1
    with pytest.raises(bad):
        ops.inverse_points_through_phi(pts[:, :2], phi, EYE, EYE)                     # points [n,2]
    with pytest.raises(bad):
        ops.inverse_points_through_phi(pts.reshape(-1), phi, EYE, EYE)                # points [3n]
    with pytest.raises(bad):
        ops.inverse_points_through_phi(pts.cpu(), phi, EYE, EYE)                      # host points
    with pytest.raises(bad):
        ops.inverse_points_through_phi(pts, phi, EYE, EYE, max_iter=0)
    with pytest.raises(bad):
        ops.inverse_points_through_phi(pts, phi, EYE, EYE, tol=0.0)
    with pytest.raises(bad):
        ops.invert_phi(phi[0])
    with pytest.raises(bad):
        ops.invert_phi(phi[:2])
    with pytest.raises(bad):
        ops.invert_phi(phi.double())
    with pytest.raises(bad):
        ops.invert_phi(phi[:, :, :1])                                                 # Hn = 1
    with pytest.raises(bad):
        ops.invert_phi(phi.cpu())
    with pytest.raises(bad):
        ops.invert_phi(phi, max_iter=0)
    with pytest.raises(bad):
        ops.invert_phi(phi, tol=-1e-7)
    with pytest.raises(bad):
        ops.invert_phi(phi, out=phi)                                                  # in place
    with pytest.raises(bad):
        ops.invert_phi(phi, out=torch.empty((3, 4, 5, 7), device="cuda"))
    with pytest.raises(ValueError):
        mp.transform_mesh(mp.Mesh(np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32)), np.zeros((4, 5, 6), np.float32), _meta((4, 5, 6), [1, 1, 1]),
                          _meta((4, 5, 6), [1, 1, 1]), inverse=True)
    out = ops.inverse_points_through_phi(pts, phi, EYE, EYE)                          # and the device is fine afterwards
    psi, stats = ops.invert_phi(phi)
    assert torch.equal(out, pts) and torch.equal(psi, phi) and stats.unconverged == 0 and stats.max_iterations == 1
