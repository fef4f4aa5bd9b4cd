"""GPU: points pushed through phi (csrc/mesh_transform.hip, ops.transform_points_through_phi, mesh_processing.transform_mesh) against
the fp64 restatement of tests/mesh_transform_ref.py to one float32 ulp, the exact cases bit for bit, an analytic stretch, and the
argument errors."""
import numpy as np
import pytest
import torch

import mesh_transform_ref as ref
from oai_analysis_2_amd import _lib, ops
from oai_analysis_2_amd import mesh_processing as mp
from oai_analysis_2_amd.image import Image
from oai_analysis_2_amd.registration import DisplacementTransform

pytestmark = pytest.mark.gpu


def _meta(shape_zyx, spacing, origin=(0.0, 0.0, 0.0), direction=None):
    return Image(np.broadcast_to(np.zeros((), np.float32), shape_zyx), spacing, origin, np.eye(3) if direction is None else direction)


def _rotated_flipped():
    """A rotation about a skew axis (Rodrigues) with the y axis flipped: det = -1."""
    k = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    d = (np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K) @ np.diag([1.0, -1.0, 1.0])
    assert np.linalg.det(d) < 0
    return d


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


def _draw_points(rng, n, net, p2n):
    """n float32 points whose network coordinates are uniform over the buffer widened by 3.9 % of each axis on both sides: 0.928^3 = 0.8
    of them fall inside, a fifth outside.  No point lies within 1e-6 voxels of a face of the buffer, by construction."""
    Dn, Hn, Wn = net
    size = np.array([Wn, Hn, Dn], np.float64)
    x = rng.uniform(-0.5 - 0.0386 * size, size - 0.5 + 0.0386 * size, size=(n, 3))
    for face in (np.full(3, -0.5), size - 0.5):              # a coordinate drawn within 1e-3 voxels of a face moves to 1e-3 from it, on its own side:
        d = x - face                                         # the rounding of the points to float32 (some 1e-5 voxels here) then leaves every point
        x = np.where(np.abs(d) < 1e-3, face + np.where(d < 0, -1e-3, 1e-3), x)       # at least 1e-6 from every face, which the test asserts
    A, b = p2n
    return ((x - b) @ np.linalg.inv(A).T).astype(np.float32)


@pytest.mark.parametrize("net", [(2, 2, 2), (3, 4, 5), (6, 7, 9)])
def test_against_the_fp64_restatement_to_one_float32_ulp(net):
    rng = np.random.default_rng(100 + net[2])
    phi = ref.random_phi(net, rng, 0.2)
    A = _meta((11, 13, 17), [0.36, 0.37, 0.7], [10.0, -20.0, 5.0], _rotated_flipped())
    B = _meta((8, 12, 10), [0.4, 0.35, 0.75], [0.0, -1.0, 2.0], _rotated_flipped().T)
    phi_d = torch.from_numpy(phi).cuda()
    n_out = n_all = 0
    for cin, cout in (("physical", "physical"), ("spacing", "spacing")):
        p2n, n2o = mp.mesh_point_affines(A, B, net, cin, cout)
        for n in (0, 1, 63, 64, 65, 1000):
            pts = _draw_points(rng, n, net, p2n)
            want, inside, x = ref.transform_points_ref(pts, phi, p2n, n2o)
            assert n == 0 or ref.face_margin(x, net).min() >= 1e-6          # every drawn point is kept: none sits on a face of the buffer
            got, got_in = ops.transform_points_through_phi(torch.from_numpy(pts).cuda(), phi_d, p2n, n2o, return_inside=True)
            assert got.shape == (n, 3) and got.dtype == torch.float32 and got_in.shape == (n,) and got_in.dtype == torch.uint8
            got, got_in = got.cpu().numpy(), got_in.cpu().numpy().astype(bool)
            assert np.array_equal(got_in, inside)                           # the mask: exactly
            w32 = want.astype(np.float32)
            err = np.abs(got.astype(np.float64) - w32.astype(np.float64))
            ulp = np.abs(np.spacing(w32)).astype(np.float64)
            if n:
                print(net, cin, "n", n, "outside", int((~inside).sum()), "max error in ulps", float((err / ulp).max()),
                      "not bitwise", int((_bits(got) != _bits(w32)).sum()))
            assert (err <= ulp).all()
            n_out, n_all = n_out + int((~inside).sum()), n_all + n
            alone = ops.transform_points_through_phi(torch.from_numpy(pts).cuda(), phi_d, p2n, n2o)       # without the mask: the same points
            assert np.array_equal(_bits(alone), _bits(got))
    assert 0.1 < n_out / n_all < 0.3                                        # about a fifth fell outside the buffer


def test_exact_cases_buffer_faces_outside_points_and_lattice_points():
    net = (6, 7, 9)
    Dn, Hn, Wn = net
    B = _meta(net, [2.0, 1.0, 0.5], [-4.0, 0.5, 8.0])
    A = _meta(net, [4.0, 2.0, 1.0], [1.0, -2.5, 3.0])
    p2n, n2o = mp.mesh_point_affines(A, B, net)
    assert np.array_equal(p2n[0], np.diag(1.0 / B.spacing)) and np.array_equal(n2o[0], np.diag(A.spacing)) and not p2n[1].any() and not n2o[1].any()
    phi = ref.random_phi(net, np.random.default_rng(7), 0.2)
    phi_d = torch.from_numpy(phi).cuda()
    # network coordinates on the faces of the buffer: exactly -0.5 is inside, exactly n - 0.5 is outside (the half-open test)
    x = np.array([[-0.5, 3, 2], [4, -0.5, 2], [4, 3, -0.5], [Wn - 0.5, 3, 2], [4, Hn - 0.5, 2], [4, 3, Dn - 0.5], [-0.5, -0.5, -0.5],
                  [Wn - 0.5, -0.5, -0.5], [-3.0, 2, 2], [4, 30.0, 2]], np.float64)
    pts = (x * B.spacing).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64) / B.spacing, x)                       # exactly representable
    got, inside = ops.transform_points_through_phi(torch.from_numpy(pts).cuda(), phi_d, p2n, n2o, return_inside=True)
    assert inside.cpu().tolist() == [1, 1, 1, 0, 0, 0, 1, 0, 0, 0]
    out = ~inside.cpu().numpy().astype(bool)
    assert np.array_equal(_bits(got)[out], _bits((x * A.spacing).astype(np.float32))[out])     # outside: the pure affine image
    want, want_in, _ = ref.transform_points_ref(pts, phi, p2n, n2o)
    assert np.array_equal(want_in, ~out) and np.array_equal(_bits(got), _bits(want.astype(np.float32)))
    # every lattice point: float32(lattice + displacement), the displacement being what oai_phi_to_itk_displacement stores
    disp = ops.phi_to_itk_displacement(phi_d).cpu().numpy()                            # float64 [D,H,W,3], xyz
    assert np.array_equal(disp, ref.displacement(phi))
    zz, yy, xx = np.mgrid[0:Dn, 0:Hn, 0:Wn]
    lat = np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(np.float64)
    got, inside = ops.transform_points_through_phi(torch.from_numpy((lat * B.spacing).astype(np.float32)).cuda(), phi_d, p2n, n2o, return_inside=True)
    assert bool(inside.all())
    want = ((lat + disp.reshape(-1, 3)) * A.spacing).astype(np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    unit = mp.mesh_point_affines(_meta(net, [1.0, 1.0, 1.0]), _meta(net, [1.0, 1.0, 1.0]), net)           # spacing 1 on both sides: literally lattice + displacement
    got = ops.transform_points_through_phi(torch.from_numpy(lat.astype(np.float32)).cuda(), phi_d, *unit)
    assert np.array_equal(_bits(got), _bits((lat + disp.reshape(-1, 3)).astype(np.float32)))


def test_identity_phi_returns_the_mesh_bit_for_bit():
    net = (6, 10, 12)
    img = _meta(net, [2.0, 1.0, 0.5], [1.0, -2.5, 3.0])
    rng = np.random.default_rng(3)
    verts = rng.uniform(-4, 26, size=(300, 3)).astype(np.float32)                     # inside and outside the buffer alike
    faces = rng.integers(0, 300, size=(500, 3)).astype(np.int32)
    mesh = mp.Mesh(verts, faces, {"Distance": rng.uniform(size=300).astype(np.float32), "vec": rng.uniform(size=(300, 2))})
    phi = ref.identity_phi(net)
    for tr, kw in ((phi, dict(image_A=img, image_B=img)), (torch.from_numpy(phi).cuda(), dict(image_A=img, image_B=img)),
                   (DisplacementTransform(ref.displacement(phi), img, img, phi), {})):
        out = mp.transform_mesh(mesh, tr, **kw)
        assert isinstance(out, mp.Mesh) and out.verts.dtype == np.float32 and np.array_equal(_bits(out.verts), _bits(verts))
        assert np.array_equal(out.faces, faces) and out.faces.dtype == np.int32
        assert sorted(out.point_data) == ["Distance", "vec"] and all(np.array_equal(out.point_data[k], mesh.point_data[k]) for k in mesh.point_data)
    with pytest.raises(ValueError, match="image_A and image_B"):
        mp.transform_mesh(mesh, phi)
    with pytest.raises(ValueError, match="no phi"):
        mp.transform_mesh(mesh, DisplacementTransform(ref.displacement(phi), img, img, None))


def _plane(x0):
    """A triangulated plane x = x0 over y in [2, 13], z in [1, 6] (unit steps)."""
    ys, zs = np.arange(2, 14), np.arange(1, 7)
    zz, yy = np.meshgrid(zs, ys, indexing="ij")
    verts = np.stack([np.full(yy.size, x0), yy.reshape(-1), zz.reshape(-1)], axis=1).astype(np.float32)
    idx = np.arange(yy.size).reshape(len(zs), len(ys))
    a, b, c, d = idx[:-1, :-1].reshape(-1), idx[:-1, 1:].reshape(-1), idx[1:, 1:].reshape(-1), idx[1:, :-1].reshape(-1)
    return mp.Mesh(verts, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32))


def test_analytic_stretch_along_x():
    """phi stretches x by 1.25 about the centre: two planes 4 apart come out 5 apart.  Tolerance: float32 epsilon (6e-8) x coordinate
    magnitude (< 100) x a handful of roundings in the fp32 displacement rebuild, about 3e-5, under the 1e-4 asserted.  Measured on an
    MI355X: 0 (the pushed planes come out at x = 22.125 and 27.125, the distance at 5.0; the test prints what it sees)."""
    net = (8, 16, 64)
    img = _meta(net, [1.0, 1.0, 1.0])
    phi = ref.identity_phi(net)
    x01 = phi[2].copy()
    phi[2] = (0.5 + 1.25 * (x01 - 0.5)).astype(np.float32)
    near, far = _plane(24.0), _plane(28.0)
    before = mp.point_distance(near.verts, far)
    assert np.abs(before - 4.0).max() <= 1e-6
    p_near, p_far = mp.transform_mesh(near, phi, img, img), mp.transform_mesh(far, phi, img, img)
    assert np.array_equal(p_near.verts[:, 1:], near.verts[:, 1:]) and np.array_equal(p_far.faces, far.faces)      # y and z are untouched
    after = mp.point_distance(p_near.verts, p_far)
    print("pushed x", float(p_near.verts[:, 0].min()), float(p_near.verts[:, 0].max()), float(p_far.verts[:, 0].min()), float(p_far.verts[:, 0].max()),
          "max |distance - 5|", float(np.abs(after - 5.0).max()))
    assert np.abs(p_near.verts[:, 0] - (31.5 + 1.25 * (24.0 - 31.5))).max() <= 1e-4
    assert np.abs(after - 5.0).max() <= 1e-4


def test_bad_arguments_raise_and_do_not_fault():
    phi = torch.from_numpy(ref.identity_phi((4, 5, 6))).cuda()
    pts = torch.zeros((10, 3), device="cuda")
    eye = (np.eye(3), np.zeros(3))
    bad = (_lib.OaiError, ValueError)
    with pytest.raises(bad):
        ops.transform_points_through_phi(pts, phi[0], eye, eye)                       # rank 3
    with pytest.raises(bad):
        ops.transform_points_through_phi(pts, phi[:2], eye, eye)                      # two channels
    with pytest.raises(bad):
        ops.transform_points_through_phi(pts, phi.double(), eye, eye)                 # dtype
    with pytest.raises(bad):
        ops.transform_points_through_phi(pts, phi[:, :1], eye, eye)                   # Dn = 1
    with pytest.raises(bad):
        ops.transform_points_through_phi(pts[:, :2], phi, eye, eye)                   # points [n,2]
    with pytest.raises(bad):
        ops.transform_points_through_phi(pts.reshape(-1), phi, eye, eye)              # points [3n]
    with pytest.raises(bad):
        ops.transform_points_through_phi(pts.cpu(), phi, eye, eye)                    # host points
    with pytest.raises(ValueError):
        mp.transform_mesh(mp.Mesh(np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32)), np.zeros((4, 5, 6), np.float32), _meta((4, 5, 6), [1, 1, 1]),
                          _meta((4, 5, 6), [1, 1, 1]))
    out = ops.transform_points_through_phi(pts, phi, eye, eye)                        # and the device is fine afterwards
    assert torch.equal(out, pts)
