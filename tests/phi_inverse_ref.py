"""fp64 restatement of the inverse of phi (csrc/phi_inverse.hip, ops.inverse_points_through_phi, ops.invert_phi); numpy only.

TEST INFRASTRUCTURE.  *** PARITY UNPINNED ***: ITK is not installed; this restates what itk.Transform.GetInverseTransform means for a
displacement field -- a numerical inverse of the map that is held -- on top of the forward restatement of tests/mesh_transform_ref.py.

``solve_ref`` performs the kernel's operations in the kernel's order (the forward value is ``oracle.resample._trilinear_clamped``, the
gradient is written from the same eight corners, the Newton step by the same adjugate expressions), so iterates, status bytes and
iteration counts are the kernel's to the bit; the only rounding left open is the final one to float32.
"""
from __future__ import annotations

import numpy as np

import mesh_transform_ref as mref
from oracle.resample import _trilinear_clamped

DET_MIN = 1e-3


def smooth_phi(net_shape, amp_xyz) -> np.ndarray:
    """float32 [3,D,H,W]: identity + amp_c * sin(pi x/(W-1)) sin(pi y/(H-1)) sin(pi z/(D-1)) * a slow cosine, ``amp_xyz`` in network
    voxels per ITK component (x, y, z).  The displacement is exactly zero on the boundary lattice (set, not left to sin(pi)), so T is
    continuous across the faces of the buffer and every y has a preimage."""
    D, H, W = (int(v) for v in net_shape)
    ident = mref.identity_phi(net_shape).astype(np.float64)
    z, y, x = np.meshgrid(np.arange(D) / (D - 1.0), np.arange(H) / (H - 1.0), np.arange(W) / (W - 1.0), indexing="ij")
    bump = np.sin(np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z)
    bump[[0, -1], :, :] = 0.0
    bump[:, [0, -1], :] = 0.0
    bump[:, :, [0, -1]] = 0.0
    phi = ident.copy()
    for c, n in enumerate((W, H, D)):                       # ITK component c lives in phi channel 2 - c
        slow = np.cos(0.4 + 0.6 * x - 0.4 * y + 0.5 * z + 0.3 * c)
        phi[2 - c] += float(amp_xyz[c]) / (n - 1.0) * bump * slow
    return phi.astype(np.float32)


def disp_and_gradient(disp: np.ndarray, x: np.ndarray):
    """(d [n,3], G [n,3,3]) at network coordinates x [n,3]: d = the clamped trilinear lerp of ``disp`` (float64 [D,H,W,3]), G[:, c, k] =
    d d_c / d x_k of the same polynomial.  A clamped axis has a zero column: at the upper end the two corners coincide, at the lower
    end (coordinate below 0) the column is set to zero."""
    nz, ny, nx = disp.shape[:3]
    ix, iy, iz = x[:, 0], x[:, 1], x[:, 2]
    d = _trilinear_clamped(disp, ix, iy, iz)
    cx, cy, cz = np.clip(ix, 0.0, nx - 1.0), np.clip(iy, 0.0, ny - 1.0), np.clip(iz, 0.0, nz - 1.0)
    x0, y0, z0 = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64), np.floor(cz).astype(np.int64)
    x1, y1, z1 = np.minimum(x0 + 1, nx - 1), np.minimum(y0 + 1, ny - 1), np.minimum(z0 + 1, nz - 1)
    fx, fy, fz = (cx - x0)[:, None], (cy - y0)[:, None], (cz - z0)[:, None]
    v = [disp[zz, yy, xx] for zz in (z0, z1) for yy in (y0, y1) for xx in (x0, x1)]          # corner (zhi, yhi, xhi) at 4 zhi + 2 yhi + xhi
    gx = ((v[1] - v[0]) * (1 - fy) + (v[3] - v[2]) * fy) * (1 - fz) + ((v[5] - v[4]) * (1 - fy) + (v[7] - v[6]) * fy) * fz
    c00, c01 = v[0] * (1 - fx) + v[1] * fx, v[2] * (1 - fx) + v[3] * fx
    c10, c11 = v[4] * (1 - fx) + v[5] * fx, v[6] * (1 - fx) + v[7] * fx
    gy = (c01 - c00) * (1 - fz) + (c11 - c10) * fz
    gz = (c10 * (1 - fy) + c11 * fy) - (c00 * (1 - fy) + c01 * fy)
    G = np.stack([np.where((ix < 0.0)[:, None], 0.0, gx), np.where((iy < 0.0)[:, None], 0.0, gy), np.where((iz < 0.0)[:, None], 0.0, gz)], axis=2)
    return d, G


def forward_net(phi: np.ndarray, x: np.ndarray) -> np.ndarray:
    """T(x) in network index space: x + the clamped trilinear displacement inside the buffer, x outside it."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    d = _trilinear_clamped(mref.displacement(phi), x[:, 0], x[:, 1], x[:, 2]) if len(x) else np.zeros((0, 3))
    return x + np.where(mref.inside_buffer(x, phi.shape[1:])[:, None], d, 0.0)


def solve_ref(phi: np.ndarray, y: np.ndarray, max_iter: int = 30, tol: float = 1e-7):
    """x with T(x) = y per row of y [n,3] (network index space).  Returns (x [n,3], status uint8 [n], iterations int [n], residual [n]):
    status 1 = converged inside the buffer, 2 = converged outside it, 0 = not converged (x = y); residual = max_c |r_c| at convergence."""
    disp = mref.displacement(phi)
    y = np.asarray(y, np.float64).reshape(-1, 3)
    n = len(y)
    x = y.copy()
    out, status, iters, resid = y.copy(), np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros(n)
    active = np.arange(n)
    with np.errstate(all="ignore"):
        for it in range(int(max_iter)):
            if len(active) == 0:
                break
            xa, ya = x[active], y[active]
            iters[active] = it + 1
            inside = mref.inside_buffer(xa, phi.shape[1:])
            d, G = disp_and_gradient(disp, xa)
            d, G = np.where(inside[:, None], d, 0.0), np.where(inside[:, None, None], G, 0.0)
            r = (xa + d) - ya
            rmax = np.fmax(np.fmax(np.abs(r[:, 0]), np.abs(r[:, 1])), np.abs(r[:, 2]))
            done = rmax <= tol
            idx = active[done]
            out[idx], status[idx], resid[idx] = xa[done], np.where(inside[done], 1, 2), rmax[done]
            J00, J01, J02 = 1.0 + G[:, 0, 0], G[:, 0, 1], G[:, 0, 2]
            J10, J11, J12 = G[:, 1, 0], 1.0 + G[:, 1, 1], G[:, 1, 2]
            J20, J21, J22 = G[:, 2, 0], G[:, 2, 1], 1.0 + G[:, 2, 2]
            det = (J00 * (J11 * J22 - J12 * J21) - J01 * (J10 * J22 - J12 * J20)) + J02 * (J10 * J21 - J11 * J20)
            r0, r1, r2 = r[:, 0], r[:, 1], r[:, 2]
            s0 = (((J11 * J22 - J12 * J21) * r0 + (J02 * J21 - J01 * J22) * r1) + (J01 * J12 - J02 * J11) * r2) / det
            s1 = (((J12 * J20 - J10 * J22) * r0 + (J00 * J22 - J02 * J20) * r1) + (J02 * J10 - J00 * J12) * r2) / det
            s2 = (((J10 * J21 - J11 * J20) * r0 + (J01 * J20 - J00 * J21) * r1) + (J00 * J11 - J01 * J10) * r2) / det
            newton = np.abs(det) > DET_MIN
            s = np.stack([np.where(newton, s0, r0), np.where(newton, s1, r1), np.where(newton, s2, r2)], axis=1)
            go = ~done & np.isfinite(s).all(axis=1)
            x[active[go]] = xa[go] - s[go]
            active = active[go]
    return out, status, iters, resid


def inverse_points_ref(points: np.ndarray, phi: np.ndarray, point_to_net, net_to_out, max_iter: int = 30, tol: float = 1e-7):
    """(out float64 [n,3], status, iterations, y float64 [n,3] network coordinates of the points, x the solved network points)."""
    y = mref.apply_affine(point_to_net, np.asarray(points, np.float32).astype(np.float64))
    x, status, iters, _ = solve_ref(phi, y, max_iter, tol)
    return mref.apply_affine(net_to_out, x), status, iters, y, x


def lattice(net_shape) -> np.ndarray:
    """float64 [D*H*W, 3]: every lattice point (x, y, z), x fastest."""
    D, H, W = (int(v) for v in net_shape)
    zz, yy, xx = np.mgrid[0:D, 0:H, 0:W]
    return np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(np.float64)


def invert_phi_ref(phi: np.ndarray, max_iter: int = 30, tol: float = 1e-7):
    """(psi float32 [3,D,H,W], status uint8 [D,H,W], stats): stats = (points, unconverged, converged outside, max residual over the
    converged points, sum of iterations, max iterations), as oai_invert_phi's double[6]."""
    D, H, W = (int(v) for v in phi.shape[1:])
    x, status, iters, resid = solve_ref(phi, lattice((D, H, W)), max_iter, tol)
    psi = np.stack([(x[:, 2 - ch] * (1.0 / (n - 1))).astype(np.float32).reshape(D, H, W) for ch, n in enumerate((D, H, W))])
    stats = (D * H * W, int((status == 0).sum()), int((status == 2).sum()), float(resid.max()), int(iters.sum()), int(iters.max()))
    return psi, status.reshape(D, H, W), stats


def gradient_row_sum(phi: np.ndarray) -> float:
    """max over the cell centres and the components c of sum_k |d u_c / d x_k|: the bound L on how much T - identity stretches."""
    D, H, W = (int(v) for v in phi.shape[1:])
    zz, yy, xx = np.mgrid[0:D - 1, 0:H - 1, 0:W - 1]
    centres = np.stack([xx, yy, zz], -1).reshape(-1, 3) + 0.5
    return float(np.abs(disp_and_gradient(mref.displacement(phi), centres)[1]).sum(axis=2).max())


def inverse_affine(Ab):
    A, b = np.asarray(Ab[0], np.float64).reshape(3, 3), np.asarray(Ab[1], np.float64).reshape(3)
    Ai = np.linalg.inv(A)
    return Ai, -Ai @ b
