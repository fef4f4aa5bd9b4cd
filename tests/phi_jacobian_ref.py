"""fp64 restatement of the Jacobian determinant of phi (csrc/phi_jacobian.hip, ops.phi_jacobian, qc.registration_qc); numpy only.

TEST INFRASTRUCTURE.  *** PARITY UNPINNED ***: the fold count is what ``icon_registration.losses.flips`` computes; icon_registration is
not installed, so ``flips_form`` restates it as recalled (backward differences of the raw map, ``cross(a, b) . c < 0``, torch fp32).

``det_ref`` performs the kernel's operations in its order on ``mesh_transform_ref.displacement`` (the fp32 rebuild of the displacement
in network voxels, widened): the only difference left to the float32 map is its last rounding, and the fp64 statistics differ by
the order of their sums alone.  ``flips_form`` is the independent definition: other operands (raw phi, not the displacement), another
precision, another expression of the determinant.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import mesh_transform_ref as ref

EPS32 = float(np.finfo(np.float32).eps)


def det_ref(phi: np.ndarray) -> np.ndarray:
    """float64 [D-1,H-1,W-1]: J[r][k] = delta_rk + (u_r(p) - u_r(p - e_k)), r and k over (x, y, z); a NaN / Inf in phi goes where it goes."""
    return det_of_displacement(ref.displacement(phi))


def det_of_displacement(u: np.ndarray) -> np.ndarray:
    """``det_ref`` after the rebuild: the same stencil on a given displacement float64 [D,H,W,3] (xyz components, network voxels)."""
    c = u[1:, 1:, 1:]
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = c - u[1:, 1:, :-1], c - u[1:, :-1, 1:], c - u[:-1, 1:, 1:]
        J00, J01, J02 = 1.0 + dx[..., 0], dy[..., 0], dz[..., 0]
        J10, J11, J12 = dx[..., 1], 1.0 + dy[..., 1], dz[..., 1]
        J20, J21, J22 = dx[..., 2], dy[..., 2], 1.0 + dz[..., 2]
        return (J00 * (J11 * J22 - J12 * J21) - J01 * (J10 * J22 - J12 * J20)) + J02 * (J10 * J21 - J11 * J20)


def stats_ref(det: np.ndarray) -> dict:
    """What the kernel's seven doubles stand for, the sums exactly rounded (math.fsum), plus the sums of magnitudes their bounds need."""
    d = det.reshape(-1)
    ok = np.isfinite(d)
    f = d[ok]
    sq = f * f
    return dict(cells=int(d.size), folds=int((f < 0).sum()), nonfinite=int((~ok).sum()), n_finite=int(f.size),
                min=float(f.min()) if f.size else float("inf"), max=float(f.max()) if f.size else float("-inf"),
                sum=math.fsum(f.tolist()), sum_sq=math.fsum(sq.tolist()), sum_abs=float(np.abs(f).sum()), sum_sq_abs=float(sq.sum()))


def flips_form(phi: np.ndarray) -> np.ndarray:
    """ICON's ``flips`` integrand on the raw map, torch fp32: a, b, c = the backward differences of phi along d, h, w (each a vector over
    the channels), dV = cross(a, b) . c; returned widened and scaled by (D-1)(H-1)(W-1) so that it reads in the units of ``det_ref``
    (the same determinant: rows and columns permuted alike).  float64 [D-1,H-1,W-1]; ``flips`` itself is ``(dV < 0).sum()``."""
    p = torch.from_numpy(np.ascontiguousarray(phi, dtype=np.float32))[None]
    a = p[:, :, 1:, 1:, 1:] - p[:, :, :-1, 1:, 1:]
    b = p[:, :, 1:, 1:, 1:] - p[:, :, 1:, :-1, 1:]
    c = p[:, :, 1:, 1:, 1:] - p[:, :, 1:, 1:, :-1]
    dV = torch.sum(torch.cross(a, b, 1) * c, axis=1)[0]
    D, H, W = phi.shape[1:]
    return dV.double().numpy() * float((D - 1) * (H - 1) * (W - 1))


def drawn_phi(shape, amp: float) -> np.ndarray:
    """identity + uniform(-amp, amp) VOXELS per component (divided by n - 1), float32 [3,D,H,W]; rng = default_rng(100 + W)."""
    D, H, W = (int(v) for v in shape)
    ident = ref.identity_phi(shape)
    if amp == 0:
        return ident
    rng = np.random.default_rng(100 + W)
    scale = np.array([D - 1, H - 1, W - 1], np.float64)[:, None, None, None]
    return (ident.astype(np.float64) + rng.uniform(-amp, amp, size=ident.shape) / scale).astype(np.float32)


def clear_of_zero(phi: np.ndarray, floor: float = 1e-5, rounds: int = 20):
    """(phi, det_ref(phi)) with every finite |det| >= floor: the x coordinate of a voxel whose cell reads closer to zero than that is moved
    by a hundredth of a voxel (which moves the determinant of its cell by about as much), until none is left.  A deterministic repair of
    a drawn input, so that no sign depends on a last bit."""
    phi = phi.copy()
    W = phi.shape[3]
    for _ in range(rounds):
        det = det_ref(phi)
        with np.errstate(invalid="ignore"):
            z, y, x = np.nonzero(np.abs(det) < floor)
        if not len(z):
            return phi, det
        phi[2, z + 1, y + 1, x + 1] += np.float32(0.01 / (W - 1))
    raise AssertionError("clear_of_zero did not converge")


STRETCH = (1.1, 0.8, 1.25)                # along z, y, x (phi channel order): det = 1.1


def stretch_phi(shape) -> np.ndarray:
    """An axis-aligned stretch about the centre: channel k = 0.5 + s_k * (identity_k - 0.5), in float32."""
    phi = ref.identity_phi(shape)
    for k, s in enumerate(STRETCH):
        phi[k] = (np.float32(0.5) + np.float32(s) * (phi[k] - np.float32(0.5))).astype(np.float32)
    return phi


def stretch_tolerance(shape) -> float:
    """Bound of |det - 1.1| for ``stretch_phi``, from float32 epsilon x the rebuild's magnitude.  Channel k depends on its own index
    alone, so the off-diagonal differences are exactly zero and det = J_zz J_yy J_xx.  Per axis, with n - 1 steps: a value of the stretched
    map carries up to three float32 roundings of numbers below 1.25, at most 1.5 eps in all, and the subtraction of the identity one more
    half eps of a number below 0.125: 1.6 eps, times (n - 1) in voxels; the product by (n - 1) adds eps/2 x |u| with |u| <= |s - 1| (n - 1) / 2;
    the identity's own rounding moves the exact difference by |s - 1| eps (n - 1) / 2.  A diagonal entry is a difference of two such values."""
    err = []
    for n, s in zip(shape, STRETCH):
        point = 1.6 * EPS32 * (n - 1) + 0.5 * EPS32 * abs(s - 1) * (n - 1) / 2
        err.append(2 * point + abs(s - 1) * EPS32 * (n - 1) / 2)
    sz, sy, sx = STRETCH
    return err[0] * sy * sx + err[1] * sz * sx + err[2] * sz * sy
