"""fp64 restatement of the point transform through phi (csrc/mesh_transform.hip, mesh_processing.transform_mesh); numpy only.

TEST INFRASTRUCTURE.  *** PARITY UNPINNED ***: the reference would push a mesh with ``itk.transform_mesh_filter`` and the registration's
CompositeTransform; ITK is not installed, so this restates ITK's documented behaviour exactly as oracle/resample.py does for the
resample (whose pieces it reuses): B point -> network index space -> + linearly interpolated displacement inside the field's buffer
([-0.5, n - 0.5) per axis), identity outside -> A point.

``transform_points_ref`` takes the two composed affines the kernel takes and performs the kernel's operations in its order (the affine
rows left to right, the lerp of ``_trilinear_clamped``), so the only difference left to a float32 result is its last rounding.
``point_chain_ref`` walks the chain leg by leg from the images' geometry, without composing anything: the check of mesh_point_affines.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.icon import displacement_itk, identity_map, network_affine
from oracle.resample import _trilinear_clamped

COORDS = ("spacing", "physical")


def identity_phi(net_shape) -> np.ndarray:
    """float32 [3,D,H,W]: the map whose displacement is exactly zero."""
    return identity_map(tuple(int(v) for v in net_shape))[0].numpy().copy()


def random_phi(net_shape, rng, amplitude: float = 0.2) -> np.ndarray:
    """identity_map + uniform(-amplitude, amplitude), float32 [3,D,H,W]."""
    ident = identity_phi(net_shape)
    return (ident + rng.uniform(-amplitude, amplitude, size=ident.shape).astype(np.float32)).astype(np.float32)


def displacement(phi: np.ndarray) -> np.ndarray:
    """float64 [D,H,W,3], xyz components, network voxel units: fp32 (phi - identity) * (n - 1), widened."""
    return displacement_itk(torch.from_numpy(np.ascontiguousarray(phi, dtype=np.float32))[None])


def apply_affine(Ab, p: np.ndarray) -> np.ndarray:
    """A @ p + b per row of p [n,3], each row's sum left to right as the kernel writes it (no BLAS, no fused multiply-add)."""
    A, b = np.asarray(Ab[0], np.float64).reshape(3, 3), np.asarray(Ab[1], np.float64).reshape(3)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    return np.stack([A[r, 0] * p[:, 0] + A[r, 1] * p[:, 1] + A[r, 2] * p[:, 2] + b[r] for r in range(3)], axis=1)


def inside_buffer(x: np.ndarray, net_shape) -> np.ndarray:
    Dn, Hn, Wn = (int(v) for v in net_shape)
    return ((x[:, 0] >= -0.5) & (x[:, 0] < Wn - 0.5) & (x[:, 1] >= -0.5) & (x[:, 1] < Hn - 0.5) & (x[:, 2] >= -0.5) & (x[:, 2] < Dn - 0.5))


def face_margin(x: np.ndarray, net_shape) -> np.ndarray:
    """Per point, the smallest distance (network voxels) of a coordinate to one of the buffer's +-0.5 faces."""
    Dn, Hn, Wn = (int(v) for v in net_shape)
    n = np.array([Wn, Hn, Dn], np.float64)
    return np.minimum(np.abs(x + 0.5), np.abs(x - (n - 0.5))).min(axis=1) if len(x) else np.zeros(0)


def transform_points_ref(points: np.ndarray, phi: np.ndarray, point_to_net, net_to_out):
    """(out float64 [n,3], inside bool [n], x float64 [n,3] network coordinates) for float32 points [n,3]."""
    x = apply_affine(point_to_net, np.asarray(points, np.float32).astype(np.float64))
    inside = inside_buffer(x, phi.shape[1:])
    d = _trilinear_clamped(displacement(phi), x[:, 0], x[:, 1], x[:, 2]) if len(x) else np.zeros((0, 3))
    x2 = x + np.where(inside[:, None], d, 0.0)
    return apply_affine(net_to_out, x2), inside, x


def _to_index(points, img, coords):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if coords == "spacing":
        return p / img.spacing
    return (p - img.origin) @ np.linalg.inv(img.direction @ np.diag(img.spacing)).T


def _from_index(idx, img, coords):
    if coords == "spacing":
        return idx * img.spacing
    return idx @ (img.direction @ np.diag(img.spacing)).T + img.origin


def net_to_physical(x_net: np.ndarray, img, net_shape) -> np.ndarray:
    """``resampling_transform(image, shape)``: network index space -> the image's physical space."""
    M, c_net, c_img = network_affine(img.spacing, img.origin, img.direction, img.size_xyz, tuple(net_shape))
    return (np.asarray(x_net, np.float64) - c_net) @ M.T + c_img


def point_chain_ref(points, disp, net_shape, meta_A, meta_B, coords_in="spacing", coords_out="spacing"):
    """The chain leg by leg, nothing composed: coords_in -> B index -> B physical -> network index space -> + displacement (``disp``
    float64 [D,H,W,3] on ``net_shape``, or None for zero) -> A physical -> A continuous index -> coords_out.  Returns (out, x_net, inside)."""
    M_B, c_net, c_B = network_affine(meta_B.spacing, meta_B.origin, meta_B.direction, meta_B.size_xyz, tuple(net_shape))
    p_B = _from_index(_to_index(points, meta_B, coords_in), meta_B, "physical")
    x = (p_B - c_B) @ np.linalg.inv(M_B).T + c_net
    inside = inside_buffer(x, net_shape)
    d = np.zeros_like(x) if disp is None else _trilinear_clamped(disp, x[:, 0], x[:, 1], x[:, 2])
    q = net_to_physical(x + np.where(inside[:, None], d, 0.0), meta_A, net_shape)
    return _from_index(_to_index(q, meta_A, "physical"), meta_A, coords_out), x, inside
