"""Tensor-level wrappers over the C ABI (torch is plumbing: device memory + the current stream).

Every function takes contiguous fp32 ``torch`` tensors on the HIP device, passes ``data_ptr()``
to liboai_hip.so through ``_lib.call`` -- which makes the named device (the one the output is
allocated on) current and fills in its current stream where ``_lib.STREAM`` stands -- and returns
the output tensor.  No torch compute op is used on the product path.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib


def _chk(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.OaiError(f"{name} must live on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.OaiError(f"{name} must be {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


check_tensor = _chk          # for the package's other modules (qc.py)


def _ptr(t: Optional[torch.Tensor], n: int = 1):
    """What the C ABI takes for an optional tensor: its address, or NULL for an absent one and for every tensor of a call over
    ``n`` = 0 elements."""
    return t.data_ptr() if (t is not None and n) else None


def _is_phi(t: torch.Tensor) -> bool:
    return t.dim() == 4 and t.shape[0] == 3


def _check_phi(phi: torch.Tensor) -> None:
    if not _is_phi(phi):
        raise ValueError(f"phi must be [3,D,H,W], got {tuple(phi.shape)}")


def _check_points(points: torch.Tensor) -> None:
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [n,3], got {tuple(points.shape)}")


def _check_same_gpu(name_a: str, a: torch.Tensor, name_b: str, b: torch.Tensor) -> None:
    if b.device != a.device:
        raise ValueError(f"{name_a} ({a.device}) and {name_b} ({b.device}) must live on the same GPU")


def warp_set_option(name: str, value: int) -> None:
    """Process-wide tuning option of the warp kernels (include/oai_hip.h: oai_warp_set_option): "brick" 0|1 -- grid_sample3d / compose through
    the LDS-staged brick kernel; bit-identical outputs."""
    _lib.call("oai_warp_set_option", name.encode(), int(value))


def grid_sample3d(src: torch.Tensor, coords: Optional[torch.Tensor], out_shape: Optional[Sequence[int]] = None) -> torch.Tensor:
    """src [C,d,h,w], coords [3,D,H,W] in [0,1] (None = identity of out_shape) -> [C,D,H,W]."""
    src = _chk(src, "src")
    Cn, d, h, w = src.shape
    if coords is not None:
        coords = _chk(coords, "coords")
        D, H, W = coords.shape[1:]
    else:
        D, H, W = out_shape
    out = torch.empty((Cn, D, H, W), dtype=torch.float32, device=src.device)
    _lib.call("oai_grid_sample3d", src.data_ptr(), Cn, d, h, w, _ptr(coords), D, H, W, out.data_ptr(), _lib.STREAM, device=src.device)
    return out


def compose(disp: torch.Tensor, coords: Optional[torch.Tensor], out_shape: Optional[Sequence[int]] = None,
            shortcut: bool = True) -> torch.Tensor:
    """coords + sample(disp, coords); coords None = identity map of out_shape (or of disp's grid)."""
    disp = _chk(disp, "disp")
    _, d, h, w = disp.shape
    if coords is not None:
        coords = _chk(coords, "coords")
        D, H, W = coords.shape[1:]
    else:
        D, H, W = out_shape if out_shape is not None else (d, h, w)
    out = torch.empty((3, D, H, W), dtype=torch.float32, device=disp.device)
    _lib.call("oai_compose", disp.data_ptr(), d, h, w, _ptr(coords), D, H, W, int(shortcut), out.data_ptr(), _lib.STREAM, device=disp.device)
    return out


def warp_chain(out_shape: Sequence[int], fields: Sequence[torch.Tensor] = (), start: Optional[torch.Tensor] = None,
               image: Optional[torch.Tensor] = None) -> torch.Tensor:
    """c = identity(out_shape) [+ start]; c = c + sample(f, c) for f in fields (<= 8 = OAI_WARP_CHAIN_MAX_FIELDS); returns sample(image, c) [D,H,W] when an
    image [d,h,w] is given, else c [3,D,H,W].  One launch, bit-identical to the compose / grid_sample3d calls it replaces."""
    D, H, W = (int(v) for v in out_shape)
    fields = [_chk(f, "field") for f in fields]
    if len(fields) > 8 or not all(_is_phi(f) for f in fields):
        raise ValueError("at most eight fields, each [3,d,h,w]")
    dev = (fields[0] if fields else start if start is not None else image).device
    if start is not None:
        start = _chk(start, "start")
        if tuple(start.shape) != (3, D, H, W):
            raise ValueError("start must be [3,D,H,W] on the output grid")
    if image is not None:
        image = _chk(image, "image")
        if image.dim() != 3:
            raise ValueError("image must be [d,h,w]")
    ptrs = (C.c_void_p * max(1, len(fields)))(*[f.data_ptr() for f in fields])
    dims = (C.c_int * max(3, 3 * len(fields)))(*[int(v) for f in fields for v in f.shape[1:]])
    out = torch.empty((D, H, W) if image is not None else (3, D, H, W), dtype=torch.float32, device=dev)
    idims = tuple(image.shape) if image is not None else (0, 0, 0)
    _lib.call("oai_warp_chain", _ptr(start), D, H, W, len(fields), ptrs, dims, _ptr(image), *idims, out.data_ptr(), _lib.STREAM, device=dev)
    return out


def avgpool2(x: torch.Tensor) -> torch.Tensor:
    x = _chk(x, "x")
    Cn, D, H, W = x.shape
    out = torch.empty((Cn, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=x.device)
    _lib.call("oai_avgpool2_3d", x.data_ptr(), Cn, D, H, W, out.data_ptr(), _lib.STREAM, device=x.device)
    return out


def resize_trilinear(x: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    x = _chk(x, "x")
    Cn, d, h, w = x.shape
    D, H, W = (int(v) for v in size)
    out = torch.empty((Cn, D, H, W), dtype=torch.float32, device=x.device)
    _lib.call("oai_resize_trilinear", x.data_ptr(), Cn, d, h, w, out.data_ptr(), D, H, W, _lib.STREAM, device=x.device)
    return out


def phi_to_itk_displacement(phi: torch.Tensor) -> torch.Tensor:
    """phi [3,D,H,W] -> float64 [D,H,W,3] (xyz components, network voxel units)."""
    phi = _chk(phi, "phi")
    _, D, H, W = phi.shape
    out = torch.empty((D, H, W, 3), dtype=torch.float64, device=phi.device)
    _lib.call("oai_phi_to_itk_displacement", phi.data_ptr(), D, H, W, out.data_ptr(), _lib.STREAM, device=phi.device)
    return out


def make_affine(A: np.ndarray, b: np.ndarray) -> _lib.Affine:
    a = _lib.Affine()
    a.A[:] = [float(v) for v in np.asarray(A, np.float64).reshape(9)]
    a.b[:] = [float(v) for v in np.asarray(b, np.float64).reshape(3)]
    return a


def resample_through_disp(prob: torch.Tensor, disp: torch.Tensor, b_index_to_net, net_to_a_index,
                          out_shape_zyx: Sequence[int]) -> torch.Tensor:
    prob = _chk(prob, "prob")
    disp = _chk(disp, "disp", torch.float64)
    nzA, nyA, nxA = prob.shape
    Dn, Hn, Wn, _ = disp.shape
    nzB, nyB, nxB = (int(v) for v in out_shape_zyx)
    out = torch.empty((nzB, nyB, nxB), dtype=torch.float32, device=prob.device)
    a1, a2 = make_affine(*b_index_to_net), make_affine(*net_to_a_index)
    _lib.call("oai_resample_through_disp", prob.data_ptr(), nzA, nyA, nxA, disp.data_ptr(), Dn, Hn, Wn, C.byref(a1), C.byref(a2), out.data_ptr(),
              nzB, nyB, nxB, _lib.STREAM, device=prob.device)
    return out


def resample_maps_through_phi(maps: torch.Tensor, phi: torch.Tensor, b_index_to_net, net_to_a_index,
                              out_shape_zyx: Sequence[int]) -> torch.Tensor:
    """maps [n,zA,yA,xA] (n <= 4) pulled through the dense map phi [3,D,H,W] onto a grid of ``out_shape_zyx``: one launch,
    bit-identical to ``phi_to_itk_displacement`` + ``resample_through_disp`` per map."""
    maps = _chk(maps, "maps")
    phi = _chk(phi, "phi")
    if maps.dim() != 4 or not _is_phi(phi):
        raise ValueError("maps must be [n,z,y,x] and phi [3,D,H,W]")
    n, nzA, nyA, nxA = maps.shape
    _, Dn, Hn, Wn = phi.shape
    nzB, nyB, nxB = (int(v) for v in out_shape_zyx)
    out = torch.empty((n, nzB, nyB, nxB), dtype=torch.float32, device=maps.device)
    a1, a2 = make_affine(*b_index_to_net), make_affine(*net_to_a_index)
    _lib.call("oai_resample_maps_through_phi", maps.data_ptr(), n, nzA, nyA, nxA, phi.data_ptr(), Dn, Hn, Wn, C.byref(a1), C.byref(a2),
              out.data_ptr(), nzB, nyB, nxB, _lib.STREAM, device=maps.device)
    return out


def transform_points_through_phi(points: torch.Tensor, phi: torch.Tensor, point_to_net, net_to_out, return_inside: bool = False):
    """points float32 [n,3] (x,y,z) pushed through the dense map phi [3,D,H,W]: ``net_to_out(x + displacement(x))`` with
    ``x = point_to_net(p)``, the displacement trilinear inside phi's buffer and zero outside it (include/oai_hip.h, "Points pushed
    through phi").  The affines are (A [3,3], b [3]) pairs in fp64.  Returns float32 [n,3]; with ``return_inside`` also the uint8 [n]
    mask of the points that lay inside the buffer."""
    points = _chk(points, "points")
    phi = _chk(phi, "phi")
    _check_points(points)
    _check_phi(phi)
    _check_same_gpu("points", points, "phi", phi)
    n = int(points.shape[0])
    _, Dn, Hn, Wn = (int(v) for v in phi.shape)
    out = torch.empty((n, 3), dtype=torch.float32, device=points.device)
    inside = torch.empty(n, dtype=torch.uint8, device=points.device) if return_inside else None
    a1, a2 = make_affine(*point_to_net), make_affine(*net_to_out)
    _lib.call("oai_transform_points_through_phi", points.data_ptr(), n, phi.data_ptr(), Dn, Hn, Wn, C.byref(a1), C.byref(a2), out.data_ptr(),
              _ptr(inside), _lib.STREAM, device=points.device)
    return (out, inside) if return_inside else out


@dataclass
class PhiInverseStats:
    """What the solver behind ``invert_phi`` did over the lattice (include/oai_hip.h, "The inverse of phi")."""
    points: int                 # lattice points D * H * W
    unconverged: int            # status 0: left at their identity coordinate
    outside: int                # status 2: converged at a point outside phi's buffer, where the forward map is the identity
    max_residual: float         # max |T(x) - y| over the converged points, network voxels
    mean_iterations: float      # evaluations of the forward map per point
    max_iterations: int


def _check_solver(max_iter, tol) -> None:
    if int(max_iter) < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter}")
    if not float(tol) > 0.0:
        raise ValueError(f"tol must be positive, got {tol}")


def inverse_points_through_phi(points: torch.Tensor, phi: torch.Tensor, point_to_net, net_to_out, max_iter: int = 30, tol: float = 1e-7,
                               return_status: bool = False):
    """points float32 [n,3] (x,y,z) pulled back through the dense map phi [3,D,H,W]: ``net_to_out(x)`` with ``T(x) = point_to_net(p)``,
    T the forward map of ``transform_points_through_phi`` in network index space, solved per point by Newton's method to ``tol``
    network voxels in at most ``max_iter`` iterations (include/oai_hip.h, "The inverse of phi").  The affines are (A [3,3], b [3])
    pairs in fp64.  Returns float32 [n,3]; with ``return_status`` also the uint8 [n] status: 1 = converged inside phi's buffer, 2 =
    converged outside it, 0 = not converged (the point is then moved by the affines alone)."""
    points = _chk(points, "points")
    phi = _chk(phi, "phi")
    _check_points(points)
    _check_phi(phi)
    _check_same_gpu("points", points, "phi", phi)
    _check_solver(max_iter, tol)
    n = int(points.shape[0])
    _, Dn, Hn, Wn = (int(v) for v in phi.shape)
    out = torch.empty((n, 3), dtype=torch.float32, device=points.device)
    status = torch.empty(n, dtype=torch.uint8, device=points.device) if return_status else None
    a1, a2 = make_affine(*point_to_net), make_affine(*net_to_out)
    _lib.call("oai_inverse_points_through_phi", points.data_ptr(), n, phi.data_ptr(), Dn, Hn, Wn, C.byref(a1), C.byref(a2), int(max_iter),
              float(tol), out.data_ptr(), _ptr(status), _lib.STREAM, device=points.device)
    return (out, status) if return_status else out


def invert_phi(phi: torch.Tensor, max_iter: int = 30, tol: float = 1e-7, return_status: bool = False, out: Optional[torch.Tensor] = None):
    """The dense inverse psi of the dense map phi float32 [3,D,H,W] on the same lattice and in the same storage convention: psi is a
    phi (``resample_maps_through_phi``, ``transform_points_through_phi`` and ``phi_jacobian`` read it unchanged) that takes patient
    points to atlas points (include/oai_hip.h, "The inverse of phi").  Returns ``(psi, stats)`` -- psi a new float32 [3,D,H,W] device
    tensor, or ``out``; stats a ``PhiInverseStats``, read back with one synchronisation -- and with ``return_status`` also the uint8
    [D,H,W] status of every lattice point (1 converged inside the buffer, 2 converged outside it, 0 not converged)."""
    phi = _chk(phi, "phi")
    _check_phi(phi)
    _check_solver(max_iter, tol)
    _, D, H, W = (int(v) for v in phi.shape)
    if out is None:
        psi = torch.empty_like(phi)
    else:
        if out.device != phi.device or out.dtype != torch.float32 or tuple(out.shape) != tuple(phi.shape) or not out.is_contiguous() \
                or out.data_ptr() == phi.data_ptr():
            raise ValueError(f"out must be a contiguous float32 {tuple(phi.shape)} tensor on {phi.device} that is not phi itself")
        psi = out
    status = torch.empty((D, H, W), dtype=torch.uint8, device=phi.device) if return_status else None
    stats = torch.empty(6, dtype=torch.float64, device=phi.device)
    ws = _lib.workspace("oai_invert_phi", phi.device, D, H, W)
    _lib.call("oai_invert_phi", phi.data_ptr(), D, H, W, int(max_iter), float(tol), psi.data_ptr(), _ptr(status), ws.data_ptr(), ws.numel(),
              stats.data_ptr(), _lib.STREAM, device=phi.device)
    s = stats.cpu().numpy()
    record = PhiInverseStats(int(s[0]), int(s[1]), int(s[2]), float(s[3]), float(s[4] / s[0]), int(s[5]))
    return (psi, record, status) if return_status else (psi, record)


def _out_slot(out: Optional[torch.Tensor], n: int, dtype, device, name: str) -> torch.Tensor:
    """The small device result of a QC entry point: a fresh tensor, or the caller's slot of a buffer that is downloaded in one piece."""
    if out is None:
        return torch.empty(n, dtype=dtype, device=device)
    if out.device != device or out.dtype != dtype or tuple(out.shape) != (n,) or not out.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} [{n}] tensor on {device}")
    return out


def phi_jacobian(phi: torch.Tensor, return_map: bool = False, out: Optional[torch.Tensor] = None):
    """The Jacobian determinant of the dense map phi float32 [3,D,H,W] per cell (z,y,x) in [1,D) x [1,H) x [1,W), backward differences of
    the displacement in network voxels (include/oai_hip.h, "Registration QC").  Returns the float64 [7] DEVICE tensor (cells, folds,
    non-finite cells, min, max, sum, sum of squares; ``out``: written there instead of a new tensor); with ``return_map`` also the
    float32 [D-1,H-1,W-1] map.  Does not synchronise: read the stats when they are needed (qc.registration_qc does, once)."""
    phi = _chk(phi, "phi")
    _check_phi(phi)
    _, D, H, W = (int(v) for v in phi.shape)
    stats = _out_slot(out, 7, torch.float64, phi.device, "out")
    det = torch.empty((max(D - 1, 0), max(H - 1, 0), max(W - 1, 0)), dtype=torch.float32, device=phi.device) if return_map else None
    ws = _lib.workspace("oai_phi_jacobian", phi.device, D, H, W)
    _lib.call("oai_phi_jacobian", phi.data_ptr(), D, H, W, _ptr(det), ws.data_ptr(), ws.numel(), stats.data_ptr(), _lib.STREAM, device=phi.device)
    return (stats, det) if return_map else stats


def mask_overlap(a: torch.Tensor, b: Optional[torch.Tensor] = None, threshold: float = 0.5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Overlap counts of two float32 device tensors of equal size under ``value > threshold`` (a non-finite value is in no set): the
    int64 [4] DEVICE tensor |A|, |B|, |A and B|, positions with a non-finite value.  ``b`` None: |A| and zeros.  Exact; does not
    synchronise."""
    a = _chk(a, "a")
    if b is not None:
        b = _chk(b, "b")
        if b.numel() != a.numel():
            raise ValueError(f"a and b must have the same number of elements, got {a.numel()} and {b.numel()}")
        _check_same_gpu("a", a, "b", b)
    n = int(a.numel())
    counts = _out_slot(out, 4, torch.int64, a.device, "out")
    ws = _lib.workspace("oai_mask_overlap", a.device, n)
    _lib.call("oai_mask_overlap", _ptr(a, n), _ptr(b, n), n, float(threshold), _ptr(ws, n), ws.numel(), counts.data_ptr(), _lib.STREAM,
              device=a.device)
    return counts


def image_normalize(vol: torch.Tensor, window_min_perc: float = 0.1, window_max_perc: float = 99.9,
                    output_min: float = 0.0, output_max: float = 1.0, return_window: bool = False):
    """``image_normalize`` of oai_analysis/dask_processing.py:10-26 on the device (fp32 image)."""
    vol = _chk(vol, "vol")
    out = torch.empty_like(vol)
    ws = _lib.workspace("oai_image_normalize", vol.device)
    win = torch.empty(2, dtype=torch.float32, device=vol.device)
    _lib.call("oai_image_normalize", vol.data_ptr(), vol.numel(), float(window_min_perc), float(window_max_perc), float(output_min),
              float(output_max), out.data_ptr(), win.data_ptr(), ws.data_ptr(), ws.numel(), _lib.STREAM, device=vol.device)
    return (out, win) if return_window else out


# ---- surface-distance QC (include/oai_hip.h, "Surface-distance QC"; csrc/edt.hip) --------------------------------------------------------
SURFACE_MODES = {"set": 0, "surface": 1, "complement": 2}


def _volume3(t: torch.Tensor, name: str, dtype) -> torch.Tensor:
    t = _chk(t, name, dtype)
    if t.dim() != 3:
        raise ValueError(f"{name} must be a [z,y,x] volume, got shape {tuple(t.shape)}")
    return t


def mask_surface(map: torch.Tensor, threshold: float = 0.5, mode: str = "surface") -> torch.Tensor:
    """The set ``finite and > threshold`` of a float32 [z,y,x] device volume as a uint8 volume: ``mode`` "set" -- the set itself;
    "surface" -- its voxels with a face neighbour outside the set or outside the volume (``A ^ binary_erosion(A)``, MedPy's rule);
    "complement" -- everything else.  Does not synchronise."""
    if mode not in SURFACE_MODES:
        raise ValueError(f"mode must be one of {sorted(SURFACE_MODES)}, got {mode!r}")
    map = _volume3(map, "map", torch.float32)
    D, H, W = (int(v) for v in map.shape)
    out = torch.empty((D, H, W), dtype=torch.uint8, device=map.device)
    _lib.call("oai_mask_surface", map.data_ptr(), D, H, W, float(threshold), SURFACE_MODES[mode], out.data_ptr(), _lib.STREAM, device=map.device)
    return out


def _edt(features: torch.Tensor, spacing_xyz, scale: float, into: Optional[torch.Tensor], squared: bool, count: bool):
    """One oai_edt call: (dist, sq or None, n_features or None).  ``into``: the float32 map that ``scale * distance`` is added to."""
    features = _volume3(features, "features", torch.uint8)
    D, H, W = (int(v) for v in features.shape)
    dist = torch.empty((D, H, W), dtype=torch.float32, device=features.device) if into is None else into
    sq = torch.empty((D, H, W), dtype=torch.float64, device=features.device) if squared else None
    n = torch.empty(1, dtype=torch.int64, device=features.device) if count else None
    ws = _lib.workspace("oai_edt", features.device, D, H, W)
    spacing = (C.c_double * 3)(*[float(v) for v in np.asarray(spacing_xyz, np.float64).reshape(3)])
    _lib.call("oai_edt", features.data_ptr(), D, H, W, spacing, float(scale), int(into is not None), dist.data_ptr(), _ptr(sq), ws.data_ptr(),
              ws.numel(), _ptr(n), _lib.STREAM, device=features.device)
    return dist, sq, n


def distance_transform(features: torch.Tensor, spacing_xyz=(1.0, 1.0, 1.0), return_squared: bool = False, return_count: bool = False):
    """The exact Euclidean distance transform of a uint8 [z,y,x] device volume: per voxel the distance to the nearest voxel with a
    non-zero byte, in the units of ``spacing_xyz`` (x, y, z) -- ``scipy.ndimage.distance_transform_edt(features == 0, sampling=
    spacing_xyz[::-1])``, +inf when there is no feature.  Returns the float32 map; with ``return_squared`` also the float64 squared
    distances (bit-equal to the brute-force minimum, include/oai_hip.h); with ``return_count`` also the int64 [1] DEVICE feature count.
    Does not synchronise."""
    dist, sq, n = _edt(features, spacing_xyz, 1.0, None, return_squared, return_count)
    got = (dist,) + ((sq,) if return_squared else ()) + ((n,) if return_count else ())
    return got if len(got) > 1 else dist


def signed_distance(map: torch.Tensor, spacing_xyz=(1.0, 1.0, 1.0), threshold: float = 0.5) -> torch.Tensor:
    """The signed distance map of the set ``finite and > threshold`` of a float32 [z,y,x] device volume: positive outside the set (the
    distance to it), negative inside (minus the distance to the complement) -- scipy's ``edt(~m) - edt(m)``.  Two oai_edt calls, the
    second subtracting in place.  Does not synchronise."""
    dist, _, _ = _edt(mask_surface(map, threshold, "set"), spacing_xyz, 1.0, None, False, False)
    _edt(mask_surface(map, threshold, "complement"), spacing_xyz, -1.0, dist, False, False)
    return dist


def surface_distance(surf_a: torch.Tensor, dist_to_b: torch.Tensor, surf_b: torch.Tensor, dist_to_a: torch.Tensor,
                     percentiles: Sequence[float] = (95.0,), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The surface-distance figures of two surfaces (uint8 masks) given each one's distance map (float32, ``distance_transform`` of the
    surface): the float64 [8] DEVICE tensor n_A, n_B, sum d(A->B), sum d(B->A), max d(A->B), max d(B->A) and up to two percentiles of
    the pooled distances (``np.percentile`` bit for bit; NaN where not asked for).  With an empty surface everything but the counts is
    NaN.  ``out``: written there instead of a new tensor.  Does not synchronise."""
    surf_a, surf_b = _chk(surf_a, "surf_a", torch.uint8), _chk(surf_b, "surf_b", torch.uint8)
    dist_to_b, dist_to_a = _chk(dist_to_b, "dist_to_b"), _chk(dist_to_a, "dist_to_a")
    n = int(surf_a.numel())
    for name, t in (("dist_to_b", dist_to_b), ("surf_b", surf_b), ("dist_to_a", dist_to_a)):
        if int(t.numel()) != n or t.device != surf_a.device:
            raise ValueError(f"{name} must have surf_a's {n} elements and live on its GPU")
    pct = [float(p) for p in percentiles]
    if len(pct) > 2:
        raise ValueError(f"at most two percentiles per call, got {len(pct)}")
    stats = _out_slot(out, 8, torch.float64, surf_a.device, "out")
    ws = _lib.workspace("oai_surface_distance", surf_a.device, n)
    _lib.call("oai_surface_distance", _ptr(surf_a, n), _ptr(dist_to_b, n), _ptr(surf_b, n), _ptr(dist_to_a, n), n,
              (C.c_float * 2)(*(pct + [0.0, 0.0])[:2]), len(pct), ws.data_ptr(), ws.numel(), stats.data_ptr(), _lib.STREAM, device=surf_a.device)
    return stats


# ---- image-similarity QC (include/oai_hip.h, "Image-similarity QC"; csrc/similarity.hip) -------------------------------------------------
def gaussian_taps(sigma: float):
    """(float64 [2 radius + 1] taps, radius) of the Gaussian that ``lncc`` filters with: ``radius = int(2 sigma)`` (4 sigma + 1 samples
    for an integer sigma, ICON's LNCC kernel as recalled), ``w_k = exp(-k^2 / (2 sigma^2))`` normalised to sum 1 in fp64.
    ``sigma <= 0``: the single tap 1.0."""
    sigma = float(sigma)
    if not sigma > 0.0:
        return np.ones(1, np.float64), 0
    radius = int(2.0 * sigma)
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / w.sum(), radius


def _pair(a: torch.Tensor, b: torch.Tensor, mask: Optional[torch.Tensor]):
    """a, b (float32) and the optional uint8 mask, contiguous, of one size on one GPU."""
    a, b = _chk(a, "a"), _chk(b, "b")
    if tuple(b.shape) != tuple(a.shape) or b.device != a.device:
        raise ValueError(f"a and b must share one shape and one GPU, got {tuple(a.shape)} on {a.device} and {tuple(b.shape)} on {b.device}")
    if mask is not None:
        mask = _chk(mask, "mask", torch.uint8)
        if tuple(mask.shape) != tuple(a.shape) or mask.device != a.device:
            raise ValueError(f"mask must have a's shape {tuple(a.shape)} and live on its GPU, got {tuple(mask.shape)} on {mask.device}")
    return a, b, mask


def image_moments(a: torch.Tensor, b: torch.Tensor, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The float64 [8] DEVICE tensor of two float32 device tensors of one shape: counted positions (admitted by the uint8 ``mask``, both
    values finite), admitted positions left out for a non-finite value, sum a, sum b, sum a^2, sum b^2, sum ab, sum (a - b)^2 -- fp64,
    bit-reproducible (include/oai_hip.h, "Image-similarity QC").  ``out``: written there instead of a new tensor.  Does not synchronise."""
    a, b, mask = _pair(a, b, mask)
    n = int(a.numel())
    stats = _out_slot(out, 8, torch.float64, a.device, "out")
    ws = _lib.workspace("oai_image_moments", a.device, n)
    _lib.call("oai_image_moments", _ptr(a, n), _ptr(b, n), n, _ptr(mask, n), _ptr(ws, n), ws.numel(), stats.data_ptr(), _lib.STREAM, device=a.device)
    return stats


def joint_histogram(a: torch.Tensor, b: torch.Tensor, bins: int = 64, range_a=(0.0, 1.0), range_b=(0.0, 1.0),
                    mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The int64 [bins*bins + 1] DEVICE tensor of two float32 device tensors of one shape: ``hist[ia*bins + ib]`` counts the pairs, the
    last entry the admitted positions skipped for a non-finite value.  Float32 binning with values outside a range clamped into the end
    bins (include/oai_hip.h).  Exact; ``out``: written there instead of a new tensor.  Does not synchronise."""
    a, b, mask = _pair(a, b, mask)
    n, bins = int(a.numel()), int(bins)
    if not 1 <= bins <= 128:
        raise ValueError(f"bins must be in [1, 128], got {bins}")
    hist = _out_slot(out, bins * bins + 1, torch.int64, a.device, "out")
    _lib.call("oai_joint_histogram", _ptr(a, n), _ptr(b, n), n, (C.c_float * 2)(*[float(v) for v in range_a]),
              (C.c_float * 2)(*[float(v) for v in range_b]), bins, _ptr(mask, n), hist.data_ptr(), _lib.STREAM, device=a.device)
    return hist


def histogram_entropies(hist: torch.Tensor, bins: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The float64 [4] DEVICE tensor N, H_A, H_B, H_AB (natural logarithm) of a ``joint_histogram`` table; N = 0 gives three NaNs.
    ``out``: written there instead of a new tensor.  Does not synchronise."""
    hist, bins = _chk(hist, "hist", torch.int64), int(bins)
    if not 1 <= bins <= 128 or int(hist.numel()) < bins * bins:
        raise ValueError(f"hist must hold bins*bins counts with bins in [1, 128], got {int(hist.numel())} entries for bins = {bins}")
    ent = _out_slot(out, 4, torch.float64, hist.device, "out")
    _lib.call("oai_histogram_entropies", hist.data_ptr(), bins, ent.data_ptr(), _lib.STREAM, device=hist.device)
    return ent


def lncc(a: torch.Tensor, b: torch.Tensor, sigma: float = 4.0, eps: float = 1e-5, mask: Optional[torch.Tensor] = None,
         return_map: bool = False, out: Optional[torch.Tensor] = None):
    """The local normalised cross-correlation of two float32 [z,y,x] device volumes under a Gaussian window (``gaussian_taps(sigma)``;
    sigma = 4 and eps = 1e-5 are ICON's values for the knee model, as recalled): the float64 [6] DEVICE tensor counted voxels, admitted
    voxels left out for a non-finite cc, sum cc, sum cc^2, min, max (include/oai_hip.h); with ``return_map`` also the float64 [z,y,x]
    map of cc.  The mean of cc is the network's similarity; its loss is one minus that.  ``out``: the stats are written there instead
    of a new tensor.  Does not synchronise."""
    a, b, mask = _pair(_volume3(a, "a", torch.float32), _volume3(b, "b", torch.float32), mask)
    D, H, W = (int(v) for v in a.shape)
    taps, radius = gaussian_taps(sigma)
    stats = _out_slot(out, 6, torch.float64, a.device, "out")
    cc = torch.empty((D, H, W), dtype=torch.float64, device=a.device) if return_map else None
    ws = _lib.workspace("oai_lncc", a.device, D, H, W)
    _lib.call("oai_lncc", a.data_ptr(), b.data_ptr(), D, H, W, (C.c_double * len(taps))(*taps.tolist()), radius, float(eps), _ptr(mask), _ptr(cc),
              ws.data_ptr(), ws.numel(), stats.data_ptr(), _lib.STREAM, device=a.device)
    return (stats, cc) if return_map else stats


# ---- segmentation-shape QC (include/oai_hip.h, "Segmentation-shape QC"; csrc/components.hip) ---------------------------------------------
SUMMARY_SLOTS = 12           # int64 per labelling call: include/oai_hip.h, oai_label_components


def label_components(map_or_mask: torch.Tensor, threshold: float = 0.5, connectivity: int = 26, complement: bool = False, min_voxels: int = 0,
                     return_labels: bool = True, return_sizes: bool = False, out: Optional[torch.Tensor] = None):
    """The connected components of a [z,y,x] device volume under 6, 18 or 26 connectivity.  A float32 tensor is a map: the set is
    ``finite and > threshold``; a uint8 or bool tensor is a mask: the set is ``!= 0``.  ``complement``: label what is NOT in the set.
    Returns ``(summary, labels, sizes)``: the int64 [12] DEVICE summary (voxels, voxels of the set, K, largest size, its label, second
    largest, components below ``min_voxels`` and their voxels, components touching the border and their voxels, non-finite positions,
    0; ``out``: written there instead of a new tensor); int32 labels, 0 off the set and 1..K in raster order of each component's first
    voxel -- ``scipy.ndimage.label`` to the element -- or None; the int32 per-voxel size of the voxel's component, or None.
    Deterministic; does not synchronise."""
    if map_or_mask.dtype == torch.bool:
        map_or_mask = map_or_mask.view(torch.uint8)
    if map_or_mask.dtype not in (torch.float32, torch.uint8):
        raise _lib.OaiError(f"map_or_mask must be float32 (a map) or uint8 / bool (a mask), got {map_or_mask.dtype}")
    is_map = map_or_mask.dtype == torch.float32
    vol = _volume3(map_or_mask, "map_or_mask", map_or_mask.dtype)
    D, H, W = (int(v) for v in vol.shape)
    summary = _out_slot(out, SUMMARY_SLOTS, torch.int64, vol.device, "out")
    labels = torch.empty((D, H, W), dtype=torch.int32, device=vol.device) if return_labels else None
    sizes = torch.empty((D, H, W), dtype=torch.int32, device=vol.device) if return_sizes else None
    ws = _lib.workspace("oai_label_components", vol.device, D, H, W)
    _lib.call("oai_label_components", vol.data_ptr() if is_map else None, None if is_map else vol.data_ptr(), D, H, W, float(threshold),
              int(bool(complement)), int(connectivity), int(min_voxels), _ptr(labels), _ptr(sizes), _ptr(ws, ws.numel()), ws.numel(),
              summary.data_ptr(), _lib.STREAM, device=vol.device)
    return summary, labels, sizes


def component_sizes(labels: torch.Tensor, n_components: int) -> torch.Tensor:
    """The int64 [n_components] DEVICE table of voxel counts per label 1..n_components of an int32 label volume (``np.bincount(labels)[1:]``);
    labels outside 0..n_components are ignored.  Does not synchronise."""
    labels = _chk(labels, "labels", torch.int32)
    k = int(n_components)
    if k < 0:
        raise ValueError(f"n_components must be >= 0, got {n_components}")
    n = int(labels.numel())
    sizes = (torch.empty if n else torch.zeros)(k, dtype=torch.int64, device=labels.device)     # the call clears the table unless it is a no-op
    _lib.call("oai_component_sizes", _ptr(labels, n), n, k, _ptr(sizes, k), _lib.STREAM, device=labels.device)
    return sizes


# ---- thickness QC (include/oai_hip.h, "Thickness QC"; csrc/local_thickness.hip) ----------------------------------------------------------
MAX_WINDOW_VOXELS = 262144   # 64^3: two orders of magnitude above a 6 mm cartilage at the DESS spacing (17 x 17 x 9 = 2601 voxels)
THICKNESS_SLOTS = 4          # int64 per oai_local_thickness call: centres, voxel tests, capped centres, the largest window
STATS_SLOTS = 8              # float64 per oai_masked_stats call


def local_thickness(rsq: torch.Tensor, spacing_xyz=(1.0, 1.0, 1.0), max_window_voxels: int = MAX_WINDOW_VOXELS, return_squared: bool = False,
                    return_stats: bool = False, out: Optional[torch.Tensor] = None):
    """The local thickness of a float64 [z,y,x] device field of squared radii (``distance_transform(complement, return_squared=True)``,
    or any other source): per centre -- a voxel whose entry is finite and > 0 -- twice the largest radius among the centres whose open
    ball contains it, in the units of ``spacing_xyz`` (x, y, z); 0 elsewhere.  Bit-identical to the brute force over all pairs
    (include/oai_hip.h).  Returns the float32 map; with ``return_squared`` also the float64 squared radii; with ``return_stats`` also the
    int64 [4] DEVICE tensor centres, voxel tests done, capped centres, the largest window (``out``: written there instead of a new
    tensor).  A centre whose clipped window holds more than ``max_window_voxels`` voxels covers only itself and is counted: a guard
    against a blob that fills the volume, not an accuracy knob.  Does not synchronise."""
    rsq = _volume3(rsq, "rsq", torch.float64)
    D, H, W = (int(v) for v in rsq.shape)
    thick = torch.empty((D, H, W), dtype=torch.float32, device=rsq.device)
    sq = torch.empty((D, H, W), dtype=torch.float64, device=rsq.device) if return_squared else None
    stats = _out_slot(out, THICKNESS_SLOTS, torch.int64, rsq.device, "out") if (return_stats or out is not None) else None
    ws = _lib.workspace("oai_local_thickness", rsq.device, D, H, W, pad=True)
    spacing = (C.c_double * 3)(*[float(v) for v in np.asarray(spacing_xyz, np.float64).reshape(3)])
    _lib.call("oai_local_thickness", rsq.data_ptr(), D, H, W, spacing, int(max_window_voxels), _ptr(sq), thick.data_ptr(), ws.data_ptr(), ws.numel(),
              _ptr(stats), _lib.STREAM, device=rsq.device)
    got = (thick,) + ((sq,) if return_squared else ()) + ((stats,) if return_stats else ())
    return got if len(got) > 1 else thick


def masked_stats(values: torch.Tensor, mask: Optional[torch.Tensor] = None, percentiles: Sequence[float] = (50.0, 95.0),
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The statistics of a float32 device tensor under a uint8 / bool mask of its shape (None: every element): the float64 [8] DEVICE
    tensor counted elements (admitted and finite), sum, sum of squares, min, max, up to two percentiles (``np.percentile`` of the
    counted values bit for bit; NaN where not asked for) and the admitted non-finite values.  With nothing counted the sums, the
    extremes and the percentiles are NaN.  fp64 sums in a fixed order: bit-reproducible (include/oai_hip.h, "Thickness QC").  ``out``:
    written there instead of a new tensor.  Does not synchronise."""
    values = _chk(values, "values")
    if mask is not None:
        mask = _chk(mask.view(torch.uint8) if mask.dtype == torch.bool else mask, "mask", torch.uint8)
        if tuple(mask.shape) != tuple(values.shape) or mask.device != values.device:
            raise ValueError(f"mask must have the values' shape {tuple(values.shape)} and live on their GPU, got {tuple(mask.shape)} on {mask.device}")
    pct = [float(p) for p in percentiles]
    if len(pct) > 2:
        raise ValueError(f"at most two percentiles per call, got {len(pct)}")
    n = int(values.numel())
    stats = _out_slot(out, STATS_SLOTS, torch.float64, values.device, "out")
    ws = _lib.workspace("oai_masked_stats", values.device, n)
    _lib.call("oai_masked_stats", _ptr(values, n), _ptr(mask, n), n, (C.c_float * 2)(*(pct + [0.0, 0.0])[:2]), len(pct), ws.data_ptr(), ws.numel(),
              stats.data_ptr(), _lib.STREAM, device=values.device)
    return stats


# ---- cartilage morphometry (include/oai_hip.h, "Cartilage morphometry"; csrc/morphometry.hip) ----------------------------------------------
REGION_SLOTS = 12            # float64 per region of oai_region_stats
MAX_REGIONS = 64


def region_stats(values: torch.Tensor, weights: torch.Tensor, labels: Optional[torch.Tensor] = None, covered: Optional[torch.Tensor] = None,
                 n_regions: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per region the twelve sums behind an area-weighted thickness summary: float32 ``values`` [n] and float64 ``weights`` [n] on the
    device, int32 ``labels`` [n] (None: every element in region 0; a label outside [0, n_regions) belongs to no region) and a uint8 /
    bool ``covered`` mask (None: every element).  An element is measured when it is covered and its value is finite.  Returns the float64
    [n_regions, 12] DEVICE tensor: elements, covered, measured; sum w over all, covered, measured; sum w t, sum (w t) t, min t, max t,
    sum t, sum t t over the measured elements.  An empty region reads 0, +inf for the minimum and -inf for the maximum.  fp64 sums in a
    fixed order: bit-reproducible (include/oai_hip.h).  ``out``: written there instead of a new tensor.  Does not synchronise."""
    values = _chk(values, "values").reshape(-1)
    n, R = int(values.numel()), int(n_regions)
    if not 1 <= R <= MAX_REGIONS:
        raise ValueError(f"n_regions must be in [1, {MAX_REGIONS}], got {n_regions}")
    weights = _chk(weights, "weights", torch.float64).reshape(-1)
    if labels is not None:
        labels = _chk(labels, "labels", torch.int32).reshape(-1)
    if covered is not None:
        covered = _chk(covered.view(torch.uint8) if covered.dtype == torch.bool else covered, "covered", torch.uint8).reshape(-1)
    for name, t in (("weights", weights), ("labels", labels), ("covered", covered)):
        if t is not None and (t.numel() != n or t.device != values.device):
            raise ValueError(f"{name} must have the values' {n} elements and live on their GPU, got {t.numel()} on {t.device}")
    stats = _out_slot(None if out is None else out.reshape(-1), R * REGION_SLOTS, torch.float64, values.device, "out")
    ws = _lib.workspace("oai_region_stats", values.device, n, R)
    _lib.call("oai_region_stats", _ptr(values, n), _ptr(weights, n), _ptr(labels, n), _ptr(covered, n), n, R, ws.data_ptr(), ws.numel(),
              stats.data_ptr(), _lib.STREAM, device=values.device)
    return stats.reshape(R, REGION_SLOTS)


# ---- cohort statistics (include/oai_hip.h, "Cohort statistics"; csrc/group_stats.hip) -----------------------------------------------------
STATS_TWO_SAMPLE, STATS_ONE_SAMPLE = 0, 1
OAI_TFCE_E_HALF, OAI_TFCE_E_ONE = 0, 1
OAI_TFCE_H_ONE, OAI_TFCE_H_TWO = 0, 1
TFCE_E_MODES = {0.5: OAI_TFCE_E_HALF, 1.0: OAI_TFCE_E_ONE}
TFCE_H_MODES = {1.0: OAI_TFCE_H_ONE, 2.0: OAI_TFCE_H_TWO}


@dataclass
class GroupPrepared:
    """The prepared block of ``group_prepare`` and views of its arrays (include/oai_hip.h states the layout): ``C``, ``Qm`` float64 [N,V];
    ``S``, ``Q``, ``mean``, ``std`` float64 [V]; ``n`` int32 [V].  ``mask``: the uint8 [N,V] mask it was prepared with, or None."""
    block: torch.Tensor
    n_knees: int
    n_verts: int
    centre: bool
    mask: Optional[torch.Tensor]
    C: torch.Tensor
    Qm: torch.Tensor
    S: torch.Tensor
    Q: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    n: torch.Tensor


def _block_views(block: torch.Tensor, layout) -> dict:
    """Views of the arrays of a prepared block: ``layout`` names them front to back as (name, dtype, shape), each starting on the next
    multiple of 256 bytes, as csrc/common.h hands a workspace out."""
    off, parts = 0, {}
    for name, dtype, shape in layout:
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        parts[name] = block[off:off + nbytes].view(dtype).reshape(shape)
        off += (nbytes + 255) // 256 * 256
    return parts


def _tile_workspace(workspace: Optional[torch.Tensor], need: int, device) -> torch.Tensor:
    """The caller's buffer for a t tile (reused between batches) once it is checked, or a new one of ``need`` bytes."""
    ws = torch.empty(need, dtype=torch.uint8, device=device) if workspace is None else workspace
    if ws.numel() < need or ws.device != device or ws.dtype != torch.uint8:
        raise ValueError(f"workspace must be a uint8 buffer of at least {need} bytes on {device}")
    return ws


def _graph_tile(values: torch.Tensor, offsets: torch.Tensor, neighbours: torch.Tensor):
    """What the graph kernels take: a float64 tile [R >= 1, V >= 1] and the int32 CSR adjacency of its V vertices on the same GPU.
    Returns (values, offsets, neighbours, R, V), the tensors contiguous."""
    values = _chk(values, "values", torch.float64)
    if values.dim() != 2 or values.shape[0] < 1 or values.shape[1] < 1:
        raise ValueError(f"values must be [R >= 1, V >= 1], got {tuple(values.shape)}")
    R, V = int(values.shape[0]), int(values.shape[1])
    offsets, neighbours = _chk(offsets, "offsets", torch.int32), _chk(neighbours, "neighbours", torch.int32)
    if offsets.numel() != V + 1 or offsets.device != values.device or neighbours.device != values.device:
        raise ValueError(f"offsets must be [{V + 1}] and live with neighbours on the values' GPU, got {offsets.numel()} on {offsets.device}")
    return values, offsets, neighbours, R, V


def _out_tile(out: Optional[torch.Tensor], name: str, dtype, values: torch.Tensor, may_alias: bool) -> torch.Tensor:
    """The caller's output tile of a graph kernel once it is checked -- contiguous, of ``dtype``, with the shape and GPU of ``values``
    and, unless the kernel ``may_alias`` its input, not ``values`` itself -- or a new one."""
    if out is None:
        return torch.empty(tuple(values.shape), dtype=dtype, device=values.device)
    if (out.device != values.device or out.dtype != dtype or tuple(out.shape) != tuple(values.shape) or not out.is_contiguous()
            or (not may_alias and out.data_ptr() == values.data_ptr())):
        raise ValueError(f"{name} must be a contiguous {str(dtype).split('.')[1]} [{values.shape[0]}, {values.shape[1]}] tensor on {values.device}"
                         + ("" if may_alias else " other than values"))
    return out


def _stats_mask(mask: Optional[torch.Tensor], like: torch.Tensor) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    mask = _chk(mask.view(torch.uint8) if mask.dtype == torch.bool else mask, "mask", torch.uint8)
    if tuple(mask.shape) != tuple(like.shape) or mask.device != like.device:
        raise ValueError(f"mask must have the values' shape {tuple(like.shape)} and live on their GPU, got {tuple(mask.shape)} on {mask.device}")
    return mask


def group_prepare(values: torch.Tensor, mask: Optional[torch.Tensor] = None, centre: bool = True) -> GroupPrepared:
    """What every permutation of a test re-sums, once per test: float32 ``values`` [N,V] (knee-major) and an optional uint8 / bool ``mask``
    [N,V] (non-zero: the knee has a value at the vertex) -> per vertex n, mean, std, and the values c (centred on the mean unless
    ``centre`` is False: the one-sample test's paired differences) with their squares and sums.  fp64, knees in ascending index:
    bit-reproducible (include/oai_hip.h).  Does not synchronise."""
    values = _chk(values, "values")
    if values.dim() != 2 or values.shape[0] < 2 or values.shape[1] < 1:
        raise ValueError(f"values must be [N >= 2, V >= 1], got {tuple(values.shape)}")
    mask = _stats_mask(mask, values)
    N, V = int(values.shape[0]), int(values.shape[1])
    block = _lib.workspace("oai_group_prepare", values.device, N, V)
    _lib.call("oai_group_prepare", values.data_ptr(), _ptr(mask), N, V, int(bool(centre)), block.data_ptr(), block.numel(), _lib.STREAM,
              device=values.device)
    parts = _block_views(block, (("C", torch.float64, (N, V)), ("Qm", torch.float64, (N, V)), ("S", torch.float64, (V,)), ("Q", torch.float64, (V,)),
                                 ("mean", torch.float64, (V,)), ("std", torch.float64, (V,)), ("n", torch.int32, (V,))))
    return GroupPrepared(block, N, V, bool(centre), mask, **parts)


def _check_bits(bits: torch.Tensor, n_knees: int) -> torch.Tensor:
    bits = _chk(bits.view(torch.int32) if bits.dtype == torch.uint32 else bits, "bits", torch.int32)
    if bits.dim() != 2 or bits.shape[1] != (n_knees + 31) // 32:
        raise ValueError(f"bits must be [P, {(n_knees + 31) // 32}] packed 32-bit words for {n_knees} knees, got {tuple(bits.shape)}")
    return bits


def permutation_t(prepared: GroupPrepared, bits: torch.Tensor, p0: int, p1: int, mode: int = STATS_TWO_SAMPLE,
                  workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The t tile of the labellings [p0, p1) of ``bits`` (packed 32-bit words [P, ceil(N/32)] on the device, int32 or uint32 storage): float64
    [p1 - p0, V], NaN where no t exists.  ``mode`` STATS_TWO_SAMPLE: pooled t of the knees whose bit is set against the others;
    STATS_ONE_SAMPLE: t of the values with the sign of every set knee flipped (``prepared`` with ``centre=False``).  ``workspace``: a uint8
    device buffer to hold the tile (reused between batches) instead of a new one.  Does not synchronise."""
    bits = _check_bits(bits, prepared.n_knees)
    p0, p1 = int(p0), int(p1)
    if not 0 <= p0 < p1 <= bits.shape[0]:
        raise ValueError(f"rows [{p0}, {p1}) are not rows of the {bits.shape[0]} labellings")
    if mode not in (STATS_TWO_SAMPLE, STATS_ONE_SAMPLE):
        raise ValueError(f"mode must be STATS_TWO_SAMPLE or STATS_ONE_SAMPLE, got {mode!r}")
    if prepared.centre != (mode == STATS_TWO_SAMPLE):
        raise ValueError("the two-sample test needs group_prepare(centre=True), the one-sample test centre=False")
    dev, V = prepared.block.device, prepared.n_verts
    need = int(_lib.load().oai_permutation_t_workspace_bytes(p1 - p0, V))
    ws = _tile_workspace(workspace, need, dev)
    _lib.call("oai_permutation_t", prepared.block.data_ptr(), prepared.block.numel(), _ptr(prepared.mask), bits.data_ptr(), prepared.n_knees, V, p0, p1,
              int(mode), ws.data_ptr(), ws.numel(), _lib.STREAM, device=dev)
    return ws[:(p1 - p0) * V * 8].view(torch.float64).reshape(p1 - p0, V)


def permutation_reduce(tile: torch.Tensor, p0: int, t0: torch.Tensor, max_abs: torch.Tensor, exceed: torch.Tensor) -> None:
    """Fold the t tile of rows [p0, p0 + len(tile)) into the test's running results, all on the device: ``max_abs`` float64 [P] gets each
    row's max |t| (0.0 for a row without a valid t); ``exceed`` int64 [V] counts, per vertex, the rows with |t| >= |observed t|.  The
    batch with ``p0`` = 0 holds the observed labelling as its row 0: it writes ``t0`` float64 [V] and starts ``exceed``; later batches
    read ``t0`` and add.  Does not synchronise."""
    tile = _chk(tile, "tile", torch.float64)
    rows, V = int(tile.shape[0]), int(tile.shape[1])
    p0 = int(p0)
    t0, max_abs, exceed = _chk(t0, "t0", torch.float64), _chk(max_abs, "max_abs", torch.float64), _chk(exceed, "exceed", torch.int64)
    if tuple(t0.shape) != (V,) or tuple(exceed.shape) != (V,) or max_abs.dim() != 1 or not 0 <= p0 <= max_abs.numel() - rows:
        raise ValueError(f"t0 and exceed must be [{V}] and max_abs must hold rows [{p0}, {p0 + rows}), got {tuple(t0.shape)}, {tuple(exceed.shape)}, "
                         f"{tuple(max_abs.shape)}")
    ws = _lib.workspace("oai_permutation_reduce", tile.device, rows, V)
    _lib.call("oai_permutation_reduce", tile.data_ptr(), V, p0, p0 + rows, ws.data_ptr(), ws.numel(), t0.data_ptr(), max_abs.data_ptr(),
              exceed.data_ptr(), _lib.STREAM, device=tile.device)


def graph_clusters(values: torch.Tensor, offsets: torch.Tensor, neighbours: torch.Tensor, threshold: float, max_extent: Optional[torch.Tensor] = None,
                   return_labels: bool = False):
    """Per row of the float64 ``values`` [R,V], the connected components of {value > threshold} and of {value < -threshold} on the graph
    given as the CSR adjacency of ``mesh_processing.vertex_adjacency_device`` (int32 ``offsets`` [V+1], ``neighbours``).  Returns the int32
    [R] DEVICE tensor of each row's largest component (vertices; both signs; 0 if none; ``max_extent``: written there); with
    ``return_labels`` also row 0's int32 [V] labels (the component's smallest vertex index, -1 outside both sets) and per-vertex component
    sizes.  Integers only.  Does not synchronise."""
    values, offsets, neighbours, R, V = _graph_tile(values, offsets, neighbours)
    if not float(threshold) > 0.0:
        raise ValueError(f"threshold must be > 0, got {threshold!r}")
    ext = _out_slot(max_extent, R, torch.int32, values.device, "max_extent")
    label = torch.empty(V, dtype=torch.int32, device=values.device) if return_labels else None
    size = torch.empty(V, dtype=torch.int32, device=values.device) if return_labels else None
    ws = _lib.workspace("oai_graph_clusters", values.device, R, V)
    _lib.call("oai_graph_clusters", values.data_ptr(), R, V, offsets.data_ptr(), _ptr(neighbours, neighbours.numel()), int(neighbours.numel()),
              float(threshold), ws.data_ptr(), ws.numel(), ext.data_ptr(), _ptr(label), _ptr(size), _lib.STREAM, device=values.device)
    return (ext, label, size) if return_labels else ext


def graph_tfce(values: torch.Tensor, offsets: torch.Tensor, neighbours: torch.Tensor, dh: float = 0.1, E: float = 1.0, H: float = 2.0,
               weights: Optional[torch.Tensor] = None, unit: float = 1.0, max_steps: int = 1000, out: Optional[torch.Tensor] = None,
               clipped: Optional[torch.Tensor] = None):
    """Threshold-free cluster enhancement of every row of the float64 ``values`` [R,V] on the graph given as in ``graph_clusters``
    (include/oai_hip.h, "Threshold-free cluster enhancement"): per vertex the sum over the levels k * ``dh`` <= |value| of
    extent^E * level^H * dh, with the sign of the value.  The extent of a vertex at a level is the summed int64 ``weights`` [V] of its
    component times ``unit``, or the component's vertex count without weights.  E is 0.5 or 1, H is 1 or 2.  Returns the float64 [R,V]
    and int32 [R] DEVICE tensors (tfce, clipped): ``clipped`` counts the row's vertices whose |value| reaches past ``max_steps`` levels
    (``out``, ``clipped``: written there).  Bit-reproducible.  Does not synchronise."""
    values, offsets, neighbours, R, V = _graph_tile(values, offsets, neighbours)
    if float(E) not in TFCE_E_MODES or float(H) not in TFCE_H_MODES:
        raise ValueError(f"E must be 0.5 or 1 and H must be 1 or 2, got E = {E!r}, H = {H!r}")
    if not (float(dh) > 0.0 and math.isfinite(float(dh))):
        raise ValueError(f"dh must be finite and > 0, got {dh!r}")
    if not float(unit) > 0.0:
        raise ValueError(f"unit must be > 0, got {unit!r}")
    if not 1 <= int(max_steps) <= 65536:
        raise ValueError(f"max_steps must be 1 .. 65536, got {max_steps!r}")
    if weights is not None:
        weights = _chk(weights, "weights", torch.int64)
        if tuple(weights.shape) != (V,) or weights.device != values.device:
            raise ValueError(f"weights must be int64 [{V}] on the values' GPU, got {tuple(weights.shape)} on {weights.device}")
    out = _out_tile(out, "out", torch.float64, values, may_alias=False)
    clip = _out_slot(clipped, R, torch.int32, values.device, "clipped")
    ws = _lib.workspace("oai_graph_tfce", values.device, R, V)
    _lib.call("oai_graph_tfce", values.data_ptr(), R, V, offsets.data_ptr(), _ptr(neighbours, neighbours.numel()), int(neighbours.numel()),
              _ptr(weights), float(unit), float(dh), TFCE_E_MODES[float(E)], TFCE_H_MODES[float(H)], int(max_steps), ws.data_ptr(), ws.numel(),
              out.data_ptr(), clip.data_ptr(), _lib.STREAM, device=values.device)
    return out, clip


MAX_SMOOTH_SWEEPS = 4096


def graph_smooth(values: torch.Tensor, offsets: torch.Tensor, neighbours: torch.Tensor, edge_weights: torch.Tensor,
                 mask: Optional[torch.Tensor] = None, self_weights: Optional[torch.Tensor] = None, sweeps: int = 1, fill: bool = False,
                 out: Optional[torch.Tensor] = None, out_mask: Optional[torch.Tensor] = None):
    """``sweeps`` sweeps of normalised neighbourhood averaging of every row of the float64 ``values`` [R,V] on the graph given as in
    ``graph_clusters``, with the float64 ``edge_weights`` aligned with ``neighbours`` and the float64 ``self_weights`` [V] (None: 1.0)
    (include/oai_hip.h, "Surface smoothing").  ``mask`` uint8 / bool [R,V]: non-zero = the entry is valid (None: all are); an invalid entry
    is never read into a sum.  ``fill`` False: a missing entry stays missing; True: it takes the average of its valid neighbours, so the
    valid set grows by one ring per sweep.  Weights must be finite and >= 0: not checked.  Returns the float64 [R,V] and uint8 [R,V]
    DEVICE tensors (values, mask): +0.0 and 0 where the result is missing (``out``, ``out_mask``: written there; ``out`` may be
    ``values`` and ``out_mask`` may be ``mask``).  Bit-reproducible.  Does not synchronise."""
    values, offsets, neighbours, R, V = _graph_tile(values, offsets, neighbours)
    dev = values.device
    edge_weights = _chk(edge_weights, "edge_weights", torch.float64)
    if edge_weights.numel() != neighbours.numel() or edge_weights.device != dev:
        raise ValueError(f"edge_weights must be float64 [{neighbours.numel()}] on the values' GPU, got {tuple(edge_weights.shape)} on "
                         f"{edge_weights.device}")
    if self_weights is not None:
        self_weights = _chk(self_weights, "self_weights", torch.float64)
        if tuple(self_weights.shape) != (V,) or self_weights.device != dev:
            raise ValueError(f"self_weights must be float64 [{V}] on the values' GPU, got {tuple(self_weights.shape)} on {self_weights.device}")
    if not 1 <= int(sweeps) <= MAX_SMOOTH_SWEEPS:
        raise ValueError(f"sweeps must be 1 .. {MAX_SMOOTH_SWEEPS}, got {sweeps!r}")
    mask = _stats_mask(mask, values)
    out = _out_tile(out, "out", torch.float64, values, may_alias=True)
    out_mask = _out_tile(out_mask, "out_mask", torch.uint8, values, may_alias=True)
    ws = _lib.workspace("oai_graph_smooth", dev, R, V)
    n_nbrs = int(neighbours.numel())
    _lib.call("oai_graph_smooth", values.data_ptr(), _ptr(mask), R, V, offsets.data_ptr(), _ptr(neighbours, n_nbrs), n_nbrs,
              _ptr(edge_weights, n_nbrs), _ptr(self_weights), int(sweeps), int(bool(fill)), ws.data_ptr(), ws.numel(), out.data_ptr(),
              out_mask.data_ptr(), _lib.STREAM, device=dev)
    return out, out_mask


# ---- longitudinal change (include/oai_hip.h, "Longitudinal change"; csrc/visit_slopes.hip) --------------------------------------------------
SLOPE_OUTPUTS = ("rate", "avg", "fit_ref", "resid_sd", "n", "mask")
MAX_VISIT_ROWS = 1 << 24             # rows, subjects and slots of one oai_visit_slopes call


@dataclass
class VisitSlopes:
    """The per-subject line fits of ``visit_slopes``, device tensors [S, V] (None for an output that was not asked for): ``rate``, ``avg``,
    ``fit_ref``, ``resid_sd`` float64 -- +0.0 where ``mask`` is 0, ``resid_sd`` NaN where the fit rests on two visits; ``n`` int32, the
    visits with a value at the vertex, also where ``mask`` is 0; ``mask`` uint8, 1 where the fit exists."""
    rate: Optional[torch.Tensor] = None
    avg: Optional[torch.Tensor] = None
    fit_ref: Optional[torch.Tensor] = None
    resid_sd: Optional[torch.Tensor] = None
    n: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None
    min_visits: int = 2
    min_span: float = 0.0


def visit_slopes(values: torch.Tensor, offsets: torch.Tensor, rows: torch.Tensor, times: torch.Tensor, reference_time: torch.Tensor,
                 mask: Optional[torch.Tensor] = None, min_visits: int = 2, min_span: float = 0.0, want: Sequence[str] = SLOPE_OUTPUTS) -> VisitSlopes:
    """A straight line through every subject's visits at every vertex (include/oai_hip.h, "Longitudinal change"): float32 ``values`` [R,V],
    one row per knee and visit in any order, with an optional uint8 / bool ``mask`` [R,V] (non-zero: valid); subject s owns the slots
    ``offsets[s] .. offsets[s+1] - 1`` (int32 [S+1]) of ``rows`` (int32 [E]: the row of ``values``) and ``times`` (float64 [E]: years);
    ``reference_time`` float64 [S] is where ``fit_ref`` is evaluated.  A fit exists where at least ``min_visits`` (>= 2) visits are valid
    at the vertex, they are not all at one time, and they span at least ``min_span`` years.  ``want``: which of ``SLOPE_OUTPUTS`` are
    allocated and computed.  fp64, slots in ascending position: bit-reproducible.  Does not synchronise."""
    values = _chk(values, "values")
    if values.dim() != 2 or not 1 <= values.shape[0] <= MAX_VISIT_ROWS or values.shape[1] < 1:
        raise ValueError(f"values must be [1 <= R <= 2^24, V >= 1], got {tuple(values.shape)}")
    R, V, dev = int(values.shape[0]), int(values.shape[1]), values.device
    mask = _stats_mask(mask, values)
    offsets, rows = _chk(offsets, "offsets", torch.int32).reshape(-1), _chk(rows, "rows", torch.int32).reshape(-1)
    times, reference_time = _chk(times, "times", torch.float64).reshape(-1), _chk(reference_time, "reference_time", torch.float64).reshape(-1)
    S, E = int(offsets.numel()) - 1, int(rows.numel())
    if not 1 <= S <= MAX_VISIT_ROWS or E > MAX_VISIT_ROWS or times.numel() != E or reference_time.numel() != S:
        raise ValueError(f"offsets must hold S + 1 entries for 1 <= S <= 2^24 subjects, rows and times one entry per slot (at most 2^24) and "
                         f"reference_time S, got {offsets.numel()}, {E}, {times.numel()}, {reference_time.numel()}")
    for name, t in (("offsets", offsets), ("rows", rows), ("times", times), ("reference_time", reference_time)):
        _check_same_gpu("values", values, name, t)
    if int(min_visits) < 2:
        raise ValueError(f"min_visits must be at least 2, got {min_visits!r}")
    if not (float(min_span) >= 0.0 and math.isfinite(float(min_span))):
        raise ValueError(f"min_span must be finite and >= 0, got {min_span!r}")
    want = tuple(want)
    if not want or len(set(want)) != len(want) or not set(want) <= set(SLOPE_OUTPUTS):
        raise ValueError(f"want must name some of {SLOPE_OUTPUTS}, each once, got {want!r}")
    dtypes = {"n": torch.int32, "mask": torch.uint8}
    out = {name: torch.empty((S, V), dtype=dtypes.get(name, torch.float64), device=dev) for name in want}
    ws = _lib.workspace("oai_visit_slopes", dev, R, V, S, E)
    _lib.call("oai_visit_slopes", values.data_ptr(), _ptr(mask), R, V, offsets.data_ptr(), S, _ptr(rows, E), _ptr(times, E), E,
              reference_time.data_ptr(), int(min_visits), float(min_span), ws.data_ptr(), ws.numel(),
              *[_ptr(out.get(name)) for name in SLOPE_OUTPUTS], _lib.STREAM, device=dev)
    return VisitSlopes(min_visits=int(min_visits), min_span=float(min_span), **out)


# ---- cohort regression (include/oai_hip.h, "Cohort regression"; csrc/group_regression.hip) ---------------------------------------------------
MAX_DESIGN_COLUMNS = 6


@dataclass
class RegressionPrepared:
    """The prepared block of ``regression_prepare`` and views of its arrays (include/oai_hip.h states the layout): ``R`` float64 [N,V], the
    residuals of the (centred) values on the nuisance columns; ``Q``, ``mean`` float64 [V]; ``n`` int32 [V]; ``ok`` uint8 [V].  ``mask``:
    the uint8 [N,V] mask it was prepared with, or None; ``n_nuisance``: the q it was prepared with."""
    block: torch.Tensor
    n_knees: int
    n_verts: int
    n_nuisance: int
    centre: bool
    mask: Optional[torch.Tensor]
    R: torch.Tensor
    Q: torch.Tensor
    mean: torch.Tensor
    n: torch.Tensor
    ok: torch.Tensor


def _design(design, name: str, n_knees: int, device, lo: int, hi: int) -> torch.Tensor:
    design = _chk(design, name, torch.float64)
    if design.dim() != 2 or design.shape[0] != n_knees or not lo <= design.shape[1] <= hi or design.device != device:
        raise ValueError(f"{name} must be float64 [{n_knees}, {lo} .. {hi}] on {device}, got {tuple(design.shape)} on {design.device}")
    return design


def regression_prepare(values: torch.Tensor, mask: Optional[torch.Tensor] = None, nuisance: Optional[torch.Tensor] = None,
                       centre: bool = True) -> RegressionPrepared:
    """What every permutation of a regression re-uses, once per test: float32 ``values`` [N,V], an optional uint8 / bool ``mask`` [N,V] and
    the float64 ``nuisance`` columns [N,q] (0 <= q <= 5, the intercept among them; None: q = 0) -> per vertex n, mean, the residuals of the
    values (less their mean when ``centre``) on the nuisance columns over the knees with a value, their sum of squares Q, and ``ok``
    (the nuisance system has full rank there and n - q - 1 >= 1).  fp64 in a stated order: bit-reproducible.  Does not synchronise."""
    values = _chk(values, "values")
    if values.dim() != 2 or values.shape[0] < 2 or values.shape[1] < 1:
        raise ValueError(f"values must be [N >= 2, V >= 1], got {tuple(values.shape)}")
    mask = _stats_mask(mask, values)
    N, V = int(values.shape[0]), int(values.shape[1])
    q = 0
    if nuisance is not None and nuisance.numel() > 0:
        nuisance = _design(nuisance, "nuisance", N, values.device, 1, MAX_DESIGN_COLUMNS - 1)
        q = int(nuisance.shape[1])
    block = _lib.workspace("oai_regression_prepare", values.device, N, V)
    _lib.call("oai_regression_prepare", values.data_ptr(), _ptr(mask), nuisance.data_ptr() if q else None, N, V, q, int(bool(centre)),
              block.data_ptr(), block.numel(), _lib.STREAM, device=values.device)
    parts = _block_views(block, (("R", torch.float64, (N, V)), ("Q", torch.float64, (V,)), ("mean", torch.float64, (V,)), ("n", torch.int32, (V,)),
                                 ("ok", torch.uint8, (V,))))
    return RegressionPrepared(block, N, V, q, bool(centre), mask, **parts)


def _regression_batch(prepared: RegressionPrepared, design, perm, p0, p1, lo: int, hi: int, out0, out0_name: str, out0_shape):
    """What ``regression_t`` and ``regression_f`` check alike: the design with ``lo`` .. ``hi`` columns, the index rows, the row range and
    the optional float64 output of row 0.  Returns (design, perm, p0, p1, out0)."""
    dev, N = prepared.block.device, prepared.n_knees
    design = _design(design, "design", N, dev, lo, hi)
    perm = _chk(perm, "perm", torch.int32)
    if perm.dim() != 2 or perm.shape[1] != N or perm.device != dev:
        raise ValueError(f"perm must be int32 [P, {N}] on {dev}, got {tuple(perm.shape)} on {perm.device}")
    p0, p1 = int(p0), int(p1)
    if not 0 <= p0 < p1 <= perm.shape[0]:
        raise ValueError(f"rows [{p0}, {p1}) are not rows of the {perm.shape[0]} permutations")
    if out0 is not None:
        out0 = _chk(out0, out0_name, torch.float64)
        if tuple(out0.shape) != tuple(out0_shape) or out0.device != dev:
            raise ValueError(f"{out0_name} must be float64 {list(out0_shape)} on {dev}, got {tuple(out0.shape)} on {out0.device}")
    return design, perm, p0, p1, out0


def _regression_tile(name: str, prepared, head, size, p0: int, p1: int, workspace, out0) -> torch.Tensor:
    """The call tail of the four batch entry points once their arguments are checked: the workspace of rows [p0, p1) (``size``: what
    ``name``_workspace_bytes takes after the row count), the call -- ``head``: the entry point's arguments between the prepared block
    and p0 -- and the tile, the front of the workspace."""
    dev, V = prepared.block.device, prepared.n_verts
    need = int(getattr(_lib.load(), name + "_workspace_bytes")(p1 - p0, *size))
    ws = _tile_workspace(workspace, need, dev)
    _lib.call(name, prepared.block.data_ptr(), prepared.block.numel(), *head, p0, p1, ws.data_ptr(), ws.numel(), _ptr(out0), _lib.STREAM, device=dev)
    return ws[:(p1 - p0) * V * 8].view(torch.float64).reshape(p1 - p0, V)


def regression_t(prepared: RegressionPrepared, design: torch.Tensor, perm: torch.Tensor, p0: int, p1: int, workspace: Optional[torch.Tensor] = None,
                 slope0: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The t tile of rows [p0, p1) of ``perm`` (int32 [P,N] on the device: knee j of a row takes design row ``perm[row, j]``; row 0 the
    identity): float64 [p1 - p0, V], the t of the LAST column of the float64 ``design`` [N,p] (p = the prepared q + 1), NaN where no t
    exists.  ``slope0`` float64 [V]: with ``p0`` = 0, receives row 0's coefficient of that column.  ``workspace``: a uint8 device buffer of
    ``oai_regression_t_workspace_bytes`` (reused between batches) instead of a new one; the tile is its front.  Does not synchronise."""
    N, V = prepared.n_knees, prepared.n_verts
    p = prepared.n_nuisance + 1
    design, perm, p0, p1, slope0 = _regression_batch(prepared, design, perm, p0, p1, p, p, slope0, "slope0", (V,))
    return _regression_tile("oai_regression_t", prepared, (_ptr(prepared.mask), design.data_ptr(), perm.data_ptr(), N, V, p), (V, N, p), p0, p1,
                            workspace, slope0)


def regression_f(prepared: RegressionPrepared, design: torch.Tensor, perm: torch.Tensor, p0: int, p1: int, n_interest: int,
                 workspace: Optional[torch.Tensor] = None, coef0: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The F tile of rows [p0, p1) of ``perm`` (as in ``regression_t``): float64 [p1 - p0, V], the F of the LAST ``n_interest`` columns of
    the float64 ``design`` [N,p], tested jointly given the columns before them (include/oai_hip.h, "Cohort F test"), NaN where no F
    exists.  ``prepared`` must have been prepared with the first p - ``n_interest`` columns as its nuisance: p = the prepared q +
    ``n_interest``.  ``coef0`` float64 [n_interest, V]: with ``p0`` = 0, receives row 0's coefficients of those columns.  ``workspace``: a
    uint8 device buffer of ``oai_regression_f_workspace_bytes`` (reused between batches) instead of a new one; the tile is its front.
    Does not synchronise."""
    N, V = prepared.n_knees, prepared.n_verts
    k = int(n_interest)
    if not 1 <= k <= MAX_DESIGN_COLUMNS - prepared.n_nuisance:
        raise ValueError(f"n_interest must be 1 .. {MAX_DESIGN_COLUMNS - prepared.n_nuisance} beside the {prepared.n_nuisance} nuisance columns "
                         f"of the prepared block, got {n_interest!r}")
    p = prepared.n_nuisance + k
    design, perm, p0, p1, coef0 = _regression_batch(prepared, design, perm, p0, p1, p, p, coef0, "coef0", (k, V))
    return _regression_tile("oai_regression_f", prepared, (_ptr(prepared.mask), design.data_ptr(), perm.data_ptr(), N, V, p, k), (V, N, p), p0, p1,
                            workspace, coef0)


# ---- cluster-robust regression (include/oai_hip.h, "Cluster-robust regression"; csrc/cluster_robust.hip) -----------------------------------
MAX_CLUSTER_ROWS = 1 << 20


@dataclass
class ClusterPrepared:
    """The cluster block of ``cluster_prepare`` and views of its arrays (include/oai_hip.h states the layout): those of
    ``RegressionPrepared`` (``R``, ``Q``, ``mean``, ``n``, ``ok``), then ``H``, ``K`` float64 [p,S,V], ``U`` float64 [S,V], ``L`` float64
    [p (p + 1) / 2, V], ``c`` float64 [V], ``G`` int32 [V] and ``okc`` uint8 [V].  ``mask``: the uint8 [N,V] mask it was prepared with, or
    None."""
    block: torch.Tensor
    n_rows: int
    n_verts: int
    n_clusters: int
    n_columns: int
    mask: Optional[torch.Tensor]
    R: torch.Tensor
    Q: torch.Tensor
    mean: torch.Tensor
    n: torch.Tensor
    ok: torch.Tensor
    H: torch.Tensor
    K: torch.Tensor
    U: torch.Tensor
    L: torch.Tensor
    c: torch.Tensor
    G: torch.Tensor
    okc: torch.Tensor


def cluster_prepare(values: torch.Tensor, mask: Optional[torch.Tensor], design: torch.Tensor, offsets: torch.Tensor,
                    centre: bool = True) -> ClusterPrepared:
    """What every resample of a cluster-robust regression re-uses, once per test: float32 ``values`` [N,V] with the rows in CLUSTER-MAJOR
    order, an optional uint8 / bool ``mask`` [N,V], the float64 ``design`` [N,p] with the regressor of interest LAST (1 <= p <= 6) and the
    int32 ``offsets`` [S+1]: cluster s owns rows ``offsets[s] .. offsets[s+1] - 1``.  Runs ``oai_regression_prepare`` with the first
    p - 1 columns as the nuisance (``centre``: as in ``regression_prepare``) into the front of one block and ``oai_cluster_prepare`` behind
    it: per vertex the factor of the design's normal equations over the valid rows, per (cluster, vertex) the score sums, G, the CR1
    factor and ``okc``.  fp64 in a stated order: bit-reproducible.  Does not synchronise."""
    values = _chk(values, "values")
    if values.dim() != 2 or not 2 <= values.shape[0] <= MAX_CLUSTER_ROWS or values.shape[1] < 1:
        raise ValueError(f"values must be [2 <= N <= 2^20, V >= 1], got {tuple(values.shape)}")
    mask = _stats_mask(mask, values)
    N, V, dev = int(values.shape[0]), int(values.shape[1]), values.device
    design = _design(design, "design", N, dev, 1, MAX_DESIGN_COLUMNS)
    p = int(design.shape[1])
    offsets = _chk(offsets, "offsets", torch.int32).reshape(-1)
    S = int(offsets.numel()) - 1
    if not 2 <= S <= N or offsets.device != dev:
        raise ValueError(f"offsets must hold S + 1 entries for 2 <= S <= {N} clusters on {dev}, got {offsets.numel()} on {offsets.device}")
    nuisance = design[:, :p - 1].contiguous() if p > 1 else None
    block = _lib.workspace("oai_cluster_prepare", dev, N, V, S, p)
    _lib.call("oai_regression_prepare", values.data_ptr(), _ptr(mask), _ptr(nuisance), N, V, p - 1, int(bool(centre)), block.data_ptr(), block.numel(),
              _lib.STREAM, device=dev)
    _lib.call("oai_cluster_prepare", _ptr(mask), design.data_ptr(), offsets.data_ptr(), N, V, S, p, block.data_ptr(), block.numel(), _lib.STREAM,
              device=dev)
    f64, T = torch.float64, p * (p + 1) // 2
    parts = _block_views(block, (("R", f64, (N, V)), ("Q", f64, (V,)), ("mean", f64, (V,)), ("n", torch.int32, (V,)), ("ok", torch.uint8, (V,)),
                                 ("H", f64, (p, S, V)), ("K", f64, (p, S, V)), ("U", f64, (S, V)), ("L", f64, (T, V)), ("c", f64, (V,)),
                                 ("G", torch.int32, (V,)), ("okc", torch.uint8, (V,))))
    return ClusterPrepared(block, N, V, S, p, mask, **parts)


def cluster_t(prepared: ClusterPrepared, bits: torch.Tensor, p0: int, p1: int, workspace: Optional[torch.Tensor] = None,
              slope0: Optional[torch.Tensor] = None, se0: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The t tile of rows [p0, p1) of ``bits`` (packed flip rows over the CLUSTERS, [P, ceil(S / 32)] as int32 or uint32 on the device: a set
    bit flips the sign of the cluster's null-model residuals; row 0 flips nothing): float64 [p1 - p0, V], the cluster-robust t of the
    LAST design column under the restricted wild cluster bootstrap, NaN where no t exists.  ``slope0``, ``se0`` float64 [V]: with ``p0`` =
    0, receive row 0's coefficient of that column and its sandwich standard error.  ``workspace``: a uint8 device buffer of
    ``oai_cluster_t_workspace_bytes`` (reused between batches) instead of a new one; the tile is its front.  Does not synchronise."""
    dev, N, V, S, p = prepared.block.device, prepared.n_rows, prepared.n_verts, prepared.n_clusters, prepared.n_columns
    if bits.dtype == getattr(torch, "uint32", None):
        bits = bits.view(torch.int32)
    bits = _chk(bits, "bits", torch.int32)
    if bits.dim() != 2 or bits.shape[1] != (S + 31) // 32 or bits.device != dev:
        raise ValueError(f"bits must be [P, {(S + 31) // 32}] packed flip rows of the {S} clusters on {dev}, got {tuple(bits.shape)} on {bits.device}")
    p0, p1 = int(p0), int(p1)
    if not 0 <= p0 < p1 <= bits.shape[0]:
        raise ValueError(f"rows [{p0}, {p1}) are not rows of the {bits.shape[0]} flip rows")
    outs = []
    for name, out0 in (("slope0", slope0), ("se0", se0)):
        if out0 is not None:
            out0 = _chk(out0, name, torch.float64)
            if tuple(out0.shape) != (V,) or out0.device != dev:
                raise ValueError(f"{name} must be float64 [{V}] on {dev}, got {tuple(out0.shape)} on {out0.device}")
        outs.append(out0)
    need = int(_lib.load().oai_cluster_t_workspace_bytes(p1 - p0, V))
    ws = _tile_workspace(workspace, need, dev)
    _lib.call("oai_cluster_t", prepared.block.data_ptr(), prepared.block.numel(), bits.data_ptr(), N, V, S, p, p0, p1, ws.data_ptr(), ws.numel(),
              _ptr(outs[0]), _ptr(outs[1]), _lib.STREAM, device=dev)
    return ws[:(p1 - p0) * V * 8].view(torch.float64).reshape(p1 - p0, V)


# ---- vertex-wise design columns (include/oai_hip.h, "Vertex-wise design columns"; csrc/group_regression_vx.hip) ------------------------------
MAX_VERTEX_COLUMNS = 2


@dataclass
class RegressionVxPrepared:
    """The prepared block of ``regression_vx_prepare`` and views of its arrays (include/oai_hip.h states the layout): ``R``, ``Q``, ``mean``,
    ``n``, ``ok`` as in ``RegressionPrepared`` -- ``n`` counts the COMPLETE cases --, then ``n_dropped`` int32 [V] (knees with a value whose
    covariate is missing), ``m`` uint8 [N,V] (the effective mask) and ``WC`` float64 [S,N,V] (the completed per-vertex columns).
    ``n_vertex_nuisance``, ``n_vertex_interest``, ``n_global_nuisance``: the s_n, s_i and q_g it was prepared with."""
    block: torch.Tensor
    n_knees: int
    n_verts: int
    n_vertex_nuisance: int
    n_vertex_interest: int
    n_global_nuisance: int
    centre: bool
    R: torch.Tensor
    Q: torch.Tensor
    mean: torch.Tensor
    n: torch.Tensor
    ok: torch.Tensor
    n_dropped: torch.Tensor
    m: torch.Tensor
    WC: torch.Tensor


def regression_vx_prepare(values: torch.Tensor, mask: Optional[torch.Tensor], vertex_columns: torch.Tensor,
                          vertex_mask: Optional[torch.Tensor] = None, nuisance: Optional[torch.Tensor] = None, n_vertex_interest: int = 0,
                          centre: bool = True) -> RegressionVxPrepared:
    """What every permutation of a regression with per-vertex design columns re-uses, once per test: float32 ``values`` [N,V] with an
    optional uint8 / bool ``mask``; float32 ``vertex_columns`` [S,N,V] (S = 1 or 2, in the design's order: nuisance first, and with
    ``n_vertex_interest`` = 1 the regressor of interest last) with an optional ``vertex_mask`` [S,N,V]; the float64 global ``nuisance``
    columns [N,q_g] (the intercept among them; None: q_g = 0) -> per vertex the complete cases, the completed columns and the residuals of
    the values on the nuisance columns over them.  fp64 in a stated order: bit-reproducible.  Does not synchronise."""
    values = _chk(values, "values")
    if values.dim() != 2 or values.shape[0] < 2 or values.shape[1] < 1:
        raise ValueError(f"values must be [N >= 2, V >= 1], got {tuple(values.shape)}")
    mask = _stats_mask(mask, values)
    N, V = int(values.shape[0]), int(values.shape[1])
    w = _chk(vertex_columns, "vertex_columns")
    if w.dim() != 3 or not 1 <= w.shape[0] <= MAX_VERTEX_COLUMNS or tuple(w.shape[1:]) != (N, V) or w.device != values.device:
        raise ValueError(f"vertex_columns must be float32 [1 .. {MAX_VERTEX_COLUMNS}, {N}, {V}] on {values.device}, got {tuple(w.shape)} on {w.device}")
    S, si = int(w.shape[0]), int(n_vertex_interest)
    if si not in (0, 1):
        raise ValueError(f"n_vertex_interest must be 0 or 1, got {n_vertex_interest!r}")
    wmask = None
    if vertex_mask is not None:
        wmask = _chk(vertex_mask.view(torch.uint8) if vertex_mask.dtype == torch.bool else vertex_mask, "vertex_mask", torch.uint8)
        if tuple(wmask.shape) != tuple(w.shape) or wmask.device != w.device:
            raise ValueError(f"vertex_mask must have the shape of vertex_columns {tuple(w.shape)} and live on their GPU, got {tuple(wmask.shape)} "
                             f"on {wmask.device}")
    qg = 0
    if nuisance is not None and nuisance.numel() > 0:
        nuisance = _design(nuisance, "nuisance", N, values.device, 1, MAX_DESIGN_COLUMNS - 1 - (S - si))
        qg = int(nuisance.shape[1])
    block = _lib.workspace("oai_regression_vx_prepare", values.device, N, V, S)
    _lib.call("oai_regression_vx_prepare", values.data_ptr(), _ptr(mask), w.data_ptr(), _ptr(wmask), nuisance.data_ptr() if qg else None, N, V, S - si,
              si, qg, int(bool(centre)), block.data_ptr(), block.numel(), _lib.STREAM, device=values.device)
    parts = _block_views(block, (("R", torch.float64, (N, V)), ("Q", torch.float64, (V,)), ("mean", torch.float64, (V,)), ("n", torch.int32, (V,)),
                                 ("ok", torch.uint8, (V,)), ("n_dropped", torch.int32, (V,)), ("m", torch.uint8, (N, V)),
                                 ("WC", torch.float64, (S, N, V))))
    return RegressionVxPrepared(block, N, V, S - si, si, qg, bool(centre), **parts)


def _regression_vx_batch(name: str, prepared: RegressionVxPrepared, design, perm, p0, p1, n_global: int, extra, workspace, out0, out0_name: str,
                         out0_shape) -> torch.Tensor:
    """The one call path of ``regression_vx_t`` and ``regression_vx_f``: the global columns [N, n_global] (None where there are none), the
    index rows, the row range, the optional output of row 0, the workspace; ``extra``: the entry point's own arguments after s_i."""
    dev, N, V = prepared.block.device, prepared.n_knees, prepared.n_verts
    sn, si = prepared.n_vertex_nuisance, prepared.n_vertex_interest
    p = sn + si + n_global
    if n_global == 0 and (design is None or design.numel() == 0):
        design = torch.empty((N, 1), dtype=torch.float64, device=dev)         # checked like any design; never read
        lo = 1
    else:
        lo = n_global
    design, perm, p0, p1, out0 = _regression_batch(prepared, design, perm, p0, p1, lo, lo, out0, out0_name, out0_shape)
    return _regression_tile(name, prepared, (design.data_ptr() if n_global else None, perm.data_ptr(), N, V, p, sn, si, *extra), (V, N, p, sn + si),
                            p0, p1, workspace, out0)


def regression_vx_t(prepared: RegressionVxPrepared, design: Optional[torch.Tensor], perm: torch.Tensor, p0: int, p1: int,
                    workspace: Optional[torch.Tensor] = None, slope0: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The t tile of rows [p0, p1) of ``perm`` (as in ``regression_t``): float64 [p1 - p0, V], the t of the LAST design column -- the
    per-vertex regressor when the block was prepared with ``n_vertex_interest`` = 1, otherwise the last column of the float64 global
    ``design`` [N, q_g + 1] (None when there are no global columns at all).  Knee j of a row takes the WHOLE design row ``perm[row, j]``,
    the per-vertex entries included.  ``slope0`` float64 [V]: with ``p0`` = 0, receives row 0's coefficient of that column.  ``workspace``:
    a uint8 device buffer of ``oai_regression_vx_t_workspace_bytes``, reused between batches; the tile is its front.  Does not synchronise."""
    n_global = prepared.n_global_nuisance + (0 if prepared.n_vertex_interest else 1)
    return _regression_vx_batch("oai_regression_vx_t", prepared, design, perm, p0, p1, n_global, (), workspace, slope0, "slope0", (prepared.n_verts,))


def regression_vx_f(prepared: RegressionVxPrepared, design: torch.Tensor, perm: torch.Tensor, p0: int, p1: int, n_interest: int,
                    workspace: Optional[torch.Tensor] = None, coef0: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The F tile of rows [p0, p1) of ``perm``: float64 [p1 - p0, V], the F of the LAST ``n_interest`` columns of the float64 global
    ``design`` [N, q_g + n_interest], tested jointly given the per-vertex nuisance columns and the global ones before them.  The block must
    have been prepared with ``n_vertex_interest`` = 0.  ``coef0`` float64 [n_interest, V]: with ``p0`` = 0, receives row 0's coefficients of
    those columns.  ``workspace``: as in ``regression_vx_t``.  Does not synchronise."""
    k = int(n_interest)
    most = MAX_DESIGN_COLUMNS - prepared.n_vertex_nuisance - prepared.n_global_nuisance
    if prepared.n_vertex_interest:
        raise ValueError("regression_vx_f tests global columns: the block was prepared with a per-vertex column of interest, which regression_vx_t tests")
    if not 1 <= k <= most:
        raise ValueError(f"n_interest must be 1 .. {most} beside the {prepared.n_vertex_nuisance} + {prepared.n_global_nuisance} nuisance columns of "
                         f"the prepared block, got {n_interest!r}")
    return _regression_vx_batch("oai_regression_vx_f", prepared, design, perm, p0, p1, prepared.n_global_nuisance + k, (k,), workspace, coef0, "coef0",
                                (k, prepared.n_verts))


# ---- normative deviation (include/oai_hip.h, "Normative deviation"; csrc/normative.hip) ------------------------------------------------------
NORMATIVE_SCORE_ROWS = 8             # rows per thread of the score kernel


@dataclass
class NormativeFit:
    """The model block of ``normative_fit`` and views of its arrays (include/oai_hip.h states the layout, component-major): ``gamma``
    float64 [p,V], ``L`` float64 [p (p + 1) / 2, V], ``rss`` float64 [V], ``n`` int32 [V], ``ok`` uint8 [V]."""
    block: torch.Tensor
    n_verts: int
    n_columns: int
    gamma: torch.Tensor
    L: torch.Tensor
    rss: torch.Tensor
    n: torch.Tensor
    ok: torch.Tensor


def normative_block(n_verts: int, n_columns: int, device) -> NormativeFit:
    """An UNFILLED model block for ``n_verts`` vertices and ``n_columns`` design columns on ``device``: what ``normative_fit`` writes, and
    what a caller that kept the arrays of a model copies them back into."""
    V, p = int(n_verts), int(n_columns)
    if V < 1 or not 1 <= p <= MAX_DESIGN_COLUMNS:
        raise ValueError(f"a model block needs V >= 1 vertices and 1 .. {MAX_DESIGN_COLUMNS} design columns, got {n_verts!r}, {n_columns!r}")
    block = _lib.workspace("oai_normative_fit", device, V, p)
    parts = _block_views(block, (("gamma", torch.float64, (p, V)), ("L", torch.float64, (p * (p + 1) // 2, V)), ("rss", torch.float64, (V,)),
                                 ("n", torch.int32, (V,)), ("ok", torch.uint8, (V,))))
    return NormativeFit(block, V, p, **parts)


def normative_fit(values: torch.Tensor, design: torch.Tensor, mask: Optional[torch.Tensor] = None) -> NormativeFit:
    """The per-vertex linear model of a reference cohort: float32 ``values`` [N,V], an optional uint8 / bool ``mask`` [N,V] and the float64
    ``design`` [N,p] (1 <= p <= 6, the intercept among its columns) -> per vertex the coefficients, the Cholesky factor of the normal
    equations over the knees with a value, the residual sum of squares, n and ok.  fp64 in a stated order: bit-reproducible.  Does not
    synchronise."""
    values = _chk(values, "values")
    if values.dim() != 2 or values.shape[0] < 2 or values.shape[1] < 1:
        raise ValueError(f"values must be [N >= 2, V >= 1], got {tuple(values.shape)}")
    mask = _stats_mask(mask, values)
    N, V = int(values.shape[0]), int(values.shape[1])
    design = _design(design, "design", N, values.device, 1, MAX_DESIGN_COLUMNS)
    model = normative_block(V, int(design.shape[1]), values.device)
    _lib.call("oai_normative_fit", values.data_ptr(), _ptr(mask), design.data_ptr(), N, V, model.n_columns, model.block.data_ptr(),
              model.block.numel(), _lib.STREAM, device=values.device)
    return model


def normative_score(model: NormativeFit, values: torch.Tensor, design_rows: torch.Tensor, mask: Optional[torch.Tensor] = None, loo: bool = False,
                    workspace: Optional[torch.Tensor] = None, diff: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The z tile of the knees ``values`` (float32 [R,V], optional uint8 / bool ``mask``) against ``model``, each with its design row
    (float64 ``design_rows`` [R,p]): float64 [R,V], NaN where no score exists.  ``loo`` False: the knees are not in the fit (the
    prediction-interval t); True: row k is the fit's own row k (the externally studentised residual).  ``diff`` float64 [R,V]: receives the
    deviation in mm.  ``workspace``: a uint8 device buffer to hold the tile instead of a new one.  Does not synchronise."""
    values = _chk(values, "values")
    if values.dim() != 2 or values.shape[0] < 1 or values.shape[1] != model.n_verts or values.device != model.block.device:
        raise ValueError(f"values must be [R >= 1, {model.n_verts}] on {model.block.device}, got {tuple(values.shape)} on {values.device}")
    mask = _stats_mask(mask, values)
    R, V, dev = int(values.shape[0]), model.n_verts, values.device
    design_rows = _design(design_rows, "design_rows", R, dev, model.n_columns, model.n_columns)
    if diff is not None:
        diff = _out_tile(diff, "diff", torch.float64, values, may_alias=True)
    need = int(_lib.load().oai_normative_score_workspace_bytes(R, V))
    ws = _tile_workspace(workspace, need, dev)
    _lib.call("oai_normative_score", model.block.data_ptr(), model.block.numel(), values.data_ptr(), _ptr(mask), design_rows.data_ptr(), R, V,
              model.n_columns, int(bool(loo)), ws.data_ptr(), ws.numel(), _ptr(diff), _lib.STREAM, device=dev)
    return ws[:R * V * 8].view(torch.float64).reshape(R, V)


def deviation_summary(tile: torch.Tensor, z_threshold: float, weights: Optional[torch.Tensor] = None):
    """Per row of the float64 z ``tile`` [R,V], over its entries that are not NaN: the float64 [R,3] and int64 [R,6] DEVICE tensors (stats,
    counts) -- stats = (max |z|, min z, max z); counts = (valid entries, the vertex of max |z| -- the smallest at a tie --, the vertex count
    and the summed int64 ``weights`` [V] of {z < -z_threshold}, the same of {z > z_threshold}); without ``weights`` every weight is 1.
    Exact maxima and integer sums.  Does not synchronise."""
    tile = _chk(tile, "tile", torch.float64)
    if tile.dim() != 2 or tile.shape[0] < 1 or tile.shape[1] < 1:
        raise ValueError(f"tile must be [R >= 1, V >= 1], got {tuple(tile.shape)}")
    if not float(z_threshold) > 0.0:
        raise ValueError(f"z_threshold must be > 0, got {z_threshold!r}")
    R, V, dev = int(tile.shape[0]), int(tile.shape[1]), tile.device
    if weights is not None:
        weights = _chk(weights, "weights", torch.int64)
        if tuple(weights.shape) != (V,) or weights.device != dev:
            raise ValueError(f"weights must be int64 [{V}] on the tile's GPU, got {tuple(weights.shape)} on {weights.device}")
    stats = torch.empty((R, 3), dtype=torch.float64, device=dev)
    counts = torch.empty((R, 6), dtype=torch.int64, device=dev)
    ws = _lib.workspace("oai_deviation_summary", dev, R, V)
    _lib.call("oai_deviation_summary", tile.data_ptr(), R, V, _ptr(weights), float(z_threshold), ws.data_ptr(), ws.numel(), stats.data_ptr(),
              counts.data_ptr(), _lib.STREAM, device=dev)
    return stats, counts


# ---- bootstrap intervals (include/oai_hip.h, "Bootstrap intervals"; csrc/bootstrap.hip) -----------------------------------------------------
MAX_QUANTILES = 4                    # probabilities per call of column_quantiles


def _span_vector(t: Optional[torch.Tensor], name: str, dtype, n: int, device) -> torch.Tensor:
    """The caller's contiguous [n] output of ``dtype`` on ``device`` once it is checked, or a new one."""
    if t is None:
        return torch.empty(n, dtype=dtype, device=device)
    if t.dtype != dtype or tuple(t.shape) != (n,) or t.device != device or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {str(dtype).split('.')[1]} [{n}] tensor on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def _replicate_tile(tile: torch.Tensor, name: str = "tile"):
    tile = _chk(tile, name, torch.float64)
    if tile.dim() != 2 or tile.shape[0] < 1 or tile.shape[1] < 1:
        raise ValueError(f"{name} must be [R >= 1, V >= 1], got {tuple(tile.shape)}")
    return tile, int(tile.shape[0]), int(tile.shape[1])


def bootstrap_coef(values: torch.Tensor, design: torch.Tensor, counts: torch.Tensor, r0: int, r1: int, mask: Optional[torch.Tensor] = None,
                   v0: int = 0, v1: Optional[int] = None, workspace: Optional[torch.Tensor] = None, n: Optional[torch.Tensor] = None,
                   ok: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The coefficient tile of rows [r0, r1) of ``counts`` (uint16 [R,N] on the device: how often knee i enters resample r; row 0 all ones
    by convention) on the vertex span [v0, v1): float64 [r1 - r0, v1 - v0], the coefficient of the LAST column of the float64 ``design``
    [N,p] (1 <= p <= 6) in the per-vertex weighted least squares of the float32 ``values`` [N,V] over the knees that the uint8 / bool
    ``mask`` [N,V] calls valid (None: all), NaN where the resample has no full rank there.  ``n``, ``ok`` int32 [V]: with ``r0`` = 0 their
    entries [v0, v1) receive the valid knees and whether row 0 has a coefficient.  ``workspace``: a uint8 device buffer of
    ``oai_bootstrap_coef_workspace_bytes`` (reused between spans) instead of a new one; the tile is its front.  fp64 in a stated order:
    bit-reproducible.  Does not synchronise."""
    values = _chk(values, "values")
    if values.dim() != 2 or values.shape[0] < 2 or values.shape[1] < 1:
        raise ValueError(f"values must be [N >= 2, V >= 1], got {tuple(values.shape)}")
    mask = _stats_mask(mask, values)
    N, V, dev = int(values.shape[0]), int(values.shape[1]), values.device
    design = _design(design, "design", N, dev, 1, MAX_DESIGN_COLUMNS)
    p = int(design.shape[1])
    counts = _chk(counts, "counts", torch.uint16)
    if counts.dim() != 2 or counts.shape[1] != N or counts.device != dev:
        raise ValueError(f"counts must be uint16 [R, {N}] on {dev}, got {tuple(counts.shape)} on {counts.device}")
    r0, r1, v0, v1 = int(r0), int(r1), int(v0), V if v1 is None else int(v1)
    if not 0 <= r0 < r1 <= counts.shape[0]:
        raise ValueError(f"rows [{r0}, {r1}) are not rows of the {counts.shape[0]} resamples")
    if not 0 <= v0 < v1 <= V:
        raise ValueError(f"the span [{v0}, {v1}) does not lie in the {V} vertices")
    n = None if n is None else _span_vector(n, "n", torch.int32, V, dev)
    ok = None if ok is None else _span_vector(ok, "ok", torch.int32, V, dev)
    need = int(_lib.load().oai_bootstrap_coef_workspace_bytes(r1 - r0, v1 - v0, N, p))
    ws = _tile_workspace(workspace, need, dev)
    _lib.call("oai_bootstrap_coef", values.data_ptr(), _ptr(mask), design.data_ptr(), counts.data_ptr(), N, V, p, v0, v1, r0, r1, ws.data_ptr(),
              ws.numel(), _ptr(n), _ptr(ok), _lib.STREAM, device=dev)
    return ws[:(r1 - r0) * (v1 - v0) * 8].view(torch.float64).reshape(r1 - r0, v1 - v0)


@dataclass
class BootstrapMoments:
    """Per vertex of a replicate tile, over rows 1..: ``n_finite`` int32 (B'), ``mean``, ``se`` float64, and the int32 counts ``below``,
    ``equal`` of the finite replicates below / equal to row 0's entry.  DEVICE tensors [V]."""
    n_finite: torch.Tensor
    mean: torch.Tensor
    se: torch.Tensor
    below: torch.Tensor
    equal: torch.Tensor


def bootstrap_moments(tile: torch.Tensor) -> BootstrapMoments:
    """What an interval needs from the replicates of the float64 ``tile`` [R,V] (row 0 the observed data, rows 1.. the resamples) besides
    their order statistics: see ``BootstrapMoments``.  Two passes in ascending row, fp64: bit-reproducible.  Does not synchronise."""
    tile, R, V = _replicate_tile(tile)
    dev = tile.device
    out = BootstrapMoments(torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.float64, device=dev),
                           torch.empty(V, dtype=torch.float64, device=dev), torch.empty(V, dtype=torch.int32, device=dev),
                           torch.empty(V, dtype=torch.int32, device=dev))
    _lib.call("oai_bootstrap_moments", tile.data_ptr(), R, V, out.n_finite.data_ptr(), out.mean.data_ptr(), out.se.data_ptr(), out.below.data_ptr(),
              out.equal.data_ptr(), _lib.STREAM, device=dev)
    return out


def column_quantiles(tile: torch.Tensor, probabilities, first_row: int = 0, workspace: Optional[torch.Tensor] = None):
    """Exact quantiles per vertex of rows [first_row, R) of the float64 ``tile`` [R,V], over the entries that are not NaN, as
    ``np.quantile(..., method="linear")`` in float64 (-0.0 sorts before +0.0).  ``probabilities``: a sequence of K <= 4 floats shared by all
    vertices, or a float64 DEVICE tensor [K,V] of per-vertex ones.  Returns (float64 [K,V], int32 [V] = the entries that are not NaN),
    DEVICE tensors; NaN for a vertex without entries and for a probability that is NaN or outside [0, 1].  ``workspace``: a uint8 device
    buffer of ``oai_column_quantiles_workspace_bytes`` instead of a new one.  Does not synchronise."""
    tile, R, V = _replicate_tile(tile)
    dev = tile.device
    first_row = int(first_row)
    if not 0 <= first_row <= R:
        raise ValueError(f"first_row must be 0 .. {R}, got {first_row}")
    if isinstance(probabilities, torch.Tensor):
        probs = _chk(probabilities, "probabilities", torch.float64)
        if probs.dim() != 2 or not 1 <= probs.shape[0] <= MAX_QUANTILES or probs.shape[1] != V or probs.device != dev:
            raise ValueError(f"per-vertex probabilities must be float64 [1 .. {MAX_QUANTILES}, {V}] on {dev}, got {tuple(probs.shape)} on {probs.device}")
        K, host, device_ptr = int(probs.shape[0]), None, probs.data_ptr()
    else:
        q = [float(x) for x in np.asarray(probabilities, np.float64).reshape(-1)]
        if not 1 <= len(q) <= MAX_QUANTILES:
            raise ValueError(f"needs 1 .. {MAX_QUANTILES} probabilities, got {len(q)}")
        K, host, device_ptr = len(q), (C.c_double * len(q))(*q), None
    out = torch.empty((K, V), dtype=torch.float64, device=dev)
    count = torch.empty(V, dtype=torch.int32, device=dev)
    need = int(_lib.load().oai_column_quantiles_workspace_bytes(R, V))
    ws = _tile_workspace(workspace, need, dev)
    _lib.call("oai_column_quantiles", tile.data_ptr(), R, V, first_row, K, host, device_ptr, ws.data_ptr(), ws.numel(), out.data_ptr(),
              count.data_ptr(), _lib.STREAM, device=dev)
    return out, count


def bootstrap_sup(tile: torch.Tensor, se: torch.Tensor, sup: torch.Tensor) -> None:
    """Raise the running ``sup`` float64 [R] (started at 0.0 by the caller) by each row's max over the vertices of
    |tile[r, v] - tile[0, v]| / se[v], taken where row 0's entry is finite and ``se`` > 0 and the entry is not NaN: the sup-t statistic of
    a simultaneous band, folded across vertex spans.  A max: exact in any order.  Does not synchronise."""
    tile, R, V = _replicate_tile(tile)
    dev = tile.device
    se, sup = _span_vector(se, "se", torch.float64, V, dev), _span_vector(sup, "sup", torch.float64, R, dev)
    _lib.call("oai_bootstrap_sup", tile.data_ptr(), R, V, se.data_ptr(), sup.data_ptr(), _lib.STREAM, device=dev)


def jackknife_acceleration(jack: torch.Tensor, strata: torch.Tensor, n_strata: int, mask: Optional[torch.Tensor] = None, v0: int = 0) -> torch.Tensor:
    """The BCa acceleration per vertex from the float64 jackknife tile ``jack`` [N, span] (``bootstrap_coef`` of the N count rows "all
    ones except a 0 at knee i" on the span that starts at ``v0``), the int32 stratum label of every knee (0 .. ``n_strata`` - 1) and the
    cohort's uint8 / bool ``mask`` [N,V] (None: every knee valid): float64 [span] on the device, NaN where it does not exist
    (include/oai_hip.h has the formula; a single stratum gives the textbook one).  Does not synchronise."""
    jack, N, span = _replicate_tile(jack, "jack")
    dev = jack.device
    strata = _span_vector(strata, "strata", torch.int32, N, dev)
    v0 = int(v0)
    if mask is not None:
        mask = _chk(mask.view(torch.uint8) if mask.dtype == torch.bool else mask, "mask", torch.uint8)
        if mask.dim() != 2 or mask.shape[0] != N or mask.device != dev:
            raise ValueError(f"mask must be [{N}, V] on {dev}, got {tuple(mask.shape)} on {mask.device}")
    V = int(mask.shape[1]) if mask is not None else v0 + span
    if N < 2 or not 0 <= v0 <= V - span:
        raise ValueError(f"the jackknife tile needs N >= 2 rows and a span [{v0}, {v0 + span}) within the {V} vertices")
    if not 1 <= int(n_strata) <= 1 << 16:
        raise ValueError(f"n_strata must be 1 .. 65536, got {n_strata!r}")
    accel = torch.empty(span, dtype=torch.float64, device=dev)
    _lib.call("oai_jackknife_acceleration", jack.data_ptr(), _ptr(mask), strata.data_ptr(), N, V, v0, v0 + span, int(n_strata), accel.data_ptr(),
              _lib.STREAM, device=dev)
    return accel


# ---- rank transform (include/oai_hip.h, "Rank transform"; csrc/rank_transform.hip) ------------------------------------------------------------
OAI_RANK_PLAIN, OAI_RANK_SIGNED = 0, 1
SCORE_KINDS = {"rank": 0, "centred": 1, "normal": 2}
MAX_RANK_KNEES = 1 << 22             # a midrank up to N is exact in float32
MAX_RANK_GROUPS = 16


@dataclass
class ColumnRanks:
    """``twice_rank`` int32 [N,V]: twice the midrank of every valid entry among the valid entries of its vertex, 0 where the entry is not
    valid, negative in signed mode where the value is; ``n_valid`` int32 [V]; ``tie_term`` int64 [V], the sum over the vertex's tie
    groups of t^3 - t.  DEVICE tensors."""
    twice_rank: torch.Tensor
    n_valid: torch.Tensor
    tie_term: torch.Tensor


def _rank_tile(twice_rank: torch.Tensor):
    twice_rank = _chk(twice_rank, "twice_rank", torch.int32)
    if twice_rank.dim() != 2 or not 1 <= twice_rank.shape[0] <= MAX_RANK_KNEES or twice_rank.shape[1] < 1:
        raise ValueError(f"twice_rank must be [1 <= N <= 2^22, V >= 1], got {tuple(twice_rank.shape)}")
    return twice_rank, int(twice_rank.shape[0]), int(twice_rank.shape[1])


def column_ranks(values: torch.Tensor, mask: Optional[torch.Tensor] = None, signed: bool = False) -> ColumnRanks:
    """Per vertex the midranks of the float32 ``values`` [N,V] (knee-major) among the entries that the uint8 / bool ``mask`` [N,V] calls
    valid (None: all) and that are not NaN: see ``ColumnRanks``.  ``signed``: the ranks of |value| with the value's sign, zeros dropped
    before ranking (Wilcoxon's signed ranks).  Float ``<`` and ``==``: -0.0 ties +0.0, infinities are ordinary values.  Integer counts
    throughout: the result depends on no order.  O(N^2 V) compares.  Does not synchronise."""
    values = _chk(values, "values")
    if values.dim() != 2 or not 1 <= values.shape[0] <= MAX_RANK_KNEES or values.shape[1] < 1:
        raise ValueError(f"values must be [1 <= N <= 2^22, V >= 1], got {tuple(values.shape)}")
    mask = _stats_mask(mask, values)
    N, V, dev = int(values.shape[0]), int(values.shape[1]), values.device
    out = ColumnRanks(torch.empty((N, V), dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev),
                      torch.empty(V, dtype=torch.int64, device=dev))
    _lib.call("oai_column_ranks", values.data_ptr(), _ptr(mask), N, V, OAI_RANK_SIGNED if signed else OAI_RANK_PLAIN, out.twice_rank.data_ptr(),
              out.n_valid.data_ptr(), out.tie_term.data_ptr(), _lib.STREAM, device=dev)
    return out


def rank_sums(twice_rank: torch.Tensor, labels=None, n_groups: int = 2):
    """Per group of knees and vertex the number of valid entries and twice the sum of their |ranks|: (int32 [G,V], int64 [G,V]), DEVICE
    tensors, from the int32 ``twice_rank`` [N,V] of ``column_ranks``.  ``labels``: a HOST sequence of N integers 0 .. ``n_groups`` - 1
    (1 <= n_groups <= 16), checked before anything is launched; None: two groups by the sign of the entry, the negative ones first --
    2 W- and 2 W+ of signed ranks.  Integer sums: exact in any order.  Does not synchronise."""
    twice_rank, N, V = _rank_tile(twice_rank)
    dev, G = twice_rank.device, int(n_groups)
    if not 1 <= G <= MAX_RANK_GROUPS:
        raise ValueError(f"n_groups must be 1 .. {MAX_RANK_GROUPS}, got {n_groups!r}")
    host = None
    if labels is None:
        if G != 2:
            raise ValueError(f"without labels the two groups are the signs of the entries: n_groups must be 2, got {G}")
    else:
        lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
        if lab.shape != (N,) or lab.dtype.kind not in "iub" or (lab.astype(np.int64) < 0).any() or (lab.astype(np.int64) >= G).any():
            raise ValueError(f"labels must hold one integer 0 .. {G - 1} per knee ({N}), got {lab.dtype} {lab.shape}")
        host = np.ascontiguousarray(lab, dtype=np.uint8)
    n_g = torch.empty((G, V), dtype=torch.int32, device=dev)
    twice_sum = torch.empty((G, V), dtype=torch.int64, device=dev)
    _lib.call("oai_rank_sums", twice_rank.data_ptr(), None if host is None else host.ctypes.data, N, V, G, n_g.data_ptr(), twice_sum.data_ptr(),
              _lib.STREAM, device=dev)
    return n_g, twice_sum


def rank_scores(twice_rank: torch.Tensor, n_valid: torch.Tensor, kind: str = "rank", c: float = 0.375):
    """Scores of the ranks of ``column_ranks``: (float64 [N,V], uint8 [N,V] = the entry is valid), DEVICE tensors; 0.0 where the entry is
    not valid.  ``kind`` "rank": the midrank itself (signed ranks keep their sign); "centred": the midrank minus (n_valid + 1) / 2; both
    exact.  "normal": Phi^-1((r - c) / (n_valid - 2 c + 1)) of the midrank r, the rank-based inverse-normal transform, with ``c`` in
    [0, 1/2] -- Blom 3/8 (the default), Tukey 1/3, Bliss-Rankit 1/2, van der Waerden 0; that one is held to a tolerance against
    scipy.special.ndtri, not to the bit (include/oai_hip.h).  Does not synchronise."""
    twice_rank, N, V = _rank_tile(twice_rank)
    dev = twice_rank.device
    n_valid = _span_vector(n_valid, "n_valid", torch.int32, V, dev)
    if kind not in SCORE_KINDS:
        raise ValueError(f"kind must be one of {sorted(SCORE_KINDS)}, got {kind!r}")
    c = float(c)
    if not 0.0 <= c <= 0.5:
        raise ValueError(f"c must lie in [0, 1/2], got {c!r}")
    score = torch.empty((N, V), dtype=torch.float64, device=dev)
    mask = torch.empty((N, V), dtype=torch.uint8, device=dev)
    _lib.call("oai_rank_scores", twice_rank.data_ptr(), n_valid.data_ptr(), N, V, SCORE_KINDS[kind], c, score.data_ptr(), mask.data_ptr(), _lib.STREAM,
              device=dev)
    return score, mask


# ---- cohort PCA (include/oai_hip.h, "Cohort PCA"; csrc/cohort_pca.hip) ------------------------------------------------------------------------
DOT_CHUNK = 512                      # vertices per chunk of the ordered dot
CROSS_TILE = 64                      # edge of a workgroup's tile of rows_cross
CROSS_SPLIT_MAX_TILES = 256          # the split form of rows_cross runs up to this many tiles of the full rectangle
MAX_CROSS_ROWS = 1 << 20


def _rows_matrix(t: torch.Tensor, name: str):
    t = _chk(t, name, torch.float64)
    if t.dim() != 2 or not 1 <= t.shape[0] <= MAX_CROSS_ROWS or t.shape[1] < 1:
        raise ValueError(f"{name} must be [1 <= n <= 2^20, V >= 1], got {tuple(t.shape)}")
    return t, int(t.shape[0]), int(t.shape[1])


def cohort_whiten(values: torch.Tensor, mask: Optional[torch.Tensor], mean: torch.Tensor, root_weights: torch.Tensor, return_norm2: bool = False):
    """The whitened knees of the float32 ``values`` [N,V] (knee-major): float64 [N,V] with a_iv = (y_iv - mean_v) * root_weights_v, one
    subtraction then one product, and exactly 0.0 -- by a select -- where the uint8 / bool ``mask`` [N,V] (None: all valid) is zero, the
    value is NaN or the root weight is 0.  ``mean``, ``root_weights``: float64 [V] on the values' GPU.  ``return_norm2``: also the float64
    [N] squared norms of the rows, summed in the ordered-dot order (chunks of 512 vertices): the diagonal of ``rows_cross`` of the result.
    Does not synchronise."""
    values = _chk(values, "values")
    if values.dim() != 2 or values.shape[0] < 1 or values.shape[1] < 1:
        raise ValueError(f"values must be [N >= 1, V >= 1], got {tuple(values.shape)}")
    mask = _stats_mask(mask, values)
    N, V, dev = int(values.shape[0]), int(values.shape[1]), values.device
    mean, root_weights = _chk(mean, "mean", torch.float64), _chk(root_weights, "root_weights", torch.float64)
    for name, t in (("mean", mean), ("root_weights", root_weights)):
        _check_same_gpu("values", values, name, t)
        if tuple(t.shape) != (V,):
            raise ValueError(f"{name} must be [{V}], got {tuple(t.shape)}")
    out = torch.empty((N, V), dtype=torch.float64, device=dev)
    norm2 = torch.empty(N, dtype=torch.float64, device=dev) if return_norm2 else None
    _lib.call("oai_cohort_whiten", values.data_ptr(), _ptr(mask), mean.data_ptr(), root_weights.data_ptr(), N, V, out.data_ptr(), _ptr(norm2),
              _lib.STREAM, device=dev)
    return (out, norm2) if return_norm2 else out


def rows_cross_workspace(n_a: int, n_b: int, n_verts: int, device) -> Optional[torch.Tensor]:
    """The uint8 workspace with which ``rows_cross`` runs its split form at this shape, or None where it would walk all the same (more
    than 256 tiles of 64 x 64)."""
    ws = _lib.workspace("oai_rows_cross", device, int(n_a), int(n_b), int(n_verts))
    return ws if ws.numel() else None


def rows_cross(a: torch.Tensor, b: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 [n_a, n_b]: the ordered dot of every row of the float64 ``a`` [n_a,V] with every row of ``b`` [n_b,V] -- chunks of 512
    vertices, ascending v inside a chunk, ascending chunks, a product then an add (include/oai_hip.h).  ``b`` None: the Gram matrix of
    ``a``, of which only the tiles on or above the diagonal are computed and the rest mirrored; symmetric to the bit.  ``workspace``: a
    uint8 tensor of ``rows_cross_workspace``; with it, and at most 256 tiles, the work is split over the chunks as well (the form for a few
    hundred rows), without it one workgroup walks all chunks of a tile.  The same bits either way.  Does not synchronise."""
    a, n_a, V = _rows_matrix(a, "a")
    if b is None:
        b, n_b = a, n_a
    else:
        b, n_b, Vb = _rows_matrix(b, "b")
        _check_same_gpu("a", a, "b", b)
        if Vb != V:
            raise ValueError(f"a and b must have the same vertices, got {V} and {Vb}")
    if workspace is not None:
        workspace = _chk(workspace, "workspace", torch.uint8)
        _check_same_gpu("a", a, "workspace", workspace)
    out = torch.empty((n_a, n_b), dtype=torch.float64, device=a.device)
    _lib.call("oai_rows_cross", a.data_ptr(), n_a, b.data_ptr(), n_b, V, out.data_ptr(), _ptr(workspace), 0 if workspace is None else workspace.numel(),
              _lib.STREAM, device=a.device)
    return out


def rows_combine(coef: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """float64 [K, V]: row c is the sum over i of coef[c, i] * rows[i], in ascending i with one accumulator, a product then an add
    (include/oai_hip.h, "Ordered combine").  ``coef`` float64 [K,N], ``rows`` float64 [N,V].  Does not synchronise."""
    coef, K, N = _rows_matrix(coef, "coef")
    rows, Nr, V = _rows_matrix(rows, "rows")
    _check_same_gpu("coef", coef, "rows", rows)
    if Nr != N:
        raise ValueError(f"coef [{K}, {N}] needs {N} rows, got {Nr}")
    out = torch.empty((K, V), dtype=torch.float64, device=rows.device)
    _lib.call("oai_rows_combine", coef.data_ptr(), rows.data_ptr(), K, N, V, out.data_ptr(), _lib.STREAM, device=rows.device)
    return out
