"""Mesh / thickness step after the hot path -- the surface of oai_analysis/mesh_processing.py on the MI355X.

Reference functions mirrored (same names, argument meaning and return roles):

    get_mesh(itk_image, num_iterations=150)            mesh_processing.py:325-340   marching cubes @0.5 + smoothing
    smooth_mesh(mesh, num_iterations=150)              :298-307
    split_mesh(mesh, mesh_type="FC", on_device=False)  :353-378   inner / outer surface (KMeans on centroids + normals)
    get_distance(inner_mesh, outer_mesh)               :310-322   closest-point distance, both directions
    get_thickness_mesh(itk_image, mesh_type, ...)      :381-395
    get_cell_centroid / get_cell_normals               :26-46
    map_attributes(source_mesh, target_mesh)           :400-408   vtkPointInterpolator (radius mean, closest-point fallback)
    compute_least_square_circle(x, y)                  :411-447   circle fit (scipy leastsq in the reference)
    get_cylinder(vertice)                              :450-455
    get_projection_from_circle_and_vertice(v, circle)  :459-478
    project_thickness(mapped_mesh, mesh_type="FC")     :483-534   2-D atlas thickness map (FC: cylinder angle; TC: plateau PCA)

vtk / trimesh / skimage are not installed here, so meshes are ``Mesh`` objects (float32 vertices [n,3] in (x,y,z)*spacing,
int32 faces [m,3], per-point data) instead of ``vtkPolyData``; ``Mesh.to_vtk()`` adapts when vtk imports.  The three heavy
steps run in HIP kernels behind the C ABI (oai_mc_*, oai_mesh_smooth, oai_mesh_point_distance; csrc/mesh.hip); the edge
graph and the connected-component filter (> 3000 cells, :119-137) are host logic.  The KMeans split has two paths: by default
the reference's own host code under the installed sklearn (its own dependency); with ``on_device=True`` csrc/mesh_split.hip
(oai_mesh_split_*, oai_mesh_submesh) restates sklearn >= 1.4's KMeans in fp64 and builds both sub-meshes on the GPU, pinned face for
face against the reference's split functions (tests/golden/mesh_split.npz); it does not import sklearn.  Marching cubes, smoothing
and distance are unpinned: see oracle/mesh.py for what is restated.  The atlas thickness map runs in csrc/thickness_map.hip (oai_map_attributes*, oai_fit_circle, oai_project_circle,
oai_project_plateaus): project_thickness and its circle helpers are pinned against the reference's own functions
(tests/golden/thickness_projection.npz); map_attributes restates vtkPointInterpolator's defaults and is unpinned.  There is no CPU
fallback for the kernels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .image import as_image


@dataclass
class Mesh:
    verts: np.ndarray                       # float32 [n,3], (x,y,z) in the image's spacing units
    faces: np.ndarray                       # int32 [m,3]
    point_data: Dict[str, np.ndarray] = field(default_factory=dict)

    def GetNumberOfPoints(self) -> int:      # the vtkPolyData calls the reference makes on meshes
        return len(self.verts)

    def GetNumberOfCells(self) -> int:
        return len(self.faces)

    def GetBounds(self):
        lo, hi = self.verts.min(axis=0), self.verts.max(axis=0)
        return (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])

    def to_vtk(self):  # pragma: no cover - vtk is absent in this environment
        import vtk
        from vtk.util import numpy_support as ns
        cells = vtk.vtkCellArray()
        cells.SetData(ns.numpy_to_vtk(np.arange(0, 3 * len(self.faces) + 1, 3).astype("int")), ns.numpy_to_vtk(self.faces.reshape(-1).astype("int")))
        pts = vtk.vtkPoints()
        pts.SetData(ns.numpy_to_vtk(self.verts.astype(np.float64), deep=True))
        out = vtk.vtkPolyData()
        out.SetPoints(pts)
        out.SetPolys(cells)
        for name, arr in self.point_data.items():
            a = ns.numpy_to_vtk(np.asarray(arr, np.float64), deep=True)
            a.SetName(name)
            out.GetPointData().AddArray(a)
        return out


def _dev(a: np.ndarray, dtype) -> torch.Tensor:
    if not torch.cuda.is_available():
        raise RuntimeError("oai_analysis_2_amd.mesh_processing runs on the GPU only (no CPU fallback)")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---- marching cubes ----------------------------------------------------------------------------------------------------------
def marching_cubes(volume_zyx, level: float = 0.5, spacing_xyz=(1.0, 1.0, 1.0)) -> Tuple[np.ndarray, np.ndarray]:
    """(verts, faces) of the iso-surface; ``volume_zyx`` may be a numpy array or a float32 torch tensor already on the device."""
    lib = _lib.load()
    vol = volume_zyx if isinstance(volume_zyx, torch.Tensor) else _dev(np.asarray(volume_zyx), np.float32)
    vol = vol.to(torch.float32).contiguous()
    if not vol.is_cuda:
        vol = vol.cuda()
    D, H, W = (int(v) for v in vol.shape)
    ws = torch.empty(int(lib.oai_mc_workspace_bytes(D, H, W)), dtype=torch.uint8, device=vol.device)
    nv, nt = C.c_longlong(), C.c_longlong()
    with torch.cuda.device(vol.device):
        _lib.check(lib.oai_mc_count(vol.data_ptr(), D, H, W, float(level), ws.data_ptr(), ws.numel(), C.byref(nv), C.byref(nt), _stream()),
                   "oai_mc_count")
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=vol.device)
        faces = torch.empty((nt.value, 3), dtype=torch.int32, device=vol.device)
        sp = (C.c_float * 3)(*[float(v) for v in spacing_xyz])
        _lib.check(lib.oai_mc_emit(vol.data_ptr(), D, H, W, float(level), sp, ws.data_ptr(), verts.data_ptr(), faces.data_ptr(), _stream()),
                   "oai_mc_emit")
    return verts.cpu().numpy(), faces.cpu().numpy()


# ---- host-side graph helpers -------------------------------------------------------------------------------------------------
def vertex_adjacency(n_verts: int, faces: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """CSR edge graph (offsets [n+1], neighbours ascending, no duplicates)."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.concatenate([e, e[:, ::-1]])
    key = np.unique(e[:, 0] * n_verts + e[:, 1])
    src, dst = key // n_verts, key % n_verts
    off = np.zeros(n_verts + 1, dtype=np.int64)
    np.add.at(off, src + 1, 1)
    return np.cumsum(off).astype(np.int32), dst.astype(np.int32)


def keep_large_regions(verts: np.ndarray, faces: np.ndarray, min_cells: int = 3000) -> Tuple[np.ndarray, np.ndarray]:
    """get_vtk_mesh's vtkPolyDataConnectivityFilter loop (mesh_processing.py:114-141): keep connected regions with more than
    ``min_cells`` triangles, drop unreferenced points."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(verts)
    if len(faces) == 0:
        return verts[:0], faces
    f = faces.astype(np.int64)
    g = coo_matrix((np.ones(2 * len(f), np.int8), (np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]]))), shape=(n, n))
    _, label = connected_components(g, directed=False)
    face_label = label[f[:, 0]]
    cells = np.bincount(face_label, minlength=label.max() + 1)
    keep_face = cells[face_label] > min_cells
    f = f[keep_face]
    used = np.zeros(n, dtype=bool)
    used[f.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return verts[used], remap[f].astype(np.int32)


def smooth_mesh(input_mesh: Mesh, num_iterations: int = 150, relaxation_factor: float = 0.01) -> Mesh:
    """vtkSmoothPolyDataFilter with its defaults (relaxation 0.01, boundary smoothing on, no feature edges)."""
    lib = _lib.load()
    n = len(input_mesh.verts)
    if n == 0 or num_iterations <= 0:
        return Mesh(input_mesh.verts.copy(), input_mesh.faces.copy(), dict(input_mesh.point_data))
    off, nbr = vertex_adjacency(n, input_mesh.faces)
    v_in, d_off, d_nbr = _dev(input_mesh.verts, np.float32), _dev(off, np.int32), _dev(nbr, np.int32)
    tmp, out = torch.empty_like(v_in), torch.empty_like(v_in)
    with torch.cuda.device(v_in.device):
        _lib.check(lib.oai_mesh_smooth(v_in.data_ptr(), n, d_off.data_ptr(), d_nbr.data_ptr(), int(num_iterations), float(relaxation_factor),
                                       tmp.data_ptr(), out.data_ptr(), _stream()), "oai_mesh_smooth")
    return Mesh(out.cpu().numpy(), input_mesh.faces.copy(), dict(input_mesh.point_data))


def get_mesh(itk_image, num_iterations: int = 150, min_cells: int = 3000) -> Mesh:
    """mesh_processing.py:325-340: iso-surface of the probability map at 0.5 in (x,y,z)*spacing, small regions dropped
    (get_vtk_mesh), then smoothed."""
    img = as_image(itk_image)
    verts, faces = marching_cubes(np.asarray(img.array, dtype=np.float32), 0.5, img.spacing)
    verts, faces = keep_large_regions(verts, faces, min_cells)
    return smooth_mesh(Mesh(verts, faces), num_iterations=num_iterations)


# ---- per-cell attributes (trimesh in the reference) ------------------------------------------------------------------------------
def get_cell_centroid(mesh: Mesh) -> np.ndarray:
    v = mesh.verts.astype(np.float64)
    return v[mesh.faces].sum(axis=1) / 3.0


def get_cell_normals(mesh: Mesh) -> np.ndarray:
    v = mesh.verts.astype(np.float64)
    a, b, c = v[mesh.faces[:, 0]], v[mesh.faces[:, 1]], v[mesh.faces[:, 2]]
    n = np.cross(b - a, c - a)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return n / np.where(length > 0, length, 1.0)


def get_sub_mesh(mesh: Mesh, face_list: np.ndarray) -> Mesh:
    """get_vtk_sub_mesh (:150-194): the selected faces with points renumbered in order of first use."""
    f = mesh.faces[np.asarray(face_list, dtype=np.int64)]
    flat = f.reshape(-1)
    uniq, first = np.unique(flat, return_index=True)
    order = uniq[np.argsort(first)]
    remap = np.full(len(mesh.verts), -1, dtype=np.int64)
    remap[order] = np.arange(len(order))
    return Mesh(mesh.verts[order], remap[f].astype(np.int32))


def split_tibial_cartilage_surface(mesh: Mesh, mesh_normals, mesh_centroids):
    """mesh_processing.py:197-223"""
    from sklearn.cluster import KMeans
    cn = (mesh_centroids - np.mean(mesh_centroids, axis=0)) / (np.max(mesh_centroids, axis=0) - np.min(mesh_centroids, axis=0))
    features = np.concatenate((cn * 1, mesh_normals * 10), axis=1)
    labels = KMeans(n_clusters=2, algorithm="lloyd", random_state=5).fit(features).labels_
    io = labels * 2 - 1
    if mesh_normals[io == -1, 1].mean() < 0:
        io = -io
    inner, outer = np.where(io == -1)[0], np.where(io == 1)[0]
    return get_sub_mesh(mesh, inner), get_sub_mesh(mesh, outer), inner, outer


def cluster_and_segment(mesh_centroids_normalized, face_normal_value, dot_output):
    """mesh_processing.py:227-240"""
    from sklearn.cluster import KMeans
    features = np.concatenate((mesh_centroids_normalized * 1, face_normal_value, dot_output), axis=1)
    labels = KMeans(n_clusters=2, algorithm="lloyd", n_init=5, random_state=5).fit(features).labels_ * 2 - 1
    if face_normal_value[labels == -1, 1].mean() < 0:
        labels = -labels
    return labels


def split_femoral_cartilage_surface(mesh: Mesh, face_normal, face_centroid, num_divisions: int = 3):
    """mesh_processing.py:243-294: KMeans per x-slab on (centroid, normal, (bbox centre - centroid) * normal)"""
    cn = (face_centroid - np.mean(face_centroid, axis=0)) / (np.max(face_centroid, axis=0) - np.min(face_centroid, axis=0))
    xmin, xmax, ymin, ymax, zmin, zmax = mesh.GetBounds()
    center = (np.array([xmin, ymin, zmin]) + np.array([xmax, ymax, zmax])) / 2
    dot_output = np.multiply(center - face_centroid, face_normal)
    x_coord = cn[:, 0]
    io = np.zeros(cn.shape[0])
    min_x, max_x = np.min(x_coord), np.max(x_coord)
    step = (max_x - min_x) / num_divisions
    for i in range(num_divisions):
        lower = min_x + step * i
        idx = np.where((x_coord >= lower) & (x_coord < lower + step))[0]
        if len(idx) < 2:
            continue
        np.put(io, idx, cluster_and_segment(cn[idx], face_normal[idx], dot_output[idx]))
    inner, outer = np.where(io == -1)[0], np.where(io == 1)[0]
    return get_sub_mesh(mesh, inner), get_sub_mesh(mesh, outer), inner, outer


# ---- the same split on the device (csrc/mesh_split.hip) -------------------------------------------------------------------------
_MESH_TYPE = {"FC": 0, "TC": 1}
_N_INIT = {"FC": 5, "TC": 1}                 # cluster_and_segment: n_init=5; the TC fit: n_init="auto" = 1 run (sklearn >= 1.4)
_KMEANS_SEED, _KMEANS_MAX_ITER = 5, 300


@dataclass
class DeviceSplit:
    """What the device split leaves on the GPU: the mesh, side per face (int8: -1 inner, +1 outer, 0 in no FC slab), the per-face
    centroids / normals (fp64, bit-identical to get_cell_centroid / get_cell_normals) and each fit's iteration count (best run)."""
    verts: torch.Tensor
    faces: torch.Tensor
    side: torch.Tensor
    centroids: torch.Tensor
    normals: torch.Tensor
    n_iter: np.ndarray


def _kmeans_draws(counts, n_init: int, seed: int = _KMEANS_SEED):
    """The random numbers sklearn's KMeans(random_state=seed).fit draws on an n-sample slab, fit by fit: per init, the first
    k-means++ centre rs.choice(n, p=w / w.sum()) with w = ones(n), then rs.uniform(size=2) for the two local trials."""
    first, uni = [], []
    for n in counts:
        n = int(n)
        if n < 2:
            raise ValueError(f"n_samples={n} should be >= n_clusters=2.")
        rs = np.random.RandomState(seed)
        w = np.ones(n, dtype=np.float64)
        for _ in range(n_init):
            first.append(int(rs.choice(n, p=w / w.sum())))
            uni.extend(float(u) for u in rs.uniform(size=2))
    return first, uni


def split_mesh_device(mesh: Mesh, mesh_type: str = "FC") -> DeviceSplit:
    """The KMeans labelling of split_femoral_cartilage_surface (FC) / split_tibial_cartilage_surface (anything else) on the GPU.
    A slab with fewer than 2 faces raises the ValueError sklearn raises, as the reference does; the host path of this package skips
    such an FC slab instead (its faces keep side 0)."""
    lib = _lib.load()
    kind = "FC" if mesh_type == "FC" else "TC"
    nv, nf = len(mesh.verts), len(mesh.faces)
    if nf < 2:
        raise ValueError(f"n_samples={nf} should be >= n_clusters=2.")
    v, f = _dev(mesh.verts.reshape(-1, 3), np.float32), _dev(mesh.faces.reshape(-1, 3), np.int32)
    ws = torch.empty(int(lib.oai_mesh_split_workspace_bytes(nv, nf, _MESH_TYPE[kind], _N_INIT[kind])), dtype=torch.uint8, device=v.device)
    cent = torch.empty((nf, 3), dtype=torch.float64, device=v.device)
    nrm = torch.empty((nf, 3), dtype=torch.float64, device=v.device)
    side = torch.empty(nf, dtype=torch.int8, device=v.device)
    counts = (C.c_longlong * 3)()
    with torch.cuda.device(v.device):
        _lib.check(lib.oai_mesh_split_features(v.data_ptr(), nv, f.data_ptr(), nf, _MESH_TYPE[kind], ws.data_ptr(), ws.numel(), cent.data_ptr(),
                                               nrm.data_ptr(), counts, _stream()), "oai_mesh_split_features")
        n_slabs = 3 if kind == "FC" else 1
        first, uni = _kmeans_draws(list(counts)[:n_slabs], _N_INIT[kind])
        n_iter = (C.c_int * 3)()
        _lib.check(lib.oai_mesh_split_kmeans(nf, _MESH_TYPE[kind], ws.data_ptr(), ws.numel(), nrm.data_ptr(), _N_INIT[kind], _KMEANS_MAX_ITER, counts,
                                             (C.c_longlong * len(first))(*first), (C.c_double * len(uni))(*uni), side.data_ptr(), n_iter, _stream()),
                   "oai_mesh_split_kmeans")
    return DeviceSplit(v, f, side, cent, nrm, np.array(list(n_iter)[:n_slabs], dtype=np.int64))


def get_sub_mesh_device(split: DeviceSplit, which: int) -> Tuple[Mesh, np.ndarray]:
    """get_sub_mesh(mesh, np.where(side == which)[0]) built on the GPU: (sub-mesh, face list)."""
    lib = _lib.load()
    nv, nf = int(split.verts.shape[0]), int(split.faces.shape[0])
    dev = split.verts.device
    ws = torch.empty(int(lib.oai_mesh_submesh_workspace_bytes(nv, nf)), dtype=torch.uint8, device=dev)
    vo = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    fo = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    io = torch.empty(nf, dtype=torch.int32, device=dev)
    n_v, n_f = C.c_longlong(), C.c_longlong()
    with torch.cuda.device(dev):
        _lib.check(lib.oai_mesh_submesh(split.verts.data_ptr(), nv, split.faces.data_ptr(), nf, split.side.data_ptr(), int(which), ws.data_ptr(),
                                        ws.numel(), vo.data_ptr(), fo.data_ptr(), io.data_ptr(), C.byref(n_v), C.byref(n_f), _stream()),
                   "oai_mesh_submesh")
    return (Mesh(vo[:n_v.value].cpu().numpy(), fo[:n_f.value].cpu().numpy()), io[:n_f.value].cpu().numpy().astype(np.int64))


def _split_surface_device(mesh: Mesh, mesh_type: str):
    sp = split_mesh_device(mesh, mesh_type)
    inner, inner_list = get_sub_mesh_device(sp, -1)
    outer, outer_list = get_sub_mesh_device(sp, 1)
    return inner, outer, inner_list, outer_list


def split_femoral_cartilage_surface_device(mesh: Mesh):
    """split_femoral_cartilage_surface (:243-294) on the GPU: (inner mesh, outer mesh, inner face list, outer face list)."""
    return _split_surface_device(mesh, "FC")


def split_tibial_cartilage_surface_device(mesh: Mesh):
    """split_tibial_cartilage_surface (:197-223) on the GPU: (inner mesh, outer mesh, inner face list, outer face list)."""
    return _split_surface_device(mesh, "TC")


def split_mesh(mesh: Mesh, mesh_type: str = "FC", on_device: bool = False) -> Tuple[Mesh, Mesh]:
    """mesh_processing.py:353-378.  ``on_device``: the KMeans split and both sub-meshes on the GPU (sklearn >= 1.4 semantics,
    split_femoral_cartilage_surface_device / split_tibial_cartilage_surface_device); the default is the reference's host code.
    One difference besides the sklearn version: an FC slab with fewer than 2 faces raises ValueError on the device path (as the
    reference's KMeans does), where the host path skips the slab and leaves its faces in neither sub-mesh."""
    if on_device:
        inner, outer, _, _ = _split_surface_device(mesh, mesh_type)
        return inner, outer
    normals, centroids = get_cell_normals(mesh), get_cell_centroid(mesh)
    if mesh_type == "FC":
        inner, outer, _, _ = split_femoral_cartilage_surface(mesh, normals, centroids)
    else:
        inner, outer, _, _ = split_tibial_cartilage_surface(mesh, normals, centroids)
    return inner, outer


# ---- thickness -----------------------------------------------------------------------------------------------------------------
def point_distance(points: np.ndarray, mesh: Mesh, broad_phase: bool = True) -> np.ndarray:
    """Unsigned distance from each point to the mesh surface.  ``broad_phase``: bin the triangles into a uniform grid whose cell is
    the longest triangle edge (>= 2 voxels' worth) so that a point only tests the triangles around it; False = brute force."""
    lib = _lib.load()
    p, v, f = _dev(points, np.float32), _dev(mesh.verts, np.float32), _dev(mesh.faces, np.int32)
    out = torch.empty(len(points), dtype=torch.float32, device=p.device)
    with torch.cuda.device(p.device):
        if broad_phase and len(mesh.faces) > 0:
            tri = mesh.verts[mesh.faces].astype(np.float64)
            edge = max(np.linalg.norm(tri[:, 0] - tri[:, 1], axis=1).max(), np.linalg.norm(tri[:, 1] - tri[:, 2], axis=1).max(),
                       np.linalg.norm(tri[:, 2] - tri[:, 0], axis=1).max())
            lo, hi = mesh.verts.min(axis=0).astype(np.float64), mesh.verts.max(axis=0).astype(np.float64)
            h = max(float(edge) * 1.0001, float((hi - lo).max()) / 512.0, 1e-6)              # at most 512 cells per axis
            dims = np.maximum(np.ceil((hi - lo) / h).astype(np.int64) + 1, 1)
            glo = (C.c_float * 3)(*[float(x) for x in lo - 0.5 * h * 1e-3])
            gd = (C.c_int * 3)(*[int(x) for x in dims])
            ws = torch.empty(int(lib.oai_mesh_grid_workspace_bytes(gd, len(mesh.faces))), dtype=torch.uint8, device=p.device)
            _lib.check(lib.oai_mesh_point_distance_grid(p.data_ptr(), len(points), v.data_ptr(), f.data_ptr(), len(mesh.faces), glo, float(h), gd,
                                                        ws.data_ptr(), ws.numel(), out.data_ptr(), _stream()), "oai_mesh_point_distance_grid")
        else:
            _lib.check(lib.oai_mesh_point_distance(p.data_ptr(), len(points), v.data_ptr(), f.data_ptr(), len(mesh.faces), out.data_ptr(), _stream()),
                       "oai_mesh_point_distance")
    return out.cpu().numpy()


def get_distance(inner_mesh: Mesh, outer_mesh: Mesh) -> Tuple[Mesh, Mesh]:
    """vtkDistancePolyDataFilter (:310-322): every point of each mesh gets the unsigned distance to the other mesh's surface
    as point data "Distance"."""
    d_in = point_distance(inner_mesh.verts, outer_mesh)
    d_out = point_distance(outer_mesh.verts, inner_mesh)
    return (Mesh(inner_mesh.verts, inner_mesh.faces, {**inner_mesh.point_data, "Distance": d_in}),
            Mesh(outer_mesh.verts, outer_mesh.faces, {**outer_mesh.point_data, "Distance": d_out}))


def get_thickness_mesh(itk_image, mesh_type: str = "FC", num_iterations: int = 150, min_cells: int = 3000,
                       split_on_device: bool = False) -> Tuple[Mesh, Mesh]:
    """mesh_processing.py:381-395 (which, like this, always smooths with 150 iterations).  ``split_on_device``: see split_mesh (it
    raises ValueError on a mesh with an FC slab of fewer than 2 faces, which the default path skips)."""
    mesh = get_mesh(itk_image, num_iterations=150, min_cells=min_cells)
    inner, outer = split_mesh(mesh, mesh_type, on_device=split_on_device)
    return get_distance(inner, outer)


# ---- atlas thickness map (mesh_processing.py:400-534) ----------------------------------------------------------------------------
def _point_arrays(mesh: Mesh) -> Tuple[list, np.ndarray]:
    """The mesh's point arrays as float32 component rows [n_comp][n] and (name, shape) of each array."""
    n = len(mesh.verts)
    names, rows = [], []
    for name, arr in mesh.point_data.items():
        a = np.asarray(arr)
        if a.shape[:1] != (n,):
            raise ValueError(f"point array {name!r} has shape {a.shape}, the mesh has {n} points")
        names.append((name, a.shape))
        rows.append(a.reshape(n, -1).T.astype(np.float32))
    return names, (np.concatenate(rows, axis=0) if rows else np.zeros((0, n), np.float32))


def map_attributes(source_mesh: Mesh, target_mesh: Mesh, radius: float = 1.0, broad_phase: bool = True) -> Mesh:
    """mesh_processing.py:400-408: vtkPointInterpolator(SetNullPointsStrategyToClosestPoint), source arrays onto target points.

    Restated from VTK 9's documented defaults (vtk is not installed here; this half of the step is unpinned): vtkLinearKernel,
    the RADIUS footprint, Radius = 1.0, NormalizeWeights on.  For each target point, every source point array takes the unweighted
    mean over the source points with ``|p - q|^2 <= radius^2``; with no source point that close, the value of the closest source
    point (ties: the smallest index).  Sums are fp64, results float32 (as get_distance).  The output has the target's verts, faces
    and point data plus the interpolated source arrays; on a name clash the source array wins.  ``broad_phase``: bin the source
    points into a uniform grid (cells >= radius, at most 512 per axis); False = brute force over every source point (same result).
    """
    lib = _lib.load()
    if len(source_mesh.verts) == 0:
        raise ValueError("map_attributes: the source mesh has no points")
    names, vals = _point_arrays(source_mesh)
    out_data = dict(target_mesh.point_data)
    n_tgt, n_src, n_comp = len(target_mesh.verts), len(source_mesh.verts), vals.shape[0]
    if n_comp == 0:
        return Mesh(target_mesh.verts, target_mesh.faces, out_data)
    s, v, t = _dev(source_mesh.verts, np.float32), _dev(vals, np.float32), _dev(target_mesh.verts.reshape(-1, 3), np.float32)
    out = torch.empty((n_comp, n_tgt), dtype=torch.float32, device=s.device)
    with torch.cuda.device(s.device):
        if broad_phase:
            lo = source_mesh.verts.min(axis=0).astype(np.float64)
            hi = source_mesh.verts.max(axis=0).astype(np.float64)
            h = max(float(radius) * 1.0001, float((hi - lo).max()) / 512.0, 1e-6)          # at most 512 cells per axis
            dims = np.maximum(np.ceil((hi - lo) / h).astype(np.int64) + 1, 1)
            glo = (C.c_double * 3)(*[float(x) for x in lo - 0.5 * h * 1e-3])
            gd = (C.c_int * 3)(*[int(x) for x in dims])
            ws = torch.empty(int(lib.oai_point_grid_workspace_bytes(gd, n_src)), dtype=torch.uint8, device=s.device)
            _lib.check(lib.oai_map_attributes_grid(s.data_ptr(), n_src, v.data_ptr(), n_comp, t.data_ptr(), n_tgt, float(radius), glo, float(h), gd,
                                                   ws.data_ptr(), ws.numel(), out.data_ptr(), _stream()), "oai_map_attributes_grid")
        else:
            _lib.check(lib.oai_map_attributes(s.data_ptr(), n_src, v.data_ptr(), n_comp, t.data_ptr(), n_tgt, float(radius), out.data_ptr(), _stream()),
                       "oai_map_attributes")
    res = out.cpu().numpy()
    row = 0
    for name, shape in names:
        k = int(np.prod(shape[1:], dtype=np.int64))
        out_data[name] = res[row:row + k].T.reshape((n_tgt,) + tuple(shape[1:]))
        row += k
    return Mesh(target_mesh.verts, target_mesh.faces, out_data)


def _fit_circle_dev(pts: torch.Tensor, col_x: int, col_y: int) -> Tuple[np.ndarray, float]:
    lib = _lib.load()
    n = int(pts.shape[0])
    ws = torch.empty(max(int(lib.oai_thickness_map_workspace_bytes(n)), 1), dtype=torch.uint8, device=pts.device)
    centre, radius, its = (C.c_double * 2)(), C.c_double(), C.c_int()
    with torch.cuda.device(pts.device):
        _lib.check(lib.oai_fit_circle(pts.data_ptr(), n, col_x, col_y, ws.data_ptr(), ws.numel(), centre, C.byref(radius), C.byref(its), _stream()),
                   "oai_fit_circle")
    return np.array([centre[0], centre[1]], dtype=np.float64), float(radius.value)


def compute_least_square_circle(x, y) -> Tuple[np.ndarray, float]:
    """mesh_processing.py:411-447: the centre minimising sum (R_i - mean R)^2 and the mean radius R = mean R_i.

    The reference runs scipy leastsq with the centred Jacobian from the centroid; this is Gauss-Newton with step halving on the
    2x2 normal equations from the centroid, fp64 sums on the device (the points are taken as float32, the mesh's precision).
    Returns (centre float64 [2], R float64)."""
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    if x.shape != y.shape:
        raise ValueError("compute_least_square_circle: x and y differ in length")
    pts = np.zeros((len(x), 3), np.float32)
    pts[:, 0], pts[:, 1] = x, y
    centre, r = _fit_circle_dev(_dev(pts, np.float32), 0, 1)
    return centre, np.float64(r)


def get_cylinder(vertice):
    """mesh_processing.py:450-455: ((centre, r), (z_min, z_max)) of the circle fitted to columns 0 and 1."""
    v = np.asarray(vertice)
    centre, r = compute_least_square_circle(v[:, 0], v[:, 1])
    return (centre, r), (np.min(v[:, 2]), np.max(v[:, 2]))


def _project_circle_dev(pts: torch.Tensor, col_x: int, col_y: int, centre) -> Tuple[np.ndarray, np.ndarray]:
    lib = _lib.load()
    n = int(pts.shape[0])
    angle = torch.empty(n, dtype=torch.float64, device=pts.device)
    z = torch.empty(n, dtype=torch.float64, device=pts.device)
    c = (C.c_double * 2)(float(centre[0]), float(centre[1]))
    with torch.cuda.device(pts.device):
        _lib.check(lib.oai_project_circle(pts.data_ptr(), n, col_x, col_y, c, angle.data_ptr(), z.data_ptr(), _stream()), "oai_project_circle")
    return angle.cpu().numpy(), z.cpu().numpy()


def get_projection_from_circle_and_vertice(vertice, circle) -> Tuple[np.ndarray, np.ndarray]:
    """mesh_processing.py:459-478: embedded [n,2] = (atan2(y - c_y, x - c_x), z) (computed on the device in fp64) and plot_xy [n,2],
    the angle in degrees rescaled to 1.5 x the z range (host)."""
    v = np.asarray(vertice)
    centre, _ = circle
    angle, z = _project_circle_dev(_dev(v, np.float32), 0, 1, centre)
    embedded = np.stack([angle, z], axis=1)
    deg = angle / np.pi * 180
    zz = v[:, 2]
    deg = (deg - np.min(deg)) / (np.max(deg) - np.min(deg))
    plot_xy = np.zeros_like(embedded)
    plot_xy[:, 0] = deg * (np.max(zz) - np.min(zz)) * 1.5 + np.min(zz)
    plot_xy[:, 1] = zz
    return embedded, plot_xy


def project_thickness(mapped_mesh: Mesh, mesh_type: str = "FC", embedded=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """mesh_processing.py:483-534: the 2-D thickness map of a mesh mapped to the atlas.  Returns float64 (x, y, thickness).

    The thickness is ``point_data["Distance"]``, else the mesh's only point array.  ``embedded`` is unused, as in the reference.
    FC: columns x and y swapped, circle fitted (compute_least_square_circle); x = atan2(y - c_y, x - c_x), y = z, thickness in point
    order.  TC: plateaus split at z < 50 (raw units); per plateau the centred scores on the top-2 axes of its 3x3 scatter matrix
    (equal to the reference's KernelPCA(n_components=2), linear kernel, which builds an n x n kernel matrix), each axis signed as
    sklearn's svd_flip(u) does (the point with the largest |score| scores positive, first index on a tie); the left plateau rotated
    by -50 degrees, the right one by -160 degrees with x negated and 50 added to y; the right plateau's points first.  An empty
    plateau raises ValueError (the reference crashes there)."""
    lib = _lib.load()
    if "Distance" in mapped_mesh.point_data:
        thickness = np.asarray(mapped_mesh.point_data["Distance"])
    elif len(mapped_mesh.point_data) == 1:
        thickness = np.asarray(next(iter(mapped_mesh.point_data.values())))
    else:
        raise ValueError(f"project_thickness: no 'Distance' array and not exactly one point array ({sorted(mapped_mesh.point_data)})")
    verts = np.asarray(mapped_mesh.verts)
    n = len(verts)
    if thickness.shape != (n,):
        raise ValueError(f"project_thickness: the thickness has shape {thickness.shape}, the mesh has {n} points")
    pts = _dev(verts, np.float32)
    if mesh_type == "FC":
        centre, _ = _fit_circle_dev(pts, 1, 0)                        # vertices[:, [1, 0]] = vertices[:, [0, 1]]
        angle, z = _project_circle_dev(pts, 1, 0, centre)
        return angle, z, thickness.astype(np.float64)
    z = verts[:, 2].astype(np.float32)
    if not (z >= 50).any() or not (z < 50).any():
        raise ValueError("project_thickness(TC): one tibial plateau is empty (no point with z < 50 or none with z >= 50)")
    th = _dev(thickness, np.float32)
    ws = torch.empty(int(lib.oai_thickness_map_workspace_bytes(n)), dtype=torch.uint8, device=pts.device)
    out = torch.empty((3, n), dtype=torch.float64, device=pts.device)
    n_right, n_left = C.c_longlong(), C.c_longlong()
    with torch.cuda.device(pts.device):
        _lib.check(lib.oai_project_plateaus(pts.data_ptr(), th.data_ptr(), n, ws.data_ptr(), ws.numel(), out[0].data_ptr(), out[1].data_ptr(),
                                            out[2].data_ptr(), C.byref(n_right), C.byref(n_left), _stream()), "oai_project_plateaus")
    res = out[:, :n_right.value + n_left.value].cpu().numpy()
    return res[0].copy(), res[1].copy(), res[2].copy()
