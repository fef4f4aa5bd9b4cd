"""Mesh / thickness step after the hot path -- the surface of oai_analysis/mesh_processing.py on the MI355X.

Reference functions mirrored (same names, argument meaning and return roles):

    get_mesh(itk_image, num_iterations=150)            mesh_processing.py:325-340   marching cubes @0.5 + smoothing
    get_mesh_from_probability_map(image)               :343-350   itk cuberille @0.5, vertices projected to the iso-surface
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
    transform_mesh(mesh, transform, ...)               --         mesh vertices pushed through phi, atlas -> patient space
    mesh_point_affines(image_A, image_B, net_shape)    --         the two affine legs around phi for points, fp64 on the host

transform_mesh has no line in the reference: it would do this step with itk.transform_mesh_filter and the registration's composite
transform, if at all.  It is restated from ITK's documented composite-transform behaviour and unpinned, like the resample
(oracle/resample.py); the kernel is csrc/mesh_transform.hip (oai_transform_points_through_phi), restated in fp64 in
tests/mesh_transform_ref.py, and _transform_points_dev is its device-tensor form for the resident chain of thickness.py.

vtk / trimesh / skimage are not installed here, so meshes are ``Mesh`` objects (float32 vertices [n,3] in (x,y,z)*spacing,
int32 faces [m,3], per-point data) instead of ``vtkPolyData``; ``Mesh.to_vtk()`` adapts when vtk imports.  The three heavy
steps run in HIP kernels behind the C ABI (oai_mc_*, oai_mesh_smooth, oai_mesh_point_distance; csrc/mesh.hip); by default the edge
graph and the connected-component filter (> 3000 cells, :119-137) are host logic.  ``get_mesh(on_device=True)`` /
``get_thickness_mesh(on_device=True)`` run them on the GPU too (csrc/mesh_graph.hip: oai_mesh_components, oai_mesh_keep_large_regions,
oai_mesh_adjacency, oai_mesh_grid_params), so the whole thickness step stays resident until its result; bit-identical to the host
graph code and to ``split_on_device=True``.  The KMeans split has two paths: by default
the reference's own host code under the installed sklearn (its own dependency); with ``on_device=True`` csrc/mesh_split.hip
(oai_mesh_split_*, oai_mesh_submesh) restates sklearn >= 1.4's KMeans in fp64 and builds both sub-meshes on the GPU, pinned face for
face against the reference's split functions (tests/golden/mesh_split.npz); it does not import sklearn.  Marching cubes, smoothing
and distance are unpinned: see oracle/mesh.py for what is restated.  The atlas thickness map runs in csrc/thickness_map.hip (oai_map_attributes*, oai_fit_circle, oai_project_circle,
oai_project_plateaus): project_thickness and its circle helpers are pinned against the reference's own functions
(tests/golden/thickness_projection.npz); map_attributes restates vtkPointInterpolator's defaults and is unpinned.
get_mesh_from_probability_map restates itk.cuberille_image_to_mesh_filter in csrc/cuberille.hip (oai_cuberille_*; unpinned)
and returns ITK's physical points.  The thickness image (thickness_image_build / thickness_image; csrc/thickness_image.hip, oai_thickness_image_*)
rasterises a projected mesh once -- per pixel the smallest covering face index, its corners and barycentric weights, restated in
tests/thickness_image_ref.py -- and gathers per-point values through it; _map_attributes_dev / _thickness_inner_dev are the device-tensor
forms of map_attributes and of get_thickness_mesh's resident branch (inner mesh and inner -> outer distance only) that thickness.py chains
without downloads.  mesh_areas (per-face and per-vertex area, csrc/morphometry.hip) and point_footprint (what map_attributes saw of the source points:
the count inside the radius, the nearest distance and index) have no line in the reference either; thickness.py builds the per-knee morphometry on
them.  mesh_topology, mesh_geometry and mesh_self_intersections (csrc/mesh_quality.hip) ask the questions of qc.mesh_quality about any mesh: edge
classes and their counts, area / volume / triangle quality, faces that pass through each other; unpinned too.  There is no CPU fallback for the kernels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from .image import as_image
from .registration import DisplacementTransform, resample_affines


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


def _dev(a, dtype, tail=(), device=None) -> torch.Tensor:
    """An array or a tensor as a contiguous device tensor of the numpy ``dtype``, reshaped to [-1, *tail] when ``tail`` is given.  An
    array is converted on the host and uploaded; a tensor that is already on a GPU stays there unless ``device`` names another."""
    if not torch.cuda.is_available():
        raise RuntimeError("oai_analysis_2_amd.mesh_processing runs on the GPU only (no CPU fallback)")
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))
    if device is not None or not t.is_cuda:
        t = t.to(device if device is not None else "cuda")
    t = t.to(getattr(torch, np.dtype(dtype).name))
    return (t.reshape(-1, *tail) if tail else t).contiguous()


# ---- marching cubes ----------------------------------------------------------------------------------------------------------
def _marching_cubes_dev(vol: torch.Tensor, level: float, spacing_xyz) -> Tuple[torch.Tensor, torch.Tensor]:
    """(verts float32 [n,3], faces int32 [m,3]) of the iso-surface, left on the volume's device."""
    vol = _dev(vol, np.float32)
    D, H, W = (int(v) for v in vol.shape)
    ws = _lib.workspace("oai_mc", vol.device, D, H, W)
    nv, nt = C.c_longlong(), C.c_longlong()
    _lib.call("oai_mc_count", vol.data_ptr(), D, H, W, float(level), ws.data_ptr(), ws.numel(), C.byref(nv), C.byref(nt), _lib.STREAM,
              device=vol.device)
    verts = torch.empty((nv.value, 3), dtype=torch.float32, device=vol.device)
    faces = torch.empty((nt.value, 3), dtype=torch.int32, device=vol.device)
    sp = (C.c_float * 3)(*[float(v) for v in spacing_xyz])
    _lib.call("oai_mc_emit", vol.data_ptr(), D, H, W, float(level), sp, ws.data_ptr(), verts.data_ptr(), faces.data_ptr(), _lib.STREAM,
              device=vol.device)
    return verts, faces


def marching_cubes(volume_zyx, level: float = 0.5, spacing_xyz=(1.0, 1.0, 1.0)) -> Tuple[np.ndarray, np.ndarray]:
    """(verts, faces) of the iso-surface; ``volume_zyx`` may be a numpy array or a float32 torch tensor already on the device."""
    _lib.load()
    verts, faces = _marching_cubes_dev(volume_zyx, level, spacing_xyz)
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


# ---- the same graph steps on the device (csrc/mesh_graph.hip) ------------------------------------------------------------------
def mesh_components_device(faces, n_verts: int, return_rounds: bool = False):
    """Connected components of the face graph on the GPU: int32 label per vertex = the smallest vertex index of its component (an
    unreferenced vertex is its own component).  ``return_rounds``: also the number of hook / jump rounds it took."""
    f = _dev(faces, np.int32, (3,))
    nf, n = int(f.shape[0]), int(n_verts)
    label = torch.empty(n, dtype=torch.int32, device=f.device)
    ws = _lib.workspace("oai_mesh_components", f.device, n, nf, pad=True)
    rounds = C.c_int()
    _lib.call("oai_mesh_components", f.data_ptr(), nf, n, ws.data_ptr(), ws.numel(), label.data_ptr(), C.byref(rounds), _lib.STREAM, device=f.device)
    return (label, rounds.value) if return_rounds else label


def keep_large_regions_device(verts, faces, min_cells: int = 3000) -> Tuple[torch.Tensor, torch.Tensor]:
    """keep_large_regions on the GPU: torch tensors in (float32 [n,3], int32 [m,3]), device tensors out, equal to the host's."""
    v, f = _dev(verts, np.float32, (3,)), _dev(faces, np.int32, (3,))
    nv, nf = int(v.shape[0]), int(f.shape[0])
    ws = _lib.workspace("oai_mesh_keep_large_regions", v.device, nv, nf)
    vo, fo = torch.empty_like(v), torch.empty_like(f)
    n_v, n_f = C.c_longlong(), C.c_longlong()
    _lib.call("oai_mesh_keep_large_regions", v.data_ptr(), nv, f.data_ptr(), nf, int(min_cells), ws.data_ptr(), ws.numel(), vo.data_ptr(),
              fo.data_ptr(), C.byref(n_v), C.byref(n_f), _lib.STREAM, device=v.device)
    return vo[:n_v.value], fo[:n_f.value]


def vertex_adjacency_device(n_verts: int, faces) -> Tuple[torch.Tensor, torch.Tensor]:
    """vertex_adjacency on the GPU: int32 device tensors (offsets [n+1], neighbours), equal to the host's."""
    f = _dev(faces, np.int32, (3,))
    n, nf = int(n_verts), int(f.shape[0])
    ws = _lib.workspace("oai_mesh_adjacency", f.device, n, nf)
    off = torch.empty(n + 1, dtype=torch.int32, device=f.device)
    nbr = torch.empty(max(6 * nf, 1), dtype=torch.int32, device=f.device)
    n_nbrs = C.c_longlong()
    _lib.call("oai_mesh_adjacency", f.data_ptr(), nf, n, ws.data_ptr(), ws.numel(), off.data_ptr(), nbr.data_ptr(), C.byref(n_nbrs), _lib.STREAM,
              device=f.device)
    return off, nbr[:n_nbrs.value]


def _smooth_dev(v: torch.Tensor, off: torch.Tensor, nbr: torch.Tensor, num_iterations: int, relaxation_factor: float) -> torch.Tensor:
    tmp, out = torch.empty_like(v), torch.empty_like(v)
    _lib.call("oai_mesh_smooth", v.data_ptr(), int(v.shape[0]), off.data_ptr(), nbr.data_ptr(), int(num_iterations), float(relaxation_factor),
              tmp.data_ptr(), out.data_ptr(), _lib.STREAM, device=v.device)
    return out


def smooth_mesh(input_mesh: Mesh, num_iterations: int = 150, relaxation_factor: float = 0.01) -> Mesh:
    """vtkSmoothPolyDataFilter with its defaults (relaxation 0.01, boundary smoothing on, no feature edges)."""
    _lib.load()
    n = len(input_mesh.verts)
    if n == 0 or num_iterations <= 0:
        return Mesh(input_mesh.verts.copy(), input_mesh.faces.copy(), dict(input_mesh.point_data))
    off, nbr = vertex_adjacency(n, input_mesh.faces)
    out = _smooth_dev(_dev(input_mesh.verts, np.float32), _dev(off, np.int32), _dev(nbr, np.int32), num_iterations, relaxation_factor)
    return Mesh(out.cpu().numpy(), input_mesh.faces.copy(), dict(input_mesh.point_data))


def _mesh_resident(vol: torch.Tensor, spacing_xyz, num_iterations: int, min_cells: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """get_mesh with every step on the device: marching cubes, large regions, edge graph, smoothing.  Device (verts, faces)."""
    v, f = _marching_cubes_dev(vol, 0.5, spacing_xyz)
    v, f = keep_large_regions_device(v, f, min_cells)
    n = int(v.shape[0])
    if n == 0 or num_iterations <= 0:
        return v, f
    off, nbr = vertex_adjacency_device(n, f)
    return _smooth_dev(v, off, nbr, num_iterations, 0.01), f


def _probmap_dev(image, spacing_xyz=None, origin_xyz=None, direction=None, strict: bool = False):
    """The probability map -- an Image, an array, an itk image or a device tensor -- as (float32 [z,y,x] device volume, spacing,
    origin, direction): the image's own geometry, unit / zero / identity for a tensor.  The explicit arguments describe a tensor.
    ``strict`` (the cuberille path): they also replace an Image's own geometry, and an Image that is not 3-D is refused here; without
    it (get_mesh, get_thickness_mesh, ThicknessAtlas: ``spacing_xyz`` goes with a tensor) an Image keeps its own."""
    if isinstance(image, torch.Tensor):
        if image.dim() != 3:
            raise ValueError(f"expected a [z,y,x] probability map, got shape {tuple(image.shape)}")
        vol, explicit = _dev(image, np.float32), True
        s, o, d = np.ones(3), np.zeros(3), np.eye(3)
    else:
        img = as_image(image)
        if strict and img.array.ndim != 3:
            raise ValueError(f"expected a [z,y,x] probability map, got shape {img.array.shape}")
        vol, explicit = _dev(img.array, np.float32), strict
        s, o, d = img.spacing, img.origin, img.direction
    if explicit:
        s = s if spacing_xyz is None else spacing_xyz
        o = o if origin_xyz is None else origin_xyz
        d = d if direction is None else direction
    return (vol, np.asarray(s, np.float64).reshape(3).copy(), np.asarray(o, np.float64).reshape(3).copy(),
            np.asarray(d, np.float64).reshape(3, 3).copy())


def get_mesh(itk_image, num_iterations: int = 150, min_cells: int = 3000, on_device: bool = False, spacing_xyz=None) -> Mesh:
    """mesh_processing.py:325-340: iso-surface of the probability map at 0.5 in (x,y,z)*spacing, small regions dropped
    (get_vtk_mesh), then smoothed.  ``on_device``: the region filter and the edge graph on the GPU too (csrc/mesh_graph.hip), one
    download at the end, the same bits; ``itk_image`` may then also be a float32 [z,y,x] device tensor with ``spacing_xyz``."""
    if on_device:
        v, f = _mesh_resident(*_probmap_dev(itk_image, spacing_xyz)[:2], num_iterations, min_cells)
        return Mesh(v.cpu().numpy(), f.cpu().numpy())
    img = as_image(itk_image)
    verts, faces = marching_cubes(np.asarray(img.array, dtype=np.float32), 0.5, img.spacing)
    verts, faces = keep_large_regions(verts, faces, min_cells)
    return smooth_mesh(Mesh(verts, faces), num_iterations=num_iterations)


# ---- cuberille iso-surface (itk.cuberille_image_to_mesh_filter; csrc/cuberille.hip) --------------------------------------------
def cuberille_device(image, iso_surface_value: float = 0.5, *, generate_triangle_faces: bool = True,
                     project_vertices_to_iso_surface: bool = True, project_vertex_surface_distance_threshold: float = 0.05,
                     project_vertex_step_length: float = -1.0, project_vertex_step_length_relaxation_factor: float = 0.95,
                     project_vertex_maximum_number_of_steps: int = 50, move_after_converged: bool = True, spacing_xyz=None,
                     origin_xyz=None, direction=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The cuberille surface left on the device: (verts float32 [n,3] physical points, faces int32 [2m,3] or [m,4] quads, steps int32
    [n] = projection steps per vertex).  Contract: include/oai_hip.h, "Cuberille iso-surface"."""
    vol, s, o, d = _probmap_dev(image, spacing_xyz, origin_xyz, direction, strict=True)
    D, H, W = (int(v) for v in vol.shape)
    geo = np.concatenate([o, s, d.reshape(-1), np.linalg.inv(d @ np.diag(s)).reshape(-1)])
    flip = bool(np.linalg.det(d) < 0)
    ws = _lib.workspace("oai_cuberille", vol.device, D, H, W)
    if ws.numel() == 0:
        raise ValueError(f"cuberille: volume {D}x{H}x{W} is empty or too large")
    nv, nf = C.c_longlong(), C.c_longlong()
    iso = float(iso_surface_value)
    _lib.call("oai_cuberille_count", vol.data_ptr(), D, H, W, iso, ws.data_ptr(), ws.numel(), C.byref(nv), C.byref(nf), _lib.STREAM,
              device=vol.device)
    verts = torch.empty((nv.value, 3), dtype=torch.float32, device=vol.device)
    faces = torch.empty((2 * nf.value, 3) if generate_triangle_faces else (nf.value, 4), dtype=torch.int32, device=vol.device)
    steps = torch.empty(nv.value, dtype=torch.int32, device=vol.device)
    if nv.value == 0:                                                # nothing inside: no faces either
        return verts, faces, steps
    _lib.call("oai_cuberille_emit", vol.data_ptr(), D, H, W, iso, (C.c_double * 24)(*[float(x) for x in geo]), int(flip),
              int(bool(generate_triangle_faces)), int(bool(project_vertices_to_iso_surface)), float(project_vertex_surface_distance_threshold),
              float(project_vertex_step_length), float(project_vertex_step_length_relaxation_factor), int(project_vertex_maximum_number_of_steps),
              int(bool(move_after_converged)), ws.data_ptr(), ws.numel(), nv.value, nf.value, verts.data_ptr(), faces.data_ptr(), steps.data_ptr(),
              _lib.STREAM, device=vol.device)
    return verts, faces, steps


def get_mesh_from_probability_map(image, *, iso_surface_value: float = 0.5, generate_triangle_faces: bool = True,
                                  project_vertices_to_iso_surface: bool = True, project_vertex_surface_distance_threshold: float = 0.05,
                                  project_vertex_step_length: float = -1.0, project_vertex_step_length_relaxation_factor: float = 0.95,
                                  project_vertex_maximum_number_of_steps: int = 50, move_after_converged: bool = True, spacing_xyz=None,
                                  origin_xyz=None, direction=None) -> Mesh:
    """mesh_processing.py:343-350: itk.cuberille_image_to_mesh_filter with the reference's settings (the defaults here) on the GPU.

    Restated, unpinned (ITK is not installed): one quad per face between an inside voxel (value >= iso) and an outside
    neighbour, one vertex per lattice point, numbered in order of first use, then each vertex walked to the iso-surface along the
    interpolated gradient.  Vertices are ITK's physical points, origin + direction @ (spacing * index) -- unlike ``get_mesh``, which
    returns skimage's (x, y, z) * spacing without the origin.  ``image`` is an ``Image``, an array, an ``itk.Image`` or a float32
    [z,y,x] device tensor (e.g. VolumeResult.fc_atlas) with the optional ``spacing_xyz`` / ``origin_xyz`` / ``direction``.
    ``move_after_converged``: the recalled form moves once more on the step that converges.  Faces are int32
    triangles [2m,3], or quads [m,4] with ``generate_triangle_faces=False``."""
    verts, faces, _ = cuberille_device(
        image, iso_surface_value, generate_triangle_faces=generate_triangle_faces, project_vertices_to_iso_surface=project_vertices_to_iso_surface,
        project_vertex_surface_distance_threshold=project_vertex_surface_distance_threshold, project_vertex_step_length=project_vertex_step_length,
        project_vertex_step_length_relaxation_factor=project_vertex_step_length_relaxation_factor,
        project_vertex_maximum_number_of_steps=project_vertex_maximum_number_of_steps, move_after_converged=move_after_converged,
        spacing_xyz=spacing_xyz, origin_xyz=origin_xyz, direction=direction)
    return Mesh(verts.cpu().numpy(), faces.cpu().numpy())


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


def _split_dev(v: torch.Tensor, f: torch.Tensor, mesh_type: str) -> DeviceSplit:
    kind = "FC" if mesh_type == "FC" else "TC"
    nv, nf = int(v.shape[0]), int(f.shape[0])
    if nf < 2:
        raise ValueError(f"n_samples={nf} should be >= n_clusters=2.")
    ws = _lib.workspace("oai_mesh_split", v.device, nv, nf, _MESH_TYPE[kind], _N_INIT[kind])
    cent = torch.empty((nf, 3), dtype=torch.float64, device=v.device)
    nrm = torch.empty((nf, 3), dtype=torch.float64, device=v.device)
    side = torch.empty(nf, dtype=torch.int8, device=v.device)
    counts = (C.c_longlong * 3)()
    _lib.call("oai_mesh_split_features", v.data_ptr(), nv, f.data_ptr(), nf, _MESH_TYPE[kind], ws.data_ptr(), ws.numel(), cent.data_ptr(),
              nrm.data_ptr(), counts, _lib.STREAM, device=v.device)
    n_slabs = 3 if kind == "FC" else 1
    first, uni = _kmeans_draws(list(counts)[:n_slabs], _N_INIT[kind])
    n_iter = (C.c_int * 3)()
    _lib.call("oai_mesh_split_kmeans", nf, _MESH_TYPE[kind], ws.data_ptr(), ws.numel(), nrm.data_ptr(), _N_INIT[kind], _KMEANS_MAX_ITER, counts,
              (C.c_longlong * len(first))(*first), (C.c_double * len(uni))(*uni), side.data_ptr(), n_iter, _lib.STREAM, device=v.device)
    return DeviceSplit(v, f, side, cent, nrm, np.array(list(n_iter)[:n_slabs], dtype=np.int64))


def split_mesh_device(mesh: Mesh, mesh_type: str = "FC") -> DeviceSplit:
    """The KMeans labelling of split_femoral_cartilage_surface (FC) / split_tibial_cartilage_surface (anything else) on the GPU.
    A slab with fewer than 2 faces raises the ValueError sklearn raises, as the reference does; the host path of this package skips
    such an FC slab instead (its faces keep side 0)."""
    _lib.load()
    nf = len(mesh.faces)
    if nf < 2:
        raise ValueError(f"n_samples={nf} should be >= n_clusters=2.")
    return _split_dev(_dev(mesh.verts, np.float32, (3,)), _dev(mesh.faces, np.int32, (3,)), mesh_type)


def _sub_mesh_dev(split: DeviceSplit, which: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """get_sub_mesh_device, left on the device: (verts, faces, face list int32)."""
    nv, nf = int(split.verts.shape[0]), int(split.faces.shape[0])
    dev = split.verts.device
    ws = _lib.workspace("oai_mesh_submesh", dev, nv, nf)
    vo = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    fo = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    io = torch.empty(nf, dtype=torch.int32, device=dev)
    n_v, n_f = C.c_longlong(), C.c_longlong()
    _lib.call("oai_mesh_submesh", split.verts.data_ptr(), nv, split.faces.data_ptr(), nf, split.side.data_ptr(), int(which), ws.data_ptr(),
              ws.numel(), vo.data_ptr(), fo.data_ptr(), io.data_ptr(), C.byref(n_v), C.byref(n_f), _lib.STREAM, device=dev)
    return vo[:n_v.value], fo[:n_f.value], io[:n_f.value]


def get_sub_mesh_device(split: DeviceSplit, which: int) -> Tuple[Mesh, np.ndarray]:
    """get_sub_mesh(mesh, np.where(side == which)[0]) built on the GPU: (sub-mesh, face list)."""
    v, f, io = _sub_mesh_dev(split, which)
    return Mesh(v.cpu().numpy(), f.cpu().numpy()), io.cpu().numpy().astype(np.int64)


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
def _grid_from_params(lo: np.ndarray, hi: np.ndarray, reach) -> Tuple[float, np.ndarray, np.ndarray]:
    """The uniform grid of a broad phase: cell h, dims and lowered corner from the float64 bounds and the length a cell must cover
    (point_distance: the longest edge; map_attributes: the radius)."""
    h = max(float(reach) * 1.0001, float((hi - lo).max()) / 512.0, 1e-6)             # at most 512 cells per axis
    dims = np.maximum(np.ceil((hi - lo) / h).astype(np.int64) + 1, 1)
    return h, dims, lo - 0.5 * h * 1e-3


def mesh_grid_params_device(verts, faces) -> Tuple[np.ndarray, np.ndarray, np.float64]:
    """(lo, hi, longest edge) as point_distance computes them on the host -- float32 bounds as float64, the longest edge in fp64 --
    from device tensors, with one 56-byte download."""
    v, f = _dev(verts, np.float32, (3,)), _dev(faces, np.int32, (3,))
    out = torch.empty(7, dtype=torch.float64, device=v.device)
    ws = _lib.workspace("oai_mesh_grid_params", v.device)
    _lib.call("oai_mesh_grid_params", v.data_ptr(), int(v.shape[0]), f.data_ptr(), int(f.shape[0]), ws.data_ptr(), ws.numel(), out.data_ptr(),
              _lib.STREAM, device=v.device)
    o = out.cpu().numpy()
    return o[0:3].copy(), o[3:6].copy(), np.sqrt(o[6])          # sqrt is monotone and correctly rounded: the max of the host's norms


def _point_distance_dev(p: torch.Tensor, v: torch.Tensor, f: torch.Tensor, grid=None) -> torch.Tensor:
    """Distances from the points p to the mesh (v, f), all device tensors.  ``grid`` = (lo, hi, edge) selects the broad phase."""
    n_points, n_tris = int(p.shape[0]), int(f.shape[0])
    out = torch.empty(n_points, dtype=torch.float32, device=p.device)
    if grid is not None:
        h, dims, lo = _grid_from_params(*grid)
        glo = (C.c_float * 3)(*[float(x) for x in lo])
        gd = (C.c_int * 3)(*[int(x) for x in dims])
        ws = _lib.workspace("oai_mesh_grid", p.device, gd, n_tris)
        _lib.call("oai_mesh_point_distance_grid", p.data_ptr(), n_points, v.data_ptr(), f.data_ptr(), n_tris, glo, float(h), gd, ws.data_ptr(),
                  ws.numel(), out.data_ptr(), _lib.STREAM, device=p.device)
    else:
        _lib.call("oai_mesh_point_distance", p.data_ptr(), n_points, v.data_ptr(), f.data_ptr(), n_tris, out.data_ptr(), _lib.STREAM, device=p.device)
    return out


def point_distance(points: np.ndarray, mesh: Mesh, broad_phase: bool = True) -> np.ndarray:
    """Unsigned distance from each point to the mesh surface.  ``broad_phase``: bin the triangles into a uniform grid whose cell is
    the longest triangle edge (>= 2 voxels' worth) so that a point only tests the triangles around it; False = brute force."""
    _lib.load()
    p, v, f = _dev(points, np.float32), _dev(mesh.verts, np.float32), _dev(mesh.faces, np.int32)
    grid = None
    if broad_phase and len(mesh.faces) > 0:
        tri = mesh.verts[mesh.faces].astype(np.float64)
        edge = max(np.linalg.norm(tri[:, 0] - tri[:, 1], axis=1).max(), np.linalg.norm(tri[:, 1] - tri[:, 2], axis=1).max(),
                   np.linalg.norm(tri[:, 2] - tri[:, 0], axis=1).max())
        grid = (mesh.verts.min(axis=0).astype(np.float64), mesh.verts.max(axis=0).astype(np.float64), edge)
    return _point_distance_dev(p, v, f, grid).cpu().numpy()


def get_distance(inner_mesh: Mesh, outer_mesh: Mesh) -> Tuple[Mesh, Mesh]:
    """vtkDistancePolyDataFilter (:310-322): every point of each mesh gets the unsigned distance to the other mesh's surface
    as point data "Distance"."""
    d_in = point_distance(inner_mesh.verts, outer_mesh)
    d_out = point_distance(outer_mesh.verts, inner_mesh)
    return (Mesh(inner_mesh.verts, inner_mesh.faces, {**inner_mesh.point_data, "Distance": d_in}),
            Mesh(outer_mesh.verts, outer_mesh.faces, {**outer_mesh.point_data, "Distance": d_out}))


def _distance_dev(p: torch.Tensor, v: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    """point_distance(p, Mesh(v, f)) with the grid parameters taken on the device."""
    return _point_distance_dev(p, v, f, mesh_grid_params_device(v, f) if f.shape[0] > 0 else None)


def _resident_split(vol: torch.Tensor, spacing_xyz, mesh_type: str, min_cells: int = 3000) -> DeviceSplit:
    """The resident chain up to the split, the one place it is spelled out: marching cubes, large regions, edge graph, 150 smoothing
    sweeps, device k-means.  A caller builds the sub-meshes (_sub_mesh_dev) and distances (_distance_dev) it needs from the result.
    Raises ValueError on a map without a large region."""
    return _split_dev(*_mesh_resident(vol, spacing_xyz, 150, min_cells), mesh_type)


def get_thickness_mesh(itk_image, mesh_type: str = "FC", num_iterations: int = 150, min_cells: int = 3000,
                       split_on_device: bool = False, on_device: bool = False, spacing_xyz=None) -> Tuple[Mesh, Mesh]:
    """mesh_processing.py:381-395 (which, like this, always smooths with 150 iterations).  ``split_on_device``: see split_mesh (it
    raises ValueError on a mesh with an FC slab of fewer than 2 faces, which the default path skips).

    ``on_device``: the whole step stays on the GPU -- marching cubes, large regions, edge graph, smoothing, the device split and
    the distance both ways -- and only the two result meshes are downloaded; the same bits as ``split_on_device=True``.
    ``itk_image`` may then also be a float32 [z,y,x] device tensor (VolumeResult.fc_atlas / tc_atlas) with ``spacing_xyz``."""
    if not on_device:
        mesh = get_mesh(itk_image, num_iterations=150, min_cells=min_cells)
        inner, outer = split_mesh(mesh, mesh_type, on_device=split_on_device)
        return get_distance(inner, outer)
    sp = _resident_split(*_probmap_dev(itk_image, spacing_xyz)[:2], mesh_type, min_cells)
    (iv, if_, _), (ov, of, _) = _sub_mesh_dev(sp, -1), _sub_mesh_dev(sp, 1)
    d_in, d_out = _distance_dev(iv, ov, of), _distance_dev(ov, iv, if_)
    return (Mesh(iv.cpu().numpy(), if_.cpu().numpy(), {"Distance": d_in.cpu().numpy()}),
            Mesh(ov.cpu().numpy(), of.cpu().numpy(), {"Distance": d_out.cpu().numpy()}))


def _thickness_inner_dev(vol: torch.Tensor, spacing_xyz, mesh_type: str, min_cells: int = 3000) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The resident branch of get_thickness_mesh without its second distance and without downloads: (inner verts, inner faces,
    distance inner -> outer) as device tensors, the bits of ``get_thickness_mesh(..., on_device=True)[0]`` (a point's distance does not
    depend on the other direction having been computed).  Raises the same ValueError on a map without a large region."""
    return _thickness_from_split(_resident_split(vol, spacing_xyz, mesh_type, min_cells))


def _thickness_from_split(sp: DeviceSplit) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """_thickness_inner_dev from the split on: for a caller that also wants the split itself (the mesh QC of thickness.py)."""
    (iv, if_, _), (ov, of, _) = _sub_mesh_dev(sp, -1), _sub_mesh_dev(sp, 1)
    return iv, if_, _distance_dev(iv, ov, of)


# ---- mesh points pushed through phi (itk.transform_mesh_filter with the registration's transform; csrc/mesh_transform.hip) -----------
_COORDS = ("spacing", "physical")


def mesh_point_affines(image_A, image_B, net_shape, coords_in: str = "spacing", coords_out: str = "spacing", inverse: bool = False):
    """The two affine legs around phi for POINTS, composed on the host in fp64 on top of registration.resample_affines:

        point_to_net : ``coords_in`` on image_B's grid -> B index -> network index space
        net_to_out   : network index space -> A continuous index -> ``coords_out`` on image_A's grid

    "spacing" is get_mesh's convention, (x, y, z) * spacing with no origin or direction; "physical" is ITK's physical point,
    origin + direction @ (spacing * index), what get_mesh_from_probability_map returns.  ``image_A`` / ``image_B``: Images (metadata is
    enough: spacing, origin, direction and the array's shape); ``net_shape`` = phi's (D, H, W).  Returns ((A, b), (A, b)).

    ``inverse``: the legs of the OTHER direction, for the point solver (oai_inverse_points_through_phi): ``coords_in`` then refers to
    image_A's grid and ``coords_out`` to image_B's, and the pair is the fp64 host inverse of the forward pair with the coordinates swapped,

        point_to_net : ``coords_in`` on image_A's grid -> network index space      (the inverse of the forward net_to_out)
        net_to_out   : network index space -> ``coords_out`` on image_B's grid     (the inverse of the forward point_to_net)"""
    for c in (coords_in, coords_out):
        if c not in _COORDS:
            raise ValueError(f"coords must be one of {_COORDS}, got {c!r}")
    if inverse:
        (P, p), (Q, q) = mesh_point_affines(image_A, image_B, net_shape, coords_out, coords_in)
        Qi, Pi = np.linalg.inv(Q), np.linalg.inv(P)
        return (Qi, -Qi @ q), (Pi, -Pi @ p)
    A, B = as_image(image_A), as_image(image_B)
    (A1, b1), (A2, b2) = resample_affines(A, B, tuple(int(v) for v in net_shape))
    if coords_in == "spacing":
        C_in, c_in = np.diag(1.0 / B.spacing), np.zeros(3)
    else:
        P_B, o_B = B.index_to_physical_affine()
        C_in = np.linalg.inv(P_B)
        c_in = -C_in @ o_B
    if coords_out == "spacing":
        C_out, c_out = np.diag(A.spacing), np.zeros(3)
    else:
        C_out, c_out = A.index_to_physical_affine()
    return (A1 @ C_in, A1 @ c_in + b1), (C_out @ A2, C_out @ b2 + c_out)


def _transform_points_dev(points: torch.Tensor, phi: torch.Tensor, point_to_net, net_to_out, return_inside: bool = False):
    """transform_mesh's vertex step on device tensors: float32 [n,3] in, float32 [n,3] out (and the uint8 inside mask), nothing
    downloaded.  ``phi`` float32 [3,D,H,W] on the points' device; the affines from mesh_point_affines."""
    return ops.transform_points_through_phi(points, phi, point_to_net, net_to_out, return_inside=return_inside)


def _inverse_points_dev(points: torch.Tensor, phi: torch.Tensor, point_to_net, net_to_out, max_iter: int = 30, tol: float = 1e-7,
                        return_status: bool = False):
    """transform_mesh(..., inverse=True)'s vertex step on device tensors: float32 [n,3] in, float32 [n,3] out (and the uint8 status: 1
    converged inside phi's buffer, 2 outside it, 0 not converged and moved by the affines alone), nothing downloaded.  The affines
    from mesh_point_affines(..., inverse=True)."""
    return ops.inverse_points_through_phi(points, phi, point_to_net, net_to_out, max_iter=max_iter, tol=tol, return_status=return_status)


def transform_mesh(mesh: Mesh, transform, image_A=None, image_B=None, coords_in: str = "spacing", coords_out: str = "spacing",
                   inverse: bool = False, max_iter: int = 30, tol: float = 1e-7) -> Mesh:
    """The mesh with its vertices pushed through the registration's map: from image_B's (the atlas') space to image_A's (the patient's),
    the direction phi provides.  What itk.transform_mesh_filter does with ``create_itk_transform``'s CompositeTransform -- the reference
    has no such call; restated from ITK's documented composite-transform behaviour, unpinned like the resample (oracle/resample.py):
    affine into network index space, + the trilinear displacement inside the field's buffer (identity outside it), affine out.

    ``transform``: a registration.DisplacementTransform (it carries ``phi`` and both geometries), or a float32 [3,D,H,W] phi (array or
    device tensor, VolumeResult.phi) with ``image_A`` and ``image_B``.  ``coords_in`` / ``coords_out``: see mesh_point_affines; a mesh
    written with meshwrite in "physical" coordinates overlays the patient's image.  Faces and point data are carried over unchanged.

    ``inverse``: the other direction, from image_A's (the patient's) space to image_B's (the atlas'), with the same ``transform``:
    every vertex is solved for by Newton's method on phi itself (csrc/phi_inverse.hip), exact to ``tol`` network voxels; no stored
    inverse is interpolated.  ``coords_in`` then refers to image_A's grid and ``coords_out`` to image_B's.  A vertex that does not
    converge within ``max_iter`` (inside a fold of phi) is moved by the affines alone; _inverse_points_dev(..., return_status=True)
    counts them.  Unpinned like the forward push: ITK is absent."""
    _lib.load()
    if isinstance(transform, DisplacementTransform):
        if transform.phi is None:
            raise ValueError("transform_mesh: the DisplacementTransform carries no phi")
        phi = transform.phi
        image_A = transform.image_A if image_A is None else image_A
        image_B = transform.image_B if image_B is None else image_B
    else:
        phi = transform
    if image_A is None or image_B is None:
        raise ValueError("transform_mesh: a bare phi needs image_A and image_B (the geometries on either side of it)")
    shape = tuple(phi.shape)
    if len(shape) != 4 or shape[0] != 3:
        raise ValueError(f"transform_mesh: phi must be [3,D,H,W], got {shape}")
    p2n, n2o = mesh_point_affines(image_A, image_B, shape[1:], coords_in, coords_out, inverse=inverse)
    phi_d = _dev(phi, np.float32)
    verts = _dev(mesh.verts, np.float32, (3,), device=phi_d.device)
    out = _inverse_points_dev(verts, phi_d, p2n, n2o, max_iter, tol) if inverse else _transform_points_dev(verts, phi_d, p2n, n2o)
    return Mesh(out.cpu().numpy(), mesh.faces.copy(), dict(mesh.point_data))


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


def _map_attributes_dev(src_verts: torch.Tensor, src_vals: torch.Tensor, tgt_verts: torch.Tensor, radius: float = 1.0, grid=None) -> torch.Tensor:
    """map_attributes' grid broad phase on device tensors: float32 source points [n_src,3], values [n_comp,n_src], targets [n_tgt,3]
    -> float32 [n_comp,n_tgt], nothing downloaded.  ``grid`` = (lo, hi), the float64 bounds of the source points as the host path takes
    them (float32 minima / maxima widened; mesh_grid_params_device returns the same)."""
    n_src, n_comp, n_tgt = int(src_verts.shape[0]), int(src_vals.shape[0]), int(tgt_verts.shape[0])
    if n_src == 0:
        raise ValueError("map_attributes: the source mesh has no points")
    lo, hi = (np.asarray(x, dtype=np.float64).reshape(3) for x in grid)
    out = torch.empty((n_comp, n_tgt), dtype=torch.float32, device=src_verts.device)
    h, dims, lo = _grid_from_params(lo, hi, radius)
    glo = (C.c_double * 3)(*[float(x) for x in lo])
    gd = (C.c_int * 3)(*[int(x) for x in dims])
    ws = _lib.workspace("oai_point_grid", src_verts.device, gd, n_src)
    _lib.call("oai_map_attributes_grid", src_verts.data_ptr(), n_src, src_vals.data_ptr(), n_comp, tgt_verts.data_ptr(), n_tgt, float(radius), glo,
              float(h), gd, ws.data_ptr(), ws.numel(), out.data_ptr(), _lib.STREAM, device=src_verts.device)
    return out


def map_attributes(source_mesh: Mesh, target_mesh: Mesh, radius: float = 1.0, broad_phase: bool = True) -> Mesh:
    """mesh_processing.py:400-408: vtkPointInterpolator(SetNullPointsStrategyToClosestPoint), source arrays onto target points.

    Restated from VTK 9's documented defaults (vtk is not installed here; this half of the step is unpinned): vtkLinearKernel,
    the RADIUS footprint, Radius = 1.0, NormalizeWeights on.  For each target point, every source point array takes the unweighted
    mean over the source points with ``|p - q|^2 <= radius^2``; with no source point that close, the value of the closest source
    point (ties: the smallest index).  Sums are fp64, results float32 (as get_distance).  The output has the target's verts, faces
    and point data plus the interpolated source arrays; on a name clash the source array wins.  ``broad_phase``: bin the source
    points into a uniform grid (cells >= radius, at most 512 per axis); False = brute force over every source point (same result).
    """
    _lib.load()
    if len(source_mesh.verts) == 0:
        raise ValueError("map_attributes: the source mesh has no points")
    names, vals = _point_arrays(source_mesh)
    out_data = dict(target_mesh.point_data)
    n_tgt, n_src, n_comp = len(target_mesh.verts), len(source_mesh.verts), vals.shape[0]
    if n_comp == 0:
        return Mesh(target_mesh.verts, target_mesh.faces, out_data)
    if n_tgt == 0:                                    # nothing to interpolate: the arrays keep their trailing shapes (an empty tensor has no pointer to pass)
        res = np.zeros((n_comp, 0), np.float32)
    else:
        s, v, t = _dev(source_mesh.verts, np.float32), _dev(vals, np.float32), _dev(target_mesh.verts, np.float32, (3,))
        if broad_phase:
            out = _map_attributes_dev(s, v, t, radius, grid=(source_mesh.verts.min(axis=0).astype(np.float64), source_mesh.verts.max(axis=0).astype(np.float64)))
        else:
            out = torch.empty((n_comp, n_tgt), dtype=torch.float32, device=s.device)
            _lib.call("oai_map_attributes", s.data_ptr(), n_src, v.data_ptr(), n_comp, t.data_ptr(), n_tgt, float(radius), out.data_ptr(), _lib.STREAM,
                      device=s.device)
        res = out.cpu().numpy()
    row = 0
    for name, shape in names:
        k = int(np.prod(shape[1:], dtype=np.int64))
        out_data[name] = res[row:row + k].T.reshape((n_tgt,) + tuple(shape[1:]))
        row += k
    return Mesh(target_mesh.verts, target_mesh.faces, out_data)


# ---- cartilage morphometry: the footprint behind map_attributes and mesh areas (csrc/thickness_map.hip, csrc/morphometry.hip) --------
def _point_footprint_dev(src_verts: torch.Tensor, tgt_verts: torch.Tensor, radius: float = 1.0, grid=None):
    """What decided mean versus fallback in ``_map_attributes_dev(src_verts, .., tgt_verts, radius, grid)``, on the same arguments minus
    the values: device tensors (count int32 [n_tgt], nearest squared distance float64, nearest source index int32), nothing downloaded.
    ``grid`` = (lo, hi) as there; None: brute force over every source point (the same bits)."""
    n_src, n_tgt = int(src_verts.shape[0]), int(tgt_verts.shape[0])
    if n_src == 0:
        raise ValueError("point_footprint: there are no source points")
    dev = src_verts.device
    count, d2, j = (torch.empty(n_tgt, dtype=t, device=dev) for t in (torch.int32, torch.float64, torch.int32))
    if grid is None:
        _lib.call("oai_point_footprint", src_verts.data_ptr(), n_src, tgt_verts.data_ptr(), n_tgt, float(radius), count.data_ptr(), d2.data_ptr(),
                  j.data_ptr(), _lib.STREAM, device=dev)
        return count, d2, j
    h, dims, lo = _grid_from_params(*(np.asarray(x, dtype=np.float64).reshape(3) for x in grid), radius)
    glo = (C.c_double * 3)(*[float(x) for x in lo])
    gd = (C.c_int * 3)(*[int(x) for x in dims])
    ws = _lib.workspace("oai_point_grid", dev, gd, n_src)
    _lib.call("oai_point_footprint_grid", src_verts.data_ptr(), n_src, tgt_verts.data_ptr(), n_tgt, float(radius), glo, float(h), gd, ws.data_ptr(),
              ws.numel(), count.data_ptr(), d2.data_ptr(), j.data_ptr(), _lib.STREAM, device=dev)
    return count, d2, j


def point_footprint(points: np.ndarray, source_points: np.ndarray, radius: float = 1.0, broad_phase: bool = True):
    """Per point, what ``map_attributes(source, target, radius)`` saw of the source points: (count, nearest_distance, nearest_index) --
    the number of source points within ``radius`` (int32; map_attributes took their mean exactly where it is > 0), the distance to the
    closest source point (float64, the square root of the kernel's fp64 squared distance) and its index (int32, the smallest on a tie:
    the point whose value the fallback took).  ``broad_phase`` as in map_attributes; both forms give the same bits."""
    _lib.load()
    src = np.ascontiguousarray(source_points, dtype=np.float32).reshape(-1, 3)
    if len(src) == 0:
        raise ValueError("point_footprint: there are no source points")
    s, t = _dev(src, np.float32, (3,)), _dev(points, np.float32, (3,))
    grid = (src.min(axis=0).astype(np.float64), src.max(axis=0).astype(np.float64)) if broad_phase else None
    count, d2, j = _point_footprint_dev(s, t, radius, grid)
    return count.cpu().numpy(), np.sqrt(d2.cpu().numpy()), j.cpu().numpy()


def _mesh_areas_dev(verts: torch.Tensor, faces: torch.Tensor, return_face_area: bool = False):
    """mesh_areas on device tensors (float32 [n,3], int32 [m,3]): the float64 [n] vertex areas (and the float64 [m] face areas), nothing
    downloaded."""
    n, m = int(verts.shape[0]), int(faces.shape[0])
    va = torch.empty(n, dtype=torch.float64, device=verts.device)
    fa = torch.empty(m, dtype=torch.float64, device=verts.device) if return_face_area else None
    ws = _lib.workspace("oai_mesh_areas", verts.device, n, m, pad=True)
    _lib.call("oai_mesh_areas", ops._ptr(verts, n), n, ops._ptr(faces, m), m, ws.data_ptr(), ws.numel(), ops._ptr(fa, m), ops._ptr(va, n), _lib.STREAM,
              device=verts.device)
    return (va, fa) if return_face_area else va


def mesh_areas(mesh: Mesh) -> Tuple[np.ndarray, np.ndarray]:
    """(vertex_area [n], face_area [m]) of a triangle mesh as float64 arrays, in the squared unit of its vertices.  A face's area is half
    the norm of its edge cross product in fp64; a vertex owns a third of every face that names it, summed in ascending face index (then
    corner), so the vertex areas add up to the surface area and weigh a per-vertex quantity by surface, not by sampling density.  A
    vertex that no face names gets 0.0.  Bit-reproducible (include/oai_hip.h, "Cartilage morphometry")."""
    _lib.load()
    v, f = _dev(mesh.verts, np.float32, (3,)), _dev(mesh.faces, np.int32, (3,))
    va, fa = _mesh_areas_dev(v, f, return_face_area=True)
    return va.cpu().numpy(), fa.cpu().numpy()


# ---- mesh QC: topology, geometry and self-intersections of a surface (csrc/mesh_quality.hip) ---------------------------------------------
TOPOLOGY_FIELDS = ("faces", "degenerate_faces", "referenced_vertices", "edges", "boundary_edges", "misoriented_edges", "non_manifold_edges",
                   "interface_edges", "faces_inner", "faces_unassigned", "faces_outer", "euler_characteristic", "boundary_loops", "interface_loops",
                   "bad_faces", "manifold_edges")
GEOMETRY_FIELDS = ("area", "signed_volume", "boundary_length", "interface_length", "min_edge", "max_edge", "mean_edge", "min_face_area",
                   "max_face_area", "min_quality", "mean_quality", "low_quality_faces", "edges", "faces")
INTERSECTION_FIELDS = ("pairs", "flagged_faces", "entries_needed", "overflow")
TOPOLOGY_SLOTS, GEOMETRY_SLOTS, INTERSECTION_SLOTS = 16, 16, 4
EDGE_BOUNDARY, EDGE_MANIFOLD, EDGE_MISORIENTED, EDGE_NON_MANIFOLD, EDGE_CLASS_MASK, EDGE_INTERFACE = 1, 2, 3, 4, 15, 16
MAX_GRID_CELLS = 1 << 21         # cells of the self-intersection grid: the cell is enlarged until the grid has no more
Q_MIN = 0.1                      # default of the low-quality count: a triangle with q < 0.1 is a sliver


def _mesh_topology_dev(faces: torch.Tensor, n_verts: int, side: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """oai_mesh_topology on device tensors (faces int32 [m,3], side int8 [m] or None): (edge_class uint8 [m,3], record int64 [16]), both
    on the device, nothing downloaded or checked -- record[14] counts the faces with an index outside the mesh."""
    m, n = int(faces.shape[0]), int(n_verts)
    if side is not None and (side.dtype != torch.int8 or side.numel() != m):
        raise ValueError(f"side must be int8 with one entry per face ({m}), got {side.dtype} x {side.numel()}")
    cls = torch.empty((m, 3), dtype=torch.uint8, device=faces.device)
    rec = torch.empty(TOPOLOGY_SLOTS, dtype=torch.int64, device=faces.device) if out is None else out
    ws = _lib.workspace("oai_mesh_topology", faces.device, n, m, pad=True)
    _lib.call("oai_mesh_topology", ops._ptr(faces, m), m, n, ops._ptr(side, m), ws.data_ptr(), ws.numel(), ops._ptr(cls, m), rec.data_ptr(), _lib.STREAM,
              device=faces.device)
    return cls, rec


def _mesh_geometry_dev(verts: torch.Tensor, faces: torch.Tensor, edge_class: torch.Tensor, origin=None, q_min: float = Q_MIN,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """oai_mesh_geometry on device tensors with the ``edge_class`` of _mesh_topology_dev: the float64 [16] record on the device.
    ``origin``: the point the signed volume's tetrahedra are taken from (default (0, 0, 0); any point gives the same volume of a closed
    mesh up to rounding)."""
    n, m = int(verts.shape[0]), int(faces.shape[0])
    o = (C.c_double * 3)(*([0.0, 0.0, 0.0] if origin is None else [float(x) for x in np.asarray(origin, dtype=np.float64).reshape(3)]))
    rec = torch.empty(GEOMETRY_SLOTS, dtype=torch.float64, device=verts.device) if out is None else out
    ws = _lib.workspace("oai_mesh_geometry", verts.device, m, pad=True)
    _lib.call("oai_mesh_geometry", ops._ptr(verts, n), n, ops._ptr(faces, m), m, ops._ptr(edge_class, m), o, float(q_min), ws.data_ptr(), ws.numel(),
              rec.data_ptr(), _lib.STREAM, device=verts.device)
    return rec


def _intersection_grid(lo: np.ndarray, hi: np.ndarray, cell: float) -> Tuple[float, np.ndarray]:
    """(cell, dims) of the self-intersection grid over the bounds: the cell enlarged by quarters until there are at most MAX_GRID_CELLS."""
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("mesh_self_intersections: the mesh has non-finite vertices")
    h = float(cell)
    if not h > 0.0 or not np.isfinite(h):
        raise ValueError(f"cell_size must be positive and finite, got {cell!r}")
    while True:
        dims = np.floor((hi - lo) / h).astype(np.int64) + 1
        if int(dims.prod()) <= MAX_GRID_CELLS:
            return h, dims
        h *= 1.25


def _mesh_self_intersections_dev(verts: torch.Tensor, faces: torch.Tensor, cell_size: Optional[float] = None, max_entries: Optional[int] = None,
                                 out: Optional[torch.Tensor] = None):
    """oai_mesh_self_intersections on device tensors: (flag uint8 [m], record int64 [4]) on the device; the record is not checked here
    (record[3] = 1: the bin entries did not fit ``max_entries`` and nothing was tested).  The grid is derived from the mesh's bounds and
    longest edge (mesh_grid_params_device: one 56-byte download).  ``cell_size`` None: a little over the longest edge, so a face's box
    spans at most 2 cells per axis and the default ``max_entries`` = 8 per face cannot overflow."""
    n, m = int(verts.shape[0]), int(faces.shape[0])
    flag = torch.empty(m, dtype=torch.uint8, device=verts.device)
    rec = torch.empty(INTERSECTION_SLOTS, dtype=torch.int64, device=verts.device) if out is None else out
    if m == 0 or n == 0:
        lo, h, dims = np.zeros(3), 1.0, np.ones(3, np.int64)
    else:
        lo, hi, edge = mesh_grid_params_device(verts, faces)
        if np.isnan(edge):
            raise ValueError(f"mesh_self_intersections: a face indexes outside the {n} vertices")
        h, dims = _intersection_grid(lo, hi, max(float(edge) * 1.0001, 1e-30) if cell_size is None else cell_size)
    cap = 8 * m if max_entries is None else int(max_entries)
    gd = (C.c_int * 3)(*[int(x) for x in dims])
    glo = (C.c_double * 3)(*[float(x) for x in lo])
    ws = _lib.workspace("oai_mesh_self_intersections", verts.device, m, gd, cap, pad=True)
    _lib.call("oai_mesh_self_intersections", ops._ptr(verts, n), n, ops._ptr(faces, m), m, glo, float(h), gd, cap, ws.data_ptr(), ws.numel(),
              ops._ptr(flag, m), rec.data_ptr(), _lib.STREAM, device=verts.device)
    return flag, rec


def check_mesh_records(topology=None, intersections=None) -> None:
    """What the device could only count: raise on a face index outside the mesh (topology record) and on an overflowed bin list."""
    if topology is not None and int(topology[14]):
        raise ValueError(f"mesh_topology: {int(topology[14])} face(s) index outside the vertices")
    if intersections is not None and int(intersections[3]):
        raise _lib.OaiError(f"mesh_self_intersections: the grid needs {int(intersections[2])} bin entries, more than max_entries: overflow "
                            "(nothing was tested; pass a larger max_entries or cell_size)")


def mesh_topology(mesh: Mesh, side=None) -> Tuple[Dict[str, int], np.ndarray]:
    """Is this mesh closed and consistently oriented?  (record, edge_class): the counts named in TOPOLOGY_FIELDS and a uint8 [m,3] class
    per half-edge -- 0 where it does not own its edge, else EDGE_BOUNDARY (the edge has one face), EDGE_MANIFOLD (two faces running
    opposite ways), EDGE_MISORIENTED (two, the same way), EDGE_NON_MANIFOLD (three or more), plus EDGE_INTERFACE on a manifold edge
    between a face of side -1 and one of side +1 (``side``: int8 per face, DeviceSplit.side).  Integer work on the GPU, exact and the same
    on every run (include/oai_hip.h, "Mesh quality").  A face index outside the vertices raises ValueError."""
    _lib.load()
    f = _dev(mesh.faces, np.int32, (3,))
    s = None if side is None else _dev(side, np.int8, device=f.device)
    cls, rec = _mesh_topology_dev(f, len(mesh.verts), s)
    rec = rec.cpu().numpy()
    check_mesh_records(topology=rec)
    return {k: int(rec[i]) for i, k in enumerate(TOPOLOGY_FIELDS)}, cls.cpu().numpy()


def mesh_geometry(mesh: Mesh, side=None, origin=None, q_min: float = Q_MIN) -> Dict[str, float]:
    """Area, signed enclosed volume ((sum of det(a-o, b-o, c-o)) / 6: positive for outward faces, meaningful on a closed mesh only),
    boundary and interface length, edge-length, face-area and triangle-quality figures (GEOMETRY_FIELDS) in fp64, bit-reproducible.
    The quality q = 4 sqrt(3) A / (sum of squared edge lengths) is 1 for an equilateral and 0 for a flat triangle; ``low_quality_faces``
    counts q < ``q_min``.  ``side`` as in mesh_topology (for the interface length)."""
    _lib.load()
    v, f = _dev(mesh.verts, np.float32, (3,)), _dev(mesh.faces, np.int32, (3,))
    s = None if side is None else _dev(side, np.int8, device=f.device)
    cls, trec = _mesh_topology_dev(f, int(v.shape[0]), s)
    rec = _mesh_geometry_dev(v, f, cls, origin, q_min).cpu().numpy()
    check_mesh_records(topology=trec.cpu().numpy())
    return {k: float(rec[i]) for i, k in enumerate(GEOMETRY_FIELDS)}


def mesh_self_intersections(mesh: Mesh, cell_size: Optional[float] = None, max_entries: Optional[int] = None) -> Tuple[Dict[str, int], np.ndarray]:
    """Does this mesh fold through itself?  (record, flag): INTERSECTION_FIELDS and a uint8 per face, 1 on every face of an intersecting
    pair.  Two faces that share no vertex index intersect when an edge of one properly pierces the other (fp64 orientation determinants
    with strict signs).  Two limits: coplanar overlap and mere touching are not counted, and a fold between faces that share a vertex is
    not seen.  Faces are binned into a uniform grid first; the answer does not depend on it.  ``cell_size`` None: the mesh's longest
    edge, which needs at most 8 bin entries per face; an explicit smaller cell takes its workspace from ``max_entries`` (default 8 per
    face) and raises OaiError when the faces need more.  The grid has at most MAX_GRID_CELLS cells: the cell is enlarged when needed."""
    _lib.load()
    v, f = _dev(mesh.verts, np.float32, (3,)), _dev(mesh.faces, np.int32, (3,))
    flag, rec = _mesh_self_intersections_dev(v, f, cell_size, max_entries)
    rec = rec.cpu().numpy()
    check_mesh_records(intersections=rec)
    return {k: int(rec[i]) for i, k in enumerate(INTERSECTION_FIELDS)}, flag.cpu().numpy()


def _fit_circle_dev(pts: torch.Tensor, col_x: int, col_y: int) -> Tuple[np.ndarray, float]:
    n = int(pts.shape[0])
    ws = _lib.workspace("oai_thickness_map", pts.device, n, pad=True)
    centre, radius, its = (C.c_double * 2)(), C.c_double(), C.c_int()
    _lib.call("oai_fit_circle", pts.data_ptr(), n, col_x, col_y, ws.data_ptr(), ws.numel(), centre, C.byref(radius), C.byref(its), _lib.STREAM,
              device=pts.device)
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
    n = int(pts.shape[0])
    angle = torch.empty(n, dtype=torch.float64, device=pts.device)
    z = torch.empty(n, dtype=torch.float64, device=pts.device)
    c = (C.c_double * 2)(float(centre[0]), float(centre[1]))
    _lib.call("oai_project_circle", pts.data_ptr(), n, col_x, col_y, c, angle.data_ptr(), z.data_ptr(), _lib.STREAM, device=pts.device)
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
    _lib.load()
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
    ws = _lib.workspace("oai_thickness_map", pts.device, n)
    out = torch.empty((3, n), dtype=torch.float64, device=pts.device)
    n_right, n_left = C.c_longlong(), C.c_longlong()
    _lib.call("oai_project_plateaus", pts.data_ptr(), th.data_ptr(), n, ws.data_ptr(), ws.numel(), out[0].data_ptr(), out[1].data_ptr(),
              out[2].data_ptr(), C.byref(n_right), C.byref(n_left), _lib.STREAM, device=pts.device)
    res = out[:, :n_right.value + n_left.value].cpu().numpy()
    return res[0].copy(), res[1].copy(), res[2].copy()


# ---- thickness image: the atlas' projection rasterised once, a gather per knee (csrc/thickness_image.hip) -------------------------
@dataclass
class ThicknessRaster:
    """What thickness_image_build leaves on the GPU for an [H, W] image: per pixel the owning face (int32, -1 = none), its three point
    indices (int32 [H,W,3]) and the barycentric weights of the pixel centre (float64 [H,W,3]).  Pixel (j, i) has its centre at
    (lo[0] + (i + 0.5) * step[0], lo[1] + (j + 0.5) * step[1])."""
    owner: torch.Tensor
    corners: torch.Tensor
    weights: torch.Tensor
    lo: np.ndarray
    step: np.ndarray
    n_covered: int
    n_points: int


def thickness_image_grid(uv: np.ndarray, image_shape) -> Tuple[np.ndarray, np.ndarray]:
    """(lo[2], step[2]) of an [H, W] raster over the finite points of uv [n,2]: lo = the minima, one step per axis = extent / W and
    extent / H (the axes need not share a unit: FC has radians against mm).  An axis of zero extent raises ValueError."""
    H, W = (int(x) for x in image_shape)
    if H < 1 or W < 1:
        raise ValueError(f"thickness image: image_shape {tuple(image_shape)} must be at least 1 x 1")
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    fin = uv[np.isfinite(uv).all(axis=1)]
    if len(fin) == 0:
        raise ValueError("thickness image: no finite projected point")
    lo, hi = fin.min(axis=0), fin.max(axis=0)
    step = np.array([(hi[0] - lo[0]) / W, (hi[1] - lo[1]) / H], dtype=np.float64)
    if not (step > 0).all():
        raise ValueError(f"thickness image: the projected points have no extent along an axis (min {lo}, max {hi})")
    return lo, step


def thickness_image_build(uv, faces, face_skip=None, image_shape=(256, 256)) -> ThicknessRaster:
    """Rasterise a projected mesh once: ``uv`` float64 [n,2] in mesh point order (array or device tensor), ``faces`` int32 [m,3],
    ``face_skip`` bool [m] (faces that must own nothing, e.g. those bridging the two tibial plateaus).  A pixel belongs to the smallest
    face index whose triangle contains its centre (edges inclusive); contract in include/oai_hip.h, "Thickness image"."""
    _lib.load()
    H, W = (int(x) for x in image_shape)
    uv_host = uv.detach().cpu().numpy() if isinstance(uv, torch.Tensor) else np.asarray(uv)
    lo, step = thickness_image_grid(uv_host, (H, W))
    uv_d = _dev(uv, np.float64, (2,))
    f = _dev(faces, np.int32, (3,))
    n_pts, n_faces = int(uv_d.shape[0]), int(f.shape[0])
    if n_faces == 0:
        raise ValueError("thickness image: the mesh has no faces")
    skip = None
    if face_skip is not None:
        skip = _dev(face_skip, np.uint8, device=uv_d.device)
        if skip.shape != (n_faces,):
            raise ValueError(f"thickness image: face_skip has shape {tuple(skip.shape)}, the mesh has {n_faces} faces")
    dev = uv_d.device
    owner = torch.empty((H, W), dtype=torch.int32, device=dev)
    corners = torch.empty((H, W, 3), dtype=torch.int32, device=dev)
    weights = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
    ws = _lib.workspace("oai_thickness_image", dev, n_faces, H, W)
    n_cov = C.c_longlong()
    _lib.call("oai_thickness_image_build", uv_d.data_ptr(), n_pts, f.data_ptr(), n_faces, skip.data_ptr() if skip is not None else None,
              (C.c_double * 2)(*lo), (C.c_double * 2)(*step), H, W, ws.data_ptr(), ws.numel(), owner.data_ptr(), corners.data_ptr(),
              weights.data_ptr(), C.byref(n_cov), _lib.STREAM, device=dev)
    return ThicknessRaster(owner, corners, weights, lo, step, int(n_cov.value), n_pts)


def thickness_image(raster: ThicknessRaster, values):
    """The thickness image of per-point values on the rastered mesh: float32 [H,W] for values [n], [K,H,W] for [K,n]; NaN where no face
    owns the pixel, and NaN spreads from a NaN point to the pixels of its faces.  A device tensor gives a device tensor, an array an array."""
    on_dev = isinstance(values, torch.Tensor)
    v = _dev(values, np.float32, device=raster.owner.device)
    if v.dim() not in (1, 2) or v.shape[-1] != raster.n_points:
        raise ValueError(f"thickness image: values of shape {tuple(v.shape)} do not match the raster's {raster.n_points} points")
    K = 1 if v.dim() == 1 else int(v.shape[0])
    H, W = (int(x) for x in raster.owner.shape)
    img = torch.empty((K, H, W), dtype=torch.float32, device=v.device)
    for k0 in range(0, K, 65535):
        k1 = min(K, k0 + 65535)
        _lib.call("oai_thickness_image_apply", raster.owner.data_ptr(), raster.corners.data_ptr(), raster.weights.data_ptr(), H, W,
                  v.reshape(K, -1)[k0:k1].data_ptr(), raster.n_points, k1 - k0, img[k0:k1].data_ptr(), _lib.STREAM, device=v.device)
    img = img[0] if v.dim() == 1 else img
    return img if on_dev else img.cpu().numpy()
