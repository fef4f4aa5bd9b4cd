"""Regenerate tests/golden/thickness_projection.npz from the reference's own project_thickness (mesh_processing.py:411-534).

Needs a checkout of uncbiag/OAI_analysis_2 named by $OAI_REFERENCE; runs on the CPU.  The reference module imports itk, vtk and
trimesh at the top, none of which the projection uses: they are replaced by empty stub modules.  project_thickness then runs on a
duck-typed mesh (GetPointData().GetScalars(), GetPoints().GetData()).  KernelPCA with more than 200 points runs ARPACK from a random
start vector drawn from numpy's global RNG, so the RNG is seeded before every call.

    OAI_REFERENCE=/path/to/OAI_analysis_2 python tests/golden/make_golden_thickness_map.py

With --edges it writes tests/golden/thickness_projection_edges.npz instead: the same calls on the smallest inputs the projection takes
(an FC sheet of 3 points and one of 40, a TC set of 3 + 3 points and one of 150 + 60, which stays on KernelPCA's dense path) and leaves
thickness_projection.npz alone.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "thickness_projection.npz")
OUT_EDGES = os.path.join(HERE, "thickness_projection_edges.npz")


class _Stub(types.ModuleType):
    """an empty module; any attribute (the annotations' itk.Mesh, ...) is a placeholder type"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def load_reference_mesh_processing(ref_root):
    for name in ("itk", "vtk", "vtk.util", "vtk.util.numpy_support", "trimesh"):
        sys.modules.setdefault(name, _Stub(name))
    sys.modules["vtk"].util = sys.modules["vtk.util"]
    sys.modules["vtk.util"].numpy_support = sys.modules["vtk.util.numpy_support"]
    path = os.path.join(ref_root, "oai_analysis", "mesh_processing.py")
    spec = importlib.util.spec_from_file_location("ref_mesh_processing", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Arr:
    def __init__(self, a):
        self.a = a

    def GetScalars(self):
        return self.a

    def GetData(self):
        return self.a


class DuckMesh:
    """the two vtkPolyData calls project_thickness makes"""

    def __init__(self, verts, scalars):
        self.v, self.s = verts, scalars

    def GetPointData(self):
        return _Arr(self.s)

    def GetPoints(self):
        return _Arr(self.v.copy())


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)          # float32-representable fp64 inputs


def make_inputs(seed=20241008):
    rng = np.random.default_rng(seed)
    # FC-like curved sheet: an arc of a cylinder about the (swapped) axis, crossing the +-pi cut of atan2
    n_fc = 1500
    phi = rng.uniform(np.pi - 1.1, np.pi + 1.1, n_fc)
    rad = 31.0 + rng.normal(0.0, 0.4, n_fc)
    c_swapped = np.array([61.5, 48.25])                          # centre in (x, y) after the reference's column swap
    xs = c_swapped[0] + rad * np.cos(phi)
    ys = c_swapped[1] + rad * np.sin(phi)
    fc = f32(np.stack([ys, xs, rng.uniform(10.0, 90.0, n_fc)], axis=1))   # stored unswapped: column 0 is the swapped y
    fc_t = f32(rng.uniform(0.5, 3.5, n_fc))
    # TC-like: two tilted plateaus on either side of z = 50
    def plateau(n, centre, axes, scale):
        q = rng.normal(size=(n, 3)) * scale
        return centre + q @ axes.T
    a = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    b = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    left = plateau(700, np.array([40.0, 55.0, 30.0]), a, np.array([9.0, 5.0, 0.8]))
    right = plateau(600, np.array([42.0, 60.0, 72.0]), b, np.array([8.0, 4.5, 0.7]))
    left[:, 2] = np.minimum(left[:, 2], 49.5)
    right[:, 2] = np.maximum(right[:, 2], 50.0)
    tc = np.concatenate([left, right])
    tc = f32(tc[rng.permutation(len(tc))])                        # the halves interleaved in point order
    tc_t = f32(rng.uniform(0.5, 3.0, len(tc)))
    return fc, fc_t, tc, tc_t


def make_edge_inputs(seed=20250917):
    """{name: (verts, thickness)}: fc3, fc40 (arcs as in make_inputs) and tc3_3, tc150_60 (plateaus of those sizes, interleaved)"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in (3, 40):
        phi = rng.uniform(np.pi - 1.1, np.pi + 1.1, n)
        rad = 31.0 + rng.normal(0.0, 0.4, n)
        fc = np.stack([48.25 + rad * np.sin(phi), 61.5 + rad * np.cos(phi), rng.uniform(10.0, 90.0, n)], axis=1)
        out[f"fc{n}"] = (f32(fc), f32(rng.uniform(0.5, 3.5, n)))
    for n_left, n_right in ((3, 3), (150, 60)):
        halves = []
        for n, centre in ((n_left, [40.0, 55.0, 30.0]), (n_right, [42.0, 60.0, 72.0])):
            axes = np.linalg.qr(rng.normal(size=(3, 3)))[0]
            halves.append(np.array(centre) + (rng.normal(size=(n, 3)) * np.array([9.0, 5.0, 0.8])) @ axes.T)
        halves[0][:, 2] = np.minimum(halves[0][:, 2], 49.5)
        halves[1][:, 2] = np.maximum(halves[1][:, 2], 50.0)
        tc = np.concatenate(halves)
        out[f"tc{n_left}_{n_right}"] = (f32(tc[rng.permutation(len(tc))]), f32(rng.uniform(0.5, 3.0, len(tc))))
    return out


def main_edges(mp):
    arrays = {}
    for name, (verts, th) in make_edge_inputs().items():
        np.random.seed(0)
        x, y, t = mp.project_thickness(DuckMesh(verts, th), mesh_type="FC" if name.startswith("fc") else "TC")
        arrays.update({f"{name}_verts": verts, f"{name}_thickness": th, f"{name}_x": np.asarray(x, np.float64),
                       f"{name}_y": np.asarray(y, np.float64), f"{name}_t": np.asarray(t, np.float64)})
        if name.startswith("fc"):
            sw = verts[:, [1, 0, 2]]
            np.random.seed(0)
            centre, r = mp.compute_least_square_circle(sw[:, 0], sw[:, 1])
            arrays.update({f"{name}_circle_centre": np.asarray(centre, np.float64), f"{name}_circle_radius": np.float64(r)})
    np.savez(OUT_EDGES, **arrays)
    print(f"wrote {OUT_EDGES}: {sorted(arrays)}")


def main():
    ref = os.environ.get("OAI_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "oai_analysis")):
        sys.exit("set OAI_REFERENCE to a checkout of uncbiag/OAI_analysis_2")
    mp = load_reference_mesh_processing(ref)
    if "--edges" in sys.argv[1:]:
        return main_edges(mp)
    fc, fc_t, tc, tc_t = make_inputs()
    np.random.seed(0)
    fc_x, fc_y, fc_th = mp.project_thickness(DuckMesh(fc, fc_t), mesh_type="FC")
    np.random.seed(0)
    tc_x, tc_y, tc_th = mp.project_thickness(DuckMesh(tc, tc_t), mesh_type="TC")
    sw = fc[:, [1, 0, 2]]                                          # the swapped vertices project_thickness fits
    np.random.seed(0)
    centre, r = mp.compute_least_square_circle(sw[:, 0], sw[:, 1])
    emb, plot_xy = mp.get_projection_from_circle_and_vertice(sw, (centre, r))
    np.savez(OUT, fc_verts=fc, fc_thickness=fc_t, tc_verts=tc, tc_thickness=tc_t,
             fc_x=np.asarray(fc_x, np.float64), fc_y=np.asarray(fc_y, np.float64), fc_t=np.asarray(fc_th, np.float64),
             tc_x=np.asarray(tc_x, np.float64), tc_y=np.asarray(tc_y, np.float64), tc_t=np.asarray(tc_th, np.float64),
             circle_centre=np.asarray(centre, np.float64), circle_radius=np.float64(r),
             embedded=np.asarray(emb, np.float64), plot_xy=np.asarray(plot_xy, np.float64))
    print(f"wrote {OUT}: FC {len(fc)} points, TC {len(tc)} points, centre {centre}, R {r}")


if __name__ == "__main__":
    main()
