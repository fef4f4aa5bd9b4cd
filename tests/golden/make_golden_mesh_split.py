"""Regenerate tests/golden/mesh_split.npz from the reference's own split functions (mesh_processing.py:197-294).

Needs a checkout of uncbiag/OAI_analysis_2 named by $OAI_REFERENCE and scikit-learn; runs on the CPU.  The reference module is loaded
as make_golden_thickness_map does (itk / vtk / trimesh stubbed).  Its get_vtk_sub_mesh is replaced by one that returns the face list,
and its KMeans by a subclass that records every fit's features, cluster_centers_ and n_iter_.  The meshes are built on the CPU with
oracle.mesh (marching cubes + smoothing): an FC-like curved slab and a TC-like pair of plateaus.  The duck-typed mesh answers
GetBounds with the float32 bounds of its vertices, as the package's Mesh does.

Stored per mesh (prefix fc_ / tc_): verts float32, faces int32, side int8 per face in {-1, 0, 1}, margin float32 per face (|d0 - d1| /
(d0 + d1) against the recorded final centres, the smallest over the fits that hold the face; 1 for a face in no slab), n_iter per fit.

    OAI_REFERENCE=/path/to/OAI_analysis_2 python tests/golden/make_golden_mesh_split.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "mesh_split.npz")
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden_thickness_map import load_reference_mesh_processing  # noqa: E402


class DuckMesh:
    """the two vtkPolyData calls the split functions make"""

    def __init__(self, verts, faces):
        self.verts, self.faces = verts, faces

    def GetBounds(self):
        lo, hi = self.verts.min(axis=0), self.verts.max(axis=0)
        return (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])

    def GetNumberOfCells(self):
        return len(self.faces)


def _sig(t):
    return 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))


def make_meshes():
    from oracle import mesh as om
    # FC-like: a curved slab (part of a thick cylindrical shell about the z axis), ~6 voxels thick
    D, H, W = 40, 72, 96
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    r = np.sqrt((x - 48) ** 2 + (y + 20) ** 2)
    ang = np.arctan2(x - 48, y + 20)
    prob = _sig(2.0 * (np.abs(r - 62) - 3.0)) * _sig(4.0 * (np.abs(ang) - 0.75)) * _sig(2.0 * (np.abs(z - 20) - 15))
    v, f = om.marching_cubes(prob.astype(np.float32), 0.5, (0.36, 0.36, 0.7))
    fc = (om.smooth(v, f, 30).astype(np.float32), f.astype(np.int32))
    # TC-like: two tilted plateaus side by side, ~5 voxels thick
    D, H, W = 36, 48, 120
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    top = 24 + 0.08 * (x - 60) + 0.05 * (y - 24) + 0.02 * (x - 60) ** 2 / 10
    slab = _sig(2.0 * (np.abs(z - top) - 2.5))
    left = _sig(2.0 * (np.sqrt(((x - 32) / 1.2) ** 2 + (y - 24) ** 2) - 21))
    right = _sig(2.0 * (np.sqrt(((x - 88) / 1.1) ** 2 + (y - 24) ** 2) - 20))
    v, f = om.marching_cubes((slab * np.maximum(left, right)).astype(np.float32), 0.5, (0.36, 0.36, 0.7))
    tc = (om.smooth(v, f, 30).astype(np.float32), f.astype(np.int32))
    return fc, tc


def main():
    ref = os.environ.get("OAI_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "oai_analysis")):
        sys.exit("set OAI_REFERENCE to a checkout of uncbiag/OAI_analysis_2")
    import sklearn
    from oai_analysis_2_amd import mesh_processing as mp     # the numpy helpers only
    mod = load_reference_mesh_processing(ref)
    fits = []

    class RecordingKMeans(mod.KMeans):
        def fit(self, X, y=None, sample_weight=None):
            out = super().fit(X, y, sample_weight)
            fits.append((np.array(X, np.float64), self.cluster_centers_.copy(), int(self.n_iter_)))
            return out

    mod.KMeans = RecordingKMeans
    mod.get_vtk_sub_mesh = lambda mesh, face_list: np.asarray(face_list)
    out = {"sklearn_version": np.array(sklearn.__version__)}
    (fv, ff), (tv, tf) = make_meshes()
    for name, (v, f) in (("fc", (fv, ff)), ("tc", (tv, tf))):
        m = mp.Mesh(v, f)
        normals, centroids = mp.get_cell_normals(m), mp.get_cell_centroid(m)
        fits.clear()
        split = mod.split_femoral_cartilage_surface if name == "fc" else mod.split_tibial_cartilage_surface
        _, _, inner, outer = split(DuckMesh(v, f), normals, centroids)
        side = np.zeros(len(f), np.int8)
        side[inner] = -1
        side[outer] = 1
        # the faces of each fit, in order: FC slabs by the reference's rule, TC all faces
        cn = (centroids - np.mean(centroids, axis=0)) / (np.max(centroids, axis=0) - np.min(centroids, axis=0))
        if name == "fc":
            x = cn[:, 0]
            lo, hi = np.min(x), np.max(x)
            step = (hi - lo) / 3
            members = [np.flatnonzero((x >= lo + step * i) & (x < lo + step * i + step)) for i in range(3)]
        else:
            members = [np.arange(len(f))]
        assert len(members) == len(fits)
        margin = np.ones(len(f))
        for idx, (X, c, _) in zip(members, fits):
            d = ((X[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
            margin[idx] = np.minimum(margin[idx], np.abs(d[:, 0] - d[:, 1]) / (d[:, 0] + d[:, 1]))
        out.update({f"{name}_verts": v, f"{name}_faces": f, f"{name}_side": side, f"{name}_margin": margin.astype(np.float32),
                    f"{name}_n_iter": np.array([it for _, _, it in fits], np.int64)})
        print(f"{name}: {len(v)} vertices, {len(f)} faces, sides {np.bincount(side + 1, minlength=3)} (-1/0/+1), "
              f"n_iter {[it for _, _, it in fits]}, min margin {margin.min():.3g}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} B), sklearn {sklearn.__version__}")


if __name__ == "__main__":
    main()
