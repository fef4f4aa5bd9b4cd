"""Timing of the mesh / thickness step on a full-size 160x384x384 probability map: a cartilage-like curved
slab (5 voxels thick, ~300 x 120 voxels wide), the sizes of mesh_processing.get_thickness_mesh on a real femoral cartilage."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oai_analysis_2_amd import mesh_processing as mp
from oai_analysis_2_amd.image import Image

D, H, W = 160, 384, 384
z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
sig = lambda t: 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))
R, T = 220.0, 5.0
r = np.sqrt((x - 192) ** 2 + ((z - 80) * 1.9) ** 2 + (y + 60) ** 2)
prob = (sig(2.0 * (np.abs(r - R) - T / 2)) * sig(2.0 * (np.sqrt((x - 192) ** 2 + ((z - 80) * 1.9) ** 2) - 140))).astype(np.float32)
img = Image(prob, [0.36, 0.36, 0.7])
vol = torch.from_numpy(prob).cuda()

def timed(name, fn, reps=3):
    fn(); torch.cuda.synchronize()
    t = time.time()
    for _ in range(reps): out = fn()
    torch.cuda.synchronize()
    dt = (time.time() - t) / reps
    print(f"{name:52s} {dt*1e3:9.2f} ms")
    return out

v, f = timed("marching cubes 160x384x384 (count + emit + D2H)", lambda: mp.marching_cubes(vol, 0.5, img.spacing))
print(f"   {len(v)} vertices, {len(f)} triangles; volume read 2x94 MB + 5 x 94 MB of counts/offsets")
v, f = mp.keep_large_regions(v, f, 3000)
mesh = mp.Mesh(v, f)
sm = timed("smooth 150 iterations (incl. host edge graph)", lambda: mp.smooth_mesh(mesh, 150))
t = time.time(); inner, outer = mp.split_mesh(sm, "FC"); print(f"{'split (host KMeans, as the reference)':52s} {(time.time()-t)*1e3:9.2f} ms   inner {len(inner.faces)} / outer {len(outer.faces)} faces")
d = timed("distance both directions (uniform-grid broad phase)", lambda: mp.get_distance(inner, outer), reps=2)
import functools
mp_point = mp.point_distance
timed("distance both directions (brute force)", lambda: (mp_point(inner.verts, outer, False), mp_point(outer.verts, inner, False)), reps=2)
print("   median thickness", float(np.median(d[0].point_data["Distance"])), "(slab: 5 voxels x 0.36-0.7 mm)")
pairs = len(inner.verts) * len(outer.faces) + len(outer.verts) * len(inner.faces)
print(f"   brute force = {pairs/1e9:.2f} G point-triangle tests")

# the inner / outer split: the reference's host KMeans (sklearn) against the device path (features -> both sub-meshes on the host)
t = time.time(); h_in, h_out, h_il, h_ol = mp.split_femoral_cartilage_surface(sm, mp.get_cell_normals(sm), mp.get_cell_centroid(sm))
t_host = time.time() - t
print(f"{'split FC, host (sklearn KMeans, 3 slabs x n_init 5)':52s} {t_host*1e3:9.2f} ms")
reps = 5
mp.split_femoral_cartilage_surface_device(sm); torch.cuda.synchronize()
t_dev = time.time()
for _ in range(reps): d_res = mp.split_femoral_cartilage_surface_device(sm)
torch.cuda.synchronize()
t_dev = (time.time() - t_dev) / reps
print(f"{'split FC, device (features, 15 runs, 2 sub-meshes)':52s} {t_dev*1e3:9.2f} ms   (mean of {reps})")
n_iter = mp.split_mesh_device(sm, "FC").n_iter
same = np.array_equal(d_res[2], h_il) and np.array_equal(d_res[3], h_ol)
print(f"   {len(sm.faces)} faces; device n_iter per slab {n_iter.tolist()}; face lists agree with the host: {same}; "
      f"host / device = {t_host / t_dev:.1f}x (both times as printed above)")
