"""Wall time of the thickness step (mesh_processing.get_thickness_mesh) resident on the GPU (on_device=True) against the current
path with the device split (split_on_device=True), in one process: scripts/bench_mesh.py's full-size FC slab and the TC-sized bowl
of tests/test_mesh_gpu.py::test_thickness_of_a_shell.  Also checks the two results are the same bits and prints the number of
hook / jump rounds the component labelling needs on each mesh.  --reps N: timed runs per path (default 3); --case fc|tc|both;
--resident-only: only the resident path, nothing else (for a kernel trace of it)."""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oai_analysis_2_amd import mesh_processing as mp
from oai_analysis_2_amd.image import Image

sig = lambda t: 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))


def fc_slab():
    D, H, W = 160, 384, 384
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    r = np.sqrt((x - 192) ** 2 + ((z - 80) * 1.9) ** 2 + (y + 60) ** 2)
    prob = sig(2.0 * (np.abs(r - 220.0) - 2.5)) * sig(2.0 * (np.sqrt((x - 192) ** 2 + ((z - 80) * 1.9) ** 2) - 140))
    return Image(prob.astype(np.float32), [0.36, 0.36, 0.7])


def tc_bowl():
    D, H, W = 48, 96, 96
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    r = np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4 + (y + 30) ** 2)
    prob = sig(2.0 * (np.abs(r - 60.0) - 3.0)) * sig(2.0 * (np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4) - 30))
    return Image(prob.astype(np.float32), [1.0, 1.0, 1.0])


def timed(fn, reps):
    out = fn()                                           # warm-up (library load, kernels, allocator)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--case", choices=["fc", "tc", "both"], default="both")
    ap.add_argument("--resident-only", action="store_true")
    a = ap.parse_args()
    cases = [c for c in (("fc", "FC slab 160x384x384", fc_slab, "FC", 3000), ("tc", "TC bowl 48x96x96", tc_bowl, "TC", 100)) if a.case in (c[0], "both")]
    for _, name, make, kind, min_cells in cases:
        img = make()
        vol = torch.from_numpy(img.array).cuda()
        if a.resident_only:
            _, t_res = timed(lambda: mp.get_thickness_mesh(vol, kind, min_cells=min_cells, on_device=True, spacing_xyz=img.spacing), a.reps)
            print(f"{name}: on_device=True, device tensor in ms: " + " ".join(f"{t:8.2f}" for t in t_res))
            continue
        ref, t_cur = timed(lambda: mp.get_thickness_mesh(img, kind, min_cells=min_cells, split_on_device=True), a.reps)
        got, t_res = timed(lambda: mp.get_thickness_mesh(img, kind, min_cells=min_cells, on_device=True), a.reps)
        got_t, t_ten = timed(lambda: mp.get_thickness_mesh(vol, kind, min_cells=min_cells, on_device=True, spacing_xyz=img.spacing), a.reps)
        same = all(np.array_equal(x.verts, y.verts) and np.array_equal(x.faces, y.faces) and
                   np.array_equal(x.point_data["Distance"], y.point_data["Distance"]) for r in (got, got_t) for x, y in zip(r, ref))
        v, f = mp._marching_cubes_dev(vol, 0.5, img.spacing)
        _, rounds = mp.mesh_components_device(f, int(v.shape[0]), return_rounds=True)
        kv, kf = mp.keep_large_regions_device(v, f, min_cells)
        fmt = lambda ts: " ".join(f"{t:8.2f}" for t in ts)
        print(f"{name}: {int(f.shape[0])} MC faces, {int(kf.shape[0])} kept; inner {len(ref[0].faces)} / outer {len(ref[1].faces)} faces; "
              f"component rounds {rounds}; bitwise equal: {same}")
        print(f"  split_on_device=True (host graph code)     ms: {fmt(t_cur)}")
        print(f"  on_device=True, Image in                   ms: {fmt(t_res)}   current / resident = {np.median(t_cur) / np.median(t_res):.1f}x")
        print(f"  on_device=True, device tensor in           ms: {fmt(t_ten)}")


if __name__ == "__main__":
    main()
