"""Timing of the atlas thickness map (mesh_processing.py:400-534) at the sizes of the reference's commented-out asserts
(test/test_all.py:69-70): 65 000 FC points and 20 480 TC points.  Synthetic meshes: an FC-like cylinder arc and two TC-like plateaus
on either side of z = 50, the subject mesh mapped onto a jittered copy (the atlas).  Times are per call of the Python functions
(host <-> device copies included), median of --reps after one warm-up.

For comparison, the reference's project_thickness on the CPU (sklearn KernelPCA builds an n x n kernel matrix per plateau):
2.84 s at 20 480 TC points and 0.02 s at 65 000 FC points (16 threads).  --cpu times that KernelPCA call here as well."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oai_analysis_2_amd import mesh_processing as mp  # noqa: E402

EMPTY = np.zeros((0, 3), np.int32)


def fc_points(n, rng):
    phi = rng.uniform(np.pi - 1.1, np.pi + 1.1, n)
    rad = 31.0 + rng.normal(0.0, 0.4, n)
    return np.stack([48.0 + rad * np.sin(phi), 61.5 + rad * np.cos(phi), rng.uniform(10, 90, n)], axis=1).astype(np.float32)


def tc_points(n, rng):
    half = []
    for k, (centre, z) in enumerate((((40.0, 55.0), 30.0), ((42.0, 60.0), 72.0))):
        m = n // 2 if k == 0 else n - n // 2
        q = rng.normal(size=(m, 3)) * np.array([9.0, 5.0, 0.8])
        half.append(np.stack([centre[0] + q[:, 0], centre[1] + q[:, 1], np.clip(z + q[:, 2] + 0.2 * q[:, 0], 0, 49.9) if k == 0
                              else np.clip(z + q[:, 2] + 0.2 * q[:, 0], 50, 100)], axis=1))
    return np.concatenate(half).astype(np.float32)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu", action="store_true", help="also time sklearn KernelPCA on the TC plateaus (the reference's call)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0)}
    for kind, n, make in (("FC", 65000, fc_points), ("TC", 20480, tc_points)):
        src = make(n, rng)
        atlas = (src + rng.normal(0, 0.3, src.shape)).astype(np.float32)
        source = mp.Mesh(src, EMPTY, {"Distance": rng.uniform(0.5, 3.5, n).astype(np.float32)})
        target = mp.Mesh(atlas, EMPTY)
        mapped = mp.map_attributes(source, target)
        res[f"{kind}_points"] = n
        res[f"{kind}_map_attributes_grid_ms"] = 1e3 * timed(lambda: mp.map_attributes(source, target), args.reps)
        res[f"{kind}_map_attributes_brute_ms"] = 1e3 * timed(lambda: mp.map_attributes(source, target, broad_phase=False), max(2, args.reps // 4))
        res[f"{kind}_project_thickness_ms"] = 1e3 * timed(lambda: mp.project_thickness(mapped, kind), args.reps)
        if kind == "TC" and args.cpu:
            from sklearn.decomposition import KernelPCA
            z = atlas[:, 2].astype(np.float64)
            t = time.perf_counter()
            for sel in (z < 50, z >= 50):
                np.random.seed(0)
                KernelPCA(n_components=2, degree=3.0).fit_transform(atlas[sel].astype(np.float64))
            res["TC_sklearn_kernelpca_cpu_ms"] = 1e3 * (time.perf_counter() - t)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
