#!/usr/bin/env python
"""Timings behind profiles/group_stats.md; prints one JSON line per row.

The input is SYNTHETIC: a latitude / longitude sphere of 150 x 200 + 2 = 30 002 vertices (radius 20 mm) stands for the atlas inner
surface, and N = 200 knees are 2 mm + 0.3 mm noise on it, 5 % of the entries missing, 100 knees per group.

    python scripts/group_stats_timing.py device [--rounds 5] [--permutations 1000]
        stats.two_sample_test without and with a cluster threshold, alternating round by round in one process: host clock around the
        call (it ends in its one download), warm.  Under ``rocprofv3 --kernel-trace --stats`` with ``--rounds 1`` the per-kernel times:
        the run then holds one warm-up and one timed test of either kind, so every kernel of the test without clusters is launched
        four times as often as the test launches it, the cluster kernel twice as often.
    python scripts/group_stats_timing.py numpy [--permutations 100]
        wall time of the numpy restatement (tests/group_stats_ref.py) on this machine's CPU for the same cohort: t, max |t| and the
        exceedance counts, and then the clusters too.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_KNEES, RINGS, SEGMENTS, RADIUS, THRESHOLD = 200, 150, 200, 20.0, 3.0


def sphere():
    """(verts float32 [RINGS * SEGMENTS + 2, 3], faces int32): rings of SEGMENTS vertices between two poles."""
    lat = np.pi * (np.arange(RINGS) + 1) / (RINGS + 1)
    lon = 2 * np.pi * np.arange(SEGMENTS) / SEGMENTS
    ring = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.outer(np.sin(lat), np.sin(lon)), np.outer(np.cos(lat), np.ones(SEGMENTS))], axis=2)
    verts = np.concatenate([ring.reshape(-1, 3), [[0, 0, 1], [0, 0, -1]]]) * RADIUS
    at = lambda r, s: r * SEGMENTS + s % SEGMENTS
    r, s = np.meshgrid(np.arange(RINGS - 1), np.arange(SEGMENTS), indexing="ij")
    quads = np.concatenate([np.stack([at(r, s), at(r + 1, s), at(r, s + 1)], axis=2).reshape(-1, 3),
                            np.stack([at(r, s + 1), at(r + 1, s), at(r + 1, s + 1)], axis=2).reshape(-1, 3)])
    s = np.arange(SEGMENTS)
    north, south = RINGS * SEGMENTS, RINGS * SEGMENTS + 1
    caps = np.concatenate([np.stack([np.full(SEGMENTS, north), at(0, s), at(0, s + 1)], axis=1),
                           np.stack([np.full(SEGMENTS, south), at(RINGS - 1, s + 1), at(RINGS - 1, s)], axis=1)])
    return verts.astype(np.float32), np.concatenate([quads, caps]).astype(np.int32)


def cohort_arrays(n_verts):
    rng = np.random.default_rng(200)
    Y = (2.0 + 0.3 * rng.normal(size=(N_KNEES, n_verts))).astype(np.float32)
    mask = rng.random((N_KNEES, n_verts)) >= 0.05
    return Y, mask, np.arange(N_KNEES) % 2 == 0


def _spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def device(args):
    import torch
    from oai_analysis_2_amd import mesh_processing as mp, stats
    verts, faces = sphere()
    atlas = SimpleNamespace(inner={"FC": mp.Mesh(verts, faces)}, device=torch.device("cuda", 0))
    Y, mask, groups = cohort_arrays(len(verts))
    cohort = stats.ThicknessCohort(atlas, "FC", chunk=N_KNEES)
    for y, m in zip(Y, mask):
        cohort.add_vector(y, valid=m)
    perms = stats.label_permutations(groups, args.permutations, seed=0)
    variants = {"two_sample_test": None, "two_sample_test_clusters": THRESHOLD}

    def ms(threshold):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = stats.two_sample_test(cohort, groups, permutations=perms, cluster_threshold=threshold)
        return 1e3 * (time.perf_counter() - t), res

    for thr in variants.values():
        ms(thr)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, thr in variants.items():
            t, res = ms(thr)
            times[name].append(t)
    V, P = len(verts), len(perms)
    print(json.dumps({"row": "device", "n_knees": N_KNEES, "n_verts": V, "n_faces": len(faces), "permutations": P,
                      "batch": {"plain": stats.default_batch(V, P, False), "clusters": stats.default_batch(V, P, True)},
                      "fp64_operations_of_the_t_kernel": 2 * P * V * N_KNEES, "ms_per_test": {k: _spread(v) for k, v in times.items()},
                      "observed": {"max_abs": float(res.max_abs[0]), "p_fwer_min": float(np.nanmin(res.p_fwer)), "clusters": len(res.clusters),
                                   "largest_null_extent": int(res.max_extent.max())}}), flush=True)


def restatement(args):
    import group_stats_ref as gref
    from oai_analysis_2_amd import mesh_processing as mp, stats
    verts, faces = sphere()
    Y, mask, groups = cohort_arrays(len(verts))
    rows = stats.label_permutations(groups, args.permutations, seed=0).rows()
    t0 = time.perf_counter()
    t = gref.permutation_t(gref.prepare(Y, mask), mask, rows, gref.TWO_SAMPLE)
    gref.reduce_tiles(t)
    t1 = time.perf_counter()
    off, nbr = mp.vertex_adjacency(len(verts), faces)
    gref.clusters(t, off, nbr, THRESHOLD)
    t2 = time.perf_counter()
    print(json.dumps({"row": "numpy", "n_knees": N_KNEES, "n_verts": len(verts), "permutations": len(rows), "cpus": os.cpu_count(),
                      "seconds": {"t_max_exceed": round(t1 - t0, 2), "clusters_scipy": round(t2 - t1, 2)}}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=("device", "numpy"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--permutations", type=int, default=None)
    a = ap.parse_args()
    if a.permutations is None:
        a.permutations = 1000 if a.row == "device" else 100
    {"device": device, "numpy": restatement}[a.row](a)
