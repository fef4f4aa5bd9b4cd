#!/usr/bin/env python
"""Timings behind profiles/group_tfce.md; prints one JSON line per row.

The input is SYNTHETIC, the cohort of scripts/group_stats_timing.py: a latitude / longitude sphere of 30 002 vertices, N = 200 knees of
2 mm + 0.3 mm noise, 5 % of the entries missing, 100 knees per group; P = 1000 labellings; TFCE with dh = 0.1, E = 1, H = 2, area extent.

    python scripts/group_tfce_timing.py test [--rounds 9] [--permutations 1000]
        stats.two_sample_test without and with ``tfce``, alternating round by round in one process: host clock around the call (it ends
        in its one download), warm.
    python scripts/group_tfce_timing.py kernel [--repeats 9] [--permutations 1000]
        On the t tile of the first batch of the test with tfce (``stats.default_batch(V, P, False, tfce=True)`` labellings), device events
        around the call, warm, the median of ``--repeats``: ops.graph_tfce, and the yardstick from the code that was there before it --
        ops.graph_clusters, one pass per level, which is what TFCE costs when it is composed of cluster passes (the passes alone: the
        composition would also have to turn each pass's sizes into its term and add it).  The yardstick is given two ways: one pass at
        |t| > 3.0 (the figure of profiles/group_stats.md) times the tile's largest level count K, and the sum of the K passes really
        run at the thresholds k * dh.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from group_stats_timing import N_KNEES, THRESHOLD, _spread, cohort_arrays, sphere  # noqa: E402

DH = 0.1


def _cohort():
    import torch
    from oai_analysis_2_amd import mesh_processing as mp, stats
    verts, faces = sphere()
    atlas = SimpleNamespace(inner={"FC": mp.Mesh(verts, faces)}, device=torch.device("cuda", 0))
    Y, mask, groups = cohort_arrays(len(verts))
    cohort = stats.ThicknessCohort(atlas, "FC", chunk=N_KNEES)
    for y, m in zip(Y, mask):
        cohort.add_vector(y, valid=m)
    return cohort, groups


def test(args):
    import torch
    from oai_analysis_2_amd import stats
    cohort, groups = _cohort()
    perms = stats.label_permutations(groups, args.permutations, seed=0)
    variants = {"two_sample_test": None, "two_sample_test_tfce": stats.TFCE(dh=DH)}

    def ms(tfce):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = stats.two_sample_test(cohort, groups, permutations=perms, tfce=tfce)
        return 1e3 * (time.perf_counter() - t), res

    for tfce in variants.values():
        ms(tfce)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, tfce in variants.items():
            t, res = ms(tfce)
            times[name].append(t)
    V, P = cohort.n_verts, len(perms)
    print(json.dumps({"row": "test", "n_knees": N_KNEES, "n_verts": V, "permutations": P, "dh": DH,
                      "batch": {"plain": stats.default_batch(V, P, False), "tfce": stats.default_batch(V, P, False, tfce=True)},
                      "ms_per_test": {k: _spread(v) for k, v in times.items()},
                      "observed": {"max_abs": float(res.max_abs[0]), "max_tfce": float(res.max_tfce[0]), "p_fwer_min": float(np.nanmin(res.p_fwer)),
                                   "p_tfce_min": float(np.nanmin(res.p_tfce)), "tfce_clipped": res.tfce_clipped}}), flush=True)


def kernel(args):
    import torch
    from oai_analysis_2_amd import ops, stats
    cohort, groups = _cohort()
    dev = cohort.device
    V, P = cohort.n_verts, args.permutations
    rows = stats.default_batch(V, P, False, tfce=True)
    bits = torch.from_numpy(stats.label_permutations(groups, P, seed=0).bits.view(np.int32)).to(dev)
    tile = ops.permutation_t(ops.group_prepare(cohort.values, cohort.mask), bits, 0, rows, ops.STATS_TWO_SAMPLE).clone()
    off, nbr = cohort.surface_graph()
    weights = torch.from_numpy(stats.tfce_weights(cohort.vertex_areas())).to(dev)
    levels = int(torch.nan_to_num(tile.abs(), nan=0.0).max().item() / DH)
    out = torch.empty_like(tile)
    extent = torch.empty(rows, dtype=torch.int32, device=dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            torch.cuda.synchronize()
            ms.append(start.elapsed_time(stop))
        return _spread(ms)

    def every_level():
        for k in range(1, levels + 1):
            ops.graph_clusters(tile, off, nbr, k * DH, max_extent=extent)

    tfce_ms = timed(lambda: ops.graph_tfce(tile, off, nbr, dh=DH, weights=weights, unit=2.0 ** -20, out=out))
    count_ms = timed(lambda: ops.graph_tfce(tile, off, nbr, dh=DH, out=out))
    one_ms = timed(lambda: ops.graph_clusters(tile, off, nbr, THRESHOLD, max_extent=extent))
    all_ms = timed(every_level)
    print(json.dumps({"row": "kernel", "rows": rows, "n_verts": V, "dh": DH, "largest_level_count": levels,
                      "graph_tfce_ms": tfce_ms, "graph_tfce_vertex_count_ms": count_ms,
                      "graph_clusters_one_pass_at_3.0_ms": one_ms, "one_pass_times_levels_ms": round(one_ms["median"] * levels, 2),
                      "graph_clusters_every_level_ms": all_ms}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=("test", "kernel"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--permutations", type=int, default=1000)
    a = ap.parse_args()
    {"test": test, "kernel": kernel}[a.row](a)
