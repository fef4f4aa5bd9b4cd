#!/usr/bin/env python
"""Timings behind profiles/group_regression.md; prints one JSON line per row.

The input is SYNTHETIC, the cohort of scripts/group_stats_timing.py: N = 200 knees of 2 mm + 0.3 mm noise on 30 002 vertices, 5 % of
the entries missing.  The design is an intercept, a sex dummy, age (and at p = 6 two more continuous covariates) and a continuous x.

    python scripts/group_regression_timing.py device [--repeats 9] [--permutations 1000]
        ops.regression_t over all the rows in one call (gather, the per-row factor without a mask, the t kernel), device events around
        the call, warm, the median of ``--repeats``; between repeats a 512 MiB buffer is overwritten so that no input is left in the L2
        or the Infinity Cache.  p = 4 with and without a mask, p = 6 with a mask; ops.regression_prepare likewise; and, as the
        yardstick on the same machine, ops.permutation_t (two-sample, masked) on the same cohort.  Under
        ``rocprofv3 --kernel-trace --stats`` with ``--repeats 1`` the per-kernel times.
    python scripts/group_regression_timing.py numpy [--verts 1000] [--permutations 8]
        wall time of the numpy restatement (tests/group_regression_ref.py) on this machine's CPU for a slice of the same cohort,
        p = 4 with a mask, and its extrapolation to 30 002 vertices and 1000 rows (the work is proportional to both).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_KNEES, N_VERTS = 200, 30002


def cohort_arrays(n_verts=N_VERTS):
    rng = np.random.default_rng(200)
    Y = (2.0 + 0.3 * rng.normal(size=(N_KNEES, n_verts))).astype(np.float32)
    mask = rng.random((N_KNEES, n_verts)) >= 0.05
    return Y, mask


def design(p):
    rng = np.random.default_rng(p)
    cols = [np.ones(N_KNEES), (np.arange(N_KNEES) % 2).astype(np.float64), rng.uniform(45, 80, N_KNEES)]
    cols += [rng.normal(size=N_KNEES) for _ in range(p - 4)] + [rng.normal(size=N_KNEES)]
    D = np.stack(cols, axis=1)
    D[:, 2:] -= D[:, 2:].mean(axis=0)
    D[:, 1:] /= np.sqrt((D[:, 1:] ** 2).sum(axis=0))
    return np.ascontiguousarray(D)


def fp64_operations(p, masked):
    """Per (knee, row, vertex): b is a multiply and an add per column; with a mask M is one fused operation per entry of the triangle."""
    return 2 * p + (p * (p + 1) // 2 if masked else 0)


def _spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def device(args):
    import torch
    from oai_analysis_2_amd import _lib, ops, stats
    dev = torch.device("cuda", 0)
    Y, mask = cohort_arrays()
    Yd, md = torch.from_numpy(Y).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev)
    P = args.permutations
    index = torch.from_numpy(stats.index_permutations(N_KNEES, P, seed=0).index).to(dev)
    bits = torch.from_numpy(stats.label_permutations(np.arange(N_KNEES) % 2 == 0, P, seed=0).bits.view(np.int32)).to(dev)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    peak = 39.3e12                                                         # fp64 vector instructions x lanes per second (profiles/group_stats.md)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeats):
            flush.fill_(1)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            torch.cuda.synchronize()
            out.append(start.elapsed_time(stop))
        return _spread(out)

    group = ops.group_prepare(Yd, md)
    tile_ws = _lib.workspace("oai_permutation_t", dev, P, N_VERTS)
    ms = timed(lambda: ops.permutation_t(group, bits, 0, P, ops.STATS_TWO_SAMPLE, workspace=tile_ws))
    print(json.dumps({"row": "oai_permutation_t two-sample masked (yardstick)", "rows": P, "ms": ms, "fp64_operations_per_knee_row_vertex": 2,
                      "share_of_fp64_issue_rate": round(2 * P * N_VERTS * N_KNEES / (ms["median"] * 1e-3) / peak, 3)}), flush=True)
    del group, tile_ws
    for p, masked in ((4, True), (4, False), (6, True), (6, False)):
        D = design(p)
        Dd, Zd = torch.from_numpy(D).to(dev), torch.from_numpy(np.ascontiguousarray(D[:, :-1])).to(dev)
        m = md if masked else None
        prep_ms = timed(lambda: ops.regression_prepare(Yd, m, Zd))
        prepared = ops.regression_prepare(Yd, m, Zd)
        ws = _lib.workspace("oai_regression_t", dev, P, N_VERTS, N_KNEES, p)
        ms = timed(lambda: ops.regression_t(prepared, Dd, index, 0, P, workspace=ws))
        n_ops = fp64_operations(p, masked)
        print(json.dumps({"row": f"oai_regression_t p={p} {'masked' if masked else 'no mask'}", "rows": P, "ms": ms, "prepare_ms": prep_ms,
                          "fp64_operations_per_knee_row_vertex": n_ops, "workspace_MiB": round(ws.numel() / 2 ** 20, 1),
                          "share_of_fp64_issue_rate": round(n_ops * P * N_VERTS * N_KNEES / (ms["median"] * 1e-3) / peak, 3)}), flush=True)
        del prepared, ws


def restatement(args):
    import group_regression_ref as rref
    from oai_analysis_2_amd import stats
    Y, mask = cohort_arrays(args.verts)
    D = design(4)
    index = stats.index_permutations(N_KNEES, args.permutations, seed=0).index
    t0 = time.perf_counter()
    prep = rref.prepare(Y, mask, D[:, :-1])
    t1 = time.perf_counter()
    rref.regression_t(prep, mask, D, index)
    t2 = time.perf_counter()
    scale = (N_VERTS / args.verts) * (1000 / args.permutations)
    print(json.dumps({"row": "numpy p=4 masked", "n_knees": N_KNEES, "n_verts": args.verts, "rows": len(index), "cpus": os.cpu_count(),
                      "seconds": {"prepare": round(t1 - t0, 2), "t": round(t2 - t1, 2)},
                      "t_extrapolated_to_30002_vertices_and_1000_rows_seconds": round((t2 - t1) * scale, 1)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=("device", "numpy"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--permutations", type=int, default=None)
    ap.add_argument("--verts", type=int, default=1000)
    a = ap.parse_args()
    if a.permutations is None:
        a.permutations = 1000 if a.row == "device" else 8
    {"device": device, "numpy": restatement}[a.row](a)
