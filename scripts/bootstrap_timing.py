#!/usr/bin/env python
"""Timings behind profiles/bootstrap.md; prints one JSON line per row.

The input is SYNTHETIC, the cohort and the designs of scripts/group_regression_timing.py: N = 200 knees of 2 mm + 0.3 mm noise on 30 002
vertices, 5 % of the entries missing; an intercept, a sex dummy, age and a continuous x (p = 4).  B = 2000 resamples (seed 0).

    python scripts/bootstrap_timing.py [--repeats 9] [--bootstrap 2000] [--skip-ci] [--columns 4] [--coef-only]
        ops.bootstrap_coef over all B + 1 rows in one call, with and without a mask, and -- the yardstick, same session -- ops.regression_t
        over as many index rows of the same cohort and design; ops.column_quantiles, ops.bootstrap_moments and ops.bootstrap_sup on the
        tile; stats.bootstrap_ci end to end per method (wall time, host steps and downloads included).  Device events around each call,
        warm, the median of ``--repeats``; between repeats a 512 MiB buffer is overwritten so that no input is left in the L2 or the
        Infinity Cache.  ``--columns 1 2 3 4 5 6 --coef-only``: the coefficient kernel and its yardstick alone, per p (below p = 4 the
        design is a subset of the p = 4 columns that ends in x): the rows-per-thread table of csrc/bootstrap.hip was chosen with it.
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

from group_regression_timing import N_KNEES, N_VERTS, _spread, cohort_arrays, design  # noqa: E402

PEAK = 39.3e12                                                             # fp64 vector instructions x lanes per second (profiles/group_stats.md)


def bootstrap_operations(p, masked):
    """Per (knee, row, vertex): u is a multiply; h a multiply and an add per column; with a mask M a multiply and an add per entry."""
    return 1 + 2 * p + (p * (p + 1) if masked else 0)


def regression_operations(p, masked):
    return 2 * p + (p * (p + 1) // 2 if masked else 0)


def design_of(p):
    return design(p) if p >= 4 else np.ascontiguousarray(design(4)[:, {1: [3], 2: [0, 3], 3: [0, 1, 3]}[p]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--bootstrap", type=int, default=2000)
    ap.add_argument("--skip-ci", action="store_true")
    ap.add_argument("--columns", type=int, nargs="+", default=[4])
    ap.add_argument("--coef-only", action="store_true")
    args = ap.parse_args()
    import torch
    from oai_analysis_2_amd import _lib, mesh_processing as mp, ops, stats
    dev = torch.device("cuda", 0)
    Y, mask = cohort_arrays()
    Yd, md = torch.from_numpy(Y).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev)
    B = args.bootstrap
    R = B + 1
    counts = torch.from_numpy(stats.bootstrap_counts(N_KNEES, B, seed=0).counts).to(dev)
    index = torch.from_numpy(stats.index_permutations(N_KNEES, R, seed=0).index).to(dev)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

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

    def row(what, ms, **more):
        print(json.dumps({"what": what, "N": N_KNEES, "V": N_VERTS, "p": p, "rows": R, "ms": ms, **more}), flush=True)

    work = N_KNEES * R * N_VERTS
    for p in args.columns:
        Dd = torch.from_numpy(design_of(p)).to(dev)
        ws = _lib.workspace("oai_bootstrap_coef", dev, R, N_VERTS, N_KNEES, p)
        ws_t = _lib.workspace("oai_regression_t", dev, R, N_VERTS, N_KNEES, p)
        for masked, m in ((True, md), (False, None)):
            ms = timed(lambda: ops.bootstrap_coef(Yd, Dd, counts, 0, R, mask=m, workspace=ws))
            prep = ops.regression_prepare(Yd, m, Dd[:, :-1].contiguous() if p > 1 else None, centre=p > 1)
            ms_t = timed(lambda: ops.regression_t(prep, Dd, index, 0, R, workspace=ws_t))
            row("oai_bootstrap_coef", ms, masked=masked, operations=bootstrap_operations(p, masked),
                issue_share=round(work * bootstrap_operations(p, masked) / (ms["median"] * 1e-3) / PEAK, 4))
            row("oai_regression_t (yardstick)", ms_t, masked=masked, operations=regression_operations(p, masked),
                issue_share=round(work * regression_operations(p, masked) / (ms_t["median"] * 1e-3) / PEAK, 4),
                bootstrap_over_t=round(ms["median"] / ms_t["median"], 3))
            del prep
        del ws_t
    if args.coef_only:
        return
    tile = ops.bootstrap_coef(Yd, Dd, counts, 0, R, mask=md, workspace=ws)
    ws_q = _lib.workspace("oai_column_quantiles", dev, R, N_VERTS)
    ms = timed(lambda: ops.column_quantiles(tile, (0.025, 0.975), first_row=1, workspace=ws_q))
    moved = 8 * B * N_VERTS * (2 + 9)                                      # the tile read and the keys written once; the keys read by the count and 8 passes
    row("oai_column_quantiles, 2 shared probabilities", ms, bytes_tile=8 * B * N_VERTS, bytes_moved=moved,
        gb_per_s=round(moved / (ms["median"] * 1e-3) / 1e9, 1))
    per_vertex = torch.rand((2, N_VERTS), dtype=torch.float64, device=dev)
    row("oai_column_quantiles, 2 per-vertex probabilities", timed(lambda: ops.column_quantiles(tile, per_vertex, first_row=1, workspace=ws_q)))
    mom = ops.bootstrap_moments(tile)
    row("oai_bootstrap_moments", timed(lambda: ops.bootstrap_moments(tile)), bytes_moved=2 * 8 * R * N_VERTS)
    sup = torch.zeros(R, dtype=torch.float64, device=dev)
    row("oai_bootstrap_sup", timed(lambda: ops.bootstrap_sup(tile, mom.se, sup)), bytes_moved=8 * R * N_VERTS)
    del tile, ws, ws_q, flush
    if args.skip_ci:
        return
    atlas = SimpleNamespace(inner={"FC": mp.Mesh(np.zeros((N_VERTS, 3), np.float32), np.zeros((0, 3), np.int32))}, device=dev)
    cohort = stats.ThicknessCohort(atlas, "FC", chunk=N_KNEES)
    Ynan = np.where(mask, Y, np.nan).astype(np.float32)
    for r in Ynan:
        cohort.add_vector(r)
    age, x = design(4)[:, 2], design(4)[:, 3]
    for method in stats.BOOTSTRAP_METHODS:
        for simultaneous in (False, True):
            wall = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stats.bootstrap_ci(cohort, x=x, covariates=np.stack([np.arange(N_KNEES) % 2, age], axis=1), n_bootstrap=B, method=method,
                                   simultaneous=simultaneous)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            row(f"stats.bootstrap_ci, slope, {method}" + (", simultaneous" if simultaneous else ""), _spread(wall[1:]), wall_first=round(wall[0], 1))


if __name__ == "__main__":
    main()
