#!/usr/bin/env python
"""Timings behind profiles/vertex_covariates.md; prints one JSON line per row.

The input is SYNTHETIC, the cohort and the designs of scripts/group_regression_timing.py: N = 200 knees of 2 mm + 0.3 mm noise on 30 002
vertices, 5 % of the entries missing; the per-vertex columns are maps of 2.5 mm + 0.4 mm noise with 5 % of their entries missing,
independently.  The global columns are the first p - S nuisance columns of that script's design and its x.

    python scripts/vertex_covariates_timing.py kernel [--repeats 9] [--permutations 1000] [--shapes 4:1,6:2]
        ops.regression_vx_t over all the rows in one call (the gather and the hot kernel) beside ops.regression_t with a mask at the same
        p, in the same process on the same build: device events around the call, warm, the median of ``--repeats``; between repeats a
        512 MiB buffer is overwritten so that no input is left in the L2 or the Infinity Cache.  ops.regression_vx_prepare beside
        ops.regression_prepare likewise.  ``--shapes``: p:S pairs.  With OAI_LIB_PATH naming a diagnostic build made with
        -DOAI_VX_ROWS_SHIFT=1 or -1, the same rows with the rows-per-thread table doubled or halved.
    python scripts/vertex_covariates_timing.py test [--permutations 1000]
        stats.regression_test end to end (upload of the design, prepare, every batch, the one download) with and without
        ``vertex_covariates``, p = 4 in all either way: a host clock around the call, which ends in its download, warm, median of 5.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from group_regression_timing import N_KNEES, N_VERTS, _spread, cohort_arrays, design, fp64_operations  # noqa: E402


def map_arrays(S):
    rng = np.random.default_rng(300)
    W = (2.5 + 0.4 * rng.normal(size=(S, N_KNEES, N_VERTS))).astype(np.float32)
    wmask = rng.random((S, N_KNEES, N_VERTS)) >= 0.05
    return np.where(wmask, W, np.float32(0)), wmask


def vx_operations(p, S):
    """Per (knee, row, vertex): those of the masked kernel at the same p, and one multiply more for every entry of M's triangle that has a
    per-vertex factor -- all but the (p - S)(p - S + 1) / 2 global x global ones, which come from the table."""
    pg = p - S
    return fp64_operations(p, True) + p * (p + 1) // 2 - pg * (pg + 1) // 2


def design_of(p):
    """The design of scripts/group_regression_timing.py from four columns on; below that an intercept and standard normal columns."""
    if p >= 4:
        return design(p)
    rng = np.random.default_rng(p)
    return np.ascontiguousarray(np.stack([np.ones(N_KNEES)] + [rng.normal(size=N_KNEES) for _ in range(p - 1)], axis=1))


def kernel(args):
    import torch
    from oai_analysis_2_amd import _lib, ops, stats
    dev = torch.device("cuda", 0)
    Y, mask = cohort_arrays()
    Yd, md = torch.from_numpy(Y).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev)
    P = args.permutations
    index = torch.from_numpy(stats.index_permutations(N_KNEES, P, seed=0).index).to(dev)
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

    for p, S in args.shapes:
        D = design_of(p)
        Dd, Zd = torch.from_numpy(D).to(dev), torch.from_numpy(np.ascontiguousarray(D[:, :-1])).to(dev)
        row = {"p": p, "S": S, "rows": P, "lib": os.path.basename(_lib.LIB_PATH)}
        if p >= 2:                                                         # the yardstick: the masked t kernel at the same p
            row["regression_prepare_ms"] = timed(lambda: ops.regression_prepare(Yd, md, Zd))
            prepared = ops.regression_prepare(Yd, md, Zd)
            ws = _lib.workspace("oai_regression_t", dev, P, N_VERTS, N_KNEES, p)
            row["regression_t_masked_ms"] = timed(lambda: ops.regression_t(prepared, Dd, index, 0, P, workspace=ws))
            del prepared, ws
        W, wmask = map_arrays(S)
        Wd, wd = torch.from_numpy(W).to(dev), torch.from_numpy(wmask.astype(np.uint8)).to(dev)
        # the maps stand for the S columns after the intercept; where that leaves the intercept alone (or nothing), the last map is x
        G = np.ascontiguousarray(np.delete(D, slice(1, 1 + S), axis=1)) if p > 1 else np.zeros((N_KNEES, 0))
        si = 1 if G.shape[1] <= 1 else 0
        Gd = torch.from_numpy(G).to(dev) if G.shape[1] else None
        nuisance = G if si else G[:, :-1]
        Nd = torch.from_numpy(np.ascontiguousarray(nuisance)).to(dev) if nuisance.shape[1] else None
        row["regression_vx_prepare_ms"] = timed(lambda: ops.regression_vx_prepare(Yd, md, Wd, wd, Nd, n_vertex_interest=si))
        prepared = ops.regression_vx_prepare(Yd, md, Wd, wd, Nd, n_vertex_interest=si)
        ws = _lib.workspace("oai_regression_vx_t", dev, P, N_VERTS, N_KNEES, p, S)
        ms = timed(lambda: ops.regression_vx_t(prepared, Gd, index, 0, P, workspace=ws))
        n_ops = vx_operations(p, S)
        row.update(regression_vx_t_ms=ms, fp64_operations_per_knee_row_vertex=n_ops, workspace_MiB=round(ws.numel() / 2 ** 20, 1),
                   share_of_fp64_issue_rate=round(n_ops * P * N_VERTS * N_KNEES / (ms["median"] * 1e-3) / peak, 3))
        if "regression_t_masked_ms" in row:
            row["ratio_to_masked_t"] = round(ms["median"] / row["regression_t_masked_ms"]["median"], 3)
        print(json.dumps(row), flush=True)
        del prepared, ws, Wd, wd


def test(args):
    import torch
    from oai_analysis_2_amd import mesh_processing as mp, stats
    dev = torch.device("cuda", 0)
    atlas = SimpleNamespace(inner={"FC": mp.Mesh(np.zeros((N_VERTS, 3), np.float32), np.zeros((0, 3), np.int32))}, device=dev)
    Y, mask = cohort_arrays()
    W, wmask = map_arrays(1)

    def cohort(values, valid):
        c = stats.ThicknessCohort(atlas, "FC", chunk=N_KNEES)
        for row, ok in zip(values, valid):
            c.add_vector(row, None, ok)
        return c

    rates, base = cohort(Y, mask), cohort(W[0], wmask[0])
    D = design(4)
    x, cov3, cov2 = D[:, 3], D[:, 1:3], D[:, 1:2]

    def clocked(fn):
        fn()
        out = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                           # ends in its download
            out.append((time.perf_counter() - t0) * 1e3)
        return _spread(out)

    P = args.permutations
    print(json.dumps({"row": "regression_test p=4, global columns only", "rows": P,
                      "ms": clocked(lambda: stats.regression_test(rates, x, covariates=cov3, n_permutations=P))}), flush=True)
    print(json.dumps({"row": "regression_test p=4, one of them vertex_covariates", "rows": P,
                      "ms": clocked(lambda: stats.regression_test(rates, x, covariates=cov2, vertex_covariates=base, n_permutations=P))}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=("kernel", "test"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--permutations", type=int, default=1000)
    ap.add_argument("--shapes", default="4:1,6:2")
    a = ap.parse_args()
    a.shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    {"kernel": kernel, "test": test}[a.row](a)
