#!/usr/bin/env python
"""Timings behind profiles/cluster_robust.md; prints one JSON line per row.

The input is SYNTHETIC: S subjects with 3 .. 7 visits each (five on average) of 2 mm + a random intercept (sd 0.3 mm) + 0.1 mm noise on
30 002 vertices, 5 % of the entries missing under a mask.  The design is an intercept, a sex dummy, years (and at p = 6 two more
continuous covariates) and years x group as the regressor of interest.

    python scripts/cluster_robust_timing.py device [--repeats 7] [--flips 1000] [--subjects 200 2000] [--columns 4 6] [--only-t]
        per (S, p, mask): ops.cluster_prepare (oai_regression_prepare + oai_cluster_prepare), oai_cluster_prepare alone, ops.cluster_t
        over all the flip rows in one call, stats.marginal_test end to end (wall clock, it ends in its one download) and, for scale,
        ops.regression_t at N = S knees and equal p.  Device events around each call, warm, the median of ``--repeats``; between repeats
        a 512 MiB buffer is overwritten so that no input is left in the L2 or the Infinity Cache.  ``--only-t``: the t kernel alone (the
        diagnostic libraries with another rows-per-thread table, loaded through OAI_LIB_PATH).  Under ``rocprofv3 --kernel-trace
        --stats`` with ``--repeats 1`` the per-kernel times.
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

N_VERTS = 30002
FP64_PEAK = 39.3e12                   # fp64 vector instructions x lanes per second (profiles/group_stats.md)
HBM_PEAK = 8.0e12                     # bytes per second (MI355X_MICROARCH.md)


def visits(S, p, n_verts=N_VERTS):
    rng = np.random.default_rng([S, p])
    counts = 3 + (np.arange(S) % 5)
    owner = np.repeat(np.arange(S), counts)
    N = len(owner)
    years = np.concatenate([np.arange(k, dtype=np.float64) + rng.uniform(0, 0.3, k) for k in counts])
    group = (np.arange(S) % 2).astype(np.float64)[owner]
    sex = ((np.arange(S) // 2) % 2).astype(np.float64)[owner]
    cov = [sex, years, group] + [rng.normal(size=N) for _ in range(p - 5)]
    Y = (2.0 + 0.3 * rng.normal(size=(S, n_verts)).astype(np.float32)[owner] + 0.1 * rng.normal(size=(N, n_verts)).astype(np.float32)).astype(np.float32)
    mask = rng.random((N, n_verts)) >= 0.05
    return Y, mask, owner, years * group, np.stack(cov[:p - 2], axis=1)


def rows_per_thread(p):               # csrc/cluster_robust.hip
    return 16 if p <= 4 else 8


def _spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def device(args):
    import torch
    from oai_analysis_2_amd import _lib, mesh_processing as mp, ops, stats
    dev = torch.device("cuda", 0)
    P = args.flips
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

    for S in args.subjects:
        for p in args.columns:
            Y, mask, owner, x, cov = visits(S, p)
            N, V = Y.shape
            _, order, offsets = stats.cluster_rows(owner.tolist())
            assert np.array_equal(order, np.arange(N))
            _, D, _ = stats._design_columns(x, cov, True, N)
            Yd, md = torch.from_numpy(Y).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev)
            Dd, od = torch.from_numpy(D).to(dev), torch.from_numpy(offsets).to(dev)
            bits = torch.from_numpy(np.ascontiguousarray(stats.sign_flips(S, P, seed=0).bits).view(np.int32)).to(dev)
            for masked in (True, False):
                m = md if masked else None
                row = {"row": f"S={S} N={N} p={p} {'masked' if masked else 'no mask'}", "flip_rows": P, "rows_shift": args.rows_shift}
                prepared = ops.cluster_prepare(Yd, m, Dd, od)
                if not args.only_t:
                    row["prepare_ms"] = timed(lambda: ops.cluster_prepare(Yd, m, Dd, od))
                    row["cluster_prepare_alone_ms"] = timed(lambda: _lib.call(
                        "oai_cluster_prepare", None if m is None else m.data_ptr(), Dd.data_ptr(), od.data_ptr(), N, V, S, p, prepared.block.data_ptr(),
                        prepared.block.numel(), _lib.STREAM, device=dev))
                ws = _lib.workspace("oai_cluster_t", dev, P, V)
                ms = timed(lambda: ops.cluster_t(prepared, bits, 0, P, workspace=ws))
                n_ops = (3 * p + 1) * P * V * S                                   # pass 1: p, pass 2: 2 p + 1, per (row, cluster, vertex)
                groups = -(-P // max(1, int(rows_per_thread(p) * 2.0 ** args.rows_shift)))
                read = (2 * p + 1) * S * V * 8 * groups                            # every row group streams the planes of its vertices
                once = (2 * p + 1) * S * V * 8 + P * V * 8                        # the planes once and the tile: what must cross the HBM
                sec = ms["median"] * 1e-3
                row.update(cluster_t_ms=ms, block_GiB=round(prepared.block.numel() / 2 ** 30, 2), fp64_operations=n_ops,
                           share_of_fp64_issue_rate=round(n_ops / sec / FP64_PEAK, 3), bytes_read_by_threads=read,
                           read_TB_per_s=round(read / sec / 1e12, 2), bytes_planes_once_and_tile=once,
                           share_of_hbm_bandwidth_if_read_once=round(once / sec / HBM_PEAK, 3))
                del ws
                if not args.only_t:
                    atlas = SimpleNamespace(inner={"FC": mp.Mesh(np.zeros((V, 3), np.float32), np.zeros((0, 3), np.int32))}, device=dev)
                    cohort = stats.ThicknessCohort(atlas, "FC")
                    cohort._values, cohort._mask, cohort.ids = Yd, (md if masked else torch.ones_like(md)), list(range(N))
                    wall = []
                    for _ in range(3):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        stats.marginal_test(cohort, x, covariates=cov, clusters=owner.tolist(), n_bootstrap=P, seed=0)
                        wall.append((time.perf_counter() - t0) * 1e3)
                    row["marginal_test_wall_ms"] = _spread(wall[1:])
                del prepared
                print(json.dumps(row), flush=True)
            if args.only_t:
                continue
            # for scale: the Freedman-Lane t of the parent commit on one row per subject, equal p
            first = torch.from_numpy(offsets[:-1].astype(np.int64)).to(dev)
            Ys, ms_ = Yd.index_select(0, first), md.index_select(0, first)
            Ds = torch.from_numpy(np.ascontiguousarray(stats._design_columns(x[offsets[:-1]] + np.arange(S) % 3, cov[offsets[:-1]], True, S)[1])).to(dev)
            index = torch.from_numpy(stats.index_permutations(S, P, seed=0).index).to(dev)
            for masked in (True, False):
                prep = ops.regression_prepare(Ys, ms_ if masked else None, Ds[:, :-1].contiguous())
                ws = _lib.workspace("oai_regression_t", dev, P, V, S, p)
                ms = timed(lambda: ops.regression_t(prep, Ds, index, 0, P, workspace=ws))
                n_ops = (2 * p + (p * (p + 1) // 2 if masked else 0)) * P * V * S
                print(json.dumps({"row": f"oai_regression_t (for scale) N={S} p={p} {'masked' if masked else 'no mask'}", "rows": P, "ms": ms,
                                  "share_of_fp64_issue_rate": round(n_ops / (ms["median"] * 1e-3) / FP64_PEAK, 3)}), flush=True)
                del prep, ws


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=("device",))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--flips", type=int, default=1000)
    ap.add_argument("--subjects", type=int, nargs="+", default=[200, 2000])
    ap.add_argument("--columns", type=int, nargs="+", default=[4, 6])
    ap.add_argument("--only-t", action="store_true")
    ap.add_argument("--rows-shift", type=int, default=0, help="the OAI_CLUSTER_ROWS_SHIFT of the diagnostic library that is loaded")
    device(ap.parse_args())
