#!/usr/bin/env python
"""Timings and the normal-score error behind profiles/rank_transform.md; prints one JSON line per row.

The input is SYNTHETIC: N knees of 2 mm + 0.3 mm noise on 30 002 vertices (seed 200), 5 % of the entries missing where a mask is used.

    python scripts/rank_transform_timing.py [--repeats 9] [--knees 200 2000] [--skip-ranked]
        ops.column_ranks with and without a mask, plain and signed, per N: ms, and pair-compares (N^2 V, each a `<` and a `==`) per
        second against the VALU issue rate at 4 instructions per pair; ops.group_prepare of the same cohort beside it for scale;
        ops.rank_scores per kind; ThicknessCohort.ranked end to end (wall time).  Device events around each call, warm, the median of
        ``--repeats``; between repeats a 512 MiB buffer is overwritten so that no input is left in the L2 or the Infinity Cache.
    python scripts/rank_transform_timing.py --error
        the largest |device - scipy.special.ndtri| of the normal score over EVERY (n, twice_rank) with n <= 4096, the four named constants,
        and the extreme ranks of n = 2^22: the figure that tests/test_rank_transform_gpu.py takes its gate from.
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
ISSUE = 256 * 4 * 32 * 2.4e9                                              # VALU lane-instructions per second: CUs x SIMDs x lanes per cycle x clock
PER_PAIR = 4                                                               # v_cmp, v_addc for `<` and again for `==`
CONSTANTS = {"blom": 0.375, "tukey": 1.0 / 3.0, "rankit": 0.5, "waerden": 0.0}


def _spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def cohort_arrays(n_knees):
    rng = np.random.default_rng(200)
    Y = (2.0 + 0.3 * rng.normal(size=(n_knees, N_VERTS))).astype(np.float32)
    mask = rng.random((n_knees, N_VERTS)) >= 0.05
    return Y, mask


def error():
    import scipy.special
    import torch
    from oai_analysis_2_amd import ops
    dev = torch.device("cuda", 0)
    big = 1 << 22
    worst = {}
    for lo, hi in ((1, 1024), (1025, 2048), (2049, 3072), (3073, 4096), (big, big)):
        if lo == big:
            tr = np.array([2, 3, 4, 2 * big - 2, 2 * big - 1, 2 * big, -2, -2 * big], np.int32)[:, None]
            n = np.array([big], np.int32)
        else:
            n = np.arange(lo, hi + 1, dtype=np.int32)
            tr = np.arange(2, 2 * hi + 1, dtype=np.int32)[:, None] * np.ones((1, len(n)), np.int32)
            tr = np.where(tr <= 2 * n[None, :], tr, 0).astype(np.int32)
        tr_d, n_d = torch.from_numpy(tr).to(dev), torch.from_numpy(n).to(dev)
        valid = tr != 0
        r = 0.5 * np.abs(tr).astype(np.float64)
        for name, c in CONSTANTS.items():
            got = ops.rank_scores(tr_d, n_d, "normal", c)[0].cpu().numpy()
            with np.errstate(invalid="ignore"):
                want = np.where(tr < 0, -1.0, 1.0) * scipy.special.ndtri(np.where(valid, (r - c) / ((n[None, :].astype(np.float64) - 2.0 * c) + 1.0), 0.5))
            err = float(np.abs(np.where(valid, got - want, 0.0)).max())
            assert np.isfinite(got).all()
            worst[name] = max(worst.get(name, 0.0), err)
            print(json.dumps({"what": "normal score error", "n": [int(lo), int(hi)], "c": name, "entries": int(valid.sum()), "max_abs_error": err}), flush=True)
    print(json.dumps({"what": "normal score error, all", "per_constant": worst, "max_abs_error": max(worst.values())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--knees", type=int, nargs="+", default=[200, 2000])
    ap.add_argument("--skip-ranked", action="store_true")
    ap.add_argument("--error", action="store_true")
    args = ap.parse_args()
    if args.error:
        return error()
    import torch
    from oai_analysis_2_amd import mesh_processing as mp, ops, stats
    dev = torch.device("cuda", 0)
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

    for N in args.knees:
        def row(what, ms, **more):
            print(json.dumps({"what": what, "N": N, "V": N_VERTS, "ms": ms, **more}), flush=True)

        Y, mask = cohort_arrays(N)
        Yd, md = torch.from_numpy(Y).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev)
        pairs = N * N * N_VERTS
        for masked, m in ((True, md), (False, None)):
            for signed in (False, True):
                ms = timed(lambda: ops.column_ranks(Yd, m, signed=signed))
                per_s = pairs / (ms["median"] * 1e-3)
                row("oai_column_ranks", ms, masked=masked, signed=signed, pair_compares_per_s=float(f"{per_s:.4g}"),
                    issue_share=round(per_s * PER_PAIR / ISSUE, 4))
            row("oai_group_prepare (for scale)", timed(lambda: ops.group_prepare(Yd, m)), masked=masked)
        ranks = ops.column_ranks(Yd, md)
        for kind in ("rank", "centred", "normal"):
            row(f"oai_rank_scores, {kind}", timed(lambda: ops.rank_scores(ranks.twice_rank, ranks.n_valid, kind)), bytes_moved=N * N_VERTS * (4 + 8 + 1))
        del ranks
        if args.skip_ranked:
            continue
        atlas = SimpleNamespace(inner={"FC": mp.Mesh(np.zeros((N_VERTS, 3), np.float32), np.zeros((0, 3), np.int32))}, device=dev)
        cohort = stats.ThicknessCohort(atlas, "FC", chunk=N)
        cohort._values, cohort._mask, cohort.ids = Yd * md, md, list(range(N))
        for method in ("rank", "inormal", "signed"):
            wall = []
            for _ in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cohort.ranked(method)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            row(f"ThicknessCohort.ranked({method!r}), wall", _spread(wall[1:]), wall_first=round(wall[0], 2))
        del cohort, Yd, md


if __name__ == "__main__":
    main()
