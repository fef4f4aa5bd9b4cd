#!/usr/bin/env python
"""Timings behind profiles/normative.md; prints one JSON line per row.

The input is SYNTHETIC, on the sphere of scripts/group_stats_timing.py (30 002 vertices, 20 mm radius): N = 200 and N = 2000 reference
knees of 2.4 mm + 0.3 mm noise with a design of p = 4 columns (intercept, age ~ N(60, 9), a 0 / 1 column, BMI ~ N(28, 4), centred), with a
mask that drops 5 % of the entries and without one.

    python scripts/bench_normative.py [--repeats 9] [--knees 200 2000] [--columns 4]
        Device events around each call, warm, the median of ``--repeats``:
          fit            ops.normative_fit                                   bytes: 2 passes x N x V x (4 + 1), plus the model block
          loo            ops.normative_score of the N reference rows, loo    bytes: N x V x (4 + 1 + 8), plus the model block once
          loo_diff       the same with the deviation in mm                   bytes: N x V x (4 + 1 + 16)
          new_knee       ops.normative_score of ONE row, not in the fit      bytes: the model block + V x (4 + 1 + 8)
          summary        ops.deviation_summary of the N-row tile             bytes: N x V x 8 (+ V x 8 of weights)
          clusters       ops.graph_clusters of the N-row tile (rows = knees), in batches within stats.WORKSPACE_BUDGET
          group_prepare  ops.group_prepare at the same N and V, the yardstick from the code that was there before: 2 passes of the same
                         loads and 16 bytes written per entry
        Every row reports ms, the bytes it must move and the rate that makes.  ``model.loo()`` and ``model.deviation()`` of one knee are
        timed end to end (host wall clock, downloads included) on top.
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

from group_stats_timing import _spread, sphere  # noqa: E402


def _timed(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        ms.append(start.elapsed_time(stop))
    return _spread(ms)


def _row(name, N, masked, spread, nbytes=None, **more):
    row = {"what": name, "knees": N, "mask": masked, "ms": spread}
    if nbytes is not None:
        row.update(MB=round(nbytes / 1e6, 1), TB_per_s=round(nbytes / (spread["median"] * 1e-3) / 1e12, 3))
    row.update(more)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--knees", type=int, nargs="+", default=[200, 2000])
    ap.add_argument("--columns", type=int, default=4)
    args = ap.parse_args()
    import torch
    from oai_analysis_2_amd import mesh_processing as mp, ops, stats
    verts, faces = sphere()
    V, p = len(verts), args.columns
    atlas = SimpleNamespace(inner={"FC": mp.Mesh(verts.astype(np.float32), faces)}, device=torch.device("cuda", 0))
    dev = atlas.device
    for N in args.knees:
        rng = np.random.default_rng(N)
        cov = np.stack([rng.normal(60.0, 9.0, N), (np.arange(N) % 2).astype(np.float64), rng.normal(28.0, 4.0, N), rng.normal(size=N),
                        rng.normal(size=N)], axis=1)[:, :p - 1]
        design, means, scales, _ = stats._normative_design(cov, True, N)
        Y = torch.from_numpy((2.4 + 0.3 * rng.normal(size=(N, V))).astype(np.float32)).to(dev)
        drop = torch.from_numpy((rng.random((N, V)) >= 0.05).astype(np.uint8)).to(dev)
        Z = torch.from_numpy(design).to(dev)
        block_bytes = int(ops.normative_block(V, p, dev).block.numel())
        cohort = stats.ThicknessCohort(atlas, "FC", chunk=N)
        cohort._values, cohort._mask, cohort.ids = Y, drop, list(range(N))
        offsets, neighbours = cohort.surface_graph()
        weights = torch.from_numpy(stats.tfce_weights(cohort.vertex_areas())).to(dev)
        for masked in (True, False):
            mask = drop if masked else None
            mb = 1 if masked else 0
            _row("fit", N, masked, _timed(lambda: ops.normative_fit(Y, Z, mask), args.repeats), 2 * N * V * (4 + mb) + block_bytes, columns=p)
            model = ops.normative_fit(Y, Z, mask)
            ws = torch.empty(N * V * 8 + 256, dtype=torch.uint8, device=dev)
            diff = torch.empty((N, V), dtype=torch.float64, device=dev)
            _row("loo", N, masked, _timed(lambda: ops.normative_score(model, Y, Z, mask, loo=True, workspace=ws), args.repeats),
                 N * V * (4 + mb + 8) + block_bytes)
            _row("loo_diff", N, masked, _timed(lambda: ops.normative_score(model, Y, Z, mask, loo=True, workspace=ws, diff=diff), args.repeats),
                 N * V * (4 + mb + 16))
            _row("new_knee", N, masked, _timed(lambda: ops.normative_score(model, Y[:1], Z[:1], None if mask is None else mask[:1], loo=False,
                                                                           workspace=ws), args.repeats), block_bytes + V * (4 + mb + 8))
            tile = ops.normative_score(model, Y, Z, mask, loo=True, workspace=ws)
            _row("summary", N, masked, _timed(lambda: ops.deviation_summary(tile, 2.0, weights), args.repeats), N * V * 8 + V * 8)
            rows = int(max(1, min(N, stats.WORKSPACE_BUDGET // (V * stats._DEVIATION_BYTES))))
            extent = torch.empty(N, dtype=torch.int32, device=dev)

            def clusters():
                for r0 in range(0, N, rows):
                    ops.graph_clusters(tile[r0:r0 + rows], offsets, neighbours, 2.0, max_extent=extent[r0:r0 + rows])
            _row("clusters", N, masked, _timed(clusters, args.repeats), batch_rows=rows)
            _row("group_prepare", N, masked, _timed(lambda: ops.group_prepare(Y, mask), args.repeats), 2 * N * V * (4 + mb) + N * V * 16)
            del tile, ws, diff, model
        # the public path, end to end on the host clock: fit, the members, one new knee
        for what, fn in (("NormativeModel.fit + loo()", lambda: stats.NormativeModel.fit(cohort, cov).loo()),
                         ("deviation() of one knee", None)):
            if fn is None:
                fitted = stats.NormativeModel.fit(cohort, cov)
                fitted.reference(2.0)
                knee, row = Y[0].clone(), cov[0]
                fn = lambda: fitted.deviation(knee, covariates=row)            # noqa: E731
            fn()
            torch.cuda.synchronize()
            wall = []
            for _ in range(max(args.repeats // 3, 3)):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall.append(1e3 * (time.perf_counter() - t0))
            _row(what, N, True, _spread(wall))
        del Y, drop, cohort
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
