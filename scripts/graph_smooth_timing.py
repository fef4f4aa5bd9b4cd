#!/usr/bin/env python
"""Timings behind profiles/surface_smoothing.md; prints one JSON line per row.

The input of ``kernel`` and ``cohort`` is SYNTHETIC, the cohort of scripts/group_stats_timing.py: a latitude / longitude sphere of 30 002
vertices and 20 mm radius, N = 200 knees of 2 mm + 0.3 mm noise, 5 % of the entries missing.  The sweep count K is the one that
``stats.SurfaceSmoother`` derives for ``--fwhm`` (5 mm) on that mesh.

    python scripts/graph_smooth_timing.py kernel [--repeats 9] [--fwhm 5.0]
        Device events around the call, warm, the median of ``--repeats``: ops.graph_smooth of the float64 [200, V] tile with K sweeps and
        with one (the difference over K - 1 is the cost of a sweep without the two transposes), in keep and in fill mode, with and without
        a mask, and with the CSR rows of the stand-in's two degree-200 poles emptied; and the yardstick from code that was there before
        it -- torch.sparse.mm of the row-normalised float64 CSR operator applied K times on the device to the [V, 200] matrix, nothing
        missing (it does less: it handles no missing data).  Also the floor:
        (2 * 8 + 2) * N * V bytes per sweep at 6.3 TB/s plus K kernel boundaries of 1.5 .. 1.9 us.
    python scripts/graph_smooth_timing.py cohort [--rounds 9] [--fwhm 5.0]
        ``ThicknessCohort.smoothed`` end to end (widen, smooth, round to float32), device events, warm.
    python scripts/graph_smooth_timing.py inference [--permutations 2000]
        The painted-cap cohort of tests/test_graph_tfce_gpu.py (+0.10 mm on the 61 cap vertices of a 642-vertex sphere, 24 knees):
        cap vertices with p_fwer <= 0.05 and with p_tfce <= 0.05, unsmoothed and smoothed at two FWHMs.  Reported, not asserted.
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from group_stats_timing import N_KNEES, _spread, cohort_arrays, sphere  # noqa: E402

HBM_BYTES_PER_S, BOUNDARY_US = 6.3e12, (1.5, 1.9)


def _cohort():
    import torch
    from oai_analysis_2_amd import mesh_processing as mp, stats
    verts, faces = sphere()
    atlas = SimpleNamespace(inner={"FC": mp.Mesh(verts.astype(np.float32), faces)}, device=torch.device("cuda", 0))
    Y, mask, _ = cohort_arrays(len(verts))
    cohort = stats.ThicknessCohort(atlas, "FC", chunk=N_KNEES)
    for y, m in zip(Y, mask):
        cohort.add_vector(y, valid=m)
    return cohort


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


def kernel(args):
    import torch
    from oai_analysis_2_amd import ops, stats
    cohort = _cohort()
    smoother = stats.SurfaceSmoother(cohort.atlas, "FC", args.fwhm, graph=cohort.surface_graph())
    off, nbr = smoother.graph
    K, V, N = smoother.sweeps, cohort.n_verts, len(cohort)
    tile, mask = cohort.values.to(torch.float64), cohort.mask.clone()
    out, out_mask = torch.empty_like(tile), torch.empty_like(mask)

    def run(sweeps, fill, with_mask):
        return _timed(lambda: ops.graph_smooth(tile, off, nbr, smoother.weights, mask=mask if with_mask else None, sweeps=sweeps, fill=fill, out=out,
                                               out_mask=out_mask), args.repeats)
    times = {"keep": run(K, False, True), "fill": run(K, True, True), "no_mask": run(K, False, False), "one_sweep_keep": run(1, False, True)}
    per_sweep_us = 1e3 * (times["keep"]["median"] - times["one_sweep_keep"]["median"]) / max(K - 1, 1)
    # the two poles of the stand-in have degree 200, which no vertex of an atlas mesh has: the same sweeps with their two CSR rows emptied
    # (they stay neighbours of their rings) show what that serial tail costs
    hubless = off.clone()
    hubless[V - 2:] = off[V - 2]
    times["keep_poles_without_neighbours"] = _timed(lambda: ops.graph_smooth(tile, hubless, nbr, smoother.weights, mask=mask, sweeps=K, out=out,
                                                                             out_mask=out_mask), args.repeats)

    # the yardstick: the same operator with nothing missing, as a sparse matrix applied K times
    yardstick = None
    try:
        off_h, w_h = off.cpu().numpy().astype(np.int64), smoother.weights.cpu().numpy()
        owner = np.repeat(np.arange(V), np.diff(off_h))
        d = 1.0 + np.bincount(owner, w_h, minlength=V)
        order = np.lexsort((np.concatenate([nbr.cpu().numpy(), np.arange(V)]), np.concatenate([owner, np.arange(V)])))
        rows = np.concatenate([owner, np.arange(V)])[order]
        cols = np.concatenate([nbr.cpu().numpy(), np.arange(V)])[order]
        vals = (np.concatenate([w_h, np.ones(V)]) / d[np.concatenate([owner, np.arange(V)])])[order]
        crow = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=V))])
        A = torch.sparse_csr_tensor(torch.from_numpy(crow).cuda(), torch.from_numpy(cols.astype(np.int64)).cuda(), torch.from_numpy(vals).cuda(),
                                    size=(V, V), dtype=torch.float64)
        X = tile.t().contiguous()

        def power():
            Z = X
            for _ in range(K):
                Z = torch.sparse.mm(A, Z)
            return Z
        yardstick = _timed(power, args.repeats)
        full = ops.graph_smooth(tile, off, nbr, smoother.weights, sweeps=K)[0]
        agreement = float((power().t() - full).abs().max().item())
    except Exception as exc:                                               # the yardstick is not this library's code: say what it did
        yardstick, agreement = f"{type(exc).__name__}: {exc}", None
    floor_ms = [1e3 * K * ((2 * 8 + 2) * N * V / HBM_BYTES_PER_S + b * 1e-6) for b in BOUNDARY_US]
    print(json.dumps({"row": "kernel", "n_rows": N, "n_verts": V, "neighbour_slots": int(nbr.numel()), "fwhm_mm": args.fwhm, "sweeps": K,
                      "sigma_step_mm": round(smoother.sigma_step, 4), "achieved_fwhm_mm": round(smoother.achieved_fwhm_mm, 4),
                      "graph_smooth_ms": times, "per_sweep_us": round(per_sweep_us, 2),
                      "sparse_mm_K_times_ms": yardstick, "max_abs_difference_to_sparse_mm": agreement,
                      "floor_ms": [round(f, 3) for f in floor_ms],
                      "multiple_of_floor": [round(times["keep"]["median"] / f, 2) for f in floor_ms]}), flush=True)


def cohort(args):
    cohort = _cohort()
    smoothed = cohort.smoothed(fwhm_mm=args.fwhm)
    ms = _timed(lambda: cohort.smoothed(fwhm_mm=args.fwhm), args.rounds)
    print(json.dumps({"row": "cohort", "n_knees": len(cohort), "n_verts": cohort.n_verts, "fwhm_mm": args.fwhm, "sweeps": smoothed.smoothing.sweeps,
                      "achieved_fwhm_mm": round(smoothed.smoothing.achieved_fwhm_mm, 4), "smoothed_ms": ms,
                      "note": "includes building the smoother: one download of the graph and the host-side weights"}), flush=True)


def inference(args):
    import torch
    from oai_analysis_2_amd import mesh_processing as mp, stats
    from test_graph_tfce_gpu import _icosphere, _painted
    verts, faces = _icosphere()
    atlas = SimpleNamespace(inner={"FC": mp.Mesh(verts * np.float32(20.0), faces)}, device=torch.device("cuda", 0))
    Y, groups, cap = _painted(0.10)
    cohort = stats.ThicknessCohort(atlas, "FC")
    for row in Y:
        cohort.add_vector(row)
    rows = []
    for fwhm in (None,) + tuple(args.fwhms):
        c = cohort if fwhm is None else cohort.smoothed(fwhm_mm=fwhm)
        res = stats.two_sample_test(c, groups, n_permutations=args.permutations, seed=1, tfce=stats.TFCE(extent="vertices"))
        rows.append({"fwhm_mm": fwhm, "sweeps": None if fwhm is None else c.smoothing.sweeps,
                     "achieved_fwhm_mm": None if fwhm is None else round(c.smoothing.achieved_fwhm_mm, 3),
                     "cap_p_fwer": int((res.p_fwer[cap] <= 0.05).sum()), "cap_p_tfce": int((res.p_tfce[cap] <= 0.05).sum()),
                     "outside_p_fwer": int((res.p_fwer[~cap] <= 0.05).sum()), "outside_p_tfce": int((res.p_tfce[~cap] <= 0.05).sum())})
    print(json.dumps({"row": "inference", "cap_vertices": int(cap.sum()), "n_verts": len(cap), "n_knees": len(Y), "permutations": args.permutations,
                      "vertices_with_p_at_most_0.05": rows}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=("kernel", "cohort", "inference"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--fwhm", type=float, default=5.0)
    ap.add_argument("--fwhms", type=float, nargs=2, default=(6.0, 10.0))
    ap.add_argument("--permutations", type=int, default=2000)
    a = ap.parse_args()
    {"kernel": kernel, "cohort": cohort, "inference": inference}[a.row](a)
