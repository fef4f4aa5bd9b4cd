#!/usr/bin/env python
"""Timings behind profiles/cohort_pca.md; prints one JSON line per row.

The input is SYNTHETIC: N knees on 30 002 vertices (seed 200) -- 2 mm, four smooth modes of 0.4 .. 0.1 mm, 0.1 mm of noise -- with 5 % of
the entries missing, and vertex weights drawn from 0.2 .. 1.8 mm^2.

    python scripts/cohort_pca_timing.py [--repeats 9] [--knees 200 2000] [--skip-svd]
        ops.cohort_whiten (with and without the squared norms), ops.rows_cross of the whitened cohort in its walk and its split form
        (the split form only where the entry point takes it: at most 256 tiles), ops.rows_combine for ten modes, and rows_cross of one
        new knee against ten modes: ms under device events, warm, the median of ``--repeats``; between repeats a 512 MiB buffer is
        overwritten so that no input is left in the L2 or the Infinity Cache.  The cross kernel as pair-vertices per second against the
        fp64 VALU issue rate at two instructions (a multiply, an add) per pair-vertex, counted over the 64 x 64 tiles it computes (the
        upper triangle).  Then the host: np.linalg.eigh of the Gram matrix, ThicknessPCA.fit and transform end to end (wall time), and
        beside them np.linalg.svd of the same whitened matrix on this machine's CPU with the threads the environment grants.
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
ISSUE_FP64 = 256 * 4 * 16 * 2.4e9                                          # fp64 VALU lane-operations per second: a wave64 operation holds its SIMD for four cycles
PER_PAIR = 2                                                               # v_mul_f64, v_add_f64
TILE = 64


def _spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def cohort_arrays(n_knees):
    rng = np.random.default_rng(200)
    t = np.linspace(0.0, 1.0, N_VERTS)
    shapes = np.stack([np.sin(np.pi * (k + 1) * t) for k in range(4)])
    Y = (2.0 + (rng.normal(size=(n_knees, 4)) * np.array([0.4, 0.3, 0.2, 0.1])) @ shapes + 0.1 * rng.normal(size=(n_knees, N_VERTS))).astype(np.float32)
    return Y, rng.random((n_knees, N_VERTS)) >= 0.05, rng.uniform(0.2, 1.8, size=N_VERTS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--knees", type=int, nargs="+", default=[200, 2000])
    ap.add_argument("--skip-svd", action="store_true")
    args = ap.parse_args()
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

        Y, mask, w = cohort_arrays(N)
        Yd, md = torch.from_numpy(Y).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev)
        prep = ops.group_prepare(Yd, md)
        mean, rw = prep.mean.clone(), torch.from_numpy(np.sqrt(w)).to(dev)
        del prep
        row("oai_cohort_whiten", timed(lambda: ops.cohort_whiten(Yd, md, mean, rw)), bytes_moved=N * N_VERTS * (4 + 1 + 8))
        row("oai_cohort_whiten, with norm2", timed(lambda: ops.cohort_whiten(Yd, md, mean, rw, return_norm2=True)))
        A = ops.cohort_whiten(Yd, md, mean, rw)
        tiles = -(-N // TILE)
        computed = tiles * (tiles + 1) // 2 * TILE * TILE * N_VERTS           # pair-vertices of the tiles on or above the diagonal
        for form, ws in (("walk", None), ("split", ops.rows_cross_workspace(N, N, N_VERTS, dev))):
            if form == "split" and ws is None:
                row("oai_rows_cross, split", None, note="more than 256 tiles: the entry point walks")
                continue
            ms = timed(lambda: ops.rows_cross(A, workspace=ws))
            per_s = computed / (ms["median"] * 1e-3)
            row(f"oai_rows_cross, {form}", ms, upper_tiles=tiles * (tiles + 1) // 2, workspace_mib=0 if ws is None else ws.numel() >> 20,
                pair_vertices_per_s=float(f"{per_s:.4g}"), fp64_issue_share=round(per_s * PER_PAIR / ISSUE_FP64, 4),
                useful_share=round(N * (N + 1) / 2 * N_VERTS / computed, 4))
        G = ops.rows_cross(A, workspace=ops.rows_cross_workspace(N, N, N_VERTS, dev)).cpu().numpy()
        t0 = time.perf_counter()
        lam, U = np.linalg.eigh(G)
        row("np.linalg.eigh of G (host)", round((time.perf_counter() - t0) * 1e3, 2))
        coef = torch.from_numpy(np.ascontiguousarray(U[:, ::-1][:, :10].T / np.sqrt(lam[::-1][:10])[:, None])).to(dev)
        row("oai_rows_combine, 10 modes", timed(lambda: ops.rows_combine(coef, A)), bytes_moved=3 * N * N_VERTS * 8)
        R = ops.rows_combine(coef, A)
        row("oai_rows_cross, one new knee against 10 modes, walk form", timed(lambda: ops.rows_cross(A[:1], R)))
        ws1 = ops.rows_cross_workspace(1, 10, N_VERTS, dev)
        row("oai_rows_cross, one new knee against 10 modes, split form", timed(lambda: ops.rows_cross(A[:1], R, workspace=ws1)))
        if not args.skip_svd:
            host = A.cpu().numpy()
            t0 = time.perf_counter()
            s = np.linalg.svd(host, full_matrices=False, compute_uv=True)[1]
            row("np.linalg.svd of the whitened matrix (host CPU)", round((time.perf_counter() - t0) * 1e3, 1),
                threads=os.environ.get("OMP_NUM_THREADS"), singular_value_error=float(np.abs(s[:10] - np.sqrt(lam[::-1][:10])).max() / s[0]))
            del host
        del A, R, G
        atlas = SimpleNamespace(inner={"FC": mp.Mesh(np.zeros((N_VERTS, 3), np.float32), np.zeros((0, 3), np.int32))}, device=dev)
        cohort = stats.ThicknessCohort(atlas, "FC", chunk=N)
        cohort._values, cohort._mask, cohort.ids = Yd * md, md, list(range(N))
        wall, eigh = [], []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model = cohort.pca(10, weights=w)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            eigh.append(model.eigh_seconds * 1e3)
        row("ThicknessCohort.pca(10), wall", _spread(wall[1:]), wall_first=round(wall[0], 2), of_which_eigh=_spread(eigh[1:]))
        one = Y[0].copy()
        wall = []
        for _ in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.transform(one)
            wall.append((time.perf_counter() - t0) * 1e3)
        row("ThicknessPCA.transform(one knee), wall", _spread(wall[1:]))
        del cohort, model, Yd, md


if __name__ == "__main__":
    main()
