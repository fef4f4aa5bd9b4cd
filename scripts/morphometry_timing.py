#!/usr/bin/env python
"""Timings behind profiles/morphometry.md; prints one JSON line per row.

    python scripts/morphometry_timing.py measure [--root TREE] [--rounds 7]
        ms per knee of ThicknessAtlas.measure on one synthetic knee -- FC: scripts/bench_thickness_stage.py's slab (160x384x384), TC: its
        bowl -- host clock around a synchronised call, warm.  In this checkout measure() and measure(morphometry=True) alternate round by
        round in one process; ``--root TREE`` imports the package from another checkout (the parent commit, which has no ``morphometry``
        argument) and times its measure() alone.
    python scripts/morphometry_timing.py kernels [--rounds 7]
        HIP-event time of the three primitives at that knee's sizes: oai_mesh_areas on the atlas FC inner mesh, oai_point_footprint_grid
        of the knee's inner vertices against the atlas', oai_region_stats over the atlas vertices with 1 and with 8 regions.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOL_SHAPE = (160, 384, 384)
MIN_CELLS = {"FC": 3000, "TC": 100}


def _maps(np, Image):
    sig = lambda t: 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))

    def slab(shift_x):
        D, H, W = VOL_SHAPE
        z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
        x = x - shift_x
        r = np.sqrt((x - 192) ** 2 + ((z - 80) * 1.9) ** 2 + (y + 60) ** 2)
        return Image((sig(2.0 * (np.abs(r - 220.0) - 2.5)) * sig(2.0 * (np.sqrt((x - 192) ** 2 + ((z - 80) * 1.9) ** 2) - 140))).astype(np.float32),
                     [0.36, 0.36, 0.7])

    def bowl(shift_x):
        D, H, W = 48, 96, 96
        z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
        x = x - shift_x
        r = np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4 + (y + 30) ** 2)
        return Image((sig(2.0 * (np.abs(r - 60.0) - 3.0)) * sig(2.0 * (np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4) - 30))).astype(np.float32), [1.0, 1.0, 1.0])

    return slab, bowl


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def _setup(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from oai_analysis_2_amd.image import Image
    from oai_analysis_2_amd.thickness import ThicknessAtlas
    slab, bowl = _maps(np, Image)
    atlas = ThicknessAtlas(slab(1.5), bowl(1.5), min_cells=MIN_CELLS)
    knee = tuple(torch.from_numpy(m.array).cuda() for m in (slab(0.0), bowl(0.0)))
    return np, torch, atlas, knee


def measure(args):
    np, torch, atlas, knee = _setup(args.root or ROOT)

    def ms(**kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = atlas.measure(*knee, **kw)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), out

    variants = {"measure": {}} if args.root else {"measure": {}, "measure_morphometry": {"morphometry": True}}
    for kw in variants.values():                                  # warm: workspaces, the lazily computed atlas areas
        ms(**kw)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, kw in variants.items():
            t, out = ms(**kw)
            times[name].append(t)
    row = {"row": "measure", "tree": args.root or ROOT, "atlas_points": {k: atlas.n_points(k) for k in ("FC", "TC")},
           "ms_per_knee": {name: _spread(v) for name, v in times.items()}}
    if not args.root:
        rec = out.morphometry
        row["record"] = {k: {"area_mm2": rec[k].all.area_mm2, "denuded_mm2": rec[k].all.denuded_mm2, "mean_thickness_covered": rec[k].all.mean_thickness_covered,
                             "vertex_mean": rec[k].all.vertex_mean} for k in rec}
    print(json.dumps(row), flush=True)


def kernels(args):
    np, torch, atlas, knee = _setup(ROOT)
    from oai_analysis_2_amd import mesh_processing as mp, ops

    def events(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                fn()
            e1.record()
            torch.cuda.synchronize()
            rounds.append(1e3 * e0.elapsed_time(e1) / 3)         # microseconds per call, every launch of the entry point (workspace allocation included)
        return _spread(rounds)

    verts = atlas._targets["FC"]
    faces = mp._dev(atlas.inner["FC"].faces, np.int32, (3,), device=verts.device)
    iv, if_, dist = mp._thickness_inner_dev(knee[0], atlas.spacing["FC"], "FC", MIN_CELLS["FC"])
    lo, hi, _ = mp.mesh_grid_params_device(iv, if_)
    vec = mp._map_attributes_dev(iv, dist.reshape(1, -1), verts, atlas.radius, grid=(lo, hi))[0]
    area = mp._mesh_areas_dev(verts, faces)
    labels = (torch.arange(verts.shape[0], device=verts.device) % 8).to(torch.int32)
    row = {"row": "kernels", "n_verts": int(verts.shape[0]), "n_faces": int(faces.shape[0]), "n_src": int(iv.shape[0]), "us_per_call": {
        "oai_mesh_areas": events(lambda: mp._mesh_areas_dev(verts, faces)),
        "oai_point_footprint_grid": events(lambda: mp._point_footprint_dev(iv, verts, atlas.radius, grid=(lo, hi))),
        "oai_map_attributes_grid (context)": events(lambda: mp._map_attributes_dev(iv, dist.reshape(1, -1), verts, atlas.radius, grid=(lo, hi))),
        "oai_region_stats R=1": events(lambda: ops.region_stats(vec, area)),
        "oai_region_stats R=8": events(lambda: ops.region_stats(vec, area, labels, None, 8))}}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=("measure", "kernels"))
    ap.add_argument("--root", default=None, help="measure: import the package from this checkout instead (the parent commit)")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    {"measure": measure, "kernels": kernels}[a.row](a)
