#!/usr/bin/env python
"""Timings behind profiles/mesh_quality.md; prints one JSON line per row.

    python scripts/mesh_quality_timing.py measure [--root TREE] [--rounds 7]
        ms per knee of ThicknessAtlas.measure on the synthetic knee of scripts/morphometry_timing.py (FC: the 160x384x384 slab of
        scripts/bench_thickness_stage.py, TC: its bowl) -- host clock around a synchronised call, warm.  In this checkout measure() and
        measure(mesh_qc=True) alternate round by round in one process, and the knee's record is printed; ``--root TREE`` imports the
        package from another checkout (the parent commit, which has no ``mesh_qc`` argument) and times its measure() alone.
    python scripts/mesh_quality_timing.py kernels [--rounds 7]
        HIP-event time of the three entry points on that knee's FC mesh (the whole mesh with its side vector); under
        ``rocprofv3 --kernel-trace --stats`` the per-kernel times.
"""
import argparse
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from morphometry_timing import MIN_CELLS, ROOT, _setup, _spread  # noqa: E402


def measure(args):
    np, torch, atlas, knee = _setup(args.root or ROOT)

    def ms(**kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = atlas.measure(*knee, **kw)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), out

    variants = {"measure": {}} if args.root else {"measure": {}, "measure_mesh_qc": {"mesh_qc": True}}
    for kw in variants.values():
        ms(**kw)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, kw in variants.items():
            t, out = ms(**kw)
            times[name].append(t)
    row = {"row": "measure", "tree": args.root or ROOT, "atlas_points": {k: atlas.n_points(k) for k in ("FC", "TC")},
           "ms_per_knee": {name: _spread(v) for name, v in times.items()}}
    if not args.root:
        row["record"] = {k: dataclasses.asdict(v) for k, v in out.mesh_qc.items()}
    print(json.dumps(row), flush=True)


def kernels(args):
    np, torch, atlas, knee = _setup(ROOT)
    from oai_analysis_2_amd import mesh_processing as mp

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
            rounds.append(1e3 * e0.elapsed_time(e1) / 3)         # microseconds per call: every launch of the entry point, workspace allocation included
        return _spread(rounds)

    sp = mp._resident_split(knee[0], atlas.spacing["FC"], "FC", MIN_CELLS["FC"])
    v, f, side = sp.verts, sp.faces, sp.side
    cls, _ = mp._mesh_topology_dev(f, int(v.shape[0]), side)
    row = {"row": "kernels", "n_verts": int(v.shape[0]), "n_faces": int(f.shape[0]), "us_per_call": {
        "oai_mesh_topology": events(lambda: mp._mesh_topology_dev(f, int(v.shape[0]), side)),
        "oai_mesh_geometry": events(lambda: mp._mesh_geometry_dev(v, f, cls)),
        "oai_mesh_self_intersections (grid parameters and their download included)": events(lambda: mp._mesh_self_intersections_dev(v, f))}}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=("measure", "kernels"))
    ap.add_argument("--root", default=None, help="measure: import the package from this checkout instead (the parent commit)")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    {"measure": measure, "kernels": kernels}[a.row](a)
