#!/usr/bin/env python
"""Timings behind profiles/surface_distance.md.

    python scripts/surface_distance_timing.py all [--root-parent TREE]
        every row below, each in a child process of its own under its own time limit; stops at the first row that fails.
    python scripts/surface_distance_timing.py edt --features surface|random|single
        HIP-event time of oai_edt at the atlas grid of bench.py's workload (160x384x384, OAI DESS spacing) for a cartilage-like
        surface, a 0.3 % random set and a single corner feature (every scan runs the length of its line: the worst case), beside its
        compulsory bytes (features read, distances written) and its workspace traffic.
    python scripts/surface_distance_timing.py surface_distance
        oai_surface_distance on two cartilage-like surfaces three voxels apart, with one percentile, and oai_mask_surface.
    python scripts/surface_distance_timing.py pipeline [--root TREE] [--variants no_qc,qc_reference,qc_surface]
        wall time per volume of VolumePipeline.run at bench.py's workload shape, the variants alternating round by round in one process.
        ``--root TREE --variants no_qc,qc_reference`` imports the package from another checkout (the parent commit).

Prints one JSON line per row.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

VOL_SHAPE = (160, 384, 384)       # bench.py
SPACING = (0.36458333, 0.36458333, 0.7)
ROW_LIMIT_S = 240


def _shell(np, shift):
    """A cartilage-like sheet five voxels thick on a sphere cap: float32 probabilities, 1 inside."""
    D, H, W = VOL_SHAPE
    z, y, x = np.ogrid[0:D, 0:H, 0:W]
    r = np.sqrt((x - shift - W / 2.0) ** 2 + ((z - D / 2.0) * 1.9) ** 2 + (y + 60.0) ** 2)
    return ((np.abs(r - 220.0) < 2.5) & (np.hypot(x - shift - W / 2.0, (z - D / 2.0) * 1.9) < 140.0)).astype(np.float32)


def _time_events(torch, fn, args, reps):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        rounds.append(1e3 * e0.elapsed_time(e1) / reps)                 # microseconds per call: every kernel of the entry point
    return {"us_per_call_median": statistics.median(rounds), "us_per_call_min": min(rounds), "us_per_call_max": max(rounds)}


def edt(args):
    import numpy as np
    import torch
    from oai_analysis_2_amd import _lib, ops
    lib = _lib.load()
    D, H, W = VOL_SHAPE
    n = D * H * W
    if args.features == "surface":
        feat = ops.mask_surface(torch.from_numpy(_shell(np, 0.0)).cuda(), 0.5, "surface")
    elif args.features == "random":
        feat = torch.from_numpy((np.random.default_rng(0).uniform(size=VOL_SHAPE) < 0.003).astype(np.uint8)).cuda()
    else:
        feat = torch.zeros(VOL_SHAPE, dtype=torch.uint8, device="cuda")
        feat[0, 0, 0] = 1
    dist = torch.empty(VOL_SHAPE, dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.oai_edt_workspace_bytes(D, H, W)), dtype=torch.uint8, device="cuda")
    import ctypes as C
    spacing = (C.c_double * 3)(*SPACING)
    stream = torch.cuda.current_stream().cuda_stream

    def call():                                                         # the library call alone: no allocation
        _lib.check(lib.oai_edt(feat.data_ptr(), D, H, W, spacing, 1.0, 0, dist.data_ptr(), None, ws.data_ptr(), ws.numel(), None, stream))
    t = _time_events(torch, call, args, args.reps)
    finite = dist[torch.isfinite(dist)]
    t.update(features=int(feat.sum()), compulsory_MB=5 * n / 1e6, workspace_traffic_MB=12 * n / 1e6, workspace_MB=ws.numel() / 1e6,
             max_distance=float(finite.max()), TBps_compulsory=5 * n / (t["us_per_call_median"] * 1e-6) / 1e12)
    print(json.dumps({"what": "edt", "features_kind": args.features, "shape": VOL_SHAPE, "spacing": SPACING, "reps": args.reps,
                      "rounds": args.rounds, **t}), flush=True)


def surface_distance(args):
    import numpy as np
    import torch
    from oai_analysis_2_amd import ops
    n = VOL_SHAPE[0] * VOL_SHAPE[1] * VOL_SHAPE[2]
    a, b = torch.from_numpy(_shell(np, 0.0)).cuda(), torch.from_numpy(_shell(np, 3.0)).cuda()
    sa, sb = ops.mask_surface(a, 0.5, "surface"), ops.mask_surface(b, 0.5, "surface")
    to_a, to_b = ops.distance_transform(sa, SPACING), ops.distance_transform(sb, SPACING)
    out = {}
    for name, fn, nbytes in (("mask_surface", lambda: ops.mask_surface(a, 0.5, "surface"), 5 * n),
                             ("surface_distance_one_percentile", lambda: ops.surface_distance(sa, to_b, sb, to_a, (95.0,)), 2 * n + 4 * 2 * n),
                             ("surface_distance_no_percentile", lambda: ops.surface_distance(sa, to_b, sb, to_a, ()), 2 * n)):
        t = _time_events(torch, fn, args, args.reps)
        t.update(compulsory_MB=nbytes / 1e6, TBps=nbytes / (t["us_per_call_median"] * 1e-6) / 1e12)
        out[name] = t
    print(json.dumps({"what": "surface_distance", "shape": VOL_SHAPE, "reps": args.reps, "rounds": args.rounds, "cases": out,
                      "figures": ops.surface_distance(sa, to_b, sb, to_a, (95.0,)).cpu().tolist()}), flush=True)


def pipeline(args):
    import torch
    from oai_analysis_2_amd.image import Image
    from oai_analysis_2_amd.pipeline import CROP_ZYX, OVERLAP_ZYX, TILE_ZYX, VolumePipeline
    from oai_analysis_2_amd.qc import QCReference
    from oai_analysis_2_amd.registration import IconEngine
    from oai_analysis_2_amd.segmentation.engine import UNetEngine
    from oai_analysis_2_amd.synth import make_icon_state_dict, make_unet_state_dict, make_volume
    unet = UNetEngine(make_unet_state_dict(0), precision="fp16x3")
    atlas = Image(make_volume(1000, VOL_SHAPE), [0.36, 0.36, 0.7], [0.0, 0.0, 0.0])
    pipe = VolumePipeline(unet, IconEngine(make_icon_state_dict(0, last_scale=0.1)), atlas)
    vols_np = [make_volume(i, VOL_SHAPE) for i in range(2)]
    vols = [torch.from_numpy(v).cuda() for v in vols_np]
    meta = Image(vols_np[0], [0.36, 0.36, 0.7], [2.0, -3.0, 1.0])
    unet.calibrate_volume(vols[0], TILE_ZYX, OVERLAP_ZYX, CROP_ZYX)
    first = pipe.run(vols[0], meta, check=False)
    fc, tc = first.fc_atlas.clone(), first.tc_atlas.clone()
    del first
    makers = {"no_qc": lambda: {}, "qc_reference": lambda: {"qc": QCReference(fc, tc)},
              "qc_surface": lambda: {"qc": QCReference(fc, tc, surface=True, spacing_xyz=atlas.spacing)}}
    variants = {name: makers[name]() for name in args.variants.split(",") if name}
    for kw in variants.values():
        for i in range(args.warmup):
            pipe.run(vols[i % 2], meta, check=False, **kw)
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    record = None
    for _ in range(args.rounds):                                            # the variants alternate round by round
        for name, kw in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = None
            for i in range(args.steps):
                del res
                res = pipe.run(vols[i % 2], meta, check=False, **kw)
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
            if name == "qc_surface":
                record = {k: vars(v) for k, v in res.qc.surface.items()}
    print(json.dumps({"what": "pipeline", "root": args.root or ".", "steps": args.steps, "rounds": args.rounds,
                      "ms_per_volume": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v} for k, v in ms.items()},
                      "last_surface_record": record}), flush=True)


def run_all(args):
    """Every row in a fresh child process under ROW_LIMIT_S; the first failure ends the run."""
    me = os.path.abspath(__file__)
    rows = [["edt", "--features", "surface"], ["edt", "--features", "random"], ["edt", "--features", "single", "--reps", "5"], ["surface_distance"]]
    if args.root_parent:
        rows.append(["pipeline", "--root", args.root_parent, "--variants", "no_qc,qc_reference"])
    rows.append(["pipeline"])
    if args.root_parent:
        rows.append(["pipeline", "--root", args.root_parent, "--variants", "no_qc,qc_reference"])
    for row in rows:
        try:
            rc = subprocess.run([sys.executable, me, *row], timeout=ROW_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps({"what": "failed", "row": row, "status": rc}), flush=True)
            sys.exit(rc if rc > 0 else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["all", "edt", "surface_distance", "pipeline"])
    ap.add_argument("--features", default="surface", choices=["surface", "random", "single"])
    ap.add_argument("--root", default=None, help="import oai_analysis_2_amd from this checkout instead of the one this script lies in")
    ap.add_argument("--root-parent", default=None, help="all: a checkout of the parent commit, built, for the pipeline comparison")
    ap.add_argument("--variants", default="no_qc,qc_reference,qc_surface")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    {"all": run_all, "edt": edt, "surface_distance": surface_distance, "pipeline": pipeline}[args.what](args)


if __name__ == "__main__":
    main()
