#!/usr/bin/env python
"""Timings behind profiles/registration_qc.md.

    python scripts/registration_qc_timing.py kernels
        HIP-event time of oai_phi_jacobian at 80x192x192 (with and without the map) and of oai_mask_overlap at 384*384*160 elements,
        steady state, beside their compulsory bytes.
    python scripts/registration_qc_timing.py pipeline [--root TREE] [--qc none|both]
        wall time per volume of VolumePipeline.run at bench.py's workload shape.  ``--qc both`` alternates rounds without QC and
        with ``qc=QCReference`` in one process; ``--root TREE --qc none`` imports the package from another checkout (the parent commit,
        which has no ``qc`` argument) for the comparison on the same box in the same session.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

HBM_ACHIEVABLE_TBPS = 6.29        # MI355X_MICROARCH.md: float4 copy, measured
VOL_SHAPE = (160, 384, 384)       # bench.py
NET_SHAPE = (80, 192, 192)


def kernels(args):
    import numpy as np
    import torch
    from oai_analysis_2_amd import ops
    rng = np.random.default_rng(0)
    D, H, W = NET_SHAPE
    zz, yy, xx = np.meshgrid(np.arange(D) / (D - 1), np.arange(H) / (H - 1), np.arange(W) / (W - 1), indexing="ij")
    scale = np.array([D - 1, H - 1, W - 1], np.float64)[:, None, None, None]
    phi = torch.from_numpy((np.stack([zz, yy, xx]) + rng.uniform(-0.45, 0.45, size=(3, D, H, W)) / scale).astype(np.float32)).cuda()
    n = VOL_SHAPE[0] * VOL_SHAPE[1] * VOL_SHAPE[2]
    a = torch.from_numpy(rng.uniform(0, 1, size=n).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.uniform(0, 1, size=n).astype(np.float32)).cuda()
    cells = (D - 1) * (H - 1) * (W - 1)
    cases = {
        "phi_jacobian": (lambda: ops.phi_jacobian(phi), 4 * phi.numel()),
        "phi_jacobian+map": (lambda: ops.phi_jacobian(phi, return_map=True), 4 * phi.numel() + 4 * cells),
        "mask_overlap": (lambda: ops.mask_overlap(a, b), 8 * n),
        "mask_overlap(one map)": (lambda: ops.mask_overlap(a), 4 * n),
    }
    out = {}
    for name, (fn, nbytes) in cases.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            rounds.append(1e3 * e0.elapsed_time(e1) / args.reps)            # microseconds per call (both kernels of the entry point + the allocations)
        us = statistics.median(rounds)
        out[name] = {"us_per_call_median": us, "us_per_call_min": min(rounds), "us_per_call_max": max(rounds), "compulsory_MB": nbytes / 1e6,
                     "TBps": nbytes / (us * 1e-6) / 1e12, "frac_of_achievable_hbm": nbytes / (us * 1e-6) / 1e12 / HBM_ACHIEVABLE_TBPS}
    print(json.dumps({"what": "kernels", "reps": args.reps, "rounds": args.rounds, "hbm_achievable_TBps": HBM_ACHIEVABLE_TBPS, "cases": out}), flush=True)


def pipeline(args):
    import torch
    from oai_analysis_2_amd.image import Image
    from oai_analysis_2_amd.pipeline import CROP_ZYX, OVERLAP_ZYX, TILE_ZYX, VolumePipeline
    from oai_analysis_2_amd.registration import IconEngine
    from oai_analysis_2_amd.segmentation.engine import UNetEngine
    from oai_analysis_2_amd.synth import make_icon_state_dict, make_unet_state_dict, make_volume
    unet = UNetEngine(make_unet_state_dict(0), precision="fp16x3")
    pipe = VolumePipeline(unet, IconEngine(make_icon_state_dict(0, last_scale=0.1)), Image(make_volume(1000, VOL_SHAPE), [0.36, 0.36, 0.7], [0.0, 0.0, 0.0]))
    vols_np = [make_volume(i, VOL_SHAPE) for i in range(2)]
    vols = [torch.from_numpy(v).cuda() for v in vols_np]
    meta = Image(vols_np[0], [0.36, 0.36, 0.7], [2.0, -3.0, 1.0])
    unet.calibrate_volume(vols[0], TILE_ZYX, OVERLAP_ZYX, CROP_ZYX)
    variants = {"no_qc": {}}
    first = pipe.run(vols[0], meta, check=False)
    if args.qc == "both":
        from oai_analysis_2_amd.qc import QCReference
        variants["qc_reference"] = {"qc": QCReference(first.fc_atlas.clone(), first.tc_atlas.clone())}
    del first
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
            if kw:
                q = res.qc
                record = {"folds": q.jacobian.folds, "cells": q.jacobian.cells, "det_min": q.jacobian.det_min, "det_max": q.jacobian.det_max,
                          "det_mean": q.jacobian.det_mean, "volume_scale": q.volume_scale, "dice": q.dice, "cartilage_mm3": q.cartilage_mm3}
    print(json.dumps({"what": "pipeline", "root": args.root or ".", "steps": args.steps, "rounds": args.rounds,
                      "ms_per_volume": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v} for k, v in ms.items()},
                      "last_record": record}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "pipeline"])
    ap.add_argument("--root", default=None, help="import oai_analysis_2_amd from this checkout instead of the one this script lies in")
    ap.add_argument("--qc", default="both", choices=["none", "both"])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    (kernels if args.what == "kernels" else pipeline)(args)


if __name__ == "__main__":
    main()
