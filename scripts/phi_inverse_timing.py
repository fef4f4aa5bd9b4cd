#!/usr/bin/env python
"""Timings behind profiles/phi_inverse.md.

    python scripts/phi_inverse_timing.py kernels
        HIP-event time of oai_invert_phi at 80x192x192 and of oai_inverse_points_through_phi at 65 000 points on a smooth field, steady
        state, beside their compulsory bytes, beside oai_transform_points_through_phi and oai_phi_jacobian on the same field, and the
        solver's iteration statistics.
    python scripts/phi_inverse_timing.py stage
        wall time of ThicknessAtlas.measure on stand-in cartilage maps in the three spaces ("atlas", "patient", "patient_grid").
    python scripts/phi_inverse_timing.py pipeline [--root TREE] [--spaces off,patient,patient_grid]
        wall time per volume of VolumePipeline.run at bench.py's workload shape, the variants alternating round by round in one process.
        ``--root TREE --spaces off`` imports the package from another checkout (the parent commit, which has no "patient_grid") for the
        comparison on the same box in the same session.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

VOL_SHAPE = (160, 384, 384)       # bench.py
NET_SHAPE = (80, 192, 192)
N_POINTS = 65000


def _smooth_phi(np, shape, amp_voxels):
    """identity + a product of half sines (zero on the boundary lattice) times a slow cosine, ``amp_voxels`` per (x, y, z) component"""
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D) / (D - 1.0), np.arange(H) / (H - 1.0), np.arange(W) / (W - 1.0), indexing="ij")
    bump = np.sin(np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z)
    ident = [(np.arange(n) * (1.0 / (n - 1))).astype(np.float32).astype(np.float64) for n in shape]
    phi = np.stack(np.meshgrid(*ident, indexing="ij"))
    for c, n in enumerate((W, H, D)):
        phi[2 - c] += amp_voxels[c] / (n - 1.0) * bump * np.cos(0.4 + 2.0 * x - 1.5 * y + 1.0 * z + 0.3 * c)
    return phi.astype(np.float32)


def _time_events(torch, fn, args):
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
        rounds.append(1e3 * e0.elapsed_time(e1) / args.reps)                # microseconds per call (every kernel of the entry point + the allocations)
    return {"us_per_call_median": statistics.median(rounds), "us_per_call_min": min(rounds), "us_per_call_max": max(rounds)}


def kernels(args):
    import numpy as np
    import torch
    from oai_analysis_2_amd import _lib, ops
    lib = _lib.load()
    D, H, W = NET_SHAPE
    out = {}
    for field, amp in (("smooth, 6/6/3 voxels", (6.0, 6.0, 3.0)), ("identity", (0.0, 0.0, 0.0))):
        phi = torch.from_numpy(_smooth_phi(np, NET_SHAPE, amp)).cuda()
        rng = np.random.default_rng(0)
        pts = torch.from_numpy(rng.uniform([0, 0, 0], [W - 1, H - 1, D - 1], size=(N_POINTS, 3)).astype(np.float32)).cuda()
        eye = (np.eye(3), np.zeros(3))
        psi, stats = ops.invert_phi(phi)
        # the dense entry point without ops.invert_phi's read-back of the stats (one synchronisation): the library call alone
        ws = torch.empty(int(lib.oai_invert_phi_workspace_bytes(D, H, W)), dtype=torch.uint8, device="cuda")
        st = torch.empty(6, dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def dense():
            _lib.check(lib.oai_invert_phi(phi.data_ptr(), D, H, W, 30, 1e-7, psi.data_ptr(), None, ws.data_ptr(), ws.numel(), st.data_ptr(), stream))
        cases = {
            "invert_phi": (dense, 2 * 4 * phi.numel()),                                       # phi read once, psi written once
            "inverse_points": (lambda: ops.inverse_points_through_phi(pts, phi, eye, eye), 24 * N_POINTS),
            "transform_points": (lambda: ops.transform_points_through_phi(pts, phi, eye, eye), 24 * N_POINTS),
            "phi_jacobian": (lambda: ops.phi_jacobian(phi), 4 * phi.numel()),
        }
        res = {}
        for name, (fn, nbytes) in cases.items():
            t = _time_events(torch, fn, args)
            t.update(compulsory_MB=nbytes / 1e6, TBps=nbytes / (t["us_per_call_median"] * 1e-6) / 1e12)
            res[name] = t
        _, status = ops.inverse_points_through_phi(pts, phi, eye, eye, return_status=True)
        res["dense_stats"] = stats.__dict__
        res["points_status_counts"] = np.bincount(status.cpu().numpy(), minlength=3).tolist()
        res["psi_folds"] = float(ops.phi_jacobian(psi).cpu()[1])
        out[field] = res
    print(json.dumps({"what": "kernels", "net": NET_SHAPE, "points": N_POINTS, "reps": args.reps, "rounds": args.rounds, "fields": out}), flush=True)


def _standins(np):
    """the femoral slab and the tibial bowl of tests/test_thickness_stage_gpu.py"""
    from oai_analysis_2_amd.image import Image
    sig = lambda t: 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))

    def slab(shift):
        z, y, x = np.mgrid[0:80, 0:192, 0:192].astype(np.float32)
        x = x - shift
        r = np.sqrt((x - 96) ** 2 + ((z - 40) * 1.9) ** 2 + (y + 30) ** 2)
        return Image((sig(2.0 * (np.abs(r - 110.0) - 2.5)) * sig(2.0 * (np.sqrt((x - 96) ** 2 + ((z - 40) * 1.9) ** 2) - 70))).astype(np.float32), [0.36, 0.36, 0.7])

    def bowl(shift):
        z, y, x = np.mgrid[0:48, 0:96, 0:96].astype(np.float32)
        x = x - shift
        r = np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4 + (y + 30) ** 2)
        return Image((sig(2.0 * (np.abs(r - 60.0) - 3.0)) * sig(2.0 * (np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4) - 30))).astype(np.float32), [1.0, 1.0, 1.0])
    return slab, bowl


def stage(args):
    import numpy as np
    import torch
    from oai_analysis_2_amd.image import Image
    from oai_analysis_2_amd.thickness import ThicknessAtlas
    slab, bowl = _standins(np)
    out = {}
    atlas = ThicknessAtlas(slab(1.5), bowl(1.5), image_shape=(96, 128), min_cells={"FC": 3000, "TC": 100})
    for kind, make in (("FC", slab), ("TC", bowl)):                                  # one cartilage at a time: each map has its own grid
        knee = make(0.0)
        vol = torch.from_numpy(knee.array).cuda()
        empty = torch.zeros((8, 8, 8), device="cuda")
        maps = (vol, empty) if kind == "FC" else (empty, vol)
        shape = tuple(vol.shape)
        net = (20, 48, 48)
        phi = torch.from_numpy(_smooth_phi(np, net, (1.5, 1.5, 0.75))).cuda()
        meta = Image(np.broadcast_to(np.zeros((), np.float32), shape), knee.spacing, [0.0, 0.0, 0.0], np.eye(3))
        variants = {"atlas": {}, "patient": dict(phi=phi, image_A=meta), "patient_grid": dict(phi=phi, image_A=meta, space="patient_grid")}
        ms = {name: [] for name in variants}
        last = {}
        for name, kw in variants.items():
            atlas.measure(*maps, **kw)
        for _ in range(args.rounds):
            for name, kw in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[name] = atlas.measure(*maps, **kw)
                ms[name].append(1e3 * (time.perf_counter() - t0))
        out[kind] = {name: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "median_thickness": float(np.nanmedian(last[name][kind])),
                            "errors": last[name].errors, "outside": last[name].outside, "unconverged": getattr(last[name], "unconverged", None)}
                     for name, v in ms.items()}
    print(json.dumps({"what": "stage", "rounds": args.rounds, "cartilage": out}), flush=True)


def pipeline(args):
    import numpy as np
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
    spaces = [s for s in args.spaces.split(",") if s]
    variants = {}
    if [s for s in spaces if s != "off"]:
        from oai_analysis_2_amd.thickness import ThicknessAtlas
        slab, bowl = _standins(np)
        atlas = ThicknessAtlas(slab(1.5), bowl(1.5), image_shape=(96, 128), min_cells={"FC": 3000, "TC": 100})
    for s in spaces:
        variants[s] = {} if s == "off" else dict(thickness=atlas, thickness_space=s)
    for kw in variants.values():
        for i in range(args.warmup):
            pipe.run(vols[i % 2], meta, check=False, **kw)
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    errors = {}
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
                errors[name] = res.thickness.errors
    print(json.dumps({"what": "pipeline", "root": args.root or ".", "steps": args.steps, "rounds": args.rounds,
                      "ms_per_volume": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v} for k, v in ms.items()},
                      "thickness_errors": errors}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "stage", "pipeline"])
    ap.add_argument("--root", default=None, help="import oai_analysis_2_amd from this checkout instead of the one this script lies in")
    ap.add_argument("--spaces", default="off,patient,patient_grid")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    {"kernels": kernels, "stage": stage, "pipeline": pipeline}[args.what](args)


if __name__ == "__main__":
    main()
