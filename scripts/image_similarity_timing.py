#!/usr/bin/env python
"""Timings behind profiles/image_similarity.md.

    python scripts/image_similarity_timing.py kernels
        HIP-event time of each entry point of csrc/similarity.hip at 80x192x192 with sigma = 4 and 64 bins, steady state, beside what it
        moves; the joint histogram on uniform data and on a volume that is 95 % zeros (the run folding that was timed with an earlier form of
        this script is no longer in the library: profiles/image_similarity.md).
    python scripts/image_similarity_timing.py pipeline
        wall time per volume of VolumePipeline.run at bench.py's workload shape with qc=QCReference(..., surface=True) against the same
        with image= (and roi_mm=) added, the variants alternating round by round in one process.

Every run is one process and prints one JSON line; run each under a time limit of its own.
"""
import argparse
import json
import statistics
import time

VOL_SHAPE = (160, 384, 384)       # bench.py
NET_SHAPE = (80, 192, 192)


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
        rounds.append(1e3 * e0.elapsed_time(e1) / args.reps)                # microseconds per call (every kernel of the entry point)
    return {"us_per_call_median": statistics.median(rounds), "us_per_call_min": min(rounds), "us_per_call_max": max(rounds)}


def kernels(args):
    import numpy as np
    import torch
    from oai_analysis_2_amd import _lib, ops
    from oai_analysis_2_amd.synth import make_volume
    lib = _lib.load()
    D, H, W = NET_SHAPE
    n = D * H * W
    rng = np.random.default_rng(0)
    a = torch.from_numpy(make_volume(1, NET_SHAPE)).cuda()
    b = torch.from_numpy(make_volume(2, NET_SHAPE)).cuda()
    uniform = [torch.from_numpy(rng.uniform(0, 1, NET_SHAPE).astype(np.float32)).cuda() for _ in range(2)]
    sparse = [torch.from_numpy(np.where(rng.uniform(size=NET_SHAPE) < 0.95, 0.0, rng.uniform(0, 1, NET_SHAPE)).astype(np.float32)).cuda() for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    # the library calls alone, on buffers allocated once
    taps, radius = ops.gaussian_taps(4.0)
    import ctypes as C
    ctaps = (C.c_double * len(taps))(*taps.tolist())
    ws = torch.empty(int(lib.oai_lncc_workspace_bytes(D, H, W)), dtype=torch.uint8, device="cuda")
    wm = torch.empty(int(lib.oai_image_moments_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    st = torch.empty(8, dtype=torch.float64, device="cuda")
    hist = torch.empty(64 * 64 + 1, dtype=torch.int64, device="cuda")
    unit = (C.c_float * 2)(0.0, 1.0)

    def lncc():
        _lib.check(lib.oai_lncc(a.data_ptr(), b.data_ptr(), D, H, W, ctaps, radius, 1e-5, None, None, ws.data_ptr(), ws.numel(), st.data_ptr(), stream))

    def moments():
        _lib.check(lib.oai_image_moments(a.data_ptr(), b.data_ptr(), n, None, wm.data_ptr(), wm.numel(), st.data_ptr(), stream))

    def histogram(pair, bins=64):
        return lambda: _lib.check(lib.oai_joint_histogram(pair[0].data_ptr(), pair[1].data_ptr(), n, unit, unit, bins, None, hist.data_ptr(), stream))

    def entropies():
        _lib.check(lib.oai_histogram_entropies(hist.data_ptr(), 64, st.data_ptr(), stream))

    cases = {"lncc": (lncc, 8 * n + 4 * 40 * n), "image_moments": (moments, 8 * n), "histogram_entropies": (entropies, 8 * 4097)}
    res = {}
    for name, pair in (("uniform", uniform), ("95 % zeros", sparse), ("synthetic knee", (a, b))):
        cases[f"joint_histogram, {name}"] = (histogram(pair), 8 * n)
    for name, case in cases.items():
        t = _time_events(torch, case[0], args)
        t.update(compulsory_MB=case[1] / 1e6, TBps=case[1] / (t["us_per_call_median"] * 1e-6) / 1e12)
        res[name] = t
    res["lncc_stats"] = ops.lncc(a, b).cpu().tolist()
    print(json.dumps({"what": "kernels", "net": NET_SHAPE, "reps": args.reps, "rounds": args.rounds, "cases": res}), flush=True)


def pipeline(args):
    import numpy as np
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
    maps = [Image(m.cpu().numpy(), atlas.spacing) for m in (first.fc_atlas, first.tc_atlas)]
    variants = {"off": dict(), "surface": dict(qc=QCReference(*maps, surface=True)),
                "surface + image": dict(qc=QCReference(*maps, surface=True, image=atlas)),
                "surface + image + roi": dict(qc=QCReference(*maps, surface=True, image=atlas, roi_mm=5.0))}
    for kw in variants.values():
        for i in range(args.warmup):
            pipe.run(vols[i % 2], meta, check=False, **kw)
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    last = {}
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
            if res.qc is not None and res.qc.similarity is not None:
                last[name] = {k: {"lncc": r.lncc, "ncc": r.ncc, "nmi": r.nmi, "n": r.n} for k, r in res.qc.similarity.items()}
    print(json.dumps({"what": "pipeline", "steps": args.steps, "rounds": args.rounds,
                      "ms_per_volume": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v} for k, v in ms.items()},
                      "similarity": last}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "pipeline"])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    {"kernels": kernels, "pipeline": pipeline}[args.what](args)


if __name__ == "__main__":
    main()
