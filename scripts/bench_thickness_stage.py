"""Timing of the per-knee thickness stage (oai_analysis_2_amd/thickness.py) on full-size maps; prints ONE JSON line.

    stage            ThicknessAtlas.measure, warm, ms per knee -- FC: scripts/bench_mesh.py's slab (160x384x384), TC: the bowl of
                     tests/test_mesh_graph_gpu.py -- beside the chain of public functions that existed before the stage
                     (get_thickness_mesh(on_device=True) -> map_attributes, atlas meshes prebuilt), alternated in this process
    raster           thickness_image_build once per atlas, thickness_image per knee
    cohort           volumes/s of CohortRunner(keep_on_device=True) drained alone against the same run with thickness_stream behind it.
                     Synthetic weights produce no cartilage, so THIS SCRIPT (not the library) puts the slab / bowl tensors in place of
                     fc_atlas / tc_atlas before thickness_stream; the runner is the one process_cohort builds, without the NIfTI reads
    per_knee_wall    normalise -> segment + register + resample -> thickness -> thickness images of one volume, host array to images
    patient          (--patient) ThicknessAtlas.measure(..., phi=, image_A=) -- both sub-meshes pushed through a smooth phi on the
                     80x192x192 network grid before the distance -- beside the atlas-space measure on the same maps, alternated in this
                     process, and the point transform alone (profiles/thickness_native.md)

    python scripts/bench_thickness_stage.py [--repeats 3] [--volumes 24] [--no-cohort] [--patient]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oai_analysis_2_amd import mesh_processing as mp, ops                     # noqa: E402
from oai_analysis_2_amd.image import Image                                    # noqa: E402
from oai_analysis_2_amd.thickness import ThicknessAtlas                       # noqa: E402

VOL_SHAPE = (160, 384, 384)
MIN_CELLS = {"FC": 3000, "TC": 100}
sig = lambda t: 1.0 / (1.0 + np.exp(np.clip(t, -60, 60)))


def slab(shift_x=0.0):
    D, H, W = VOL_SHAPE
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    x = x - shift_x
    R, T = 220.0, 5.0
    r = np.sqrt((x - 192) ** 2 + ((z - 80) * 1.9) ** 2 + (y + 60) ** 2)
    return Image((sig(2.0 * (np.abs(r - R) - T / 2)) * sig(2.0 * (np.sqrt((x - 192) ** 2 + ((z - 80) * 1.9) ** 2) - 140))).astype(np.float32),
                 [0.36, 0.36, 0.7])


def bowl(shift_x=0.0):
    D, H, W = 48, 96, 96
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    x = x - shift_x
    r = np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4 + (y + 30) ** 2)
    return Image((sig(2.0 * (np.abs(r - 60.0) - 3.0)) * sig(2.0 * (np.sqrt((x - 48) ** 2 + (z - 24) ** 2 * 4) - 30))).astype(np.float32), [1.0, 1.0, 1.0])


def ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t), out


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--volumes", type=int, default=24)
    ap.add_argument("--no-cohort", action="store_true", help="the stage and the raster only (no U-Net / ICON engines are built)")
    ap.add_argument("--patient", action="store_true", help="also time the patient-space measure against the atlas-space one (alternated)")
    args = ap.parse_args()
    reps = max(args.repeats, 3)
    knee = {"FC": slab(0.0), "TC": bowl(0.0)}
    maps = {k: torch.from_numpy(v.array).cuda() for k, v in knee.items()}
    t_atlas, atlas = ms(lambda: ThicknessAtlas(slab(1.5), bowl(1.5), min_cells=MIN_CELLS))
    out = {"what": "per-knee thickness stage, FC slab 160x384x384 + TC bowl 48x96x96", "atlas_build_ms_incl_map_generation": t_atlas,
           "atlas_points": {k: atlas.n_points(k) for k in ("FC", "TC")}, "image_shape": list(atlas.image_shape)}

    def chain():                                             # what a caller could do before the stage existed
        res = {}
        for kind in ("FC", "TC"):
            src, _ = mp.get_thickness_mesh(maps[kind], kind, min_cells=MIN_CELLS[kind], on_device=True, spacing_xyz=knee[kind].spacing)
            res[kind] = mp.map_attributes(src, atlas.inner[kind]).point_data["Distance"]
        return res

    stage = lambda: atlas.measure(maps["FC"], maps["TC"])
    k0, c0 = stage(), chain()                                # warm both
    same = all(np.array_equal(k0[k].view(np.int32), c0[k].view(np.int32)) for k in ("FC", "TC"))
    t_stage, t_chain = [], []
    for _ in range(reps):                                    # alternated in one process
        t_stage.append(ms(stage)[0])
        t_chain.append(ms(chain)[0])
    out["stage_ms_per_knee"] = spread(t_stage)
    out["parent_equivalent_chain_ms_per_knee"] = spread(t_chain)
    out["stage_equals_chain_bitwise"] = same
    out["median_thickness"] = {k: float(np.nanmedian(k0[k])) for k in ("FC", "TC")}

    if args.patient:
        net = (80, 192, 192)                                 # registration.NET_SHAPE
        grids = np.mgrid[0:net[0], 0:net[1], 0:net[2]].astype(np.float64)
        ident = np.stack([grids[d] * (1.0 / (net[d] - 1)) for d in range(3)]).astype(np.float32)
        phi = torch.from_numpy((ident + 0.01 * np.sin(2 * np.pi * ident[[1, 2, 0]])).astype(np.float32)).cuda()      # smooth, up to 1 % of each extent
        meta_A = Image(np.broadcast_to(np.zeros((), np.float32), VOL_SHAPE), [0.36, 0.36, 0.7], [2.0, -3.0, 1.0])
        patient = lambda: atlas.measure(maps["FC"], maps["TC"], phi=phi, image_A=meta_A)
        p0 = patient()                                       # warm
        n_pat = max(reps, 10)
        t_atl, t_pat = [], []
        for _ in range(n_pat):                               # alternated in one process
            t_atl.append(ms(stage)[0])
            t_pat.append(ms(patient)[0])
        diff = [b - a for a, b in zip(t_atl, t_pat)]
        verts = torch.from_numpy(atlas.inner["FC"].verts).cuda()
        legs = mp.mesh_point_affines(meta_A, Image(np.broadcast_to(np.zeros((), np.float32), VOL_SHAPE), knee["FC"].spacing), net)
        push = lambda: [mp._transform_points_dev(verts, phi, *legs, return_inside=True) for _ in range(100)]
        push()
        out["patient"] = {"atlas_space_ms_per_knee": spread(t_atl), "patient_space_ms_per_knee": spread(t_pat), "extra_ms_per_knee_paired": spread(diff),
                          "extra_share_of_stage": statistics.median(diff) / statistics.median(t_atl), "errors": p0.errors, "outside": p0.outside,
                          "median_thickness": {k: float(np.nanmedian(p0[k])) for k in ("FC", "TC")},
                          "transform_alone_ms_per_call": spread([ms(push)[0] / 100 for _ in range(5)]), "transform_points": int(verts.shape[0]),
                          "phi": "identity + 0.01 sin(2 pi u) per channel on 80x192x192", "image_A": "160x384x384, spacing 0.36 0.36 0.7"}

    uv, faces = atlas.uv["FC"], torch.from_numpy(atlas.inner["FC"].faces).cuda()
    mp.thickness_image_build(uv, faces, None, atlas.image_shape)
    out["raster_build_ms_fc"] = spread([ms(lambda: mp.thickness_image_build(uv, faces, None, atlas.image_shape))[0] for _ in range(reps)])
    out["raster_covered_fraction_fc"] = atlas.raster["FC"].n_covered / float(atlas.image_shape[0] * atlas.image_shape[1])
    fc_dev = torch.from_numpy(k0.fc).cuda()
    atlas.image(fc_dev, "FC")
    out["raster_apply_ms_per_knee_fc"] = spread([ms(lambda: atlas.image(fc_dev, "FC"))[0] for _ in range(max(reps, 10))])

    if not args.no_cohort:
        from oai_analysis_2_amd.cohort import CohortRunner
        from oai_analysis_2_amd.dask_processing import thickness_stream
        from oai_analysis_2_amd.pipeline import CROP_ZYX, OVERLAP_ZYX, TILE_ZYX, VolumePipeline
        from oai_analysis_2_amd.registration import IconEngine
        from oai_analysis_2_amd.segmentation.engine import UNetEngine
        from oai_analysis_2_amd.synth import make_icon_state_dict, make_unet_state_dict, make_volume
        unet = UNetEngine(make_unet_state_dict(0), precision="fp16x3")
        pipe = VolumePipeline(unet, IconEngine(make_icon_state_dict(0, last_scale=0.1)), Image(make_volume(1000, VOL_SHAPE), [0.36, 0.36, 0.7], [0.0, 0.0, 0.0]))
        base = [make_volume(i, VOL_SHAPE) for i in range(4)]
        unet.calibrate_volume(torch.from_numpy(base[0]).cuda(), TILE_ZYX, OVERLAP_ZYX, CROP_ZYX)
        imgs = [Image(base[i % 4], [0.36, 0.36, 0.7], [2.0, -3.0, 1.0]) for i in range(args.volumes)]

        def swapped(it):                                     # the script's substitution: cartilage-like maps in place of the synthetic network's
            for i, r in it:
                yield i, dataclasses.replace(r, fc_atlas=maps["FC"], tc_atlas=maps["TC"])

        def drain(with_thickness):
            runner = CohortRunner(pipe, keep_on_device=True)
            src = runner.run(imgs)
            if with_thickness:
                src = thickness_stream(swapped(src), atlas, results_complete=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stamps, n_err = [], 0
            for _, r in src:
                stamps.append(time.perf_counter() - t0)
                n_err += len(r.errors) if with_thickness else 0
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            runner.close()
            gaps = [1e3 * (b - a) for a, b in zip([0.0] + stamps, stamps)]
            # steady state = the MEDIAN interval between results away from the fill and the drain (behind thickness_stream the last
            # results come in quick succession once the runner has drained: a mean over a fixed window would count those)
            return {"volumes_per_s": len(stamps) / dt, "total_ms": 1e3 * dt, "steady_ms_per_volume": statistics.median(gaps[3:-3]) if len(gaps) > 8 else None,
                    "errors": n_err, "result_intervals_ms": [round(g, 1) for g in gaps]}

        drain(False), drain(True)                            # warm: pinned buffers, allocator, worker threads
        rows = {"without": [], "with_thickness": []}
        for _ in range(reps):
            rows["without"].append(drain(False))
            rows["with_thickness"].append(drain(True))
        coh = {}
        for name, rr in rows.items():
            coh[name] = {"volumes_per_s": spread([r["volumes_per_s"] for r in rr]),
                         "steady_ms_per_volume": spread([r["steady_ms_per_volume"] for r in rr]) if rr[0]["steady_ms_per_volume"] else None,
                         "steady_ms_per_volume_by_run": [round(r["steady_ms_per_volume"], 2) if r["steady_ms_per_volume"] else None for r in rr],
                         "total_ms": spread([r["total_ms"] for r in rr]), "errors": sum(r["errors"] for r in rr),
                         "result_intervals_ms_last_run": rr[-1]["result_intervals_ms"]}
        p0, p1 = coh["without"]["steady_ms_per_volume"], coh["with_thickness"]["steady_ms_per_volume"]
        if p0 and p1:
            st = out["stage_ms_per_knee"]["median"]
            # the cost of the stage per volume from the TOTALS (fill and drain included: the last knee's stage has nothing to hide under)
            extra = (coh["with_thickness"]["total_ms"]["median"] - coh["without"]["total_ms"]["median"]) / args.volumes
            coh["period_ms"] = {"without": p0["median"], "with_thickness": p1["median"], "without_plus_stage_alone": p0["median"] + st,
                                "extra_ms_per_volume_from_totals": extra, "hidden_share_of_stage_from_totals": 1.0 - extra / st}
        coh["volumes"] = args.volumes
        out["cohort"] = coh

        # one knee, host array to thickness images
        raw = base[1] * 900.0 + 17.0
        meta = Image(raw, [0.36, 0.36, 0.7], [2.0, -3.0, 1.0])

        def one_knee():
            v = ops.image_normalize(torch.from_numpy(raw).cuda(), 0.1, 99.9, 0, 1)
            res = pipe.run(v, meta)
            th = atlas.measure(maps["FC"], maps["TC"], keep_on_device=True)          # (the cartilage-like maps: see `cohort` above)
            return res, {k: atlas.image(th[k], k).cpu() for k in ("FC", "TC") if k not in atlas.projection_errors}   # (the bowl lies on one side of z = 50: no TC projection)
        one_knee()
        out["per_knee_wall_s"] = spread([ms(one_knee)[0] / 1e3 for _ in range(reps)])
        out["per_knee_wall_note"] = ("host array -> normalise -> segment + register + both maps on the atlas -> thickness on the atlas vertices -> thickness image, "
                                     "weights resident; the reference's per-patient figure is 148 s (2 min 28 s), which includes its model downloads")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
