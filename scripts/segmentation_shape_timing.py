"""The measurement behind profiles/segmentation_shape.md, at the workload's 160 x 384 x 384: one oai_label_components per connectivity (the
set and its complement), qc.segmentation_shape for both cartilages, scipy.ndimage.label on the host as the yardstick and, with --pipeline,
VolumePipeline.run with and without seg_qc.  Needs a GPU.  Usage: python scripts/segmentation_shape_timing.py [--pipeline] [--out DIR]"""
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import edt_ref as er
from oai_analysis_2_amd import ops, qc

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "."
os.makedirs(OUT, exist_ok=True)
res = {}


def cartilage_like(seed):
    low = er.blobs((40, 96, 96), seed=seed).astype(np.float32)
    v = np.repeat(np.repeat(np.repeat(low, 4, 0), 4, 1), 4, 2)
    thr = np.quantile(low, 0.985)
    m = np.where(v > thr, np.float32(0.9), np.float32(0.05))
    rng = np.random.default_rng(seed)
    m[rng.uniform(size=m.shape) < 2e-5] = np.float32(0.8)           # noise islands
    return np.ascontiguousarray(m)


def timed(fn, warm=3, reps=10, inner=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()))


maps = {k: cartilage_like(s) for k, s in (("FC", 1), ("TC", 2))}
dev = {k: torch.from_numpy(v).cuda() for k, v in maps.items()}
frac = {k: float((v > 0.5).mean()) for k, v in maps.items()}
res["set_fraction"] = frac
for c in (6, 18, 26):
    s = ops.label_components(dev["FC"], connectivity=c)[0].cpu().numpy().tolist()
    res[f"summary_{c}"] = s
    res[f"label_set_{c}"] = timed(lambda: ops.label_components(dev["FC"], connectivity=c, return_labels=True))
    res[f"label_set_summary_only_{c}"] = timed(lambda: ops.label_components(dev["FC"], connectivity=c, return_labels=False))
    res[f"label_complement_{c}"] = timed(lambda: ops.label_components(dev["FC"], connectivity=c, complement=True, return_labels=False))
    print(c, res[f"label_set_{c}"], res[f"label_complement_{c}"], flush=True)


def both():
    views, _ = qc._result_slots(dev["FC"].device, [slot for k in ("FC", "TC") for slot in qc._shape_layout(k)])
    for k in ("FC", "TC"):
        qc._queue_shape(dev[k], 0.5, 26, 0, (0.1, 0.9), views, k)
    return views


res["segmentation_shape_both_queued"] = timed(both)
t = []
for _ in range(8):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = qc.segmentation_shapes(dev)
    t.append((time.perf_counter() - t0) * 1e3)
res["segmentation_shape_both_host_ms"] = dict(median_ms=float(np.median(t[2:])), min_ms=float(min(t[2:])), max_ms=float(max(t[2:])))
res["record_FC"] = {k: (v if not isinstance(v, float) or v == v else None) for k, v in rec["FC"].__dict__.items()}
res["clean_keep_largest"] = timed(lambda: qc.clean_segmentation(dev["FC"]))
print(res["segmentation_shape_both_queued"], res["segmentation_shape_both_host_ms"], flush=True)
json.dump(res, open(os.path.join(OUT, "profile_components.json"), "w"), indent=1)

try:
    import scipy.ndimage as ndi
    m = maps["FC"] > 0.5
    for c, r in ((6, 1), (26, 3)):
        tt = []
        for _ in range(3):
            t0 = time.perf_counter()
            lab, k = ndi.label(m, ndi.generate_binary_structure(3, r))
            tt.append((time.perf_counter() - t0) * 1e3)
        res[f"scipy_label_{c}_ms"] = dict(median_ms=float(np.median(tt)), min_ms=float(min(tt)), max_ms=float(max(tt)), K=int(k))
        got = ops.label_components(dev["FC"], connectivity=c)
        res[f"scipy_equal_{c}"] = bool(np.array_equal(got[1].cpu().numpy(), lab)) and int(got[0][2]) == k
    t0 = time.perf_counter()
    ndi.label(~m, ndi.generate_binary_structure(3, 1))
    res["scipy_label_complement_6_ms"] = (time.perf_counter() - t0) * 1e3
except ImportError:
    res["scipy"] = "absent"
json.dump(res, open(os.path.join(OUT, "profile_components.json"), "w"), indent=1)
print(json.dumps({k: v for k, v in res.items() if k.startswith("scipy")}), flush=True)

if "--pipeline" in sys.argv:
    from oai_analysis_2_amd.image import Image
    from oai_analysis_2_amd.pipeline import CROP_ZYX, OVERLAP_ZYX, TILE_ZYX, VolumePipeline
    from oai_analysis_2_amd.registration import IconEngine
    from oai_analysis_2_amd.segmentation.engine import UNetEngine
    from oai_analysis_2_amd.synth import make_icon_state_dict, make_unet_state_dict, make_volume
    shape = (160, 384, 384)
    unet = UNetEngine(make_unet_state_dict(0), precision="fp16x3")
    atlas = Image(make_volume(1000, shape), [0.36, 0.36, 0.7], [0.0, 0.0, 0.0])
    pipe = VolumePipeline(unet, IconEngine(make_icon_state_dict(0, last_scale=0.1)), atlas)
    vol_np = make_volume(0, shape)
    vol = torch.from_numpy(vol_np).cuda()
    meta = Image(vol_np, [0.36, 0.36, 0.7], [2.0, -3.0, 1.0])
    unet.calibrate_volume(vol, TILE_ZYX, OVERLAP_ZYX, CROP_ZYX)
    for _ in range(2):
        pipe.run(vol, meta); pipe.run(vol, meta, seg_qc=True)
    off, on = [], []
    for _ in range(6):                                           # alternating, host clock around a run that ends synchronised
        for flag, into in ((False, off), (True, on)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = pipe.run(vol, meta, seg_qc=flag)
            torch.cuda.synchronize(); into.append((time.perf_counter() - t0) * 1e3)
    res["pipeline_run_ms"] = dict(median=float(np.median(off)), min=float(min(off)), max=float(max(off)))
    res["pipeline_run_seg_qc_ms"] = dict(median=float(np.median(on)), min=float(min(on)), max=float(max(on)))
    res["pipeline_seg_qc_FC"] = {k: (v if not isinstance(v, float) or v == v else None) for k, v in r.seg_qc["FC"].__dict__.items()}
    print(res["pipeline_run_ms"], res["pipeline_run_seg_qc_ms"], flush=True)
    json.dump(res, open(os.path.join(OUT, "profile_components.json"), "w"), indent=1)
