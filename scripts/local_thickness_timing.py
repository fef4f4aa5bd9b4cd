"""The measurement behind profiles/local_thickness.md, at the workload's 160 x 384 x 384 with the DESS spacing: oai_local_thickness on a
synthetic curved sheet of cartilage-like thickness and on one ball of radius 20 voxels, beside the EDT that feeds it; oai_masked_stats;
qc.local_thickness with both radius sources.  With the diagnostic library (python -m oai_analysis_2_amd.build --diag, then
OAI_LIB_PATH=build/diag/liboai_hip_diag.so) also 16 lanes per centre against a whole wave against the library's mix of the two,
alternating in one process, and the share of atomics that the plain load skipped.  The per-kernel times come from a kernel trace of this script run with --trace (one call per
case, nothing else).  Needs a GPU.  Usage: python scripts/local_thickness_timing.py [--trace] [--out DIR]"""
import ctypes as C
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oai_analysis_2_amd import _lib, ops, qc

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "."
os.makedirs(OUT, exist_ok=True)
SHAPE, SPACING = (160, 384, 384), (0.36458333, 0.36458333, 0.7)
DIAG = bool(os.environ.get("OAI_LIB_PATH"))
res = {"shape": SHAPE, "spacing": SPACING, "diag_library": DIAG}


def sheet():
    """A curved sheet over a disc, 1.5 to 3 mm thick (2 to 4 voxels along z, 4 to 8 in the plane where it tilts): synthetic, shaped
    like a femoral cartilage plate, not a segmentation."""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float32) for n in SHAPE), indexing="ij", sparse=True)
    u, v = (x - 192.0) / 150.0, (y - 192.0) / 150.0
    mid = 56.0 + 55.0 * (u * u + 0.6 * v * v) + 6.0 * np.sin(3.0 * u)                   # voxels along z: a bowl, steep at the rim
    half_mm = 0.75 + 0.75 * np.clip(1.0 - (u * u + v * v), 0.0, 1.0)
    inside = (np.abs(z - mid) * np.float32(SPACING[2]) < half_mm) & (u * u + v * v < 1.0)
    return np.where(inside, np.float32(0.9), np.float32(0.05))


def ball(radius=20.0):
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float32) - (n - 1) / 2.0 for n in SHAPE), indexing="ij", sparse=True)
    return np.where(x * x + y * y + z * z <= radius * radius, np.float32(0.9), np.float32(0.05))


def timed(fn, warm=2, reps=7, inner=3):
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


def raw_call(rsq, ws, thick, stats):
    D, H, W = SHAPE
    _lib.call("oai_local_thickness", rsq.data_ptr(), D, H, W, (C.c_double * 3)(*SPACING), ops.MAX_WINDOW_VOXELS, None, thick.data_ptr(),
              ws.data_ptr(), ws.numel(), stats.data_ptr(), _lib.STREAM, device=rsq.device)


cases = {"sheet": sheet(), "ball20": ball()}
for name, m in cases.items():
    vol = torch.from_numpy(m).cuda()
    r = res[name] = {"set_voxels": int((m > 0.5).sum())}
    edt = lambda: ops.distance_transform(ops.mask_surface(vol, 0.5, "complement"), SPACING, return_squared=True)
    rsq = edt()[1]
    ws = _lib.workspace("oai_local_thickness", vol.device, *SHAPE)
    thick = torch.empty(SHAPE, dtype=torch.float32, device=vol.device)
    stats = torch.empty(4, dtype=torch.int64, device=vol.device)
    if "--trace" in sys.argv:                     # one call per case under the kernel trace
        raw_call(rsq, ws, thick, stats)
        torch.cuda.synchronize()
        r["stats"] = stats.cpu().numpy().tolist()
        continue
    r["edt_ms"] = timed(edt)
    r["local_thickness_ms"] = timed(lambda: raw_call(rsq, ws, thick, stats))
    r["stats"] = stats.cpu().numpy().tolist()
    r["tests_per_s_whole_call"] = r["stats"][1] / (r["local_thickness_ms"]["median_ms"] * 1e-3)
    r["thickness_max_mm"] = float(thick.max())
    setmask = ops.mask_surface(vol, 0.5, "set")
    r["masked_stats_ms"] = timed(lambda: ops.masked_stats(thick, setmask))
    if DIAG:
        for g in (16, 64, 0) * 2:                 # alternating: the same process, the same buffers.  0: the library's own choice
            os.environ["OAI_LT_GROUP"] = str(g)
            r.setdefault(f"group{g}_ms", []).append(timed(lambda: raw_call(rsq, ws, thick, stats)))
            counters = ws[(8 * rsq.numel() + 255) // 256 * 256:][:64].view(torch.int64).cpu().numpy()      # the counters follow the keys
            r[f"group{g}_met_issued"] = [int(counters[4]), int(counters[5])]
        del os.environ["OAI_LT_GROUP"]
    else:
        t = []
        for radius in ("voxel", "mesh"):
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rec = qc.local_thickness(vol, SPACING, radius=radius)
                t.append((time.perf_counter() - t0) * 1e3)
            r[f"qc_{radius}_host_ms"] = dict(median_ms=float(np.median(t[-3:])), min_ms=float(min(t[-3:])), max_ms=float(max(t[-3:])))
            r[f"record_{radius}"] = {k: (v if not isinstance(v, float) or v == v else None) for k, v in rec.__dict__.items() if k != "thickness_map"}
    print(name, json.dumps(r), flush=True)
    json.dump(res, open(os.path.join(OUT, "profile_local_thickness" + ("_diag" if DIAG else "") + ".json"), "w"), indent=1)
json.dump(res, open(os.path.join(OUT, "profile_local_thickness" + ("_trace" if "--trace" in sys.argv else "_diag" if DIAG else "") + ".json"), "w"), indent=1)
