"""Wall time of get_mesh_from_probability_map's device part (mesh_processing.cuberille_device, csrc/cuberille.hip) on
scripts/bench_mesh_resident.py's full-size FC slab (160x384x384), device tensor in, device tensors out, warm, with the reference's
settings; vertex, face and projection-step statistics; and the numpy restatement (tests/cuberille_ref.py) on a crop of the same map,
timed on the host and compared bit for bit with the device result of that crop.  --reps N: timed calls (default 5, at least 3);
--kernel-only: only the timed calls, nothing else (for a kernel trace)."""
import argparse, os, sys, time
import numpy as np, torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from bench_mesh_resident import fc_slab
from oai_analysis_2_amd import mesh_processing as mp
from oai_analysis_2_amd.image import Image

CROP = (slice(48, 112), slice(96, 224), slice(128, 256))            # 64 x 128 x 128 voxels of the slab, across the cartilage shell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    reps = max(a.reps, 3)
    img = fc_slab()
    vol = torch.from_numpy(img.array).cuda()
    call = lambda: mp.cuberille_device(vol, spacing_xyz=img.spacing, origin_xyz=img.origin, direction=img.direction)
    out = call()                                                    # warm-up: library load, code objects, allocator
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    if a.kernel_only:
        print("cuberille FC slab ms: " + " ".join(f"{t:.2f}" for t in ts))
        return
    v, f, k = (x.cpu().numpy() for x in out)
    again = call()
    same = all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(again, (v, f, k)))
    print(f"FC slab {tuple(img.array.shape)}, spacing {tuple(img.spacing)}: {len(v)} vertices, {len(f)} triangles; "
          f"same bits on a second call: {same}")
    print(f"  ms per call (warm, {reps} reps): " + " ".join(f"{t:.2f}" for t in ts) + f"   median {np.median(ts):.2f}")
    print(f"  projection steps per vertex: mean {k.mean():.2f}, median {np.median(k):.0f}, p99 {np.percentile(k, 99):.0f}, max {k.max()}, "
          f"at the cap (> 50 moves): {int((k > 50).sum())}; histogram 0..8: {np.bincount(k, minlength=9)[:9].tolist()}")
    import cuberille_ref as ref
    crop = np.ascontiguousarray(img.array[CROP])
    t = time.perf_counter()
    want = ref.cuberille(crop, 0.5, spacing=img.spacing)
    t_ref = time.perf_counter() - t
    cv, cf, ck = (x.cpu().numpy() for x in mp.cuberille_device(Image(crop, img.spacing)))
    bits = cv.tobytes() == want["verts"].tobytes() and np.array_equal(cf, want["faces"]) and np.array_equal(ck, want["steps"])
    print(f"  numpy restatement on the crop {crop.shape} ({crop.size} voxels, {len(want['verts'])} vertices): {t_ref * 1e3:.0f} ms on the host; "
          f"device result bitwise equal: {bits}")


if __name__ == "__main__":
    main()
