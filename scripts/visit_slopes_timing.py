#!/usr/bin/env python
"""Timings behind profiles/longitudinal.md; prints one JSON line.

The input is SYNTHETIC: 200 subjects x 7 visits on V = 30 002 vertices (the size of an atlas inner mesh), the 1400 rows of the visit
matrix in scrambled order, thickness of 2.5 mm + 0.05 mm noise with a loss of 0.05 mm a year, 10 % of the entries missing.

    python scripts/visit_slopes_timing.py [--repeats 21]
        Device events around the call, warm, the median of ``--repeats``, the variants alternating round by round:
          kernel        ops.visit_slopes with all six outputs (the slot table's small launch included)
          rate_only     with rate and mask alone: what ``LongitudinalCohort.change("rate")`` asks for (pass 3 does not run)
          torch         the same sums written as plain torch ops on the device -- index_select of the rows into [S, 7, V], masked sums over
                        the visit axis in float64 -- the thing the kernel replaces.  It is only possible because every subject here
                        has the same number of visits; it fixes no order of summation and is compared with a tolerance, not to the bit.
        and the bytes the kernel must move -- every value and mask byte once in, every output once out -- with the bandwidth that the
        kernel's time implies against the 6.3 TB/s that a copy reaches on this GPU.
        With OAI_LIB_PATH pointing at a diagnostic build, OAI_VISIT_SLOPES_HOLD=0 in the environment times the design that re-reads
        every slot in every pass instead of holding the first eight in registers.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from group_stats_timing import _spread  # noqa: E402

N_SUBJECTS, N_VISITS, N_VERTS, MISSING = 200, 7, 30002, 0.10
HBM_BYTES_PER_S = 6.3e12


def study():
    import visit_slopes_ref as vref
    rng = np.random.default_rng(7)
    schedule = vref.oai_like_schedule(rng, N_SUBJECTS, N_VISITS, N_VISITS)
    times = np.concatenate(schedule)
    E = len(times)
    offsets = (np.arange(N_SUBJECTS + 1) * N_VISITS).astype(np.int32)
    rows = rng.permutation(E).astype(np.int32)
    Y = np.empty((E, N_VERTS), np.float32)
    Y[rows] = (2.5 + 0.05 * rng.normal(size=(E, N_VERTS)) - 0.05 * times[:, None]).astype(np.float32)
    mask = (rng.random((E, N_VERTS)) >= MISSING).astype(np.uint8)
    return Y, mask, offsets, rows, times, np.array([t[0] for t in schedule])


def torch_formulation(Y, mask, rows, times, tref, min_visits=2):
    """rate, avg, fit_ref, resid_sd, n, ok as [S, V] from masked sums over the visit axis of [S, 7, V]."""
    import torch
    y = Y.index_select(0, rows).view(N_SUBJECTS, N_VISITS, -1).to(torch.float64)
    m = mask.index_select(0, rows).view(N_SUBJECTS, N_VISITS, -1) != 0
    t = times.view(N_SUBJECTS, N_VISITS, 1)
    zero = torch.zeros((), dtype=torch.float64, device=Y.device)
    n = m.sum(dim=1)
    nd = n.to(torch.float64)
    tb = torch.where(m, t, zero).sum(dim=1) / nd
    yb = torch.where(m, y, zero).sum(dim=1) / nd
    dt, dy = t - tb[:, None, :], y - yb[:, None, :]
    Sxx = torch.where(m, dt * dt, zero).sum(dim=1)
    Sxy = torch.where(m, dt * dy, zero).sum(dim=1)
    rate = Sxy / Sxx
    r = dy - rate[:, None, :] * dt
    rss = torch.where(m, r * r, zero).sum(dim=1)
    ok = (n >= min_visits) & (Sxx > 0)
    fit_ref = yb + rate * (tref[:, None] - tb)
    resid_sd = torch.sqrt(rss / (nd - 2.0))
    return [torch.where(ok, x, zero) for x in (rate, yb, fit_ref, resid_sd)] + [n.to(torch.int32), ok.to(torch.uint8)]


def main(args):
    import torch
    from oai_analysis_2_amd import _lib, ops
    Y, mask, offsets, rows, times, tref = (torch.from_numpy(a).cuda() for a in study())
    rows64 = rows.to(torch.int64)
    variants = {"kernel": lambda: ops.visit_slopes(Y, offsets, rows, times, tref, mask=mask),
                "rate_only": lambda: ops.visit_slopes(Y, offsets, rows, times, tref, mask=mask, want=("rate", "mask")),
                "torch": lambda: torch_formulation(Y, mask, rows64, times, tref)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            torch.cuda.synchronize()
            ms[name].append(start.elapsed_time(stop))
    got, ref = variants["kernel"](), variants["torch"]()
    ok = (got.mask != 0) & (ref[5] != 0)
    differ = {"mask": int((got.mask != ref[5]).sum().item()), "n": int((got.n != ref[4]).sum().item()),
              "rate_max_abs": float(((got.rate - ref[0]).abs() * ok).max().item()), "fit_ref_max_abs": float(((got.fit_ref - ref[2]).abs() * ok).max().item()),
              "resid_sd_max_abs": float(torch.where(ok & (got.n >= 3), (got.resid_sd - ref[3]).abs(), torch.zeros_like(ref[3])).max().item())}
    E, S, V = int(rows.numel()), N_SUBJECTS, N_VERTS
    moved = {"kernel": E * V * (4 + 1) + S * V * (4 * 8 + 4 + 1), "rate_only": E * V * (4 + 1) + S * V * (8 + 1)}
    spread = {k: _spread(v) for k, v in ms.items()}
    print(json.dumps({"row": "visit_slopes", "library": os.path.basename(_lib.LIB_PATH), "hold": os.environ.get("OAI_VISIT_SLOPES_HOLD", "default"),
                      "n_subjects": S, "visits_per_subject": N_VISITS, "n_rows": E, "n_verts": V, "missing": MISSING, "repeats": args.repeats,
                      "ms": spread, "bytes_moved": moved,
                      "implied_TB_per_s": {k: round(moved[k] / (spread[k]["median"] * 1e-3) / 1e12, 3) for k in moved},
                      "floor_ms_at_6.3_TB_per_s": {k: round(1e3 * moved[k] / HBM_BYTES_PER_S, 4) for k in moved},
                      "torch_over_kernel": round(spread["torch"]["median"] / spread["kernel"]["median"], 2),
                      "kernel_against_torch": differ}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    main(ap.parse_args())
