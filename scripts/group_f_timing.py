#!/usr/bin/env python
"""Timings behind profiles/group_f.md; prints one JSON line per row.

The input is SYNTHETIC, the cohort of scripts/group_regression_timing.py: N = 200 knees of 2 mm + 0.3 mm noise on 30 002 vertices, 5 % of
the entries missing.  The F design is an intercept, age, and the 0 / 1 dummies of a factor whose level is the knee index modulo k + 1:
(p, k) = (4, 2) is a 3-level factor and (6, 4) a 5-level one, each with one covariate.

    python scripts/group_f_timing.py kernel [--repeats 9] [--permutations 1000]
        ops.regression_f over all the rows in one call and, IN THE SAME RUN, ops.regression_t at the same p (the design of
        scripts/group_regression_timing.py), each with and without a mask: device events around the call, warm, the median of
        ``--repeats``; between repeats a 512 MiB buffer is overwritten so that no input is left in the L2 or the Infinity Cache.
    python scripts/group_f_timing.py test [--rounds 9] [--permutations 1000]
        stats.anova_test (5 levels and one covariate) without and with ``tfce``, alternating round by round in one process, on the
        sphere of scripts/group_stats_timing.py: host clock around the call (it ends in its one download), warm.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from group_regression_timing import N_KNEES, N_VERTS, _spread, cohort_arrays, design, fp64_operations  # noqa: E402

SHAPES = ((4, 2), (6, 4))


def factor(k):
    """(the level of every knee, age): k + 1 levels in turn."""
    return np.arange(N_KNEES) % (k + 1), np.random.default_rng(k).uniform(45, 80, N_KNEES)


def f_design(p, k):
    """[N, p]: the intercept, p - k - 1 covariates (age first), the k dummies; centred and scaled as stats.f_test does."""
    level, age = factor(k)
    rng = np.random.default_rng(100 + p)
    cols = [np.ones(N_KNEES), age] + [rng.normal(size=N_KNEES) for _ in range(p - k - 2)] + [(level == g).astype(np.float64) for g in range(1, k + 1)]
    D = np.stack(cols, axis=1)
    D[:, 1:] -= D[:, 1:].mean(axis=0)
    D[:, 1:] /= np.sqrt((D[:, 1:] ** 2).sum(axis=0))
    return np.ascontiguousarray(D)


def kernel(args):
    import torch
    from oai_analysis_2_amd import _lib, ops, stats
    dev = torch.device("cuda", 0)
    Y, mask = cohort_arrays()
    Yd, md = torch.from_numpy(Y).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev)
    P = args.permutations
    index = torch.from_numpy(stats.index_permutations(N_KNEES, P, seed=0).index).to(dev)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    peak = 39.3e12                                                         # fp64 vector instructions x lanes per second (profiles/group_stats.md)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeats):
            flush.fill_(1)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            torch.cuda.synchronize()
            out.append(start.elapsed_time(stop))
        return _spread(out)

    for p, k in SHAPES:
        for masked in (True, False):
            m = md if masked else None
            n_ops = fp64_operations(p, masked)
            rows = {}
            for name, D, q in (("oai_regression_t", design(p), p - 1), ("oai_regression_f", f_design(p, k), p - k)):
                Dd, Zd = torch.from_numpy(D).to(dev), torch.from_numpy(np.ascontiguousarray(D[:, :q])).to(dev)
                prepared = ops.regression_prepare(Yd, m, Zd)
                ws = _lib.workspace(name, dev, P, N_VERTS, N_KNEES, p)
                if name == "oai_regression_t":
                    rows[name] = timed(lambda: ops.regression_t(prepared, Dd, index, 0, P, workspace=ws))
                else:
                    rows[name] = timed(lambda: ops.regression_f(prepared, Dd, index, 0, P, k, workspace=ws))
                    tile = ops.regression_f(prepared, Dd, index, 0, P, k, workspace=ws)
                    observed = {"max_f": float(torch.nan_to_num(tile[0]).max()), "nan_in_row_0": int(torch.isnan(tile[0]).sum())}
                del prepared, ws
            print(json.dumps({"row": f"p={p} k={k} {'masked' if masked else 'no mask'}", "rows": P, "ms": rows,
                              "f_over_t": round(rows["oai_regression_f"]["median"] / rows["oai_regression_t"]["median"], 4),
                              "fp64_operations_per_knee_row_vertex": n_ops, "observed": observed,
                              "share_of_fp64_issue_rate": {name: round(n_ops * P * N_VERTS * N_KNEES / (ms["median"] * 1e-3) / peak, 3)
                                                           for name, ms in rows.items()}}), flush=True)


def test(args):
    import torch
    from group_stats_timing import cohort_arrays as sphere_cohort, sphere
    from oai_analysis_2_amd import mesh_processing as mp, stats
    verts, faces = sphere()
    atlas = SimpleNamespace(inner={"FC": mp.Mesh(verts, faces)}, device=torch.device("cuda", 0))
    Y, mask, _ = sphere_cohort(len(verts))
    cohort = stats.ThicknessCohort(atlas, "FC", chunk=N_KNEES)
    for y, m in zip(Y, mask):
        cohort.add_vector(y, valid=m)
    level, age = factor(4)
    perms = stats.index_permutations(N_KNEES, args.permutations, seed=0)
    variants = {"anova_test": None, "anova_test_tfce": True}

    def ms(tfce):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = stats.anova_test(cohort, level, covariates=age, permutations=perms, tfce=tfce)
        return 1e3 * (time.perf_counter() - t), res

    for tfce in variants.values():
        ms(tfce)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, tfce in variants.items():
            t, res = ms(tfce)
            times[name].append(t)
    V, P = cohort.n_verts, len(perms)
    print(json.dumps({"row": "test", "n_knees": N_KNEES, "n_verts": V, "permutations": P, "levels": 5, "covariates": 1,
                      "batch": {"plain": stats.regression_batch(V, N_KNEES, 6, P, False), "tfce": stats.regression_batch(V, N_KNEES, 6, P, False, tfce=True)},
                      "ms_per_test": {k: _spread(v) for k, v in times.items()},
                      "observed": {"max_f": float(res.max_f[0]), "max_tfce": float(res.max_tfce[0]), "p_fwer_min": float(np.nanmin(res.p_fwer)),
                                   "p_tfce_min": float(np.nanmin(res.p_tfce)), "tfce_clipped": res.tfce_clipped}}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=("kernel", "test"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--permutations", type=int, default=1000)
    a = ap.parse_args()
    {"kernel": kernel, "test": test}[a.row](a)
