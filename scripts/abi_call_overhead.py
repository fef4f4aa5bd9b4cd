"""The measurement behind profiles/abi_call_path.md: the host cost of one call through the Python side of the C ABI.  10 000 un-synchronised
ops.mask_overlap calls on an 8-element tensor, then one synchronise: wall time per call, which at this size is the Python call path (argument
checks, two small allocations, the device switch, the stream lookup, the ctypes call) and the launch, not the kernel.  Needs a GPU.
Usage: python scripts/abi_call_overhead.py [--root TREE] [--calls N] [--rounds R]    (--root: import the package from another checkout)"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=None, help="import oai_analysis_2_amd from this checkout instead of the one this script lies in")
ap.add_argument("--calls", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from oai_analysis_2_amd import ops

a = torch.rand(8).cuda()
for _ in range(200):
    ops.mask_overlap(a)
torch.cuda.synchronize()
us = []
for _ in range(args.rounds):
    t0 = time.perf_counter()
    for _ in range(args.calls):
        ops.mask_overlap(a)
    torch.cuda.synchronize()
    us.append(1e6 * (time.perf_counter() - t0) / args.calls)
print(json.dumps({"what": "abi_call_overhead", "root": args.root or ".", "calls": args.calls, "us_per_call_median": statistics.median(us),
                  "us_per_call_min": min(us), "us_per_call_max": max(us), "rounds": us}), flush=True)
