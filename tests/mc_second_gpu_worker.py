"""Child process of tests/test_mc_second_gpu.py: the first library call of the process is marching cubes on cuda:1, then the same on
cuda:0 (and on cuda:1 again); each must equal oracle/mesh.py.  The case tables are __constant__ memory, which every GPU holds on its own."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oai_analysis_2_amd import mesh_processing as mp      # noqa: E402
from oai_analysis_2_amd.synth import make_volume          # noqa: E402
from oracle import mesh as om                             # noqa: E402


def main():
    assert torch.cuda.device_count() >= 2
    vol = make_volume(0, (24, 40, 36))
    level, spacing = float(np.median(vol)), (0.36, 0.37, 0.7)
    rv, rf = om.marching_cubes(vol, level, spacing)
    assert len(rf) > 1000
    for device in ("cuda:1", "cuda:0", "cuda:1"):
        gv, gf = mp.marching_cubes(torch.from_numpy(vol).to(device), level, spacing)
        print(device, gv.shape, gf.shape, "reference", rv.shape, rf.shape, flush=True)
        assert gf.shape == rf.shape and np.array_equal(gf, rf), device
        assert gv.tobytes() == rv.tobytes(), device


if __name__ == "__main__":
    main()
