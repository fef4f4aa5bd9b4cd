"""GPU: marching cubes on a GPU that is not the first one of its process (tests/mc_second_gpu_worker.py, a fresh child process so that
no earlier call has uploaded the case tables): csrc/mesh.hip uploads its __constant__ tables once per device."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_first_call_on_the_second_gpu_then_on_the_first():
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs two GPUs in one process, this machine shows {torch.cuda.device_count()}")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mc_second_gpu_worker.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
