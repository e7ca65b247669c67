"""GPU: weighted shards (L = W_loc o A_loc) with TWO processes sharing the one GPU of the test box (tools/ranks_chain_check.py --backend gloo).

Each rank builds ITS rows of the seeded A and W, runs the weighted adjoint and normal operator as ranged fused chains with the exchange of a
finished range behind its kernel, and CG on the normal equations; the launcher compares with the CPU oracle.  RCCL refuses two ranks on one
device, so the exchange is staged through the host over gloo.  The script runs in its own processes under a hard time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weighted_shards_on_two_ranks_of_one_gpu(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ranks_chain_check.py"), str(tmp_path), "--ranks", "2", "--backend", "gloo"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "RANKS CHAINS OK" in out.stdout
