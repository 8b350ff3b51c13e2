"""tools/gpu_encode_random.py --tiles as a regression test: the seeded random encoder configurations of
tests/test_encode_random_gpu.py, each with a random tile size (strips included), every frame against vecgen (or the CPU
rebuild from the reported planes), the oracle, the source and OpenJPEG."""
import ast
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAWS = 32


def test_random_tiled_configurations():
    """one seed of 32 draws; every draw is tiled and compared, some of them are strips, and a quarter or more also go
    through OpenJPEG.  The time limit only ends a hang."""
    tool = os.path.join(ROOT, "tools", "gpu_encode_random.py")
    r = subprocess.run([sys.executable, tool, "--tiles", str(DRAWS), "7"], capture_output=True, text=True, timeout=600)
    last = r.stdout.splitlines()[-1] if r.stdout.strip() else ""
    print(last)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert last.startswith("done ") and "'bad': 0" in last and "'skipped': 0" in last, last
    stat = ast.literal_eval(last[5:])
    assert stat["draws"] == DRAWS and stat["ok"] == DRAWS and stat["tiled"] == DRAWS and stat["strips"] > 0
    assert 4 * stat["opj"] >= stat["draws"], stat
