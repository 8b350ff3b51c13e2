"""tools/gpu_encode_random.py as a regression test: seeded random encoder configurations, every frame against vecgen
(or the CPU rebuild from the reported planes), the oracle, the source and OpenJPEG."""
import ast
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAWS = 200


def test_random_configurations():
    """two seeds of 200 draws: layout, sizes 1 .. 700 (a third of the widths above 256), levels 0 .. 8 / 11 / 32, every
    legal block shape, MCT, 5/3 or 9/7 at a log-uniform step, content, automatic or fixed guard bits, batches of 1 .. 4
    frames of different sizes with padded and poisoned rows, a budget in one draw of three.  Every draw is compared,
    and at least a quarter of them also go through OpenJPEG.  The time limit only ends a hang (the decoder sweep's)."""
    tool = os.path.join(ROOT, "tools", "gpu_encode_random.py")
    for seed in ("5", "6"):
        r = subprocess.run([sys.executable, tool, str(DRAWS), seed], capture_output=True, text=True, timeout=900)
        last = r.stdout.splitlines()[-1] if r.stdout.strip() else ""
        print(last)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert last.startswith("done ") and "'bad': 0" in last and "'skipped': 0" in last, last
        stat = ast.literal_eval(last[5:])
        assert stat["draws"] == DRAWS and stat["ok"] == DRAWS
        assert 4 * stat["opj"] >= stat["draws"], stat
