"""tools/gpu_transcode_random.py as a regression test: the seeded random sources of tests/xc_random.py through the
transcoder, every call against the CPU rebuild from the source's indices, the product decoder, the oracle and the
refusals (the tool's docstring has the list).  The seeds are the ones tests/test_transcode_random_host.py pins on the
CPU; a seed's draws run in slices, each a child process of its own."""
import ast
import os
import subprocess
import sys

import pytest

from test_transcode_random_host import CAP, DRAWS, SEEDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE = 25
CASES = [(seed, first, False) for seed in SEEDS for first in range(0, DRAWS, SLICE)] + [(SEEDS[0], 0, True), (SEEDS[1], DRAWS - SLICE, True)]
STATE = {"fatal": None}                                   # the case after which nothing more is started on the device


@pytest.mark.parametrize("seed,first,rounds", CASES, ids=["%d_%03d%s" % (s, f, "_rounds" if r else "") for s, f, r in CASES])
def test_random_sources(seed, first, rounds):
    """SLICE draws of a seed: none bad, none skipped, every draw compared or left out for one of the two reasons the CPU
    test allows, and those within its cap.  The time limit only ends a hang.  After a child that reported a failure of
    the device, died of a signal or ran into the limit, the remaining cases fail without starting one"""
    assert STATE["fatal"] is None, "not started: the device failed in %s" % (STATE["fatal"],)
    tool = os.path.join(ROOT, "tools", "gpu_transcode_random.py")
    cmd = [sys.executable, tool] + (["--rounds"] if rounds else []) + [str(SLICE), str(seed), str(first)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        STATE["fatal"] = (seed, first, rounds, "time limit")
        raise
    if r.returncode < 0 or "FATAL" in r.stdout:
        STATE["fatal"] = (seed, first, rounds, r.returncode)
    last = r.stdout.splitlines()[-1] if r.stdout.strip() else ""
    print(last)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert last.startswith("done ") and "'bad': 0" in last and "'skipped': 0" in last, last
    stat = ast.literal_eval(last[5:])
    assert stat["draws"] == SLICE and stat["ok"] + stat["left_out"] == SLICE, stat
    assert stat["left_out"] <= CAP * SLICE, stat
    assert stat["calls"] > 0 and stat["blocks"] > 0, stat
    if rounds:
        assert stat["calls_of_rounds"] > 0, stat
