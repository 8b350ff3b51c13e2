"""bench.py's plain run: --dump-outputs writes a fixed sample of what the last timed step decoded, and what is not
needed for `value` (parity, the other legs) runs only with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

H, W, C = bench.HEIGHT, bench.WIDTH, bench.NCOMP


class FrameJob:
    """stands in for one of the bench's jobs: frame f of job j is frame f * njobs + j of the batch, `frame(g)` of it"""

    def __init__(self, j, njobs, frame):
        self.j, self.njobs, self.frame = j, njobs, frame

    def download_frame(self, f):
        return None, [self.frame(f * self.njobs + self.j).reshape(H, W * C)]


def _dump(path, frame, njobs, nframes):
    bench.dump_outputs(str(path), [FrameJob(j, njobs, frame) for j in range(njobs)], njobs, nframes)
    return {n: np.load(os.path.join(str(path), n)) for n in sorted(os.listdir(str(path)))}


def test_dump_outputs_is_a_fixed_sample_of_the_frames(tmp_path):
    base = (np.arange(H * W * C, dtype=np.uint32) * 7 % 256).astype(np.uint8)

    def frame(g):                                            # frame g differs from frame 0 by g (mod 256) everywhere
        return (base + np.uint8(g % 256)).reshape(H, W, C)
    njobs, nframes = 2, 128
    a = _dump(tmp_path / "a", frame, njobs, nframes)
    b = _dump(tmp_path / "b", frame, njobs, nframes)
    assert sorted(a) == ["frame_index.npy", "frames_row_sums.npy", "frames_sample.npy"]
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(a[name], b[name]), name
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in a) <= 64 << 20
    idx = a["frame_index.npy"].astype(np.int64)
    assert len(idx) == bench.DUMP_FRAMES == len(set(idx)) and idx[0] == 0 and idx[-1] == nframes - 1
    sample, rows = a["frames_sample.npy"], a["frames_row_sums.npy"]
    assert sample.shape == (len(idx), bench.DUMP_SAMPLES) and rows.shape == (len(idx), H, C)
    for k, g in enumerate(idx):
        assert np.array_equal(rows[k], frame(g).sum(axis=1))
        assert np.all((sample[k] - sample[0]) % 256 == (g - idx[0]) % 256), g     # same positions, frame g
    assert len(np.unique(sample[0])) == 256


def test_dump_outputs_of_a_small_batch(tmp_path):
    out = _dump(tmp_path, lambda g: np.full((H, W, C), g + 1, np.uint8), 1, 2)
    assert out["frame_index.npy"].tolist() == [0.0, 1.0]
    assert np.all(out["frames_sample.npy"][1] == 2.0)


@pytest.mark.parametrize("argv,msg", [(["--steps", "0"], "--steps must be at least 1"),
                                      (["--part1", "80"], "--part1 is a leg of --full")])
def test_bench_refuses_before_touching_the_gpu(argv, msg):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and msg in out.stderr
    assert not out.stdout.strip()


@pytest.mark.gpu
def test_plain_run_dumps_what_it_decoded(tmp_path):
    """a small plain run: the JSON line of the timed steps alone, and its dump equals the same sample of the source
    images (the frames are lossless)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vecgen
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "4", "--distinct", "2", "--dump-outputs", str(tmp_path / "got")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["value"] > 0
    assert res["parity_checked"] is False and res["config"]["block_errors"] == 0
    assert "roofline" not in res and "cpu_baseline" not in res and "stream240" not in res
    src = [np.stack(vecgen.synth_image(W, H, C, depth=8, seed=2 + i, noise=8), -1).astype(np.uint8) for i in range(2)]
    want = _dump(tmp_path / "want", lambda g: src[g % 2], 2, 4)
    got = {n: np.load(str(tmp_path / "got" / n)) for n in want}
    for name in want:
        assert np.array_equal(got[name], want[name]), name
