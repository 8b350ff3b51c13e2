"""htj2k_compare_frames_ssim / htj2k_job_compare_ssim / the encoder's ssim switch on the GPU against the numpy model
(ssim_model): q32 and nwin for equality, ssim and all to 1e-12.

The sweep.  k_frame_ssim has one instantiation per (bytes per sample, interleaved components); the widths put no window,
one window, the ignored tail and the seam between waves (63 groups of 1, 2 or 4 block columns) into a row, the heights
the same for block rows and the default strip.  24 widths times the 14 layouts is more than the 200 cases a sweep may
have, so the subset takes every instantiation at every width (8 x 24 = 192 cases) and walks through the layouts of an
instantiation from width to width: every layout, every width, and every kernel at every width occur.  rgba64le is added
to the layouts of test_compare_gpu.py because no other one reaches the 32-byte group.  Linesize modes, base offsets,
host and device operands and the dirt are those of test_compare_gpu.py.
Run as a program, the module runs the sweeps on its own contexts: test_everything_on_poisoned_buffers does that in a
child process under HTJ2K_POISON=1."""
import ctypes
import math
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: device operands are made through it)

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.dirname(HERE)]

import cmp_model as cm
import ffmpeg_ht_amd as m
import ssim_model as sm
from test_compare_gpu import LAYOUTS as CMP_LAYOUTS, LS_MODES, OFFSETS, Operand, pair

LAYOUTS = CMP_LAYOUTS + [("gray", 4), ("rgba64le", 16)]
WIDTHS = [7, 8, 11, 12, 15, 16, 20, 67, 68, 252, 255, 256, 259, 260, 264, 508, 512, 516, 520, 1020, 1024, 1028, 1032, 1036]
HEIGHTS = [7, 8, 11, 12, 16, 36, 37]


def kernel_of(fmt):
    nc, planar, _, _, _, by = cm.LAYOUTS[fmt]
    return by, 1 if planar else nc


def _cases():
    rnd = random.Random(21)
    by_kernel = {}
    for f, b in LAYOUTS:
        by_kernel.setdefault(kernel_of(f), []).append((f, b))
    picked = []
    for k in sorted(by_kernel):
        ls = by_kernel[k]
        for i, w in enumerate(WIDTHS):
            f, b = ls[i % len(ls)]
            picked.append((f, b, w, rnd.choice(HEIGHTS)))
    return [(f, b, w, h, LS_MODES[i % 4], OFFSETS[(i // 4) % 4]) for i, (f, b, w, h) in enumerate(picked)]


CASES = _cases()
assert len(CASES) <= 200
SMALL_CHROMA = [("yuv420p", 8, 14, 14), ("yuv420p", 8, 15, 15), ("yuv420p", 8, 17, 17)]     # chroma with 0, 1 and 1 windows


def identical(got, want):
    """two results of the library, or lists of them: every figure the same (NaN beside NaN)"""
    if isinstance(got, list):
        return len(got) == len(want) and all(identical(g, w) for g, w in zip(got, want))
    return sm.same(got, want, tol=0)


def model(a, b):
    return sm.ssim(a.raw_planes(), b.raw_planes(), a.fmt, a.bits)


def check_case(dec, fmt, bits, w, h, ls_mode, off, seed):
    a, b = pair(fmt, w, h, bits, seed, ls_mode, off, LS_MODES[(LS_MODES.index(ls_mode) + 1) % 4], OFFSETS[(OFFSETS.index(off) + 1) % 4])
    want = model(a, b)
    got = dec.compare_ssim([a.frame()], [b.frame()], fmt, bits)[0]
    assert sm.same(got, want), (fmt, bits, w, h, ls_mode, off, got, want)
    (fa, ka), (fb, kb) = a.on_device(), b.on_device()
    got = dec.compare_ssim([fa], [fb], fmt, bits, on_device=(True, True))[0]
    assert sm.same(got, want), ("device", fmt, bits, w, h, ls_mode, off, got, want)
    rng = np.random.default_rng(seed + 1)
    a.write(rng)
    a.dirty_padding(rng)
    b.dirty_padding(rng)
    assert sm.same(dec.compare_ssim([a.frame()], [b.frame()], fmt, bits)[0], want), ("dirt", fmt, bits, w, h)
    return want


def check_small_chroma(dec):
    for (fmt, bits, w, h), chroma in zip(SMALL_CHROMA, (0, 1, 1)):
        want = check_case(dec, fmt, bits, w, h, "row+1", 1, seed=w)
        assert want["nwin"] == [((w >> 2) - 1) * ((h >> 2) - 1), chroma, chroma, 0]


def check_strips(dec):
    """strip seams inside small frames: every strip height gives the struct of the default"""
    try:
        for fmt, bits in (("gray", 8), ("rgb24", 8), ("yuv422p10le", 10)):
            for w, h in ((68, 36), (260, 37)):
                a, b = pair(fmt, w, h, bits, w + h, "to64", 0, "row+13", 2)
                want = model(a, b)
                (fa, ka), (fb, kb) = a.on_device(), b.on_device()
                for rows in (0, 1, 2, 3, 8):
                    dec.set_int("ssim_rows", rows)
                    got = dec.compare_ssim([a.frame()], [b.frame()], fmt, bits)[0]
                    assert sm.same(got, want), (fmt, w, h, rows, got, want)
                    assert identical(dec.compare_ssim([fa], [fb], fmt, bits, on_device=(True, True))[0], got)
        for bad in (-1, 257, 1 << 20):
            with pytest.raises(m.Htj2kError) as e:
                dec.set_int("ssim_rows", bad)
            assert e.value.code == -22
        dec.set_int("ssim_rows", 256)
    finally:
        dec.set_int("ssim_rows", 0)


def op(fmt, w, h, bits, values, seed=0, ls="row", off=0):
    return Operand(fmt, w, h, bits, np.random.default_rng(seed), ls, off, values=values)


def check_contents(dec):
    for fmt, bits, w, h in (("gray", 8, 68, 36), ("rgb48le", 16, 67, 16), ("yuv422p10le", 10, 260, 12), ("gray16le", 16, 40, 20)):
        rng = np.random.default_rng(w)
        peak = (1 << bits) - 1
        a, _ = pair(fmt, w, h, bits, 5, "row+1", 1)
        noise = [np.clip(v + rng.integers(-1, 2, size=v.shape), 0, peak) for v in a.values]
        inv = [peak - v for v in a.values]
        for name, vb in (("noise", noise), ("inverse", inv)):
            b = op(fmt, w, h, bits, vb, 6, "to64", 2)
            want = model(a, b)
            got = dec.compare_ssim([a.frame()], [b.frame()], fmt, bits)[0]
            assert sm.same(got, want), (name, fmt, got, want)
            nc = cm.LAYOUTS[fmt][0]
            if name == "noise":
                assert all(s > 0.9 for s in got["ssim"][:nc]), got
            else:
                assert all(q < 0 and s < -0.9 for q, s in zip(got["q32"][:nc], got["ssim"][:nc])), got     # negative sums
    # the largest A .. D: all-zero against all-peak, all-peak against itself, at 16 bits
    w, h = 300, 44
    zero, full = np.zeros((h, w), np.uint16), np.full((h, w), 65535, np.uint16)
    nwin = (w // 4 - 1) * (h // 4 - 1)
    got = dec.compare_ssim([[zero]], [[full]], "gray16le", 16)[0]
    assert sm.same(got, sm.ssim([zero], [full], "gray16le", 16)) and got["nwin"] == [nwin, 0, 0, 0] and 0 < got["ssim"][0] < 1e-4
    got = dec.compare_ssim([[full]], [[full]], "gray16le", 16)[0]
    assert got["q32"] == [nwin << 32, 0, 0, 0] and got["ssim"][0] == 1.0 and got["all"] == 1.0


def check_division(dec):
    """one window: the device's (A * B) / (C * D) and rint against numpy's, bit for bit"""
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        a = rng.integers(0, 65536, size=(8, 8)).astype(np.uint16)
        b = np.where(rng.random((8, 8)) < 0.5, a, rng.integers(0, 65536, size=(8, 8))).astype(np.uint16)
        want = sm.ssim([a], [b], "gray16le", 16)
        got = dec.compare_ssim([[a]], [[b]], "gray16le", 16)[0]
        s = [int(t[0, 0]) for t in sm.window_sums(a.astype(np.int64), b.astype(np.int64))]
        print("division: sums", s, "device q", got["q32"][0], "model q", want["q32"][0])
        assert got["nwin"] == [1, 0, 0, 0] and got["q32"] == want["q32"], (seed, s, got, want)


def check_batches(dec):
    for fmt, bits in (("rgb24", 8), ("yuv422p10le", 10), ("rgba64le", 16)):
        # sizes that differ, the second pair without a window
        ps = [pair(fmt, w, h, bits, 10 + i, LS_MODES[i], OFFSETS[i], LS_MODES[3 - i], OFFSETS[3 - i])
              for i, (w, h) in enumerate([(68, 12), (17, 7), (260, 9), (24, 37)])]
        want = [model(a, b) for a, b in ps]
        assert want[1]["nwin"] == [0] * 4 and math.isnan(want[1]["all"]) and all(x["nwin"][0] for x in (want[0], want[2], want[3]))
        host_a, host_b = [a.frame() for a, _ in ps], [b.frame() for _, b in ps]
        da, db = [a.on_device() for a, _ in ps], [b.on_device() for _, b in ps]
        dev_a, dev_b = [f for f, _ in da], [f for f, _ in db]
        for on_a, on_b in ((False, False), (True, False), (False, True), (True, True)):
            got = dec.compare_ssim(dev_a if on_a else host_a, dev_b if on_b else host_b, fmt, bits, on_device=(on_a, on_b))
            assert len(got) == 4 and all(sm.same(g, w) for g, w in zip(got, want)), (fmt, on_a, on_b, got, want)
        assert dec.compare_ms() > 0
        # a pair without windows alone: valid, nothing launched
        got = dec.compare_ssim(host_a[1:2], host_b[1:2], fmt, bits)
        assert sm.same(got[0], want[1]) and dec.compare_ms() == 0
        with pytest.raises(m.Htj2kError) as e:
            dec.compare_ssim(host_a[:2], [host_b[0], host_b[2]], fmt, bits)
        assert e.value.code == -22
    with pytest.raises(m.Htj2kError) as e:
        dec.compare_ssim([[np.zeros((8, 8), np.uint8)]], [[np.zeros((8, 8), np.uint8)]], "gray", 3)
    assert e.value.code == -22


def check_many_frames(dec, n=70000):
    """more pairs than grid.z takes in one launch: 8 x 8 gray frames, one window each, out of two buffers"""
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    b = np.where(rng.random((n, 64)) < 0.5, a, rng.integers(0, 256, size=(n, 64), dtype=np.uint8)).astype(np.uint8)
    rec = np.dtype({"names": ["data", "linesize", "width", "height", "pix_fmt"], "formats": [("<u8", 4), ("<i4", 4), "<i4", "<i4", "<i4"],
                    "offsets": [0, 32, 48, 52, 56], "itemsize": ctypes.sizeof(m.Frame)})
    tabs = []
    for x in (a, b):
        t = np.zeros(n, rec)
        t["data"][:, 0] = x.ctypes.data + 64 * np.arange(n, dtype=np.uint64)
        t["linesize"][:, 0] = 8
        t["width"], t["height"], t["pix_fmt"] = 8, 8, m.PIX_NAMES.index("gray")
        tabs.append(t)
    out = (m.FrameSsim * n)()
    r = dec.L.htj2k_compare_frames_ssim(dec.h, tabs[0].ctypes.data_as(ctypes.c_void_p), 0, tabs[1].ctypes.data_as(ctypes.c_void_p), 0,
                                        n, 8, out)
    assert r == 0
    got = np.frombuffer(out, np.dtype({"names": ["q32", "nwin", "ssim", "all"], "formats": [("<i8", 4), ("<u8", 4), ("<f8", 4), "<f8"],
                                       "offsets": [0, 32, 64, 96], "itemsize": ctypes.sizeof(m.FrameSsim)}))
    x, y = a.astype(np.int64), b.astype(np.int64)
    q = sm.window_q(x.sum(1), y.sum(1), (x * x + y * y).sum(1), (x * y).sum(1), 8)
    assert np.array_equal(got["q32"][:, 0], q) and not got["q32"][:, 1:].any()
    assert (got["nwin"][:, 0] == 1).all() and not got["nwin"][:, 1:].any()
    assert np.all(np.abs(got["all"] - q / 4294967296.0) <= 1e-12) and np.isnan(got["ssim"][:, 1:]).all()


def check_jobs(orc):
    import streams
    cs422 = streams._enc((140, 52, 3, 10, 12, 20, (1, 2, 2), (1, 1, 1)), depth=10, dx=[1, 2, 2], dy=[1, 1, 1], width=140, height=52,
                         nlevels=2)
    for cs, fmt in ((streams.get("rgb_mct")[0], "rgb24"), (cs422, "yuv422p10le")):
        dec = m.Decoder(device_id=0, req_pix_fmt=m.PIX_NAMES.index(fmt))
        info, oplanes, _ = orc.decode(cs, req_pix_fmt=m.PIX_NAMES.index(fmt))
        bits = info.bits_per_raw_sample
        job = dec.job().parse_batch([cs, cs]).upload().run()
        assert m.PIX_NAMES[job.frame_info(0).pix_fmt] == fmt
        nwin = [max((cw >> 2) - 1, 0) * max((ch >> 2) - 1, 0) for cw, ch in cm.comp_dims(fmt, info.width, info.height)] + [0] * 4
        got = job.compare_ssim([oplanes, oplanes])
        assert all(g["nwin"] == nwin[:4] and g["q32"] == [n << 32 for n in nwin[:4]] and g["all"] == 1.0 for g in got), got
        rng = np.random.default_rng(41)
        ref = [np.where(rng.random(p.shape) < 0.7, p, rng.integers(0, 1 << bits, size=p.shape)).astype(p.dtype) for p in oplanes]
        got = job.compare_ssim([oplanes, ref])
        want = sm.ssim(oplanes, ref, fmt, bits)
        assert sm.same(got[1], want) and got[0]["all"] == 1.0 and want["all"] < 1.0, (got, want)
        assert identical(job.compare_ssim([oplanes, ref], bits=bits), got)
        assert identical(dec.compare_ssim([job.device_frame(0), job.device_frame(1)], [oplanes, ref], fmt, bits, on_device=(True, False)), got)
        # a run without the pack stage is refused; the next full run answers again
        job.run(stages=1)
        with pytest.raises(m.Htj2kError) as e:
            job.compare_ssim([oplanes, ref])
        assert e.value.code == -22
        job.run()
        assert identical(job.compare_ssim([oplanes, ref]), got)
        with pytest.raises(m.Htj2kError) as e:
            job.compare_ssim([oplanes, ref], bits=3)
        assert e.value.code == -22
        # a batch with a frame that does not parse is refused as a whole (htj2k_job_parse_batch): there is no job to ask
        with pytest.raises(m.Htj2kError):
            job.parse_batch([cs, b"\x00\x01garbage" * 9])
        arr, keep = m._frame_array([oplanes, ref], m.PIX_NAMES.index(fmt))
        assert dec.L.htj2k_job_compare_ssim(dec.h, job.h, arr, 0, 0, (m.FrameSsim * 2)()) == -22
        job.free()
        dec.close()


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,bits,w,h,ls_mode,off", CASES)
def test_layouts_widths_and_heights(dec, fmt, bits, w, h, ls_mode, off):
    check_case(dec, fmt, bits, w, h, ls_mode, off, seed=w * 7 + h)


@pytest.mark.gpu
def test_every_layout_width_and_kernel_occurs():
    assert {c[4] for c in CASES} == set(LS_MODES) and {c[5] for c in CASES} == set(OFFSETS)
    assert {(c[0], c[1]) for c in CASES} == set(LAYOUTS) and {c[3] for c in CASES} == set(HEIGHTS)
    assert {(kernel_of(c[0]), c[2]) for c in CASES} == {(k, w) for k in {kernel_of(f) for f, _ in LAYOUTS} for w in WIDTHS}
    assert len({kernel_of(f) for f, _ in LAYOUTS}) == 8


@pytest.mark.gpu
def test_small_chroma(dec):
    check_small_chroma(dec)


@pytest.mark.gpu
def test_strip_seams(dec):
    check_strips(dec)


@pytest.mark.gpu
def test_contents(dec):
    check_contents(dec)


@pytest.mark.gpu
def test_one_window_divides_as_numpy_does(dec):
    check_division(dec)


@pytest.mark.gpu
def test_batches(dec):
    check_batches(dec)


@pytest.mark.gpu
def test_more_frames_than_one_launch_takes(dec):
    check_many_frames(dec)


@pytest.mark.gpu
def test_jobs(orc):
    check_jobs(orc)


@pytest.mark.gpu
@pytest.mark.parametrize("loop", [False, True])
def test_measured_encodes(dec, loop):
    """streams and EncMeasured are those of the call without the switch; info["ssim"] is the model's on the input against
    Decoder.decode of the final stream"""
    from test_encode_measured_gpu import case, decoded
    enc, decs = m.Encoder(0), {}
    try:
        fi, si = (0, 2) if loop else (0, 0)                  # 5/3 with the RCT measures short of 44 dB after round 1
        fmt, bits, planes, opts = case(fi, si)
        fmt2, bits2, planes2, _ = case(fi, si, seed=9)
        frames = [planes, planes2]
        kw = dict(close_loop=True, target_psnr=44.0) if loop else {}
        off_s, off_i = enc.encode_measured(dec, frames, fmt, bits, **kw, **opts)
        with pytest.raises(m.Htj2kError) as e:                 # the last call had the switch off
            enc.last_ssim(0)
        assert e.value.code == -22
        on_s, on_i = enc.encode_measured(dec, frames, fmt, bits, ssim=True, **kw, **opts)
        assert on_s == off_s
        assert [{k: v for k, v in i.items() if k != "ssim"} for i in on_i] == off_i and all("ssim" not in i for i in off_i)
        for f, (cs, info) in enumerate(zip(on_s, on_i)):
            want = sm.ssim(frames[f], decoded(decs, fmt, cs), fmt, bits)
            assert sm.same(info["ssim"], want) and identical(info["ssim"], enc.last_ssim(f)), (f, info, want)
            assert info["diff"]["psnr"] < math.inf and want["all"] < 1.0          # lossy
            print("measured", fmt, "loop" if loop else "report", f, "%.3f dB" % info["diff"]["psnr"], "ssim %.6f" % want["all"],
                  "rounds", info["rounds"])
        with pytest.raises(m.Htj2kError) as e:
            enc.last_ssim(2)
        assert e.value.code == -22
        enc.encode_batch([planes], fmt, bits, **opts)          # any other call forgets the figures
        with pytest.raises(m.Htj2kError):
            enc.last_ssim(0)
        L = enc.L
        assert L.htj2k_enc_measure_ssim(enc.h, 2) == -22 and L.htj2k_enc_measure_ssim(enc.h, -1) == -22
    finally:
        enc.close()
        for d in decs.values():
            d.close()


def run_everything(dec):
    for fmt, bits, w, h, ls_mode, off in CASES:
        check_case(dec, fmt, bits, w, h, ls_mode, off, seed=w * 7 + h)
    check_small_chroma(dec)
    check_strips(dec)
    check_contents(dec)
    check_division(dec)
    check_batches(dec)
    check_many_frames(dec)


POISON_TIMEOUT = 120


@pytest.mark.gpu
def test_everything_on_poisoned_buffers():
    """HTJ2K_POISON=1 (read once per process, so a fresh child): every new device buffer starts as 0xA5 bytes, and the
    sweeps must still give the model's results"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=POISON_TIMEOUT,
                       env=dict(os.environ, HTJ2K_POISON="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "poisoned buffers: ok" in r.stdout, r.stdout[-3000:]


if __name__ == "__main__":
    t0 = time.time()
    _dec = m.Decoder(device_id=0)
    run_everything(_dec)
    _dec.close()
    print("%s buffers: ok, %.1f s" % ("poisoned" if os.environ.get("HTJ2K_POISON") == "1" else "plain", time.time() - t0))
