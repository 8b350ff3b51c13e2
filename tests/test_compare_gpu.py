"""htj2k_compare_frames / htj2k_job_compare on the GPU against the numpy model (cmp_model): every integer for equality,
psnr to 1e-9 dB.

Layouts and depths x widths at the tails of the 16-byte and 48-byte groups x odd heights (a seeded subset), linesizes equal
to the row, row + 1, row + 13 and rounded to 64, base pointers off by 0, 1, 2 and 15 bytes on host and on device
operands, padding and the bits outside the sample filled with dirt that differs between the two operands, the extremes of
the sums, batches (sizes that differ, all four host / device combinations, more frames than grid.z takes) and jobs.
Run as a program, the module runs all of it on its own contexts: test_everything_on_poisoned_buffers does that in a child
process under HTJ2K_POISON=1."""
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

LAYOUTS = [("gray", 8), ("ya8", 8), ("rgb24", 8), ("rgba", 8), ("gray16le", 16), ("ya16le", 16), ("rgb48le", 16), ("rgb48le", 12),
           ("yuv420p", 8), ("yuv422p10le", 10), ("yuv422p10le", 9), ("yuva444p16le", 16), ("xyz12le", 12)]
WIDTHS = [1, 3, 15, 16, 17, 47, 48, 49, 63, 65, 257]
HEIGHTS = [1, 2, 5]
LS_MODES = ["row", "row+1", "row+13", "to64"]
OFFSETS = [0, 1, 2, 15]


def _cases():
    full = [(f, b, w, h) for f, b in LAYOUTS for w in WIDTHS for h in HEIGHTS]
    picked = random.Random(20).sample(full, 140)
    # every layout at every width at least once, whatever the draw
    have = {(f, b, w) for f, b, w, _ in picked}
    picked += [(f, b, w, HEIGHTS[(i + len(f)) % 3]) for i, (f, b) in enumerate(LAYOUTS) for w in WIDTHS if (f, b, w) not in have]
    return [(f, b, w, h, LS_MODES[i % 4], OFFSETS[(i // 4) % 4]) for i, (f, b, w, h) in enumerate(picked)]


CASES = _cases()
assert len(CASES) < 200


class Operand:
    """one frame in host memory with a linesize and a base offset of its own: every byte of its buffers is dirt except
    the `bits` bits of each sample"""

    def __init__(self, fmt, w, h, bits, rng, ls_mode="row", off=0, values=None):
        self.fmt, self.w, self.h, self.bits = fmt, w, h, bits
        self.bytes = cm.LAYOUTS[fmt][5]
        self.dt = np.uint8 if self.bytes == 1 else np.uint16
        self.off = off
        self.bufs, self.ls, self.shapes = [], [], cm.plane_shapes(fmt, w, h)
        for p, (rows, cols) in enumerate(self.shapes):
            row = cols * self.bytes
            ls = {"row": row, "row+1": row + 1, "row+13": row + 13, "to64": -(-row // 64) * 64}[ls_mode]
            self.ls.append(ls)
            self.bufs.append(rng.integers(0, 256, size=off + ls * rows + 16, dtype=np.uint8))
        self.values = values if values is not None else [rng.integers(0, 1 << bits, size=s).astype(np.int64) for s in self.shapes]
        self.write(rng)

    def write(self, rng):
        """the samples into the buffers, fresh dirt in the bits below the shift and above the sample"""
        sh, top = cm.shift(self.fmt, self.bits), 8 * self.bytes
        for p, (rows, cols) in enumerate(self.shapes):
            word = self.values[p] << sh
            if sh:
                word |= rng.integers(0, 1 << sh, size=word.shape)
            if sh + self.bits < top:
                word |= rng.integers(0, 1 << (top - sh - self.bits), size=word.shape) << (sh + self.bits)
            raw = word.astype("<u%d" % self.bytes).view(np.uint8).reshape(rows, cols * self.bytes)
            for y in range(rows):
                at = self.off + y * self.ls[p]
                self.bufs[p][at:at + cols * self.bytes] = raw[y]

    def dirty_padding(self, rng):
        keep = self.raw_planes()
        for p, (rows, cols) in enumerate(self.shapes):
            self.bufs[p][:] = rng.integers(0, 256, size=self.bufs[p].size, dtype=np.uint8)
            for y in range(rows):
                at = self.off + y * self.ls[p]
                self.bufs[p][at:at + cols * self.bytes] = keep[p][y].view(np.uint8)

    def raw_planes(self):
        """the words as they lie in memory, dirt in their unused bits included: what the model is given"""
        out = []
        for p, (rows, cols) in enumerate(self.shapes):
            n = cols * self.bytes
            rowsb = [self.bufs[p][self.off + y * self.ls[p]: self.off + y * self.ls[p] + n] for y in range(rows)]
            out.append(np.stack(rowsb).copy().view("<u%d" % self.bytes))
        return out

    def frame(self, bases=None):
        fr = m.Frame()
        for p in range(len(self.shapes)):
            fr.data[p] = (self.bufs[p].ctypes.data if bases is None else bases[p]) + self.off
            fr.linesize[p] = self.ls[p]
        fr.width, fr.height, fr.pix_fmt = self.w, self.h, m.PIX_NAMES.index(self.fmt)
        return fr

    def on_device(self):
        """(frame of device addresses, tensors to keep): the same bytes, dirt and offset on the device"""
        ts = [torch.from_numpy(b).cuda() for b in self.bufs]
        torch.cuda.synchronize()
        return self.frame([t.data_ptr() for t in ts]), ts


def pair(fmt, w, h, bits, seed, ls_a="row", off_a=0, ls_b="row", off_b=0):
    """two operands of one geometry: about half of b's samples are a's"""
    rng = np.random.default_rng(seed)
    a = Operand(fmt, w, h, bits, rng, ls_a, off_a)
    vb = [np.where(rng.random(v.shape) < 0.5, v, rng.integers(0, 1 << bits, size=v.shape)) for v in a.values]
    b = Operand(fmt, w, h, bits, rng, ls_b, off_b, values=vb)
    return a, b


def model(a, b):
    return cm.compare(a.raw_planes(), b.raw_planes(), a.fmt, a.bits)


def check_case(dec, fmt, bits, w, h, ls_mode, off, seed):
    # the two operands differ in everything that must not matter: linesize, offset, dirt
    a, b = pair(fmt, w, h, bits, seed, ls_mode, off, LS_MODES[(LS_MODES.index(ls_mode) + 1) % 4], OFFSETS[(OFFSETS.index(off) + 1) % 4])
    want = model(a, b)
    got = dec.compare([a.frame()], [b.frame()], fmt, bits)[0]
    assert cm.same(got, want), (fmt, bits, w, h, ls_mode, off, got, want)
    # device operands at the same offsets: the planes are read in place, on the narrower path where they are not aligned
    (fa, ka), (fb, kb) = a.on_device(), b.on_device()
    got = dec.compare([fa], [fb], fmt, bits, on_device=(True, True))[0]
    assert cm.same(got, want), ("device", fmt, bits, w, h, ls_mode, off, got, want)
    # fresh dirt in the padding and outside the samples changes nothing
    rng = np.random.default_rng(seed + 1)
    a.write(rng)
    a.dirty_padding(rng)
    b.dirty_padding(rng)
    assert cm.same(dec.compare([a.frame()], [b.frame()], fmt, bits)[0], want), ("dirt", fmt, bits, w, h)


def check_extremes(dec):
    w, h = 300, 220
    zero, full = np.zeros((h, w), np.uint16), np.full((h, w), 65535, np.uint16)
    got = dec.compare([[zero]], [[full]], "gray16le", 16)[0]
    assert got["sse"] == [w * h * 65535 * 65535, 0, 0, 0] and got["sse"][0] > (1 << 47)      # no 32-bit lane sum holds two samples
    assert got["ndiff"] == [w * h, 0, 0, 0] and got["max_abs"] == [65535, 0, 0, 0] and got["nsamples"] == [w * h, 0, 0, 0]
    assert abs(got["psnr"]) < 1e-9 and cm.same(got, cm.compare([zero], [full], "gray16le", 16))
    for fmt, bits in LAYOUTS:
        a, _ = pair(fmt, 49, 5, bits, 3, "row+13", 1)
        b = Operand(fmt, 49, 5, bits, np.random.default_rng(4), "to64", 0, values=a.values)   # other dirt, the same samples
        got = dec.compare([a.frame()], [b.frame()], fmt, bits)[0]
        nc = cm.LAYOUTS[fmt][0]
        assert got["sse"] == [0] * 4 and got["ndiff"] == [0] * 4 and got["max_abs"] == [0] * 4 and got["psnr"] == math.inf
        assert got["nsamples"] == [cw * ch for cw, ch in cm.comp_dims(fmt, 49, 5)] + [0] * (4 - nc)


def check_batches(dec):
    for fmt, bits in (("rgb24", 8), ("yuv422p10le", 10), ("rgb48le", 12)):
        ps = [pair(fmt, w, h, bits, 10 + i, LS_MODES[i], OFFSETS[i], LS_MODES[3 - i], OFFSETS[3 - i])
              for i, (w, h) in enumerate([(65, 5), (17, 2), (257, 3)])]
        want = [model(a, b) for a, b in ps]
        host_a, host_b = [a.frame() for a, _ in ps], [b.frame() for _, b in ps]
        da, db = [a.on_device() for a, _ in ps], [b.on_device() for _, b in ps]
        dev_a, dev_b = [f for f, _ in da], [f for f, _ in db]
        for on_a, on_b in ((False, False), (True, False), (False, True), (True, True)):
            got = dec.compare(dev_a if on_a else host_a, dev_b if on_b else host_b, fmt, bits, on_device=(on_a, on_b))
            assert len(got) == 3 and all(cm.same(g, w) for g, w in zip(got, want)), (fmt, on_a, on_b, got, want)
        assert dec.compare_ms() > 0
        # a batch of two layouts, and a frame of another size than its partner, are refused
        with pytest.raises(m.Htj2kError) as e:
            dec.compare(host_a[:2], [host_b[0], host_b[2]], fmt, bits)
        assert e.value.code == -22


def check_many_frames(dec, n=70000):
    """more pairs than grid.z takes in one launch: 3 x 2 gray frames out of two buffers"""
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, size=(n, 6), dtype=np.uint8)
    b = np.where(rng.random((n, 6)) < 0.5, a, rng.integers(0, 256, size=(n, 6), dtype=np.uint8)).astype(np.uint8)
    rec = np.dtype({"names": ["data", "linesize", "width", "height", "pix_fmt"], "formats": [("<u8", 4), ("<i4", 4), "<i4", "<i4", "<i4"],
                    "offsets": [0, 32, 48, 52, 56], "itemsize": ctypes.sizeof(m.Frame)})
    tabs = []
    for x in (a, b):
        t = np.zeros(n, rec)
        t["data"][:, 0] = x.ctypes.data + 6 * np.arange(n, dtype=np.uint64)
        t["linesize"][:, 0] = 3
        t["width"], t["height"], t["pix_fmt"] = 3, 2, m.PIX_NAMES.index("gray")
        tabs.append(t)
    out = (m.FrameDiff * n)()
    t0 = time.time()
    r = dec.L.htj2k_compare_frames(dec.h, tabs[0].ctypes.data_as(ctypes.c_void_p), 0, tabs[1].ctypes.data_as(ctypes.c_void_p), 0,
                                   n, 8, out)
    took = time.time() - t0
    assert r == 0
    got = np.frombuffer(out, np.dtype({"names": ["sse", "ndiff", "nsamples", "max_abs", "psnr"],
                                       "formats": [("<u8", 4), ("<u8", 4), ("<u8", 4), ("<u4", 4), "<f8"],
                                       "offsets": [0, 32, 64, 96, 112], "itemsize": ctypes.sizeof(m.FrameDiff)}))
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    sse = (d * d).sum(1)
    assert np.array_equal(got["sse"][:, 0], sse.astype(np.uint64)) and not got["sse"][:, 1:].any()
    assert np.array_equal(got["ndiff"][:, 0], (d != 0).sum(1).astype(np.uint64)) and np.array_equal(got["max_abs"][:, 0], d.max(1).astype(np.uint32))
    assert (got["nsamples"][:, 0] == 6).all() and not got["nsamples"][:, 1:].any()
    with np.errstate(divide="ignore"):
        want = np.where(sse == 0, np.inf, 10 * np.log10(255.0 * 255.0 * 6.0 / np.maximum(sse, 1)))
    assert np.array_equal(np.isinf(got["psnr"]), sse == 0) and np.all(np.abs(got["psnr"][sse > 0] - want[sse > 0]) < 1e-9)
    return took


def decoded_job(dec, enc, fmt, bits, sizes, seed):
    """(job after a full run, the frames that went in): lossless streams of the encoder, so the job's planes are the input"""
    rng = np.random.default_rng(seed)
    sh = cm.shift(fmt, bits)
    dt = np.uint8 if cm.LAYOUTS[fmt][5] == 1 else np.uint16
    frames = [[(rng.integers(0, 1 << bits, size=s) << sh).astype(dt) for s in cm.plane_shapes(fmt, w, h)] for w, h in sizes]
    streams = enc.encode_batch(frames, fmt, bits, levels=2)
    job = dec.job().parse_batch(streams).upload().run()
    return job, frames


def check_jobs(enc):
    for fmt, bits in (("rgb24", 8), ("yuv422p10le", 10), ("gray16le", 16)):
        dec = m.Decoder(device_id=0, req_pix_fmt=m.PIX_NAMES.index(fmt))
        sizes = [(65, 5), (17, 3), (48, 2), (257, 5), (1, 1)]
        job, frames = decoded_job(dec, enc, fmt, bits, sizes, 30)
        rng = np.random.default_rng(31)
        ref = [[np.where(rng.random(p.shape) < 0.7, p, rng.integers(0, 1 << bits, size=p.shape) << cm.shift(fmt, bits)).astype(p.dtype)
                for p in f] for f in frames]
        got = job.compare(ref)
        down = [job.download_frame(f)[1] for f in range(len(sizes))]
        assert all(np.array_equal(x, y) for f, g in zip(down, frames) for x, y in zip(f, g))
        assert got == dec.compare(down, ref, fmt, bits) == job.compare(ref, bits=bits)
        assert all(cm.same(g, cm.compare(d, r, fmt, bits)) for g, d, r in zip(got, down, ref))
        assert all(g["psnr"] == math.inf for g in job.compare(frames))
        # device operands off by 0, 1, 2 and 15 bytes inside the row: the job's planes, read in place.  Whatever the
        # layout, the rest of the rows of plane 0 is a gray frame of bytes; under rgb24 15 bytes are five pixels
        f = 3
        fr, info = job.device_frame(f), job.frame_info(f)
        rowb = info.plane_width[0] * info.plane_bytes_per_sample[0]
        for off in OFFSETS:
            sub = m.Frame.from_buffer_copy(fr)
            sub.data[0], sub.width, sub.pix_fmt = fr.data[0] + off, rowb - off, m.PIX_NAMES.index("gray")
            hostp = [np.ascontiguousarray(down[f][0].view(np.uint8)[:, off:])]
            refp = [np.ascontiguousarray(ref[f][0].view(np.uint8)[:, off:])]
            for bb in (8, 5):
                one = dec.compare([sub], [refp], "gray", bb, on_device=(True, False))[0]
                assert cm.same(one, cm.compare(hostp, refp, "gray", bb)), (fmt, off, bb)
            if fmt == "rgb24" and off % 3 == 0:
                sub.width, sub.pix_fmt = info.width - off // 3, info.pix_fmt
                one = dec.compare([[p[:, off:] for p in ref[f]]], [sub], fmt, bits, on_device=(False, True))[0]
                assert cm.same(one, cm.compare([p[:, off:] for p in ref[f]], [p[:, off:] for p in down[f]], fmt, bits)), (fmt, off)
        # a run that did not write the frames is refused; the next full run is compared again
        job.run(stages=1)
        with pytest.raises(m.Htj2kError) as e:
            job.compare(ref)
        assert e.value.code == -22
        job.run()
        assert all(cm.same(g, cm.compare(d, r, fmt, bits)) for g, d, r in zip(job.compare(ref), down, ref))
        with pytest.raises(m.Htj2kError) as e:
            job.compare([[p[:, :-1] for p in fr_] for fr_ in ref])          # another size than the job's frames
        assert e.value.code == -22
        job.free()
        dec.close()


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def enc():
    e = m.Encoder(device_id=0)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,bits,w,h,ls_mode,off", CASES)
def test_layouts_rows_and_bases(dec, fmt, bits, w, h, ls_mode, off):
    check_case(dec, fmt, bits, w, h, ls_mode, off, seed=w * 7 + h)


@pytest.mark.gpu
def test_every_row_layout_and_offset_occurs():
    assert {c[4] for c in CASES} == set(LS_MODES) and {c[5] for c in CASES} == set(OFFSETS)
    assert {(c[0], c[1], c[2]) for c in CASES} == {(f, b, w) for f, b in LAYOUTS for w in WIDTHS}


@pytest.mark.gpu
def test_extremes(dec):
    check_extremes(dec)


@pytest.mark.gpu
def test_batches(dec):
    check_batches(dec)


@pytest.mark.gpu
def test_more_frames_than_one_launch_takes(dec):
    check_many_frames(dec)


@pytest.mark.gpu
def test_jobs(enc):
    check_jobs(enc)


def run_everything(dec, enc):
    for fmt, bits, w, h, ls_mode, off in CASES:
        check_case(dec, fmt, bits, w, h, ls_mode, off, seed=w * 7 + h)
    check_extremes(dec)
    check_batches(dec)
    check_many_frames(dec)
    check_jobs(enc)


POISON_TIMEOUT = 120


@pytest.mark.gpu
def test_everything_on_poisoned_buffers():
    """HTJ2K_POISON=1 (read once per process, so a fresh child): every new device buffer starts as 0xA5 bytes, and all of
    the above must still give the model's results"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=POISON_TIMEOUT,
                       env=dict(os.environ, HTJ2K_POISON="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "poisoned buffers: ok" in r.stdout, r.stdout[-3000:]


if __name__ == "__main__":
    t0 = time.time()
    _dec, _enc = m.Decoder(device_id=0), m.Encoder(device_id=0)
    run_everything(_dec, _enc)
    _dec.close()
    _enc.close()
    print("%s buffers: ok, %.1f s" % ("poisoned" if os.environ.get("HTJ2K_POISON") == "1" else "plain", time.time() - t0))
