"""htj2k_resize_frames / htj2k_job_resize_frames / htj2k_pipe_receive_resized on the GPU against the numpy model
(resize_frames_model): every byte of every destination plane between 0xC3 guard zones, with no tolerance.

Fifteen layouts under three filters down, up and at one pixel; outputs at the tile's width and height and around them
under every chroma shift; the most taps an axis can have; sample bits below the precision with dirt around the sample;
odd bases and odd linesizes on both sides; the knobs resize_rows and resize_share; constants, peaks and the identity;
unlike frames in one call and more planes than grid.z takes; the tensor route beside it; jobs, pipes, a proxy encoded and
decoded again; every refusal on a live context.  Run as a program, the module runs all of it on its own contexts:
test_everything_on_poisoned_buffers does that in a child process under HTJ2K_POISON=1."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: device operands and destinations are made through it)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [HERE, ROOT]

import cmp_model as cm
import ffmpeg_ht_amd as m
import oracle
import resize_frames_model as fm
import streams
from test_hash_gpu import HFrame, damaged_copy
from test_tensor_gpu import bounded, yuv422p10_stream

LAYOUTS = ["gray", "ya8", "rgb24", "rgba", "rgb48le", "rgba64le", "gray16le", "yuv410p", "yuv411p", "yuv420p", "yuv440p", "yuva420p",
           "yuv422p10le", "yuv444p12le", "xyz12le"]
LS_MODES = ["row", "row+1", "row+13", "to64"]
OFFSETS = [0, 1, 2, 15]
FILTERS = [fm.NEAREST, fm.BILINEAR, fm.TRIANGLE]
EINVAL, PATCHWELCOME = -22, -0x45574150
GUARD, FILL = 256, 0xC3
TILE_W, TILE_H = 32, 16                                  # RS_TW, RS_TH of csrc/resize_kernels.hpp
CALLS = {"n": 0}


class DFrame:
    """one destination frame in device memory: every plane in a buffer of 0xC3 bytes with a guard zone at either end, a
    base offset and a linesize of its own"""

    def __init__(self, fmt, w, h, ls_mode="row", off=0):
        self.fmt, self.w, self.h, self.off = fmt, w, h, off
        _, _, rows, rowbytes = m.Decoder.plane_sizes(fmt, w, h)
        self.geo = list(zip(rows, rowbytes))
        self.ls = [{"row": rb, "row+1": rb + 1, "row+13": rb + 13, "to64": -(-rb // 64) * 64}[ls_mode] for _, rb in self.geo]
        self.bufs = [torch.full((2 * GUARD + off + ls * r,), FILL, dtype=torch.uint8, device="cuda") for (r, _), ls in zip(self.geo, self.ls)]

    def frame(self):
        fr = m.Frame()
        for p, b in enumerate(self.bufs):
            fr.data[p] = b.data_ptr() + GUARD + self.off
            fr.linesize[p] = self.ls[p]
        fr.width, fr.height, fr.pix_fmt = self.w, self.h, m.PIX_NAMES.index(self.fmt)
        return fr

    def untouched(self):
        return all(bool((b == FILL).all()) for b in self.bufs)

    def check(self, want, what):
        """every byte: the model's samples where a row has samples, 0xC3 everywhere else"""
        for p, ((rows, rb), ls, b) in enumerate(zip(self.geo, self.ls, self.bufs)):
            host = b.cpu().numpy()
            expect = np.full(host.size, FILL, np.uint8)
            w8 = np.ascontiguousarray(want[p]).view(np.uint8).reshape(rows, rb)
            for y in range(rows):
                at = GUARD + self.off + y * ls
                expect[at:at + rb] = w8[y]
            bad = np.flatnonzero(host != expect)
            assert bad.size == 0, (what, p, len(bad), bad[:6].tolist(), host[bad[:6]].tolist(), expect[bad[:6]].tolist())


def windows_array(windows):
    return None if windows is None else (ctypes.c_int32 * (4 * len(windows)))(*[int(v) for w in windows for v in w])


def raw_call(dec, sarr, on_device, n, bits, windows, filt, darr):
    torch.cuda.synchronize()
    return dec.L.htj2k_resize_frames(dec.h, sarr, int(on_device), n, int(bits), windows_array(windows), int(filt), darr)


def check(dec, frames, fmt, bits, size, windows=None, filt=fm.TRIANGLE, on_device=False, dst_ls="row", dst_off=0, want=None):
    """one call against the model, every byte of every destination buffer -> the destination frames"""
    n = len(frames)
    if want is None:
        want = fm.batch([f.arrays() for f in frames], fmt, bits, size, windows, filt)
    keep = []
    if on_device:
        made = [f.on_device() for f in frames]
        keep = [k for _, k in made]
        sarr = (m.Frame * n)(*[fr for fr, _ in made])
    else:
        sarr = (m.Frame * n)(*[f.frame() for f in frames])
    dst = [DFrame(fmt, size[0], size[1], dst_ls, dst_off) for _ in range(n)]
    darr = (m.Frame * n)(*[d.frame() for d in dst])
    what = (fmt, bits, size, windows, filt, on_device, dst_ls, dst_off, [(f.w, f.h, f.ls, f.off) for f in frames[:4]])
    r = raw_call(dec, sarr, on_device, n, bits, windows, filt, darr)
    assert r == 0, (r, what)
    for i, d in enumerate(dst):
        d.check(want[i], what + (i,))
    CALLS["n"] += 1
    del keep
    return dst


def low_bits(fmt):
    return {"rgb48le": 12, "rgba64le": 11, "yuv422p10le": 9}.get(fmt, cm.LAYOUTS[fmt][4] - 1)


def check_layout(dec, fmt, li):
    """three filters on 37 x 23 to 16 x 9 and to 75 x 50, 1 x 1 to 4 x 4 and 4 x 4 to 1 x 1; host and device sources, every
    linesize and base on both sides; every other call at fewer bits than the layout's, the source's other bits dirty"""
    depth = cm.LAYOUTS[fmt][4]
    k = 0
    for ci, ((w, h), size) in enumerate((((37, 23), (16, 9)), ((37, 23), (75, 50)), ((1, 1), (4, 4)), ((4, 4), (1, 1)))):
        for filt in FILTERS:
            k += 1
            f = HFrame(fmt, w, h, np.random.default_rng(100 * li + k), LS_MODES[(li + k) % 4], OFFSETS[(li + 2 * k) % 4])
            check(dec, [f], fmt, low_bits(fmt) if k % 2 else depth, size, None, filt, k % 3 != 0, LS_MODES[(li + k + 1) % 4], OFFSETS[(k + li // 2) % 4])


def check_seams(dec):
    """outputs at the tile's size, one below and one above, in luma and -- at two and four times the size -- in chroma"""
    rng = np.random.default_rng(31)
    for fi, (fmt, (w, h)) in enumerate((("rgb24", (70, 40)), ("yuv420p", (19, 11)), ("yuv410p", (50, 37)), ("yuv411p", (47, 9)), ("yuv440p", (21, 45)),
                                       ("yuv422p10le", (40, 20)))):
        f = HFrame(fmt, w, h, rng, "row+1", 1)
        depth = cm.LAYOUTS[fmt][4]
        for ow in (TILE_W - 1, TILE_W, TILE_W + 1):
            for oh in (TILE_H, TILE_H + 1):
                check(dec, [f], fmt, depth, (ow, oh), None, FILTERS[(ow + oh + fi) % 3], oh % 2, "row+13", 1)
        sw, sh = max(fm.plane_shifts(fmt))
        if sw or sh:                                         # the chroma planes' own seams, odd sizes among them
            for ow in ((TILE_W << sw) - 1, (TILE_W << sw) + 1):
                for oh in ((TILE_H << sh) - 1, (TILE_H << sh) + 1):
                    check(dec, [f], fmt, depth, (ow, oh), None, FILTERS[(ow + oh) % 3], True, "row+1", 2)


def check_taps(dec):
    """1024 x 4 to 16 x 4 and 16 x 1024 to 16 x 16: 128 taps an axis, the most there are"""
    import resize_model as rm
    assert max(len(rm.weights(1024, 16, rm.TRIANGLE, x)[1]) for x in range(16)) == 128
    rng = np.random.default_rng(32)
    for fmt in ("gray", "rgb48le", "yuv420p"):
        check(dec, [HFrame(fmt, 1024, 4, rng, "to64")], fmt, cm.LAYOUTS[fmt][4], (16, 4), None, fm.TRIANGLE, True)
        check(dec, [HFrame(fmt, 16, 1024, rng, "row+1", 1)], fmt, cm.LAYOUTS[fmt][4], (16, 16), None, fm.TRIANGLE, False, "row+1", 1)


def check_alignment(dec):
    """two-byte layouts on odd bases and odd linesizes, source and destination, each side alone and both"""
    rng = np.random.default_rng(33)
    for fmt in ("gray16le", "rgb48le", "rgba64le", "yuv422p10le", "xyz12le"):
        for src_ls, src_off, dst_ls, dst_off in (("row+1", 1, "row", 0), ("row", 0, "row+1", 1), ("row+13", 15, "row+13", 1), ("row+1", 0, "row", 1),
                                                 ("to64", 1, "to64", 2)):
            f = HFrame(fmt, 35, 9, rng, src_ls, src_off)
            for k, size in enumerate(((13, 5), (41, 12))):
                check(dec, [f], fmt, cm.LAYOUTS[fmt][4], size, None, FILTERS[1 + k], True, dst_ls, dst_off)


def check_knobs(dec):
    """resize_rows and resize_share never show in the bytes"""
    rng = np.random.default_rng(34)
    cases = [("yuv422p10le", HFrame("yuv422p10le", 50, 41, rng, "row+13", 15), 10, (13, 9), None),
             ("rgb24", HFrame("rgb24", 256, 21, rng, "row+1", 1), 8, (10, 7), None),
             ("yuv420p", HFrame("yuv420p", 64, 40, rng), 8, (70, 33), [(2, 4, 40, 31)])]
    for fmt, f, bits, size, windows in cases:
        want = fm.batch([f.arrays()], fmt, bits, size, windows, fm.TRIANGLE)
        for knob, values in (("resize_rows", (1, 3, 8, 16)), ("resize_share", (1, 2, 3, 4, 5, 6))):
            for v in values:
                dec.set_int(knob, v)
                try:
                    check(dec, [f], fmt, bits, size, windows, fm.TRIANGLE, True, want=want)
                finally:
                    dec.set_int(knob, 0)
    assert 41 % 3 == 2 and 41 % 8 == 1                       # steps that leave odd rows


def check_invariants(dec):
    """constants stay constant and the peak stays the peak; ww = out_w and wh = out_h is a crop of every plane"""
    rng = np.random.default_rng(35)
    for fmt, value in (("gray16le", 0xFF), ("gray16le", 0), ("rgb24", 0xFF), ("yuv420p", 0x80)):
        f = HFrame(fmt, 130, 70, rng, "to64", 0, value=value)
        for filt in FILTERS:
            for size in ((3, 2), (131, 71), (40, 70)):
                for d in check(dec, [f], fmt, cm.LAYOUTS[fmt][4], size, None, filt, True):
                    for b, (rows, rb), ls in zip(d.bufs, d.geo, d.ls):
                        host = b.cpu().numpy()
                        assert all((host[GUARD + y * ls: GUARD + y * ls + rb] == value).all() for y in range(rows))
    for i, fmt in enumerate(LAYOUTS):
        depth, st = cm.LAYOUTS[fmt][4], fm.step(fmt)
        f = HFrame(fmt, 45, 19, rng, LS_MODES[i % 4], OFFSETS[i % 4])
        for j, (window, filt) in enumerate((((0, 0, 45, 19), fm.TRIANGLE), ((8, 4, 33, 15), fm.BILINEAR), ((16, 8, 13, 5), fm.NEAREST))):
            crop, word_shift, mask = [], cm.shift(fmt, depth), (1 << depth) - 1
            for p, (sw, sh) in zip(f.arrays(), fm.plane_shifts(fmt)):
                px, py, pw, ph = fm.plane_window(window, sw, sh)
                part = p[py:py + ph, px * st:(px + pw) * st]
                crop.append(np.ascontiguousarray((((part >> word_shift) & mask) << word_shift).astype(p.dtype)))   # the samples; other bits zero
            check(dec, [f], fmt, depth, window[2:], [window], filt, (i + j) % 2, LS_MODES[(i + j) % 4], OFFSETS[(i + j + 1) % 4], want=[crop])


def check_batches(dec):
    """frames of four sizes with four windows and reductions in one call"""
    rng = np.random.default_rng(51)
    sizes = [(40, 10), (33, 42), (200, 7), (17, 9)]
    windows = [(8, 4, 24, 6), (0, 0, 33, 42), (4, 0, 192, 7), (16, 8, 1, 1)]
    for fmt, bits in (("rgb24", 8), ("yuv420p", 8), ("yuv410p", 7), ("yuv422p10le", 10), ("rgba64le", 16)):
        for on_device in (False, True):
            fs = [HFrame(fmt, w, h, rng, LS_MODES[i], OFFSETS[3 - i]) for i, (w, h) in enumerate(sizes)]
            for filt in FILTERS:
                check(dec, fs, fmt, bits, (12, 6), windows, filt, on_device, LS_MODES[filt], filt)
        check(dec, fs, fmt, bits, (5, 4), None, fm.TRIANGLE, True)      # each frame whole


def check_many_frames(dec, n=70000):
    """more planes than grid.z takes in one launch: 2 x 2 gray frames out of one buffer, each to 1 x 1 of another"""
    a = np.random.default_rng(9).integers(0, 256, size=(n, 2, 2), dtype=np.uint8)
    rec = np.dtype({"names": ["data", "linesize", "width", "height", "pix_fmt"], "formats": [("<u8", 4), ("<i4", 4), "<i4", "<i4", "<i4"],
                    "offsets": [0, 32, 48, 52, 56], "itemsize": ctypes.sizeof(m.Frame)})
    src, dst = np.zeros(n, rec), np.zeros(n, rec)
    out = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    src["data"][:, 0] = a.ctypes.data + 4 * np.arange(n, dtype=np.uint64)
    src["linesize"][:, 0] = 2
    src["width"], src["height"], src["pix_fmt"] = 2, 2, m.PIX_NAMES.index("gray")
    dst["data"][:, 0] = out.data_ptr() + GUARD + np.arange(n, dtype=np.uint64)
    dst["linesize"][:, 0] = 1
    dst["width"], dst["height"], dst["pix_fmt"] = 1, 1, m.PIX_NAMES.index("gray")
    want = (a.astype(np.int64).sum(axis=(1, 2)) * (1 << 26) + fm.HALF) >> fm.SHIFT       # four taps of 2^13 x 2^13
    assert np.array_equal(want[:8], [int(fm.frame([a[i]], "gray", 8, (1, 1))[0][0, 0]) for i in range(8)])
    r = raw_call(dec, src.ctypes.data_as(ctypes.c_void_p), 0, n, 8, None, fm.TRIANGLE, dst.ctypes.data_as(ctypes.c_void_p))
    assert r == 0
    host = out.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + n:] == FILL).all()
    assert np.array_equal(host[GUARD:GUARD + n], want.astype(np.uint8))


def check_tensor_route(dec):
    """layouts without sub-sampling: to_tensor_resized in float32 at scale 1 and bias 0 is the same sum before its
    rounding, so it differs from the sample by one integer rounding (0.5) plus one binary32 step at 65 535 (2^-8)"""
    rng = np.random.default_rng(52)
    for fmt in ("gray", "ya8", "rgb24", "rgba", "rgb48le", "rgba64le", "gray16le", "yuv444p12le", "xyz12le"):
        nc, planar, _, _, depth, _ = cm.LAYOUTS[fmt]
        f = HFrame(fmt, 37, 23, rng)
        planes = f.arrays()
        for size in ((16, 9), (75, 50)):
            for filt in FILTERS:
                want = fm.frame(planes, fmt, depth, size, None, filt)
                check(dec, [f], fmt, depth, size, None, filt, False, want=[want])        # the new samples are the model's
                t = dec.to_tensor_resized([planes], fmt, depth, size, None, m.RESIZE_FILTERS[filt], "float32", "NCHW", 1.0, 0.0).cpu().numpy()[0]
                got = cm.components(want, fmt, depth)
                for c in range(nc):
                    assert float(np.abs(t[c].astype(np.float64) - got[c]).max()) <= 0.5 + 2.0 ** -8, (fmt, size, filt, c)


def keep_planes(fmt, size, keep, i=0):
    """frame i of what the Python calls return, as the model's arrays"""
    _, _, rows, rowbytes = m.Decoder.plane_sizes(fmt, size[0], size[1])
    two = cm.LAYOUTS[fmt][5] == 2
    out = []
    for p, (r, rb) in enumerate(zip(rows, rowbytes)):
        a = keep[i * len(rows) + p].cpu().numpy().reshape(r, rb)
        out.append(a.view("<u2") if two else a)
    return out


def same_planes(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


def check_python(dec):
    """Decoder.resize_frames: numpy planes or device frames in, frames that the other calls take out"""
    rng = np.random.default_rng(12)
    fs = [HFrame("yuv420p", 33, 6, rng), HFrame("yuv420p", 20, 9, rng)]
    planes = [f.arrays() for f in fs]
    arr, keep = dec.resize_frames(planes, "yuv420p", 8, (9, 5))
    assert len(arr) == 2 and len(keep) == 6 and (arr[1].width, arr[1].height) == (9, 5) and dec.compare_ms() > 0
    want = fm.batch(planes, "yuv420p", 8, (9, 5))
    assert all(same_planes(keep_planes("yuv420p", (9, 5), keep, i), want[i]) for i in range(2))
    crc = dec.framecrc(arr, "yuv420p", on_device=True)
    assert [c["adler32"] for c in crc] == [c["adler32"] for c in dec.framecrc(want, "yuv420p")]
    assert all(d["sse"] == [0, 0, 0, 0] for d in dec.compare(arr, want, "yuv420p", 8, on_device=(True, False)))
    devs = [f.on_device() for f in fs]
    wins = [(2, 0, 30, 6), (4, 2, 10, 7)]
    arr2, keep2 = dec.resize_frames([d for d, _ in devs], "yuv420p", 7, (40, 11), wins, "bilinear", on_device=True)
    want = fm.batch(planes, "yuv420p", 7, (40, 11), wins, fm.BILINEAR)
    assert all(same_planes(keep_planes("yuv420p", (40, 11), keep2, i), want[i]) for i in range(2))
    for bad in (None, (0, 4), (4, -1)):
        with pytest.raises(ValueError):
            dec.resize_frames(planes, "yuv420p", 8, bad)
    with pytest.raises(ValueError):
        dec.resize_frames(planes, "yuv420p", 8, (4, 4), filter="lanczos")
    with pytest.raises(ValueError):
        dec.resize_frames(planes, "yuv420p", 8, (4, 4), windows=[(0, 0, 4, 4)] * 3)
    with pytest.raises(m.Htj2kError) as e:
        dec.resize_frames(planes, "yuv420p", 8, (4, 4), windows=(1, 0, 4, 4))
    assert e.value.code == EINVAL


def check_jobs(dec, orc):
    get = lambda name: streams.get(name)[0]
    groups = [("rgb24", [get("rgb_mct"), get("rgb_tiles")]), ("yuv420p", [get("yuv420p8"), get("yuv420p8")]),
              ("yuv422p10le", [yuv422p10_stream()] * 2), ("gray16le", [get("gray16")] * 2)]
    job = dec.job()
    for fmt, datas in groups:
        job.parse_batch(datas).upload()
        with pytest.raises(m.Htj2kError) as e:               # before the first run
            job.resized_frames((8, 8))
        assert e.value.code == EINVAL
        job.run()
        info = job.frame_info(0)
        assert m.PIX_NAMES[info.pix_fmt] == fmt
        bits = info.bits_per_raw_sample
        want_planes = [orc.decode(d)[1] for d in datas]
        arr, keep, status = job.resized_frames((24, 17))                                             # each frame whole, bits 0: the job's
        assert status == [0, 0] and dec.compare_ms() > 0
        want = fm.batch(want_planes, fmt, bits, (24, 17))
        assert all(same_planes(keep_planes(fmt, (24, 17), keep, i), want[i]) for i in range(2)), fmt
        wins = [(4, 2, info.width - 9, info.height - 7), (info.width - 3 & ~1, info.height - 2 & ~1, 3, 2)]
        arr, keep, status = job.resized_frames((31, 9), wins, "bilinear", bits=bits - 1)
        want = fm.batch(want_planes, fmt, bits - 1, (31, 9), wins, fm.BILINEAR)
        assert all(same_planes(keep_planes(fmt, (31, 9), keep, i), want[i]) for i in range(2)), fmt
        with pytest.raises(m.Htj2kError) as e:               # a window that leaves the frame
            job.resized_frames((4, 4), (2, 0, info.width, 2))
        assert e.value.code == EINVAL
        job.run(stages=3)                                    # a run that did not write the frames
        with pytest.raises(m.Htj2kError) as e:
            job.resized_frames((4, 4))
        assert e.value.code == EINVAL
    # blocks that the decoder rejects stay zero: the frame is still a frame, and is resampled
    good = get("gray_l5_cb64")
    bad = damaged_copy(good)
    planes_bad = orc.decode(bad)[1]
    assert orc.block_errors() > 0
    job.parse_batch([good, bad, good]).upload().run()
    arr, keep, status = job.resized_frames((19, 23))
    assert status == [0, 0, 0] and job.block_errors() == orc.block_errors()
    want = fm.batch([orc.decode(good)[1], planes_bad, orc.decode(good)[1]], "gray", 8, (19, 23))
    assert all(same_planes(keep_planes("gray", (19, 23), keep, i), want[i]) for i in range(3)) and not np.array_equal(want[0][0], want[1][0])
    # frames of different layouts in one job
    job.parse_batch([get("rgb_mct"), get("gray_l5_cb64")]).upload().run()
    with pytest.raises(m.Htj2kError) as e:
        job.resized_frames((8, 8))
    assert e.value.code == EINVAL
    job.free()


def check_pipes(dec, orc, wait=60):
    """resized frames in between plain receives, with a packet that fails to parse"""
    names = ["rgb_mct", "yuv420p8", "gray16", "tiny_7x5"]
    pkts = [streams.get(names[i % 4])[0] for i in range(12)]
    pkts[5] = pkts[5][:40]                                   # fails to parse: its batch is retried packet by packet
    want = [None if i == 5 else orc.decode(p)[:2] for i, p in enumerate(pkts)]
    pipe = bounded(lambda: dec.pipe(batch=4, depth=2), wait)
    try:
        sent = got = 0
        while got < len(pkts):
            while sent < len(pkts) and bounded(lambda: pipe.send(pkts[sent]), wait):
                sent += 1
            if sent == len(pkts):
                bounded(pipe.flush, wait)
            if got == 5:
                with pytest.raises(m.Htj2kError) as e:       # its own error, and the pipe moves on
                    bounded(lambda: pipe.receive_resized((4, 4)), wait)
                assert e.value.code < 0 and e.value.code != m.EAGAIN
                got += 1
                continue
            info_o, planes_o = want[got]
            fmt, bits = m.PIX_NAMES[info_o.pix_fmt], info_o.bits_per_raw_sample
            if got % 3 == 0:
                info, planes = bounded(pipe.receive, wait)
                assert all(np.array_equal(a, b) for a, b in zip(planes, planes_o)), got
            elif got == 8:                                   # a refusal consumes the frame
                with pytest.raises(m.Htj2kError) as e:
                    bounded(lambda: pipe.receive_resized((4, 4), (0, 0, info_o.width + 1, 1)), wait)
                assert e.value.code == EINVAL
            else:
                window = None if got % 2 else (2, 2, info_o.width - 3, info_o.height - 3)
                filt = FILTERS[got % 3]
                arr, keep, info = bounded(lambda: pipe.receive_resized((9, 6), window, m.RESIZE_FILTERS[filt]), wait)
                assert (info.width, info.height, info.pix_fmt) == (info_o.width, info_o.height, info_o.pix_fmt), got
                assert (arr[0].width, arr[0].height, arr[0].pix_fmt) == (9, 6, info_o.pix_fmt)
                assert same_planes(keep_planes(fmt, (9, 6), keep), fm.frame(planes_o, fmt, bits, (9, 6), window, filt)), got
            got += 1
        assert bounded(lambda: pipe.receive_resized((4, 4)), wait) is None and bounded(pipe.receive, wait) is None    # drained
    finally:
        bounded(pipe.close, wait)


def check_proxy(dec, orc):
    """a 64 x 48 lossless stream decoded as a job, resized to 32 x 24, encoded from the device and decoded again: the
    model's frames, exactly"""
    enc = m.Encoder(device_id=0)
    try:
        for fmt, data in (("yuv422p10le", yuv422p10_stream()), ("rgb24", streams._enc((64, 48, 3, 8, 5), mct=1, nlevels=3))):
            info_o, planes_o = orc.decode(data)[:2]
            assert (info_o.width, info_o.height) == (64, 48) and m.PIX_NAMES[info_o.pix_fmt] == fmt
            bits = info_o.bits_per_raw_sample
            job = dec.job().parse_batch([data, data]).upload().run()
            arr, keep, status = job.resized_frames((32, 24))
            assert status == [0, 0]
            proxies = enc.encode_device([arr[0], arr[1]], fmt, bits, levels=3)
            want = fm.frame(planes_o, fmt, bits, (32, 24))
            for px in proxies:
                info_p, planes_p = orc.decode(px, req_pix_fmt=info_o.pix_fmt)[:2]
                assert (info_p.width, info_p.height, info_p.pix_fmt, info_p.lossless) == (32, 24, info_o.pix_fmt, 1)
                assert same_planes([np.asarray(p) for p in planes_p], want), fmt
            back = dec.job().parse_batch(proxies).upload().run()
            assert all(d["sse"] == [0, 0, 0, 0] for d in back.compare([want, want], bits))
            back.free()
            job.free()
    finally:
        enc.close()


def check_refusals(dec):
    """every refusal on a live context: nothing launched, the destination and its guards untouched, and the context works on"""
    rng = np.random.default_rng(3)
    f = HFrame("yuv420p", 20, 10, rng)
    other = HFrame("yuv422p", 20, 10, rng)
    pal = HFrame("pal8", 20, 10, rng)
    wide = HFrame("yuv420p", 130, 2, rng)

    def with_(fr, **kw):
        for k, v in kw.items():
            which, p = k.split("_")
            if which == "data":
                fr.data[int(p)] = v
            elif which == "linesize":
                fr.linesize[int(p)] = v
            else:
                setattr(fr, which, int(p) if v is None else v)
        return fr

    d = lambda fmt="yuv420p", size=(8, 6): DFrame(fmt, size[0], size[1], "row+1", 1)
    cases = [  # (sources, destinations, changes to destination 0's frame, n or None, bits, windows, filter, answer)
        ([f], [d()], {}, 0, 8, None, 2, EINVAL),
        ([pal], [d()], {}, None, 8, None, 2, PATCHWELCOME),
        ([f], [d()], {}, None, 9, None, 2, EINVAL),
        ([f], [d()], {}, None, 0, None, 2, EINVAL),
        ([f], [d()], {}, None, 8, None, 3, EINVAL),
        ([f], [d()], {}, None, 8, None, -1, EINVAL),
        ([f, other], [d(), d()], {}, None, 8, None, 2, EINVAL),
        ([f], [d("yuv422p")], {}, None, 8, None, 2, EINVAL),
        ([f, f], [d(), d(size=(8, 7))], {}, None, 8, None, 2, EINVAL),
        ([f], [d()], {"width_x": 0}, None, 8, None, 2, EINVAL),
        ([f], [d()], {}, None, 8, [(0, 0, 0, 4)], 2, EINVAL),
        ([f], [d()], {}, None, 8, [(0, 0, 4, -1)], 1, EINVAL),
        ([f], [d()], {}, None, 8, [(-2, 0, 4, 4)], 2, EINVAL),
        ([f], [d()], {}, None, 8, [(0, -2, 4, 4)], 0, EINVAL),
        ([f], [d()], {}, None, 8, [(18, 0, 4, 4)], 2, EINVAL),
        ([f], [d()], {}, None, 8, [(0, 8, 4, 4)], 2, EINVAL),
        ([f, f], [d(), d()], {}, None, 8, [(0, 0, 20, 10), (0, 0, 21, 10)], 2, EINVAL),
        ([f], [d()], {}, None, 8, [(1, 0, 4, 4)], 2, EINVAL),
        ([f], [d()], {}, None, 8, [(0, 1, 4, 4)], 0, EINVAL),
        ([wide], [d(size=(2, 2))], {}, None, 8, None, 2, PATCHWELCOME),
        ([wide], [d(size=(4, 2))], {}, None, 8, [(0, 0, 130, 2)], 2, 0),       # 130 <= 64 x 4: in scope, and runs
        ([wide], [d(size=(2, 2))], {}, None, 8, [(2, 0, 128, 2)], 2, 0),
        ([wide], [d(size=(2, 2))], {}, None, 8, None, 1, 0),
        ([f], [d()], {"data_1": None}, None, 8, None, 2, EINVAL),
        ([f], [d()], {"linesize_0": 7}, None, 8, None, 2, EINVAL),
        ([f], [d()], {"linesize_2": -5}, None, 8, None, 2, EINVAL),
    ]
    for i, (srcs, dsts, change, n, bits, windows, filt, answer) in enumerate(cases):
        sarr = (m.Frame * len(srcs))(*[s.frame() for s in srcs])
        frames = [x.frame() for x in dsts]
        with_(frames[0], **change)
        r = raw_call(dec, sarr, 0, len(srcs) if n is None else n, bits, windows, filt, (m.Frame * len(frames))(*frames))
        assert r == answer, (i, r)
        if answer:
            assert all(x.untouched() for x in dsts), i
    no_src = raw_call(dec, None, 0, 1, 8, None, 2, (m.Frame * 1)(d().frame()))
    no_dst = raw_call(dec, (m.Frame * 1)(f.frame()), 0, 1, 8, None, 2, None)
    assert no_src == EINVAL and no_dst == EINVAL
    check(dec, [f], "yuv420p", 8, (7, 3), None, fm.BILINEAR)    # the context still works


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_layouts_filters_and_sizes(dec, fmt):
    check_layout(dec, fmt, LAYOUTS.index(fmt))


@pytest.mark.gpu
def test_tile_seams_under_every_chroma_shift(dec):
    check_seams(dec)


@pytest.mark.gpu
def test_the_most_taps_an_axis_has(dec):
    check_taps(dec)


@pytest.mark.gpu
def test_odd_bases_and_linesizes_of_two_byte_layouts(dec):
    check_alignment(dec)


@pytest.mark.gpu
def test_knobs_never_show_in_the_bytes(dec):
    check_knobs(dec)


@pytest.mark.gpu
def test_constants_peaks_and_the_identity(dec):
    check_invariants(dec)


@pytest.mark.gpu
def test_unlike_frames_windows_and_reductions_in_one_call(dec):
    check_batches(dec)


@pytest.mark.gpu
def test_more_planes_than_one_launch_takes(dec):
    check_many_frames(dec)


@pytest.mark.gpu
def test_the_tensor_route_beside_it(dec):
    check_tensor_route(dec)


@pytest.mark.gpu
def test_python_entry_points(dec):
    check_python(dec)


@pytest.mark.gpu
def test_jobs(dec, orc):
    check_jobs(dec, orc)


@pytest.mark.gpu
def test_pipes(dec, orc):
    check_pipes(dec, orc)


@pytest.mark.gpu
def test_proxy_round_trip(dec, orc):
    check_proxy(dec, orc)


@pytest.mark.gpu
def test_refusals_on_a_live_context(dec):
    check_refusals(dec)


def run_everything(dec, orc):
    for i, fmt in enumerate(LAYOUTS):
        check_layout(dec, fmt, i)
    check_seams(dec)
    check_taps(dec)
    check_alignment(dec)
    check_knobs(dec)
    check_invariants(dec)
    check_batches(dec)
    check_many_frames(dec)
    check_tensor_route(dec)
    check_python(dec)
    check_jobs(dec, orc)
    check_pipes(dec, orc)
    check_proxy(dec, orc)
    check_refusals(dec)


POISON_TIMEOUT = 300


@pytest.mark.gpu
def test_everything_on_poisoned_buffers():
    """HTJ2K_POISON=1 (read once per process, so a fresh child): every new device buffer of the library starts as 0xA5
    bytes, and all of the above must still give the model's results.  The child's exit status comes first."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True,
                       timeout=POISON_TIMEOUT, env=dict(os.environ, HTJ2K_POISON="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "poisoned buffers: ok" in r.stdout, r.stdout[-3000:]


if __name__ == "__main__":
    t0 = time.time()
    _dec, _orc = m.Decoder(device_id=0), oracle.OracleDecoder()
    run_everything(_dec, _orc)
    _dec.close()
    _orc.close()
    print("%s buffers: ok, %.1f s, %d calls" % ("poisoned" if os.environ.get("HTJ2K_POISON") == "1" else "plain", time.time() - t0, CALLS["n"]))
