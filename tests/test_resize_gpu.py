"""htj2k_frames_to_tensor_resized / htj2k_job_to_tensor_resized / htj2k_pipe_receive_tensor_resized on the GPU against the
numpy model (resize_model): every bit of every element.

Three filters, three element types and two layouts on ten layouts of frames; windows whose chroma footprints are cut at
both ends, windows on every frame edge, the most taps an axis can have, outputs at the tile's width and around it, the
seams of the row streaming inside small frames (knob resize_rows), constant pictures at the largest accumulator; identity
windows against the plain call; unlike frames in one call, more planes than grid.z takes; host and device operands with
linesizes and bases off every alignment and 0xAB in the padding; destinations between 0xA5 guard zones at their element's
own alignment; every refusal on a live context; jobs, pipes and a context shared with the measuring calls.  Run as a
program, the module runs all of it on its own contexts: test_everything_on_poisoned_buffers does that in a child process
under HTJ2K_POISON=1."""
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
import resize_model as rm
import streams
import tensor_model as tm
from test_hash_gpu import HFrame, damaged_copy
from test_tensor_gpu import bounded, tensor_bits, yuv422p10_stream

LAYOUTS = ["gray", "ya8", "rgb24", "rgb48le", "rgba", "yuv420p", "yuv422p10le", "yuv410p", "yuva444p16le", "xyz12le"]
LS_MODES = ["row", "row+1", "row+13", "to64"]
OFFSETS = [0, 1, 2, 15]
LAYOUT_NAMES = ["NCHW", "NHWC"]
FILTERS = [rm.NEAREST, rm.BILINEAR, rm.TRIANGLE]
PAIRS = [(1 / 255, 0.0), (1 / 1023, -0.5), (3.0, -7.25), (1 / (255 * 0.229), -0.485 / 0.229), (2.0 ** -12, 0.0), (-1.0, 0.0)]
EINVAL, PATCHWELCOME = -22, -0x45574150
GUARD, SURPLUS = 4096, 48
ROUTE = 4
TILE_W, TILE_H = 32, 16                                  # RS_TW, RS_TH of csrc/resize_kernels.hpp
CALLS = {"n": 0}


def windows_array(windows):
    return None if windows is None else (ctypes.c_int32 * (4 * len(windows)))(*[int(v) for w in windows for v in w])


def raw_call(dec, arr, on_device, n, bits, spec, windows, filt, nbytes, dst_off_bytes=0):
    """the C call on a destination between two guard zones, `SURPLUS` bytes larger than needed -> (return value, the whole
    buffer as a host array, where the images start in it)"""
    at = GUARD + dst_off_bytes
    buf = torch.full((at + nbytes + SURPLUS + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    r = dec.L.htj2k_frames_to_tensor_resized(dec.h, arr, int(on_device), n, int(bits), ctypes.byref(spec), windows_array(windows), int(filt),
                                             ctypes.c_void_p(buf.data_ptr() + at), ctypes.c_size_t(nbytes + SURPLUS))
    return r, buf.cpu().numpy(), at


def convert(dec, frames, fmt, bits, size, windows, filt, dtype, layout, scale, bias, on_device, dst_off=0):
    """-> bit patterns shaped as the model's; the guards and the surplus bytes must still be 0xA5, the route 4"""
    n, nc = len(frames), tm.ncomp(fmt)
    ow, oh = size
    es = tm.ESIZE[dtype]
    nbytes = n * nc * ow * oh * es
    spec = m.tensor_spec(dtype, layout, size, scale, bias)
    keep = []
    if on_device:
        made = [f.on_device() for f in frames]
        keep = [k for _, k in made]
        arr = (m.Frame * n)(*[fr for fr, _ in made])
    else:
        arr = (m.Frame * n)(*[f.frame() for f in frames])
    r, host, at = raw_call(dec, arr, on_device, n, bits, spec, windows, filt, nbytes, dst_off * es)
    assert r == 0, (r, fmt, dtype, layout, size, windows, filt)
    assert (host[:at] == 0xA5).all(), "bytes in front of dst were written"
    assert (host[at + nbytes:] == 0xA5).all(), "bytes beyond the images were written"
    assert dec.tensor_last_route() == ROUTE
    CALLS["n"] += 1
    del keep
    return host[at:at + nbytes].view(tm.BITS_DTYPE[dtype]).reshape((n, nc, oh, ow) if layout == "NCHW" else (n, oh, ow, nc))


def check(dec, frames, fmt, bits, size, windows=None, filt=rm.TRIANGLE, dtype="float16", layout="NCHW", scale=None, bias=None,
          on_device=False, dst_off=0, want=None):
    """one call against the model -> the bits"""
    if want is None:
        want = rm.batch([f.arrays() for f in frames], fmt, bits, dtype, layout, size, windows, filt, scale, bias)
    what = (fmt, bits, size, windows, filt, dtype, layout, scale, bias, on_device, dst_off, [(f.w, f.h, f.ls, f.off) for f in frames[:4]])
    got = convert(dec, frames, fmt, bits, size, windows, filt, dtype, layout, scale, bias, on_device, dst_off)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [hex(int(got[tuple(b)])) for b in bad[:4]], [hex(int(want[tuple(b)])) for b in bad[:4]])
    return got


def low_bits(fmt):
    return {"rgb48le": 12, "yuv422p10le": 9}.get(fmt, cm.LAYOUTS[fmt][4] - 1)


def check_layout(dec, fmt, li):
    """filters x element types x layouts on a 3 x 3 reduction, a 1 x 1 output and a window one pixel wide upscaled to 17;
    host and device operands, every linesize and base, a destination off by one element"""
    depth = cm.LAYOUTS[fmt][4]
    cases = [((21, 15), None, (7, 5)), ((21, 15), None, (1, 1)), ((21, 15), (9, 2, 1, 11), (17, 11))]
    k = 0
    for ci, ((w, h), window, size) in enumerate(cases):
        for on_device in (False, True):
            f = HFrame(fmt, w, h, np.random.default_rng(100 * li + 10 * ci + on_device), LS_MODES[(li + ci + on_device) % 4],
                       OFFSETS[(li + 2 * ci + 3 * on_device) % 4])
            for filt in FILTERS:
                for dtype in tm.DTYPES:
                    for layout in LAYOUT_NAMES:
                        k += 1
                        if (k + on_device) % 2:                              # each half of the combinations on one kind of operand
                            continue
                        scale, bias = PAIRS[k % len(PAIRS)]
                        bits = low_bits(fmt) if k % 7 == 0 else depth
                        check(dec, [f], fmt, bits, size, None if window is None else [window], filt, dtype, layout, scale, bias, on_device,
                              dst_off=k % 3 == 0)


def check_shapes(dec):
    """the shapes at which the kernel can go wrong"""
    rng = np.random.default_rng(31)
    # a 37 x 53 window of a 64 x 61 frame at odd origins: chroma footprints cut at both ends, down and up
    for i, fmt in enumerate(("yuv420p", "yuv410p", "yuv422p10le", "rgb24")):
        f = HFrame(fmt, 64, 61, rng, LS_MODES[i], OFFSETS[i])
        for j, filt in enumerate(FILTERS):
            check(dec, [f], fmt, cm.LAYOUTS[fmt][4], (16, 20), [(21, 7, 37, 53)], filt, tm.DTYPES[(i + j) % 3], LAYOUT_NAMES[j % 2], 1 / 255, -0.5, i % 2)
            check(dec, [f], fmt, cm.LAYOUTS[fmt][4], (50, 70), [(21, 7, 37, 53)], filt, tm.DTYPES[(i + j + 1) % 3], LAYOUT_NAMES[(j + 1) % 2], 1 / 255, 0.0,
                  (i + 1) % 2)
    # windows on every edge of the frame: taps beyond it are dropped
    f = HFrame("yuv420p", 40, 30, rng, "row+13", 1)
    for window in ((0, 0, 20, 15), (20, 0, 20, 30), (0, 15, 40, 15), (20, 15, 20, 15), (0, 0, 40, 30), (39, 29, 1, 1), (0, 29, 40, 1)):
        for filt in FILTERS:
            check(dec, [f], "yuv420p", 8, (9, 7), [window], filt, "float32", "NCHW", 1.0, 0.0, True)
    # ww = 64 out_w exactly on a 512 x 9 frame: the most taps an axis has, 128
    assert max(len(rm.weights(512, 8, rm.TRIANGLE, x)[1]) for x in range(8)) == 128
    for fmt in ("gray", "rgb48le"):
        f = HFrame(fmt, 512, 9, rng, "to64")
        for on_device in (False, True):
            check(dec, [f], fmt, cm.LAYOUTS[fmt][4], (8, 3), None, rm.TRIANGLE, "float32", "NHWC", 1.0, 0.0, on_device)
    f = HFrame("gray16le", 9, 512, rng, "row+1", 1)
    check(dec, [f], "gray16le", 16, (3, 8), None, rm.TRIANGLE, "float32", "NCHW", 1.0, 0.0, True)
    # every number of lanes that share the taps of a horizontal sum: 1, 2, 4, 8, 16, 32 at 5 to 129 taps (resize_share)
    # chosen by the library (knob 0), and each of them forced on a reduction, an enlargement and a one-tap axis
    for fmt in ("rgb24", "yuv420p16le"):
        f = HFrame(fmt, 256, 5, rng, "row+1", 1)
        for ow in (128, 40, 20, 10, 5, 4):
            check(dec, [f], fmt, cm.LAYOUTS[fmt][4], (ow, 3), None, rm.TRIANGLE, "float32", "NCHW", 1.0, 0.0, ow % 4 == 0)
        for knob in range(1, 7):
            dec.set_int("resize_share", knob)
            try:
                for k, (ow, filt) in enumerate(((23, rm.TRIANGLE), (4, rm.TRIANGLE), (300, rm.BILINEAR), (256, rm.TRIANGLE), (9, rm.NEAREST))):
                    check(dec, [f], fmt, cm.LAYOUTS[fmt][4], (ow, 2), None, filt, "float32", LAYOUT_NAMES[k % 2], 1.0, 0.0, (k + knob) % 2)
            finally:
                dec.set_int("resize_share", 0)
    # outputs at the tile's size, one below and one above it, from a frame that is reduced and one that is enlarged
    for fmt, (w, h) in (("rgb24", (70, 40)), ("yuv420p", (19, 11))):
        f = HFrame(fmt, w, h, rng, "row+1", 2)
        for ow in (TILE_W - 1, TILE_W, TILE_W + 1):
            for oh in (TILE_H - 1, TILE_H, TILE_H + 1):
                check(dec, [f], fmt, 8, (ow, oh), None, FILTERS[(ow + oh) % 3], "float16", LAYOUT_NAMES[ow % 2], 1 / 255, 0.0, oh % 2)
    # the seams of the row streaming: the smallest step, and steps that leave one odd row
    f = HFrame("yuv422p10le", 50, 41, rng, "row+13", 15)
    want = {}
    for rows in (0, 1, 5, 16):
        dec.set_int("resize_rows", rows)
        try:
            for filt in FILTERS:
                for size, window in (((13, 9), None), ((33, 35), (3, 5, 40, 31)), ((50, 41), None)):
                    got = check(dec, [f], "yuv422p10le", 10, size, None if window is None else [window], filt, "bfloat16", "NHWC", 1 / 1023, -0.5, True)
                    assert np.array_equal(want.setdefault((filt, size), got), got)
        finally:
            dec.set_int("resize_rows", 0)
    assert 41 % 5 == 1                                       # the whole frame to 9 rows is one tile of 41 source rows: 8 steps of 5 and one row
    # constant pictures stay constant: 16-bit samples all 65535 (the accumulator at its largest) and all 0
    for value, sample in ((0xFF, 65535), (0, 0)):
        f = HFrame("gray16le", 130, 70, rng, "to64", 0, value=value)
        for filt in FILTERS:
            for size in ((3, 2), (131, 71), (40, 70)):
                got = check(dec, [f], "gray16le", 16, size, None, filt, "float32", "NCHW", 1.0, 0.0, True)
                assert (got.view(np.float32) == sample).all()


def check_identity(dec):
    """ww = out_w and wh = out_h: the plain call's bits from the new kernel, whatever the filter"""
    rng = np.random.default_rng(41)
    for i, fmt in enumerate(LAYOUTS):
        depth = cm.LAYOUTS[fmt][4]
        f = HFrame(fmt, 45, 19, rng, LS_MODES[i % 4], OFFSETS[i % 4])
        planes = [f.arrays()]
        for j, (window, filt) in enumerate((((0, 0, 45, 19), rm.TRIANGLE), ((7, 3, 33, 16), rm.BILINEAR), ((16, 2, 16, 5), rm.NEAREST))):
            dtype, layout = tm.DTYPES[(i + j) % 3], LAYOUT_NAMES[(i + j) % 2]
            size = window[2:]
            plain = dec.to_tensor(planes, fmt, depth, dtype, layout, size=size, origins=window[:2], scale=1 / 255, bias=-0.5)
            assert dec.tensor_last_route() in (1, 2, 3)
            resized = dec.to_tensor_resized(planes, fmt, depth, size, [window], m.RESIZE_FILTERS[filt], dtype, layout, 1 / 255, -0.5)
            assert dec.tensor_last_route() == ROUTE
            assert np.array_equal(tensor_bits(resized), tensor_bits(plain)), (fmt, window, filt)
            check(dec, [f], fmt, depth, size, [window], filt, dtype, layout, 1 / 255, -0.5, True, want=tensor_bits(plain))


def check_batches(dec):
    """frames of four sizes with four windows and reductions in one call"""
    rng = np.random.default_rng(51)
    sizes = [(40, 9), (33, 42), (200, 7), (17, 5)]
    windows = [(8, 2, 24, 6), (0, 0, 33, 42), (3, 1, 192, 6), (16, 4, 1, 1)]
    for fmt, bits in (("rgb24", 8), ("yuv420p", 8), ("yuv422p10le", 10), ("rgba", 8)):
        for on_device in (False, True):
            fs = [HFrame(fmt, w, h, rng, LS_MODES[i], OFFSETS[3 - i]) for i, (w, h) in enumerate(sizes)]
            for filt, dtype, layout in ((rm.TRIANGLE, "float16", "NCHW"), (rm.BILINEAR, "float32", "NHWC"), (rm.NEAREST, "bfloat16", "NCHW")):
                check(dec, fs, fmt, bits, (12, 6), windows, filt, dtype, layout, 1 / 255, 0.0, on_device)
        check(dec, fs, fmt, bits, (5, 4), None, rm.TRIANGLE, "float16", "NHWC", 1.0, 0.5, True)      # each frame whole


def check_many_frames(dec, n=70000):
    """more planes than grid.z takes in one launch: 8 x 8 gray frames out of one buffer, each to 4 x 4"""
    a = np.random.default_rng(9).integers(0, 256, size=(n, 8, 8), dtype=np.uint8)
    rec = np.dtype({"names": ["data", "linesize", "width", "height", "pix_fmt"], "formats": [("<u8", 4), ("<i4", 4), "<i4", "<i4", "<i4"],
                    "offsets": [0, 32, 48, 52, 56], "itemsize": ctypes.sizeof(m.Frame)})
    t = np.zeros(n, rec)
    t["data"][:, 0] = a.ctypes.data + 64 * np.arange(n, dtype=np.uint64)
    t["linesize"][:, 0] = 8
    t["width"], t["height"], t["pix_fmt"] = 8, 8, m.PIX_NAMES.index("gray")
    W = rm.matrix(8, 4, rm.TRIANGLE)
    acc = np.einsum("yY,nYX,xX->nyx", W, a.astype(np.int64), W)
    want = tm.value_bits((acc.astype(np.float64) * 2.0 ** -28).astype(np.float32), 1 / 255, -0.5, "float16")
    spec = m.tensor_spec("float16", "NCHW", (4, 4), 1 / 255, -0.5)
    r, host, at = raw_call(dec, t.ctypes.data_as(ctypes.c_void_p), 0, n, 8, spec, None, rm.TRIANGLE, n * 32)
    assert r == 0 and dec.tensor_last_route() == ROUTE
    assert (host[:at] == 0xA5).all() and (host[at + n * 32:] == 0xA5).all()
    assert np.array_equal(host[at:at + n * 32].view(np.uint16).reshape(n, 4, 4), want)


def check_refusals(dec):
    """every refusal on a live context: nothing launched, dst and its guards untouched, route 0, and the context works on"""
    rng = np.random.default_rng(3)
    f = HFrame("yuv420p", 20, 10, rng)
    other = HFrame("yuv422p", 20, 10, rng)
    pal = HFrame("pal8", 20, 10, rng)
    wide = HFrame("gray", 130, 2, rng)
    ok = m.tensor_spec("float16", size=(4, 4))
    need = 3 * 4 * 4 * 2

    def spec(**kw):
        s = m.tensor_spec("float16", size=(4, 4))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def floats(field, k, v):
        s = m.tensor_spec("float16", size=(4, 4))
        getattr(s, field)[k] = v
        return s

    def frame_with(g, **kw):
        fr = g.frame()
        for k, v in kw.items():
            which, p = k.split("_")
            if which == "data":
                fr.data[int(p)] = v
            else:
                fr.linesize[int(p)] = v
        return fr

    cases = [  # (frames, n or None, bits, spec, windows, filter, bytes of dst, offset of dst, what it answers)
        ([f.frame()], 0, 8, ok, None, 2, need, 0, EINVAL),
        ([pal.frame()], None, 8, ok, None, 2, need, 0, PATCHWELCOME),
        ([f.frame()], None, 9, ok, None, 2, need, 0, EINVAL),
        ([f.frame()], None, 8, spec(dtype=3), None, 2, need, 0, EINVAL),
        ([f.frame()], None, 8, spec(layout=2), None, 2, need, 0, EINVAL),
        ([f.frame()], None, 8, ok, None, 3, need, 0, EINVAL),
        ([f.frame()], None, 8, ok, None, -1, need, 0, EINVAL),
        ([f.frame()], None, 8, floats("scale", 2, float("nan")), None, 2, need, 0, EINVAL),
        ([f.frame()], None, 8, floats("bias", 0, float("inf")), None, 2, need, 0, EINVAL),
        ([f.frame()], None, 8, spec(out_w=0, out_h=0), None, 2, need, 0, EINVAL),
        ([f.frame()], None, 8, spec(out_w=4, out_h=0), None, 2, need, 0, EINVAL),
        ([f.frame(), other.frame()], None, 8, ok, None, 2, 2 * need, 0, EINVAL),
        ([frame_with(f, data_1=None)], None, 8, ok, None, 2, need, 0, EINVAL),
        ([frame_with(f, linesize_0=19)], None, 8, ok, None, 2, need, 0, EINVAL),
        ([frame_with(f, linesize_2=-10)], None, 8, ok, None, 2, need, 0, EINVAL),
        ([f.frame()], None, 8, ok, [(0, 0, 0, 4)], 2, need, 0, EINVAL),
        ([f.frame()], None, 8, ok, [(0, 0, 4, -1)], 1, need, 0, EINVAL),
        ([f.frame()], None, 8, ok, [(-1, 0, 4, 4)], 2, need, 0, EINVAL),
        ([f.frame()], None, 8, ok, [(0, -1, 4, 4)], 0, need, 0, EINVAL),
        ([f.frame()], None, 8, ok, [(17, 0, 4, 4)], 2, need, 0, EINVAL),
        ([f.frame()], None, 8, ok, [(0, 7, 4, 4)], 2, need, 0, EINVAL),
        ([f.frame(), f.frame()], None, 8, ok, [(0, 0, 20, 10), (0, 0, 21, 10)], 2, 2 * need, 0, EINVAL),
        ([f.frame()], None, 8, spec(out_w=32769, out_h=1), None, 1, 3 * 32769 * 2, 0, PATCHWELCOME),
        ([wide.frame()], None, 8, spec(out_w=2, out_h=2), None, 2, need, 0, PATCHWELCOME),
        ([wide.frame()], None, 8, spec(out_w=4, out_h=2), [(0, 0, 130, 2)], 2, need, 0, ROUTE),     # 130 <= 64 x 4: in scope, and runs
        ([wide.frame()], None, 8, spec(out_w=2, out_h=2), [(1, 0, 129, 2)], 2, need, 0, PATCHWELCOME),
        ([f.frame()], None, 8, ok, None, 2, need - 1 - SURPLUS, 0, EINVAL),
        ([f.frame()], None, 8, ok, None, 2, need, 1, EINVAL),
        ([f.frame()], None, 8, m.tensor_spec("float32", size=(4, 4)), None, 2, 2 * need, 2, EINVAL),
    ]
    for i, (frames, n, bits, s, windows, filt, nbytes, off, answer) in enumerate(cases):
        check(dec, [f], "yuv420p", 8, (4, 4))                  # a call that launches, so that a route is there to be cleared
        arr = (m.Frame * len(frames))(*frames)
        r, host, at = raw_call(dec, arr, 0, len(frames) if n is None else n, bits, s, windows, filt, nbytes, off)
        if answer == ROUTE:
            assert r == 0 and dec.tensor_last_route() == ROUTE, (i, r)
            continue
        assert r == answer, (i, r)
        assert (host == 0xA5).all(), i
        assert dec.tensor_last_route() == 0, i
    for knob, values in (("resize_rows", (-1, 17, 100)), ("resize_share", (-1, 7))):
        for bad in values:
            with pytest.raises(m.Htj2kError) as e:
                dec.set_int(knob, bad)
            assert e.value.code == EINVAL
    check(dec, [f], "yuv420p", 8, (7, 3), None, rm.BILINEAR, "float32", "NHWC")    # the context still works


def check_python(dec):
    """Decoder.to_tensor_resized: numpy planes in, a torch tensor out; `out` is checked"""
    rng = np.random.default_rng(12)
    fs = [HFrame("rgb24", 33, 6, rng), HFrame("rgb24", 20, 9, rng)]
    planes = [f.arrays() for f in fs]
    t = dec.to_tensor_resized(planes, "rgb24", 8, (8, 4), scale=1 / 255)
    assert t.dtype == torch.float16 and tuple(t.shape) == (2, 3, 4, 8) and t.is_contiguous() and t.is_cuda
    assert np.array_equal(tensor_bits(t), rm.batch(planes, "rgb24", 8, "float16", "NCHW", (8, 4), None, rm.TRIANGLE, 1 / 255, 0.0))
    assert dec.tensor_last_route() == ROUTE and dec.compare_ms() > 0
    out = torch.zeros((2, 40, 50, 3), dtype=torch.bfloat16, device="cuda")
    t2 = dec.to_tensor_resized(planes, "rgb24", 8, (50, 40), (1, 1, 15, 5), "bilinear", torch.bfloat16, "NHWC", [1, 2, 3], 0.5, out=out)
    assert t2 is out
    assert np.array_equal(tensor_bits(out), rm.batch(planes, "rgb24", 8, "bfloat16", "NHWC", (50, 40), [(1, 1, 15, 5)] * 2, rm.BILINEAR, [1, 2, 3], 0.5))
    devs = [f.on_device() for f in fs]
    t3 = dec.to_tensor_resized([d for d, _ in devs], "rgb24", 8, (5, 5), [(0, 0, 33, 6), (2, 2, 10, 7)], "nearest", "float32", on_device=True)
    assert np.array_equal(tensor_bits(t3), rm.batch(planes, "rgb24", 8, "float32", "NCHW", (5, 5), [(0, 0, 33, 6), (2, 2, 10, 7)], rm.NEAREST))
    for bad in (torch.zeros((2, 40, 50, 3), dtype=torch.float16, device="cuda"), torch.zeros((2, 40, 50, 4), dtype=torch.bfloat16, device="cuda"),
                torch.zeros((2, 40, 50, 3), dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            dec.to_tensor_resized(planes, "rgb24", 8, (50, 40), None, "bilinear", torch.bfloat16, "NHWC", out=bad)
    with pytest.raises(ValueError):
        dec.to_tensor_resized(planes, "rgb24", 8, None)
    with pytest.raises(ValueError):
        dec.to_tensor_resized(planes, "rgb24", 8, (4, 4), filter="lanczos")
    with pytest.raises(ValueError):
        dec.to_tensor_resized(planes, "rgb24", 8, (4, 4), windows=[(0, 0, 4, 4)] * 3)
    assert m.Decoder.resize_weights(8, 4, "triangle", 1) == rm.weights(8, 4, rm.TRIANGLE, 1)


def check_jobs(dec, orc):
    get = lambda name: streams.get(name)[0]
    groups = [("rgb24", [get("rgb_mct"), get("rgb_tiles")]), ("yuv420p", [get("yuv420p8"), get("yuv420p8")]),
              ("yuv422p10le", [yuv422p10_stream()] * 2), ("gray16le", [get("gray16")] * 2)]
    job = dec.job()
    for li, (fmt, datas) in enumerate(groups):
        job.parse_batch(datas).upload()
        with pytest.raises(m.Htj2kError) as e:               # before the first run
            job.to_tensor_resized((8, 8))
        assert e.value.code == EINVAL and dec.tensor_last_route() == 0
        job.run()
        info = job.frame_info(0)
        assert m.PIX_NAMES[info.pix_fmt] == fmt
        bits = info.bits_per_raw_sample
        want_planes = [orc.decode(d)[1] for d in datas]
        scale = 1 / ((1 << bits) - 1)
        t, status = job.to_tensor_resized((24, 17), scale=scale)                                     # each frame whole, bits 0: the job's
        assert status == [0, 0] and tuple(t.shape) == (2, tm.ncomp(fmt), 17, 24) and dec.tensor_last_route() == ROUTE
        assert np.array_equal(tensor_bits(t), rm.batch(want_planes, fmt, bits, "float16", "NCHW", (24, 17), None, rm.TRIANGLE, scale, 0.0)), fmt
        wins = [(5, 3, info.width - 9, info.height - 7), (info.width - 3, info.height - 2, 3, 2)]
        t, status = job.to_tensor_resized((31, 9), wins, "bilinear", "float32", "NHWC", scale, -0.5, bits=bits - 1)
        assert np.array_equal(tensor_bits(t), rm.batch(want_planes, fmt, bits - 1, "float32", "NHWC", (31, 9), wins, rm.BILINEAR, scale, -0.5)), fmt
        with pytest.raises(m.Htj2kError) as e:               # a window that leaves the frame
            job.to_tensor_resized((4, 4), (1, 0, info.width, 2))
        assert e.value.code == EINVAL and dec.tensor_last_route() == 0
        job.run(stages=3)                                    # a run that did not write the frames
        with pytest.raises(m.Htj2kError) as e:
            job.to_tensor_resized((4, 4))
        assert e.value.code == EINVAL
    # blocks that the decoder rejects stay zero: the frame is still a frame, and is resampled
    good = get("gray_l5_cb64")
    bad = damaged_copy(good)
    planes_bad = orc.decode(bad)[1]
    assert orc.block_errors() > 0
    job.parse_batch([good, bad, good]).upload().run()
    t, status = job.to_tensor_resized((19, 23), None, "triangle", "float32", "NCHW", 1 / 255)
    assert status == [0, 0, 0] and job.block_errors() == orc.block_errors()
    want = rm.batch([orc.decode(good)[1], planes_bad, orc.decode(good)[1]], "gray", 8, "float32", "NCHW", (19, 23), None, rm.TRIANGLE, 1 / 255, 0.0)
    assert np.array_equal(tensor_bits(t), want) and not np.array_equal(want[0], want[1])
    # frames of different layouts in one job
    job.parse_batch([get("rgb_mct"), get("gray_l5_cb64")]).upload().run()
    with pytest.raises(m.Htj2kError) as e:
        job.to_tensor_resized((8, 8))
    assert e.value.code == EINVAL
    job.free()


def check_pipes(dec, orc, wait=60):
    """resized tensors in between plain receives, with a packet that fails to parse"""
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
                    bounded(lambda: pipe.receive_tensor_resized((4, 4)), wait)
                assert e.value.code < 0 and e.value.code != m.EAGAIN
                got += 1
                continue
            info_o, planes_o = want[got]
            fmt, bits = m.PIX_NAMES[info_o.pix_fmt], info_o.bits_per_raw_sample
            if got % 3 == 0:
                info, planes = bounded(pipe.receive, wait)
                assert all(np.array_equal(a, b) for a, b in zip(planes, planes_o)), got
            elif got % 3 == 1:
                window = None if got % 2 else (1, 1, info_o.width - 2, info_o.height - 3)
                filt = FILTERS[(got // 3) % 3]
                t, info = bounded(lambda: pipe.receive_tensor_resized((9, 6), window, m.RESIZE_FILTERS[filt], "float16", "NCHW", 1 / 255, -0.5), wait)
                assert (info.width, info.height, info.pix_fmt) == (info_o.width, info_o.height, info_o.pix_fmt), got
                assert np.array_equal(tensor_bits(t), rm.image(planes_o, fmt, bits, "float16", "NCHW", (9, 6), window, filt, 1 / 255, -0.5)[None]), got
            elif got == 8:                                   # a refusal consumes the frame
                with pytest.raises(m.Htj2kError) as e:
                    bounded(lambda: pipe.receive_tensor_resized((4, 4), (0, 0, info_o.width + 1, 1)), wait)
                assert e.value.code == EINVAL
            else:
                t, info = bounded(lambda: pipe.receive_tensor("float32", "NHWC"), wait)
                assert np.array_equal(tensor_bits(t), tm.image(planes_o, fmt, bits, "float32", "NHWC")[None]), got
            got += 1
        assert bounded(lambda: pipe.receive_tensor_resized((4, 4)), wait) is None and bounded(pipe.receive, wait) is None    # drained
    finally:
        bounded(pipe.close, wait)


def check_shared_context(dec):
    """a compare, an SSIM, a hash and a resized tensor call one after the other on one context, twice: they share
    MeasCall's buffers, and each must still give its model's answer"""
    from test_measure_shared_gpu import build_steps
    steps, keep = build_steps()
    rng = np.random.default_rng(8)
    fs = [HFrame("yuv420p", 70, 9, rng, "row+13", 1), HFrame("yuv420p", 33, 20, rng, "to64", 0)]
    want = rm.batch([f.arrays() for f in fs], "yuv420p", 8, "bfloat16", "NCHW", (32, 4), [(16, 2, 50, 7), (1, 3, 30, 17)], rm.TRIANGLE, 1 / 255, 0.0)
    for _ in range(2):
        for name, call, expect, same, exact, launches in steps:
            got = call(dec)
            assert same(got, expect), name
            check(dec, fs, "yuv420p", 8, (32, 4), [(16, 2, 50, 7), (1, 3, 30, 17)], rm.TRIANGLE, "bfloat16", "NCHW", 1 / 255, 0.0, want=want)
            assert dec.compare_ms() > 0
    del keep


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_filters_dtypes_layouts(dec, fmt):
    check_layout(dec, fmt, LAYOUTS.index(fmt))


@pytest.mark.gpu
def test_shapes_that_can_go_wrong(dec):
    check_shapes(dec)


@pytest.mark.gpu
def test_identity_windows_equal_the_plain_call(dec):
    check_identity(dec)


@pytest.mark.gpu
def test_unlike_frames_windows_and_reductions_in_one_call(dec):
    check_batches(dec)


@pytest.mark.gpu
def test_more_planes_than_one_launch_takes(dec):
    check_many_frames(dec)


@pytest.mark.gpu
def test_refusals_on_a_live_context(dec):
    check_refusals(dec)


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
def test_context_shared_with_the_measuring_calls(dec):
    check_shared_context(dec)


def run_everything(dec, orc):
    for i, fmt in enumerate(LAYOUTS):
        check_layout(dec, fmt, i)
    check_shapes(dec)
    check_identity(dec)
    check_batches(dec)
    check_many_frames(dec)
    check_refusals(dec)
    check_python(dec)
    check_jobs(dec, orc)
    check_pipes(dec, orc)
    check_shared_context(dec)


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
