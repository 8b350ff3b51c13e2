"""htj2k_frames_to_tensor / htj2k_job_to_tensor / htj2k_pipe_receive_tensor on the GPU against the numpy model
(tensor_model): every bit of every element, on both kernel routes.

Every layout family, three element types and two layouts; rows at the tails of the 16- and 48-byte groups, linesizes equal
to the row, row + 1, row + 13 and rounded to 64, base pointers off by 0, 1, 2 and 15 bytes, 0xAB dirt in the padding, host
and device operands; windows on and off group boundaries and chroma samples; destinations with 0xA5 guard zones; values
at the corners of the number formats; batches, more planes than grid.z takes, refusals on a live context, jobs, pipes,
and a context shared with the measuring calls.  The route every call took is asserted, and every call that took the fast
route is made again on the general one and compared bit for bit.  Run as a program, the module runs all of it on its own
contexts: test_everything_on_poisoned_buffers does that in a child process under HTJ2K_POISON=1."""
import ctypes
import os
import subprocess
import sys
import threading
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
import hash_model as hm
import oracle
import streams
import tensor_model as tm
from test_hash_gpu import HFrame, damaged_copy

LAYOUTS = ["gray", "gray16le", "ya8", "ya16le", "rgb24", "rgb48le", "rgba", "rgba64le", "yuv444p", "yuv444p16le", "yuv422p",
           "yuv422p10le", "yuv420p", "yuv420p16le", "yuva420p", "yuv411p", "yuv410p", "xyz12le"]
LS_MODES = ["row", "row+1", "row+13", "to64"]
OFFSETS = [0, 1, 2, 15]
HEIGHTS = [1, 2, 3, 5]
LAYOUT_NAMES = ["NCHW", "NHWC"]
# (scale, bias) as in test_tensor_host: normalisations, fp16 subnormals, fp16 +-inf, a negative scale, binary32
# subnormals, exact ties for fp16 and bf16 at 16 bits, results of exactly -0 and +0
PAIRS = [(1 / 255, 0.0), (1 / 1023, -0.5), (2.0 ** -20, 0.0), (3.0, -7.25), (-3.0, -7.25), (1 / (255 * 0.229), -0.485 / 0.229),
         (2.0 ** -134, 0.0), (2.0 ** -12, 0.0), (-1.0, -0.0), (-1.0, 0.0)]
EINVAL, PATCHWELCOME = -22, -0x45574150
GUARD, SURPLUS = 4096, 48
FAST, GENERAL = 1, 2
CALLS = {"n": 0, "fast": 0, "general": 0}               # what the module did, for the program's last line


def low_bits(fmt):
    """a depth below the layout's own: the sample then sits among bits that are not part of it"""
    return {"rgb48le": 12, "yuv422p10le": 9}.get(fmt, cm.LAYOUTS[fmt][4] - 1)


def group_pixels(fmt):
    """pixels of a lane's group on the fast route"""
    nc, planar, _, _, _, b = cm.LAYOUTS[fmt]
    step = 1 if planar else nc
    return (48 if step == 3 else 16) // (step * b)


def expected_route(frames, fmt, layout, origins, on_device, path=0):
    """the header's rule, restated: a plane is on the fast route when it has no chroma shift, its window starts on a
    group boundary of the source row and its base and linesize are multiples of 16 (a host operand is uploaded to such a
    place), NHWC only when the plane holds all channels"""
    nc, planar, cw, ch, _, b = cm.LAYOUTS[fmt]
    step = 1 if planar else nc
    group = 48 if step == 3 else 16
    route = 0
    for i, f in enumerate(frames):
        ox = origins[i][0] if origins is not None else 0
        for p in range(len(f.geo)):
            k = p if planar else 0
            shifted = k in (1, 2) and (cw or ch)
            aligned = (not on_device) or (f.off % 16 == 0 and f.ls[p] % 16 == 0)
            fast = path == 0 and not shifted and not (layout == "NHWC" and planar and nc > 1) and (ox * step * b) % group == 0 and aligned
            route |= FAST if fast else GENERAL
    return route


def raw_call(dec, arr, on_device, n, bits, spec, origins, nbytes, dst_off_bytes=0, fill=0xA5):
    """the C call on a destination between two guard zones, `SURPLUS` bytes larger than needed -> (return value, the whole
    buffer as a host array, where the images start in it)"""
    at = GUARD + dst_off_bytes
    buf = torch.full((at + nbytes + SURPLUS + GUARD,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    org = None if origins is None else (ctypes.c_int32 * (2 * len(origins)))(*[int(v) for o in origins for v in o])
    torch.cuda.synchronize()
    r = dec.L.htj2k_frames_to_tensor(dec.h, arr, int(on_device), n, int(bits), ctypes.byref(spec), org,
                                     ctypes.c_void_p(buf.data_ptr() + at), ctypes.c_size_t(nbytes + SURPLUS))
    return r, buf.cpu().numpy(), at


def convert(dec, frames, fmt, bits, dtype, layout, size, origins, scale, bias, on_device, dst_off=0):
    """-> (bit patterns shaped as the model's, route); the guards and the surplus bytes must still be 0xA5"""
    n, nc = len(frames), tm.ncomp(fmt)
    ow, oh = size if size is not None else (frames[0].w, frames[0].h)
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
    r, host, at = raw_call(dec, arr, on_device, n, bits, spec, origins, nbytes, dst_off * es)
    assert r == 0, (r, fmt, dtype, layout, size, origins)
    assert (host[:at] == 0xA5).all(), "bytes in front of dst were written"
    assert (host[at + nbytes:] == 0xA5).all(), "bytes beyond the images were written"
    shape = (n, nc, oh, ow) if layout == "NCHW" else (n, oh, ow, nc)
    route = dec.tensor_last_route()
    CALLS["n"] += 1
    CALLS["fast"] += bool(route & FAST)
    CALLS["general"] += bool(route & GENERAL)
    del keep
    return host[at:at + nbytes].view(tm.BITS_DTYPE[dtype]).reshape(shape), route


def check(dec, frames, fmt, bits, dtype="float16", layout="NCHW", size=None, origins=None, scale=None, bias=None,
          on_device=False, dst_off=0, want=None):
    """one call against the model, its route against the rule, and once more on the general route if it took the fast one"""
    if want is None:
        want = tm.batch([f.arrays() for f in frames], fmt, bits, dtype, layout, size, origins, scale, bias)
    what = (fmt, bits, dtype, layout, size, origins, scale, bias, on_device, dst_off, [(f.w, f.h, f.ls, f.off) for f in frames[:4]])
    got, route = convert(dec, frames, fmt, bits, dtype, layout, size, origins, scale, bias, on_device, dst_off)
    assert route == expected_route(frames, fmt, layout, origins, on_device), (route, what)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, route, len(bad), bad[:4].tolist(), [hex(int(got[tuple(b)])) for b in bad[:4]],
                           [hex(int(want[tuple(b)])) for b in bad[:4]])
    if route & FAST:
        dec.set_int("tensor_path", 1)
        try:
            again, r2 = convert(dec, frames, fmt, bits, dtype, layout, size, origins, scale, bias, on_device, dst_off)
        finally:
            dec.set_int("tensor_path", 0)
        assert r2 == GENERAL and np.array_equal(again, got), (what, r2)
    return route


def check_layout(dec, fmt, li):
    """full frames whose rows end at every tail of the groups, on every linesize, offset, element and layout"""
    depth = cm.LAYOUTS[fmt][4]
    gp = group_pixels(fmt)
    widths = [1, 5, 15, 16, 17, 47, 48, 49, 64 * gp - 1, 64 * gp + 1]
    routes = 0
    for i, w in enumerate(widths):
        h = HEIGHTS[(i + li) % 4]
        bits = low_bits(fmt) if i % 5 == 4 else depth
        scale, bias = PAIRS[(i + li) % len(PAIRS)]
        for k, on_device in enumerate((False, True)):
            f = HFrame(fmt, w, h, np.random.default_rng(1000 * li + 10 * i + k), LS_MODES[(i + li + k) % 4], OFFSETS[(i // 2 + li + 3 * k) % 4])
            routes |= check(dec, [f], fmt, bits, tm.DTYPES[(i + k) % 3], LAYOUT_NAMES[(i // 3 + k) % 2], None, None, scale, bias, on_device)
    assert routes == FAST | GENERAL, (fmt, routes)


def check_windows(dec, fmt, li):
    """windows that start on and off a group boundary and on and off a chroma sample, destination rows that are and are not
    multiples of 16 bytes, a destination off by one element; every element type and layout on each"""
    depth = cm.LAYOUTS[fmt][4]
    w, h = 41, 11
    gp = group_pixels(fmt)
    on = gp if gp <= 16 else 16                           # an origin on a group boundary
    windows = [(None, None), ((1, 1), (40, 10)), ((8, 5), (3, 1)), ((7, 4), (4, 2)), ((8, 4), (on, 3)), ((24, 2), (on, 6)),
               ((16, 3), (2 * on if 2 * on + 16 <= w else on, 7))]
    for k, on_device in enumerate((False, True)):
        f = HFrame(fmt, w, h, np.random.default_rng(77 + li + k), "to64" if on_device else "row+1", 0 if on_device else 1)
        planes = f.arrays()
        for j, (size, origin) in enumerate(windows):
            origins = None if origin is None else [origin]
            for d, dtype in enumerate(tm.DTYPES):
                for layout in LAYOUT_NAMES:
                    want = tm.image(planes, fmt, depth, dtype, layout, size, origin or (0, 0), 1 / 255, -0.5)[None]
                    check(dec, [f], fmt, depth, dtype, layout, size, origins, 1 / 255, -0.5, on_device, dst_off=(j + d) % 2, want=want)


def check_values(dec):
    """all 65536 samples of a 16-bit layout and all 256 of an 8-bit one through every scale / bias pair and element type;
    a scale and a bias of its own for every channel"""
    rng = np.random.default_rng(5)
    f16 = HFrame("gray16le", 256, 256, rng)
    vals = rng.permutation(65536).astype("<u2")
    f16.bufs[0][:65536 * 2] = vals.view(np.uint8)           # linesize = row, offset 0: the buffer is the plane
    f8 = HFrame("gray", 16, 16, rng)
    f8.bufs[0][:256] = rng.permutation(256).astype(np.uint8)
    assert np.array_equal(np.sort(f16.arrays()[0].ravel()), np.arange(65536)) and np.array_equal(np.sort(f8.arrays()[0].ravel()), np.arange(256))
    for scale, bias in PAIRS:
        for dtype in tm.DTYPES:
            check(dec, [f16], "gray16le", 16, dtype, "NCHW", None, None, scale, bias)
            check(dec, [f8], "gray", 8, dtype, "NHWC", None, None, scale, bias)
    want = tm.image(f16.arrays(), "gray16le", 16, "float16", "NCHW", None, (0, 0), 3.0, -7.25)
    assert (want == 0x7C00).any()                           # the model itself overflows to +inf here
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    for fmt, bits in (("rgb48le", 16), ("rgb24", 8), ("yuv444p", 8), ("rgba", 8), ("ya16le", 16)):
        nc = tm.ncomp(fmt)
        peak = (1 << bits) - 1
        scale = [1 / (peak * s) for s in (std + [0.5])[:nc]]
        bias = [-a / s for a, s in zip((mean + [0.25])[:nc], (std + [0.5])[:nc])]
        f = HFrame(fmt, 64, 9, rng, "to64")
        for dtype in tm.DTYPES:
            for layout in LAYOUT_NAMES:
                for on_device in (False, True):
                    check(dec, [f], fmt, bits, dtype, layout, None, None, scale, bias, on_device)


def check_batches(dec):
    """frames of different sizes with one window and an origin each; one frame; unlike routes in one call"""
    rng = np.random.default_rng(21)
    for fmt, bits in (("rgb24", 8), ("yuv420p", 8), ("gray16le", 12), ("rgba64le", 16), ("yuv422p10le", 10)):
        gp = group_pixels(fmt)
        sizes = [(40, 9), (33, 12), (64, 7), (17, 5)]
        origins = [(gp if gp <= 16 else 16, 2), (3, 0), (32, 1), (0, 0)]
        for on_device in (False, True):
            fs = [HFrame(fmt, w, h, rng, "to64" if i % 2 == 0 else "row+1", 0 if i != 3 else 1) for i, (w, h) in enumerate(sizes)]
            for dtype, layout in (("float16", "NCHW"), ("float32", "NHWC"), ("bfloat16", "NCHW")):
                route = check(dec, fs, fmt, bits, dtype, layout, (16, 5), origins, 1 / 255, 0.0, on_device)
                if not (layout == "NHWC" and cm.LAYOUTS[fmt][1]):
                    assert route == FAST | GENERAL, (fmt, route)   # origin 3 is off every group boundary, 0 is on it
            check(dec, fs[:1], fmt, bits, "float16", "NCHW", None, None, 1.0, 0.0, on_device)
    same = [HFrame("rgb24", 32, 4, rng, "to64") for _ in range(5)]
    assert check(dec, same, "rgb24", 8, "float32", "NCHW", None, None, 2.0, 1.0, True) == FAST


def check_many_frames(dec, n=70000):
    """more planes than grid.z takes in one launch: 8 x 8 gray frames out of one buffer"""
    a = np.random.default_rng(9).integers(0, 256, size=(n, 64), dtype=np.uint8)
    rec = np.dtype({"names": ["data", "linesize", "width", "height", "pix_fmt"], "formats": [("<u8", 4), ("<i4", 4), "<i4", "<i4", "<i4"],
                    "offsets": [0, 32, 48, 52, 56], "itemsize": ctypes.sizeof(m.Frame)})
    t = np.zeros(n, rec)
    t["data"][:, 0] = a.ctypes.data + 64 * np.arange(n, dtype=np.uint64)
    t["linesize"][:, 0] = 8
    t["width"], t["height"], t["pix_fmt"] = 8, 8, m.PIX_NAMES.index("gray")
    for path, dtype in ((0, "float16"), (1, "bfloat16")):
        spec = m.tensor_spec(dtype, "NCHW", None, 1 / 255, -0.5)
        dec.set_int("tensor_path", path)
        try:
            r, host, at = raw_call(dec, t.ctypes.data_as(ctypes.c_void_p), 0, n, 8, spec, None, n * 128)
        finally:
            dec.set_int("tensor_path", 0)
        assert r == 0 and dec.tensor_last_route() == (GENERAL if path else FAST)
        assert (host[:at] == 0xA5).all() and (host[at + n * 128:] == 0xA5).all()
        assert np.array_equal(host[at:at + n * 128].view(np.uint16).reshape(n, 64), tm.value_bits(a, 1 / 255, -0.5, dtype))


def check_refusals(dec):
    """every refusal on a live context: nothing launched, dst and its guards untouched, route 0, and the context works on"""
    rng = np.random.default_rng(3)
    f = HFrame("yuv420p", 20, 10, rng)
    other = HFrame("yuv422p", 20, 10, rng)
    wider = HFrame("yuv420p", 21, 10, rng)
    pal = HFrame("pal8", 20, 10, rng)
    ok = m.tensor_spec("float16")
    win = m.tensor_spec("float16", size=(4, 4))
    need = 3 * 20 * 10 * 2

    def spec(**kw):
        s = m.tensor_spec("float16")
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def floats(field, k, v):
        s = m.tensor_spec("float16")
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

    cases = [  # (frames, n or None, bits, spec, origins, bytes of dst, offset of dst, what it answers)
        ([f.frame()], 0, 8, ok, None, need, 0, EINVAL),
        ([pal.frame()], None, 8, ok, None, need, 0, PATCHWELCOME),
        ([f.frame()], None, 9, ok, None, need, 0, EINVAL),
        ([f.frame()], None, 0, ok, None, need, 0, EINVAL),
        ([f.frame()], None, 8, spec(dtype=3), None, need, 0, EINVAL),
        ([f.frame()], None, 8, spec(layout=2), None, need, 0, EINVAL),
        ([f.frame()], None, 8, floats("scale", 2, float("nan")), None, need, 0, EINVAL),
        ([f.frame()], None, 8, floats("bias", 0, float("inf")), None, need, 0, EINVAL),
        ([f.frame()], None, 8, spec(out_w=4, out_h=0), None, need, 0, EINVAL),
        ([f.frame(), other.frame()], None, 8, ok, None, 2 * need, 0, EINVAL),
        ([f.frame(), wider.frame()], None, 8, ok, None, 2 * need, 0, EINVAL),
        ([frame_with(f, data_1=None)], None, 8, ok, None, need, 0, EINVAL),
        ([frame_with(f, linesize_0=19)], None, 8, ok, None, need, 0, EINVAL),
        ([frame_with(f, linesize_2=-10)], None, 8, ok, None, need, 0, EINVAL),
        ([f.frame()], None, 8, win, [(-1, 0)], need, 0, EINVAL),
        ([f.frame()], None, 8, win, [(17, 0)], need, 0, EINVAL),
        ([f.frame()], None, 8, win, [(0, 7)], need, 0, EINVAL),
        ([f.frame()], None, 8, ok, None, need - 1 - SURPLUS, 0, EINVAL),
        ([f.frame()], None, 8, ok, None, need, 1, EINVAL),
        ([f.frame()], None, 8, m.tensor_spec("float32"), None, 2 * need, 2, EINVAL),
    ]
    for i, (frames, n, bits, s, origins, nbytes, off, answer) in enumerate(cases):
        check(dec, [f], "yuv420p", 8)                          # a call that launches, so that a route is there to be cleared
        arr = (m.Frame * len(frames))(*frames)
        r, host, at = raw_call(dec, arr, 0, len(frames) if n is None else n, bits, s, origins, nbytes, off)
        assert r == answer, (i, r)
        assert (host == 0xA5).all(), i
        assert dec.tensor_last_route() == 0, i
    with pytest.raises(m.Htj2kError) as e:
        dec.set_int("tensor_path", 2)
    assert e.value.code == EINVAL
    with pytest.raises(m.Htj2kError):
        dec.set_int("tensor_path", -1)
    check(dec, [f], "yuv420p", 8, "float32", "NHWC")             # the context still works


def tensor_bits(t):
    """a torch tensor's bit patterns as the model states them"""
    return (t.view(torch.int32).cpu().numpy().view(np.uint32) if t.dtype == torch.float32 else t.view(torch.int16).cpu().numpy().view(np.uint16))


def check_python(dec):
    """Decoder.to_tensor: numpy planes in, a torch tensor out; `out` is checked"""
    rng = np.random.default_rng(12)
    fs = [HFrame("rgb24", 33, 6, rng), HFrame("rgb24", 33, 6, rng)]
    planes = [f.arrays() for f in fs]
    t = dec.to_tensor(planes, "rgb24", 8, scale=1 / 255)
    assert t.dtype == torch.float16 and tuple(t.shape) == (2, 3, 6, 33) and t.is_contiguous() and t.is_cuda
    assert np.array_equal(tensor_bits(t), tm.batch(planes, "rgb24", 8, "float16", "NCHW", None, None, 1 / 255, 0.0))
    assert dec.tensor_last_route() == FAST and dec.compare_ms() > 0
    assert torch.equal(t.float().cpu(), torch.from_numpy(np.stack([p[0].reshape(6, 33, 3).transpose(2, 0, 1) for p in planes]).astype(np.float32) *
                                                         np.float32(1 / 255)).to(torch.float16).float())
    out = torch.zeros((2, 4, 5, 3), dtype=torch.bfloat16, device="cuda")
    t2 = dec.to_tensor(planes, "rgb24", 8, torch.bfloat16, "NHWC", size=(5, 4), origins=(7, 1), scale=[1, 2, 3], bias=0.5, out=out)
    assert t2 is out
    assert np.array_equal(tensor_bits(out), tm.batch(planes, "rgb24", 8, "bfloat16", "NHWC", (5, 4), [(7, 1)] * 2, [1, 2, 3], 0.5))
    t3 = dec.to_tensor(planes, "rgb24", 8, np.float32, origins=[(0, 0), (1, 2)], size=(32, 4))
    assert np.array_equal(tensor_bits(t3), tm.batch(planes, "rgb24", 8, "float32", "NCHW", (32, 4), [(0, 0), (1, 2)]))
    devs = [f.on_device() for f in fs]
    t4 = dec.to_tensor([d for d, _ in devs], "rgb24", 8, "float32", on_device=True)
    assert np.array_equal(tensor_bits(t4), tm.batch(planes, "rgb24", 8, "float32"))
    for bad in (torch.zeros((2, 4, 5, 3), dtype=torch.float16, device="cuda"), torch.zeros((2, 4, 5, 4), dtype=torch.bfloat16, device="cuda"),
                torch.zeros((2, 4, 5, 3), dtype=torch.bfloat16), torch.zeros((2, 4, 5, 6), dtype=torch.bfloat16, device="cuda")[..., ::2]):
        with pytest.raises(ValueError):
            dec.to_tensor(planes, "rgb24", 8, torch.bfloat16, "NHWC", size=(5, 4), out=bad)
    assert m.Decoder.tensor_image_size("rgb24", 33, 6, 8, m.tensor_spec("float16")) == (3 * 33 * 6, 3 * 33 * 6 * 2)


def yuv422p10_stream():
    return streams._enc((64, 48, 3, 10, 11, 30, (1, 2, 2), (1, 1, 1)), depth=10, dx=[1, 2, 2], dy=[1, 1, 1], width=64, height=48)


def check_jobs(dec, orc):
    get = lambda name: streams.get(name)[0]
    groups = [("rgb24", [get("rgb_mct"), get("rgb_tiles")]), ("yuv420p", [get("yuv420p8"), get("yuv420p8")]),
              ("yuv422p10le", [yuv422p10_stream()] * 2), ("gray16le", [get("gray16")] * 2)]
    job = dec.job()
    for li, (fmt, datas) in enumerate(groups):
        job.parse_batch(datas)
        with pytest.raises(m.Htj2kError) as e:               # before the upload
            job.to_tensor()
        assert e.value.code == EINVAL and dec.tensor_last_route() == 0
        job.upload()
        with pytest.raises(m.Htj2kError) as e:               # before the first run
            job.to_tensor()
        assert e.value.code == EINVAL
        job.run()
        info = job.frame_info(0)
        assert m.PIX_NAMES[info.pix_fmt] == fmt
        bits = info.bits_per_raw_sample
        want_planes = [orc.decode(d)[1] for d in datas]
        scale = 1 / ((1 << bits) - 1)
        t, status = job.to_tensor("float16", "NCHW", scale=scale)                      # bits 0: the job's
        assert status == [0, 0] and tuple(t.shape) == (2, tm.ncomp(fmt), info.height, info.width)
        assert np.array_equal(tensor_bits(t), tm.batch(want_planes, fmt, bits, "float16", "NCHW", None, None, scale, 0.0)), fmt
        t, status = job.to_tensor("float32", "NHWC", size=(24, 10), origins=[(16, 3), (5, 1)], scale=scale, bias=-0.5, bits=bits)
        assert np.array_equal(tensor_bits(t), tm.batch(want_planes, fmt, bits, "float32", "NHWC", (24, 10), [(16, 3), (5, 1)], scale, -0.5)), fmt
        t, status = job.to_tensor("bfloat16", "NCHW", size=(1, 1), origins=(info.width - 1, info.height - 1), bits=bits - 1)
        assert np.array_equal(tensor_bits(t), tm.batch(want_planes, fmt, bits - 1, "bfloat16", "NCHW", (1, 1), [(info.width - 1, info.height - 1)] * 2)), fmt
        assert dec.tensor_last_route() == GENERAL
        with pytest.raises(m.Htj2kError) as e:               # a window that leaves the frame
            job.to_tensor(size=(info.width, 2), origins=(1, 0))
        assert e.value.code == EINVAL and dec.tensor_last_route() == 0
        job.run(stages=3)                                    # a run that did not write the frames
        with pytest.raises(m.Htj2kError) as e:
            job.to_tensor()
        assert e.value.code == EINVAL
    # blocks that the decoder rejects stay zero: the frame is still a frame, and is converted
    good = get("gray_l5_cb64")
    bad = damaged_copy(good)
    planes_bad = orc.decode(bad)[1]
    assert orc.block_errors() > 0
    job.parse_batch([good, bad, good]).upload().run()
    t, status = job.to_tensor("float32", "NCHW", scale=1 / 255)
    assert status == [0, 0, 0] and job.block_errors() == orc.block_errors()
    want = tm.batch([orc.decode(good)[1], planes_bad, orc.decode(good)[1]], "gray", 8, "float32", "NCHW", None, None, 1 / 255, 0.0)
    assert np.array_equal(tensor_bits(t), want) and not np.array_equal(want[0], want[1])
    # frames of different layouts in one job
    job.parse_batch([get("rgb_mct"), get("gray_l5_cb64")]).upload().run()
    with pytest.raises(m.Htj2kError) as e:
        job.to_tensor(size=(8, 8))
    assert e.value.code == EINVAL
    job.free()


def bounded(fn, seconds):
    """fn() on a thread of its own, given up after `seconds`: a pipe that is stuck fails the test instead of holding it"""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:                           # noqa: B902  (handed to the caller)
            box["error"] = e

    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(seconds)
    assert not th.is_alive(), "a pipe operation did not come back within %d s" % seconds
    if "error" in box:
        raise box["error"]
    return box.get("value")


def check_pipes(dec, orc, wait=60):
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
            mode = got % 4
            if got == 5:
                with pytest.raises(m.Htj2kError) as e:       # its own error, and the pipe moves on
                    bounded(pipe.receive, wait)
                assert e.value.code < 0 and e.value.code != m.EAGAIN
                got += 1
                continue
            info_o, planes_o = want[got]
            fmt, bits = m.PIX_NAMES[info_o.pix_fmt], info_o.bits_per_raw_sample
            if mode == 0:
                size, origin = ((5, 4), (2, 1)) if got == 8 else (None, None)
                t, info = bounded(lambda: pipe.receive_tensor("float16", "NCHW", size=size, origin=origin, scale=1 / 255, bias=-0.5), wait)
                assert (info.width, info.height, info.pix_fmt) == (info_o.width, info_o.height, info_o.pix_fmt), got
                assert np.array_equal(tensor_bits(t), tm.image(planes_o, fmt, bits, "float16", "NCHW", size, origin or (0, 0), 1 / 255, -0.5)[None]), got
            elif mode == 1:
                info, planes = bounded(pipe.receive, wait)
                assert all(np.array_equal(a, b) for a, b in zip(planes, planes_o)), got
            elif mode == 2:
                info, h = bounded(pipe.receive_crc, wait)
                assert h == hm.frame_hash(planes_o, info) and h["adler32"] == oracle.framecrc(planes_o), got
            else:
                info = m.Info()
                assert bounded(lambda: dec.L.htj2k_pipe_info(pipe.h, ctypes.byref(info)), wait) == 0
                fr = bounded(pipe.receive_device, wait)
                assert all(np.array_equal(a, b) for a, b in zip(dec.fetch_device_frame(info, fr), planes_o)), got
                # the frame that was handed out, read in place: NHWC float32 of an interleaved layout or a single plane
                t = dec.to_tensor([fr], fmt, bits, "float32", "NHWC", on_device=True)
                assert np.array_equal(tensor_bits(t), tm.image(planes_o, fmt, bits, "float32", "NHWC")[None]), got
            got += 1
        assert bounded(pipe.receive_tensor, wait) is None and bounded(pipe.receive, wait) is None    # drained
    finally:
        bounded(pipe.close, wait)


def check_shared_context(dec):
    """a compare, an SSIM, a hash and a tensor call one after the other on one context, twice: they share MeasCall's
    buffers, and each must still give its model's answer"""
    from test_measure_shared_gpu import build_steps
    steps, keep = build_steps()
    rng = np.random.default_rng(8)
    fs = [HFrame("yuv420p", 70, 9, rng, "row+13", 1), HFrame("yuv420p", 70, 9, rng, "to64", 0)]
    for _ in range(2):
        for name, call, want, same, exact, launches in steps:
            got = call(dec)
            assert same(got, want), name
            assert check(dec, fs, "yuv420p", 8, "bfloat16", "NCHW", (32, 4), [(16, 2), (16, 3)], 1 / 255, 0.0) == FAST | GENERAL
            assert dec.compare_ms() > 0
    del keep


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_layouts_rows_linesizes_offsets(dec, fmt):
    check_layout(dec, fmt, LAYOUTS.index(fmt))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_windows(dec, fmt):
    check_windows(dec, fmt, LAYOUTS.index(fmt))


@pytest.mark.gpu
def test_values_at_the_corners_of_the_formats(dec):
    check_values(dec)


@pytest.mark.gpu
def test_batches_of_unlike_frames(dec):
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
        check_windows(dec, fmt, i)
    check_values(dec)
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
    print("%s buffers: ok, %.1f s, %d calls (%d with the fast route, %d with the general one)"
          % ("poisoned" if os.environ.get("HTJ2K_POISON") == "1" else "plain", time.time() - t0, CALLS["n"], CALLS["fast"], CALLS["general"]))
