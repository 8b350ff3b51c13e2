"""The tensor calls with a colour matrix on the GPU against the numpy model (mix_model): every bit of every element, on
both routes of the plain kernel and through the scratch pass of the resized calls.

Seventeen layouts over three element types, two tensor layouts and K = 1 .. 4; rows at the tails of the pixel groups,
linesizes and bases off the 16-byte alignment on host and device operands, 0xAB dirt in the padding, destinations between
0xA5 guard zones and at odd element offsets; windows on and off the group boundary, odd origins on sub-sampled chroma;
weights at the corners of the number formats with signed zeros compared as bits; the torch eager chain on the device; the
identity mix against the plain call; resized calls with chunk seams in the scratch; batches, more frames than grid.z takes,
jobs, a pipe with a damaged packet, refusals on a live context.  The route of every call is asserted against the rule
restated here, and every call that took the fast route is made again on the general one and compared bit for bit.  Run as a
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
import mix_model as mm
import oracle
import resize_model as rm
import streams
import tensor_model as tm
from test_hash_gpu import HFrame, damaged_copy
from test_tensor_gpu import bounded, tensor_bits, yuv422p10_stream

LAYOUTS = ["rgb24", "rgb48le", "rgba", "rgba64le", "gray", "ya8", "yuv420p", "yuv422p", "yuv444p", "yuv422p10le", "yuv420p12le",
           "yuv444p16le", "yuva420p", "yuva444p10le", "yuv410p", "yuv411p", "xyz12le"]
WIDTHS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 65, 130]
LS_MODES = ["row", "row+1", "row+13", "to64"]
OFFSETS = [0, 1, 2, 15]
LAYOUT_NAMES = ["NCHW", "NHWC"]
EINVAL, PATCHWELCOME = -22, -0x45574150
GUARD, SURPLUS = 4096, 48
FAST, GENERAL, RESIZED = 5, 6, 8
CALLS = {"n": 0, "fast": 0, "general": 0, "resized": 0}


def group_pixels(fmt):
    """pixels of a lane's group on the fast route; 0: the layout has none (a horizontal chroma shift above 1)"""
    nc, planar, cw, _, _, b = cm.LAYOUTS[fmt]
    if planar and nc > 1:
        return (16 << cw) // b if cw <= 1 else 0
    return (48 if nc == 3 else 16) // (nc * b)


def expected_route(frames, fmt, origins, on_device, path=0):
    """the header's rule, restated: a frame is on the fast route when its layout is interleaved or planar with a horizontal
    chroma shift of 0 or 1, its window starts on a boundary of the pixel group and every plane's base and linesize are
    multiples of 16 (a host operand is uploaded to such a place); any oy, both tensor layouts, every K"""
    gp = group_pixels(fmt)
    route = 0
    for i, f in enumerate(frames):
        ox = origins[i][0] if origins is not None else 0
        aligned = (not on_device) or (f.off % 16 == 0 and all(ls % 16 == 0 for ls in f.ls))
        route |= 1 if (path == 0 and gp and ox % gp == 0 and aligned) else 2
    return 4 + route


def make_mix(kind, nc, k, seed=0):
    """a K x C mix of one of the kinds the tests walk"""
    rng = np.random.default_rng(1000 * nc + 10 * k + seed)
    if kind == "rand":
        return m.tensor_mix(rng.normal(0, 1 / 64, (k, nc)), rng.normal(0, 1, k))
    if kind == "zero":                                       # all-zero rows: b alone, and +0 from +0 products
        return m.tensor_mix(np.zeros((k, nc)), [0.0, -0.0, 0.25, -3.0][:k])
    if kind == "negzero":                                    # -0 products: -0 with a -0 offset, +0 with a +0 offset
        return m.tensor_mix(np.full((k, nc), -0.0), [-0.0, 0.0, -0.0, 0.0][:k])
    if kind == "big":                                        # float16 overflows to infinities of both signs
        return m.tensor_mix(np.where(np.arange(k)[:, None] % 2 == 0, 1.0e4, -1.0e4) * np.ones((k, nc)), np.zeros(k))
    if kind == "tiny":                                       # float16 subnormals, and binary32 subnormals in row 1
        a = np.full((k, nc), 2.0 ** -22)
        a[1 % k] = 2.0 ** -140
        return m.tensor_mix(a, np.zeros(k))
    if kind == "ties":                                       # one term: exact ties for float16 and bfloat16
        a = np.zeros((k, nc))
        a[:, 0] = 2.0 ** -12
        return m.tensor_mix(a, np.zeros(k))
    if kind == "perm":                                       # BGR, alpha dropped or passed: channels reversed
        return m.tensor_mix(np.eye(nc)[::-1][:k] if k <= nc else np.vstack([np.eye(nc)[::-1], np.zeros((k - nc, nc))]), np.zeros(k))
    raise ValueError(kind)


KINDS = ["rand", "zero", "negzero", "big", "tiny", "ties", "perm"]


def raw_call(dec, arr, on_device, n, bits, spec, mix, origins, nbytes, dst_off_bytes=0, windows=None, filt=None):
    """the C call on a destination between two guard zones, `SURPLUS` bytes larger than needed -> (return value, the whole
    buffer as a host array, where the images start in it).  filt: the resized call with `windows`"""
    at = GUARD + dst_off_bytes
    buf = torch.full((at + nbytes + SURPLUS + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    mp = None if mix is None else ctypes.byref(mix)
    torch.cuda.synchronize()
    if filt is None:
        org = None if origins is None else (ctypes.c_int32 * (2 * len(origins)))(*[int(v) for o in origins for v in o])
        r = dec.L.htj2k_frames_to_tensor_mix(dec.h, arr, int(on_device), n, int(bits), ctypes.byref(spec), mp, org,
                                             ctypes.c_void_p(buf.data_ptr() + at), ctypes.c_size_t(nbytes + SURPLUS))
    else:
        win = None if windows is None else (ctypes.c_int32 * (4 * len(windows)))(*[int(v) for w in windows for v in w])
        r = dec.L.htj2k_frames_to_tensor_resized_mix(dec.h, arr, int(on_device), n, int(bits), ctypes.byref(spec), mp, win, int(filt),
                                                     ctypes.c_void_p(buf.data_ptr() + at), ctypes.c_size_t(nbytes + SURPLUS))
    return r, buf.cpu().numpy(), at


def convert(dec, frames, fmt, bits, mix, dtype, layout, size, origins, on_device, dst_off=0, windows=None, filt=None):
    """-> (bit patterns shaped as the model's, route); the guards and the surplus bytes must still be 0xA5.  mix None: the
    plain call through the same entry point, at scale 1 and bias 0"""
    n, k = len(frames), (mix.nout if mix is not None else tm.ncomp(fmt))
    ow, oh = size if size is not None else (frames[0].w, frames[0].h)
    es = tm.ESIZE[dtype]
    nbytes = n * k * ow * oh * es
    spec = m.tensor_spec(dtype, layout, size)
    keep = []
    if on_device:
        made = [f.on_device() for f in frames]
        keep = [t for _, t in made]
        arr = (m.Frame * n)(*[fr for fr, _ in made])
    else:
        arr = (m.Frame * n)(*[f.frame() for f in frames])
    r, host, at = raw_call(dec, arr, on_device, n, bits, spec, mix, origins, nbytes, dst_off * es, windows, filt)
    assert r == 0, (r, fmt, dtype, layout, size, origins, windows)
    assert (host[:at] == 0xA5).all(), "bytes in front of dst were written"
    assert (host[at + nbytes:] == 0xA5).all(), "bytes beyond the images were written"
    shape = (n, k, oh, ow) if layout == "NCHW" else (n, oh, ow, k)
    route = dec.tensor_last_route()
    CALLS["n"] += 1
    CALLS["fast"] += route in (5, 7)
    CALLS["general"] += route in (6, 7)
    CALLS["resized"] += route == 8
    del keep
    return host[at:at + nbytes].view(tm.BITS_DTYPE[dtype]).reshape(shape), route


def mismatch(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [hex(int(got[tuple(b)])) for b in bad[:4]], [hex(int(want[tuple(b)])) for b in bad[:4]])


def check(dec, frames, fmt, bits, mix, dtype="float16", layout="NCHW", size=None, origins=None, on_device=False, dst_off=0, want=None):
    """one call against the model, its route against the rule, and once more on the general route if it took the fast one"""
    if want is None:
        want = mm.batch([f.arrays() for f in frames], fmt, bits, mix, dtype, layout, size, origins)
    what = (fmt, bits, mix.nout, dtype, layout, size, origins, on_device, dst_off, [(f.w, f.h, f.ls, f.off) for f in frames[:4]])
    got, route = convert(dec, frames, fmt, bits, mix, dtype, layout, size, origins, on_device, dst_off)
    assert route == expected_route(frames, fmt, origins, on_device), (route, what)
    mismatch(got, want, (what, route))
    if route in (5, 7):
        dec.set_int("tensor_path", 1)
        try:
            again, r2 = convert(dec, frames, fmt, bits, mix, dtype, layout, size, origins, on_device, dst_off)
        finally:
            dec.set_int("tensor_path", 0)
        assert r2 == GENERAL and np.array_equal(again, got), (what, r2)
    return route


def layout_cases(fmt, li):
    """the sweep of one layout: (w, h, bits, kind, K, dtype, tensor layout, on_device, linesize mode, offset).  Every width
    twice, on a host operand (uploaded: the fast route where the layout has one) and on a device operand whose base or
    linesize is off the alignment for three K in four"""
    depth = cm.LAYOUTS[fmt][4]
    for i, w in enumerate(WIDTHS):
        h = 1 + (i + li) % 5
        bits = depth - 1 if i % 5 == 4 else depth
        for d, on_device in enumerate((False, True)):
            j = 2 * i + d
            k = 1 + (i + d + li + i // 4) % 4
            off = OFFSETS[(i + li) % 4] if on_device else OFFSETS[(i + 1) % 4]
            ls = "to64" if (on_device and i % 4 == 3) else LS_MODES[(i + li + d) % 4]
            if on_device and i % 4 == 3:
                off = 0                                      # a device operand on the fast route
            yield w, h, bits, KINDS[(j + li) % len(KINDS)], k, tm.DTYPES[(j + li) % 3], LAYOUT_NAMES[(j // 3 + li) % 2], on_device, ls, off


def check_layout(dec, fmt, li):
    nc = tm.ncomp(fmt)
    seen = set()
    for c, (w, h, bits, kind, k, dtype, layout, on_device, ls, off) in enumerate(layout_cases(fmt, li)):
        f = HFrame(fmt, w, h, np.random.default_rng(1000 * li + c), ls, off)
        route = check(dec, [f], fmt, bits, make_mix(kind, nc, k, c), dtype, layout, None, None, on_device)
        seen.add((route, k))
        seen.add((dtype, layout if k > 1 else "NCHW"))
    for k in range(1, 5):
        assert (GENERAL, k) in seen and (not group_pixels(fmt) or (FAST, k) in seen), (fmt, k, sorted(map(str, seen)))
    for dtype in tm.DTYPES:
        assert (dtype, "NCHW") in seen and (dtype, "NHWC") in seen, (fmt, dtype)


def check_windows(dec, fmt, li):
    """windows that start on and off a group boundary and on and off a chroma sample, oy odd on vertically sub-sampled
    chroma, destination rows that are and are not multiples of 16 bytes, a destination off by one element"""
    depth = cm.LAYOUTS[fmt][4]
    nc = tm.ncomp(fmt)
    w, h = 75, 11
    gp = group_pixels(fmt) or 16
    windows = [((40, 10), (1, 1)), ((3, 1), (9, 5)), ((4, 2), (7, 3)), ((gp, 3), (gp, 3)), ((2 * gp + 1, 6), (gp, 1)), ((32, 7), (2 * gp, 3)),
               ((16, 4), (0, 5))]
    for k, on_device in enumerate((False, True)):
        f = HFrame(fmt, w, h, np.random.default_rng(77 + li + k), "to64" if on_device else "row+1", 0 if on_device else 1)
        planes = f.arrays()
        for j, (size, origin) in enumerate(windows):
            if origin[0] + size[0] > w:
                continue
            for d, dtype in enumerate(tm.DTYPES):
                layout = LAYOUT_NAMES[(j + d + k) % 2]
                mix = make_mix("rand", nc, 1 + (j + d + li) % 4, j)
                want = mm.image(planes, fmt, depth, mix, dtype, layout, size, origin)[None]
                check(dec, [f], fmt, depth, mix, dtype, layout, size, [origin], on_device, dst_off=(j + d) % 2, want=want)


def check_values(dec):
    """all 65536 samples of a 16-bit layout and all 256 of an 8-bit one through every kind of weights and element type"""
    rng = np.random.default_rng(5)
    f16 = HFrame("gray16le", 256, 256, rng)
    f16.bufs[0][:65536 * 2] = rng.permutation(65536).astype("<u2").view(np.uint8)
    f8 = HFrame("rgb24", 16, 16, rng)
    f8.bufs[0][:768] = np.repeat(rng.permutation(256).astype(np.uint8), 3)
    f8.bufs[0][1:768:3] = rng.permutation(256).astype(np.uint8)
    for kind in KINDS:
        for dtype in tm.DTYPES:
            check(dec, [f16], "gray16le", 16, make_mix(kind, 1, 4), dtype, "NHWC")
            check(dec, [f8], "rgb24", 8, make_mix(kind, 3, 3), dtype, "NCHW")
    # the models themselves reach the corners: infinities, subnormals that are kept, ties, both zeros
    big = mm.image(f16.arrays(), "gray16le", 16, make_mix("big", 1, 2), "float16")
    assert (big == 0x7C00).any() and (big == 0xFC00).any()
    tiny = mm.image(f16.arrays(), "gray16le", 16, make_mix("tiny", 1, 2), "float16")
    assert ((tiny[0] & 0x7C00) == 0).sum() > 60 and (tiny[0] != 0).sum() > 60000
    tiny32 = mm.image(f16.arrays(), "gray16le", 16, make_mix("tiny", 1, 2), "float32")
    assert ((tiny32[1] & 0x7F800000) == 0).sum() >= 16384 and (tiny32[1] != 0).sum() == 65535
    ties = mm.image(f16.arrays(), "gray16le", 16, make_mix("ties", 1, 1), "float32")
    assert ((ties & 0x1FFF) == 0x1000).any() and ((ties & 0xFFFF) == 0x8000).any()
    nz = mm.image(f8.arrays(), "rgb24", 8, make_mix("negzero", 3, 4), "float32")
    assert (nz[0] == 0x80000000).all() and (nz[1] == 0).all() and (nz[2] == 0x80000000).all() and (nz[3] == 0).all()


def check_torch_chain(dec):
    """the eager chain on the device from the same buffer: repeat_interleave, .float(), separate mul and add kernels, the
    conversion; torch.equal to the library's tensor"""
    rng = np.random.default_rng(31)
    w, h = 64, 6                                             # linesizes of 128, 64 and 192 bytes: the fast route
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    f = HFrame("yuv422p10le", w, h, rng, "row", 0)
    for p, (rows, rb) in enumerate(f.geo):                   # ten-bit samples
        f.bufs[p][:rows * rb].view("<u2")[:] &= 1023
    fr, ts = f.on_device()
    mix = m.Decoder.ycbcr_mix(709, 10, gain=[1 / s for s in std], offset=[-a / s for a, s in zip(mean, std)])
    _, mat, b = mm.unpack(mix)
    y = ts[0][:h * w * 2].view(torch.int16).reshape(h, w).float()
    u, v = (ts[p][:h * (w // 2) * 2].view(torch.int16).reshape(h, w // 2).repeat_interleave(2, dim=1).float() for p in (1, 2))

    def chain(comps, rows):
        out = []
        for k in rows:
            a = torch.mul(comps[0], float(mat[k][0]))
            for c in range(1, len(comps)):
                a = torch.add(a, torch.mul(comps[c], float(mat[k][c])))
            out.append(torch.add(a, float(b[k])))
        return torch.stack(out)

    for dtype in (torch.float16, torch.float32, torch.bfloat16):
        got = dec.to_tensor([fr], "yuv422p10le", 10, dtype, "NCHW", on_device=True, mix=mix)
        assert dec.tensor_last_route() == FAST
        assert torch.equal(got[0], chain([y, u, v], range(3)).to(dtype)), dtype
    g = HFrame("rgb24", w, h, rng, "row", 0)
    gr, gs = g.on_device()
    rgb = gs[0][:h * w * 3].reshape(h, w, 3)
    comps = [rgb[:, :, c].float() for c in range(3)]
    mix = m.tensor_mix(np.eye(3)[::-1] / 255.0, [-0.5, -0.5, -0.5])
    _, mat, b = mm.unpack(mix)
    got = dec.to_tensor([gr], "rgb24", 8, torch.float16, "NHWC", on_device=True, mix=mix)
    assert torch.equal(got[0], chain(comps, range(3)).permute(1, 2, 0).contiguous().half())
    luma = m.tensor_mix([[0.299, 0.587, 0.114]])
    _, mat, b = mm.unpack(luma)
    got = dec.to_tensor([gr], "rgb24", 8, torch.float32, "NCHW", on_device=True, mix=luma)
    assert tuple(got.shape) == (1, 1, h, w) and torch.equal(got[0], chain(comps, range(1)))
    del ts, gs


def check_identity(dec, fmt, li):
    """nout = C, m the identity, b = 0: the bits of the call without a mix at scale 1 and bias 0"""
    nc, depth = tm.ncomp(fmt), cm.LAYOUTS[fmt][4]
    rng = np.random.default_rng(300 + li)
    for j, (w, h, on_device, ls, off) in enumerate(((33, 5, False, "row+1", 1), (64, 3, True, "to64", 0), (19, 4, True, "row", 2))):
        f = HFrame(fmt, w, h, rng, ls, off)
        dtype, layout = tm.DTYPES[(j + li) % 3], LAYOUT_NAMES[(j + li) % 2]
        size, origins = ((7, 2), [(5, 1)]) if j == 2 else (None, None)
        plain, r0 = convert(dec, [f], fmt, depth, None, dtype, layout, size, origins, on_device)
        assert r0 in (1, 2, 3)
        mixed = check(dec, [f], fmt, depth, m.tensor_mix(np.eye(nc)), dtype, layout, size, origins, on_device, want=plain)
        assert mixed in (FAST, GENERAL)


def check_resized(dec):
    rng = np.random.default_rng(41)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    for li, (fmt, bits) in enumerate((("yuv422p10le", 10), ("rgb24", 8), ("yuva420p", 8), ("gray", 8), ("yuv410p", 8))):
        nc = tm.ncomp(fmt)
        fs = [HFrame(fmt, 70, 34, rng, "row+1", 1), HFrame(fmt, 41, 52, rng, "to64", 0)]
        planes = [f.arrays() for f in fs]
        # up-scaling, down-scaling by 3.5 and by 17, windows of different sizes per frame
        for j, (size, windows) in enumerate((((90, 50), None), ((20, 8), [(0, 3, 70, 28), (3, 1, 35, 49)]), ((4, 2), [(1, 0, 68, 34), (7, 0, 34, 51)]),
                                             ((9, 7), [(5, 5, 9, 7), (0, 0, 41, 52)]))):
            for fi, filt in enumerate((rm.NEAREST, rm.BILINEAR, rm.TRIANGLE)):
                k = 1 + (j + fi + li) % 4
                mix = m.Decoder.ycbcr_mix(709, bits, gain=[1 / s for s in std], offset=[-a / s for a, s in zip(mean, std)]) \
                    if (nc == 3 and k == 3) else make_mix("rand", nc, k, j)
                dtype, layout = tm.DTYPES[(j + fi) % 3], LAYOUT_NAMES[(j + fi + li) % 2]
                on_device = bool((j + fi) % 2)
                want = mm.batch_resized(planes, fmt, bits, mix, dtype, layout, size, windows, filt)
                got, route = convert(dec, fs, fmt, bits, mix, dtype, layout, size, None, on_device, dst_off=fi % 2, windows=windows, filt=filt)
                assert route == RESIZED
                mismatch(got, want, (fmt, size, windows, filt, k, dtype, layout))
        # identity windows: the plain call with the same mix
        mix = make_mix("rand", nc, 3, li)
        win = [(6, 2, 32, 9), (1, 3, 32, 9)]
        a, ra = convert(dec, fs, fmt, bits, mix, "float32", "NHWC", (32, 9), None, False, windows=win, filt=rm.TRIANGLE)
        b, rb = convert(dec, fs, fmt, bits, mix, "float32", "NHWC", (32, 9), [(6, 2), (1, 3)], False)
        assert ra == RESIZED and rb in (5, 6, 7) and np.array_equal(a, b)
    # chunk seams: five frames with the scratch cut down to one image, two images and three, against the default
    fs = [HFrame("yuv420p", 30 + 7 * i, 20 + i, rng, "row+13", i % 3) for i in range(5)]
    mix = m.Decoder.ycbcr_mix(601, 8, full_range=True, alpha=False)
    whole, r = convert(dec, fs, "yuv420p", 8, mix, "float16", "NCHW", (12, 9), None, True, windows=None, filt=rm.TRIANGLE)
    mismatch(whole, mm.batch_resized([f.arrays() for f in fs], "yuv420p", 8, mix, "float16", "NCHW", (12, 9)), "five frames")
    for images in (1, 2, 3):
        dec.set_int("mix_scratch", images * 3 * 12 * 9 * 4)
        try:
            cut, r = convert(dec, fs, "yuv420p", 8, mix, "float16", "NCHW", (12, 9), None, True, windows=None, filt=rm.TRIANGLE)
        finally:
            dec.set_int("mix_scratch", 0)
        assert r == RESIZED and np.array_equal(cut, whole), images
    with pytest.raises(m.Htj2kError):
        dec.set_int("mix_scratch", -1)


def check_batches(dec):
    """frames of different sizes with one window and an origin each; unlike routes in one call"""
    rng = np.random.default_rng(21)
    for fmt, bits in (("rgb24", 8), ("yuv420p", 8), ("rgba64le", 16), ("yuv422p10le", 10), ("yuv411p", 8)):
        gp = group_pixels(fmt)
        sizes = [(72, 9), (33, 12), (64, 7), (17, 5)]
        origins = [(gp or 16, 3), (3, 0), (32, 1), (0, 0)]
        for on_device in (False, True):
            fs = [HFrame(fmt, w, h, rng, "to64" if i % 2 == 0 else "row+1", 0 if i != 3 else 1) for i, (w, h) in enumerate(sizes)]
            for dtype, layout, k in (("float16", "NCHW", 3), ("float32", "NHWC", 2), ("bfloat16", "NHWC", 4)):
                route = check(dec, fs, fmt, bits, make_mix("rand", tm.ncomp(fmt), k), dtype, layout, (16, 5), origins, on_device)
                assert route == (7 if gp else GENERAL), (fmt, route)    # origin 3 is off every group boundary, 0 is on it


def check_many_frames(dec, n=70000):
    """more frames than grid.z takes in one launch: 2 x 2 yuv420p frames out of one buffer, on both routes"""
    a = np.random.default_rng(9).integers(0, 256, size=(n, 8), dtype=np.uint8)       # Y at 0 .. 3, U at 4, V at 5
    rec = np.dtype({"names": ["data", "linesize", "width", "height", "pix_fmt"], "formats": [("<u8", 4), ("<i4", 4), "<i4", "<i4", "<i4"],
                    "offsets": [0, 32, 48, 52, 56], "itemsize": ctypes.sizeof(m.Frame)})
    t = np.zeros(n, rec)
    base = a.ctypes.data + 8 * np.arange(n, dtype=np.uint64)
    t["data"][:, 0], t["data"][:, 1], t["data"][:, 2] = base, base + 4, base + 5
    t["linesize"][:, 0], t["linesize"][:, 1], t["linesize"][:, 2] = 2, 1, 1
    t["width"], t["height"], t["pix_fmt"] = 2, 2, m.PIX_NAMES.index("yuv420p")
    mix = m.Decoder.ycbcr_mix(709, 8)
    _, mat, b = mm.unpack(mix)
    f = [a[:, :4].reshape(n, 2, 2).astype(np.float32), np.broadcast_to(a[:, 4, None, None], (n, 2, 2)).astype(np.float32),
         np.broadcast_to(a[:, 5, None, None], (n, 2, 2)).astype(np.float32)]
    vals = mm.mix_values(f, mat, b, 3)
    for path, dtype in ((0, "float16"), (1, "bfloat16")):
        want = np.stack([mm.stored(v, dtype) for v in vals], axis=1)               # (n, 3, 2, 2)
        spec = m.tensor_spec(dtype, "NCHW")
        dec.set_int("tensor_path", path)
        try:
            r, host, at = raw_call(dec, t.ctypes.data_as(ctypes.c_void_p), 0, n, 8, spec, mix, None, n * 24)
        finally:
            dec.set_int("tensor_path", 0)
        assert r == 0 and dec.tensor_last_route() == (GENERAL if path else FAST)
        assert (host[:at] == 0xA5).all() and (host[at + n * 24:] == 0xA5).all()
        assert np.array_equal(host[at:at + n * 24].view(np.uint16).reshape(n, 3, 2, 2), want)


def check_refusals(dec):
    """refusals on a live context: nothing launched, dst and its guards untouched, route 0, and the context works on"""
    rng = np.random.default_rng(3)
    f = HFrame("yuv420p", 20, 10, rng)
    ok = m.tensor_spec("float16")
    win = m.tensor_spec("float16", size=(4, 4))
    eye = lambda k: m.tensor_mix(np.eye(k, 3))
    need = lambda k: k * 20 * 10 * 2

    def bad(**kw):
        x = eye(3)
        for name, v in kw.items():
            if name == "nout":
                x.nout = v
            elif name[0] == "m":
                x.m[int(name[1])][int(name[2])] = v
            else:
                x.b[int(name[1])] = v
        return x

    cases = [  # (bits, spec, mix, origins, bytes of dst, offset of dst, resized filter or None, what it answers)
        (8, ok, bad(nout=0), None, need(4), 0, None, EINVAL),
        (8, ok, bad(nout=5), None, need(4), 0, None, EINVAL),
        (8, ok, bad(m12=float("nan")), None, need(3), 0, None, EINVAL),
        (8, ok, bad(b0=float("inf")), None, need(3), 0, None, EINVAL),
        (9, ok, eye(3), None, need(3), 0, None, EINVAL),
        (8, ok, eye(4), None, need(3) - SURPLUS, 0, None, EINVAL),        # sized for C, K > C
        (8, ok, eye(2), None, need(2), 1, None, EINVAL),
        (8, win, eye(3), [(17, 0)], need(3), 0, None, EINVAL),
        (8, win, bad(nout=7), None, need(3), 0, rm.TRIANGLE, EINVAL),
        (8, win, eye(4), None, 4 * 16 * 2 - 1 - SURPLUS, 0, rm.BILINEAR, EINVAL),
        (8, win, eye(3), None, need(3), 0, 7, EINVAL),
    ]
    good = make_mix("rand", 3, 3)
    for i, (bits, s, mix, origins, nbytes, off, filt, answer) in enumerate(cases):
        check(dec, [f], "yuv420p", 8, good)                     # a call that launches, so that a route is there to be cleared
        arr = (m.Frame * 1)(f.frame())
        r, host, at = raw_call(dec, arr, 0, 1, bits, s, mix, origins, nbytes, off, None, filt)
        assert r == answer, (i, r)
        assert (host == 0xA5).all(), i
        assert dec.tensor_last_route() == 0, i
    pal = HFrame("pal8", 20, 10, rng)
    r, host, at = raw_call(dec, (m.Frame * 1)(pal.frame()), 0, 1, 8, ok, bad(nout=0), None, need(3))
    assert r == PATCHWELCOME and (host == 0xA5).all()
    # an entry that is not read may be anything
    check(dec, [f], "yuv420p", 8, bad(m03=float("nan"), m30=float("inf"), b3=float("nan")), "float32", "NHWC")


def check_python(dec):
    """the keyword on the methods that take planes: shapes, `out`, the helper"""
    rng = np.random.default_rng(12)
    fs = [HFrame("yuv420p", 34, 6, rng), HFrame("yuv420p", 34, 6, rng)]
    planes = [f.arrays() for f in fs]
    mix = m.Decoder.ycbcr_mix(2020, 8, full_range=True, alpha=False, gain=[2, 2, 2], offset=[-1, -1, -1])
    t = dec.to_tensor(planes, "yuv420p", 8, mix=mix)
    assert t.dtype == torch.float16 and tuple(t.shape) == (2, 3, 6, 34) and dec.tensor_last_route() == FAST and dec.compare_ms() > 0
    assert np.array_equal(tensor_bits(t), mm.batch(planes, "yuv420p", 8, mix, "float16"))
    luma = m.tensor_mix([[1 / 255, 0, 0]])
    out = torch.zeros((2, 4, 5, 1), dtype=torch.bfloat16, device="cuda")
    t2 = dec.to_tensor(planes, "yuv420p", 8, torch.bfloat16, "NHWC", size=(5, 4), origins=(7, 1), out=out, mix=luma)
    assert t2 is out and np.array_equal(tensor_bits(out), mm.batch(planes, "yuv420p", 8, luma, "bfloat16", "NHWC", (5, 4), [(7, 1)] * 2))
    with pytest.raises(ValueError):
        dec.to_tensor(planes, "yuv420p", 8, torch.bfloat16, "NHWC", size=(5, 4), out=torch.zeros((2, 4, 5, 3), dtype=torch.bfloat16, device="cuda"), mix=luma)
    with pytest.raises(ValueError):
        dec.to_tensor(planes, "yuv420p", 8, mix=(np.eye(3), None))
    four = m.tensor_mix(np.ones((4, 3)) / 512, [0, 1, 2, 3])
    t3 = dec.to_tensor_resized(planes, "yuv420p", 8, (9, 4), windows=(2, 0, 30, 6), filter="bilinear", dtype="float32", mix=four)
    assert tuple(t3.shape) == (2, 4, 4, 9) and dec.tensor_last_route() == RESIZED
    assert np.array_equal(tensor_bits(t3), mm.batch_resized(planes, "yuv420p", 8, four, "float32", "NCHW", (9, 4), [(2, 0, 30, 6)] * 2, rm.BILINEAR))
    assert m.Decoder.tensor_image_size("yuv420p", 34, 6, 8, m.tensor_spec("float16"), four) == (4 * 34 * 6, 4 * 34 * 6 * 2)


def check_jobs(dec, orc):
    """a yuv422p10le and a yuv420p stream against the oracle's frames through the model"""
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    job = dec.job()
    for fmt, datas in (("yuv422p10le", [yuv422p10_stream()] * 2), ("yuv420p", [streams.get("yuv420p8")[0]] * 2)):
        job.parse_batch(datas).upload().run()
        info = job.frame_info(0)
        assert m.PIX_NAMES[info.pix_fmt] == fmt
        bits = info.bits_per_raw_sample
        want_planes = [orc.decode(d)[1] for d in datas]
        mix = m.Decoder.ycbcr_mix(709, bits, gain=[1 / s for s in std], offset=[-a / s for a, s in zip(mean, std)])
        t, status = job.to_tensor("float16", "NCHW", mix=mix)                                 # bits 0: the job's
        assert status == [0, 0] and tuple(t.shape) == (2, 3, info.height, info.width) and dec.tensor_last_route() in (5, 6, 7)
        assert np.array_equal(tensor_bits(t), mm.batch(want_planes, fmt, bits, mix, "float16")), fmt
        luma = m.tensor_mix([[1 / ((1 << bits) - 1), 0, 0]], [-0.5])
        t, status = job.to_tensor("float32", "NHWC", size=(24, 10), origins=[(16, 3), (5, 1)], bits=bits, mix=luma)
        assert tuple(t.shape) == (2, 10, 24, 1) and dec.tensor_last_route() in (5, 6, 7)
        assert np.array_equal(tensor_bits(t), mm.batch(want_planes, fmt, bits, luma, "float32", "NHWC", (24, 10), [(16, 3), (5, 1)])), fmt
        four = make_mix("rand", 3, 4)
        wins = [(1, 1, info.width - 2, info.height - 2), (0, 0, info.width, info.height)]
        t, status = job.to_tensor_resized((13, 9), wins, "triangle", "bfloat16", "NHWC", mix=four)
        assert status == [0, 0] and tuple(t.shape) == (2, 9, 13, 4) and dec.tensor_last_route() == RESIZED
        assert np.array_equal(tensor_bits(t), mm.batch_resized(want_planes, fmt, bits, four, "bfloat16", "NHWC", (13, 9), wins, rm.TRIANGLE)), fmt
        with pytest.raises(m.Htj2kError) as e:                # a mix that is refused
            job.to_tensor("float16", "NCHW", mix=m.tensor_mix([[float("nan"), 0, 0]]))
        assert e.value.code == EINVAL
    job.free()


def check_pipes(dec, orc, wait=60):
    """a pipe with a packet that fails, received with and without a mix in turn"""
    names = ["yuv420p8", "rgb_mct", "gray_l5_cb64"]
    pkts = [streams.get(names[i % 3])[0] for i in range(9)]
    pkts[2] = pkts[2][:40]                                   # fails to parse: its batch is retried packet by packet
    pkts[5] = damaged_copy(pkts[5])                          # parses, some blocks rejected: still a frame
    want = [None if i == 2 else orc.decode(p)[:2] for i, p in enumerate(pkts)]
    pipe = bounded(lambda: dec.pipe(batch=4, depth=2), wait)
    try:
        sent = got = 0
        while got < len(pkts):
            while sent < len(pkts) and bounded(lambda: pipe.send(pkts[sent]), wait):
                sent += 1
            if sent == len(pkts):
                bounded(pipe.flush, wait)
            if got == 2:
                with pytest.raises(m.Htj2kError) as e:
                    bounded(lambda: pipe.receive_tensor(mix=make_mix("rand", 3, 3)), wait)
                assert e.value.code < 0 and e.value.code != m.EAGAIN
                got += 1
                continue
            info_o, planes_o = want[got]
            fmt, bits = m.PIX_NAMES[info_o.pix_fmt], info_o.bits_per_raw_sample
            mix = make_mix("perm" if fmt == "rgb24" else "rand", tm.ncomp(fmt), 1 + got % 4, got)
            if got % 3 == 0:
                t, info = bounded(lambda: pipe.receive_tensor("float16", "NCHW", mix=mix), wait)
                assert np.array_equal(tensor_bits(t), mm.image(planes_o, fmt, bits, mix, "float16")[None]), got
            elif got % 3 == 1:
                t, info = bounded(lambda: pipe.receive_tensor("float16", "NCHW", scale=1 / 255, bias=-0.5), wait)
                assert np.array_equal(tensor_bits(t), tm.image(planes_o, fmt, bits, "float16", "NCHW", None, (0, 0), 1 / 255, -0.5)[None]), got
            else:
                t, info = bounded(lambda: pipe.receive_tensor_resized((11, 7), None, "bilinear", "float32", "NHWC", mix=mix), wait)
                assert np.array_equal(tensor_bits(t), mm.image_resized(planes_o, fmt, bits, mix, "float32", "NHWC", (11, 7), None, rm.BILINEAR)[None]), got
            assert (info.width, info.height, info.pix_fmt) == (info_o.width, info_o.height, info_o.pix_fmt), got
            got += 1
        assert bounded(lambda: pipe.receive_tensor(mix=make_mix("rand", 3, 3)), wait) is None      # drained
    finally:
        bounded(pipe.close, wait)


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


def test_the_sweep_covers_what_it_claims():
    """no device: every layout's sweep meets every K on each route it has, every element type and both tensor layouts"""
    for li, fmt in enumerate(LAYOUTS):
        seen = set()
        for w, h, bits, kind, k, dtype, layout, on_device, ls, off in layout_cases(fmt, li):
            geo = m.plane_geometry(fmt, w, h)
            lss = [{"row": rb, "row+1": rb + 1, "row+13": rb + 13, "to64": -(-rb // 64) * 64}[ls] for _, rb in geo]
            aligned = (not on_device) or (off % 16 == 0 and all(v % 16 == 0 for v in lss))
            seen.add((FAST if group_pixels(fmt) and aligned else GENERAL, k))
            seen.add((dtype, layout if k > 1 else "NCHW"))
        for k in range(1, 5):
            assert (GENERAL, k) in seen and (not group_pixels(fmt) or (FAST, k) in seen), (fmt, k)
        for dtype in tm.DTYPES:
            assert (dtype, "NCHW") in seen and (dtype, "NHWC") in seen, (fmt, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_layouts_rows_linesizes_offsets(dec, fmt):
    check_layout(dec, fmt, LAYOUTS.index(fmt))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_windows(dec, fmt):
    check_windows(dec, fmt, LAYOUTS.index(fmt))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_identity_mix_is_the_plain_call(dec, fmt):
    check_identity(dec, fmt, LAYOUTS.index(fmt))


@pytest.mark.gpu
def test_weights_at_the_corners_of_the_formats(dec):
    check_values(dec)


@pytest.mark.gpu
def test_torch_eager_chain_on_the_device(dec):
    check_torch_chain(dec)


@pytest.mark.gpu
def test_resized_calls(dec):
    check_resized(dec)


@pytest.mark.gpu
def test_batches_of_unlike_frames(dec):
    check_batches(dec)


@pytest.mark.gpu
def test_more_frames_than_one_launch_takes(dec):
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


def run_everything(dec, orc):
    for i, fmt in enumerate(LAYOUTS):
        check_layout(dec, fmt, i)
        check_windows(dec, fmt, i)
        check_identity(dec, fmt, i)
    check_values(dec)
    check_torch_chain(dec)
    check_resized(dec)
    check_batches(dec)
    check_many_frames(dec)
    check_refusals(dec)
    check_python(dec)
    check_jobs(dec, orc)
    check_pipes(dec, orc)


POISON_TIMEOUT = 300


@pytest.mark.gpu
def test_everything_on_poisoned_buffers():
    """HTJ2K_POISON=1 (read once per process, so a fresh child): every new device buffer of the library, the scratch of
    the resized calls included, starts as 0xA5 bytes, and all of the above must still give the model's results.  The
    child's exit status comes first."""
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
    print("%s buffers: ok, %.1f s, %d calls (%d with the fast route, %d with the general one, %d resized)"
          % ("poisoned" if os.environ.get("HTJ2K_POISON") == "1" else "plain", time.time() - t0, CALLS["n"], CALLS["fast"], CALLS["general"],
             CALLS["resized"]))
