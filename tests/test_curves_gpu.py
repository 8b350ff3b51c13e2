"""The tensor calls with transfer curves on the GPU against the numpy model (curve_model): every bit of every element, on
both routes of the plain kernel and through the scratch pass of the resized calls, destinations between 0xA5 guard zones.

Twelve layouts over three element types, two tensor layouts and K = 1 .. 4; widths at the tails of the pixel groups, heights
1 .. 5, linesizes and bases off the 16-byte alignment on host and device operands; windows on and off the group boundary;
tables of 2, 3, 256, 4096 and 4097 knots before the mix, after it and both, with masks that leave components and channels
out; x0 and inv_dx that put u below 0, on knots, at n - 1 and above it; all 4096 samples in every component; infinities and
inf - inf out of the mix (the NaN rule); tables with -0.0 entries; the identity against htj2k_frames_to_tensor_mix; the
torch eager chain on the device; resized calls with chunk seams; a frame large enough for several workgroups of several
steps; more frames than grid.z takes; jobs, a pipe with a damaged packet, refusals on a live context.  The route of every
call is asserted, and every call that took the fast route is made again on the general one and compared bit for bit.  Run
as a program, the module runs all of it on its own contexts: test_everything_on_poisoned_buffers does that in a child
process under HTJ2K_POISON=1."""
import ctypes
import math
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
import curve_model as cvm
import ffmpeg_ht_amd as m
import mix_model as mm
import oracle
import resize_model as rm
import streams
import tensor_model as tm
from test_curves_host import frame_of
from test_hash_gpu import HFrame, damaged_copy
from test_mix_gpu import GUARD, SURPLUS, expected_route, group_pixels, make_mix, mismatch
from test_mix_gpu import convert as convert_mix
from test_tensor_gpu import bounded, tensor_bits, yuv422p10_stream

LAYOUTS = ["xyz12le", "rgb24", "rgb48le", "rgba", "gray", "ya8", "yuv444p10le", "yuv422p10le", "yuv420p", "yuv411p", "yuv410p", "yuva420p"]
LS_MODES = ["row", "row+1", "row+13", "to64"]
OFFSETS = [0, 1, 2, 15]
LAYOUT_NAMES = ["NCHW", "NHWC"]
KNOTS = [2, 3, 256, 4096, 4097]
MODES = ["in", "out", "both"]
EINVAL, PATCHWELCOME = -22, -0x45574150
FAST, GENERAL, BOTH, RESIZED = 9, 10, 11, 12
CALLS = {"n": 0, "fast": 0, "general": 0, "resized": 0}


def widths(fmt):
    """widths at the tails of the layout's pixel group: 1, g - 1, g, g + 1, 2 g + 1 and a row of several groups"""
    g = group_pixels(fmt) or 16
    return sorted({1, max(g - 1, 1), g, g + 1, 2 * g + 1, 4 * g + 3})


def make_curves(mode, nc, k, bits, j, alpha_out=False):
    """curves of one of the kinds the tests walk: tables of KNOTS[j % 5] and KNOTS[(j + 2) % 5] knots with negative,
    non-monotone and -0.0 entries; x0 and inv_dx that make the table an exact lookup of the sample, that put samples on and
    between knots with some below the first, or that leave the upper knots unused; masks that leave components out"""
    rng = np.random.default_rng(7000 + 100 * nc + 10 * k + j)
    peak = float(1 << bits)

    def table(n, sd):
        t = rng.normal(0, sd, n).astype(np.float32)
        t[rng.integers(0, n, max(n // 16, 1))] = -0.0
        return t
    n_in, n_out = KNOTS[j % 5], KNOTS[(j + 2) % 5]
    geo_in = [(0.0, 1.0), (peak / 8, (n_in - 1) / (peak * 0.75)), (-peak / 3, (n_in - 1) / (2 * peak))][j % 3]
    span = peak / 8                                          # the mixes of make_mix("rand") give a few times peak / 64
    geo_out = [(-span / 2, (n_out - 1) / span), (0.25, (n_out - 1) / span * 4)][(j // 3) % 2]
    cin = m.tensor_curve(table(n_in, peak / 4), *geo_in) if mode in ("in", "both") else None
    cout = m.tensor_curve(table(n_out, 1.0), *geo_out) if mode in ("out", "both") else None
    full_in, full_out = (1 << min(nc, 3)) - 1, (1 << min(k, 3)) - 1
    in_mask = [full_in, (1 << nc) - 1, 1 << (j % nc), full_in & ~(1 << (j % nc))][j % 4] if nc > 1 else 1
    out_mask = [full_out, (1 << k) - 1, 1 << (j % k), 0][(j // 2) % 4]
    if alpha_out:
        in_mask, out_mask = in_mask & 7, out_mask & 7        # alpha outside the masks
    gain = rng.normal(0, 2, k).astype(np.float32)
    offset = np.array([0.0, -0.0, 0.5, -1.0], np.float32)[(np.arange(k) + j) % 4]
    return m.tensor_curves(cin, cout, in_mask, out_mask, gain, offset)


def raw_call(dec, arr, on_device, n, bits, spec, mix, curves, origins, nbytes, dst_off_bytes=0, windows=None, filt=None):
    """the C call on a destination between two guard zones, `SURPLUS` bytes larger than needed -> (return value, the whole
    buffer as a host array, where the images start in it).  filt: the resized call with `windows`"""
    at = GUARD + dst_off_bytes
    buf = torch.full((at + nbytes + SURPLUS + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    mp = None if mix is None else ctypes.byref(mix)
    qp = None if curves is None else ctypes.byref(curves)
    torch.cuda.synchronize()
    if filt is None:
        org = None if origins is None else (ctypes.c_int32 * (2 * len(origins)))(*[int(v) for o in origins for v in o])
        r = dec.L.htj2k_frames_to_tensor_curves(dec.h, arr, int(on_device), n, int(bits), ctypes.byref(spec), mp, qp, org,
                                                ctypes.c_void_p(buf.data_ptr() + at), ctypes.c_size_t(nbytes + SURPLUS))
    else:
        win = None if windows is None else (ctypes.c_int32 * (4 * len(windows)))(*[int(v) for w in windows for v in w])
        r = dec.L.htj2k_frames_to_tensor_resized_curves(dec.h, arr, int(on_device), n, int(bits), ctypes.byref(spec), mp, qp, win, int(filt),
                                                        ctypes.c_void_p(buf.data_ptr() + at), ctypes.c_size_t(nbytes + SURPLUS))
    return r, buf.cpu().numpy(), at


def convert(dec, frames, fmt, bits, mix, curves, dtype, layout, size, origins, on_device, dst_off=0, windows=None, filt=None):
    """-> (bit patterns shaped as the model's, route); the guards and the surplus bytes must still be 0xA5"""
    n, k = len(frames), mix.nout
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
    r, host, at = raw_call(dec, arr, on_device, n, bits, spec, mix, curves, origins, nbytes, dst_off * es, windows, filt)
    assert r == 0, (r, fmt, dtype, layout, size, origins, windows)
    assert (host[:at] == 0xA5).all(), "bytes in front of dst were written"
    assert (host[at + nbytes:] == 0xA5).all(), "bytes beyond the images were written"
    shape = (n, k, oh, ow) if layout == "NCHW" else (n, oh, ow, k)
    route = dec.tensor_last_route()
    CALLS["n"] += 1
    CALLS["fast"] += route in (FAST, BOTH)
    CALLS["general"] += route in (GENERAL, BOTH)
    CALLS["resized"] += route == RESIZED
    del keep
    return host[at:at + nbytes].view(tm.BITS_DTYPE[dtype]).reshape(shape), route


def check(dec, frames, fmt, bits, mix, curves, dtype="float16", layout="NCHW", size=None, origins=None, on_device=False, dst_off=0, want=None):
    """one call against the model, its route against the rule, and once more on the general route if it took the fast one"""
    if want is None:
        want = cvm.batch([f.arrays() for f in frames], fmt, bits, mix, curves, dtype, layout, size, origins)
    what = (fmt, bits, mix.nout, curves.in_.n, curves.out.n, curves.in_mask, curves.out_mask, dtype, layout, size, origins, on_device, dst_off,
            [(f.w, f.h, f.ls, f.off) for f in frames[:4]])
    got, route = convert(dec, frames, fmt, bits, mix, curves, dtype, layout, size, origins, on_device, dst_off)
    assert route == expected_route(frames, fmt, origins, on_device) + 4, (route, what)
    mismatch(got, want, (what, route))
    if route in (FAST, BOTH):
        dec.set_int("tensor_path", 1)
        try:
            again, r2 = convert(dec, frames, fmt, bits, mix, curves, dtype, layout, size, origins, on_device, dst_off)
        finally:
            dec.set_int("tensor_path", 0)
        assert r2 == GENERAL and np.array_equal(again, got), (what, r2)
    return route


def layout_cases(fmt, li):
    """the sweep of one layout: (w, h, bits, mode, K, dtype, tensor layout, on_device, linesize mode, offset, j).  Every
    width twice: on a host operand (uploaded: the fast route where the layout has one) and on a device operand whose base or
    linesize is off the alignment for all but one width in three"""
    depth = cm.LAYOUTS[fmt][4]
    for i, w in enumerate(widths(fmt)):
        h = 1 + (i + li) % 5
        bits = depth - 1 if i % 5 == 4 else depth
        for d, on_device in enumerate((False, True)):
            j = 2 * i + d
            k = 1 + (i + d + li) % 4
            off = OFFSETS[(i + li) % 4] if on_device else OFFSETS[(i + 1) % 4]
            ls = LS_MODES[(i + li + d) % 4]
            if on_device and i % 3 == 2:
                ls, off = "to64", 0                          # a device operand on the fast route
            yield w, h, bits, MODES[(j + li) % 3], k, tm.DTYPES[(j + li) % 3], LAYOUT_NAMES[(j // 3 + li) % 2], on_device, ls, off, j + li


def check_layout(dec, fmt, li):
    nc = tm.ncomp(fmt)
    seen = set()
    for c, (w, h, bits, mode, k, dtype, layout, on_device, ls, off, j) in enumerate(layout_cases(fmt, li)):
        f = HFrame(fmt, w, h, np.random.default_rng(1000 * li + c), ls, off)
        q = make_curves(mode, nc, k, bits, j, alpha_out=fmt == "yuva420p")
        route = check(dec, [f], fmt, bits, make_mix("rand", nc, k, c), q, dtype, layout, None, None, on_device)
        seen.update([route, k, dtype, layout if k > 1 else "NCHW", mode])
    assert GENERAL in seen and (not group_pixels(fmt) or FAST in seen), (fmt, sorted(map(str, seen)))
    assert seen >= {1, 2, 3, 4} | set(tm.DTYPES) | set(LAYOUT_NAMES) | set(MODES), (fmt, sorted(map(str, seen)))


def check_windows(dec, fmt, li):
    """windows that start on and off a group boundary and on and off a chroma sample, destinations off by one element"""
    depth = cm.LAYOUTS[fmt][4]
    nc = tm.ncomp(fmt)
    w, h = 75, 11
    gp = group_pixels(fmt) or 16
    windows = [((40, 10), (1, 1)), ((3, 1), (9, 5)), ((gp, 3), (gp, 3)), ((2 * gp + 1, 6), (gp, 1)), ((32, 7), (2 * gp, 3)), ((16, 4), (0, 5))]
    for k, on_device in enumerate((False, True)):
        f = HFrame(fmt, w, h, np.random.default_rng(77 + li + k), "to64" if on_device else "row+1", 0 if on_device else 1)
        planes = f.arrays()
        for j, (size, origin) in enumerate(windows):
            if origin[0] + size[0] > w:
                continue
            dtype, layout, nk = tm.DTYPES[(j + k) % 3], LAYOUT_NAMES[(j + k + li) % 2], 1 + (j + li) % 4
            mix, q = make_mix("rand", nc, nk, j), make_curves(MODES[(j + li) % 3], nc, nk, depth, j + 3 * k + li, fmt == "yuva420p")
            want = cvm.image(planes, fmt, depth, mix, q, dtype, layout, size, origin)[None]
            check(dec, [f], fmt, depth, mix, q, dtype, layout, size, [origin], on_device, dst_off=(j + k) % 2, want=want)


def all_samples_frame(seed=5):
    """a 64 x 64 xyz12le frame that holds all 4096 sample values in every component"""
    rng = np.random.default_rng(seed)
    f = HFrame("xyz12le", 64, 64, rng, "row", 0)
    comps = [rng.permutation(4096).reshape(64, 64) for _ in range(3)]
    f.bufs[0][:64 * 64 * 6] = frame_of("xyz12le", comps, 12)[0].astype("<u2").view(np.uint8).reshape(-1)
    assert all(np.array_equal(a, b) for a, b in zip(cm.components(f.arrays(), "xyz12le", 12), comps))
    return f, comps


def check_corners(dec):
    f, comps = all_samples_frame()
    # the use the calls are for, at every sample value, in three encodings
    for i, (primaries, out, n_out) in enumerate(((709, "srgb", 4097), (2020, "pq", 4096), (m.PRIMARIES_P3D65, "bt709", 256))):
        mix, q = m.Decoder.dcp_curves(primaries, out, n_out, gain=[1.0, 2.0, 255.0][i], offset=[0.0, -1.0, 0.5][i])
        for dtype in tm.DTYPES:
            check(dec, [f], "xyz12le", 12, mix, q, dtype, LAYOUT_NAMES[i % 2], on_device=bool(i % 2))
    # an exact lookup of a table with negative, non-monotone and -0.0 entries: direct indexing, but for the sign of a zero
    table = np.random.default_rng(6).normal(0, 100, 4096).astype(np.float32)
    table[::9] = -0.0
    q = m.tensor_curves(m.tensor_curve(table), None, offset=-0.0)
    got, route = convert(dec, [f], "xyz12le", 12, m.tensor_mix(np.eye(3)), q, "float32", "NCHW", None, None, False)
    assert route == FAST
    for c in range(3):
        direct = table[comps[c]]
        assert np.array_equal(got[0, c].view(np.float32)[direct != 0], direct[direct != 0]) and (got[0, c][direct == 0] << 1 == 0).all()
    check(dec, [f], "xyz12le", 12, m.tensor_mix(np.eye(3)), q, "float32", "NCHW")
    # before the mix: every u below 0; every u above n - 1; u from 0 to n - 1 and no further (twice); knots 0 and 1 with
    # samples on either side; between knots; halfway between them.  After the mix the same tables over t
    for j, (n, x0, inv_dx) in enumerate(((4, 4096.0, 1.0), (4, -8192.0, 1.0), (3, 0.0, 2.0 / 4095), (4097, 0.0, 4096.0 / 4095), (2, 2047.0, 1.0),
                                         (256, 1024.0, 1 / 8), (4096, 0.5, 1.0))):
        t = np.random.default_rng(j).normal(0, 1, n).astype(np.float32)
        q = m.tensor_curves(m.tensor_curve(t, x0, inv_dx), m.tensor_curve(t, (x0 - 2048) / 4096, inv_dx * 1024), 5, 6)
        check(dec, [f], "xyz12le", 12, make_mix("rand", 3, 3, j), q, tm.DTYPES[j % 3], LAYOUT_NAMES[j % 2], on_device=bool(j % 2))
    # weights large enough that t is +inf, -inf and inf - inf: the top knot, knot 0 and, by the NaN rule, knot 0
    big = m.tensor_mix([[3e38, 3e38, 0], [3e38, -3e38, 0], [-3e38, -3e38, 0], [0, 0, 1]])
    ends = m.tensor_curves(None, m.tensor_curve([5.0, 1.0, 2.0, 7.0], 0.0, 1.0), 0, 7, [1, 1, 1, 1], -0.0)
    want = cvm.image(f.arrays(), "xyz12le", 12, big, ends, "float32")
    lit = (comps[0] > 1) & (comps[1] > 1)
    assert (want[0].view(np.float32)[lit] == 7).all() and (want[1].view(np.float32)[lit] == 5).all() and (want[2].view(np.float32)[lit] == 5).all()
    for dtype in tm.DTYPES:
        check(dec, [f], "xyz12le", 12, big, ends, dtype, "NHWC")
        check(dec, [f], "xyz12le", 12, big, ends, dtype, "NCHW", on_device=True)
    # signed zeros: t = -0 from -0 weights and a -0 offset meets a -0.0 first knot; +0 weights meet it as well
    g = HFrame("rgb24", 33, 3, np.random.default_rng(2), "row", 0)
    zeros = m.tensor_curves(m.tensor_curve([-0.0, 0.0, -0.0, 1.0], 0.0, 1 / 64), m.tensor_curve([-0.0, 1.0, -0.0], 0.0, 1.0), 3, 7, 1.0, -0.0)
    for kind in ("negzero", "zero"):
        want = cvm.image(g.arrays(), "rgb24", 8, make_mix(kind, 3, 4), zeros, "float32")
        assert kind != "negzero" or ((want[0] == 0).all() and (want[1] == 0).all())      # maxNum(-0, +0) is +0, then -0 + (+0 * 1)
        for dtype in tm.DTYPES:
            check(dec, [g], "rgb24", 8, make_mix(kind, 3, 4), zeros, dtype, "NCHW")
            check(dec, [g], "rgb24", 8, make_mix(kind, 3, 4), zeros, dtype, "NHWC", on_device=True)


def check_identity(dec):
    """an in-curve t[j] = j with n = 2^bits, no out-curve, gain 1 and offset -0.0: htj2k_frames_to_tensor_mix's bits"""
    rng = np.random.default_rng(300)
    for li, fmt in enumerate(("xyz12le", "rgb24", "yuv422p10le", "yuv420p", "gray", "yuva420p", "yuv410p")):
        nc, depth = tm.ncomp(fmt), cm.LAYOUTS[fmt][4]
        q = m.tensor_curves(m.tensor_curve(np.arange(1 << depth, dtype=np.float32)), None, (1 << nc) - 1, 0, 1.0, -0.0)
        for j, (w, h, on_device, ls, off) in enumerate(((33, 5, False, "row+1", 1), (64, 3, True, "to64", 0), (19, 4, True, "row", 2))):
            f = HFrame(fmt, w, h, rng, ls, off)
            dtype, layout, k = tm.DTYPES[(j + li) % 3], LAYOUT_NAMES[(j + li) % 2], 1 + (j + li) % 4
            mix = make_mix(("rand", "negzero", "perm")[j], nc, k, li)
            size, origins = ((7, 2), [(5, 1)]) if j == 2 else (None, None)
            mixed, r0 = convert_mix(dec, [f], fmt, depth, mix, dtype, layout, size, origins, on_device)
            assert r0 in (5, 6)
            assert check(dec, [f], fmt, depth, mix, q, dtype, layout, size, origins, on_device, want=mixed) == r0 + 4


def check_torch_chain(dec):
    """the eager chain on the device from the same buffer: the shift, a gather, separate mul and add kernels, a clamp, an
    index and a lerp, the conversion; torch.equal to the library's tensor"""
    rng = np.random.default_rng(31)
    w, h = 64, 6
    f = HFrame("xyz12le", w, h, rng, "row", 0)
    fr, ts = f.on_device()
    words = ts[0][:h * w * 6].view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).reshape(h, w, 3)
    s = words.bitwise_right_shift(4).permute(2, 0, 1).reshape(3, h * w)
    for primaries, out, n_out, gain, offset in ((709, "srgb", 4097, None, None), (2020, "pq", 1024, 2.0, -1.0)):
        mix, q = m.Decoder.dcp_curves(primaries, out, n_out, gain, offset)
        _, mat, b = mm.unpack(mix)
        ref = cvm.torch_chain(s, torch.from_numpy(q.tables[0]).cuda(), mat[:3], b, torch.from_numpy(q.tables[1]).cuda(), float(q.out.x0),
                          float(q.out.inv_dx), list(q.gain), list(q.offset)).reshape(3, h, w)
        for dtype in (torch.float16, torch.float32, torch.bfloat16):
            got = dec.to_tensor([fr], "xyz12le", 12, dtype, "NCHW", on_device=True, mix=mix, curves=q)
            assert dec.tensor_last_route() == FAST and torch.equal(got[0], ref.to(dtype)), (primaries, dtype)
        got = dec.to_tensor([fr], "xyz12le", 12, torch.float16, "NHWC", on_device=True, mix=mix, curves=q)
        assert torch.equal(got[0], ref.permute(1, 2, 0).contiguous().half())
    del ts


def check_resized(dec):
    rng = np.random.default_rng(41)
    for li, (fmt, bits) in enumerate((("xyz12le", 12), ("yuv422p10le", 10), ("rgb24", 8), ("yuva420p", 8), ("yuv410p", 8))):
        nc = tm.ncomp(fmt)
        fs = [HFrame(fmt, 70, 34, rng, "row+1", 1), HFrame(fmt, 41, 52, rng, "to64", 0)]
        planes = [f.arrays() for f in fs]
        for j, (size, windows) in enumerate((((90, 50), None), ((20, 8), [(0, 3, 70, 28), (3, 1, 35, 49)]), ((4, 2), [(1, 0, 68, 34), (7, 0, 34, 51)]))):
            for fi, filt in enumerate((rm.NEAREST, rm.BILINEAR, rm.TRIANGLE)):
                k = 1 + (j + fi + li) % 4
                mix, q = (m.Decoder.dcp_curves(709, "srgb", 256) if (fmt == "xyz12le" and fi == 2) else
                          (make_mix("rand", nc, k, j), make_curves(MODES[(j + fi) % 3], nc, k, bits, 3 * j + fi + li, fmt == "yuva420p")))
                dtype, layout = tm.DTYPES[(j + fi) % 3], LAYOUT_NAMES[(j + fi + li) % 2]
                want = cvm.batch_resized(planes, fmt, bits, mix, q, dtype, layout, size, windows, filt)
                got, route = convert(dec, fs, fmt, bits, mix, q, dtype, layout, size, None, bool((j + fi) % 2), dst_off=fi % 2, windows=windows, filt=filt)
                assert route == RESIZED
                mismatch(got, want, (fmt, size, windows, filt, k, dtype, layout))
        # identity windows: the plain call with the same curves
        mix, q = make_mix("rand", nc, 3, li), make_curves("both", nc, 3, bits, li, fmt == "yuva420p")
        win = [(6, 2, 32, 9), (1, 3, 32, 9)]
        a, ra = convert(dec, fs, fmt, bits, mix, q, "float32", "NHWC", (32, 9), None, False, windows=win, filt=rm.TRIANGLE)
        b, rb = convert(dec, fs, fmt, bits, mix, q, "float32", "NHWC", (32, 9), [(6, 2), (1, 3)], False)
        assert ra == RESIZED and rb in (FAST, GENERAL, BOTH) and np.array_equal(a, b)
    # chunk seams: five frames with the scratch cut down to one image, two images and three, against the default
    fs = [HFrame("yuv420p", 30 + 7 * i, 20 + i, rng, "row+13", i % 3) for i in range(5)]
    mix, q = m.Decoder.ycbcr_mix(601, 8, full_range=True), m.tensor_curves(None, m.tensor_curve(m.curve_table("srgb_decode", 4097), 0.0, 4096.0))
    whole, r = convert(dec, fs, "yuv420p", 8, mix, q, "float16", "NCHW", (12, 9), None, True, windows=None, filt=rm.TRIANGLE)
    mismatch(whole, cvm.batch_resized([f.arrays() for f in fs], "yuv420p", 8, mix, q, "float16", "NCHW", (12, 9)), "five frames")
    for images in (1, 2, 3):
        dec.set_int("mix_scratch", images * 3 * 12 * 9 * 4)
        try:
            cut, r = convert(dec, fs, "yuv420p", 8, mix, q, "float16", "NCHW", (12, 9), None, True, windows=None, filt=rm.TRIANGLE)
        finally:
            dec.set_int("mix_scratch", 0)
        assert r == RESIZED and np.array_equal(cut, whole), images


def check_sizes(dec):
    """a 1024 x 96 frame under the largest tables: several workgroups of several steps each; and a batch of unlike frames
    on both routes in one call"""
    rng = np.random.default_rng(17)
    f = HFrame("xyz12le", 1024, 96, rng, "row", 0)
    mix, q = m.Decoder.dcp_curves(2020, "pq", 4097)
    assert check(dec, [f], "xyz12le", 12, mix, q, "float16", "NCHW", on_device=True) == FAST
    assert check(dec, [f], "xyz12le", 12, mix, q, "bfloat16", "NHWC", on_device=False) == FAST
    whole, _ = convert(dec, [f], "xyz12le", 12, mix, q, "float16", "NCHW", None, None, True)
    for factor in (1, 3, 4096):                              # knob "curves_grid": another grid, the same bits
        dec.set_int("curves_grid", factor)
        try:
            for path in (0, 1):
                dec.set_int("tensor_path", path)
                again, route = convert(dec, [f], "xyz12le", 12, mix, q, "float16", "NCHW", None, None, True)
                assert route == FAST + path and np.array_equal(again, whole), (factor, path)
            small, route = convert(dec, [f], "xyz12le", 12, mix, q, "float32", "NHWC", (50, 9), None, True, windows=None, filt=rm.BILINEAR)
            mismatch(small, cvm.batch_resized([f.arrays()], "xyz12le", 12, mix, q, "float32", "NHWC", (50, 9), None, rm.BILINEAR), factor)
        finally:
            dec.set_int("tensor_path", 0)
            dec.set_int("curves_grid", 0)
    with pytest.raises(m.Htj2kError):
        dec.set_int("curves_grid", -1)
    for fmt, bits in (("rgb24", 8), ("yuv422p10le", 10), ("yuv411p", 8)):
        gp = group_pixels(fmt)
        sizes, origins = [(72, 9), (33, 12), (64, 7), (17, 5)], [(gp or 16, 3), (3, 0), (32, 1), (0, 0)]
        fs = [HFrame(fmt, w, h, rng, "to64" if i % 2 == 0 else "row+1", 0 if i != 3 else 1) for i, (w, h) in enumerate(sizes)]
        for j, (dtype, layout, k) in enumerate((("float16", "NCHW", 3), ("float32", "NHWC", 2), ("bfloat16", "NHWC", 4))):
            route = check(dec, fs, fmt, bits, make_mix("rand", 3, k), make_curves(MODES[j], 3, k, bits, j), dtype, layout, (16, 5), origins, bool(j % 2))
            assert route == (BOTH if gp else GENERAL), (fmt, route)


def check_many_frames(dec, n=66000):
    """more frames than grid.z takes in one launch: 2 x 2 yuv420p frames out of one buffer, 16-knot tables, on both routes"""
    a = np.random.default_rng(9).integers(0, 256, size=(n, 8), dtype=np.uint8)       # Y at 0 .. 3, U at 4, V at 5
    rec = np.dtype({"names": ["data", "linesize", "width", "height", "pix_fmt"], "formats": [("<u8", 4), ("<i4", 4), "<i4", "<i4", "<i4"],
                    "offsets": [0, 32, 48, 52, 56], "itemsize": ctypes.sizeof(m.Frame)})
    t = np.zeros(n, rec)
    base = a.ctypes.data + 8 * np.arange(n, dtype=np.uint64)
    t["data"][:, 0], t["data"][:, 1], t["data"][:, 2] = base, base + 4, base + 5
    t["linesize"][:, 0], t["linesize"][:, 1], t["linesize"][:, 2] = 2, 1, 1
    t["width"], t["height"], t["pix_fmt"] = 2, 2, m.PIX_NAMES.index("yuv420p")
    mix = m.Decoder.ycbcr_mix(709, 8)
    rng = np.random.default_rng(10)
    q = m.tensor_curves(m.tensor_curve(rng.normal(128, 60, 16), 0.0, 15 / 255), m.tensor_curve(rng.normal(0, 1, 16), -0.25, 10.0), 7, 5, 2.0, -1.0)
    f = [a[:, :4].reshape(n, 2, 2).astype(np.float32), np.broadcast_to(a[:, 4, None, None], (n, 2, 2)).astype(np.float32),
         np.broadcast_to(a[:, 5, None, None], (n, 2, 2)).astype(np.float32)]
    vals = cvm.values(f, mix, q)
    for path, dtype in ((0, "float16"), (1, "bfloat16")):
        want = np.stack([mm.stored(v, dtype) for v in vals], axis=1)               # (n, 3, 2, 2)
        spec = m.tensor_spec(dtype, "NCHW")
        dec.set_int("tensor_path", path)
        try:
            r, host, at = raw_call(dec, t.ctypes.data_as(ctypes.c_void_p), 0, n, 8, spec, mix, q, None, n * 24)
        finally:
            dec.set_int("tensor_path", 0)
        assert r == 0 and dec.tensor_last_route() == (GENERAL if path else FAST)
        assert (host[:at] == 0xA5).all() and (host[at + n * 24:] == 0xA5).all()
        assert np.array_equal(host[at:at + n * 24].view(np.uint16).reshape(n, 3, 2, 2), want)


def check_refusals(dec):
    """refusals on a live context: nothing launched, dst and its guards untouched, route 0, and the context works on"""
    rng = np.random.default_rng(3)
    f = HFrame("yuv420p", 20, 10, rng)
    ok, win = m.tensor_spec("float16"), m.tensor_spec("float16", size=(4, 4))
    eye = m.tensor_mix(np.eye(3))
    ramp = lambda n=16: m.tensor_curve(np.arange(n, dtype=np.float32))

    def bad(**kw):
        q = m.tensor_curves(ramp(), ramp(4097))
        for name, v in kw.items():
            obj, field = (q, name) if "__" not in name else (getattr(q, name.rsplit("__", 1)[0]), name.rsplit("__", 1)[1])
            if field in ("gain", "offset"):
                getattr(obj, field)[1] = v
            else:
                setattr(obj, field, v)
        return q
    nan_tab = np.arange(16, dtype=np.float32)
    nan_tab[15] = math.nan
    cases = [(eye, m.tensor_curves(None, None), None), (None, bad(), None), (eye, bad(in___n=1), None), (eye, bad(out__n=4098), rm.TRIANGLE),
             (eye, bad(out__t=None), None), (eye, bad(in___x0=math.inf), None), (eye, bad(out__inv_dx=0.0), rm.BILINEAR),
             (eye, m.tensor_curves(m.tensor_curve(nan_tab), None), None), (eye, bad(in_mask=8), None), (eye, bad(out_mask=15), rm.NEAREST),
             (eye, bad(gain=math.nan), None), (eye, bad(offset=-math.inf), None)]
    good = make_curves("both", 3, 3, 8, 0)
    arr = (m.Frame * 1)(f.frame())
    for i, (mix, q, filt) in enumerate(cases):
        check(dec, [f], "yuv420p", 8, make_mix("rand", 3, 3), good)          # a call that launches, so that a route is there to be cleared
        r, host, at = raw_call(dec, arr, 0, 1, 8, ok if filt is None else win, mix, q, None, 3 * 20 * 10 * 2, 0, None, filt)
        assert r == EINVAL, (i, r)
        assert (host == 0xA5).all() and dec.tensor_last_route() == 0, i
    pal = HFrame("pal8", 20, 10, rng)
    r, host, at = raw_call(dec, (m.Frame * 1)(pal.frame()), 0, 1, 8, ok, eye, bad(in___n=1), None, 1200)
    assert r == PATCHWELCOME and (host == 0xA5).all()
    # entries that are not read may hold anything
    q = m.tensor_curves(ramp(), None, 7, 3, [1.0, 2.0, math.nan, math.inf], [0.0, 0.0, math.nan, math.nan])
    q.out.x0, q.out.inv_dx = math.nan, -1.0
    check(dec, [f], "yuv420p", 8, make_mix("rand", 3, 2), q, "float32", "NHWC")


def check_python(dec):
    """the keyword on the methods that take planes: shapes, `out`, the helpers"""
    rng = np.random.default_rng(12)
    fs = [HFrame("xyz12le", 34, 6, rng), HFrame("xyz12le", 34, 6, rng)]
    planes = [f.arrays() for f in fs]
    mix, q = m.Decoder.dcp_curves(709, "srgb", gain=2.0, offset=-1.0)
    t = dec.to_tensor(planes, "xyz12le", 12, mix=mix, curves=q)
    assert t.dtype == torch.float16 and tuple(t.shape) == (2, 3, 6, 34) and dec.tensor_last_route() == FAST and dec.compare_ms() > 0
    assert np.array_equal(tensor_bits(t), cvm.batch(planes, "xyz12le", 12, mix, q, "float16"))
    out = torch.zeros((2, 4, 5, 3), dtype=torch.bfloat16, device="cuda")
    t2 = dec.to_tensor(planes, "xyz12le", 12, torch.bfloat16, "NHWC", size=(5, 4), origins=(7, 1), out=out, mix=mix, curves=q)
    assert t2 is out and np.array_equal(tensor_bits(out), cvm.batch(planes, "xyz12le", 12, mix, q, "bfloat16", "NHWC", (5, 4), [(7, 1)] * 2))
    with pytest.raises(ValueError):
        dec.to_tensor(planes, "xyz12le", 12, curves=q)           # curves without a mix
    with pytest.raises(ValueError):
        dec.to_tensor(planes, "xyz12le", 12, mix=mix, curves=(q.tables[0], None))
    t3 = dec.to_tensor_resized(planes, "xyz12le", 12, (9, 4), windows=(2, 0, 30, 6), filter="bilinear", dtype="float32", mix=mix, curves=q)
    assert tuple(t3.shape) == (2, 3, 4, 9) and dec.tensor_last_route() == RESIZED
    assert np.array_equal(tensor_bits(t3), cvm.batch_resized(planes, "xyz12le", 12, mix, q, "float32", "NCHW", (9, 4), [(2, 0, 30, 6)] * 2, rm.BILINEAR))
    # the accuracy of the whole chain on the device: within 3e-5 of the true functions, as the model is
    f, comps = all_samples_frame(8)
    mix, q = m.Decoder.dcp_curves(709, "srgb", 4097)
    got = dec.to_tensor([f.arrays()], "xyz12le", 12, "float32", "NHWC", mix=mix, curves=q)[0].cpu().numpy().astype(np.float64)
    assert np.abs(got - cvm.dcp_true(np.stack(comps, -1), 709, "srgb")).max() <= 3e-5


def check_jobs(dec, orc):
    """the catalogue's rgb24 stream and a 10-bit one against the oracle's frames through the model"""
    job = dec.job()
    for li, (fmt, datas) in enumerate((("rgb24", [streams.get("rgb_mct")[0]] * 2), ("yuv422p10le", [yuv422p10_stream()] * 2))):
        job.parse_batch(datas).upload().run()
        info = job.frame_info(0)
        assert m.PIX_NAMES[info.pix_fmt] == fmt
        bits = info.bits_per_raw_sample
        want_planes = [orc.decode(d)[1] for d in datas]
        # R'G'B' or Y'CbCr to linear light: the matrix (for rgb24 a scaling) first, the sRGB or BT.709 decode after it
        mix = m.tensor_mix(np.eye(3) / 255) if fmt == "rgb24" else m.Decoder.ycbcr_mix(709, bits)
        q = m.tensor_curves(None, m.tensor_curve(m.curve_table("srgb_decode" if fmt == "rgb24" else "bt709_decode", 4097), 0.0, 4096.0))
        t, status = job.to_tensor("float16", "NCHW", mix=mix, curves=q)                         # bits 0: the job's
        assert status == [0, 0] and tuple(t.shape) == (2, 3, info.height, info.width) and dec.tensor_last_route() in (FAST, GENERAL, BOTH)
        assert np.array_equal(tensor_bits(t), cvm.batch(want_planes, fmt, bits, mix, q, "float16")), fmt
        four, q4 = make_mix("rand", 3, 4), make_curves("both", 3, 4, bits, li)
        t, status = job.to_tensor("float32", "NHWC", size=(24, 10), origins=[(16, 3), (5, 1)], bits=bits, mix=four, curves=q4)
        assert tuple(t.shape) == (2, 10, 24, 4) and dec.tensor_last_route() in (FAST, GENERAL, BOTH)
        assert np.array_equal(tensor_bits(t), cvm.batch(want_planes, fmt, bits, four, q4, "float32", "NHWC", (24, 10), [(16, 3), (5, 1)])), fmt
        wins = [(1, 1, info.width - 2, info.height - 2), (0, 0, info.width, info.height)]
        t, status = job.to_tensor_resized((13, 9), wins, "triangle", "bfloat16", "NHWC", mix=four, curves=q4)
        assert status == [0, 0] and tuple(t.shape) == (2, 9, 13, 4) and dec.tensor_last_route() == RESIZED
        assert np.array_equal(tensor_bits(t), cvm.batch_resized(want_planes, fmt, bits, four, q4, "bfloat16", "NHWC", (13, 9), wins, rm.TRIANGLE)), fmt
        with pytest.raises(m.Htj2kError) as e:                # curves that are refused
            job.to_tensor("float16", "NCHW", mix=mix, curves=m.tensor_curves(None, None))
        assert e.value.code == EINVAL
    job.free()


def check_pipes(dec, orc, wait=60):
    """a pipe with a packet that fails and a damaged one, received with curves, with curves resized and without in turn"""
    names = ["yuv420p8", "rgb_mct", "gray_l5_cb64"]
    pkts = [streams.get(names[i % 3])[0] for i in range(9)]
    pkts[2] = pkts[2][:40]                                   # fails to parse: its batch is retried packet by packet
    pkts[5] = damaged_copy(pkts[5])                          # parses, some blocks rejected: still a frame
    pkts[8] = damaged_copy(pkts[8], 1)
    how = ["curves", "resized", None, "curves", "mix", "resized", "curves", "resized", "curves"]
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
                    bounded(lambda: pipe.receive_tensor(mix=make_mix("rand", 3, 3), curves=make_curves("both", 3, 3, 8, 0)), wait)
                assert e.value.code < 0 and e.value.code != m.EAGAIN
                got += 1
                continue
            info_o, planes_o = want[got]
            fmt, bits = m.PIX_NAMES[info_o.pix_fmt], info_o.bits_per_raw_sample
            nc, k = tm.ncomp(fmt), 1 + got % 4
            mix, q = make_mix("rand", nc, k, got), make_curves(MODES[got % 3], nc, k, bits, got)
            if how[got] == "curves":
                t, info = bounded(lambda: pipe.receive_tensor("float16", "NCHW", mix=mix, curves=q), wait)
                assert np.array_equal(tensor_bits(t), cvm.image(planes_o, fmt, bits, mix, q, "float16")[None]), got
            elif how[got] == "mix":
                t, info = bounded(lambda: pipe.receive_tensor("float16", "NCHW", mix=mix), wait)
                assert np.array_equal(tensor_bits(t), mm.image(planes_o, fmt, bits, mix, "float16")[None]), got
            else:
                t, info = bounded(lambda: pipe.receive_tensor_resized((11, 7), None, "bilinear", "float32", "NHWC", mix=mix, curves=q), wait)
                assert np.array_equal(tensor_bits(t), cvm.image_resized(planes_o, fmt, bits, mix, q, "float32", "NHWC", (11, 7), None, rm.BILINEAR)[None]), got
            assert (info.width, info.height, info.pix_fmt) == (info_o.width, info_o.height, info_o.pix_fmt), got
            got += 1
        assert bounded(lambda: pipe.receive_tensor(mix=make_mix("rand", 3, 3), curves=make_curves("in", 3, 3, 8, 0)), wait) is None      # drained
    finally:
        bounded(pipe.close, wait)


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


def test_the_sweep_covers_what_it_claims():
    """no device: every layout's sweep meets every K, element type, tensor layout and kind of curves, on each route it has"""
    for li, fmt in enumerate(LAYOUTS):
        seen = set()
        for w, h, bits, mode, k, dtype, layout, on_device, ls, off, j in layout_cases(fmt, li):
            geo = m.plane_geometry(fmt, w, h)
            lss = [{"row": rb, "row+1": rb + 1, "row+13": rb + 13, "to64": -(-rb // 64) * 64}[ls] for _, rb in geo]
            aligned = (not on_device) or (off % 16 == 0 and all(v % 16 == 0 for v in lss))
            seen.update([FAST if group_pixels(fmt) and aligned else GENERAL, k, dtype, layout if k > 1 else "NCHW", mode])
        assert GENERAL in seen and (not group_pixels(fmt) or FAST in seen), (fmt, sorted(map(str, seen)))
        assert seen >= {1, 2, 3, 4} | set(tm.DTYPES) | set(LAYOUT_NAMES) | set(MODES), (fmt, sorted(map(str, seen)))
    sizes = {make_curves(mode, 3, 3, 8, j).in_.n for j in range(5) for mode in ("in", "both")}
    assert sizes == set(KNOTS)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_layouts_rows_linesizes_offsets(dec, fmt):
    check_layout(dec, fmt, LAYOUTS.index(fmt))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_windows(dec, fmt):
    check_windows(dec, fmt, LAYOUTS.index(fmt))


@pytest.mark.gpu
def test_corners_of_the_definition(dec):
    check_corners(dec)


@pytest.mark.gpu
def test_identity_curve_is_the_mix_call(dec):
    check_identity(dec)


@pytest.mark.gpu
def test_torch_eager_chain_on_the_device(dec):
    check_torch_chain(dec)


@pytest.mark.gpu
def test_resized_calls(dec):
    check_resized(dec)


@pytest.mark.gpu
def test_several_workgroups_and_unlike_frames(dec):
    check_sizes(dec)


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
    check_corners(dec)
    check_identity(dec)
    check_torch_chain(dec)
    check_resized(dec)
    check_sizes(dec)
    check_many_frames(dec)
    check_refusals(dec)
    check_python(dec)
    check_jobs(dec, orc)
    check_pipes(dec, orc)


POISON_TIMEOUT = 300


@pytest.mark.gpu
def test_everything_on_poisoned_buffers():
    """HTJ2K_POISON=1 (read once per process, so a fresh child): every new device buffer of the library, the scratch of
    the resized calls and the uploaded tables included, starts as 0xA5 bytes, and all of the above must still give the
    model's results.  The child's exit status comes first."""
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
