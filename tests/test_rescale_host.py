"""Resized frames without a device: the symbols, htj2k_frame_plane_sizes against the oracle's htj2k_info for every layout,
every refusal of htj2k_resize_frames in its order with a NULL context, and the numpy model (resize_frames_model) against
exact rationals, a numpy crop, the header's statement about the planes' reduction, and torch's interpolate on the CPU."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cmp_model as cm
import ffmpeg_ht_amd as m
import oracle
import resize_frames_model as fm
import resize_model as rm
import vecgen
from test_tensor_host import frame

EINVAL, ENOSYS, PATCHWELCOME = -22, -38, -0x45574150
FILTERS = [fm.NEAREST, fm.BILINEAR, fm.TRIANGLE]


@pytest.fixture(scope="module")
def L():
    return m.load_library()


def call(L, src, dst, bits=8, windows=None, filt=2, n=None):
    sarr = (m.Frame * len(src))(*src) if src is not None else None
    darr = (m.Frame * len(dst))(*dst) if dst is not None else None
    win = None if windows is None else (ctypes.c_int32 * len(windows))(*windows)
    return L.htj2k_resize_frames(None, sarr, 0, len(src) if n is None else n, bits, win, filt, darr)


def test_symbols_and_the_header(L):
    for name in ("htj2k_resize_frames", "htj2k_job_resize_frames", "htj2k_pipe_receive_resized", "htj2k_frame_plane_sizes"):
        assert hasattr(L, name) and name in m.EXPORTS
    for name in ("Decoder.resize_frames", "Decoder.plane_sizes", "Job.resized_frames", "Pipe.receive_resized"):
        cls, fn = name.split(".")
        assert callable(getattr(getattr(m, cls), fn))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "htj2k_amd.h")).read()
    for name in ("htj2k_resize_frames", "htj2k_job_resize_frames", "htj2k_pipe_receive_resized", "htj2k_frame_plane_sizes"):
        assert name + "(" in header
    out_of_scope = [s for s in header.split("Out of scope:")[1:] if "Lanczos" in s.split("*/")[0]]
    assert out_of_scope and all("a scaler that writes frames" not in s.split("*/")[0] for s in out_of_scope)


def layout_stream(name, w, h):
    """a small codestream that the parser hands out in layout `name` when asked to"""
    rng = np.random.default_rng(5)
    if name == "pal8":
        cs = vecgen.encode([rng.integers(0, 4, (h, w))], nlevels=1)
        return vecgen.jp2_wrap(cs, w, h, 1, 8, palette=[(i, 2 * i, 3 * i) for i in range(4)])
    nc, _, cw, ch, depth, _ = cm.LAYOUTS[name]
    dx = [1 << cw if c in (1, 2) else 1 for c in range(nc)]
    dy = [1 << ch if c in (1, 2) else 1 for c in range(nc)]
    comps = [rng.integers(0, 1 << depth, (-(-h // dy[c]), -(-w // dx[c]))) for c in range(nc)]
    return vecgen.encode(comps, depth=depth, dx=dx, dy=dy, nlevels=1, width=w, height=h)


@pytest.mark.parametrize("size", [(37, 23), (4, 1)])
def test_plane_sizes_equal_the_info_of_every_layout(size):
    w, h = size
    orc = oracle.OracleDecoder()
    for fmt, name in enumerate(m.PIX_NAMES):
        info = orc.probe(layout_stream(name, w, h), req_pix_fmt=fmt)
        assert info.pix_fmt == fmt and (info.width, info.height) == (w, h), name
        n, pw, ph, rb = m.Decoder.plane_sizes(name, w, h)
        assert n == info.nplanes and len(pw) == len(ph) == len(rb) == n, name
        assert pw == list(info.plane_width[:n]) and ph == list(info.plane_height[:n]), name
        assert rb == [info.plane_width[p] * info.plane_bytes_per_sample[p] for p in range(n)], name
        if name != "pal8":
            assert [(r, b) for r, b in zip(ph, rb)] == m.plane_geometry(name, w, h), name
    orc.close()
    Lib = m.load_library()
    a, b, c = (ctypes.c_int * 4)(), (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
    assert Lib.htj2k_frame_plane_sizes(1, w, h, None, None, None) == 1                 # the count alone
    for bad in ((-1, w, h), (len(m.PIX_NAMES), w, h), (1, 0, h), (1, w, 0), (1, -3, h)):
        assert Lib.htj2k_frame_plane_sizes(bad[0], bad[1], bad[2], a, b, c) == EINVAL, bad


def test_refusals_in_their_order_with_a_null_context(L):
    f, d = frame("yuv420p", 20, 10), frame("yuv420p", 8, 6)
    assert call(L, [f], [d]) == ENOSYS                                     # valid arguments, no context
    assert call(L, [f, frame("yuv420p", 33, 7)], [d, d], windows=[4, 2, 15, 7, 0, 0, 33, 7], filt=1) == ENOSYS
    pal, bad_fmt = frame("pal8", 20, 10), frame("yuv420p", 20, 10)
    bad_fmt.pix_fmt = len(m.PIX_NAMES)
    # 1, 2: missing arguments and n come before the layout
    assert call(L, None, [d], n=1) == EINVAL and call(L, [pal], None) == EINVAL and call(L, [pal], [d], n=0) == EINVAL
    assert call(L, [pal], [d], n=-1) == EINVAL
    # 3: the layout comes before bits and the filter
    assert call(L, [pal], [pal], bits=99, filt=9) == PATCHWELCOME
    assert call(L, [bad_fmt], [d], bits=99, filt=9) == EINVAL
    # 4: bits
    for bits in (0, 9, -1):
        assert call(L, [f], [d], bits=bits) == EINVAL
    assert call(L, [f], [d], bits=7) == ENOSYS
    # 5: the filter
    for filt in (-1, 3, 100):
        assert call(L, [f], [d], filt=filt) == EINVAL
    for filt in (0, 1, 2):
        assert call(L, [f], [d], filt=filt) == ENOSYS
    # 6: the sources: one layout, a size, planes, linesizes -- and sizes may differ
    assert call(L, [f, frame("yuv422p", 20, 10)], [d, d]) == EINVAL
    assert call(L, [f, frame("yuv420p", 21, 11)], [d, d]) == ENOSYS
    assert call(L, [frame("yuv420p", 0, 10)], [d]) == EINVAL
    g = frame("yuv420p", 20, 10)
    g.data[1] = None
    assert call(L, [g], [d]) == EINVAL
    g = frame("yuv420p", 20, 10)
    g.linesize[2] = 9
    assert call(L, [g], [d]) == EINVAL
    g.linesize[2] = -10
    assert call(L, [g], [d]) == EINVAL
    # 7: the destinations: the sources' layout, one size, at least 1
    assert call(L, [f], [frame("yuv422p", 8, 6)]) == EINVAL
    assert call(L, [f, f], [d, frame("yuv420p", 8, 7)]) == EINVAL
    assert call(L, [f], [frame("yuv420p", 0, 6)]) == EINVAL and call(L, [f], [frame("yuv420p", 8, -1)]) == EINVAL
    # 8, 9, 10: the windows
    for bad in ([0, 0, 0, 4], [0, 0, 4, 0], [0, 0, -3, 4], [-2, 0, 4, 4], [0, -2, 4, 4], [18, 0, 4, 4], [0, 8, 4, 4], [0, 0, 21, 10], [0, 0, 20, 11],
                [2 ** 31 - 1, 0, 2 ** 31 - 1, 1]):
        assert call(L, [f], [d], windows=bad) == EINVAL, bad
    assert call(L, [f], [d], windows=[16, 6, 4, 4]) == ENOSYS and call(L, [f], [d], windows=[18, 8, 1, 1]) == ENOSYS
    assert call(L, [f, f], [d, d], windows=[0, 0, 4, 4, 0, 0, 4, -4]) == EINVAL
    # 11: an origin off the chroma grid; sizes need not be on it
    for bad in ([1, 0, 4, 4], [0, 1, 4, 4], [3, 5, 4, 4]):
        assert call(L, [f], [d], windows=bad) == EINVAL, bad
    assert call(L, [f], [d], windows=[2, 4, 5, 3]) == ENOSYS
    f411, d411 = frame("yuv411p", 20, 10), frame("yuv411p", 8, 6)
    assert call(L, [f411], [d411], windows=[2, 0, 4, 4]) == EINVAL and call(L, [f411], [d411], windows=[4, 1, 4, 4]) == ENOSYS
    f440, d440 = frame("yuv440p", 20, 10), frame("yuv440p", 8, 6)
    assert call(L, [f440], [d440], windows=[1, 2, 4, 4]) == ENOSYS and call(L, [f440], [d440], windows=[0, 1, 4, 4]) == EINVAL
    rgb, drgb = frame("rgb24", 20, 10), frame("rgb24", 8, 6)
    assert call(L, [rgb], [drgb], windows=[3, 5, 4, 4]) == ENOSYS
    # 12: out of scope: a size, a reduction; after every window's own refusals, before the destination's
    big = frame("gray", 40000, 2)
    small = frame("gray", 4, 2)
    assert call(L, [big], [small], filt=1) == PATCHWELCOME and call(L, [big], [small], windows=[0, 0, 32769, 2], filt=0) == PATCHWELCOME
    assert call(L, [big], [frame("gray", 1024, 2)], windows=[7232, 0, 32768, 2]) == ENOSYS
    assert call(L, [small], [frame("gray", 32769, 2)], filt=0) == PATCHWELCOME and call(L, [small], [frame("gray", 2, 32769)], filt=1) == PATCHWELCOME
    assert call(L, [small], [frame("gray", 32768, 2)]) == ENOSYS
    wide, two = frame("yuv420p", 130, 10), frame("yuv420p", 2, 10)
    assert call(L, [wide], [two]) == PATCHWELCOME
    assert call(L, [wide], [two], filt=1) == ENOSYS and call(L, [wide], [two], filt=0) == ENOSYS
    assert call(L, [wide], [two], windows=[2, 0, 128, 10]) == ENOSYS
    assert call(L, [frame("gray", 10, 130)], [frame("gray", 10, 2)]) == PATCHWELCOME
    assert call(L, [wide], [two], windows=[1, 0, 129, 10]) == EINVAL                                   # off the grid: first
    assert call(L, [wide, wide], [two, two], windows=[0, 0, 130, 10, 0, 0, 131, 10]) == EINVAL         # frame 1 leaves its frame: first
    g = frame("yuv420p", 2, 10)
    g.data[2] = None
    assert call(L, [wide], [g]) == PATCHWELCOME                                                        # before the destination's planes
    # 13: the destination's planes and linesizes
    g = frame("yuv420p", 8, 6)
    g.data[0] = None
    assert call(L, [f], [g]) == EINVAL
    for p, ls in ((0, 7), (1, 3), (2, -4)):
        g = frame("yuv420p", 8, 6)
        g.linesize[p] = ls
        assert call(L, [f], [g]) == EINVAL, (p, ls)
    g = frame("yuv420p", 7, 5)                                             # ceilinged chroma: 4 x 3
    g.linesize[1] = 3
    assert call(L, [f], [g]) == EINVAL
    g.linesize[1] = 4
    assert call(L, [f], [g]) == ENOSYS


def test_job_and_pipe_calls_refuse_their_arguments(L):
    d = (m.Frame * 1)(frame("gray", 4, 4))
    assert L.htj2k_job_resize_frames(None, None, 0, None, 2, d, None) == EINVAL
    assert L.htj2k_pipe_receive_resized(None, None, 0, None, 2, d) == EINVAL


def exact(src, dw, dh, filt):
    """the definition in rationals: weights q / 2^14 of either axis, the sum rounded half up"""
    ph, pw = src.shape
    out = np.zeros((dh, dw), np.int64)
    for y in range(dh):
        fy, qy = rm.weights(ph, dh, filt, y)
        for x in range(dw):
            fx, qx = rm.weights(pw, dw, filt, x)
            v = sum(Fraction(a, 1 << 14) * Fraction(b, 1 << 14) * int(src[fy + j, fx + i]) for j, a in enumerate(qy) for i, b in enumerate(qx))
            out[y, x] = (v + Fraction(1, 2)).__floor__()
    return out


def test_model_against_exact_rationals_on_small_planes():
    rng = np.random.default_rng(21)
    for (h, w), (oh, ow) in (((1, 1), (4, 4)), ((4, 4), (1, 1)), ((5, 7), (3, 2)), ((3, 2), (5, 7)), ((9, 11), (4, 5)), ((2, 40), (2, 3))):
        for bits in (1, 8, 16):
            src = rng.integers(0, 1 << bits, (h, w))
            for filt in FILTERS:
                assert np.array_equal(fm.rescale(src, ow, oh, filt), exact(src, ow, oh, filt)), ((h, w), (oh, ow), bits, filt)


def random_planes(fmt, w, h, rng):
    b = cm.LAYOUTS[fmt][5]
    return [rng.integers(0, 1 << (8 * b), shape, dtype=np.uint8 if b == 1 else np.uint16) for shape in cm.plane_shapes(fmt, w, h)]


def test_identity_is_a_crop_and_constants_stay_constant():
    rng = np.random.default_rng(22)
    for fmt in ("gray", "ya8", "rgb24", "rgba64le", "yuv410p", "yuv411p", "yuv420p", "yuv440p", "yuva420p", "yuv422p10le", "xyz12le"):
        depth, st = cm.LAYOUTS[fmt][4], fm.step(fmt)
        planes = random_planes(fmt, 45, 19, rng)
        for window, filt in (((0, 0, 45, 19), fm.TRIANGLE), ((8, 4, 33, 15), fm.BILINEAR), ((16, 8, 13, 5), fm.NEAREST)):
            for bits in (depth, depth - 1):
                got = fm.frame(planes, fmt, bits, window[2:], window, filt)
                sh, mask = cm.shift(fmt, bits), (1 << bits) - 1
                for p, g, (sw, shh) in zip(planes, got, fm.plane_shifts(fmt)):
                    px, py, pw, ph = fm.plane_window(window, sw, shh)
                    crop = p[py:py + ph, px * st:(px + pw) * st]
                    assert g.dtype == p.dtype and np.array_equal(g, ((crop >> sh) & mask) << sh), (fmt, window, bits)
        for value in (0, (1 << depth) - 1):
            word = value << cm.shift(fmt, depth)
            const = [np.full(p.shape, word, p.dtype) for p in planes]
            for size in ((7, 3), (90, 40), (45, 5)):
                for filt in FILTERS:
                    assert all((g == word).all() for g in fm.frame(const, fmt, depth, size, None, filt)), (fmt, value, size)


def test_a_reduction_in_scope_for_the_frame_is_in_scope_for_every_plane():
    """the header's statement: ww <= 64 out_w implies pw <= 64 dw for shifts 0, 1 and 2, by brute force"""
    for out_w in range(1, 41):
        for ww in range(1, 64 * out_w + 1):
            for s in (0, 1, 2):
                assert fm.cdiv(ww, s) <= 64 * fm.cdiv(out_w, s), (ww, out_w, s)
        assert any(fm.cdiv(64 * out_w + 1, s) > 64 * fm.cdiv(out_w, s) for s in (0, 1, 2))      # and the frame's limit is the tight one


# frames (w, h) -> (out_w, out_h): down, up, mixed, one pixel either side, 128 taps either way
SHAPES = [((37, 23), (16, 9)), ((37, 23), (75, 50)), ((1, 1), (4, 4)), ((4, 4), (1, 1)), ((29, 13), (5, 31)), ((1024, 4), (16, 4)), ((16, 1024), (16, 16))]
TORCH_LAYOUTS = ["gray", "rgb24", "gray16le", "yuv420p", "yuv410p", "yuv411p", "yuv440p", "yuv422p10le", "xyz12le"]


def test_model_against_torch_interpolate_plane_by_plane(capsys):
    """Not bit for bit: the weights are 14-bit.  Each is off by less than 2^-14 and one tap carries a remainder below
    taps * 2^-14, so a sample differs by less than peak * 2 * (taps_x + taps_y) * 2^-14 before it is rounded; 2^-18 more
    covers torch's own binary32 sums, and 0.5 the integer rounding."""
    rng = np.random.default_rng(23)
    worst = 0.0
    for (w, h), (ow, oh) in SHAPES:
        for fmt in TORCH_LAYOUTS:
            depth, st = cm.LAYOUTS[fmt][4], fm.step(fmt)
            peak, sh = (1 << depth) - 1, cm.shift(fmt, depth)
            planes = random_planes(fmt, w, h, rng)
            for filt, aa in ((fm.BILINEAR, False), (fm.TRIANGLE, True)):
                got = fm.frame(planes, fmt, depth, (ow, oh), None, filt)
                for p, g in zip(planes, got):
                    for c in range(st):
                        src = ((p[:, c::st].astype(np.int64) >> sh) & peak)
                        (ph, pw), (dh, dw) = src.shape, g[:, c::st].shape
                        t = torch.from_numpy(src.astype(np.float32))[None, None]
                        want = F.interpolate(t, size=(dh, dw), mode="bilinear", align_corners=False, antialias=aa)[0, 0].numpy()
                        taps_x = max(len(rm.weights(pw, dw, filt, x)[1]) for x in range(dw))
                        taps_y = max(len(rm.weights(ph, dh, filt, y)[1]) for y in range(dh))
                        bound = 0.5 + peak * (2 * (taps_x + taps_y) * 2.0 ** -14 + 2.0 ** -18)
                        err = float(np.abs((g[:, c::st].astype(np.int64) >> sh).astype(np.float64) - want.astype(np.float64)).max())
                        worst = max(worst, err / bound)
                        assert err <= bound, (fmt, (w, h), (ow, oh), filt, c, err, bound)
            got = fm.frame(planes, fmt, depth, (ow, oh), None, fm.NEAREST)
            for p, g in zip(planes, got):
                for c in range(st):
                    src = ((p[:, c::st].astype(np.int64) >> sh) & peak)
                    dh, dw = g[:, c::st].shape
                    want = F.interpolate(torch.from_numpy(src.astype(np.float32))[None, None], size=(dh, dw), mode="nearest-exact")[0, 0].numpy()
                    assert np.array_equal((g[:, c::st].astype(np.int64) >> sh).astype(np.float32), want), (fmt, (w, h), (ow, oh), c)
    assert max(len(rm.weights(1024, 16, rm.TRIANGLE, x)[1]) for x in range(16)) == 128
    with capsys.disabled():
        print("\nresized frames model against torch: the largest error is %.3f of its bound" % worst)
