"""Tensors as frames without a device: the symbols, every refusal of htj2k_encode_tensor and htj2k_tensor_to_frames in
its order with a NULL context, and the numpy model (tensor_in_model) against torch on the CPU, at the corners of the
number formats, and as the right inverse of tensor_model."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cmp_model as cm
import ffmpeg_ht_amd as m
import tensor_in_model as tim
import tensor_model as tm
from test_tensor_host import FAMILIES, PAIRS, frame

EINVAL, ENOSYS, PATCHWELCOME = -22, -38, -0x45574150
BITS = [1, 8, 10, 16]


@pytest.fixture(scope="module")
def L():
    return m.load_library()


def enc_call(L, spec, fmt="yuv420p", w=20, h=10, bits=8, n=1, src=0x1000, src_bytes=1 << 40, out=0x1000, offsets=True, ctx=None):
    """htj2k_encode_tensor on memory that is never touched: refusals come before the context, and a NULL context ends the call"""
    offs = (ctypes.c_size_t * (abs(n) + 2))()
    pix = m.PIX_NAMES.index(fmt) if isinstance(fmt, str) else fmt
    return L.htj2k_encode_tensor(ctx, ctypes.c_void_p(src), ctypes.c_size_t(src_bytes), n, w, h, pix, bits,
                                 None if spec is None else ctypes.byref(spec), None, ctypes.c_void_p(out), ctypes.c_size_t(1 << 20), 0,
                                 offs if offsets else None)


def frames_call(L, spec, frames, bits=8, n=None, src=0x1000, src_bytes=1 << 40, ctx=None):
    arr = (m.Frame * len(frames))(*frames) if frames is not None else None
    return L.htj2k_tensor_to_frames(ctx, ctypes.c_void_p(src), ctypes.c_size_t(src_bytes), len(frames) if n is None else n, bits,
                                    None if spec is None else ctypes.byref(spec), arr)


def _spec(**kw):
    s = m.tensor_spec("float16")
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _bad_float(field, k, v):
    s = m.tensor_spec("float16")
    getattr(s, field)[k] = v
    return s


def test_symbols():
    L = m.load_library()
    for name in ("htj2k_encode_tensor", "htj2k_tensor_to_frames"):
        assert hasattr(L, name) and name in m.EXPORTS
    assert callable(m.Encoder.encode_tensor) and callable(m.Decoder.from_tensor)


def test_encode_tensor_refuses_in_its_order_with_a_null_context(L):
    ok = m.tensor_spec("float16")
    bad_all = _spec(dtype=7, layout=9, out_w=-1)             # everything from refusal 6 on is wrong with it
    assert enc_call(L, ok) == ENOSYS                         # valid arguments, no context
    assert enc_call(L, m.tensor_spec("float32", "NHWC"), "rgb48le", 7, 3, 12, n=5) == ENOSYS
    assert enc_call(L, ok, "xyz12le", bits=12) == ENOSYS     # the encoder's own refusal comes after the context
    # 1: a missing argument, before everything else (PAL8 would answer PATCHWELCOME at 4)
    assert enc_call(L, ok, "pal8", src=0) == EINVAL
    assert enc_call(L, None, "pal8") == EINVAL
    assert enc_call(L, ok, "pal8", out=0) == EINVAL
    assert enc_call(L, ok, "pal8", offsets=False) == EINVAL
    # 2 and 3, before the layout
    assert enc_call(L, ok, "pal8", n=0) == EINVAL and enc_call(L, ok, "pal8", n=-2) == EINVAL
    assert enc_call(L, ok, "pal8", w=0) == EINVAL and enc_call(L, ok, "pal8", h=0) == EINVAL and enc_call(L, ok, "pal8", w=-5) == EINVAL
    # 4: the layout, before bits, dtype, layout, scale, bias, the window, the size and the alignment
    assert enc_call(L, bad_all, "pal8", bits=99, src_bytes=0, src=0x1001) == PATCHWELCOME
    assert enc_call(L, _bad_float("scale", 0, math.nan), "pal8") == PATCHWELCOME
    for bad_fmt in (-1, len(m.PIX_NAMES), 1000):
        assert enc_call(L, ok, bad_fmt) == EINVAL
    # 5
    for bits in (0, -1, 9):
        assert enc_call(L, ok, bits=bits) == EINVAL
    assert enc_call(L, ok, "yuv422p10le", bits=11) == EINVAL and enc_call(L, ok, "yuv422p10le", bits=10) == ENOSYS
    # 6
    for kw in (dict(dtype=-1), dict(dtype=3), dict(layout=-1), dict(layout=2)):
        assert enc_call(L, _spec(**kw)) == EINVAL
    # 7: only the first C entries are read
    for field in ("scale", "bias"):
        for v in (math.nan, math.inf, -math.inf):
            for k in range(3):
                assert enc_call(L, _bad_float(field, k, v)) == EINVAL
            assert enc_call(L, _bad_float(field, 3, v)) == ENOSYS            # yuv420p has three components
            assert enc_call(L, _bad_float(field, 1, v), "gray") == ENOSYS
    # 8: no window in this direction, not even the whole frame
    for ow, oh in ((0, 1), (1, 0), (-1, -1), (20, 10), (4, 4), (21, 10)):
        assert enc_call(L, _spec(out_w=ow, out_h=oh)) == EINVAL
    # 9
    need = 3 * 20 * 10 * 2
    assert enc_call(L, ok, src_bytes=need) == ENOSYS and enc_call(L, ok, src_bytes=need - 1) == EINVAL
    assert enc_call(L, ok, n=3, src_bytes=3 * need - 1) == EINVAL and enc_call(L, ok, src_bytes=0) == EINVAL
    assert enc_call(L, m.tensor_spec("float32"), src_bytes=2 * need - 1) == EINVAL
    # 10: the element's own alignment, nothing more; 9 comes before it
    assert enc_call(L, ok, src=0x1001) == EINVAL and enc_call(L, ok, src=0x1002) == ENOSYS
    assert enc_call(L, m.tensor_spec("float32"), src=0x1002) == EINVAL and enc_call(L, m.tensor_spec("float32"), src=0x1004) == ENOSYS
    assert enc_call(L, m.tensor_spec("bfloat16"), src=0x1001) == EINVAL
    assert enc_call(L, ok, src=0x1001, src_bytes=need - 1) == EINVAL


def test_tensor_to_frames_refuses_in_its_order_with_a_null_context(L):
    ok = m.tensor_spec("float16")
    f = frame("yuv420p", 20, 10)
    pal = frame("pal8", 20, 10)
    assert frames_call(L, ok, [f]) == ENOSYS
    assert frames_call(L, m.tensor_spec("float32", "NHWC"), [frame("xyz12le", 7, 3)] * 4, bits=12) == ENOSYS     # XYZ12 is in scope here
    # 1 and 2 come before the layout
    assert frames_call(L, ok, [pal], src=0) == EINVAL and frames_call(L, None, [pal]) == EINVAL and frames_call(L, ok, None, n=1) == EINVAL
    assert frames_call(L, ok, [pal], n=0) == EINVAL and frames_call(L, ok, [pal], n=-3) == EINVAL
    # 3
    assert frames_call(L, _spec(dtype=7, layout=9, out_w=-1), [pal], bits=99, src_bytes=0) == PATCHWELCOME
    for bad_fmt in (-1, len(m.PIX_NAMES), 1000):
        g = frame("gray", 20, 10)
        g.pix_fmt = bad_fmt
        assert frames_call(L, ok, [g]) == EINVAL
    # 4
    for bits in (0, -1, 9):
        assert frames_call(L, ok, [f], bits=bits) == EINVAL
    assert frames_call(L, ok, [frame("xyz12le", 20, 10)], bits=13) == EINVAL
    # 5
    for kw in (dict(dtype=-1), dict(dtype=3), dict(layout=-1), dict(layout=2)):
        assert frames_call(L, _spec(**kw), [f]) == EINVAL
    # 6
    for field in ("scale", "bias"):
        for v in (math.nan, math.inf, -math.inf):
            for k in range(3):
                assert frames_call(L, _bad_float(field, k, v), [f]) == EINVAL
            assert frames_call(L, _bad_float(field, 3, v), [f]) == ENOSYS
    # 7
    for ow, oh in ((0, 1), (1, 0), (-1, -1), (20, 10), (4, 4)):
        assert frames_call(L, _spec(out_w=ow, out_h=oh), [f]) == EINVAL
    # 8: one layout, one size, a size of at least 1
    assert frames_call(L, ok, [f, frame("yuv422p", 20, 10)]) == EINVAL
    assert frames_call(L, ok, [f, frame("yuv420p", 21, 10)]) == EINVAL and frames_call(L, ok, [f, frame("yuv420p", 20, 11)]) == EINVAL
    assert frames_call(L, ok, [frame("yuv420p", 0, 10)]) == EINVAL and frames_call(L, ok, [frame("yuv420p", 20, -1)]) == EINVAL
    # 9
    for p in range(3):
        g = frame("yuv420p", 20, 10)
        g.data[p] = None
        assert frames_call(L, ok, [f, g]) == EINVAL
    g = frame("gray", 20, 10)
    g.data[1] = None                                         # a plane the layout lacks is not asked for
    assert frames_call(L, ok, [g]) == ENOSYS
    # 10
    for p, short in ((0, 19), (1, 9), (2, 9), (0, -20)):
        g = frame("yuv420p", 20, 10)
        g.linesize[p] = short
        assert frames_call(L, ok, [g]) == EINVAL
    g = frame("yuv420p", 21, 11)                             # ceilinged chroma: 11 samples a row
    g.linesize[1] = 10
    assert frames_call(L, ok, [g]) == EINVAL
    # 11, then 12
    need = 3 * 20 * 10 * 2
    assert frames_call(L, ok, [f], src_bytes=need) == ENOSYS and frames_call(L, ok, [f], src_bytes=need - 1) == EINVAL
    assert frames_call(L, ok, [f, f], src_bytes=2 * need - 1) == EINVAL
    assert frames_call(L, ok, [f], src=0x1001) == EINVAL and frames_call(L, ok, [f], src=0x1002) == ENOSYS
    assert frames_call(L, m.tensor_spec("float32"), [f], src=0x1002) == EINVAL
    assert frames_call(L, ok, [f], src=0x1001, src_bytes=need - 1) == EINVAL


def _patterns(dtype):
    """all 65 536 bit patterns of a 16-bit element type that are not NaN, and the same values as a torch tensor"""
    u = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    t = torch.from_numpy(u.view(np.int16)).view(torch.float16 if dtype == "float16" else torch.bfloat16)
    keep = ~torch.isnan(t).numpy()
    return u[keep], t[torch.from_numpy(keep)]


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%g_%g" % p)
def test_model_value_chain_agrees_with_torch(pair, dtype):
    scale, bias = pair
    u, t = _patterns(dtype)
    assert len(u) == (65536 - 2046 if dtype == "float16" else 65536 - 254)
    assert np.array_equal(tim.element_values(u, dtype), t.float().numpy())
    x = t.float() * torch.tensor(scale, dtype=torch.float32) + torch.tensor(bias, dtype=torch.float32)
    for bits in BITS:
        want = torch.round(x).clamp(0, (1 << bits) - 1).numpy().astype(np.int64)
        got = tim.samples(tim.element_values(u, dtype), scale, bias, bits)
        assert np.array_equal(got, want), (bits, np.flatnonzero(got != want)[:4])


def test_model_at_the_corners():
    f32 = np.float32
    for bits in BITS:
        peak = (1 << bits) - 1
        special = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, 1e-45, -1e-45, 1.1754942e-38, 1e30, -1e30], f32)
        assert tim.samples(special, 1.0, 0.0, bits).tolist() == [0, 0, peak, 0, 0, 0, 0, 0, 0, 0, peak, 0]
        # ties at k + 0.5 go to the even neighbour, from both sides of it
        k = np.arange(0, min(peak, 64), dtype=f32)
        got = tim.samples(k + f32(0.5), 1.0, 0.0, bits)
        assert np.array_equal(got, np.minimum((k + (k.astype(np.int64) & 1)).astype(np.int64), peak))
        # at the peak: peak - 0.5 ties to the even one of peak - 1 and peak (peak is odd: peak - 1); peak + 0.5 saturates
        near = np.array([peak - 0.5, np.nextafter(f32(peak - 0.5), f32(0)), np.nextafter(f32(peak - 0.5), f32(1e9)), peak, peak + 0.5, peak + 1], f32)
        assert tim.samples(near, 1.0, 0.0, bits).tolist() == [peak - 1, peak - 1, peak, peak, peak, peak]
        # the same through a scale and a bias: (e * 2 - 1) at e = 0.75 is 0.5, a tie to 0; at 1.25 it is 1.5, a tie to 2
        assert tim.samples(np.array([0.75, 1.25, 0.5, 0.25], f32), 2.0, -1.0, bits).tolist() == [0, min(2, peak), 0, 0]
    # subnormal elements of all three types are values, not zeros: scaled up they give their sample
    assert tim.samples(tim.element_values(np.array([0x0001, 0x03FF], np.uint16), "float16"), 2.0 ** 24, 0.0, 16).tolist() == [1, 1023]
    assert tim.samples(tim.element_values(np.array([0x0001, 0x007F], np.uint16), "bfloat16"), 2.0 ** 126, 0.0, 16).tolist() == [0, 1]
    assert tim.samples(tim.element_values(np.array([0x0040], np.uint16), "bfloat16"), 2.0 ** 127, 0.0, 16).tolist() == [1]
    assert tim.samples(tim.element_values(np.array([0x00000001, 0x007FFFFF], np.uint32), "float32"), 2.0 ** 127, 0.0, 16).tolist() == [0, 2]
    # NaN and -0 as bit patterns of every type
    for dtype, pats in (("float16", [0x7E00, 0xFE00, 0x7C01, 0x8000]), ("bfloat16", [0x7FC0, 0xFFC0, 0x7F81, 0x8000]),
                        ("float32", [0x7FC00000, 0xFFC00000, 0x7F800001, 0x80000000])):
        a = np.array(pats, tm.BITS_DTYPE[dtype])
        assert tim.samples(tim.element_values(a, dtype), 1.0, 0.0, 8).tolist() == [0, 0, 0, 0]
        assert tim.samples(tim.element_values(a, dtype), 1.0, 3.0, 8).tolist() == [0, 0, 0, 3]


SIZES = [(5, 3), (9, 5), (1, 1), (4, 4)]


def _exact(dtype, bits):
    """integers up to 2^bits - 1 are exact in the element type"""
    return dtype == "float32" or (dtype == "float16" and bits <= 11) or (dtype == "bfloat16" and bits <= 8)


def random_planes(fmt, w, h, bits, rng):
    """planes as the decoder writes them: samples of `bits` bits shifted to their place, every other bit zero"""
    nbytes = cm.LAYOUTS[fmt][5]
    return [(rng.integers(0, 1 << bits, size=s, dtype=np.int64) << cm.shift(fmt, bits)).astype(np.uint8 if nbytes == 1 else np.uint16)
            for s in cm.plane_shapes(fmt, w, h)]


@pytest.mark.parametrize("fmt", FAMILIES)
def test_model_is_the_right_inverse_of_tensor_model(fmt):
    depth = cm.LAYOUTS[fmt][4]
    rng = np.random.default_rng(FAMILIES.index(fmt))
    tried = 0
    for w, h in SIZES:
        for bits in sorted({depth, max(depth - 3, 1), 1}):
            planes = random_planes(fmt, w, h, bits, rng)
            for dtype in tm.DTYPES:
                if not _exact(dtype, bits):
                    continue
                for layout in ("NCHW", "NHWC"):
                    img = tm.image(planes, fmt, bits, dtype, layout)
                    back = tim.frame(img, fmt, bits, dtype, layout)
                    assert len(back) == len(planes)
                    for a, b in zip(back, planes):
                        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (fmt, w, h, bits, dtype, layout)
                    tried += 1
    assert tried >= 2 * len(SIZES)


@pytest.mark.parametrize("fmt,w,h", [("yuv420p", 5, 3), ("yuv422p", 9, 5), ("yuv411p", 9, 5), ("yuv410p", 5, 3), ("yuv410p", 9, 5),
                                     ("yuva420p", 5, 3), ("yuv422p10le", 5, 3)])
def test_model_takes_the_top_left_element_of_a_footprint(fmt, w, h):
    nc, _, cw, ch, depth, _ = cm.LAYOUTS[fmt]
    rng = np.random.default_rng(w * 100 + h)
    vals = rng.integers(0, 1 << depth, size=(nc, h, w)).astype(np.float32)
    planes = tim.frame(vals.view(np.uint32), fmt, depth, "float32")
    assert [p.shape for p in planes] == [tuple(s) for s in cm.plane_shapes(fmt, w, h)]
    for c in range(nc):
        sw, sh = (cw, ch) if c in (1, 2) else (0, 0)
        for y in range(planes[c].shape[0]):
            for x in range(planes[c].shape[1]):
                assert planes[c][y, x] == vals[c, y << sh, x << sw]
    nhwc = tim.frame(np.ascontiguousarray(vals.transpose(1, 2, 0)).view(np.uint32), fmt, depth, "float32", "NHWC")
    assert all(np.array_equal(a, b) for a, b in zip(nhwc, planes))


@pytest.mark.parametrize("fmt", ["rgb48le", "gray16le", "xyz12le", "yuv422p10le", "rgb24", "ya8"])
def test_model_frames_have_no_other_bits_and_no_padding(fmt):
    nc, planar, _, _, depth, nbytes = cm.LAYOUTS[fmt]
    rng = np.random.default_rng(7)
    for bits in sorted({depth, depth - 1, 1}):
        t = rng.uniform(-4, (1 << bits) + 4, size=(2, nc, 3, 5)).astype(np.float32)
        t[:, :, 0, 0], t[:, :, 0, 1] = 1e9, -5.0
        for planes in tim.frames(t.view(np.uint32), fmt, bits, "float32"):
            assert [p.shape for p in planes] == [tuple(s) for s in cm.plane_shapes(fmt, 5, 3)]      # tight rows: no padding
            sh = cm.shift(fmt, bits)
            for p in planes:
                assert p.dtype == (np.uint8 if nbytes == 1 else np.uint16)
                assert ((p.astype(np.int64) & ~(((1 << bits) - 1) << sh)) == 0).all()               # every other bit is zero
            comps = cm.components(planes, fmt, bits)
            assert max(int(c.max()) for c in comps) == (1 << bits) - 1 and min(int(c.min()) for c in comps) == 0
