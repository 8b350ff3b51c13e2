"""Frames as tensors without a device: the symbols and the spec struct, htj2k_tensor_image_size, every refusal of
htj2k_frames_to_tensor with a NULL context, and the numpy model (tensor_model) against torch on the CPU and np.repeat."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cmp_model as cm
import ffmpeg_ht_amd as m
import tensor_model as tm

EINVAL, ENOSYS, PATCHWELCOME = -22, -38, -0x45574150
FAMILIES = ["gray", "gray16le", "ya8", "ya16le", "rgb24", "rgb48le", "rgba", "rgba64le", "yuv444p", "yuv444p16le", "yuv422p",
            "yuv422p10le", "yuv420p", "yuv420p16le", "yuva420p", "yuv411p", "yuv410p", "xyz12le"]
# (scale, bias): 8- and 10-bit normalisation, fp16 subnormals, fp16 infinities of both signs, ImageNet's red channel,
# binary32 subnormals, ties between fp16 and bf16 neighbours at 16 bits, results of exactly -0 and +0
PAIRS = [(1 / 255, 0.0), (1 / 1023, -0.5), (2.0 ** -20, 0.0), (3.0, -7.25), (-3.0, -7.25), (1 / (255 * 0.229), -0.485 / 0.229),
         (2.0 ** -134, 0.0), (2.0 ** -12, 0.0), (-1.0, -0.0), (-1.0, 0.0)]


@pytest.fixture(scope="module")
def L():
    return m.load_library()


def frame(fmt, w, h, ls=None, data=0x1000):
    """a frame whose planes are never read: refusals come before the context, and a NULL context ends the call"""
    fr = m.Frame()
    nc, planar, _, _, _, b = cm.LAYOUTS.get(fmt, (1, 0, 0, 0, 8, 1))
    shapes = cm.plane_shapes(fmt, w, h) if fmt in cm.LAYOUTS else [(h, w)]
    for p, (rows, cols) in enumerate(shapes):
        fr.data[p] = data
        fr.linesize[p] = cols * b if ls is None else ls
    fr.width, fr.height, fr.pix_fmt = w, h, m.PIX_NAMES.index(fmt)
    return fr


def call(L, frames, bits, spec, origins=None, dst=0x1000, dst_bytes=1 << 40, n=None, ctx=None):
    arr = (m.Frame * len(frames))(*frames) if frames is not None else None
    org = None if origins is None else (ctypes.c_int32 * len(origins))(*origins)
    return L.htj2k_frames_to_tensor(ctx, arr, 0, len(frames) if n is None else n, bits, None if spec is None else ctypes.byref(spec),
                                    org, ctypes.c_void_p(dst), ctypes.c_size_t(dst_bytes))


def test_symbols_and_spec_struct(L):
    for name in ("htj2k_tensor_spec_default", "htj2k_tensor_image_size", "htj2k_frames_to_tensor", "htj2k_job_to_tensor",
                 "htj2k_pipe_receive_tensor", "htj2k_tensor_last_route"):
        assert hasattr(L, name) and name in m.EXPORTS
    assert ctypes.sizeof(m.TensorSpec) == 48
    buf = (ctypes.c_uint8 * 64)(*([0xEE] * 64))
    L.htj2k_tensor_spec_default(buf)
    assert bytes(buf[48:]) == b"\xee" * 16                 # the C struct is 48 bytes as well
    s = m.TensorSpec.from_buffer_copy(bytes(buf[:48]))
    assert (s.dtype, s.layout, s.out_w, s.out_h) == (0, 0, 0, 0)
    assert list(s.scale) == [1.0] * 4 and list(s.bias) == [0.0] * 4
    L.htj2k_tensor_spec_default(None)                       # nothing to fill: no crash
    assert L.htj2k_tensor_last_route(None) == EINVAL


def test_spec_from_python():
    s = m.tensor_spec(torch.bfloat16, "NHWC", (7, 3), scale=0.5, bias=[1, 2])
    assert (s.dtype, s.layout, s.out_w, s.out_h) == (2, 1, 7, 3)
    assert list(s.scale) == [0.5] * 4 and list(s.bias) == [1.0, 2.0, 0.0, 0.0]
    assert m.tensor_spec(np.float32).dtype == 0 and m.tensor_spec("float16").dtype == 1
    with pytest.raises(ValueError):
        m.tensor_spec("float64")
    with pytest.raises(ValueError):
        m.tensor_spec("float16", "CHWN")


@pytest.mark.parametrize("fmt", FAMILIES)
def test_image_size(L, fmt):
    nc, depth = cm.LAYOUTS[fmt][0], cm.LAYOUTS[fmt][4]
    for dtype in tm.DTYPES:
        for layout in ("NCHW", "NHWC"):
            assert m.Decoder.tensor_image_size(fmt, 37, 11, depth, m.tensor_spec(dtype, layout)) == (nc * 37 * 11, nc * 37 * 11 * tm.ESIZE[dtype])
            assert m.Decoder.tensor_image_size(fmt, 37, 11, 1, m.tensor_spec(dtype, layout, (5, 3))) == (nc * 15, nc * 15 * tm.ESIZE[dtype])
    spec = m.tensor_spec("float16")
    e = ctypes.c_size_t(7)
    assert L.htj2k_tensor_image_size(m.PIX_NAMES.index(fmt), 4, 4, depth, ctypes.byref(spec), ctypes.byref(e), None) == 0
    assert e.value == nc * 16                              # either result may be left out
    assert L.htj2k_tensor_image_size(m.PIX_NAMES.index(fmt), 4, 4, depth, None, None, None) == EINVAL
    for bad in ((0, 4, depth, spec), (4, 0, depth, spec), (4, 4, 0, spec), (4, 4, depth + 1, spec),
                (4, 4, depth, m.tensor_spec("float16", size=(5, 4))), (4, 4, depth, m.tensor_spec("float16", size=(4, 5)))):
        assert L.htj2k_tensor_image_size(m.PIX_NAMES.index(fmt), bad[0], bad[1], bad[2], ctypes.byref(bad[3]), None, None) == EINVAL
    assert L.htj2k_tensor_image_size(m.PIX_NAMES.index("pal8"), 4, 4, 8, ctypes.byref(spec), None, None) == PATCHWELCOME
    assert L.htj2k_tensor_image_size(-1, 4, 4, 8, ctypes.byref(spec), None, None) == EINVAL
    assert L.htj2k_tensor_image_size(len(m.PIX_NAMES), 4, 4, 8, ctypes.byref(spec), None, None) == EINVAL


def _spec(**kw):
    s = m.tensor_spec("float16")
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _bad_float(field, k, v):
    s = m.tensor_spec("float16")
    getattr(s, field)[k] = v
    return s


def test_refusals_in_their_order_with_a_null_context(L):
    ok = m.tensor_spec("float16")
    f = frame("yuv420p", 20, 10)
    assert call(L, [f], 8, ok) == ENOSYS                    # valid arguments, no context
    assert call(L, [f, f], 8, m.tensor_spec("float32", "NHWC", (3, 3)), origins=[17, 7, 0, 0], dst_bytes=2 * 27 * 4) == ENOSYS
    pal = frame("pal8", 20, 10)
    # 1 and 2 come before the layout: a PAL8 frame does not get as far as its own answer
    assert call(L, None, 8, ok, n=1) == EINVAL
    assert call(L, [pal], 8, None) == EINVAL
    assert call(L, [pal], 8, ok, dst=0) == EINVAL
    assert call(L, [pal], 8, ok, n=0) == EINVAL and call(L, [pal], 8, ok, n=-3) == EINVAL
    # 3: the layout, before bits, dtype, layout, scale, bias and the window
    assert call(L, [pal], 99, _spec(dtype=7, layout=9, out_w=-1)) == PATCHWELCOME
    assert call(L, [pal], 8, _bad_float("scale", 0, math.nan)) == PATCHWELCOME
    for bad_fmt in (-1, len(m.PIX_NAMES), 1000):
        g = frame("gray", 20, 10)
        g.pix_fmt = bad_fmt
        assert call(L, [g], 8, ok) == EINVAL
    # 4
    assert call(L, [f], 0, ok) == EINVAL and call(L, [f], 9, ok) == EINVAL and call(L, [f], -1, ok) == EINVAL
    assert call(L, [frame("yuv422p10le", 20, 10)], 11, ok) == EINVAL and call(L, [frame("yuv422p10le", 20, 10)], 10, ok) == ENOSYS
    assert call(L, [frame("xyz12le", 20, 10)], 13, ok) == EINVAL and call(L, [frame("xyz12le", 20, 10)], 12, ok) == ENOSYS
    # 5
    for kw in (dict(dtype=-1), dict(dtype=3), dict(layout=-1), dict(layout=2)):
        assert call(L, [f], 8, _spec(**kw)) == EINVAL
    # 6: only the first C entries are read
    for field in ("scale", "bias"):
        for v in (math.nan, math.inf, -math.inf):
            for k in range(3):
                assert call(L, [f], 8, _bad_float(field, k, v)) == EINVAL
            assert call(L, [f], 8, _bad_float(field, 3, v)) == ENOSYS          # yuv420p has three components
            assert call(L, [frame("gray", 20, 10)], 8, _bad_float(field, 1, v)) == ENOSYS
    # 7
    for ow, oh in ((0, 1), (1, 0), (-1, -1), (-1, 4), (4, -1)):
        assert call(L, [f], 8, _spec(out_w=ow, out_h=oh)) == EINVAL
    # 8
    assert call(L, [f, frame("yuv422p", 20, 10)], 8, ok) == EINVAL
    assert call(L, [f, frame("yuv422p", 20, 10)], 8, _spec(out_w=2, out_h=2)) == EINVAL
    # 9: sizes may differ when a window is given, not without one
    assert call(L, [f, frame("yuv420p", 21, 10)], 8, ok) == EINVAL
    assert call(L, [f, frame("yuv420p", 20, 11)], 8, ok) == EINVAL
    assert call(L, [f, frame("yuv420p", 21, 11)], 8, _spec(out_w=20, out_h=10)) == ENOSYS
    assert call(L, [frame("yuv420p", 0, 10)], 8, ok) == EINVAL and call(L, [frame("yuv420p", 20, -1)], 8, ok) == EINVAL
    # 10
    for p in range(3):
        g = frame("yuv420p", 20, 10)
        g.data[p] = None
        assert call(L, [f, g], 8, ok) == EINVAL
    g = frame("gray", 20, 10)
    g.data[1] = None                                        # a plane the layout lacks is not asked for
    assert call(L, [g], 8, ok) == ENOSYS
    # 11
    for p, short in ((0, 19), (1, 9), (2, 9), (0, -20)):
        g = frame("yuv420p", 20, 10)
        g.linesize[p] = short
        assert call(L, [g], 8, ok) == EINVAL
    g = frame("yuv420p", 21, 11)                            # ceilinged chroma: 11 samples a row
    g.linesize[1] = 10
    assert call(L, [g], 8, ok) == EINVAL
    # 12
    w = _spec(out_w=4, out_h=4)
    assert call(L, [f], 8, w, origins=[-1, 0]) == EINVAL and call(L, [f], 8, w, origins=[0, -1]) == EINVAL
    assert call(L, [f, f], 8, w, origins=[0, 0, 0, -5]) == EINVAL
    # 13
    assert call(L, [f], 8, w, origins=[16, 6]) == ENOSYS
    assert call(L, [f], 8, w, origins=[17, 6]) == EINVAL and call(L, [f], 8, w, origins=[16, 7]) == EINVAL
    assert call(L, [f], 8, _spec(out_w=21, out_h=10)) == EINVAL and call(L, [f], 8, _spec(out_w=20, out_h=11)) == EINVAL
    assert call(L, [f], 8, ok, origins=[1, 0]) == EINVAL    # 0 x 0 is the whole frame: only the origin 0, 0 fits
    assert call(L, [f], 8, w, origins=[2 ** 31 - 1, 0]) == EINVAL
    # 14
    need = 3 * 20 * 10 * 2
    assert call(L, [f], 8, ok, dst_bytes=need) == ENOSYS and call(L, [f], 8, ok, dst_bytes=need - 1) == EINVAL
    assert call(L, [f, f], 8, ok, dst_bytes=2 * need - 1) == EINVAL and call(L, [f], 8, ok, dst_bytes=0) == EINVAL
    # 15: the element's own alignment, nothing more
    assert call(L, [f], 8, ok, dst=0x1001) == EINVAL and call(L, [f], 8, ok, dst=0x1002) == ENOSYS
    f32 = m.tensor_spec("float32")
    assert call(L, [f], 8, f32, dst=0x1002) == EINVAL and call(L, [f], 8, f32, dst=0x1004) == ENOSYS
    assert call(L, [f], 8, m.tensor_spec("bfloat16"), dst=0x1001) == EINVAL
    # 14 before 15
    assert call(L, [f], 8, ok, dst=0x1001, dst_bytes=need - 1) == EINVAL


def test_job_and_pipe_calls_refuse_missing_arguments(L):
    ok = m.tensor_spec("float16")
    assert L.htj2k_job_to_tensor(None, None, 0, ctypes.byref(ok), None, ctypes.c_void_p(0x1000), ctypes.c_size_t(1 << 20), None) == EINVAL
    assert L.htj2k_pipe_receive_tensor(None, None, 0, ctypes.byref(ok), None, ctypes.c_void_p(0x1000), ctypes.c_size_t(1 << 20)) == EINVAL


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%g_%g" % p)
def test_model_conversions_agree_with_torch(pair):
    scale, bias = pair
    s = np.arange(65536, dtype=np.int64)
    t = torch.from_numpy(s.astype(np.float32)) * torch.tensor(scale, dtype=torch.float32)
    t = t + torch.tensor(bias, dtype=torch.float32)
    assert np.array_equal(tm.value_bits(s, scale, bias, "float32"), t.numpy().view(np.uint32))
    assert np.array_equal(tm.value_bits(s, scale, bias, "float16"), t.to(torch.float16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(tm.value_bits(s, scale, bias, "bfloat16"), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_pairs_reach_the_corners_they_are_there_for():
    s = np.arange(65536, dtype=np.int64)
    h = tm.value_bits(s, 2.0 ** -20, 0.0, "float16")
    assert ((h & 0x7C00) == 0).sum() > 60 and (h[1:64] != 0).all()                   # fp16 subnormals, kept
    assert (tm.value_bits(s, 3.0, -7.25, "float16") == 0x7C00).any() and (tm.value_bits(s, -3.0, -7.25, "float16") == 0xFC00).any()
    f = tm.value_bits(s, 2.0 ** -134, 0.0, "float32")
    assert ((f[1:] & 0x7F800000) == 0).any() and (f[1:] != 0).all()                  # binary32 subnormals, kept
    t = tm.value_bits(s, 2.0 ** -12, 0.0, "float32")
    assert ((t & 0x1FFF) == 0x1000).any() and ((t & 0xFFFF) == 0x8000).any()         # exact ties for fp16 and for bf16
    assert tm.value_bits(s[:1], -1.0, -0.0, "float32")[0] == 0x80000000 and tm.value_bits(s[:1], -1.0, 0.0, "float32")[0] == 0
    assert tm.value_bits(s[:1], -1.0, -0.0, "float16")[0] == 0x8000 and tm.value_bits(s[:1], -1.0, -0.0, "bfloat16")[0] == 0x8000


@pytest.mark.parametrize("fmt,w,h", [("yuv420p", 7, 5), ("yuv420p", 8, 6), ("yuv422p", 9, 3), ("yuv411p", 13, 3), ("yuv411p", 9, 1),
                                     ("yuv410p", 11, 7), ("yuv410p", 5, 9), ("yuva420p", 3, 3), ("yuv422p10le", 5, 2)])
def test_model_replication_is_np_repeat(fmt, w, h):
    rng = np.random.default_rng(w * 100 + h)
    nc, _, cw, ch, depth, b = cm.LAYOUTS[fmt]
    planes = [rng.integers(0, 1 << depth, size=s, dtype=np.uint16).astype(np.uint8 if b == 1 else np.uint16) for s in cm.plane_shapes(fmt, w, h)]
    got = tm.image(planes, fmt, depth, "float32").view(np.float32)
    assert got.shape == (nc, h, w)
    for c in range(nc):
        want = planes[c].astype(np.float32)
        if c in (1, 2):
            want = np.repeat(np.repeat(want, 1 << ch, axis=0), 1 << cw, axis=1)[:h, :w]
        assert np.array_equal(got[c], want), c
    nhwc = tm.image(planes, fmt, depth, "float32", "NHWC")
    assert np.array_equal(nhwc.transpose(2, 0, 1), got.view(np.uint32))
    win = tm.image(planes, fmt, depth, "float32", size=(w - 1, h - 1) if h > 1 else (w - 1, 1), origin=(1, 1 if h > 1 else 0))
    assert np.array_equal(win, got.view(np.uint32)[:, (1 if h > 1 else 0):, 1:])
