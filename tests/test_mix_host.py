"""The tensor calls with a colour matrix, without a device: the symbols and the mix struct, htj2k_tensor_image_size_mix,
the refusals of the _mix entry points with a NULL context (and, with mix = NULL, their agreement with the plain calls),
htj2k_tensor_mix_ycbcr against its float64 restatement, and the numpy model (mix_model) against torch on the CPU."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import cmp_model as cm
import ffmpeg_ht_amd as m
import mix_model as mm
import tensor_model as tm
from test_tensor_host import frame

EINVAL, ENOSYS, PATCHWELCOME = -22, -38, -0x45574150
NEW = ["htj2k_tensor_mix_ycbcr", "htj2k_tensor_image_size_mix", "htj2k_frames_to_tensor_mix", "htj2k_job_to_tensor_mix",
       "htj2k_pipe_receive_tensor_mix", "htj2k_frames_to_tensor_resized_mix", "htj2k_job_to_tensor_resized_mix",
       "htj2k_pipe_receive_tensor_resized_mix"]


@pytest.fixture(scope="module")
def L():
    return m.load_library()


def _org(origins):
    return None if origins is None else (ctypes.c_int32 * len(origins))(*origins)


def call_mix(L, frames, bits, spec, mix, origins=None, dst=0x1000, dst_bytes=1 << 40, n=None):
    arr = (m.Frame * len(frames))(*frames) if frames is not None else None
    return L.htj2k_frames_to_tensor_mix(None, arr, 0, len(frames) if n is None else n, bits, None if spec is None else ctypes.byref(spec),
                                        None if mix is None else ctypes.byref(mix), _org(origins), ctypes.c_void_p(dst),
                                        ctypes.c_size_t(dst_bytes))


def call_plain(L, frames, bits, spec, origins=None, dst=0x1000, dst_bytes=1 << 40, n=None):
    arr = (m.Frame * len(frames))(*frames) if frames is not None else None
    return L.htj2k_frames_to_tensor(None, arr, 0, len(frames) if n is None else n, bits, None if spec is None else ctypes.byref(spec),
                                    _org(origins), ctypes.c_void_p(dst), ctypes.c_size_t(dst_bytes))


def call_resized(L, frames, bits, spec, mix, windows=None, filt=2, dst=0x1000, dst_bytes=1 << 40, n=None, plain=False):
    arr = (m.Frame * len(frames))(*frames) if frames is not None else None
    n = len(frames) if n is None else n
    sp = None if spec is None else ctypes.byref(spec)
    if plain:
        return L.htj2k_frames_to_tensor_resized(None, arr, 0, n, bits, sp, _org(windows), filt, ctypes.c_void_p(dst), ctypes.c_size_t(dst_bytes))
    return L.htj2k_frames_to_tensor_resized_mix(None, arr, 0, n, bits, sp, None if mix is None else ctypes.byref(mix), _org(windows), filt,
                                                ctypes.c_void_p(dst), ctypes.c_size_t(dst_bytes))


def eye(k, c=4):
    return m.tensor_mix(np.eye(k, c, dtype=np.float32))


def test_symbols_and_mix_struct(L):
    for name in NEW:
        assert hasattr(L, name) and name in m.EXPORTS, name
    assert ctypes.sizeof(m.TensorMix) == 84
    buf = (ctypes.c_uint8 * 96)(*([0xEE] * 96))
    assert L.htj2k_tensor_mix_ycbcr(buf, 709, 0, 10, 1, None, None) == 0
    assert bytes(buf[84:]) == b"\xee" * 12                   # the C struct is 84 bytes as well
    got = m.TensorMix.from_buffer_copy(bytes(buf[:84]))
    assert got.nout == 4 and got.m[3][3] == np.float32(1 / 1023) and got.m[0][1] == 0.0
    mix = m.tensor_mix([[0, 0, 1], [0, 1, 0], [1, 0, 0]], [0.5, -0.0, 2])
    assert mix.nout == 3 and [list(r) for r in mix.m][:3] == [[0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 0, 0]]
    assert list(mix.b) == [0.5, 0.0, 2.0, 0.0] and math.copysign(1, mix.b[1]) == -1
    assert m.tensor_mix([[1, 2, 3, 4]]).nout == 1
    for bad in ([1, 2, 3], np.zeros((5, 3)), np.zeros((3, 5)), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            m.tensor_mix(bad)
    with pytest.raises(ValueError):
        m.tensor_mix(np.eye(3), [0, 0])


@pytest.mark.parametrize("fmt", ["gray", "ya8", "rgb24", "rgba64le", "yuv420p", "yuv422p10le", "yuva444p10le", "yuv410p", "xyz12le"])
def test_image_size(L, fmt):
    nc, depth = cm.LAYOUTS[fmt][0], cm.LAYOUTS[fmt][4]
    for dtype, layout in itertools.product(tm.DTYPES, ("NCHW", "NHWC")):
        spec = m.tensor_spec(dtype, layout)
        for k in range(1, 5):
            assert m.Decoder.tensor_image_size(fmt, 37, 11, depth, spec, eye(k)) == (k * 37 * 11, k * 37 * 11 * tm.ESIZE[dtype])
            win = m.tensor_spec(dtype, layout, (5, 3))
            assert m.Decoder.tensor_image_size(fmt, 37, 11, depth, win, eye(k)) == (k * 15, k * 15 * tm.ESIZE[dtype])
        assert m.Decoder.tensor_image_size(fmt, 37, 11, depth, spec, None) == m.Decoder.tensor_image_size(fmt, 37, 11, depth, spec)
    spec = m.tensor_spec("float16")
    e, b = ctypes.c_size_t(7), ctypes.c_size_t(7)
    pf = m.PIX_NAMES.index(fmt)
    assert L.htj2k_tensor_image_size_mix(pf, 4, 4, depth, ctypes.byref(spec), None, ctypes.byref(e), ctypes.byref(b)) == 0
    assert (e.value, b.value) == (nc * 16, nc * 32)
    assert L.htj2k_tensor_image_size_mix(pf, 4, 4, depth, None, ctypes.byref(eye(3)), None, None) == EINVAL
    assert L.htj2k_tensor_image_size_mix(pf, 4, 4, depth + 1, ctypes.byref(spec), ctypes.byref(eye(3)), None, None) == EINVAL
    bad = eye(3)
    bad.nout = 5
    assert L.htj2k_tensor_image_size_mix(pf, 4, 4, depth, ctypes.byref(spec), ctypes.byref(bad), None, None) == EINVAL
    assert L.htj2k_tensor_image_size_mix(m.PIX_NAMES.index("pal8"), 4, 4, 8, ctypes.byref(spec), ctypes.byref(bad), None, None) == PATCHWELCOME


def _mix_with(k=3, **kw):
    mix = eye(k)
    for name, v in kw.items():
        if name == "nout":
            mix.nout = v
        elif name[0] == "m":
            mix.m[int(name[1])][int(name[2])] = v
        else:
            mix.b[int(name[1])] = v
    return mix


def _spec(**kw):
    s = m.tensor_spec("float16")
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_refusals_in_their_order_with_a_null_context(L):
    ok = m.tensor_spec("float16")
    f = frame("yuv420p", 20, 10)                             # C = 3
    need = lambda k: k * 20 * 10 * 2
    assert call_mix(L, [f], 8, ok, eye(3)) == ENOSYS         # valid arguments, no context
    for k in range(1, 5):
        assert call_mix(L, [f], 8, ok, eye(k), dst_bytes=need(k)) == ENOSYS
        assert call_mix(L, [f], 8, ok, eye(k), dst_bytes=need(k) - 1) == EINVAL
    # K > C with a destination sized for C
    assert call_mix(L, [f], 8, ok, eye(4), dst_bytes=need(3)) == EINVAL
    g = frame("gray", 20, 10)
    assert call_mix(L, [g], 8, ok, eye(3), dst_bytes=1 * 20 * 10 * 2) == EINVAL and call_mix(L, [g], 8, ok, eye(3), dst_bytes=3 * 20 * 10 * 2) == ENOSYS
    # the mix is checked where scale and bias are: behind the layout, bits, dtype and layout, in front of the window
    pal = frame("pal8", 20, 10)
    for bad in (_mix_with(nout=0), _mix_with(nout=5), _mix_with(nout=-1), _mix_with(m00=math.nan), _mix_with(b2=math.inf)):
        assert call_mix(L, [f], 8, ok, bad) == EINVAL
        assert call_mix(L, [pal], 8, ok, bad) == PATCHWELCOME
        assert call_mix(L, [pal], 8, ok, bad, n=0) == EINVAL
        assert call_mix(L, [f], 8, ok, bad, dst=0) == EINVAL
    # nout first: an entry that a smaller K would not read is not looked at once K is refused; entries that are not read
    for v in (math.nan, math.inf, -math.inf):
        for k, c in itertools.product(range(3), range(3)):
            assert call_mix(L, [f], 8, ok, _mix_with(**{"m%d%d" % (k, c): v})) == EINVAL
        for k in range(3):
            assert call_mix(L, [f], 8, ok, _mix_with(**{"b%d" % k: v})) == EINVAL
            assert call_mix(L, [f], 8, ok, _mix_with(**{"m%d3" % k: v})) == ENOSYS            # column C: yuv420p has three components
            assert call_mix(L, [f], 8, ok, _mix_with(**{"m3%d" % k: v})) == ENOSYS            # row K
        assert call_mix(L, [f], 8, ok, _mix_with(b3=v)) == ENOSYS
        assert call_mix(L, [g], 8, ok, _mix_with(m01=v, m12=v, m23=v)) == ENOSYS              # gray reads column 0 only
        assert call_mix(L, [f], 8, ok, _mix_with(2, m20=v, b2=v)) == ENOSYS                   # K = 2 reads rows 0 and 1
    # with a mix scale and bias are not read
    s = m.tensor_spec("float16")
    s.scale[0], s.bias[1] = math.nan, math.inf
    assert call_mix(L, [f], 8, s, eye(3)) == ENOSYS and call_plain(L, [f], 8, s) == EINVAL
    # everything else as without a mix, in its order: a bad mix hides behind bits, dtype and layout and in front of the rest
    bad = _mix_with(nout=9)
    assert call_mix(L, [f], 9, ok, bad) == EINVAL and call_mix(L, [f], 8, _spec(dtype=3), bad) == EINVAL
    w = _spec(out_w=4, out_h=4)
    assert call_mix(L, [f], 8, w, eye(2), origins=[17, 6]) == EINVAL and call_mix(L, [f], 8, w, eye(2), origins=[16, 6]) == ENOSYS
    assert call_mix(L, [f], 8, _spec(out_w=0, out_h=3), eye(2)) == EINVAL
    assert call_mix(L, [f, frame("yuv422p", 20, 10)], 8, ok, eye(2)) == EINVAL
    assert call_mix(L, [f], 8, ok, eye(1), dst=0x1001) == EINVAL
    assert call_mix(L, [f], 8, m.tensor_spec("float32"), eye(1), dst=0x1002) == EINVAL
    # the resized calls: the same place, behind the filter
    r = m.tensor_spec("float16", "NCHW", (7, 5))
    assert call_resized(L, [f], 8, r, eye(4)) == ENOSYS
    assert call_resized(L, [f], 8, r, eye(4), dst_bytes=4 * 35 * 2 - 1) == EINVAL
    assert call_resized(L, [f], 8, r, _mix_with(nout=0)) == EINVAL
    assert call_resized(L, [f], 8, r, _mix_with(m11=math.nan), filt=9) == EINVAL
    assert call_resized(L, [f], 8, r, _mix_with(m13=math.nan)) == ENOSYS
    assert call_resized(L, [f], 8, r, eye(3), windows=[0, 0, 21, 10]) == EINVAL


def test_mix_null_refuses_as_the_plain_twin(L):
    ok = m.tensor_spec("float16")
    f = frame("yuv420p", 20, 10)
    pal = frame("pal8", 20, 10)
    nan = m.tensor_spec("float16")
    nan.scale[2] = math.nan
    short = frame("yuv420p", 20, 10)
    short.linesize[1] = 9
    hole = frame("yuv420p", 20, 10)
    hole.data[2] = None
    w = _spec(out_w=4, out_h=4)
    need = 3 * 20 * 10 * 2
    cases = [dict(frames=None, bits=8, spec=ok, n=1), dict(frames=[pal], bits=8, spec=None), dict(frames=[pal], bits=8, spec=ok, dst=0),
             dict(frames=[pal], bits=8, spec=ok, n=0), dict(frames=[pal], bits=99, spec=_spec(dtype=7)), dict(frames=[f], bits=0, spec=ok),
             dict(frames=[f], bits=9, spec=ok), dict(frames=[f], bits=8, spec=_spec(dtype=3)), dict(frames=[f], bits=8, spec=_spec(layout=2)),
             dict(frames=[f], bits=8, spec=nan), dict(frames=[f], bits=8, spec=_spec(out_w=0, out_h=1)),
             dict(frames=[f, frame("yuv422p", 20, 10)], bits=8, spec=ok), dict(frames=[f, frame("yuv420p", 21, 10)], bits=8, spec=ok),
             dict(frames=[hole], bits=8, spec=ok), dict(frames=[short], bits=8, spec=ok), dict(frames=[f], bits=8, spec=w, origins=[-1, 0]),
             dict(frames=[f], bits=8, spec=w, origins=[17, 6]), dict(frames=[f], bits=8, spec=w, origins=[16, 6]),
             dict(frames=[f], bits=8, spec=ok, dst_bytes=need - 1), dict(frames=[f], bits=8, spec=ok, dst_bytes=need),
             dict(frames=[f], bits=8, spec=ok, dst=0x1001), dict(frames=[f], bits=8, spec=ok)]
    answers = set()
    for kw in cases:
        plain = call_plain(L, **kw)
        assert call_mix(L, mix=None, **kw) == plain, kw
        answers.add(plain)
    assert answers == {EINVAL, ENOSYS, PATCHWELCOME}
    r = m.tensor_spec("float16", "NCHW", (7, 5))
    rcases = [dict(frames=[f], bits=8, spec=r), dict(frames=[f], bits=8, spec=r, filt=3), dict(frames=[f], bits=8, spec=ok),
              dict(frames=[f], bits=8, spec=r, windows=[0, 0, 0, 4]), dict(frames=[f], bits=8, spec=r, windows=[-1, 0, 4, 4]),
              dict(frames=[f], bits=8, spec=r, windows=[17, 0, 4, 4]), dict(frames=[pal], bits=8, spec=r), dict(frames=[f], bits=8, spec=nan),
              dict(frames=[f], bits=8, spec=m.tensor_spec("float16", "NCHW", (40000, 5))),
              dict(frames=[f], bits=8, spec=r, dst_bytes=3 * 35 * 2 - 1), dict(frames=[f], bits=8, spec=r, dst=0x1001)]
    for kw in rcases:
        assert call_resized(L, mix=None, **kw) == call_resized(L, mix=None, plain=True, **kw), kw
    # jobs and pipes: their own refusal without a device is the missing argument
    v, z = ctypes.c_void_p(0x1000), ctypes.c_size_t(1 << 20)
    assert L.htj2k_job_to_tensor_mix(None, None, 0, ctypes.byref(ok), None, None, v, z, None) \
        == L.htj2k_job_to_tensor(None, None, 0, ctypes.byref(ok), None, v, z, None) == EINVAL
    assert L.htj2k_job_to_tensor_resized_mix(None, None, 0, ctypes.byref(r), None, None, 2, v, z, None) \
        == L.htj2k_job_to_tensor_resized(None, None, 0, ctypes.byref(r), None, 2, v, z, None) == EINVAL
    assert L.htj2k_pipe_receive_tensor_mix(None, None, 0, ctypes.byref(ok), None, None, v, z) \
        == L.htj2k_pipe_receive_tensor(None, None, 0, ctypes.byref(ok), None, v, z) == EINVAL
    assert L.htj2k_pipe_receive_tensor_resized_mix(None, None, 0, ctypes.byref(r), None, None, 2, v, z) \
        == L.htj2k_pipe_receive_tensor_resized(None, None, 0, ctypes.byref(r), None, 2, v, z) == EINVAL
    assert L.htj2k_job_to_tensor_mix(None, None, 0, ctypes.byref(ok), ctypes.byref(eye(3)), None, v, z, None) == EINVAL


def ulps(a, b):
    """distance of two float32 arrays in units of the last place; -0 and +0 are the same place"""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


GAINS = [(None, None), ([1 / 0.229, 1 / 0.224, 1 / 0.225], [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225])]


@pytest.mark.parametrize("standard", [601, 709, 2020])
@pytest.mark.parametrize("full", [0, 1])
def test_ycbcr_helper_against_the_float64_model(standard, full):
    for bits, alpha, (gain, offset) in itertools.product((8, 10, 12, 16), (0, 1), GAINS):
        mix = m.Decoder.ycbcr_mix(standard, bits, bool(full), bool(alpha), gain, offset)
        nout, got_m, got_b = mm.unpack(mix)
        want_m, want_b = mm.ycbcr(standard, full, bits, alpha, gain, offset)
        assert nout == (4 if alpha else 3)
        assert ulps(got_m[:nout], want_m.astype(np.float32)).max() <= 1, (standard, full, bits, alpha)
        assert ulps(got_b[:nout], want_b.astype(np.float32)).max() <= 1, (standard, full, bits, alpha)
        assert (got_m[nout:] == 0).all() and (got_b[nout:] == 0).all()
        if gain is None:
            # black and white through the model: within 2^-20 of 0 and 1 in all three channels
            q, mid, peak = 1 << (bits - 8), 1 << (bits - 1), (1 << bits) - 1
            black, white = ((0, mid, mid), (peak, mid, mid)) if full else ((16 * q, mid, mid), (235 * q, mid, mid))
            comps = 4 if alpha else 3
            for px, want in ((black, 0.0), (white, 1.0)):
                f = [np.array([v], np.float32) for v in (px + (peak,))[:comps]]
                t = mm.mix_values(f, got_m, got_b, 3)
                assert all(abs(float(v[0]) - want) <= 2.0 ** -20 for v in t), (standard, full, bits, px, [float(v[0]) for v in t])
            if alpha:
                f = [np.array([v], np.float32) for v in (0, 0, 0, peak)]
                assert abs(float(mm.mix_values(f, got_m, got_b, 4)[3][0]) - 1.0) <= 2.0 ** -20


def test_ycbcr_helper_refusals(L):
    mix = m.TensorMix()
    ok3 = (ctypes.c_float * 3)(1, 1, 1)
    assert L.htj2k_tensor_mix_ycbcr(None, 709, 0, 8, 0, None, None) == EINVAL
    for standard in (0, 600, 2021, -709):
        assert L.htj2k_tensor_mix_ycbcr(ctypes.byref(mix), standard, 0, 8, 0, None, None) == EINVAL
    for bits in (7, 17, 0, -8):
        assert L.htj2k_tensor_mix_ycbcr(ctypes.byref(mix), 709, 0, bits, 0, None, None) == EINVAL
    for v in (math.nan, math.inf, -math.inf):
        for k in range(3):
            bad = (ctypes.c_float * 3)(1, 1, 1)
            bad[k] = v
            assert L.htj2k_tensor_mix_ycbcr(ctypes.byref(mix), 709, 0, 8, 0, bad, None) == EINVAL
            assert L.htj2k_tensor_mix_ycbcr(ctypes.byref(mix), 709, 0, 8, 0, None, bad) == EINVAL
    assert L.htj2k_tensor_mix_ycbcr(ctypes.byref(mix), 2020, 1, 16, 1, ok3, ok3) == 0 and mix.nout == 4
    with pytest.raises(m.Htj2kError) as e:
        m.Decoder.ycbcr_mix(1, 8)
    assert e.value.code == EINVAL


def torch_chain(f, mmat, b, nout):
    """the same chain in torch on the CPU: separate mul and add calls on float32"""
    out = []
    for k in range(nout):
        a = torch.mul(f[0], torch.tensor(mmat[k][0], dtype=torch.float32))
        for c in range(1, len(f)):
            a = torch.add(a, torch.mul(f[c], torch.tensor(mmat[k][c], dtype=torch.float32)))
        out.append(torch.add(a, torch.tensor(b[k], dtype=torch.float32)))
    return out


CORNERS = (np.array([[0.0, -0.0, -1.5, 3.0e38], [-0.0, -0.0, -0.0, 0.0], [2.0 ** -140, 65504.0, -7.25, 1.0], [1 / 3, -1 / 3, 1e-30, 2.0 ** -12]],
                    np.float32), np.array([-0.0, 0.0, 1.0, -6.1e-5], np.float32))


@pytest.mark.parametrize("bits", [8, 10, 12, 16])
def test_model_mix_agrees_with_torch(bits):
    rng = np.random.default_rng(bits)
    s = rng.integers(0, 1 << bits, size=(4, 65536)).astype(np.float32)
    s[:, :4] = [[0, 0, 0, 0], [0, 1, 0, 1], [(1 << bits) - 1] * 4, [1, 0, 0, 0]]      # zeros in every position: signed zeros of the sums
    mixes = [mm.unpack(m.Decoder.ycbcr_mix(709, bits, False, True, *GAINS[1]))[1:], mm.unpack(m.Decoder.ycbcr_mix(601, bits, True))[1:], CORNERS]
    for mmat, b in mixes:
        for ncomp in (1, 3, 4):
            f = [s[c] for c in range(ncomp)]
            want = torch_chain([torch.from_numpy(v) for v in f], mmat, b, 4)
            got = mm.mix_values(f, mmat, b, 4)
            for k in range(4):
                assert torch.equal(torch.from_numpy(got[k]).view(torch.int32), want[k].view(torch.int32)), (bits, ncomp, k)
                assert np.array_equal(mm.stored(got[k], "float16"), want[k].to(torch.float16).view(torch.int16).numpy().view(np.uint16))
                assert np.array_equal(mm.stored(got[k], "bfloat16"), want[k].to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
                assert np.array_equal(mm.stored(got[k], "float32"), want[k].view(torch.int32).numpy().view(np.uint32))
    # the corner matrix reaches what it is there for: three -0 products and a -0 offset stay -0, one +0 term or a +0
    # offset makes +0, and the large weight overflows
    z, neg = [np.zeros(1, np.float32)] * 3, np.array([-0.0] * 4, np.float32)
    t = mm.mix_values(z, CORNERS[0], neg, 4)
    assert t[1].view(np.uint32)[0] == 0x80000000 and t[0].view(np.uint32)[0] == 0
    assert mm.mix_values(z, CORNERS[0], CORNERS[1], 4)[1].view(np.uint32)[0] == 0
    assert np.isinf(mm.mix_values([np.full(1, 255, np.float32)] * 4, *CORNERS, 4)[0][0])


@pytest.mark.parametrize("fmt,w,h", [("rgb24", 17, 3), ("rgba64le", 5, 2), ("gray", 9, 1), ("ya8", 7, 3), ("yuv420p", 7, 5), ("yuv422p10le", 9, 3),
                                     ("yuv411p", 13, 3), ("yuv410p", 11, 7), ("yuva420p", 3, 3), ("yuva444p10le", 6, 2), ("xyz12le", 5, 4)])
def test_model_identity_mix_is_tensor_model(fmt, w, h):
    rng = np.random.default_rng(w * 100 + h)
    nc, _, _, _, depth, b = cm.LAYOUTS[fmt]
    planes = [rng.integers(0, 1 << (8 * b), size=s, dtype=np.uint32).astype(np.uint8 if b == 1 else np.uint16) for s in cm.plane_shapes(fmt, w, h)]
    for dtype, layout in itertools.product(tm.DTYPES, ("NCHW", "NHWC")):
        want = tm.image(planes, fmt, depth, dtype, layout, None, (0, 0), 1.0, 0.0)
        assert np.array_equal(mm.image(planes, fmt, depth, mm.identity(nc), dtype, layout), want), (dtype, layout)
        assert np.array_equal(mm.image(planes, fmt, depth, m.tensor_mix(np.eye(nc)), dtype, layout), want)
    if w > 2 and h > 1:
        want = tm.image(planes, fmt, depth, "float32", "NCHW", (w - 2, h - 1), (1, 1), 1.0, 0.0)
        assert np.array_equal(mm.image(planes, fmt, depth, mm.identity(nc), "float32", "NCHW", (w - 2, h - 1), (1, 1)), want)
    # a permutation and a dropped channel are channels of the identity
    if nc >= 3:
        full = mm.image(planes, fmt, depth, mm.identity(nc), "float32")
        bgr = mm.image(planes, fmt, depth, (np.eye(nc, dtype=np.float32)[[2, 1, 0]], None), "float32")
        assert np.array_equal(bgr, full[[2, 1, 0]])
