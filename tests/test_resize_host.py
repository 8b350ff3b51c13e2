"""Resized windows without a device: the symbols and the enum, every refusal of htj2k_frames_to_tensor_resized with a NULL
context, htj2k_resize_weights against the Python-integer model (resize_model) with the properties the header promises,
and the model itself against torch's interpolate on the CPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ffmpeg_ht_amd as m
import resize_model as rm
import tensor_model as tm
from test_tensor_host import frame

EINVAL, ENOSYS, PATCHWELCOME = -22, -38, -0x45574150
EXTREMES = [(32768, 512), (32767, 512), (32768, 513), (4097, 65), (1, 32768), (32768, 32768)]


@pytest.fixture(scope="module")
def L():
    return m.load_library()


def call(L, frames, bits, spec, windows=None, filt=2, dst=0x1000, dst_bytes=1 << 44, n=None):
    arr = (m.Frame * len(frames))(*frames) if frames is not None else None
    win = None if windows is None else (ctypes.c_int32 * len(windows))(*windows)
    return L.htj2k_frames_to_tensor_resized(None, arr, 0, len(frames) if n is None else n, bits, None if spec is None else ctypes.byref(spec),
                                            win, filt, ctypes.c_void_p(dst), ctypes.c_size_t(dst_bytes))


def spec_of(size=(4, 4), name="float16", **kw):
    s = m.tensor_spec(name, "NCHW", size)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_symbols_and_the_enum(L):
    for name in ("htj2k_resize_weights", "htj2k_frames_to_tensor_resized", "htj2k_job_to_tensor_resized", "htj2k_pipe_receive_tensor_resized"):
        assert hasattr(L, name) and name in m.EXPORTS
    assert m.RESIZE_FILTERS == ["nearest", "bilinear", "triangle"]
    assert (rm.NEAREST, rm.BILINEAR, rm.TRIANGLE) == (0, 1, 2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "htj2k_amd.h")).read()
    assert "enum { HTJ2K_RESIZE_NEAREST = 0, HTJ2K_RESIZE_BILINEAR = 1, HTJ2K_RESIZE_TRIANGLE = 2 };" in header
    for name in ("Decoder.resize_weights", "Decoder.to_tensor_resized", "Job.to_tensor_resized", "Pipe.receive_tensor_resized"):
        cls, fn = name.split(".")
        assert callable(getattr(getattr(m, cls), fn))


def test_refusals_in_their_order_with_a_null_context(L):
    ok = spec_of()
    f = frame("yuv420p", 20, 10)
    assert call(L, [f], 8, ok) == ENOSYS                                   # valid arguments, no context
    assert call(L, [f, frame("yuv420p", 33, 7)], 8, spec_of((64, 3)), [3, 1, 17, 9, 0, 0, 33, 7], filt=1, dst_bytes=2 * 3 * 64 * 3 * 2) == ENOSYS
    pal = frame("pal8", 20, 10)
    # missing arguments and n come before the layout
    assert call(L, None, 8, ok, n=1) == EINVAL and call(L, [pal], 8, None) == EINVAL
    assert call(L, [pal], 8, ok, dst=0) == EINVAL and call(L, [pal], 8, ok, n=0) == EINVAL
    # the layout comes before bits, dtype, layout, the filter and the size
    assert call(L, [pal], 99, spec_of(dtype=7, layout=9, out_w=-1), filt=9) == PATCHWELCOME
    assert call(L, [f], 9, ok) == EINVAL and call(L, [f], 0, ok) == EINVAL
    assert call(L, [f], 8, spec_of(dtype=3)) == EINVAL and call(L, [f], 8, spec_of(layout=2)) == EINVAL
    # the filter
    for filt in (-1, 3, 100):
        assert call(L, [f], 8, ok, filt=filt) == EINVAL
    for filt in (0, 1, 2):
        assert call(L, [f], 8, ok, filt=filt) == ENOSYS
    # scale and bias: the first C entries
    s = spec_of()
    s.scale[2] = float("nan")
    assert call(L, [f], 8, s) == EINVAL
    s = spec_of()
    s.bias[3] = float("inf")
    assert call(L, [f], 8, s) == ENOSYS
    # the size: both at least 1; there is no 0 x 0
    for ow, oh in ((0, 0), (0, 1), (1, 0), (-1, -1), (4, -1)):
        assert call(L, [f], 8, spec_of(out_w=ow, out_h=oh)) == EINVAL
    # the frames: one layout, a size, planes, linesizes -- and sizes may differ
    assert call(L, [f, frame("yuv422p", 20, 10)], 8, ok) == EINVAL
    assert call(L, [f, frame("yuv420p", 21, 11)], 8, ok) == ENOSYS
    assert call(L, [frame("yuv420p", 0, 10)], 8, ok) == EINVAL
    g = frame("yuv420p", 20, 10)
    g.data[1] = None
    assert call(L, [g], 8, ok) == EINVAL
    g = frame("yuv420p", 20, 10)
    g.linesize[2] = 9
    assert call(L, [g], 8, ok) == EINVAL
    # the windows
    for bad in ([0, 0, 0, 4], [0, 0, 4, 0], [0, 0, -3, 4], [-1, 0, 4, 4], [0, -1, 4, 4], [17, 0, 4, 4], [0, 7, 4, 4], [0, 0, 21, 10], [0, 0, 20, 11],
                [2 ** 31 - 1, 0, 2 ** 31 - 1, 1]):
        assert call(L, [f], 8, ok, bad) == EINVAL, bad
    assert call(L, [f], 8, ok, [16, 6, 4, 4]) == ENOSYS and call(L, [f], 8, ok, [19, 9, 1, 1]) == ENOSYS
    assert call(L, [f, f], 8, ok, [0, 0, 4, 4, 0, 0, 4, -4]) == EINVAL
    # out of scope: a size, a reduction; after every window's own refusals, before the destination's
    big = frame("gray", 40000, 2)
    assert call(L, [big], 8, ok, filt=1) == PATCHWELCOME and call(L, [big], 8, ok, [0, 0, 32769, 2], filt=0) == PATCHWELCOME
    assert call(L, [big], 8, spec_of((1024, 2)), [7232, 0, 32768, 2]) == ENOSYS
    tall = frame("gray", 2, 40000)
    assert call(L, [tall], 8, spec_of((2, 1024)), [0, 0, 2, 32769], filt=1) == PATCHWELCOME
    assert call(L, [f], 8, spec_of((32769, 4))) == PATCHWELCOME and call(L, [f], 8, spec_of((4, 32769)), filt=0) == PATCHWELCOME
    assert call(L, [f], 8, spec_of((32768, 4))) == ENOSYS
    wide = frame("gray", 130, 10)
    assert call(L, [wide], 8, spec_of((2, 10))) == PATCHWELCOME
    assert call(L, [wide], 8, spec_of((2, 10)), filt=1) == ENOSYS and call(L, [wide], 8, spec_of((2, 10)), filt=0) == ENOSYS
    assert call(L, [wide], 8, spec_of((2, 10)), [1, 0, 128, 10]) == ENOSYS
    assert call(L, [frame("gray", 10, 130)], 8, spec_of((10, 2))) == PATCHWELCOME
    assert call(L, [wide, wide], 8, spec_of((2, 10)), [0, 0, 130, 10, 0, 0, 131, 10]) == EINVAL       # frame 1 leaves its frame: first
    assert call(L, [wide], 8, spec_of((2, 10)), dst_bytes=1) == PATCHWELCOME                          # before dst_bytes
    g = frame("gray", 130, 10)
    g.linesize[0] = 129
    assert call(L, [g], 8, spec_of((2, 10))) == EINVAL                                                # behind the linesizes
    # the destination
    need = 3 * 4 * 4 * 2
    assert call(L, [f], 8, ok, dst_bytes=need) == ENOSYS and call(L, [f], 8, ok, dst_bytes=need - 1) == EINVAL
    assert call(L, [f], 8, ok, dst=0x1001) == EINVAL and call(L, [f], 8, spec_of(name="float32"), dst=0x1002) == EINVAL


def test_job_pipe_and_weight_calls_refuse_their_arguments(L):
    ok = spec_of()
    assert L.htj2k_job_to_tensor_resized(None, None, 0, ctypes.byref(ok), None, 2, ctypes.c_void_p(0x1000), ctypes.c_size_t(1 << 20), None) == EINVAL
    assert L.htj2k_pipe_receive_tensor_resized(None, None, 0, ctypes.byref(ok), None, 2, ctypes.c_void_p(0x1000), ctypes.c_size_t(1 << 20)) == EINVAL
    first, q = ctypes.c_int32(), (ctypes.c_uint16 * 129)()
    w = lambda win, out, filt, x, cap=129, fp=ctypes.byref(first), qp=q: L.htj2k_resize_weights(win, out, filt, x, fp, qp, cap)
    assert len(rm.weights(10, 4, 2, 1)[1]) == 5
    assert w(10, 4, 2, 1) == 5 and w(10, 4, 2, 1, cap=5) == 5 and w(10, 4, 2, 1, cap=4) == EINVAL
    for bad in ((0, 4, 2, 0), (10, 0, 2, 0), (10, 4, 3, 0), (10, 4, -1, 0), (10, 4, 2, 4), (10, 4, 2, -1)):
        assert w(*bad) == EINVAL, bad
    assert w(10, 4, 2, 0, fp=None) == EINVAL and w(10, 4, 2, 0, qp=None) == EINVAL
    assert w(32769, 4096, 1, 0) == PATCHWELCOME and w(4, 32769, 0, 0) == PATCHWELCOME
    assert w(65, 1, 2, 0) == PATCHWELCOME and w(65, 1, 1, 0) == 1 and w(64, 1, 2, 0) == 64
    with pytest.raises(ValueError):
        m.Decoder.resize_weights(4, 4, "cubic", 0)


def check_axis(win, out, xs, seen):
    """the C weights of the x in xs against the model, with the properties of the header"""
    for filt in (rm.NEAREST, rm.BILINEAR, rm.TRIANGLE):
        if not rm.in_scope(win, out, filt):
            continue
        for x in xs:
            first, q = m.Decoder.resize_weights(win, out, filt, x)
            assert (first, q) == rm.weights(win, out, filt, x, seen), (win, out, filt, x)
            assert sum(q) == 16384 and 1 <= len(q) <= 129 and min(q) >= 0
            assert 0 <= first and first + len(q) <= win                      # contiguous by construction, inside the window


def test_weights_equal_the_model_on_every_small_axis():
    seen = {}
    for win in range(1, 41):
        for out in range(1, 41):
            check_axis(win, out, range(out), seen)
            for filt in (rm.BILINEAR, rm.TRIANGLE):                            # the model's short walk is the definition's
                for x in range(out):
                    assert rm.weights(win, out, filt, x) == rm.weights(win, out, filt, x, walk_all=True)
    assert max(seen.values()) < 1 << 31


@pytest.mark.parametrize("win,out", EXTREMES)
def test_weights_at_the_extremes(win, out):
    seen = {}
    xs = range(out) if out <= 1024 else sorted(set(list(range(300)) + list(range(out - 300, out)) + list(range(0, out, 97))))
    check_axis(win, out, xs, seen)
    # what the header promises of the intermediates, in Python integers
    assert seen["cx"] < 1 << 31 and seen.get("centre", 0) < 1 << 31 and seen.get("shifted", 0) < 1 << 31 and seen.get("A", 0) < 1 << 23
    if (win, out) == (32768, 512):
        assert len(rm.weights(win, out, rm.TRIANGLE, 100)[1]) == 128 and seen["A"] == 1 << 22


def test_identity_and_constant_pictures_on_the_model():
    rng = np.random.default_rng(4)
    src = rng.integers(0, 65536, size=(9, 13))
    for filt in (rm.NEAREST, rm.BILINEAR, rm.TRIANGLE):
        for n in (1, 2, 7, 40):
            for x in range(n):
                assert rm.weights(n, n, filt, x) == (x, [16384])
        assert np.array_equal(rm.resample(src, 13, 9, filt), src.astype(np.float32))
        for value in (0, 1, 255, 65535):
            for (h, w), (oh, ow) in (((9, 13), (4, 5)), ((3, 130), (7, 3)), ((2, 2), (9, 31))):
                assert np.array_equal(rm.resample(np.full((h, w), value), ow, oh, filt), np.full((oh, ow), value, np.float32))
    planes = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((10, 20), (5, 10), (5, 10))]
    for dtype in tm.DTYPES:
        for layout in ("NCHW", "NHWC"):
            assert np.array_equal(rm.image(planes, "yuv420p", 8, dtype, layout, (7, 5), (3, 1, 7, 5), rm.TRIANGLE, 1 / 255, -0.5),
                                  tm.image(planes, "yuv420p", 8, dtype, layout, (7, 5), (3, 1), 1 / 255, -0.5))


# (source h, w) -> (output h, w): up, down, mixed, identity, one pixel either side, 128 taps
SHAPES = [((1, 1), (4, 4)), ((2, 3), (5, 7)), ((7, 5), (7, 5)), ((9, 11), (3, 4)), ((16, 16), (17, 31)), ((13, 29), (6, 5)),
          ((32, 32), (8, 8)), ((5, 64), (5, 1)), ((40, 24), (64, 48)), ((3, 200), (3, 7)), ((16, 1024), (16, 16))]


def test_model_against_torch_interpolate(capsys):
    """The comparison is not bit for bit: the weights are 14-bit.  Each is off by less than 2^-14 and one tap carries a
    remainder below taps * 2^-14, so a pixel differs by less than peak * 2 * (taps_x + taps_y) * 2^-14; 2^-18 more
    covers torch's own binary32 sums."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for (h, w), (oh, ow) in SHAPES:
        for bits in (8, 16):
            peak = (1 << bits) - 1
            src = rng.integers(0, peak + 1, size=(h, w))
            t = torch.from_numpy(src.astype(np.float32))[None, None]
            for filt, aa in ((rm.BILINEAR, False), (rm.TRIANGLE, True)):
                want = F.interpolate(t, size=(oh, ow), mode="bilinear", align_corners=False, antialias=aa)[0, 0].numpy()
                got = rm.resample(src, ow, oh, filt)
                taps_x = max(len(rm.weights(w, ow, filt, x)[1]) for x in range(ow))
                taps_y = max(len(rm.weights(h, oh, filt, y)[1]) for y in range(oh))
                bound = peak * (2 * (taps_x + taps_y) * 2.0 ** -14 + 2.0 ** -18)
                err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
                worst = max(worst, err / bound)
                assert err <= bound, ((h, w), (oh, ow), bits, filt, err, bound)
    assert max(len(rm.weights(1024, 16, rm.TRIANGLE, x)[1]) for x in range(16)) == 128
    with capsys.disabled():
        print("\nresize model against torch: the largest error is %.3f of its bound" % worst)


def test_model_nearest_is_torch_nearest_exact():
    rng = np.random.default_rng(12)
    for (h, w), (oh, ow) in SHAPES + [((37, 53), (224, 224)), ((224, 224), (37, 53))]:
        src = rng.integers(0, 65536, size=(h, w))
        want = F.interpolate(torch.from_numpy(src.astype(np.float32))[None, None], size=(oh, ow), mode="nearest-exact")[0, 0].numpy()
        assert np.array_equal(rm.resample(src, ow, oh, rm.NEAREST), want), ((h, w), (oh, ow))
