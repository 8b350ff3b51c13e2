"""The tensor calls with transfer curves, without a device: the symbols and the structs, every refusal of the _curves entry
points with a NULL context (and, with curves = NULL, their agreement with the _mix calls), htj2k_tensor_curve_fill and
htj2k_tensor_mix_xyz against their float64 restatements, and the numpy model (curve_model) against torch on the CPU, the
identity, the exact lookup and the true functions of a digital cinema package."""
import ctypes
import math

import numpy as np
import pytest
import torch

import curve_model as cvm
import ffmpeg_ht_amd as m
import mix_model as mm
import tensor_model as tm
from test_tensor_host import frame

EINVAL, ENOSYS, PATCHWELCOME = -22, -38, -0x45574150
NEW = ["htj2k_tensor_curve_fill", "htj2k_tensor_mix_xyz", "htj2k_frames_to_tensor_curves", "htj2k_job_to_tensor_curves",
       "htj2k_pipe_receive_tensor_curves", "htj2k_frames_to_tensor_resized_curves", "htj2k_job_to_tensor_resized_curves",
       "htj2k_pipe_receive_tensor_resized_curves"]


@pytest.fixture(scope="module")
def L():
    lib = m.load_library()
    lib.htj2k_tensor_curve_fill.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    lib.htj2k_tensor_mix_xyz.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    return lib


def _arr(v, per):
    return None if v is None else (ctypes.c_int32 * len(v))(*v)


def call(L, frames, bits, spec, mix, curves, origins=None, dst=0x1000, dst_bytes=1 << 40, resized=None, twin=False):
    """htj2k_frames_to_tensor_curves with a NULL context (resized: (windows, filter), the resized call); twin: the _mix call"""
    arr = (m.Frame * len(frames))(*frames)
    mp = None if mix is None else ctypes.byref(mix)
    head = (None, arr, 0, len(frames), bits, ctypes.byref(spec), mp) + (() if twin else (None if curves is None else ctypes.byref(curves),))
    tail = (ctypes.c_void_p(dst), ctypes.c_size_t(dst_bytes))
    if resized is None:
        fn = L.htj2k_frames_to_tensor_mix if twin else L.htj2k_frames_to_tensor_curves
        return fn(*head, _arr(origins, 2), *tail)
    fn = L.htj2k_frames_to_tensor_resized_mix if twin else L.htj2k_frames_to_tensor_resized_curves
    return fn(*head, _arr(resized[0], 4), resized[1], *tail)


def eye(k, c=3):
    return m.tensor_mix(np.eye(k, c, dtype=np.float32))


def ramp(n=16):
    return m.tensor_curve(np.arange(n, dtype=np.float32))


def test_symbols_and_structs(L):
    for name in NEW:
        assert hasattr(L, name) and name in m.EXPORTS, name
    assert ctypes.sizeof(m.TensorCurve) == 24 and ctypes.sizeof(m.TensorCurves) == 88
    assert m.TensorCurves.in_mask.offset == 48 and m.TensorCurves.gain.offset == 56 and m.TensorCurves.offset.offset == 72
    cv = m.tensor_curve([0, 0.5, 2], 1.5, 4)
    assert (cv.n, cv.x0, cv.inv_dx) == (3, 1.5, 4.0) and [cv.t[j] for j in range(3)] == [0.0, 0.5, 2.0]
    q = m.tensor_curves(cv, None)
    assert (q.in_.n, q.out.n, q.in_mask, q.out_mask) == (3, 0, 7, 7) and list(q.gain) == [1.0] * 4 and list(q.offset) == [0.0] * 4
    assert q.tables[0] is cv.table and q.tables[1] is None
    q = m.tensor_curves(None, cv, 5, 9, [2, 3], -0.0)
    assert (q.in_.n, q.out.n, q.in_mask, q.out_mask) == (0, 3, 5, 9) and list(q.gain) == [2.0, 3.0, 1.0, 1.0]
    assert all(math.copysign(1, v) == -1 for v in q.offset)
    with pytest.raises(ValueError):
        m.tensor_curves(np.arange(4.0))
    with pytest.raises(ValueError):
        m.tensor_curve(np.zeros((2, 2)))
    mix, q = m.Decoder.dcp_curves()
    assert (mix.nout, q.in_.n, q.out.n, q.in_mask, q.out_mask) == (3, 4096, 4097, 7, 7)
    assert (q.in_.x0, q.in_.inv_dx, q.out.x0, q.out.inv_dx) == (0.0, 1.0, 0.0, 4096.0)


def test_refusals_in_their_order_with_a_null_context(L):
    ok = m.tensor_spec("float16")
    f = frame("yuv420p", 20, 10)                             # C = 3
    good = lambda **kw: m.tensor_curves(ramp(), ramp(4097), **kw)
    assert call(L, [f], 8, ok, eye(3), good()) == ENOSYS     # valid arguments, no context
    assert call(L, [f], 8, ok, eye(3), m.tensor_curves(ramp(2), None)) == ENOSYS
    assert call(L, [f], 8, ok, eye(3), m.tensor_curves(None, ramp(2))) == ENOSYS
    assert call(L, [f], 8, ok, eye(3), good(), resized=(None, 2)) == EINVAL      # a resized call has no 0 x 0
    win = m.tensor_spec("float16", size=(4, 4))
    assert call(L, [f], 8, win, eye(3), good(), resized=(None, 2)) == ENOSYS

    def broken(what):
        q = good()
        nan_tab = np.arange(16, dtype=np.float32)
        if what == "both none":
            q = m.tensor_curves(None, None)
        elif what in ("n 1", "n 4098", "n -1"):
            q.out.n = int(what[2:])
        elif what == "n 4098 without a table":               # the count is refused before the pointer is looked at
            q.in_.n, q.in_.t = 4098, None
        elif what == "no table":
            q.out.t = None
        elif what in ("x0 nan", "x0 inf"):
            q.in_.x0 = float(what[3:])
        elif what in ("inv nan", "inv inf", "inv 0", "inv -1"):
            q.out.inv_dx = float(what[4:])
        elif what in ("entry nan", "entry inf", "entry big"):
            nan_tab[7] = {"nan": math.nan, "inf": -math.inf, "big": 2.0 ** 101}[what[6:]]
            q = m.tensor_curves(m.tensor_curve(nan_tab), ramp(4097))
        elif what == "in_mask":
            q.in_mask = 8
        elif what == "out_mask":
            q.out_mask = 4                                   # K = 2 below
        elif what == "gain":
            q.out_mask, q.gain[1] = 3, math.inf
        elif what == "offset":
            q.out_mask, q.offset[0] = 3, math.nan
        return q

    every = ["both none", "n 1", "n 4098", "n -1", "n 4098 without a table", "no table", "x0 nan", "x0 inf", "inv nan", "inv inf", "inv 0",
             "inv -1", "entry nan", "entry inf", "entry big", "in_mask", "out_mask", "gain", "offset"]
    pal = frame("pal8", 20, 10)
    for what in every:
        q = broken(what)
        mix = eye(2) if what in ("out_mask", "gain", "offset") else eye(3)
        assert call(L, [f], 8, ok, mix, q) == EINVAL, what
        assert call(L, [f], 8, win, mix, q, resized=(None, 2)) == EINVAL, what
        # behind the layout and the mix, in front of the windows and the destination
        assert call(L, [pal], 8, ok, mix, q) == PATCHWELCOME, what
        assert call(L, [f], 8, ok, mix, q, origins=[30, 0]) == EINVAL, what
    # curves without a mix: refused, whatever the curves hold
    assert call(L, [f], 8, ok, None, good()) == EINVAL
    assert call(L, [f], 8, ok, None, broken("n 4098 without a table")) == EINVAL
    # 2^100 itself is allowed; entries that are not read may hold anything
    edge = np.arange(16, dtype=np.float32)
    edge[3], edge[4] = 2.0 ** 100, -2.0 ** 100
    assert call(L, [f], 8, ok, eye(3), m.tensor_curves(m.tensor_curve(edge), None)) == ENOSYS
    q = m.tensor_curves(ramp(), None, out_mask=3)
    q.out.x0, q.out.inv_dx, q.out.t = math.nan, -1.0, ctypes.cast(8, ctypes.POINTER(ctypes.c_float))
    q.gain[3], q.offset[2] = math.nan, math.inf
    assert call(L, [f], 8, ok, eye(2), q) == ENOSYS
    # a gain at K - 1 is read
    q.gain[1] = math.nan
    assert call(L, [f], 8, ok, eye(2), q) == EINVAL
    # the mix itself is refused first, the window and the destination last
    bad = eye(3)
    bad.nout = 5
    assert call(L, [f], 8, ok, bad, good()) == EINVAL
    assert call(L, [f], 8, ok, eye(3), good(), dst_bytes=3 * 20 * 10 * 2 - 1) == EINVAL
    assert call(L, [f], 8, ok, eye(3), good(), dst_bytes=3 * 20 * 10 * 2) == ENOSYS


def test_curves_null_is_the_mix_call(L):
    ok, win = m.tensor_spec("float16"), m.tensor_spec("float32", "NHWC", (4, 4))
    f, pal = frame("yuv420p", 20, 10), frame("pal8", 20, 10)
    bad = eye(3)
    bad.nout = 0
    for frames, bits, spec, mix, kw in (([f], 8, ok, eye(3), {}), ([f], 8, ok, None, {}), ([f], 9, ok, eye(3), {}), ([pal], 8, ok, eye(3), {}),
                                        ([f], 8, ok, bad, {}), ([f], 8, ok, eye(4), {"dst_bytes": 1200}), ([f], 8, ok, eye(3), {"dst": 0}),
                                        ([f], 8, win, eye(3), {"origins": [17, 0]}), ([f], 8, win, eye(3), {"origins": [16, 6]}),
                                        ([f], 8, win, eye(3), {"resized": (None, 2)}), ([f], 8, win, eye(3), {"resized": ([0, 0, 21, 10], 2)}),
                                        ([f], 8, win, eye(3), {"resized": (None, 7)}), ([f], 8, ok, eye(3), {"resized": (None, 1)})):
        assert call(L, frames, bits, spec, mix, None, **kw) == call(L, frames, bits, spec, mix, None, twin=True, **kw), (bits, kw)
    spec, e, b = m.tensor_spec("bfloat16"), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert m.Decoder.tensor_image_size("xyz12le", 9, 5, 12, spec, m.Decoder.xyz_mix(709)) == (3 * 45, 3 * 45 * 2)
    for name in ("htj2k_job_to_tensor_curves", "htj2k_job_to_tensor_resized_curves", "htj2k_pipe_receive_tensor_curves",
                 "htj2k_pipe_receive_tensor_resized_curves"):
        fn = getattr(L, name)
        args = (None, None, 8, ctypes.byref(spec), None, None, None) + ((2,) if "resized" in name else ()) + (ctypes.c_void_p(0x1000), ctypes.c_size_t(64))
        assert fn(*(args + ((None,) if "job" in name else ()))) == EINVAL, name


def ulps(got, want64):
    """the distance of float32 values from float64 ones, in units of the float32 spacing at the value"""
    want32 = want64.astype(np.float32)
    ulp = np.spacing(np.abs(want32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want64) / ulp


@pytest.mark.parametrize("kind", cvm.KINDS)
def test_curve_fill_against_float64(L, kind):
    for n in (2, 3, 256, 4096, 4097):
        for lo, hi in ((0.0, 1.0), (0.25, 0.75), (-0.5, 1.5), (0.0, 4095.0 / 4096.0)):
            param = 2.6 if kind == "power" else 0.0
            got = m.curve_table(kind, n, lo, hi, param)
            assert got.dtype == np.float32 and got.shape == (n,)
            want = cvm.curve_fill(kind, n, lo, hi, param)
            assert ulps(got, want).max() <= 1.0, (kind, n, lo, hi, float(ulps(got, want).max()))
            if kind != "power":                              # the argument is clamped: flat beyond 0 .. 1
                assert got[0] == np.float32(cvm.function(kind, max(lo, 0.0))) and got[-1] == np.float32(cvm.function(kind, min(hi, 1.0)))
    assert np.array_equal(m.curve_table("power", 5, -1.0, 1.0, 0.5)[:3], np.zeros(3, np.float32))
    assert m.curve_table(cvm.KINDS.index(kind), 2)[1] == np.float32(cvm.function(kind, 1.0, 0.0))


def test_curve_fill_refusals(L):
    t = (ctypes.c_float * 4)(9, 9, 9, 9)
    for args in ((None, 4, 0, 2.6, 0.0, 1.0), (t, 1, 0, 2.6, 0.0, 1.0), (t, 0, 0, 2.6, 0.0, 1.0), (t, 4, -1, 2.6, 0.0, 1.0),
                 (t, 4, 7, 2.6, 0.0, 1.0), (t, 4, 0, 2.6, 1.0, 1.0), (t, 4, 0, 2.6, 1.0, 0.0), (t, 4, 0, math.nan, 0.0, 1.0),
                 (t, 4, 1, math.inf, 0.0, 1.0), (t, 4, 0, 2.6, -math.inf, 1.0), (t, 4, 0, 2.6, 0.0, math.nan)):
        assert L.htj2k_tensor_curve_fill(*args) == EINVAL, args[1:]
    assert list(t) == [9.0] * 4
    with pytest.raises(ValueError):
        m.curve_table("gamma", 4)
    with pytest.raises(m.Htj2kError):
        m.curve_table("power", 1)


def test_mix_xyz_against_float64(L):
    for primaries in (709, 2020, m.PRIMARIES_P3D65):
        for scale in (1.0, 52.37 / 48.0, -3.0):
            mix = m.Decoder.xyz_mix(primaries, scale)
            k, mat, b = mm.unpack(mix)
            want = cvm.xyz(primaries, scale)
            assert k == 3 and not b.any() and not mat[3].any() and not mat[:, 3].any()
            assert ulps(mat[:3, :3], want).max() <= 1.0, (primaries, scale)
        white = np.array([cvm.D65[0] / cvm.D65[1], 1.0, (1 - cvm.D65[0] - cvm.D65[1]) / cvm.D65[1]])
        _, mat, _ = mm.unpack(m.Decoder.xyz_mix(primaries))
        assert np.abs(mat[:3, :3].astype(np.float64) @ white - 1.0).max() <= 1e-6, primaries
    # 709's matrix against the four digits printed in IEC 61966-2-1, which come from a rounded matrix inverted: 4e-4 apart
    _, mat, _ = mm.unpack(m.Decoder.xyz_mix(709))
    assert np.abs(mat[:3, :3] - np.array([[3.2406, -1.5372, -0.4986], [-0.9689, 1.8758, 0.0415], [0.0557, -0.2040, 1.0570]])).max() < 5e-4
    buf = (ctypes.c_uint8 * 96)(*([0xEE] * 96))
    assert L.htj2k_tensor_mix_xyz(buf, 2020, 1.0) == 0 and bytes(buf[84:]) == b"\xee" * 12
    for args in ((None, 709, 1.0), (buf, 601, 1.0), (buf, 0, 1.0), (buf, 709, math.nan), (buf, 709, math.inf)):
        assert L.htj2k_tensor_mix_xyz(*args) == EINVAL, args[1:]


def test_model_against_a_torch_chain_on_the_cpu():
    rng = np.random.default_rng(8)
    s = rng.integers(0, 4096, (3, 50000))
    for primaries, out, n_out, gain, offset in ((709, "srgb", 4097, None, None), (2020, "pq", 1024, [2.0, 2.0, 2.0], [-1.0, -1.0, -1.0]),
                                                 (3, "bt709", 3, 255.0, 0.5)):
        mix, q = m.Decoder.dcp_curves(primaries, out, n_out, gain, offset)
        k, mat, b = mm.unpack(mix)
        want = np.stack(cvm.values([s[c].astype(np.float32) for c in range(3)], mix, q))
        assert not np.isnan(want).any()
        got = cvm.torch_chain(torch.from_numpy(s), torch.from_numpy(q.tables[0]), mat[:3], b, torch.from_numpy(q.tables[1]), float(q.out.x0),
                          float(q.out.inv_dx), list(q.gain), list(q.offset))
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), (primaries, out)


def frame_of(fmt, comps, bits):
    """planes of a frame whose components hold the given samples (cmp_model's packing: rows of interleaved samples,
    shifted as the layout stores them)"""
    h, w = comps[0].shape
    if fmt == "xyz12le":
        return [(np.stack(comps, -1).astype(np.uint16) << (16 - bits)).reshape(h, w * 3)]
    if fmt == "rgb24":
        return [(np.stack(comps, -1).astype(np.uint8) << (8 - bits)).reshape(h, w * 3)]
    raise ValueError(fmt)


def test_identity_curve_gives_the_mix_models_bits():
    rng = np.random.default_rng(5)
    for fmt, bits in (("xyz12le", 12), ("rgb24", 8), ("rgb24", 7)):
        comps = [rng.integers(0, 1 << bits, (9, 33)) for _ in range(3)]
        planes = frame_of(fmt, comps, bits)
        assert all(np.array_equal(a, b) for a, b in zip(mm.cm.components(planes, fmt, bits), comps))
        q = m.tensor_curves(m.tensor_curve(np.arange(1 << bits, dtype=np.float32)), None, offset=-0.0)
        for k, dtype, layout in ((3, "float32", "NCHW"), (4, "float16", "NHWC"), (1, "bfloat16", "NCHW")):
            mix = m.tensor_mix(rng.normal(0, 1 / 64, (k, 3)) * np.array([1, -1, 0]), np.linspace(-0.0, 1, k))
            assert np.array_equal(cvm.image(planes, fmt, bits, mix, q, dtype, layout), mm.image(planes, fmt, bits, mix, dtype, layout))


def test_exact_lookup_of_all_4096_samples():
    rng = np.random.default_rng(6)
    table = rng.normal(0, 100, 4096).astype(np.float32)      # negative and non-monotone entries
    table[17], table[18] = 0.0, -0.0
    s = np.arange(4096, dtype=np.float32)
    got = cvm.curve_eval(s, table)
    assert np.array_equal(got[np.abs(table) > 0].view(np.uint32), table[np.abs(table) > 0].view(np.uint32))
    assert got[17] == 0 and got[18] == 0                     # only the sign of a zero entry can change
    comps = [rng.permutation(4096).reshape(64, 64) for _ in range(3)]
    planes = frame_of("xyz12le", comps, 12)
    img = cvm.image(planes, "xyz12le", 12, m.tensor_mix(np.eye(3)), m.tensor_curves(m.tensor_curve(table), None, offset=-0.0))
    for c in range(3):
        direct = table[comps[c]]
        assert np.array_equal(img[c].view(np.float32)[direct != 0], direct[direct != 0])


def test_dcp_accuracy_against_the_true_functions():
    """dcp_curves(709, "srgb", 4097) in the model on 2 000 000 seeded random X'Y'Z' triples against the float64 evaluation
    of the true functions: at most 3e-5 on the nominal 0 .. 1 scale.  The interpolation bound h^2 / 8 max|f''| is 1.8e-5 at
    the sRGB knee for h = 1 / 4096; the margin covers the binary32 roundings of the mix"""
    s = np.random.default_rng(2084).integers(0, 4096, (2000000, 3))
    mix, q = m.Decoder.dcp_curves(709, "srgb", 4097)
    got = np.stack(cvm.values([s[:, c].astype(np.float32) for c in range(3)], mix, q), -1).astype(np.float64)
    err = np.abs(got - cvm.dcp_true(s, 709, "srgb")).max()
    print("largest absolute error: %.3e" % err)
    assert err <= 3e-5, err
