"""Tensors as frames with transfer curves, without a device: the symbols and the structs, the ten refusals of
htj2k_tensor_to_frames_curves and htj2k_encode_tensor_curves in their order with a NULL context (and, with curves = NULL,
their agreement with the _mix calls), htj2k_tensor_curve_fill_root and htj2k_tensor_mix_in_xyz against their float64
restatements, the numpy model (curve_in_model) against a torch chain on the CPU, the reason the `root` field exists
(the table of DESIGN.md 3.5, "Transfer curves on the way in"), the X'Y'Z' round trip and the identity."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cmp_model as cm
import curve_in_model as cim
import curve_model as cvm
import ffmpeg_ht_amd as m
import tensor_mix_in_model as tmi
from test_tensor_host import frame
from test_tensor_mix_in_host import enc_call as mix_enc_call, frames_call as mix_frames_call

EINVAL, ENOSYS, PATCHWELCOME = -22, -38, -0x45574150
NEW = ("htj2k_tensor_curve_fill_root", "htj2k_tensor_mix_in_xyz", "htj2k_tensor_to_frames_curves", "htj2k_encode_tensor_curves")
P3 = m.PRIMARIES_P3D65


@pytest.fixture(scope="module")
def L():
    lib = m.load_library()
    lib.htj2k_tensor_curve_fill_root.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                                 ctypes.c_double, ctypes.c_int]
    lib.htj2k_tensor_mix_in_xyz.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    return lib


def _p(x):
    return None if x is None else ctypes.byref(x)


def enc_call(L, spec, mix, curves, fmt="yuv420p", w=20, h=10, bits=8, n=1, src=0x1000, src_bytes=1 << 40):
    """htj2k_encode_tensor_curves with a NULL context on memory that is never touched"""
    offs = (ctypes.c_size_t * (n + 2))()
    return L.htj2k_encode_tensor_curves(None, ctypes.c_void_p(src), ctypes.c_size_t(src_bytes), n, w, h, m.PIX_NAMES.index(fmt), bits, _p(spec),
                                        _p(mix), _p(curves), None, ctypes.c_void_p(0x1000), ctypes.c_size_t(1 << 20), 0, offs)


def frames_call(L, spec, mix, curves, frames, bits=8, src=0x1000, src_bytes=1 << 40):
    arr = (m.Frame * len(frames))(*frames)
    return L.htj2k_tensor_to_frames_curves(None, ctypes.c_void_p(src), ctypes.c_size_t(src_bytes), len(frames), bits, _p(spec), _p(mix),
                                           _p(curves), arr)


def ramp(n=16, root=0):
    return m.tensor_curve_in(np.arange(n, dtype=np.float32), root=root)


def ones(nc=3, K=3):
    return m.tensor_mix_in(np.ones((nc, K)))


def test_symbols_and_structs(L):
    for name in NEW:
        assert hasattr(L, name) and name in m.EXPORTS, name
    assert ctypes.sizeof(m.TensorCurveIn) == 24 and ctypes.sizeof(m.TensorCurvesIn) == 88
    assert (m.TensorCurveIn.root.offset, m.TensorCurveIn.x0.offset, m.TensorCurveIn.t.offset) == (4, 8, 16)
    assert m.TensorCurvesIn.in_mask.offset == 48 and m.TensorCurvesIn.gain.offset == 56 and m.TensorCurvesIn.offset.offset == 72
    assert ctypes.sizeof(m.TensorCurve) == 24 and ctypes.sizeof(m.TensorCurves) == 88     # the other direction's keep their size
    cv = m.tensor_curve_in([0, 0.5, 2], 1.5, 4, 3)
    assert (cv.n, cv.root, cv.x0, cv.inv_dx) == (3, 3, 1.5, 4.0) and [cv.t[j] for j in range(3)] == [0.0, 0.5, 2.0]
    q = m.tensor_curves_in(cv, None)
    assert (q.in_.n, q.in_.root, q.out.n, q.in_mask, q.out_mask) == (3, 3, 0, 7, 7) and list(q.gain) == [1.0] * 4 and list(q.offset) == [0.0] * 4
    assert q.tables[0] is cv.table and q.tables[1] is None
    # masks left to the call: the struct holds 7, and the calls that know K and C pass its bits below them
    assert q.auto_masks == (True, True) and m.tensor_curves_in(cv, None, 3).auto_masks == (False, True)
    for fmt, K, want in (("gray", 1, (1, 1)), ("ya8", 2, (3, 3)), ("yuv420p", 4, (7, 7)), ("rgba", 3, (7, 7))):
        cut = m._curves_in_p(q, ones(cm.LAYOUTS[fmt][0], K), m.PIX_NAMES.index(fmt), 8)._obj
        assert (cut.in_mask, cut.out_mask) == want and (q.in_mask, q.out_mask) == (7, 7) and cut.tables is q.tables, fmt
    given = m.tensor_curves_in(cv, None, 7, 7)
    assert m._curves_in_p(given, ones(1, 1), m.PIX_NAMES.index("gray"), 8)._obj is given
    q = m.tensor_curves_in(None, cv, 5, 9, [2, 3], -0.0)
    assert (q.in_.n, q.out.n, q.out.root, q.in_mask, q.out_mask) == (0, 3, 3, 5, 9) and list(q.gain) == [2.0, 3.0, 1.0, 1.0]
    assert all(math.copysign(1, v) == -1 for v in q.offset)
    with pytest.raises(ValueError):
        m.tensor_curves_in(m.tensor_curve(np.arange(4.0)))       # the other direction's curve is no TensorCurveIn
    with pytest.raises(ValueError):
        m.tensor_curve_in(np.zeros((2, 2)))
    for source, n_in in (("srgb", 4097), ("bt709", 4097), ("pq", 4097), ("linear", 0)):
        mix, q = m.Decoder.dcp_curves_in(709, source)
        assert (mix.nin, mix.chroma, q.in_.n, q.in_.root, q.out.n, q.out.root, q.in_mask, q.out_mask) == (3, 0, n_in, 0, 4097, 2, 7, 7)
        assert (q.out.x0, q.out.inv_dx) == (0.0, 4096.0) and list(q.gain) == [4095.0] * 4 and list(q.offset) == [0.0] * 4
    _, q = m.Decoder.dcp_curves_in(2020, "srgb", n=1025)
    assert (q.in_.n, q.in_.inv_dx, q.out.n, q.out.inv_dx) == (1025, 1024.0, 1025, 1024.0)
    # curve_table's default is the call it was
    assert np.array_equal(m.curve_table("pq_encode", 33), m.curve_table("pq_encode", 33, root=0))


def test_the_ten_refusals_in_their_order_with_a_null_context(L):
    ok = m.tensor_spec("float16")
    f = frame("yuv420p", 20, 10)                             # C = 3
    good = lambda **kw: m.tensor_curves_in(ramp(), ramp(4097, 2), **kw)
    for q in (good(), m.tensor_curves_in(ramp(2), None), m.tensor_curves_in(None, ramp(2, 3))):
        assert frames_call(L, ok, ones(), q, [f]) == ENOSYS  # valid arguments, no context
        assert enc_call(L, ok, ones(), q) == ENOSYS

    def broken(what):
        q = good()
        tab = np.arange(16, dtype=np.float32)
        if what == "both none":
            q = m.tensor_curves_in(None, None)
        elif what in ("n 1", "n 4098", "n -1"):
            q.out.n = int(what[2:])
        elif what == "n 4098 with a bad root and no table":  # 3 before 4 and 5
            q.in_.n, q.in_.root, q.in_.t = 4098, 9, None
        elif what in ("root 4", "root -1"):
            q.out.root = int(what[5:])
        elif what == "root 4 without a table":               # 4 before 5: the root is refused before the pointer is looked at
            q.in_.root, q.in_.t = 4, None
        elif what == "no table":
            q.out.t = None
        elif what in ("x0 nan", "x0 inf"):
            q.in_.x0 = float(what[3:])
        elif what in ("inv nan", "inv inf", "inv 0", "inv -1"):
            q.out.inv_dx = float(what[4:])
        elif what in ("entry nan", "entry inf", "entry big"):
            tab[7] = {"nan": math.nan, "inf": -math.inf, "big": 2.0 ** 101}[what[6:]]
            q = m.tensor_curves_in(m.tensor_curve_in(tab), ramp(4097))
        elif what == "in_mask":
            q.in_mask = 4                                    # K = 2 below
        elif what == "out_mask":
            q.out_mask = 8
        elif what == "gain":
            q.gain[2] = math.inf
        elif what == "offset":
            q.offset[0] = math.nan
        return q

    every = ["both none", "n 1", "n 4098", "n -1", "n 4098 with a bad root and no table", "root 4", "root -1", "root 4 without a table", "no table",
             "x0 nan", "x0 inf", "inv nan", "inv inf", "inv 0", "inv -1", "entry nan", "entry inf", "entry big", "in_mask", "out_mask", "gain", "offset"]
    pal = frame("pal8", 20, 10)
    other = frame("yuv420p", 22, 10)
    for what in every:
        q = broken(what)
        mix = ones(3, 2) if what == "in_mask" else ones()
        if what == "in_mask":
            q.in_mask = 4
        assert frames_call(L, ok, mix, q, [f]) == EINVAL, what
        assert enc_call(L, ok, mix, q) == EINVAL, what
        # behind the layout and the mix, in front of the frames and the tensor's size
        assert frames_call(L, ok, mix, q, [pal]) == PATCHWELCOME, what
        assert enc_call(L, ok, mix, q, "pal8") == PATCHWELCOME, what
        assert frames_call(L, ok, mix, q, [f, other]) == EINVAL and frames_call(L, ok, mix, q, [f], src_bytes=1) == EINVAL, what
    # 1: curves without a mix, whatever the curves hold; the spec's scale is then not reached
    nan_scale = m.tensor_spec("float16")
    nan_scale.scale[0] = math.nan
    for q in (good(), broken("n 4098 with a bad root and no table")):
        assert frames_call(L, ok, None, q, [f]) == EINVAL and enc_call(L, ok, None, q) == EINVAL
        assert frames_call(L, nan_scale, None, q, [f]) == EINVAL
    # the mix itself is refused first
    bad = ones()
    bad.nin = 5
    assert frames_call(L, ok, bad, good(), [f]) == EINVAL and enc_call(L, ok, bad, good()) == EINVAL
    # 2^100 itself is allowed; entries that are not read may hold anything
    edge = np.arange(16, dtype=np.float32)
    edge[3], edge[4] = 2.0 ** 100, -2.0 ** 100
    assert frames_call(L, ok, ones(), m.tensor_curves_in(m.tensor_curve_in(edge), None), [f]) == ENOSYS
    q = m.tensor_curves_in(ramp(), None, in_mask=3)
    q.out.root, q.out.x0, q.out.inv_dx, q.out.t = 77, math.nan, -1.0, ctypes.cast(8, ctypes.POINTER(ctypes.c_float))
    q.gain[3], q.offset[3] = math.nan, math.inf
    assert frames_call(L, ok, ones(3, 2), q, [f]) == ENOSYS and enc_call(L, ok, ones(3, 2), q) == ENOSYS
    q.offset[2] = math.nan                                   # an offset at C - 1 is read
    assert frames_call(L, ok, ones(3, 2), q, [f]) == EINVAL and enc_call(L, ok, ones(3, 2), q) == EINVAL
    # the masks are held against K (in) and C (out): gray from three channels
    g = frame("gray", 20, 10)
    assert frames_call(L, ok, ones(1, 3), m.tensor_curves_in(ramp(), ramp(), 7, 1), [g]) == ENOSYS
    assert frames_call(L, ok, ones(1, 3), m.tensor_curves_in(ramp(), ramp(), 7, 2), [g]) == EINVAL
    assert frames_call(L, ok, ones(1, 3), m.tensor_curves_in(ramp(), ramp(), 8, 1), [g]) == EINVAL
    # behind the curves: the tensor's size and alignment, as the mix call has them
    assert enc_call(L, ok, ones(), good(), src_bytes=3 * 20 * 10 * 2 - 1) == EINVAL
    assert enc_call(L, ok, ones(), good(), src_bytes=3 * 20 * 10 * 2) == ENOSYS
    assert enc_call(L, ok, ones(), good(), src=0x1001) == EINVAL
    # the encoder's own limit stays: XYZ12 is not a layout it takes
    assert m.Encoder.bound(64, 48, "xyz12le", 12) == 0


def test_null_curves_answer_what_the_mix_calls_answer(L):
    ok, f = m.tensor_spec("float16"), frame("yuv420p", 20, 10)
    bad_mix = ones()
    bad_mix.chroma = 3
    nan_spec = m.tensor_spec("float16")
    nan_spec.bias[1] = math.nan
    for spec, mix, frames, kw in ((ok, ones(), [f], {}), (ok, None, [f], {}), (ok, bad_mix, [f], {}), (nan_spec, None, [f], {}), (nan_spec, ones(), [f], {}),
                                  (ok, ones(), [frame("pal8", 20, 10)], {}), (ok, ones(), [f], dict(src_bytes=5)), (ok, ones(), [f], dict(src=0x1001)),
                                  (ok, ones(3, 4), [f, f], {}), (None, ones(), [f], {})):
        assert frames_call(L, spec, mix, None, frames, **kw) == mix_frames_call(L, spec, mix, frames, **kw)
    for spec, mix, kw in ((ok, ones(), {}), (ok, None, {}), (ok, bad_mix, {}), (nan_spec, None, {}), (nan_spec, ones(), {}), (ok, ones(), dict(fmt="pal8")),
                          (ok, ones(), dict(src_bytes=5)), (ok, ones(), dict(w=0)), (ok, ones(), dict(fmt="xyz12le", bits=12)), (None, ones(), {})):
        assert enc_call(L, spec, mix, None, **kw) == mix_enc_call(L, spec, mix, **kw)


def ulps(got, want64):
    """the distance of float32 values from float64 ones in units of the float32 spacing at the wanted value"""
    want64 = np.asarray(want64, np.float64)
    spacing = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / spacing


def test_curve_fill_root_is_the_function_in_double(L):
    for kind in cvm.KINDS:
        for root in (0, 1, 2, 3):
            for n, lo, hi in ((2, 0.0, 1.0), (17, 0.0, 1.0), (1025, 0.0, 1.0), (4097, 0.0, 1.0), (33, 0.25, 1.5)):
                param = 1.0 / 2.6 if kind == "power" else 0.0
                got = m.curve_table(kind, n, lo, hi, param, root=root)
                assert float(ulps(got, cim.fill_root(kind, n, lo, hi, param, root)).max()) <= 1.0, (kind, root, n)
                if root == 0:
                    assert np.array_equal(got, m.curve_table(kind, n, lo, hi, param))
    # the ends of the DCI encode: knot 0 is 0, the last knot is 1
    t = m.curve_table("power", 4097, 0.0, 1.0, 1.0 / 2.6, root=2)
    assert t[0] == 0.0 and t[-1] == 1.0 and np.all(np.diff(t) > 0)
    buf = (ctypes.c_float * 8)()
    call = lambda *a: L.htj2k_tensor_curve_fill_root(*a)
    assert call(buf, 8, 0, 2.6, 0.0, 1.0, 2) == 0
    for args in ((None, 8, 0, 2.6, 0.0, 1.0, 2), (buf, 1, 0, 2.6, 0.0, 1.0, 2), (buf, 8, 7, 2.6, 0.0, 1.0, 2), (buf, 8, -1, 2.6, 0.0, 1.0, 2),
                 (buf, 8, 0, math.nan, 0.0, 1.0, 2), (buf, 8, 0, 2.6, math.inf, 1.0, 2), (buf, 8, 0, 2.6, 1.0, 1.0, 2), (buf, 8, 0, 2.6, 0.0, 1.0, 4),
                 (buf, 8, 0, 2.6, 0.0, 1.0, -1), (None, 8, 0, 2.6, 0.0, 1.0, 0), (buf, 8, 0, 2.6, 1.0, 0.0, 0)):
        assert call(*args) == EINVAL, args


def test_mix_in_xyz_is_the_primary_matrix_in_double(L):
    for primaries in (709, 2020, P3):
        for scale in (1.0, 48.0 / 52.37, 100.0):
            mix = m.Decoder.xyz_mix_in(primaries, scale)
            nin, chroma, mat, b = tmi.unpack(mix)
            assert (nin, chroma) == (3, 0) and not b.any() and not mat[3].any() and not mat[:, 3].any()
            assert float(ulps(mat[:3, :3], cim.mix_in_xyz(primaries, scale)).max()) <= 1.0, (primaries, scale)
            back = m.Decoder.xyz_mix(primaries, 1.0 / scale)
            inv = np.array([[back.m[k][c] for c in range(3)] for k in range(3)], np.float64)
            assert np.abs(inv @ mat[:3, :3].astype(np.float64) - np.eye(3)).max() <= 1e-6, (primaries, scale)
    # Y of white is the scale: the rows' sums are the white point
    mat = tmi.unpack(m.Decoder.xyz_mix_in(709, 1.0))[2]
    assert abs(float(mat[1, :3].astype(np.float64).sum()) - 1.0) < 1e-6
    mix = m.TensorMixIn()
    for args in ((None, 709, 1.0), (ctypes.byref(mix), 601, 1.0), (ctypes.byref(mix), 709, math.nan), (ctypes.byref(mix), 709, math.inf)):
        assert L.htj2k_tensor_mix_in_xyz(*args) == EINVAL, args[1:]


def special_values():
    return [np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, -1e-30, 1e-45, 1e-40, 1.1754944e-38, 6e-8, 0.5, 1.0, 1.0000001, 2.0, 65504.0, 3e38, 0.25, 1e-4]


def random_curves(rng, K, nc, roots=(None, None), n=(17, 9)):
    """curves whose tables are not monotone and whose ranges the pictures overshoot at both ends"""
    def one(root, knots, lo, hi, scale):
        if root is None:
            return None
        tab = (rng.uniform(-0.2, 1.0, knots) * scale).astype(np.float32)
        return tab, float(np.float32(lo)), float(np.float32((knots - 1) / (hi - lo))), root
    return {"in": one(roots[0], n[0], 0.05, 0.9, 1.0), "out": one(roots[1], n[1], 0.1, 0.8, 1.0),
            "in_mask": int(rng.integers(1, 1 << K)), "out_mask": int(rng.integers(1, 1 << nc)),
            "gain": rng.uniform(100.0, 300.0, 4).astype(np.float32), "offset": rng.uniform(-20.0, 20.0, 4).astype(np.float32)}


def struct_of(q):
    """a TensorCurvesIn from the model's dict"""
    q = cim.unpack(q)

    def one(cv):
        return None if cv is None else m.tensor_curve_in(cv[0], cv[1], cv[2], cv[3])
    return m.tensor_curves_in(one(q["in"]), one(q["out"]), q["in_mask"], q["out_mask"], q["gain"], q["offset"])


def test_the_struct_round_trips_through_the_model():
    rng = np.random.default_rng(2)
    q = random_curves(rng, 3, 3, (2, 0))
    back = cim.unpack(struct_of(q))
    for key in ("in", "out"):
        assert np.array_equal(back[key][0], q[key][0]) and back[key][1:] == q[key][1:]
    assert back["in_mask"] == q["in_mask"] and np.array_equal(back["gain"], q["gain"]) and np.array_equal(back["offset"], q["offset"])


def test_model_matches_the_torch_chain_on_the_cpu():
    rng = np.random.default_rng(3)
    sv = np.array(special_values(), np.float32)
    for fmt, bits in (("rgb48le", 12), ("rgb24", 8), ("gray", 8), ("yuv444p12le", 12), ("rgba", 8)):
        nc = cm.LAYOUTS[fmt][0]
        for ri, roots in enumerate(((0, 0), (1, 2), (3, None), (None, 3), (2, 1), (0, 3))):
            for dtype, tdt in (("float32", torch.float32), ("float16", torch.float16), ("bfloat16", torch.bfloat16)):
                K = 1 + (ri + nc) % 4
                v = rng.uniform(-0.1, 1.1, (2, K, 5, len(sv))).astype(np.float32)
                v[0, :, 0, :] = sv
                v[1, K - 1, 2, :] = sv[::-1]
                t = torch.from_numpy(v).to(tdt)
                tbits = t.view(torch.int16 if dtype != "float32" else torch.int32).numpy().view(np.uint16 if dtype != "float32" else np.uint32)
                mix = (rng.uniform(-0.3, 1.0, (nc, K)).astype(np.float32), rng.uniform(-0.1, 0.1, nc).astype(np.float32), ri % 2)
                q = random_curves(rng, K, nc, roots)
                want = cim.frames(tbits, fmt, bits, mix, q, dtype, "NCHW")
                got = cim.torch_chain(t, mix, q, bits, nc, cm.shift(fmt, bits)).numpy()
                for i in range(2):
                    comps = want[i] if cm.LAYOUTS[fmt][1] else [want[i][0].reshape(5, len(sv), nc)[:, :, c] for c in range(nc)]
                    for c in range(nc):
                        assert np.array_equal(comps[c].astype(np.int64), got[i, c]), (fmt, roots, dtype, i, c)


def code_round_trip(n, root, codes=None):
    """how many of the 4096 twelve-bit codes do not come back from their linear values (code / 4095) ^ 2.6 through a
    table of the DCI encode with n knots uniform in the 2^root-th root of x, and the largest error in 12-bit steps over the
    codes and two million dense arguments"""
    codes = np.arange(4096) if codes is None else codes
    tab = m.curve_table("power", n, 0.0, 1.0, 1.0 / 2.6, root=root)
    x = ((codes / 4095.0) ** 2.6).astype(np.float32)
    back = np.rint((cim.root_eval(x, tab, 0.0, float(n - 1), root) * np.float32(4095.0)).astype(np.float32))
    dense = np.concatenate([x, np.linspace(0.0, 1.0, 2000000).astype(np.float32)])
    err = np.abs(4095.0 * cim.root_eval(dense, tab, 0.0, float(n - 1), root).astype(np.float64) - 4095.0 * dense.astype(np.float64) ** (1.0 / 2.6))
    return int(np.count_nonzero(back != codes)), float(err.max())


def test_why_a_curve_of_this_direction_has_a_root():
    """the table of the header and of DESIGN.md 3.5: knots uniform in x lose codes whatever their number; uniform in the
    fourth root every code comes back"""
    rows = {}
    for n in (1025, 4097):
        for root in (0, 1, 2, 3):
            rows[n, root] = code_round_trip(n, root)
            print("DCI encode, %4d knots uniform in x^(1/%d): %4d of 4096 codes do not come back, max error %.4f steps"
                  % (n, 1 << root, rows[n, root][0], rows[n, root][1]))
    assert rows[4097, 0][0] > 0
    assert rows[4097, 2][0] == 0
    # PQ encode from linear light, 4097 knots: the largest error in 12-bit steps
    x = np.linspace(0.0, 1.0, 2000000).astype(np.float32)
    for root in (0, 2, 3):
        tab = m.curve_table("pq_encode", 4097, 0.0, 1.0, root=root)
        err = np.abs(4095.0 * cim.root_eval(x, tab, 0.0, 4096.0, root).astype(np.float64) - 4095.0 * cvm.function("pq_encode", x.astype(np.float64)))
        print("PQ encode, 4097 knots uniform in x^(1/%d): max error %.4f steps" % (1 << root, float(err.max())))


def in_gamut_triples(primaries, floor=20000, seed=7):
    """seeded X'Y'Z' triples whose decoded float32 linear R, G, B all lie in 0 .. 1, grey and near-grey ramps among them:
    (codes (3, N), their linear RGB, their sRGB-coded RGB), at least `floor` of them"""
    rng = np.random.default_rng(seed)
    mix, lin = m.Decoder.dcp_curves(primaries, "srgb")
    to_lin = m.tensor_curves(m.tensor_curve(lin.tables[0], 0.0, 1.0), None, 7, 7)
    # grey of every level: XYZ = L (0.9505, 1, 1.089) 48 / 52.37, so the codes are the level's code times a constant each
    white = (np.array([[0.9505], [1.0], [1.089]]) * 48.0 / 52.37) ** (1.0 / 2.6)
    grey = np.rint(np.arange(4096)[None, :] * white)
    near = [np.clip(grey + d, 0, 4095).astype(np.int64) for d in (0, 1, -1)]
    out, count = [], 0
    for block in near + [None] * 64:
        s = rng.integers(0, 4096, (3, 100000)) if block is None else block
        f = [s[c].astype(np.float32) for c in range(3)]
        rgb = np.stack(cvm.values(f, mix, to_lin))
        keep = np.all((rgb >= 0.0) & (rgb <= 1.0), axis=0)
        out.append((s[:, keep], rgb[:, keep], np.stack(cvm.values(f, mix, lin))[:, keep]))
        count += int(np.count_nonzero(keep)) if block is None else 0
        if block is None and count >= floor:
            break
    assert count >= floor, (primaries, count)
    return [np.concatenate([o[i] for o in out], axis=1) for i in range(3)]


@pytest.mark.parametrize("primaries", [709, 2020, P3])
def test_xyz_codes_come_back_through_linear_and_srgb_rgb(primaries):
    """X'Y'Z' -> RGB by the decode direction's model (dcp_curves), float32, linear and sRGB-coded -> X'Y'Z' by this
    direction's (dcp_curves_in): every in-gamut triple returns exactly"""
    codes, linear, srgb = in_gamut_triples(primaries)
    print("primaries %d: %d in-gamut triples" % (primaries, codes.shape[1]))
    for source, rgb in (("linear", linear), ("srgb", srgb)):
        mix, q = m.Decoder.dcp_curves_in(primaries, source)
        chw = [rgb[k].reshape(1, -1) for k in range(3)]
        for c in range(3):
            back = cim.component_samples(chw, "rgb48le", 12, mix, q, c).reshape(-1)
            bad = np.flatnonzero(back != codes[c])
            assert bad.size == 0, (primaries, source, c, bad.size, codes[:, bad[:4]].T.tolist(), back[bad[:4]].tolist())


def test_the_identity_curve_gives_the_mix_calls_bytes():
    rng = np.random.default_rng(5)
    ident = {"in": (np.array([0.0, 1.0], np.float32), 0.0, 1.0, 0), "gain": 1.0, "offset": 0.0}
    for fmt, bits in (("yuv420p", 8), ("yuv422p10le", 10), ("rgb48le", 12), ("yuv410p", 8), ("ya8", 8), ("xyz12le", 12)):
        nc = cm.LAYOUTS[fmt][0]
        for dtype, tdt in (("float32", torch.float32), ("float16", torch.float16), ("bfloat16", torch.bfloat16)):
            for layout, chroma in (("NCHW", 0), ("NHWC", 1)):
                K = int(rng.integers(1, 5))
                v = rng.uniform(0.0, 1.0, (2, K, 5, 7)).astype(np.float32)
                v[0, 0, 0, :4] = [0.0, 1.0, -0.0, 1e-40]
                t = torch.from_numpy(v if layout == "NCHW" else np.ascontiguousarray(v.transpose(0, 2, 3, 1))).to(tdt)
                tbits = t.view(torch.int16 if dtype != "float32" else torch.int32).numpy().view(np.uint16 if dtype != "float32" else np.uint32)
                mix = ((rng.uniform(-0.2, 1.0, (nc, K)) * ((1 << bits) - 1)).astype(np.float32), rng.uniform(-2, 20, nc).astype(np.float32), chroma)
                q = dict(ident, in_mask=(1 << K) - 1)
                a, b = cim.frames(tbits, fmt, bits, mix, q, dtype, layout), tmi.frames(tbits, fmt, bits, mix, dtype, layout)
                assert all(np.array_equal(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb)), (fmt, dtype, layout, K)
