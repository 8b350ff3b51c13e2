"""ffmpeg-ht_amd -- thin Python (ctypes) binding of the MI355X-native HTJ2K decode library.

The product is the C-ABI shared library `libhtj2k_amd.so` (include/htj2k_amd.h): host C
parser + HIP kernels behind the plugin surface of FFmpeg's `ff_jpeg2000_decoder`
(libavcodec/jpeg2000dec.c:2926-2939).  This module only loads it for tests, bench.py and
scripting; it contains no decoding logic and NO fallback: if the library or a GPU is
missing, construction fails loudly.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HTJ2K_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhtj2k_amd.so")   # HTJ2K_LIB: A/B builds side by side (tools/)

ERR_NAMES = {-0x41444E49: "INVALIDDATA", -0x45574150: "PATCHWELCOME", -0x21475542: "BUG", -0x20545845: "EXTERNAL",
             -12: "ENOMEM", -22: "EINVAL", -38: "ENOSYS"}
DWT97, DWT53, DWT97_INT = 0, 1, 2

PIX_NAMES = ["pal8", "rgb24", "rgba", "rgb48le", "rgba64le", "gray", "ya8", "gray16le", "ya16le",
             "yuv410p", "yuv411p", "yuva420p", "yuv420p", "yuv422p", "yuva422p", "yuv440p", "yuv444p", "yuva444p",
             "yuv420p9le", "yuv422p9le", "yuv444p9le", "yuva420p9le", "yuva422p9le", "yuva444p9le",
             "yuv420p10le", "yuv422p10le", "yuv444p10le", "yuva420p10le", "yuva422p10le", "yuva444p10le",
             "yuv420p12le", "yuv422p12le", "yuv444p12le", "yuv420p14le", "yuv422p14le", "yuv444p14le",
             "yuv420p16le", "yuv422p16le", "yuv444p16le", "yuva420p16le", "yuva422p16le", "yuva444p16le", "xyz12le"]


class Htj2kError(RuntimeError):
    def __init__(self, code, what=""):
        super().__init__("%s failed: %s (%d)" % (what or "htj2k", ERR_NAMES.get(code, "?"), code))
        self.code = code


class Opts(ctypes.Structure):
    _fields_ = [("bitexact", ctypes.c_int), ("reduction_factor", ctypes.c_int), ("max_pixels", ctypes.c_int64),
                ("strict", ctypes.c_int), ("device_id", ctypes.c_int), ("frames_in_flight", ctypes.c_int),
                ("req_pix_fmt", ctypes.c_int)]


class Info(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("pix_fmt", ctypes.c_int),
                ("bits_per_raw_sample", ctypes.c_int), ("profile", ctypes.c_int), ("lossless", ctypes.c_int),
                ("sar_num", ctypes.c_int), ("sar_den", ctypes.c_int), ("ncomponents", ctypes.c_int),
                ("is_ht", ctypes.c_int), ("nplanes", ctypes.c_int), ("plane_width", ctypes.c_int * 4),
                ("plane_height", ctypes.c_int * 4), ("plane_bytes_per_sample", ctypes.c_int * 4),
                ("has_palette", ctypes.c_int)]


class Frame(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p * 4), ("linesize", ctypes.c_int * 4), ("width", ctypes.c_int),
                ("height", ctypes.c_int), ("pix_fmt", ctypes.c_int)]


class Stats(ctypes.Structure):
    _fields_ = [("n_codeblocks", ctypes.c_int), ("n_block_errors", ctypes.c_int), ("ms_parse", ctypes.c_float),
                ("ms_h2d", ctypes.c_float), ("ms_kernels", ctypes.c_float), ("ms_d2h", ctypes.c_float),
                ("ms_ht", ctypes.c_float), ("ms_idwt", ctypes.c_float), ("ms_pack", ctypes.c_float)]


class FrameDiff(ctypes.Structure):
    """struct htj2k_frame_diff (include/htj2k_amd.h)"""
    _fields_ = [("sse", ctypes.c_uint64 * 4), ("ndiff", ctypes.c_uint64 * 4), ("nsamples", ctypes.c_uint64 * 4),
                ("max_abs", ctypes.c_uint32 * 4), ("psnr", ctypes.c_double)]

    def as_dict(self):
        """sse / ndiff / nsamples / max_abs as lists of four Python ints, psnr as a float"""
        d = {f: [int(v) for v in getattr(self, f)] for f in ("sse", "ndiff", "nsamples", "max_abs")}
        d["psnr"] = float(self.psnr)
        return d


class FrameSsim(ctypes.Structure):
    """struct htj2k_frame_ssim (include/htj2k_amd.h)"""
    _fields_ = [("q32", ctypes.c_int64 * 4), ("nwin", ctypes.c_uint64 * 4), ("ssim", ctypes.c_double * 4),
                ("all", ctypes.c_double)]

    def as_dict(self):
        """q32 / nwin as lists of four Python ints, ssim as a list of four floats (NaN where nwin is 0), all as a float"""
        return {"q32": [int(v) for v in self.q32], "nwin": [int(v) for v in self.nwin],
                "ssim": [float(v) for v in self.ssim], "all": float(self.all)}


class FrameHash(ctypes.Structure):
    """struct htj2k_frame_hash (include/htj2k_amd.h)"""
    _fields_ = [("adler32", ctypes.c_uint32), ("plane_adler32", ctypes.c_uint32 * 4), ("nbytes", ctypes.c_uint64)]

    def as_dict(self):
        """adler32 (what a framecrc line prints) and nbytes as Python ints, plane_adler32 as a list of four"""
        return {"adler32": int(self.adler32), "plane_adler32": [int(v) for v in self.plane_adler32], "nbytes": int(self.nbytes)}


class TensorSpec(ctypes.Structure):
    """struct htj2k_tensor_spec (include/htj2k_amd.h): dtype 0 / 1 / 2 = float32 / float16 / bfloat16, layout 0 / 1 =
    NCHW / NHWC, out_w x out_h (0 x 0: the frames' own size), scale and bias per component"""
    _fields_ = [("dtype", ctypes.c_int), ("layout", ctypes.c_int), ("out_w", ctypes.c_int), ("out_h", ctypes.c_int),
                ("scale", ctypes.c_float * 4), ("bias", ctypes.c_float * 4)]


class TensorMix(ctypes.Structure):
    """struct htj2k_tensor_mix (include/htj2k_amd.h): nout = K channels, m[k][c] the weight of the layout's component c in
    channel k, b[k] added last"""
    _fields_ = [("nout", ctypes.c_int), ("m", (ctypes.c_float * 4) * 4), ("b", ctypes.c_float * 4)]


assert ctypes.sizeof(TensorMix) == 84


def tensor_mix(m, b=None):
    """a TensorMix from a K x C matrix (K, C in 1 .. 4; its shape gives K) and K offsets (None: zeros).  Values are
    rounded to float32 once; signed zeros are kept"""
    a = np.asarray(m, np.float32)
    if a.ndim != 2 or not (1 <= a.shape[0] <= 4 and 1 <= a.shape[1] <= 4):
        raise ValueError("m: a K x C matrix, K and C in 1 .. 4")
    o = np.zeros(a.shape[0], np.float32) if b is None else np.asarray(b, np.float32)
    if o.shape != (a.shape[0],):
        raise ValueError("b: one offset per row of m")
    mix = TensorMix()
    mix.nout = a.shape[0]
    full, off = np.zeros((4, 4), np.float32), np.zeros(4, np.float32)
    full[:a.shape[0], :a.shape[1]], off[:a.shape[0]] = a, o
    ctypes.memmove(mix.m, full.ctypes.data, 64)
    ctypes.memmove(mix.b, off.ctypes.data, 16)
    return mix


def _mix_p(mix):
    """what to pass for a mix: NULL, or the struct's address"""
    if mix is None:
        return None
    if not isinstance(mix, TensorMix):
        raise ValueError("mix: a TensorMix (tensor_mix, Decoder.ycbcr_mix) or None")
    return ctypes.byref(mix)


class TensorCurve(ctypes.Structure):
    """struct htj2k_tensor_curve (include/htj2k_amd.h): n knots t[j] at x0 + j / inv_dx; n 0: no curve.  `table` keeps
    the array that t points into alive"""
    _fields_ = [("n", ctypes.c_int), ("x0", ctypes.c_float), ("inv_dx", ctypes.c_float), ("t", ctypes.POINTER(ctypes.c_float))]
    table = None


class TensorCurves(ctypes.Structure):
    """struct htj2k_tensor_curves (include/htj2k_amd.h): the curve before the mix and the one after it, the components
    and channels they apply to, and gain[k], offset[k] applied last.  `tables` keeps both curves' arrays alive"""
    _fields_ = [("in_", TensorCurve), ("out", TensorCurve), ("in_mask", ctypes.c_uint32), ("out_mask", ctypes.c_uint32),
                ("gain", ctypes.c_float * 4), ("offset", ctypes.c_float * 4)]
    tables = ()


assert ctypes.sizeof(TensorCurve) == 24 and ctypes.sizeof(TensorCurves) == 88
CURVE_KINDS = ["power", "srgb_encode", "srgb_decode", "bt709_encode", "bt709_decode", "pq_encode", "pq_decode"]
PRIMARIES_P3D65 = 3


def tensor_curve(table, x0=0.0, inv_dx=1.0):
    """a TensorCurve from its knots (a sequence of 2 .. 4097 floats, rounded to float32 once): knot j is the curve's value
    at x0 + j / inv_dx, and between knots the curve is interpolated linearly (the header has the arithmetic)"""
    a = np.ascontiguousarray(table, np.float32)
    if a.ndim != 1:
        raise ValueError("table: a sequence of knots")
    cv = TensorCurve()
    cv.n, cv.x0, cv.inv_dx = a.shape[0], x0, inv_dx
    cv.t = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    cv.table = a
    return cv


def tensor_curves(in_=None, out=None, in_mask=None, out_mask=None, gain=None, offset=None):
    """a TensorCurves from the curve before the mix and the one after it (TensorCurve or None), the masks of the components
    and channels they apply to (None: all but index 3), and per-channel gain (None: 1) and offset (None: 0), one number
    or up to four"""
    q = TensorCurves()
    for name, cv in (("in_", in_), ("out", out)):
        if cv is None:
            continue
        if not isinstance(cv, TensorCurve):
            raise ValueError("a curve: a TensorCurve (tensor_curve) or None")
        dst = getattr(q, name)
        dst.n, dst.x0, dst.inv_dx, dst.t = cv.n, cv.x0, cv.inv_dx, cv.t
    q.tables = (None if in_ is None else in_.table, None if out is None else out.table)
    q.in_mask = 7 if in_mask is None else int(in_mask)
    q.out_mask = 7 if out_mask is None else int(out_mask)
    for name, v, d in (("gain", gain, 1.0), ("offset", offset, 0.0)):
        a = np.full(4, d, np.float32)
        if v is not None:
            v = np.atleast_1d(np.asarray(v, np.float32))
            if v.ndim != 1 or v.shape[0] > 4:
                raise ValueError("%s: one number, or up to four" % name)
            a[:v.shape[0] if v.shape[0] > 1 else 4] = v
        ctypes.memmove(getattr(q, name), a.ctypes.data, 16)
    return q


def _curve_kind(kind):
    """HTJ2K_CURVE_* from its name; a number passes through (the library checks it)"""
    if isinstance(kind, str):
        if kind not in CURVE_KINDS:
            raise ValueError("curve kind %r: one of %s" % (kind, ", ".join(CURVE_KINDS)))
        return CURVE_KINDS.index(kind)
    return int(kind)


def curve_table(kind, n, lo=0.0, hi=1.0, param=0.0, root=0):
    """htj2k_tensor_curve_fill (no context, no device): n knots of the transfer function `kind` (CURVE_KINDS) over
    lo .. hi as a float32 array; param is the exponent of "power".  root (1 .. 3, for tensor_curve_in): lo .. hi is the
    range of the argument's 2^root-th root, and knot j holds the function at y_j ^ (2^root) (htj2k_tensor_curve_fill_root)"""
    t = np.zeros(max(int(n), 0), np.float32)
    L = load_library()
    if root != 0:
        L.htj2k_tensor_curve_fill_root.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                                   ctypes.c_double, ctypes.c_int]
        _check(L.htj2k_tensor_curve_fill_root(ctypes.c_void_p(t.ctypes.data if t.size else None), int(n), _curve_kind(kind), float(param),
                                              float(lo), float(hi), int(root)), "htj2k_tensor_curve_fill_root")
        return t
    L.htj2k_tensor_curve_fill.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    _check(L.htj2k_tensor_curve_fill(ctypes.c_void_p(t.ctypes.data if t.size else None), int(n), _curve_kind(kind), float(param),
                                     float(lo), float(hi)), "htj2k_tensor_curve_fill")
    return t


def _curves_p(curves, mix):
    """what to pass for curves: NULL, or the struct's address; curves need a mix"""
    if curves is None:
        return None
    if not isinstance(curves, TensorCurves):
        raise ValueError("curves: a TensorCurves (tensor_curves, Decoder.dcp_curves) or None")
    if mix is None:
        raise ValueError("curves: a mix is required (mix=)")
    return ctypes.byref(curves)


class TensorMixIn(ctypes.Structure):
    """struct htj2k_tensor_mix_in (include/htj2k_amd.h): nin = K channels of the tensor, chroma 0 / 1 = co-sited / box,
    m[c][k] the weight of tensor channel k in the layout's component c, b[c] added last"""
    _fields_ = [("nin", ctypes.c_int), ("chroma", ctypes.c_int), ("m", (ctypes.c_float * 4) * 4), ("b", ctypes.c_float * 4)]


assert ctypes.sizeof(TensorMixIn) == 88
CHROMA_RULES = ["cosited", "box"]


def _chroma(chroma):
    """HTJ2K_CHROMA_* from its name; a number passes through (the library checks it)"""
    if isinstance(chroma, str):
        if chroma not in CHROMA_RULES:
            raise ValueError("chroma %r: cosited or box" % (chroma,))
        return CHROMA_RULES.index(chroma)
    return int(chroma)


def tensor_mix_in(m, b=None, chroma="cosited"):
    """a TensorMixIn from a C x K matrix (C, K in 1 .. 4; its columns give K, the channels of the tensor) and C offsets
    (None: zeros).  Values are rounded to float32 once; signed zeros are kept"""
    a = np.asarray(m, np.float32)
    if a.ndim != 2 or not (1 <= a.shape[0] <= 4 and 1 <= a.shape[1] <= 4):
        raise ValueError("m: a C x K matrix, C and K in 1 .. 4")
    o = np.zeros(a.shape[0], np.float32) if b is None else np.asarray(b, np.float32)
    if o.shape != (a.shape[0],):
        raise ValueError("b: one offset per row of m")
    mix = TensorMixIn()
    mix.nin, mix.chroma = a.shape[1], _chroma(chroma)
    full, off = np.zeros((4, 4), np.float32), np.zeros(4, np.float32)
    full[:a.shape[0], :a.shape[1]], off[:a.shape[0]] = a, o
    ctypes.memmove(mix.m, full.ctypes.data, 64)
    ctypes.memmove(mix.b, off.ctypes.data, 16)
    return mix


def _mix_in_p(mix):
    """what to pass for a mix on the way in: NULL, or the struct's address"""
    if mix is None:
        return None
    if not isinstance(mix, TensorMixIn):
        raise ValueError("mix: a TensorMixIn (tensor_mix_in, Decoder.rgb_mix_in) or None")
    return ctypes.byref(mix)


class TensorCurveIn(ctypes.Structure):
    """struct htj2k_tensor_curve_in (include/htj2k_amd.h): n knots t[j] at x0 + j / inv_dx of the argument square-rooted
    `root` times; n 0: no curve.  `table` keeps the array that t points into alive"""
    _fields_ = [("n", ctypes.c_int), ("root", ctypes.c_int), ("x0", ctypes.c_float), ("inv_dx", ctypes.c_float),
                ("t", ctypes.POINTER(ctypes.c_float))]
    table = None


class TensorCurvesIn(ctypes.Structure):
    """struct htj2k_tensor_curves_in (include/htj2k_amd.h): the curve before the mix on the way in and the one after it,
    the tensor channels and components they apply to, and gain[c], offset[c] applied last.  `tables` keeps both curves'
    arrays alive; `auto_masks` says which of the two masks were left to the call (tensor_curves_in)"""
    _fields_ = [("in_", TensorCurveIn), ("out", TensorCurveIn), ("in_mask", ctypes.c_uint32), ("out_mask", ctypes.c_uint32),
                ("gain", ctypes.c_float * 4), ("offset", ctypes.c_float * 4)]
    tables = ()
    auto_masks = (False, False)


assert ctypes.sizeof(TensorCurveIn) == 24 and ctypes.sizeof(TensorCurvesIn) == 88


def tensor_curve_in(table, x0=0.0, inv_dx=1.0, root=0):
    """a TensorCurveIn from its knots (a sequence of 2 .. 4097 floats, rounded to float32 once): the argument is clamped
    below at 0 and square-rooted `root` times (0 .. 3; 0: taken as it is), knot j is the curve's value where that equals
    x0 + j / inv_dx, and between knots the curve is interpolated linearly (the header has the arithmetic)"""
    a = np.ascontiguousarray(table, np.float32)
    if a.ndim != 1:
        raise ValueError("table: a sequence of knots")
    cv = TensorCurveIn()
    cv.n, cv.root, cv.x0, cv.inv_dx = a.shape[0], int(root), x0, inv_dx
    cv.t = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    cv.table = a
    return cv


def tensor_curves_in(in_=None, out=None, in_mask=None, out_mask=None, gain=None, offset=None):
    """a TensorCurvesIn from the curve before the mix and the one after it (TensorCurveIn or None), the masks of the tensor
    channels and of the components they apply to, and per-component gain (None: 1) and offset (None: 0), one number or up
    to four.  A mask of None is all but index 3: the struct holds 7, and Decoder.from_tensor and Encoder.encode_tensor,
    which know the mix's K and the layout's C, pass the bits below K (or C) of it, so that the default is valid for a
    tensor of one or two channels and for gray or ya8.  A mask given as a number is passed as it is"""
    q = TensorCurvesIn()
    for name, cv in (("in_", in_), ("out", out)):
        if cv is None:
            continue
        if not isinstance(cv, TensorCurveIn):
            raise ValueError("a curve: a TensorCurveIn (tensor_curve_in) or None")
        dst = getattr(q, name)
        dst.n, dst.root, dst.x0, dst.inv_dx, dst.t = cv.n, cv.root, cv.x0, cv.inv_dx, cv.t
    q.tables = (None if in_ is None else in_.table, None if out is None else out.table)
    q.in_mask = 7 if in_mask is None else int(in_mask)
    q.out_mask = 7 if out_mask is None else int(out_mask)
    q.auto_masks = (in_mask is None, out_mask is None)
    for name, v, d in (("gain", gain, 1.0), ("offset", offset, 0.0)):
        a = np.full(4, d, np.float32)
        if v is not None:
            v = np.atleast_1d(np.asarray(v, np.float32))
            if v.ndim != 1 or v.shape[0] > 4:
                raise ValueError("%s: one number, or up to four" % name)
            a[:v.shape[0] if v.shape[0] > 1 else 4] = v
        ctypes.memmove(getattr(q, name), a.ctypes.data, 16)
    return q


def _curves_in_p(curves, mix, pix_fmt, bits):
    """what to pass for curves on the way in: NULL, or the struct's address (of a copy whose default masks are cut to
    the mix's K channels and the layout's C components); curves need a mix"""
    if curves is None:
        return None
    if not isinstance(curves, TensorCurvesIn):
        raise ValueError("curves: a TensorCurvesIn (tensor_curves_in, Decoder.dcp_curves_in) or None")
    if mix is None:
        raise ValueError("curves: a mix is required (mix=)")
    if not any(curves.auto_masks):
        return ctypes.byref(curves)
    q = TensorCurvesIn.from_buffer_copy(curves)
    q.tables = curves.tables
    if curves.auto_masks[0]:
        q.in_mask = curves.in_mask & ((1 << max(0, min(int(mix.nin), 4))) - 1)
    if curves.auto_masks[1]:
        ncomp = Decoder.tensor_image_size(pix_fmt, 1, 1, bits, tensor_spec())[0]
        q.out_mask = curves.out_mask & ((1 << ncomp) - 1)
    return ctypes.byref(q)


TENSOR_DTYPES = ["float32", "float16", "bfloat16"]
TENSOR_LAYOUTS = ["NCHW", "NHWC"]


def tensor_spec(dtype="float16", layout="NCHW", size=None, scale=None, bias=None):
    """a TensorSpec from a dtype (its name, or a torch / numpy dtype whose name ends in it), "NCHW" / "NHWC", size =
    (out_w, out_h) or None for the frames' own, and scale / bias as one number for all components or up to four"""
    s = TensorSpec()
    name = getattr(dtype, "__name__", None) or str(dtype).split(".")[-1]      # "float16", torch.float16, np.float16, np.dtype
    if name not in TENSOR_DTYPES:
        raise ValueError("dtype %r: float32, float16 or bfloat16" % (dtype,))
    if layout not in TENSOR_LAYOUTS:
        raise ValueError("layout %r: NCHW or NHWC" % (layout,))
    s.dtype, s.layout = TENSOR_DTYPES.index(name), TENSOR_LAYOUTS.index(layout)
    s.out_w, s.out_h = (0, 0) if size is None else (int(size[0]), int(size[1]))
    for field, given, default in (("scale", scale, 1.0), ("bias", bias, 0.0)):
        v = [default] * 4 if given is None else ([float(given)] * 4 if np.isscalar(given) else [float(x) for x in given])
        v += [default] * (4 - len(v))
        setattr(s, field, (ctypes.c_float * 4)(*v[:4]))
    return s


def _origins(origins, n):
    """(int32 array of 2 n or None, what to pass) from None, one (ox, oy) for all frames, or n of them"""
    if origins is None:
        return None, None
    a = np.asarray(origins, np.int32)
    if a.shape == (2,):
        a = np.tile(a, (n, 1))
    if a.shape != (n, 2):
        raise ValueError("origins: one (ox, oy), or one per frame")
    a = np.ascontiguousarray(a)
    return a, a.ctypes.data_as(ctypes.c_void_p)


RESIZE_FILTERS = ["nearest", "bilinear", "triangle"]


def _resize_filter(f):
    """HTJ2K_RESIZE_* from its name; a number passes through (the library checks it)"""
    if isinstance(f, str):
        if f not in RESIZE_FILTERS:
            raise ValueError("filter %r: nearest, bilinear or triangle" % (f,))
        return RESIZE_FILTERS.index(f)
    return int(f)


def _windows(windows, n):
    """(int32 array of 4 n or None, what to pass) from None (each frame whole), one (ox, oy, ww, wh) for all frames, or n"""
    if windows is None:
        return None, None
    a = np.asarray(windows, np.int32)
    if a.shape == (4,):
        a = np.tile(a, (n, 1))
    if a.shape != (n, 4):
        raise ValueError("windows: one (ox, oy, ww, wh), or one per frame")
    a = np.ascontiguousarray(a)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _resized_out(pix_fmt, bits, dtype, layout, size, scale, bias, n, out, device, mix=None):
    """(spec, tensor, bytes of one image) of a resized call: the image has the spec's size, whatever the frames'"""
    if size is None or int(size[0]) < 1 or int(size[1]) < 1:
        raise ValueError("size: (out_w, out_h), both at least 1")
    spec = tensor_spec(dtype, layout, size, scale, bias)
    elems, nbytes = Decoder.tensor_image_size(pix_fmt, spec.out_w, spec.out_h, bits, spec, mix)
    return spec, _tensor_out(spec, n, elems // (spec.out_w * spec.out_h), spec.out_w, spec.out_h, out, device), nbytes


def _tensor_out(spec, n, ncomp, w, h, out, device):
    """the destination of a tensor call: `out` checked (dtype, shape, contiguity, device), or a new torch tensor"""
    import torch
    dt = getattr(torch, TENSOR_DTYPES[spec.dtype])
    shape = (n, ncomp, h, w) if spec.layout == 0 else (n, h, w, ncomp)
    if out is None:
        return torch.empty(shape, dtype=dt, device="cuda:%d" % device)
    if out.dtype != dt or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda or out.device.index != device:
        raise ValueError("out must be a contiguous %s tensor of shape %r on cuda:%d" % (dt, shape, device))
    return out


_CHROMA_SHIFTS = {"410": (2, 2), "411": (2, 0), "420": (1, 1), "422": (1, 0), "440": (0, 1), "444": (0, 0)}


def plane_geometry(pix_fmt, width, height):
    """[(rows, bytes of a row that hold samples)] of every plane of a layout, from its name: the planes of a yuv(a)NNNp
    layout are its components, chroma at its ceilinged size; every other layout has one plane of interleaved samples"""
    name = PIX_NAMES[pix_fmt] if not isinstance(pix_fmt, str) else pix_fmt
    nbytes = 2 if name.endswith("le") else 1
    if not name.startswith("yuv"):
        return [(height, width * _PACKED_COMPS[PIX_NAMES.index(name)] * nbytes)]
    sw, sh = _CHROMA_SHIFTS[name[4:7] if name[3] == "a" else name[3:6]]
    luma, chroma = (height, width * nbytes), (-(-height >> sh), (-(-width >> sw)) * nbytes)
    return [luma, chroma, chroma] + ([luma] if name[3] == "a" else [])


def _device_frames(n, fmt, w, h, device):
    """n frames of w x h in device memory -> (Frame array, the torch uint8 tensors that own its planes): rows at their own
    bytes, every byte zero"""
    import torch
    if int(w) < 1 or int(h) < 1:
        raise ValueError("size: (out_w, out_h), both at least 1")
    _, _, ph, rb = Decoder.plane_sizes(fmt, int(w), int(h))
    arr, keep = (Frame * n)(), []
    for i in range(n):
        arr[i].width, arr[i].height, arr[i].pix_fmt = int(w), int(h), fmt
        for p, (rows, rowbytes) in enumerate(zip(ph, rb)):
            d = torch.zeros(rows * rowbytes, dtype=torch.uint8, device="cuda:%d" % device)
            keep.append(d)
            arr[i].data[p] = d.data_ptr()
            arr[i].linesize[p] = rowbytes
    return arr, keep


def _tensor_in(t, pix_fmt, bits, layout, scale, bias, device, mix=None):
    """the source of a tensor-as-frames call checked: a contiguous CUDA tensor of shape (n, C, H, W) or (n, H, W, C) of
    float32, float16 or bfloat16 on `device` -> (spec, n, width, height, bytes of one image).  With a mix (a TensorMixIn)
    C is its K"""
    import torch
    if isinstance(pix_fmt, str):
        pix_fmt = PIX_NAMES.index(pix_fmt)
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or not t.is_cuda or t.device.index != device or not t.is_contiguous() \
            or str(t.dtype).split(".")[-1] not in TENSOR_DTYPES or layout not in TENSOR_LAYOUTS or t.shape[0] < 1:
        raise ValueError("a contiguous float32, float16 or bfloat16 tensor of shape (n, C, H, W) or (n, H, W, C) on cuda:%d" % device)
    spec = tensor_spec(t.dtype, layout, None, scale, bias)
    n, (c, h, w) = t.shape[0], (t.shape[1:] if layout == "NCHW" else (t.shape[3], t.shape[1], t.shape[2]))
    if w < 1 or h < 1:
        raise ValueError("an image of %d x %d" % (w, h))
    if mix is None:
        elems, nbytes = Decoder.tensor_image_size(pix_fmt, w, h, bits, spec)
    else:
        e, b = ctypes.c_size_t(), ctypes.c_size_t()
        _check(load_library().htj2k_tensor_image_size_mix_in(int(pix_fmt), int(w), int(h), int(bits), ctypes.byref(spec), _mix_in_p(mix),
                                                             ctypes.byref(e), ctypes.byref(b)), "htj2k_tensor_image_size_mix_in")
        elems, nbytes = e.value, b.value
    if elems != c * h * w:
        raise ValueError("%d channels: %s has %d" % (c, "the mix" if mix is not None else PIX_NAMES[pix_fmt], elems // (h * w)))
    return spec, n, w, h, nbytes


class EncMeasureOpts(ctypes.Structure):
    """struct htj2k_enc_measure_opts (include/htj2k_amd.h)"""
    _fields_ = [("close_loop", ctypes.c_int), ("max_rounds", ctypes.c_int)]


class EncMeasured(ctypes.Structure):
    """struct htj2k_enc_measured (include/htj2k_amd.h)"""
    _fields_ = [("diff", FrameDiff), ("first_psnr", ctypes.c_double), ("target_used", ctypes.c_double),
                ("rounds", ctypes.c_int32), ("fell_back", ctypes.c_int32), ("short_measured", ctypes.c_int32)]


class BlockDesc(ctypes.Structure):
    """struct J2kBlock (csrc/j2k_plan.h): one codeblock descriptor, 32 bytes"""
    _fields_ = [("data_off", ctypes.c_uint32), ("plane_off", ctypes.c_uint32), ("lcup", ctypes.c_uint16),
                ("lref", ctypes.c_uint16), ("w", ctypes.c_uint16), ("h", ctypes.c_uint16), ("stride", ctypes.c_uint16),
                ("npasses", ctypes.c_uint8), ("zbp", ctypes.c_uint8), ("M_b", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("roi_shift", ctypes.c_uint8), ("tcomp", ctypes.c_uint8), ("f_step", ctypes.c_float),
                ("i_step", ctypes.c_int32)]


assert ctypes.sizeof(BlockDesc) == 32

EXPORTS = ["htj2k_open", "htj2k_close", "htj2k_set_log", "htj2k_probe", "htj2k_decode", "htj2k_job_parse",
           "htj2k_job_upload", "htj2k_job_run", "htj2k_job_download", "htj2k_job_wait", "htj2k_job_info",
           "htj2k_job_bytes_consumed", "htj2k_job_free", "htj2k_job_num_tilecomps", "htj2k_job_tilecomp_dims",
           "htj2k_job_read_plane", "htj2k_job_run_stages", "htj2k_job_stage_ms", "htj2k_idwt_plane",
           "htj2k_idwt_bench", "htj2k_copy_bench", "htj2k_mct_planes", "htj2k_ht_blocks", "htj2k_mq_blocks", "htj2k_job_block_errors",
           "htj2k_job_num_blocks", "htj2k_job_device_plane", "htj2k_set_int", "htj2k_version", "htj2k_device_name",
           "htj2k_job_parse_batch", "htj2k_job_parse_batch_ex", "htj2k_job_num_frames", "htj2k_job_host_ms", "htj2k_job_frame_info", "htj2k_job_download_frame",
           "htj2k_job_idwt_launches", "htj2k_job_idwt_hbm_bytes", "htj2k_job_coef16", "htj2k_job_ll16", "htj2k_job_idwt_packed", "htj2k_pk16_lift_bound", "htj2k_pk16_bounds", "htj2k_job_ht_blocks_per_wave",
           "htj2k_pipe_open", "htj2k_pipe_send", "htj2k_pipe_send_ref", "htj2k_pipe_flush", "htj2k_pipe_info", "htj2k_pipe_receive",
           "htj2k_pipe_skip", "htj2k_pipe_close", "htj2k_host_alloc", "htj2k_host_free",
           "htj2k_pipe_receive_device", "htj2k_pipe_receive_device_ref", "htj2k_pipe_release_device", "htj2k_job_device_frame", "htj2k_device_to_host",
           "htj2k_splitter_open", "htj2k_splitter_find_end", "htj2k_splitter_parse", "htj2k_splitter_close",
           "htj2k_mxf_next_essence",
           "htj2k_enc_opts_default", "htj2k_encode_bound", "htj2k_enc_layout", "htj2k_enc_assemble", "htj2k_enc_open",
           "htj2k_enc_close", "htj2k_enc_set_log", "htj2k_encode_frame", "htj2k_encode_batch", "htj2k_fdwt_plane", "htj2k_fdwt97_plane",
           "htj2k_ht_encode_blocks", "htj2k_enc_stage_ms", "htj2k_enc_ht_cycles",
           "htj2k_enc_assemble_planes", "htj2k_ht_encode_blocks_planes", "htj2k_enc_rc_stats", "htj2k_enc_last_planes",
           "htj2k_enc_rc_info", "htj2k_enc_rc_stage_ms", "htj2k_enc_tiles", "htj2k_fdwt_regions",
           "htj2k_enc_assemble_passes", "htj2k_ht_encode_blocks_passes", "htj2k_enc_last_passes", "htj2k_enc_ref_stage_ms", "htj2k_enc_rc_stats_passes",
           "htj2k_enc_ref_cycles",
           "htj2k_transcode_batch", "htj2k_transcode_frame", "htj2k_transcode_check", "htj2k_transcode_stage_ms",
           "htj2k_enc_assemble_quant", "htj2k_mq_blocks_raw", "htj2k_enc_last_rounds",
           "htj2k_enc_band_weights", "htj2k_enc_rc_base", "htj2k_enc_quality_info", "htj2k_enc_quality_stage_ms",
           "htj2k_enc_group_info", "htj2k_enc_group_stage_ms", "htj2k_enc_rc_group_select",
           "htj2k_transcode_opts_default", "htj2k_transcode_batch_opts", "htj2k_transcode_frame_opts",
           "htj2k_transcode_min_size", "htj2k_xc_rc_tables", "htj2k_ht_blocks_raw", "htj2k_transcode_check_opts",
           "htj2k_compare_frames", "htj2k_compare_ms", "htj2k_job_compare", "htj2k_encode_batch_measured",
           "htj2k_compare_frames_ssim", "htj2k_job_compare_ssim", "htj2k_enc_measure_ssim", "htj2k_enc_last_ssim",
           "htj2k_hash_frames", "htj2k_job_hash", "htj2k_pipe_receive_hash",
           "htj2k_tensor_spec_default", "htj2k_tensor_image_size", "htj2k_frames_to_tensor", "htj2k_job_to_tensor",
           "htj2k_pipe_receive_tensor", "htj2k_tensor_last_route", "htj2k_tensor_to_frames", "htj2k_encode_tensor",
           "htj2k_resize_weights", "htj2k_frames_to_tensor_resized", "htj2k_job_to_tensor_resized", "htj2k_pipe_receive_tensor_resized",
           "htj2k_tensor_mix_ycbcr", "htj2k_tensor_image_size_mix", "htj2k_frames_to_tensor_mix", "htj2k_job_to_tensor_mix",
           "htj2k_pipe_receive_tensor_mix", "htj2k_frames_to_tensor_resized_mix", "htj2k_job_to_tensor_resized_mix",
           "htj2k_pipe_receive_tensor_resized_mix",
           "htj2k_tensor_curve_fill", "htj2k_tensor_mix_xyz", "htj2k_frames_to_tensor_curves", "htj2k_job_to_tensor_curves",
           "htj2k_pipe_receive_tensor_curves", "htj2k_frames_to_tensor_resized_curves", "htj2k_job_to_tensor_resized_curves",
           "htj2k_pipe_receive_tensor_resized_curves",
           "htj2k_tensor_mix_in_rgb", "htj2k_tensor_image_size_mix_in", "htj2k_tensor_to_frames_mix", "htj2k_encode_tensor_mix",
           "htj2k_tensor_curve_fill_root", "htj2k_tensor_mix_in_xyz", "htj2k_tensor_to_frames_curves", "htj2k_encode_tensor_curves",
           "htj2k_resize_frames", "htj2k_job_resize_frames", "htj2k_pipe_receive_resized", "htj2k_frame_plane_sizes"]

_lib = None


def load_library():
    """Load libhtj2k_amd.so.  Raises if it has not been built: there is no other implementation."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libhtj2k_amd.so is not built (run `make lib` / __graft_entry__.build()); "
                              "this package has no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        L.htj2k_version.restype = ctypes.c_char_p
        L.htj2k_device_name.restype = ctypes.c_char_p
        L.htj2k_device_name.argtypes = [ctypes.c_void_p]
        L.htj2k_job_device_plane.restype = ctypes.c_void_p
        L.htj2k_host_alloc.restype = ctypes.c_void_p
        L.htj2k_host_alloc.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        L.htj2k_host_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        _lib = L
    return _lib


def _check(r, what):
    if r < 0:
        raise Htj2kError(r, what)
    return r


def _pkt(data):
    # AVPacket data carries AV_INPUT_BUFFER_PADDING_SIZE (64) zero bytes of padding (libavcodec/defs.h:40)
    return ctypes.create_string_buffer(bytes(data) + b"\0" * 64, len(data) + 64)


def packet(data):
    """(padded ctypes buffer, size): a packet that can be sent many times without re-copying it in Python"""
    return _pkt(data), len(data)


class Job:
    """One frame in the staged pipeline (htj2k_job_*)."""

    def __init__(self, dec):
        self.dec = dec
        self.h = ctypes.c_void_p(None)
        self._buf = None

    def parse(self, data):
        self._buf = _pkt(data)
        _check(self.dec.L.htj2k_job_parse(self.dec.h, self._buf, len(data), ctypes.byref(self.h)), "htj2k_job_parse")
        return self

    def parse_batch(self, datas):
        """several independent frames -> one job whose stages are single launches over the whole batch"""
        n = len(datas)
        pk = [d if isinstance(d, tuple) else packet(d) for d in datas]       # packet(): padded ctypes buffer, reusable
        self._bufs = [b for b, _ in pk]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p) for b in self._bufs])
        sizes = (ctypes.c_int * n)(*[sz for _, sz in pk])
        _check(self.dec.L.htj2k_job_parse_batch(self.dec.h, ptrs, sizes, n, ctypes.byref(self.h)), "htj2k_job_parse_batch")
        return self

    def num_frames(self):
        return _check(self.dec.L.htj2k_job_num_frames(self.h), "htj2k_job_num_frames")

    def host_ms(self):
        """(parse ms, staging-copy ms) per frame of the last parse / parse_batch, summed over the threads that worked"""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(self.dec.L.htj2k_job_host_ms(self.h, ctypes.byref(a), ctypes.byref(b)), "htj2k_job_host_ms")
        return a.value, b.value

    def frame_info(self, f):
        info = Info()
        _check(self.dec.L.htj2k_job_frame_info(self.h, f, ctypes.byref(info)), "htj2k_job_frame_info")
        return info

    def download_frame(self, f):
        info = self.frame_info(f)
        planes, fr = alloc_frame(info)
        _check(self.dec.L.htj2k_job_download_frame(self.dec.h, self.h, f, ctypes.byref(fr)), "htj2k_job_download_frame")
        return info, planes_to_arrays(info, planes)

    def idwt_launches(self, cap=256):
        """[(ms, algorithmic_bytes)] of the IDWT launches of the last run"""
        ms = (ctypes.c_float * cap)()
        by = (ctypes.c_double * cap)()
        n = _check(self.dec.L.htj2k_job_idwt_launches(self.dec.h, self.h, ms, by, cap), "htj2k_job_idwt_launches")
        return [(ms[i], by[i]) for i in range(min(n, cap))]

    def idwt_hbm_bytes(self, cap=256):
        """least HBM bytes of the same launches (differs from the algorithmic figure for a fused final level)"""
        by = (ctypes.c_double * cap)()
        n = _check(self.dec.L.htj2k_job_idwt_hbm_bytes(self.dec.h, self.h, by, cap), "htj2k_job_idwt_hbm_bytes")
        return [by[i] for i in range(min(n, cap))]

    def upload(self):
        _check(self.dec.L.htj2k_job_upload(self.dec.h, self.h), "htj2k_job_upload")
        return self

    def run(self, stages=7):
        _check(self.dec.L.htj2k_job_run_stages(self.dec.h, self.h, stages), "htj2k_job_run_stages")
        return self

    def wait(self):
        _check(self.dec.L.htj2k_job_wait(self.dec.h, self.h), "htj2k_job_wait")
        return self

    def info(self):
        info = Info()
        _check(self.dec.L.htj2k_job_info(self.h, ctypes.byref(info)), "htj2k_job_info")
        return info

    def stage_ms(self):
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        _check(self.dec.L.htj2k_job_stage_ms(self.dec.h, self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
               "htj2k_job_stage_ms")
        return a.value, b.value, c.value

    def coef16(self):
        """did the last run keep the sub-bands as 16-bit samples between block decoder and IDWT?"""
        return bool(_check(self.dec.L.htj2k_job_coef16(self.h), "htj2k_job_coef16"))

    def ht_blocks_per_wave(self):
        """codeblocks per wavefront in the MagSgn kernel of the last run: 1, 2 or 4 (htj2k_job_ht_blocks_per_wave)"""
        return _check(self.dec.L.htj2k_job_ht_blocks_per_wave(self.h), "htj2k_job_ht_blocks_per_wave")

    def ll16(self):
        """0 / 1 / 2: LL bands between the IDWT levels 32-bit / 16-bit / 16-bit, overflowed and run again (htj2k_job_ll16)"""
        return _check(self.dec.L.htj2k_job_ll16(self.h), "htj2k_job_ll16")

    def idwt_packed(self):
        """0, or the bits the LL bands had to fit for the last run's packed 16-bit final level (htj2k_job_idwt_packed)"""
        return _check(self.dec.L.htj2k_job_idwt_packed(self.h), "htj2k_job_idwt_packed")

    def num_tilecomps(self):
        return _check(self.dec.L.htj2k_job_num_tilecomps(self.h), "htj2k_job_num_tilecomps")

    def num_blocks(self):
        return _check(self.dec.L.htj2k_job_num_blocks(self.h), "htj2k_job_num_blocks")

    def block_errors(self):
        return _check(self.dec.L.htj2k_job_block_errors(self.dec.h, self.h), "htj2k_job_block_errors")

    def plane(self, tc):
        w, h, f = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(self.dec.L.htj2k_job_tilecomp_dims(self.h, tc, ctypes.byref(w), ctypes.byref(h), ctypes.byref(f)),
               "htj2k_job_tilecomp_dims")
        a = np.empty((h.value, w.value), dtype=np.float32 if f.value else np.int32)
        _check(self.dec.L.htj2k_job_read_plane(self.dec.h, self.h, tc, a.ctypes.data_as(ctypes.c_void_p),
                                               ctypes.c_size_t(a.nbytes)), "htj2k_job_read_plane")
        return a

    def download(self):
        info = self.info()
        planes, fr = alloc_frame(info)
        _check(self.dec.L.htj2k_job_download(self.dec.h, self.h, ctypes.byref(fr)), "htj2k_job_download")
        return info, planes_to_arrays(info, planes)

    def device_frame(self, f=0):
        """Frame whose data[] are the device addresses of frame f's decoded planes (htj2k_job_device_frame)"""
        fr = Frame()
        _check(self.dec.L.htj2k_job_device_frame(self.dec.h, self.h, f, ctypes.byref(fr)), "htj2k_job_device_frame")
        return fr

    def compare(self, ref_planes, bits=0, on_device=False):
        """every frame of the job's last run against ref_planes[f] (numpy planes of the job's layout, or a Frame; with
        on_device Frames of device addresses), on the device and without a download (htj2k_job_compare) -> [dict] as
        Decoder.compare.  bits 0: the job's bits_per_raw_sample"""
        n = self.num_frames()
        if len(ref_planes) != n:
            raise ValueError("%d reference frames for a job of %d" % (len(ref_planes), n))
        arr, keep = _frame_array(ref_planes, self.frame_info(0).pix_fmt)
        out = (FrameDiff * n)()
        _check(self.dec.L.htj2k_job_compare(self.dec.h, self.h, arr, int(on_device), int(bits), out), "htj2k_job_compare")
        return [d.as_dict() for d in out]

    def compare_ssim(self, ref_planes, bits=0, on_device=False):
        """compare() with the structural figure (htj2k_job_compare_ssim) -> [dict] as Decoder.compare_ssim"""
        n = self.num_frames()
        if len(ref_planes) != n:
            raise ValueError("%d reference frames for a job of %d" % (len(ref_planes), n))
        arr, keep = _frame_array(ref_planes, self.frame_info(0).pix_fmt)
        out = (FrameSsim * n)()
        _check(self.dec.L.htj2k_job_compare_ssim(self.dec.h, self.h, arr, int(on_device), int(bits), out), "htj2k_job_compare_ssim")
        return [d.as_dict() for d in out]

    def framecrc(self):
        """the checksum of every frame of the job's last run, on the device and without a download (htj2k_job_hash) ->
        [dict] as Decoder.framecrc; a frame without a plan has nbytes 0"""
        n = self.num_frames()
        out = (FrameHash * max(n, 1))()
        _check(self.dec.L.htj2k_job_hash(self.dec.h, self.h, out), "htj2k_job_hash")
        return [out[i].as_dict() for i in range(n)]

    def to_tensor(self, dtype="float16", layout="NCHW", size=None, origins=None, scale=None, bias=None, bits=0, out=None, mix=None,
                  curves=None):
        """every frame of the job's last run as one torch tensor, converted on the device and without a download
        (htj2k_job_to_tensor_mix; arguments as Decoder.to_tensor, bits 0: the job's) -> (tensor, status): status[f] is 0,
        or 1 for a frame without a plan, whose image is zeros"""
        import torch
        n = self.num_frames()
        info = self.frame_info(0)
        spec = tensor_spec(dtype, layout, size, scale, bias)
        w, h = (info.width, info.height) if size is None else (spec.out_w, spec.out_h)
        elems, nbytes = Decoder.tensor_image_size(info.pix_fmt, info.width, info.height, bits or info.bits_per_raw_sample, spec, mix)
        t = _tensor_out(spec, n, elems // (w * h), w, h, out, self.dec.device_id)
        org, org_p = _origins(origins, n)
        status = (ctypes.c_int * n)()
        torch.cuda.synchronize()
        _check(self.dec.L.htj2k_job_to_tensor_curves(self.dec.h, self.h, int(bits), ctypes.byref(spec), _mix_p(mix),
                                                     _curves_p(curves, mix), org_p,
                                                  ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(n * nbytes), status), "htj2k_job_to_tensor")
        return t, [int(v) for v in status]

    def to_tensor_resized(self, size, windows=None, filter="triangle", dtype="float16", layout="NCHW", scale=None, bias=None, bits=0,
                          out=None, mix=None, curves=None):
        """every frame of the job's last run, a window of each resampled to size = (out_w, out_h), as one torch tensor
        (htj2k_job_to_tensor_resized; arguments as Decoder.to_tensor_resized, bits 0: the job's) -> (tensor, status)"""
        import torch
        n = self.num_frames()
        info = self.frame_info(0)
        spec, t, nbytes = _resized_out(info.pix_fmt, bits or info.bits_per_raw_sample, dtype, layout, size, scale, bias, n, out,
                                       self.dec.device_id, mix)
        win, win_p = _windows(windows, n)
        status = (ctypes.c_int * n)()
        torch.cuda.synchronize()
        _check(self.dec.L.htj2k_job_to_tensor_resized_curves(self.dec.h, self.h, int(bits), ctypes.byref(spec), _mix_p(mix),
                                                     _curves_p(curves, mix), win_p,
                                                          _resize_filter(filter), ctypes.c_void_p(t.data_ptr()),
                                                          ctypes.c_size_t(n * nbytes), status),
               "htj2k_job_to_tensor_resized")
        return t, [int(v) for v in status]

    def resized_frames(self, size, windows=None, filter="triangle", bits=0):
        """every frame of the job's last run, a window of each resampled plane by plane to a frame of size = (out_w, out_h)
        in device memory (htj2k_job_resize_frames; arguments as Decoder.resize_frames, bits 0: the job's)
        -> (frames, keep, status): status[f] is 0, or 1 for a frame without a plan, whose samples are zero"""
        import torch
        n = self.num_frames()
        info = self.frame_info(0)
        if size is None:
            raise ValueError("size: (out_w, out_h), both at least 1")
        arr, keep = _device_frames(n, info.pix_fmt, size[0], size[1], self.dec.device_id)
        win, win_p = _windows(windows, n)
        status = (ctypes.c_int * n)()
        torch.cuda.synchronize()
        _check(self.dec.L.htj2k_job_resize_frames(self.dec.h, self.h, int(bits), win_p, _resize_filter(filter), arr, status),
               "htj2k_job_resize_frames")
        return arr, keep, [int(v) for v in status]

    def free(self):
        if self.h:
            self.dec.L.htj2k_job_free(self.dec.h, self.h)
            self.h = ctypes.c_void_p(None)


def _frame_array(frames, pix_fmt):
    """((Frame * n), what it points into) of frames given as Frame structs or as lists of numpy planes; a ready
    (Frame * n) array passes through"""
    if isinstance(frames, ctypes.Array):
        return frames, None
    keep, made = [], []
    for f in frames:
        if isinstance(f, Frame):
            made.append(f)
        else:
            fr, k = frame_from_planes(f, pix_fmt)
            made.append(fr)
            keep.append(k)
    return (Frame * max(len(made), 1))(*made), keep


def alloc_frame(info, align=1):
    planes, fr = [], Frame()
    for p in range(info.nplanes):
        rowbytes = info.plane_width[p] * info.plane_bytes_per_sample[p]
        ls = -(-rowbytes // align) * align
        a = np.zeros((info.plane_height[p], ls), dtype=np.uint8)
        planes.append(a)
        fr.data[p] = a.ctypes.data
        fr.linesize[p] = ls
    return planes, fr


def planes_to_arrays(info, planes):
    out = []
    for p in range(info.nplanes):
        rowbytes = info.plane_width[p] * info.plane_bytes_per_sample[p]
        a = np.ascontiguousarray(planes[p][:, :rowbytes])
        if info.bits_per_raw_sample > 8:
            a = a.view(np.uint16)
        out.append(a.reshape(info.plane_height[p], -1))
    return out


EAGAIN = -11


class Splitter:
    """htj2k_splitter_*: cuts a byte stream of back-to-back codestreams / JP2 files into packets (the reference's
    jpeg2000 AVCodecParser, libavcodec/jpeg2000_parser.c).  Host only: works without a GPU."""
    END_NOT_FOUND = -100

    def __init__(self):
        self.L = load_library()
        self.h = ctypes.c_void_p()
        _check(self.L.htj2k_splitter_open(ctypes.byref(self.h)), "htj2k_splitter_open")

    def find_end(self, data):
        buf = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
        return self.L.htj2k_splitter_find_end(self.h, buf, len(data))

    def parse(self, data):
        """-> (bytes consumed, frame bytes or None)"""
        buf = (ctypes.c_uint8 * (len(data) + 64)).from_buffer_copy(bytes(data) + bytes(64))
        fr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_int()
        used = _check(self.L.htj2k_splitter_parse(self.h, buf, len(data), ctypes.byref(fr), ctypes.byref(n)), "htj2k_splitter_parse")
        return used, (ctypes.string_at(fr, n.value) if fr else None)

    def split(self, stream, chunk=4096):
        """all frames of `stream`, fed `chunk` bytes at a time (the av_parser_parse2 loop)"""
        out, pos = [], 0
        while pos < len(stream):
            piece = stream[pos:pos + chunk]
            while True:
                used, fr = self.parse(piece)
                if fr is not None:
                    out.append(fr)
                pos += used
                piece = piece[used:]
                if not piece or (used == 0 and fr is None):
                    break
        used, fr = self.parse(b"")
        if fr:
            out.append(fr)
        return out

    def close(self):
        if self.h:
            self.L.htj2k_splitter_close(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MxfEssence(ctypes.Structure):
    """struct htj2k_mxf_essence (include/htj2k_amd.h)"""
    _fields_ = [("data", ctypes.POINTER(ctypes.c_uint8)), ("size", ctypes.c_size_t), ("klv_offset", ctypes.c_size_t),
                ("track_number", ctypes.c_uint32), ("wrapping", ctypes.c_int)]


MXF_FRAME_WRAPPED, MXF_CLIP_WRAPPED = 1, 2


def mxf_essence(data):
    """htj2k_mxf_next_essence over a whole MXF file: [(bytes, track_number, wrapping, klv_offset)] of its JPEG 2000
    picture elements (the KLV layer of libavformat/mxfdec.c).  Host only: works without a GPU."""
    L = load_library()
    L.htj2k_mxf_next_essence.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(MxfEssence)]
    data = bytes(data)
    pos, e, out = ctypes.c_size_t(0), MxfEssence(), []
    while _check(L.htj2k_mxf_next_essence(data, len(data), ctypes.byref(pos), ctypes.byref(e)), "htj2k_mxf_next_essence") == 1:
        out.append((ctypes.string_at(e.data, e.size), e.track_number, e.wrapping, e.klv_offset))
    return out


class Pipe:
    """htj2k_pipe_*: packets in, frames out (in order), `depth` batches of `batch` frames in flight"""

    def __init__(self, dec, batch=8, depth=3):
        self.dec = dec
        self.h = ctypes.c_void_p(None)
        _check(dec.L.htj2k_pipe_open(dec.h, batch, depth, ctypes.byref(self.h)), "htj2k_pipe_open")

    def send(self, data):
        """False when `depth` batches are waiting to be received.  `data`: bytes, or a (ctypes buffer, size) pair
        from packet() -- building the padded buffer costs two copies of the packet in Python"""
        if isinstance(data, tuple):                        # caller keeps the buffer alive: no copy in the library either
            buf, size = data
            r = self.dec.L.htj2k_pipe_send_ref(self.h, buf, size, None, None)
        else:
            r = self.dec.L.htj2k_pipe_send(self.h, _pkt(data), len(data))
        if r == EAGAIN:
            return False
        _check(r, "htj2k_pipe_send")
        return True

    def flush(self):
        _check(self.dec.L.htj2k_pipe_flush(self.h), "htj2k_pipe_flush")

    def receive(self, into=None):
        """-> (info, [plane arrays]) of the next frame, None when nothing is in flight; raises for a
        packet that failed (Htj2kError; the frame is consumed).  `into` = (planes, Frame) from alloc_frame to reuse buffers."""
        info = Info()
        r = self.dec.L.htj2k_pipe_info(self.h, ctypes.byref(info))
        if r == EAGAIN:
            return None
        if r < 0:
            self.dec.L.htj2k_pipe_skip(self.h)
            _check(r, "htj2k_pipe_info")
        planes, fr = into if into is not None else alloc_frame(info)
        _check(self.dec.L.htj2k_pipe_receive(self.h, ctypes.byref(fr)), "htj2k_pipe_receive")
        return info, planes_to_arrays(info, planes)

    def receive_device(self):
        """-> Frame whose data[] are device pointers (no copy), None when nothing is in flight"""
        fr = Frame()
        r = self.dec.L.htj2k_pipe_receive_device(self.h, ctypes.byref(fr))
        if r == EAGAIN:
            return None
        _check(r, "htj2k_pipe_receive_device")
        return fr

    def receive_device_ref(self):
        """-> (Frame of device pointers, token) valid until release_device(token); None when nothing is in flight"""
        fr, tok = Frame(), ctypes.c_uint64()
        r = self.dec.L.htj2k_pipe_receive_device_ref(self.h, ctypes.byref(fr), ctypes.byref(tok))
        if r == EAGAIN:
            return None
        _check(r, "htj2k_pipe_receive_device_ref")
        return fr, tok.value

    def receive_crc(self):
        """-> (info, dict as Decoder.framecrc) of the next frame, hashed on the device (htj2k_pipe_receive_hash); None when
        nothing is in flight; raises for a packet that failed (the frame is consumed)"""
        info, h = Info(), FrameHash()
        r = self.dec.L.htj2k_pipe_receive_hash(self.h, ctypes.byref(info), ctypes.byref(h))
        if r == EAGAIN:
            return None
        _check(r, "htj2k_pipe_receive_hash")
        return info, h.as_dict()

    def receive_tensor(self, dtype="float16", layout="NCHW", size=None, origin=None, scale=None, bias=None, bits=0, out=None, mix=None,
                  curves=None):
        """-> (tensor of shape (1, C, h, w) or (1, h, w, C), info) of the next frame, converted on the device
        (htj2k_pipe_receive_tensor; arguments as Decoder.to_tensor, bits 0: the frame's own); None when nothing is in
        flight; raises for a packet that failed (the frame is consumed)"""
        import torch
        info = Info()
        r = self.dec.L.htj2k_pipe_info(self.h, ctypes.byref(info))
        if r == EAGAIN:
            return None
        if r < 0:
            self.dec.L.htj2k_pipe_skip(self.h)
            _check(r, "htj2k_pipe_info")
        spec = tensor_spec(dtype, layout, size, scale, bias)
        w, h = (info.width, info.height) if size is None else (spec.out_w, spec.out_h)
        try:
            elems, nbytes = Decoder.tensor_image_size(info.pix_fmt, info.width, info.height, bits or info.bits_per_raw_sample, spec, mix)
            t = _tensor_out(spec, 1, elems // (w * h), w, h, out, self.dec.device_id)
        except Exception:
            self.dec.L.htj2k_pipe_skip(self.h)                # the frame is consumed, as by every failed receive
            raise
        org, org_p = _origins(origin, 1)
        torch.cuda.synchronize()
        _check(self.dec.L.htj2k_pipe_receive_tensor_curves(self.h, ctypes.byref(info), int(bits), ctypes.byref(spec), _mix_p(mix),
                                                     _curves_p(curves, mix), org_p,
                                                        ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(nbytes)), "htj2k_pipe_receive_tensor")
        return t, info

    def receive_tensor_resized(self, size, window=None, filter="triangle", dtype="float16", layout="NCHW", scale=None, bias=None,
                               bits=0, out=None, mix=None, curves=None):
        """-> (tensor of shape (1, C, out_h, out_w) or (1, out_h, out_w, C), info): the window (ox, oy, ww, wh; None: the
        frame whole) of the next frame resampled to size = (out_w, out_h) on the device
        (htj2k_pipe_receive_tensor_resized); None when nothing is in flight; raises for a packet that failed (the frame
        is consumed)"""
        import torch
        info = Info()
        r = self.dec.L.htj2k_pipe_info(self.h, ctypes.byref(info))
        if r == EAGAIN:
            return None
        if r < 0:
            self.dec.L.htj2k_pipe_skip(self.h)
            _check(r, "htj2k_pipe_info")
        try:
            spec, t, nbytes = _resized_out(info.pix_fmt, bits or info.bits_per_raw_sample, dtype, layout, size, scale, bias, 1, out,
                                           self.dec.device_id, mix)
            win, win_p = _windows(window, 1)
            flt = _resize_filter(filter)
        except Exception:
            self.dec.L.htj2k_pipe_skip(self.h)                # the frame is consumed, as by every failed receive
            raise
        torch.cuda.synchronize()
        _check(self.dec.L.htj2k_pipe_receive_tensor_resized_curves(self.h, ctypes.byref(info), int(bits), ctypes.byref(spec), _mix_p(mix),
                                                     _curves_p(curves, mix),
                                                                win_p, flt, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(nbytes)),
               "htj2k_pipe_receive_tensor_resized")
        return t, info

    def receive_resized(self, size, window=None, filter="triangle", bits=0):
        """-> (frame, keep, info): the window (ox, oy, ww, wh; None: the frame whole) of the next frame resampled plane by
        plane to a frame of size = (out_w, out_h) in device memory (htj2k_pipe_receive_resized; `frame` is a Frame array
        of one, `keep` the tensors that own its planes); None when nothing is in flight; raises for a packet that failed
        (the frame is consumed)"""
        import torch
        info = Info()
        r = self.dec.L.htj2k_pipe_info(self.h, ctypes.byref(info))
        if r == EAGAIN:
            return None
        if r < 0:
            self.dec.L.htj2k_pipe_skip(self.h)
            _check(r, "htj2k_pipe_info")
        try:
            if size is None:
                raise ValueError("size: (out_w, out_h), both at least 1")
            arr, keep = _device_frames(1, info.pix_fmt, size[0], size[1], self.dec.device_id)
            win, win_p = _windows(window, 1)
            flt = _resize_filter(filter)
        except Exception:
            self.dec.L.htj2k_pipe_skip(self.h)                # the frame is consumed, as by every failed receive
            raise
        torch.cuda.synchronize()
        _check(self.dec.L.htj2k_pipe_receive_resized(self.h, ctypes.byref(info), int(bits), win_p, flt, arr), "htj2k_pipe_receive_resized")
        return arr, keep, info

    def release_device(self, token):
        _check(self.dec.L.htj2k_pipe_release_device(self.h, ctypes.c_uint64(token)), "htj2k_pipe_release_device")

    def close(self):
        if self.h:
            self.dec.L.htj2k_pipe_close(self.h)
            self.h = ctypes.c_void_p(None)


class Decoder:
    """htj2k_open / htj2k_probe / htj2k_decode / htj2k_close: the FFCodec init/decode/close trio."""

    def __init__(self, device_id=0, bitexact=0, reduction_factor=0, req_pix_fmt=-1, strict=0, max_pixels=0, frames_in_flight=0):
        self.L = load_library()
        o = Opts()
        o.device_id = device_id
        o.frames_in_flight = frames_in_flight
        o.bitexact = bitexact
        o.reduction_factor = reduction_factor
        o.req_pix_fmt = req_pix_fmt
        o.strict = strict
        o.max_pixels = max_pixels
        self.h = ctypes.c_void_p(None)
        _check(self.L.htj2k_open(ctypes.byref(o), ctypes.byref(self.h)), "htj2k_open")
        self.device_id = device_id
        self._buf = None

    def close(self):
        if self.h:
            self.L.htj2k_close(self.h)
            self.h = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_name(self):
        return self.L.htj2k_device_name(self.h).decode()

    def set_int(self, name, value):
        _check(self.L.htj2k_set_int(self.h, name.encode(), int(value)), "htj2k_set_int")

    def pipe(self, batch=8, depth=3):
        return Pipe(self, batch, depth)

    def fetch_device_frame(self, info, fr):
        """[plane arrays] of a frame whose data[] are device pointers (Pipe.receive_device, Job.device_frame)"""
        planes = []
        for p in range(info.nplanes):
            ls = fr.linesize[p]
            a = np.zeros((info.plane_height[p], ls), dtype=np.uint8)
            _check(self.L.htj2k_device_to_host(self.h, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(fr.data[p]),
                                               ctypes.c_size_t(a.nbytes)), "htj2k_device_to_host")
            planes.append(a)
        return planes_to_arrays(info, planes)

    def alloc_frame_pinned(self, info):
        """frame planes in page-locked host memory (htj2k_host_alloc); free with free_frame_pinned"""
        planes, fr, ptrs = [], Frame(), []
        for p in range(info.nplanes):
            ls = info.plane_width[p] * info.plane_bytes_per_sample[p]
            n = ls * info.plane_height[p]
            ptr = self.L.htj2k_host_alloc(self.h, n)
            if not ptr:
                raise MemoryError("htj2k_host_alloc")
            ptrs.append(ptr)
            a = np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(ptr)).reshape(info.plane_height[p], ls)
            planes.append(a)
            fr.data[p] = ptr
            fr.linesize[p] = ls
        return (planes, fr), ptrs

    def free_frame_pinned(self, ptrs):
        for ptr in ptrs:
            self.L.htj2k_host_free(self.h, ptr)

    def probe(self, data):
        info = Info()
        self._buf = _pkt(data)
        _check(self.L.htj2k_probe(self.h, self._buf, len(data), ctypes.byref(info)), "htj2k_probe")
        return info

    def decode(self, data, align=1):
        """-> (info, [plane arrays], bytes_consumed, Stats)"""
        info = self.probe(data)
        planes, fr = alloc_frame(info, align)
        st = Stats()
        self._buf = _pkt(data)
        r = _check(self.L.htj2k_decode(self.h, self._buf, len(data), ctypes.byref(fr), ctypes.byref(st)), "htj2k_decode")
        return info, planes_to_arrays(info, planes), r, st

    def decode_into(self, pkt, buf):
        """htj2k_decode of a packet() into the planes of alloc_frame(): nothing is copied or allocated in Python"""
        st = Stats()
        return _check(self.L.htj2k_decode(self.h, pkt[0], pkt[1], ctypes.byref(buf[1]), ctypes.byref(st)), "htj2k_decode"), st

    def job(self):
        return Job(self)

    def compare(self, a, b, pix_fmt, bits, on_device=(False, False)):
        """htj2k_compare_frames: a[i] against b[i] on the device, one launch for all pairs -> [dict] with, per pair, sse /
        ndiff / nsamples / max_abs (lists of four ints, one per component of the layout) and psnr (pooled; inf for equal
        frames).  A frame is a list of numpy planes (frame_from_planes) or a Frame -- the way to give a linesize or an
        offset of one's own, and, with on_device[k] set, device addresses; a and b may also be ready (Frame * n) arrays."""
        n = len(a)
        if len(b) != n:
            raise ValueError("%d frames against %d" % (n, len(b)))
        fa, ka = _frame_array(a, pix_fmt)
        fb, kb = _frame_array(b, pix_fmt)
        out = (FrameDiff * max(n, 1))()
        _check(self.L.htj2k_compare_frames(self.h, fa, int(on_device[0]), fb, int(on_device[1]), n, int(bits), out),
               "htj2k_compare_frames")
        return [out[i].as_dict() for i in range(n)]

    def compare_ssim(self, a, b, pix_fmt, bits, on_device=(False, False)):
        """htj2k_compare_frames_ssim: compare() with `ffmpeg -lavfi ssim`'s figure -> [dict] with, per pair, q32 (per
        component the integer sum over its 8x8 windows of rint(ssim * 2^32)), nwin, ssim (q32 / 2^32 / nwin, NaN where a
        component has no window) and all (pooled by cw * ch).  bits >= 4."""
        n = len(a)
        if len(b) != n:
            raise ValueError("%d frames against %d" % (n, len(b)))
        fa, ka = _frame_array(a, pix_fmt)
        fb, kb = _frame_array(b, pix_fmt)
        out = (FrameSsim * max(n, 1))()
        _check(self.L.htj2k_compare_frames_ssim(self.h, fa, int(on_device[0]), fb, int(on_device[1]), n, int(bits), out),
               "htj2k_compare_frames_ssim")
        return [out[i].as_dict() for i in range(n)]

    def framecrc(self, frames, pix_fmt, on_device=False):
        """htj2k_hash_frames: what `-f framecrc` prints for each frame, computed on the device in one launch -> [dict] with
        adler32 (Adler-32 seeded with 0 over the packed planes), plane_adler32 (each plane alone) and nbytes.  A frame is a
        list of numpy planes (pal8: the indices and the palette) or a Frame, with on_device a Frame of device addresses;
        pix_fmt is one layout for all frames given as planes, or a list with one per frame."""
        n = len(frames)
        if isinstance(frames, ctypes.Array):
            arr, keep = frames, None
        else:
            fmts = list(pix_fmt) if isinstance(pix_fmt, (list, tuple)) else [pix_fmt] * n
            made = [_frame_array([f], fmt) for f, fmt in zip(frames, fmts)]
            arr, keep = (Frame * max(n, 1))(*[a[0] for a, _ in made]), [k for _, k in made]
        out = (FrameHash * max(n, 1))()
        _check(self.L.htj2k_hash_frames(self.h, arr, int(on_device), n, out), "htj2k_hash_frames")
        return [out[i].as_dict() for i in range(n)]

    @staticmethod
    def tensor_image_size(pix_fmt, width, height, bits, spec, mix=None):
        """(elements, bytes) of one image of a tensor call (htj2k_tensor_image_size_mix; no context, no device); raises the
        refusal the call itself would give.  With a mix the image has its K channels"""
        if isinstance(pix_fmt, str):
            pix_fmt = PIX_NAMES.index(pix_fmt)
        e, b = ctypes.c_size_t(), ctypes.c_size_t()
        _check(load_library().htj2k_tensor_image_size_mix(int(pix_fmt), int(width), int(height), int(bits), ctypes.byref(spec),
                                                          _mix_p(mix), ctypes.byref(e), ctypes.byref(b)), "htj2k_tensor_image_size")
        return e.value, b.value

    @staticmethod
    def ycbcr_mix(standard, bits, full_range=False, alpha=False, gain=None, offset=None):
        """htj2k_tensor_mix_ycbcr (no context, no device): the TensorMix that takes Y'CbCr samples of `bits` bits to R', G',
        B' (nominal 0 .. 1) times gain[k] plus offset[k]; standard 601, 709 or 2020; alpha: a fourth channel, component 3
        over its peak.  gain, offset: three numbers each, None: 1 and 0"""
        mix = TensorMix()
        g = None if gain is None else (ctypes.c_float * 3)(*[float(v) for v in gain])
        o = None if offset is None else (ctypes.c_float * 3)(*[float(v) for v in offset])
        _check(load_library().htj2k_tensor_mix_ycbcr(ctypes.byref(mix), int(standard), int(bool(full_range)), int(bits), int(bool(alpha)),
                                                     g, o), "htj2k_tensor_mix_ycbcr")
        return mix

    @staticmethod
    def xyz_mix(primaries, scale=1.0):
        """htj2k_tensor_mix_xyz (no context, no device): the TensorMix that takes linear XYZ to linear R, G, B of the
        primaries 709 (also sRGB), 2020 or PRIMARIES_P3D65 with white point D65, times scale"""
        mix = TensorMix()
        L = load_library()
        L.htj2k_tensor_mix_xyz.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
        _check(L.htj2k_tensor_mix_xyz(ctypes.byref(mix), int(primaries), float(scale)), "htj2k_tensor_mix_xyz")
        return mix

    @staticmethod
    def dcp_curves(primaries=709, out="srgb", n_out=4097, gain=None, offset=None):
        """(mix, curves) that take the X'Y'Z' of a digital cinema package (xyz12le at 12 bits) to R, G, B of `primaries` in
        the encoding `out` ("srgb", "bt709", "pq"): the 2.6 power law over s / 4095 as an exact 4096-knot lookup of the
        sample, the XYZ matrix with the DCI normalisation 52.37 / 48, and the encoding over 0 .. 1 with n_out knots"""
        t_in = curve_table("power", 4096, 0.0, 1.0, 2.6)
        t_out = curve_table(out + "_encode", n_out, 0.0, 1.0)
        curves = tensor_curves(tensor_curve(t_in, 0.0, 1.0), tensor_curve(t_out, 0.0, float(n_out - 1)), 7, 7, gain, offset)
        return Decoder.xyz_mix(primaries, 52.37 / 48.0), curves

    @staticmethod
    def rgb_mix_in(standard, bits, full_range=False, alpha=False, gain=None, offset=None, chroma="cosited"):
        """htj2k_tensor_mix_in_rgb (no context, no device): the TensorMixIn that takes tensor channels R', G', B' (nominal
        0 .. 1, times gain[k] plus offset[k]) to Y'CbCr samples of `bits` bits, the inverse of ycbcr_mix with the same
        arguments; alpha: a fourth channel times the peak as component 3.  chroma: "cosited" or "box" """
        mix = TensorMixIn()
        g = None if gain is None else (ctypes.c_float * 3)(*[float(v) for v in gain])
        o = None if offset is None else (ctypes.c_float * 3)(*[float(v) for v in offset])
        _check(load_library().htj2k_tensor_mix_in_rgb(ctypes.byref(mix), int(standard), int(bool(full_range)), int(bits), int(bool(alpha)),
                                                      g, o, _chroma(chroma)), "htj2k_tensor_mix_in_rgb")
        return mix

    @staticmethod
    def xyz_mix_in(primaries, scale=1.0):
        """htj2k_tensor_mix_in_xyz (no context, no device): the TensorMixIn that takes linear R, G, B of the primaries 709
        (also sRGB), 2020 or PRIMARIES_P3D65 with white point D65 to linear XYZ, times scale; the inverse of xyz_mix with
        the reciprocal scale"""
        mix = TensorMixIn()
        L = load_library()
        L.htj2k_tensor_mix_in_xyz.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
        _check(L.htj2k_tensor_mix_in_xyz(ctypes.byref(mix), int(primaries), float(scale)), "htj2k_tensor_mix_in_xyz")
        return mix

    @staticmethod
    def dcp_curves_in(primaries=709, source="srgb", n=4097):
        """(mix_in, curves_in) that take R, G, B of `primaries` in the encoding `source` ("srgb", "bt709", "pq", or "linear"
        for linear light) to the X'Y'Z' of a digital cinema package, the inverse of dcp_curves: the source's decode over
        0 .. 1 with n knots (none for "linear"), the RGB to XYZ matrix with the DCI normalisation 48 / 52.37, the power law
        1 / 2.6 over 0 .. 1 with n knots uniform in the fourth root (root 2), and a gain of 4095.  For xyz12le frames
        (from_tensor) and for rgb48le at 12 bits with mct=0 (encode_tensor), which is how the encoder writes an X'Y'Z'
        codestream: it does not take the XYZ12 layout itself, and the decoder returns such a stream as xyz12le under
        req_pix_fmt"""
        cin = None if source == "linear" else tensor_curve_in(curve_table(source + "_decode", n, 0.0, 1.0), 0.0, float(n - 1))
        cout = tensor_curve_in(curve_table("power", n, 0.0, 1.0, 1.0 / 2.6, root=2), 0.0, float(n - 1), 2)
        return Decoder.xyz_mix_in(primaries, 48.0 / 52.37), tensor_curves_in(cin, cout, 7, 7, 4095.0, 0.0)

    def tensor_last_route(self):
        """the kernels of the last tensor call on this context: 0 none, 1 the fast route, 2 the general one, 3 both, 4 a
        resized call; with a mix 5, 6, 7 (its fast route, general route, both) and 8 (resized); with curves 9, 10, 11 and 12"""
        return _check(self.L.htj2k_tensor_last_route(self.h), "htj2k_tensor_last_route")

    def to_tensor(self, frames, pix_fmt, bits, dtype="float16", layout="NCHW", size=None, origins=None, scale=None, bias=None,
                  on_device=False, out=None, mix=None, curves=None):
        """htj2k_frames_to_tensor: frames of one layout as a torch tensor on this decoder's device, (n, C, h, w) or
        (n, h, w, C): value = sample * scale[c] + bias[c] in binary32, stored as `dtype` (float32, float16 or bfloat16; a
        torch dtype or its name).  size = (w, h) of the window, None: the frames' own; origins: one (ox, oy) or one per
        frame, None: 0, 0.  A frame is a list of numpy planes or a Frame (with on_device: of device addresses).  `out`: a
        contiguous tensor of that dtype and shape to write into.  mix: a TensorMix (tensor_mix, Decoder.ycbcr_mix); the tensor
        then has its K channels, each a linear map of the pixel's components, and scale and bias are not read.
        curves: a TensorCurves (tensor_curves, Decoder.dcp_curves) beside a mix: a transfer curve before the mix and one after it, then gain and offset (htj2k_frames_to_tensor_curves); the
        other five tensor methods take mix= and curves= the same way"""
        import torch
        n = len(frames)
        if isinstance(pix_fmt, str):
            pix_fmt = PIX_NAMES.index(pix_fmt)
        arr, keep = _frame_array(frames, pix_fmt)
        spec = tensor_spec(dtype, layout, size, scale, bias)
        w, h = (arr[0].width, arr[0].height) if size is None else (spec.out_w, spec.out_h)
        elems, nbytes = self.tensor_image_size(pix_fmt, arr[0].width, arr[0].height, bits, spec, mix)
        t = _tensor_out(spec, n, elems // (w * h), w, h, out, self.device_id)
        org, org_p = _origins(origins, n)
        torch.cuda.synchronize()
        _check(self.L.htj2k_frames_to_tensor_curves(self.h, arr, int(on_device), n, int(bits), ctypes.byref(spec), _mix_p(mix),
                                                     _curves_p(curves, mix), org_p,
                                                 ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(n * nbytes)), "htj2k_frames_to_tensor")
        return t

    @staticmethod
    def resize_weights(win, out, filter, x):
        """htj2k_resize_weights (no context, no device): the taps of output index x of an axis that resamples `win`
        source pixels to `out` -> (first source index, [14-bit integer weights]); their sum is 16384"""
        first, q = ctypes.c_int32(), (ctypes.c_uint16 * 129)()
        n = _check(load_library().htj2k_resize_weights(int(win), int(out), _resize_filter(filter), int(x), ctypes.byref(first), q, 129),
                   "htj2k_resize_weights")
        return first.value, [int(v) for v in q[:n]]

    def to_tensor_resized(self, frames, pix_fmt, bits, size, windows=None, filter="triangle", dtype="float16", layout="NCHW", scale=None,
                          bias=None, on_device=False, out=None, mix=None, curves=None):
        """htj2k_frames_to_tensor_resized: a window of every frame resampled to size = (out_w, out_h) on the device, as
        to_tensor gives its crops: (n, C, out_h, out_w) or (n, out_h, out_w, C).  windows: one (ox, oy, ww, wh) or one per
        frame, None: each frame whole; frames of one layout may differ in size.  filter: "nearest" (torch's
        nearest-exact), "bilinear" (antialias=False) or "triangle" (antialias=True), in 14-bit integer weights.  The
        other arguments as to_tensor."""
        import torch
        n = len(frames)
        if isinstance(pix_fmt, str):
            pix_fmt = PIX_NAMES.index(pix_fmt)
        arr, keep = _frame_array(frames, pix_fmt)
        spec, t, nbytes = _resized_out(pix_fmt, bits, dtype, layout, size, scale, bias, n, out, self.device_id, mix)
        win, win_p = _windows(windows, n)
        torch.cuda.synchronize()
        _check(self.L.htj2k_frames_to_tensor_resized_curves(self.h, arr, int(on_device), n, int(bits), ctypes.byref(spec), _mix_p(mix),
                                                     _curves_p(curves, mix), win_p,
                                                         _resize_filter(filter), ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(n * nbytes)),
               "htj2k_frames_to_tensor_resized")
        return t

    def from_tensor(self, t, pix_fmt, bits, layout="NCHW", scale=None, bias=None, mix=None, curves=None):
        """htj2k_tensor_to_frames: the images of a contiguous CUDA tensor t, (n, C, H, W) or (n, H, W, C) of float32,
        float16 or bfloat16, as frames of `pix_fmt` in device memory: sample = rint(element * scale[c] + bias[c]) clamped
        to 0 .. 2^bits - 1, chroma taken at the top-left element of its footprint -> (frames, keep): a ctypes Frame array
        for encode_device, compare, framecrc(on_device=True) and encode_measured(in_on_device=True), and the torch uint8
        tensors that own its planes (bytes of padding are zero).  mix: a TensorMixIn (tensor_mix_in, Decoder.rgb_mix_in);
        the tensor then has its K channels, every component is a linear map of them, a chroma sample is taken or averaged
        as the mix says (htj2k_tensor_to_frames_mix), and scale and bias are not read.  curves: a TensorCurvesIn
        (tensor_curves_in, Decoder.dcp_curves_in) beside a mix: a transfer curve on the tensor's channels before the mix, one
        on the components after it, then gain and offset (htj2k_tensor_to_frames_curves)"""
        import torch
        fmt = PIX_NAMES.index(pix_fmt) if isinstance(pix_fmt, str) else pix_fmt
        spec, n, w, h, nbytes = _tensor_in(t, fmt, bits, layout, scale, bias, self.device_id, mix)
        arr, keep = (Frame * n)(), []
        for i in range(n):
            arr[i].width, arr[i].height, arr[i].pix_fmt = w, h, fmt
            for p, (rows, rowbytes) in enumerate(plane_geometry(fmt, w, h)):
                d = torch.zeros(rows * rowbytes, dtype=torch.uint8, device="cuda:%d" % self.device_id)
                keep.append(d)
                arr[i].data[p] = d.data_ptr()
                arr[i].linesize[p] = rowbytes
        torch.cuda.synchronize()
        curves_p = _curves_in_p(curves, mix, fmt, bits)
        _check(self.L.htj2k_tensor_to_frames_curves(self.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(n * nbytes), n, int(bits),
                                                    ctypes.byref(spec), _mix_in_p(mix), curves_p, arr), "htj2k_tensor_to_frames")
        return arr, keep

    @staticmethod
    def plane_sizes(pix_fmt, width, height):
        """htj2k_frame_plane_sizes (no context, no device): the planes of a width x height frame of a layout
        -> (number of planes, [samples of a row], [rows], [bytes of a row that hold samples]); pal8's second plane is its
        palette, 256 entries of 4 bytes"""
        fmt = PIX_NAMES.index(pix_fmt) if isinstance(pix_fmt, str) else int(pix_fmt)
        pw, ph, rb = (ctypes.c_int * 4)(), (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
        n = _check(load_library().htj2k_frame_plane_sizes(fmt, int(width), int(height), pw, ph, rb), "htj2k_frame_plane_sizes")
        return n, list(pw[:n]), list(ph[:n]), list(rb[:n])

    def resize_frames(self, frames, pix_fmt, bits, size, windows=None, filter="triangle", on_device=False):
        """htj2k_resize_frames: a window of every frame resampled, every plane on its own grid and in integers, to a frame
        of the same layout and of size = (out_w, out_h) in device memory -> (frames, keep), as from_tensor gives them: a
        ctypes Frame array for encode_device, compare, framecrc(on_device=True) and encode_measured(in_on_device=True), and
        the torch uint8 tensors that own its planes (bytes of padding are zero).  windows: one (ox, oy, ww, wh) or one per
        frame, None: each frame whole; the origin lies on the chroma grid; frames of one layout may differ in size.
        filter as to_tensor_resized.  A frame is a list of numpy planes or a Frame (with on_device: of device addresses)"""
        import torch
        n = len(frames)
        fmt = PIX_NAMES.index(pix_fmt) if isinstance(pix_fmt, str) else pix_fmt
        if size is None:
            raise ValueError("size: (out_w, out_h), both at least 1")
        src, keep_src = _frame_array(frames, fmt)
        arr, keep = _device_frames(n, fmt, size[0], size[1], self.device_id)
        win, win_p = _windows(windows, n)
        torch.cuda.synchronize()
        _check(self.L.htj2k_resize_frames(self.h, src, int(on_device), n, int(bits), win_p, _resize_filter(filter), arr), "htj2k_resize_frames")
        return arr, keep

    def compare_ms(self):
        """device ms of the last comparison, checksum or tensor launch(es) (htj2k_compare_ms)"""
        ms = ctypes.c_float()
        _check(self.L.htj2k_compare_ms(self.h, ctypes.byref(ms)), "htj2k_compare_ms")
        return ms.value

    # ---- kernel-level entry points ----
    def idwt(self, plane, border, levels, type_):
        a = np.ascontiguousarray(plane).copy()
        b = (ctypes.c_int * 4)(border[0][0], border[0][1], border[1][0], border[1][1])
        _check(self.L.htj2k_idwt_plane(self.h, a.ctypes.data_as(ctypes.c_void_p), b, levels, type_), "htj2k_idwt_plane")
        return a

    def idwt_bench(self, w, h, levels, type_, nplanes=1, iters=10):
        ms = ctypes.c_float()
        _check(self.L.htj2k_idwt_bench(self.h, w, h, levels, type_, nplanes, iters, ctypes.byref(ms)), "htj2k_idwt_bench")
        return ms.value

    def copy_bench(self, mbytes=512, iters=10):
        """GB/s (read + written) of a plain device-to-device copy kernel on this box: the measured copy ceiling"""
        g = ctypes.c_float()
        _check(self.L.htj2k_copy_bench(self.h, int(mbytes), int(iters), ctypes.byref(g)), "htj2k_copy_bench")
        return g.value

    def mct(self, type_, p0, p1, p2):
        a, b, c = (np.ascontiguousarray(x).copy() for x in (p0, p1, p2))
        _check(self.L.htj2k_mct_planes(self.h, a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p),
                                       c.ctypes.data_as(ctypes.c_void_p), a.size, type_), "htj2k_mct_planes")
        return a, b, c

    def mq_blocks(self, descs, pool, nsamples, dtype=np.int32, raw=False):
        """Part-1 blocks (BlockDesc.flags & 4, bytes + trailer as in j2k_plan.h) -> (samples[nsamples], status[n]);
        raw: the signed quantiser indices instead of dequantised samples (htj2k_mq_blocks_raw)"""
        n = len(descs)
        arr = (BlockDesc * n)(*descs)
        buf = ctypes.create_string_buffer(bytes(pool) + b"\0" * 64, len(pool) + 64)
        out = np.full(nsamples, 0x7FFFFFFF if dtype == np.int32 else np.nan, dtype=dtype)
        status = np.zeros(n, dtype=np.int32)
        fn = self.L.htj2k_mq_blocks_raw if raw else self.L.htj2k_mq_blocks
        _check(fn(self.h, arr, n, buf, ctypes.c_size_t(len(pool) + 64), out.ctypes.data_as(ctypes.c_void_p),
                  ctypes.c_size_t(nsamples), status.ctypes.data_as(ctypes.c_void_p)),
               "htj2k_mq_blocks_raw" if raw else "htj2k_mq_blocks")
        return out, status

    def ht_blocks(self, descs, pool, nsamples, dtype=np.int32, raw=False, route=0, out=None):
        """descs: list of BlockDesc; pool: bytes.  -> (samples[nsamples], status[n]);
        raw: the signed quantiser indices instead of dequantised samples (htj2k_ht_blocks_raw);
        route: knob "unit_ht" for this call (the kernels of a job's routes; 0 again afterwards).  Routes 3 and 4 write
        int16_t samples at the descriptors' offsets: the buffer comes back as an int16 view, 2 * nsamples long;
        out: the caller's buffer, a contiguous array of nsamples 32-bit words that is used in place -- what it holds goes
        to the device before the kernels run, and the caller can look at it after a call that raised (default: a fresh
        one of 0x7FFFFFFF or NaN)"""
        n = len(descs)
        arr = (BlockDesc * n)(*descs)
        buf = ctypes.create_string_buffer(bytes(pool) + b"\0" * 64, len(pool) + 64)
        if out is None:
            out = np.full(nsamples, 0x7FFFFFFF if dtype == np.int32 else np.nan, dtype=dtype)
        elif out.shape != (nsamples,) or out.itemsize != 4 or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("out: a contiguous array of %d 32-bit words wanted" % nsamples)
        status = np.zeros(n, dtype=np.int32)
        fn = self.L.htj2k_ht_blocks_raw if raw else self.L.htj2k_ht_blocks
        self.set_int("unit_ht", route)
        try:
            _check(fn(self.h, arr, n, buf, ctypes.c_size_t(len(pool) + 64), out.ctypes.data_as(ctypes.c_void_p),
                      ctypes.c_size_t(nsamples), status.ctypes.data_as(ctypes.c_void_p)),
                   "htj2k_ht_blocks_raw" if raw else "htj2k_ht_blocks")
        finally:
            self.set_int("unit_ht", 0)
        return (out.view(np.int16) if route in (3, 4) else out), status


# ---------------------------------------------------------------------------------------------- encoder

class EncOpts(ctypes.Structure):
    """struct htj2k_enc_opts (include/htj2k_amd.h)"""
    _fields_ = [("levels", ctypes.c_int), ("cb_w_log2", ctypes.c_int), ("cb_h_log2", ctypes.c_int), ("mct", ctypes.c_int),
                ("guard_bits", ctypes.c_int), ("irreversible", ctypes.c_int), ("qstep", ctypes.c_double),
                ("target_bytes", ctypes.c_int64), ("tile_w", ctypes.c_int), ("tile_h", ctypes.c_int),
                ("ht_passes", ctypes.c_int), ("target_psnr", ctypes.c_double)]

    def __new__(cls, *args, **kw):
        # the view ends at target_psnr, as callers written before group_bytes declare it; the C struct has grown since,
        # and htj2k_enc_opts_default writes the whole of it: every instance lies in a zeroed buffer with room for the tail
        return cls.from_buffer(bytearray(ctypes.sizeof(cls) + 64))


class EncOptsGroup(EncOpts):
    """struct htj2k_enc_opts in full: EncOpts and the tail field group_bytes"""
    _fields_ = [("group_bytes", ctypes.c_int64)]


class EncRc(ctypes.Structure):
    """struct htj2k_enc_rc (include/htj2k_amd.h)"""
    _fields_ = [("target_bytes", ctypes.c_int64), ("est_bytes", ctypes.c_int64), ("final_bytes", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("nblocks", "blocks_left_out", "ht_launches", "blocks_recoded", "trial", "last_resort")]


class EncQuality(ctypes.Structure):
    """struct htj2k_enc_quality (include/htj2k_amd.h)"""
    _fields_ = [(n, ctypes.c_double) for n in ("target_psnr", "base_psnr", "model_psnr", "lambda")] + \
               [(n, ctypes.c_int32) for n in ("short_of_target", "capped")]


class EncGroup(ctypes.Structure):
    """struct htj2k_enc_group (include/htj2k_amd.h)"""
    _fields_ = [("group_bytes", ctypes.c_int64), ("est_bytes", ctypes.c_int64), ("final_bytes", ctypes.c_int64),
                ("lambda", ctypes.c_double)] + \
               [(n, ctypes.c_int32) for n in ("nframes", "nblocks", "frames_capped", "ht_launches", "trial", "last_resort")]


class TranscodeOpts(ctypes.Structure):
    """struct htj2k_transcode_opts"""
    _fields_ = [("target_bytes", ctypes.c_int64)]

    def __new__(cls, *args, **kw):
        # the view ends at target_bytes, as callers written before ht_sources declare it; the C struct has grown since, and
        # htj2k_transcode_opts_default writes the whole of it: every instance lies in a zeroed buffer with room for the tail
        return cls.from_buffer(bytearray(ctypes.sizeof(cls) + 64))


class TranscodeOptsHt(TranscodeOpts):
    """struct htj2k_transcode_opts in full: TranscodeOpts and the tail field ht_sources"""
    _fields_ = [("ht_sources", ctypes.c_int)]


class EncBlock(ctypes.Structure):
    """struct htj2k_enc_block (include/htj2k_amd.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("comp", "res", "band", "x", "y", "w", "h", "expn")]


class EncTile(ctypes.Structure):
    """struct htj2k_enc_tile (include/htj2k_amd.h)"""
    _fields_ = [("blk0", ctypes.c_int32), ("nblk", ctypes.c_int32)] + \
               [(n, ctypes.c_int32 * 4) for n in ("x0", "y0", "x1", "y1")]


class EncQuant(ctypes.Structure):
    """struct htj2k_enc_quant (include/htj2k_amd.h)"""
    _fields_ = [("guard_bits", ctypes.c_int), ("expn", ctypes.c_uint8 * 97 * 4), ("mant", ctypes.c_uint16 * 97 * 4)]


class EncRegion(ctypes.Structure):
    """struct htj2k_enc_region (include/htj2k_amd.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("px", "py", "w", "h", "x0", "y0", "levels")]


def frame_from_planes(planes, pix_fmt, width=None, height=None):
    """(htj2k_frame, arrays it points into) for numpy planes in a decoder output layout: 2-D arrays (packed layouts:
    rows of interleaved samples, as Decoder.decode returns them) of uint8 or uint16.  Keep the arrays alive."""
    if isinstance(pix_fmt, str):
        pix_fmt = PIX_NAMES.index(pix_fmt)
    fr, keep = Frame(), []
    for p, a in enumerate(planes):
        a = np.ascontiguousarray(a)
        keep.append(a)
        fr.data[p] = a.ctypes.data
        fr.linesize[p] = a.strides[0]
    a0 = keep[0]
    if width is None:
        comps = len(planes) if len(planes) > 1 else _PACKED_COMPS.get(pix_fmt, 1)
        width = a0.shape[1] // (1 if len(planes) > 1 else comps)
    fr.width = width
    fr.height = a0.shape[0] if height is None else height
    fr.pix_fmt = pix_fmt
    return fr, keep


_PACKED_COMPS = {1: 3, 2: 4, 3: 3, 4: 4, 5: 1, 6: 2, 7: 1, 8: 2, 42: 3}


def _enc_opts(levels=5, cb=(6, 6), mct=-1, guard_bits=0, irreversible=False, qstep=1.0, target_bytes=0, tile=(0, 0),
              ht_passes=0, target_psnr=0.0, group_bytes=0):
    o = EncOptsGroup()
    o.levels, (o.cb_w_log2, o.cb_h_log2), o.mct, o.guard_bits = levels, cb, mct, guard_bits
    o.irreversible, o.qstep, o.target_bytes = int(irreversible), qstep, int(target_bytes)
    o.tile_w, o.tile_h = tile
    o.ht_passes = int(ht_passes)
    o.target_psnr = float(target_psnr)
    o.group_bytes = int(group_bytes)
    return o


class Encoder:
    """HTJ2K encoder on the GPU (htj2k_enc_*): frames in decoder output layouts in, codestreams out.
    Options: levels (0..32, default 5), cb=(w_log2, h_log2) (default (6, 6)), mct (-1 auto), guard_bits (0 auto),
    irreversible (False: lossless 5/3; True: 9/7 with quantisation), qstep (the 9/7 base step, default 1.0),
    target_bytes (0: off; else the upper limit of each frame's codestream: blocks are coded from higher bit-planes or
    left out until the frame fits, see last_planes / rc_info), tile=(w, h) (nominal tile size; 0 in a direction: one
    tile spans the image there, so (0, 128) gives strips; default (0, 0): one tile), ht_passes (0 or 1: every block is
    one cleanup pass; 2 or 3: the cleanup pass at bit-plane 1 and SigProp, or SigProp and MagRef, at plane 0 -- lossy and
    deterministic; blocks that would gain nothing keep one pass, see last_passes; with target_bytes the allocation chooses among one,
    two and three passes per block instead), target_psnr (0: off; else the PSNR in dB each frame is to reach in the terms of
    the encoder's distortion model with as few bytes as it takes, see quality_info; with target_bytes the budget is a cap),
    group_bytes (0: off; else the upper limit of the codestreams of all frames of one call together: one slope for the
    blocks of all frames, so easy frames give their bytes to hard ones, see group_info; with target_bytes both hold).
    The static methods layout / tiles / assemble / bound need no GPU."""

    def __init__(self, device_id=0):
        self.L = load_library()
        self.h = ctypes.c_void_p()
        _check(self.L.htj2k_enc_open(device_id, ctypes.byref(self.h)), "htj2k_enc_open")
        self.device_id = device_id
        self._logs = []

        @ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p)
        def _log(opaque, level, msg):
            self._logs.append(msg.decode(errors="replace"))

        self._log_cb = _log
        self.L.htj2k_enc_set_log(self.h, self._log_cb, None)

    @staticmethod
    def bound(width, height, pix_fmt, bits, **opts):
        L = load_library()
        L.htj2k_encode_bound.restype = ctypes.c_size_t
        o = _enc_opts(**opts)
        return L.htj2k_encode_bound(width, height, _fmt(pix_fmt), bits, ctypes.byref(o))

    @staticmethod
    def layout(width, height, pix_fmt, bits, **opts):
        """the code-blocks of a frame in the encoder's order: list of dicts comp/res/band/x/y/w/h/expn"""
        L = load_library()
        o = _enc_opts(**opts)
        n = _check(L.htj2k_enc_layout(width, height, _fmt(pix_fmt), bits, ctypes.byref(o), None, 0), "htj2k_enc_layout")
        tab = (EncBlock * max(n, 1))()
        _check(L.htj2k_enc_layout(width, height, _fmt(pix_fmt), bits, ctypes.byref(o), tab, n), "htj2k_enc_layout")
        return [{f: getattr(tab[i], f) for f, _ in EncBlock._fields_} for i in range(n)]

    @staticmethod
    def band_weights(width, height, pix_fmt, bits, **opts):
        """the weight of every block's band in layout()'s order (float64): squared error of the output pixels per unit of
        squared error of the block's quantisation indices, what rate control and constant quality weigh distortions by"""
        L = load_library()
        o = _enc_opts(**opts)
        n = _check(L.htj2k_enc_band_weights(width, height, _fmt(pix_fmt), bits, ctypes.byref(o), None, 0), "htj2k_enc_band_weights")
        w = np.zeros(max(n, 1), dtype=np.float64)
        _check(L.htj2k_enc_band_weights(width, height, _fmt(pix_fmt), bits, ctypes.byref(o), w.ctypes.data_as(ctypes.c_void_p), n),
               "htj2k_enc_band_weights")
        return w[:n]

    @staticmethod
    def tiles(width, height, pix_fmt, bits, **opts):
        """the tiles of a frame in codestream order: list of dicts blk0 / nblk (the tile's blocks in layout()'s order) and
        rects, per component the tile-component's (x0, y0, x1, y1) in the component plane"""
        L = load_library()
        o = _enc_opts(**opts)
        n = _check(L.htj2k_enc_tiles(width, height, _fmt(pix_fmt), bits, ctypes.byref(o), None, 0), "htj2k_enc_tiles")
        tab = (EncTile * max(n, 1))()
        _check(L.htj2k_enc_tiles(width, height, _fmt(pix_fmt), bits, ctypes.byref(o), tab, n), "htj2k_enc_tiles")
        return [{"blk0": t.blk0, "nblk": t.nblk, "rects": [(t.x0[c], t.y0[c], t.x1[c], t.y1[c]) for c in range(4)]}
                for t in tab[:n]]

    @staticmethod
    def assemble(width, height, pix_fmt, bits, blocks, max_u=None, cap=None, planes=None, lref=None, passes=None, **opts):
        """codestream from caller-coded blocks: blocks[i] = bytes of block i's cleanup segment (b"" = left out), one
        entry per block of layout(); max_u: None or one entry per block; planes: None, or per block the bit-plane it
        was coded from (sign * (|v| >> p); -1 for a block that is left out).  lref and passes (both or neither): per
        block the bytes of its refinement segment, the last lref[i] of blocks[i], and its passes 1 .. 3; planes[i] is
        then the plane of the refinement passes (the cleanup pass coded the one above)"""
        L = load_library()
        o = _enc_opts(**opts)
        n = len(blocks)
        if max_u is not None and len(max_u) != n:
            raise ValueError("max_u has %d entries for %d blocks" % (len(max_u), n))
        bufs = [ctypes.create_string_buffer(bytes(b), max(len(b), 1)) for b in blocks]
        ptrs = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
        lc = (ctypes.c_int * max(n, 1))(*[len(b) for b in blocks])
        mu = None if max_u is None else (ctypes.c_int * max(n, 1))(*max_u)
        if planes is not None and len(planes) != n:
            raise ValueError("planes has %d entries for %d blocks" % (len(planes), n))
        pl = None if planes is None else (ctypes.c_int * max(n, 1))(*[int(p) for p in planes])
        if cap is None:
            cap = Encoder.bound(width, height, pix_fmt, bits, **opts)
        out = ctypes.create_string_buffer(max(cap, 1))
        ln = ctypes.c_size_t()
        if (lref is None) != (passes is None):
            raise ValueError("lref and passes go together")
        if passes is not None:
            if len(lref) != n or len(passes) != n:
                raise ValueError("lref / passes have %d / %d entries for %d blocks" % (len(lref), len(passes), n))
            lc = (ctypes.c_int * max(n, 1))(*[len(b) - int(r) for b, r in zip(blocks, lref)])
            lr = (ctypes.c_int * max(n, 1))(*[int(r) for r in lref])
            ps = (ctypes.c_int * max(n, 1))(*[int(k) for k in passes])
            _check(L.htj2k_enc_assemble_passes(width, height, _fmt(pix_fmt), bits, ctypes.byref(o), ptrs, lc, lr, ps, mu, pl, n,
                                               out, ctypes.c_size_t(cap), ctypes.byref(ln)), "htj2k_enc_assemble_passes")
        elif pl is None:
            _check(L.htj2k_enc_assemble(width, height, _fmt(pix_fmt), bits, ctypes.byref(o), ptrs, lc, mu, n, out,
                                        ctypes.c_size_t(cap), ctypes.byref(ln)), "htj2k_enc_assemble")
        else:
            _check(L.htj2k_enc_assemble_planes(width, height, _fmt(pix_fmt), bits, ctypes.byref(o), ptrs, lc, mu, pl, n, out,
                                               ctypes.c_size_t(cap), ctypes.byref(ln)), "htj2k_enc_assemble_planes")
        return out.raw[:ln.value]

    @staticmethod
    def assemble_quant(width, height, pix_fmt, bits, blocks, lref, passes, planes, guard_bits, expn, mant=None, cap=None, **opts):
        """assemble() with the quantisation given (htj2k_enc_assemble_quant): guard_bits, and expn / mant as
        [component][band] lists (band 0 LL, then HL LH HH from the lowest resolution up; mant None: all 0)"""
        L = load_library()
        o = _enc_opts(**opts)
        q = EncQuant()
        q.guard_bits = guard_bits
        for c, row in enumerate(expn):
            for b, e in enumerate(row):
                q.expn[c][b] = int(e)
                q.mant[c][b] = int(mant[c][b]) if mant is not None else 0
        n = len(blocks)
        bufs = [ctypes.create_string_buffer(bytes(b), max(len(b), 1)) for b in blocks]
        ptrs = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
        lc = (ctypes.c_int * max(n, 1))(*[len(b) - int(r) for b, r in zip(blocks, lref)])
        lr = (ctypes.c_int * max(n, 1))(*[int(r) for r in lref])
        ps = (ctypes.c_int * max(n, 1))(*[int(k) for k in passes])
        pl = (ctypes.c_int * max(n, 1))(*[int(k) for k in planes])
        if cap is None:
            cap = Encoder.bound(width, height, pix_fmt, bits, **dict(opts, ht_passes=3))
        out = ctypes.create_string_buffer(max(cap, 1))
        ln = ctypes.c_size_t()
        _check(L.htj2k_enc_assemble_quant(width, height, _fmt(pix_fmt), bits, ctypes.byref(o), ctypes.byref(q), ptrs, lc, lr, ps,
                                          pl, n, out, ctypes.c_size_t(cap), ctypes.byref(ln)), "htj2k_enc_assemble_quant")
        return out.raw[:ln.value]

    @staticmethod
    def _transcode_check(data, ht_sources, want_min):
        """htj2k_transcode_check / htj2k_transcode_min_size; with ht_sources htj2k_transcode_check_opts"""
        L = load_library()
        logs = []

        @ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p)
        def _log(opaque, level, msg):
            logs.append(msg.decode(errors="replace"))

        buf, size = data if isinstance(data, tuple) else packet(data)
        bound, least = ctypes.c_size_t(), ctypes.c_int64()
        if ht_sources:
            name = "htj2k_transcode_check_opts"
            o = TranscodeOptsHt(0, int(ht_sources))
            r = L.htj2k_transcode_check_opts(buf, size, ctypes.byref(o), None if want_min else ctypes.byref(bound),
                                             ctypes.byref(least) if want_min else None, _log, None)
        elif want_min:
            name = "htj2k_transcode_min_size"
            r = L.htj2k_transcode_min_size(buf, size, ctypes.byref(least), _log, None)
        else:
            name = "htj2k_transcode_check"
            r = L.htj2k_transcode_check(buf, size, ctypes.byref(bound), _log, None)
        if r < 0:
            raise Htj2kError(r, name + (": " + "".join(logs).strip() if logs else ""))
        return least.value if want_min else bound.value

    @staticmethod
    def transcode_check(data, ht_sources=False):
        """htj2k_transcode_check (no GPU needed): the worst-case size of the HTJ2K stream htj2k_transcode_* writes for this
        Part-1 codestream (or JP2 file); raises Htj2kError, with the log line, for a stream that is out of scope.
        ht_sources: HT and MIXED streams are in scope (htj2k_transcode_check_opts)"""
        return Encoder._transcode_check(data, ht_sources, False)

    @staticmethod
    def transcode_min_size(data, ht_sources=False):
        """htj2k_transcode_min_size (no GPU needed): the smallest stream a transcode budget may name for this source;
        raises as transcode_check does"""
        return Encoder._transcode_check(data, ht_sources, True)

    def transcode(self, decoder, packets, cap=None, out_on_device=False, target_bytes=0, ht_sources=False):
        """Part-1 codestreams (bytes; with ht_sources HT and MIXED ones too) -> [HTJ2K codestream bytes] that decode to the same coefficients; `decoder` is a
        Decoder on the same device.  One call for all of them (htj2k_transcode_batch).  cap: the output buffer's size
        (None: the sum of transcode_check's bounds); out_on_device: the streams are written to device memory (a torch
        uint8 tensor) and fetched from there.  target_bytes (0: off): the upper limit of every frame's stream; a frame
        beyond it gets blocks in their source's form or a coarser one (htj2k_transcode_batch_opts; last_planes,
        last_passes, rc_info)"""
        n = len(packets)
        pk = [packet(d) for d in packets]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p) for b, _ in pk])
        sizes = (ctypes.c_int * n)(*[sz for _, sz in pk])
        if cap is None:
            cap = sum(Encoder.transcode_check(d, ht_sources) for d in packets)
        offs = (ctypes.c_size_t * (n + 1))()
        self._logs.clear()
        if out_on_device:
            import torch
            dev = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dst = ctypes.c_void_p(dev.data_ptr())
        else:
            out = np.zeros(max(cap, 1), dtype=np.uint8)
            dst = out.ctypes.data_as(ctypes.c_void_p)
        if target_bytes or ht_sources:
            o = TranscodeOptsHt(int(target_bytes), int(ht_sources))
            r = self.L.htj2k_transcode_batch_opts(decoder.h, self.h, ptrs, sizes, n, ctypes.byref(o), dst, ctypes.c_size_t(cap),
                                                  int(out_on_device), offs)
        else:
            r = self.L.htj2k_transcode_batch(decoder.h, self.h, ptrs, sizes, n, dst, ctypes.c_size_t(cap), int(out_on_device), offs)
        if out_on_device:
            out = dev.cpu().numpy()
        self.last_out = out
        if r < 0:
            raise Htj2kError(r, "htj2k_transcode_batch" + (": " + "".join(self._logs).strip() if self._logs else ""))
        return [out[offs[i]:offs[i + 1]].tobytes() for i in range(n)]

    def transcode_into(self, decoder, ptrs, sizes, n, out, cap, offs, out_on_device=0, target_bytes=0, ht_sources=False):
        """htj2k_transcode_batch (target_bytes: htj2k_transcode_batch_opts) on prepared ctypes arguments (timing loops:
        nothing is allocated here)"""
        if target_bytes or ht_sources:
            o = TranscodeOptsHt(int(target_bytes), int(ht_sources))
            return _check(self.L.htj2k_transcode_batch_opts(decoder.h, self.h, ptrs, sizes, n, ctypes.byref(o), out,
                                                            ctypes.c_size_t(cap), out_on_device, offs), "htj2k_transcode_batch_opts")
        return _check(self.L.htj2k_transcode_batch(decoder.h, self.h, ptrs, sizes, n, out, ctypes.c_size_t(cap), out_on_device,
                                                   offs), "htj2k_transcode_batch")

    def last_rounds(self):
        """rounds the last encode_batch / transcode went through (htj2k_enc_last_rounds)"""
        return _check(self.L.htj2k_enc_last_rounds(self.h), "htj2k_enc_last_rounds")

    def transcode_stage_ms(self):
        """device ms of the Part-1 block stage, the plane scatter, the HT stage and the gather of the last transcode"""
        ms = (ctypes.c_float * 4)()
        _check(self.L.htj2k_transcode_stage_ms(self.h, ms), "htj2k_transcode_stage_ms")
        return list(ms)

    def encode(self, planes, pix_fmt, bits, **opts):
        """one frame (numpy planes, see frame_from_planes) -> codestream bytes"""
        return self.encode_batch([planes], pix_fmt, bits, **opts)[0]

    def encode_batch(self, frames, pix_fmt, bits, **opts):
        """several frames of one layout (sizes may differ) -> [codestream bytes], one call"""
        made = [frame_from_planes(p, pix_fmt) for p in frames]
        return self._batch([f for f, _ in made], pix_fmt, bits, False, **opts)

    def encode_device(self, frames, pix_fmt, bits, **opts):
        """frames whose planes are in device memory: [htj2k_frame], e.g. from htj2k_job_device_frame"""
        return self._batch(frames, pix_fmt, bits, True, **opts)

    def _batch(self, frames, pix_fmt, bits, on_device, **opts):
        n = len(frames)
        arr = (Frame * n)(*frames)
        for i in range(n):
            arr[i].pix_fmt = _fmt(pix_fmt)
        cap = sum(Encoder.bound(f.width, f.height, pix_fmt, bits, **opts) for f in frames)
        o = _enc_opts(**opts)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        offs = (ctypes.c_size_t * (n + 1))()
        self._logs.clear()
        r = self.L.htj2k_encode_batch(self.h, arr, n, bits, ctypes.byref(o), int(on_device),
                                      out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap), 0, offs)
        if r < 0:
            raise Htj2kError(r, "htj2k_encode_batch" + (": " + "".join(self._logs).strip() if self._logs else ""))
        return [out[offs[i]:offs[i + 1]].tobytes() for i in range(n)]

    def encode_tensor(self, t, pix_fmt, bits, layout="NCHW", scale=None, bias=None, mix=None, curves=None, **opts):
        """htj2k_encode_tensor: the images of a contiguous CUDA tensor t, (n, C, H, W) or (n, H, W, C) of float32, float16
        or bfloat16 on the encoder's device -> [codestream bytes], the streams of encode_device(Decoder.from_tensor(t, ...))
        without the frames: the encoder's first stage reads the tensor.  sample = rint(element * scale[c] + bias[c])
        clamped to 0 .. 2^bits - 1 (scale None: 1, bias None: 0; one number, or one per component).  mix: a TensorMixIn
        (tensor_mix_in, Decoder.rgb_mix_in): the tensor has its K channels and goes through the colour matrix and chroma
        rule inside the same stage (htj2k_encode_tensor_mix); scale and bias are then not read.  curves: a TensorCurvesIn
        beside a mix, as Decoder.from_tensor takes it (htj2k_encode_tensor_curves)"""
        import torch
        spec, n, w, h, nbytes = _tensor_in(t, pix_fmt, bits, layout, scale, bias, self.device_id, mix)
        cap = n * Encoder.bound(w, h, pix_fmt, bits, **opts)
        o = _enc_opts(**opts)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        offs = (ctypes.c_size_t * (n + 1))()
        self._logs.clear()
        torch.cuda.synchronize()
        r = self.L.htj2k_encode_tensor_curves(self.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(n * nbytes), n, w, h, _fmt(pix_fmt),
                                              int(bits), ctypes.byref(spec), _mix_in_p(mix), _curves_in_p(curves, mix, _fmt(pix_fmt), bits), ctypes.byref(o),
                                              out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap), 0, offs)
        if r < 0:
            raise Htj2kError(r, "htj2k_encode_tensor" + (": " + "".join(self._logs).strip() if self._logs else ""))
        return [out[offs[i]:offs[i + 1]].tobytes() for i in range(n)]

    def encode_measured(self, decoder, frames, pix_fmt, bits, close_loop=False, max_rounds=0, in_on_device=False,
                        out_on_device=False, cap=None, ssim=False, **opts):
        """htj2k_encode_batch_measured: encode_batch, and every stream decoded by `decoder` (a Decoder on the same device)
        and compared with its input on the device -> (streams, [dict]): per frame diff (as Decoder.compare), first_psnr,
        target_used, rounds, fell_back, short_measured.  close_loop with target_psnr: frames that measure short of the
        target are encoded again with a moved target, for up to max_rounds quality rounds (0: the default).  frames:
        lists of numpy planes, or Frames (with in_on_device: of device addresses); out_on_device: the streams are written
        to device memory (a torch uint8 tensor) and fetched from there.  ssim: every dict gains "ssim", the final
        stream's structural similarity as Decoder.compare_ssim gives it (htj2k_enc_measure_ssim for this call)"""
        arr, keep = _frame_array(frames, _fmt(pix_fmt))
        n = len(frames)
        for i in range(n):
            arr[i].pix_fmt = _fmt(pix_fmt)
        if cap is None:
            cap = sum(Encoder.bound(arr[i].width, arr[i].height, pix_fmt, bits, **opts) for i in range(n))
        o = _enc_opts(**opts)
        mo = EncMeasureOpts(int(close_loop), int(max_rounds))
        offs = (ctypes.c_size_t * (n + 1))()
        res = (EncMeasured * max(n, 1))()
        self._logs.clear()
        if out_on_device:
            import torch
            dev = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dst = ctypes.c_void_p(dev.data_ptr())
        else:
            out = np.zeros(max(cap, 1), dtype=np.uint8)
            dst = out.ctypes.data_as(ctypes.c_void_p)
        _check(self.L.htj2k_enc_measure_ssim(self.h, int(bool(ssim))), "htj2k_enc_measure_ssim")
        r = self.L.htj2k_encode_batch_measured(decoder.h, self.h, arr, n, bits, ctypes.byref(o), ctypes.byref(mo),
                                               int(in_on_device), dst, ctypes.c_size_t(cap), int(out_on_device), offs, res)
        if ssim:
            self.L.htj2k_enc_measure_ssim(self.h, 0)
        if r < 0:
            raise Htj2kError(r, "htj2k_encode_batch_measured" + (": " + "".join(self._logs).strip() if self._logs else ""))
        if out_on_device:
            out = dev.cpu().numpy()
        info = [dict(diff=res[i].diff.as_dict(), first_psnr=res[i].first_psnr, target_used=res[i].target_used,
                     rounds=res[i].rounds, fell_back=res[i].fell_back, short_measured=res[i].short_measured) for i in range(n)]
        for i in range(n if ssim else 0):
            info[i]["ssim"] = self.last_ssim(i)
        return [out[offs[i]:offs[i + 1]].tobytes() for i in range(n)], info

    def last_ssim(self, frame):
        """htj2k_enc_last_ssim: frame's figures from the last encode_measured(..., ssim=True) -> dict as Decoder.compare_ssim"""
        s = FrameSsim()
        _check(self.L.htj2k_enc_last_ssim(self.h, int(frame), ctypes.byref(s)), "htj2k_enc_last_ssim")
        return s.as_dict()

    def encode_into(self, frames, n, bits, opts, out, cap, offs, in_on_device=0, out_on_device=0):
        """htj2k_encode_batch on prepared ctypes arguments (timing loops: nothing is allocated here)"""
        return _check(self.L.htj2k_encode_batch(self.h, frames, n, bits, ctypes.byref(opts), in_on_device, out,
                                                ctypes.c_size_t(cap), out_on_device, offs), "htj2k_encode_batch")

    def stage_ms(self):
        """device ms of unpack + RCT, forward DWT, HT cleanup, gather in the last batch"""
        ms = (ctypes.c_float * 4)()
        _check(self.L.htj2k_enc_stage_ms(self.h, ms), "htj2k_enc_stage_ms")
        return list(ms)

    def ht_cycles(self):
        """(blocks counted, [cycles of exponents + contexts, MagSgn packing, 0xFF pass, MEL + VLC, copy-out]) of the last
        HT cleanup launch; needs HTJ2K_ENC_STAMPS=1 in the environment when the Encoder is made"""
        cyc = (ctypes.c_uint64 * 5)()
        n = _check(self.L.htj2k_enc_ht_cycles(self.h, cyc), "htj2k_enc_ht_cycles")
        return n, list(cyc)

    def fdwt_plane(self, plane, levels):
        """forward 5/3 of an int32 plane (numpy, h x w) -> new array in the Mallat layout"""
        a = np.ascontiguousarray(plane, dtype=np.int32).copy()
        _check(self.L.htj2k_fdwt_plane(self.h, a.ctypes.data_as(ctypes.c_void_p), a.shape[1], a.shape[0], levels),
               "htj2k_fdwt_plane")
        return a

    def fdwt97_plane(self, plane, levels):
        """forward 9/7 of a float32 plane (numpy, h x w) -> new float32 array in the Mallat layout"""
        a = np.ascontiguousarray(plane, dtype=np.float32).copy()
        _check(self.L.htj2k_fdwt97_plane(self.h, a.ctypes.data_as(ctypes.c_void_p), a.shape[1], a.shape[0], levels),
               "htj2k_fdwt97_plane")
        return a

    def fdwt_regions(self, plane, regions, irreversible=False):
        """forward 5/3 (int32) or 9/7 (float32, irreversible) of regions of a plane, each a tile-component that starts at
        (x0, y0): regions = [(px, py, w, h, x0, y0, levels)], (px, py) where it lies in the plane -> new array"""
        a = np.ascontiguousarray(plane, dtype=np.float32 if irreversible else np.int32).copy()
        tab = (EncRegion * max(len(regions), 1))(*[EncRegion(*[int(v) for v in r]) for r in regions])
        _check(self.L.htj2k_fdwt_regions(self.h, a.ctypes.data_as(ctypes.c_void_p), a.shape[1], a.shape[0], tab,
                                         len(regions), int(irreversible)), "htj2k_fdwt_regions")
        return a

    def ht_encode_blocks(self, plane, rects, planes=None, passes=None):
        """HT cleanup encoding of blocks (x, y, w, h) of an int32 plane -> [(bytes, lcup, max_u)]; planes: None, or per
        block the bit-plane p it is coded from (sign * (|v| >> p)).  passes: None, or per block 1 .. 3 -> [(bytes, lcup,
        lref, max_u)], bytes the cleanup segment (coded from plane p + 1 where the block has more than one pass) and the
        refinement segment at plane p behind it; lref 0: the block has one pass"""
        a = np.ascontiguousarray(plane, dtype=np.int32)
        n = len(rects)
        tab = (EncBlock * max(n, 1))()
        for i, (x, y, w, h) in enumerate(rects):
            tab[i].x, tab[i].y, tab[i].w, tab[i].h = x, y, w, h
        ref = [0] * n if passes is None else [(w * h * 2 + 6) // 7 + 2 if int(k) > 1 else 0 for (_, _, w, h), k in zip(rects, passes)]
        cap = sum(((w * h * 32 + 6) // 7 + 4080 + r + 15) // 16 * 16 for (_, _, w, h), r in zip(rects, ref)) + 16
        out = np.zeros(cap, dtype=np.uint8)
        offs = (ctypes.c_size_t * (n + 1))()
        lc, mu = (ctypes.c_int * max(n, 1))(), (ctypes.c_int * max(n, 1))()
        if planes is not None and len(planes) != n:
            raise ValueError("planes has %d entries for %d blocks" % (len(planes), n))
        if passes is not None:
            if len(passes) != n:
                raise ValueError("passes has %d entries for %d blocks" % (len(passes), n))
            pl = None if planes is None else (ctypes.c_int * max(n, 1))(*[int(p) for p in planes])
            ps = (ctypes.c_int * max(n, 1))(*[int(k) for k in passes])
            lr = (ctypes.c_int * max(n, 1))()
            _check(self.L.htj2k_ht_encode_blocks_passes(self.h, a.ctypes.data_as(ctypes.c_void_p), a.shape[1], a.shape[0], tab,
                                                        n, pl, ps, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap),
                                                        offs, lc, lr, mu), "htj2k_ht_encode_blocks_passes")
            return [(out[offs[i]:offs[i] + lc[i] + lr[i]].tobytes(), lc[i], lr[i], mu[i]) for i in range(n)]
        if planes is None:
            _check(self.L.htj2k_ht_encode_blocks(self.h, a.ctypes.data_as(ctypes.c_void_p), a.shape[1], a.shape[0], tab, n,
                                                 out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap), offs, lc, mu),
                   "htj2k_ht_encode_blocks")
        else:
            pl = (ctypes.c_int * max(n, 1))(*[int(p) for p in planes])
            _check(self.L.htj2k_ht_encode_blocks_planes(self.h, a.ctypes.data_as(ctypes.c_void_p), a.shape[1], a.shape[0], tab,
                                                        n, pl, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap),
                                                        offs, lc, mu), "htj2k_ht_encode_blocks_planes")
        return [(out[offs[i]:offs[i] + lc[i]].tobytes(), lc[i], mu[i]) for i in range(n)]

    def rc_stats(self, plane, rects, nplanes=16):
        """what the rate allocation reads for blocks (x, y, w, h) of an int32 plane -> (dist uint64[n, nplanes],
        len_est uint32[n, nplanes]): distortion and estimated cleanup bytes of dropping p bit-planes"""
        a = np.ascontiguousarray(plane, dtype=np.int32)
        n = len(rects)
        tab = (EncBlock * max(n, 1))()
        for i, (x, y, w, h) in enumerate(rects):
            tab[i].x, tab[i].y, tab[i].w, tab[i].h = x, y, w, h
        dist = np.zeros((n, nplanes), dtype=np.uint64)
        ln = np.zeros((n, nplanes), dtype=np.uint32)
        _check(self.L.htj2k_enc_rc_stats(self.h, a.ctypes.data_as(ctypes.c_void_p), a.shape[1], a.shape[0], tab, n, nplanes,
                                         dist.ctypes.data_as(ctypes.c_void_p), ln.ctypes.data_as(ctypes.c_void_p)),
               "htj2k_enc_rc_stats")
        return dist, ln

    def rc_stats_passes(self, plane, rects, nplanes=16):
        """the candidates of more than one pass of blocks (x, y, w, h) of an int32 plane -> (dist2, dist3 uint64[n, nplanes],
        sp_bits, mr_bits uint32[n, nplanes]): exact distortion of "cleanup at p + 1, SigProp at p" and of "... and MagRef
        at p", and the bits the two passes write; all 0 where nothing is significant at plane p + 1"""
        a = np.ascontiguousarray(plane, dtype=np.int32)
        n = len(rects)
        tab = (EncBlock * max(n, 1))()
        for i, (x, y, w, h) in enumerate(rects):
            tab[i].x, tab[i].y, tab[i].w, tab[i].h = x, y, w, h
        d2, d3 = np.zeros((n, nplanes), dtype=np.uint64), np.zeros((n, nplanes), dtype=np.uint64)
        sp, mr = np.zeros((n, nplanes), dtype=np.uint32), np.zeros((n, nplanes), dtype=np.uint32)
        _check(self.L.htj2k_enc_rc_stats_passes(self.h, a.ctypes.data_as(ctypes.c_void_p), a.shape[1], a.shape[0], tab, n, nplanes,
                                                *[x.ctypes.data_as(ctypes.c_void_p) for x in (d2, d3, sp, mr)]),
               "htj2k_enc_rc_stats_passes")
        return d2, d3, sp, mr

    def xc_rc_tables(self, plane, rects, src_plane, src_passes, nplanes=16):
        """the tables a budgeted transcode selects from (htj2k_xc_rc_tables), for blocks (x, y, w, h) of an int32 plane of
        indices whose source gave block i its last pass at plane src_plane[i] with src_passes[i] HT passes -> (dist,
        len_est, dist2, dist3, sp_bits, mr_bits [n, nplanes] as rc_stats / rc_stats_passes, in planes relative to
        src_plane and with 2^64 - 1 where the source cannot back a candidate; own_len uint32[n]: the estimate of the
        block's own form)"""
        a = np.ascontiguousarray(plane, dtype=np.int32)
        n = len(rects)
        tab = (EncBlock * max(n, 1))()
        for i, (x, y, w, h) in enumerate(rects):
            tab[i].x, tab[i].y, tab[i].w, tab[i].h = x, y, w, h
        bp = (ctypes.c_int * max(n, 1))(*[int(v) for v in src_plane])
        bk = (ctypes.c_int * max(n, 1))(*[int(v) for v in src_passes])
        d, d2, d3 = (np.zeros((n, nplanes), dtype=np.uint64) for _ in range(3))
        ln, sp, mr = (np.zeros((n, nplanes), dtype=np.uint32) for _ in range(3))
        own = np.zeros(max(n, 1), dtype=np.uint32)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        _check(self.L.htj2k_xc_rc_tables(self.h, vp(a), a.shape[1], a.shape[0], tab, n, bp, bk, nplanes, vp(d), vp(ln), vp(d2),
                                         vp(d3), vp(sp), vp(mr), vp(own)), "htj2k_xc_rc_tables")
        return d, ln, d2, d3, sp, mr, own[:n]

    def rc_base(self, plane, rects, steps):
        """the error of the 9/7 quantiser itself for blocks (x, y, w, h) of a float32 plane of coefficients, steps[i] the
        step of block i's band -> float64[n]: per block the sum of e^2 in index units, e = c - (m + 1/2) where the
        index m = floor(c) > 0 and e = c where m = 0, c = |v| / step"""
        a = np.ascontiguousarray(plane, dtype=np.float32)
        n = len(rects)
        tab = (EncBlock * max(n, 1))()
        for i, (x, y, w, h) in enumerate(rects):
            tab[i].x, tab[i].y, tab[i].w, tab[i].h = x, y, w, h
        st = np.ascontiguousarray(steps, dtype=np.float32)
        if st.size != n:
            raise ValueError("steps has %d entries for %d blocks" % (st.size, n))
        base = np.zeros(max(n, 1), dtype=np.float64)
        _check(self.L.htj2k_enc_rc_base(self.h, a.ctypes.data_as(ctypes.c_void_p), a.shape[1], a.shape[0], tab, n,
                                        st.ctypes.data_as(ctypes.c_void_p), base.ctypes.data_as(ctypes.c_void_p)),
               "htj2k_enc_rc_base")
        return base[:n]

    def quality_info(self, i=0):
        """dict of struct htj2k_enc_quality for frame i of the last batch: target_psnr, base_psnr, model_psnr, lambda,
        short_of_target, capped"""
        info = EncQuality()
        _check(self.L.htj2k_enc_quality_info(self.h, i, ctypes.byref(info)), "htj2k_enc_quality_info")
        return {f: getattr(info, f) for f, _ in EncQuality._fields_}

    def group_info(self):
        """dict of struct htj2k_enc_group for the last batch: group_bytes, est_bytes, final_bytes, lambda, nframes, nblocks,
        frames_capped, ht_launches, trial, last_resort; all 0 after a call without group_bytes"""
        info = EncGroup()
        _check(self.L.htj2k_enc_group_info(self.h, ctypes.byref(info)), "htj2k_enc_group_info")
        return {f: getattr(info, f) for f, _ in EncGroup._fields_}

    def group_stage_ms(self):
        """device ms of the group selection's kernels in the last batch, all their runs"""
        ms = ctypes.c_float()
        _check(self.L.htj2k_enc_group_stage_ms(self.h, ctypes.byref(ms)), "htj2k_enc_group_stage_ms")
        return ms.value

    def rc_group_select(self, nblk, kmax, dist, lens, dskip, low0, weight, scale=None, floor=None, room=0, allow_trial=True):
        """the group selection on caller-made tables (htj2k_enc_rc_group_select): nblk[f] blocks per frame, concatenated;
        dist uint64[n, 16], lens uint32[n, 16] -> (planes int32[n], lambda, est, trial)"""
        def arr(a, dt):
            return None if a is None else np.ascontiguousarray(a, dtype=dt)

        def ptr(a):
            return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

        nb = arr(nblk, np.int32)
        t = [arr(kmax, np.int32), arr(dist, np.uint64), arr(lens, np.uint32), arr(dskip, np.float64), arr(low0, np.uint32),
             arr(weight, np.float64), arr(scale, np.float64), arr(floor, np.float64)]
        planes = np.zeros(max(int(nb.sum()), 1), dtype=np.int32)
        lam, est, trial = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_int()
        _check(self.L.htj2k_enc_rc_group_select(self.h, len(nb), ptr(nb), *[ptr(a) for a in t], ctypes.c_int64(int(room)),
                                                int(allow_trial), ptr(planes), ctypes.byref(lam), ctypes.byref(est),
                                                ctypes.byref(trial)), "htj2k_enc_rc_group_select")
        return planes[:int(nb.sum())], lam.value, est.value, trial.value

    def quality_stage_ms(self):
        """device ms of k_rc_base97 and of the quality runs of the select kernel in the last batch"""
        ms = (ctypes.c_float * 2)()
        _check(self.L.htj2k_enc_quality_stage_ms(self.h, ms), "htj2k_enc_quality_stage_ms")
        return list(ms)

    def last_planes(self, i=0):
        """the bit-plane chosen for every block of frame i of the last batch, in layout()'s order (-1: left out)"""
        n = _check(self.L.htj2k_enc_last_planes(self.h, i, None, 0), "htj2k_enc_last_planes")
        pl = (ctypes.c_int * max(n, 1))()
        _check(self.L.htj2k_enc_last_planes(self.h, i, pl, n), "htj2k_enc_last_planes")
        return list(pl[:n])

    def last_passes(self, i=0):
        """the passes every block of frame i of the last batch got, in layout()'s order (1 .. 3); last_planes gives the
        plane of a block's last pass"""
        n = _check(self.L.htj2k_enc_last_passes(self.h, i, None, 0), "htj2k_enc_last_passes")
        ps = (ctypes.c_int * max(n, 1))()
        _check(self.L.htj2k_enc_last_passes(self.h, i, ps, n), "htj2k_enc_last_passes")
        return list(ps[:n])

    def ref_stage_ms(self):
        """device ms of [k_ht_refine_plan + k_ht_refine_encode of the first HT launch, k_rc_stats_passes] in the last
        batch; those of the correction rounds are rc_stage_ms' third figure"""
        ms = (ctypes.c_float * 2)()
        _check(self.L.htj2k_enc_ref_stage_ms(self.h, ms), "htj2k_enc_ref_stage_ms")
        return list(ms)

    def ref_cycles(self):
        """(blocks counted, [cycles of the map, membership, SigProp bits, 0xFF pass, MagRef bits, MagRef bytes + copy-out])
        of the last k_ht_refine_encode; needs HTJ2K_ENC_STAMPS=1 in the environment when the Encoder is made"""
        cyc = (ctypes.c_uint64 * 6)()
        n = _check(self.L.htj2k_enc_ref_cycles(self.h, cyc), "htj2k_enc_ref_cycles")
        return n, list(cyc)

    def rc_info(self, i=0):
        """dict of struct htj2k_enc_rc for frame i of the last batch: target_bytes, est_bytes, final_bytes, nblocks,
        blocks_left_out, ht_launches, blocks_recoded, trial, last_resort"""
        info = EncRc()
        _check(self.L.htj2k_enc_rc_info(self.h, i, ctypes.byref(info)), "htj2k_enc_rc_info")
        return {f: getattr(info, f) for f, _ in EncRc._fields_}

    def rc_stage_ms(self):
        """device ms of k_rc_stats, k_rc_select and the HT launches of the correction rounds in the last batch"""
        ms = (ctypes.c_float * 3)()
        _check(self.L.htj2k_enc_rc_stage_ms(self.h, ms), "htj2k_enc_rc_stage_ms")
        return list(ms)

    def close(self):
        if self.h:
            self.L.htj2k_enc_close(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fmt(pix_fmt):
    return PIX_NAMES.index(pix_fmt) if isinstance(pix_fmt, str) else int(pix_fmt)
