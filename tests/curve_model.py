"""numpy restatement of the tensor calls with transfer curves (include/htj2k_amd.h "frames as tensors, with curves",
csrc/curve_kernels.hpp): the mix calls' source values (mix_model, tensor_model, resize_model), a curve before the mix on the
components of in_mask, the mix, a curve after it on the channels of out_mask, then gain and offset and tensor_model's
conversions.  curve_eval is the definition in separate np.float32 operations.  curve_fill() and xyz() are the float64
restatements of htj2k_tensor_curve_fill and htj2k_tensor_mix_xyz; dcp_true() is the float64 evaluation of the functions a
digital cinema package's X'Y'Z' goes through; torch_chain() is the chain of eager torch operations that computes the
same values today."""
import numpy as np

import cmp_model as cm
import mix_model as mm
import resize_model as rm
import tensor_model as tm

KINDS = ["power", "srgb_encode", "srgb_decode", "bt709_encode", "bt709_decode", "pq_encode", "pq_decode"]
PRIMARIES = {709: ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060)), 2020: ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046)),
             3: ((0.680, 0.320), (0.265, 0.690), (0.150, 0.060))}
D65 = (0.3127, 0.3290)
PQ = (2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0, 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0)


def curve_eval(x, table, x0=0.0, inv_dx=1.0):
    """E(x; curve) for float32 values x: every line one binary32 operation.  np.fmax / np.fmin give the operand that is not
    NaN; maxNum of -0 and +0 is +0 (as the device's v_max_f32 orders the zeros), which numpy leaves to the platform, so
    the zero is made positive here in words"""
    t = np.asarray(table, np.float32)
    n = t.shape[0]
    t = np.append(t, t[-1])                                  # t[n] taken as t[n-1]
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        u = ((x - np.float32(x0)).astype(np.float32) * np.float32(inv_dx)).astype(np.float32)
        u = np.fmin(np.fmax(u, np.float32(0.0)), np.float32(n - 1)).astype(np.float32)
        u = np.where(u == 0, np.float32(0.0), u)
        i = u.astype(np.int32)                               # truncation of a value in 0 .. n - 1
        r = (u - i.astype(np.float32)).astype(np.float32)
        d = (t[i + 1] - t[i]).astype(np.float32)
        return (t[i] + (r * d).astype(np.float32)).astype(np.float32)


def unpack(curves):
    """a TensorCurves struct as a dict: in / out are None or (table, x0, inv_dx)"""
    def one(cv, table):
        return None if cv.n == 0 else (np.array(table[:cv.n], np.float32), float(cv.x0), float(cv.inv_dx))
    return {"in": one(curves.in_, curves.tables[0]), "out": one(curves.out, curves.tables[1]), "in_mask": int(curves.in_mask),
            "out_mask": int(curves.out_mask), "gain": np.array(list(curves.gain), np.float32), "offset": np.array(list(curves.offset), np.float32)}


def values(f, mix, curves):
    """the definition from the source values f (a list of C float32 arrays): [e_k] as float32 arrays"""
    q = unpack(curves)
    nout, m, b = mm.unpack(mix)
    g = [curve_eval(v, *q["in"]) if (q["in"] is not None and (q["in_mask"] >> c) & 1) else np.asarray(v, np.float32) for c, v in enumerate(f)]
    out = []
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for k, t in enumerate(mm.mix_values(g, m, b, nout)):
            v = curve_eval(t, *q["out"]) if (q["out"] is not None and (q["out_mask"] >> k) & 1) else t
            out.append(((v * q["gain"][k]).astype(np.float32) + q["offset"][k]).astype(np.float32))
    return out


def _laid_out(f, mix, curves, dtype, layout):
    out = np.stack([mm.stored(e, dtype) for e in values(f, mix, curves)])
    return out if layout == "NCHW" else np.ascontiguousarray(out.transpose(1, 2, 0))


def image(planes, fmt, bits, mix, curves, dtype="float32", layout="NCHW", size=None, origin=(0, 0)):
    """one frame's image as bit patterns: shape (K, out_h, out_w) for NCHW, (out_h, out_w, K) for NHWC"""
    comps = cm.components(planes, fmt, bits)
    h, w = comps[0].shape
    out_w, out_h = (w, h) if size is None else size
    ox, oy = origin
    assert 0 <= ox and 0 <= oy and ox + out_w <= w and oy + out_h <= h
    f = [tm.replicate(comps[c], sw, sh, ox, oy, out_w, out_h).astype(np.float32) for c, (sw, sh) in enumerate(tm.chroma_shifts(fmt))]
    return _laid_out(f, mix, curves, dtype, layout)


def batch(frames, fmt, bits, mix, curves, dtype="float32", layout="NCHW", size=None, origins=None):
    return np.stack([image(p, fmt, bits, mix, curves, dtype, layout, size, (0, 0) if origins is None else tuple(origins[i]))
                     for i, p in enumerate(frames)])


def image_resized(planes, fmt, bits, mix, curves, dtype="float32", layout="NCHW", size=None, window=None, filt=rm.TRIANGLE):
    """the resized call with curves: resize_model's f of every component (resampled coded values), then the curves and the mix"""
    filt = rm.FILTERS.get(filt, filt)
    comps = cm.components(planes, fmt, bits)
    h, w = comps[0].shape
    ox, oy, ww, wh = (0, 0, w, h) if window is None else window
    out_w, out_h = size
    f = [rm.resample(tm.replicate(comps[c], sw, sh, ox, oy, ww, wh), out_w, out_h, filt) for c, (sw, sh) in enumerate(tm.chroma_shifts(fmt))]
    return _laid_out(f, mix, curves, dtype, layout)


def batch_resized(frames, fmt, bits, mix, curves, dtype="float32", layout="NCHW", size=None, windows=None, filt=rm.TRIANGLE):
    return np.stack([image_resized(p, fmt, bits, mix, curves, dtype, layout, size, None if windows is None else tuple(windows[i]), filt)
                     for i, p in enumerate(frames)])


def function(kind, x, param=0.0):
    """the transfer functions in float64; the argument is clamped to 0 .. 1 for all but the power law"""
    x = np.asarray(x, np.float64)
    if kind == "power":
        return np.maximum(x, 0.0) ** param
    x = np.clip(x, 0.0, 1.0)
    m1, m2, c1, c2, c3 = PQ
    if kind == "srgb_encode":
        return np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1.0 / 2.4) - 0.055)
    if kind == "srgb_decode":
        return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
    if kind == "bt709_encode":
        return np.where(x < 0.018, 4.5 * x, 1.099 * x ** 0.45 - 0.099)
    if kind == "bt709_decode":
        return np.where(x < 0.081, x / 4.5, ((x + 0.099) / 1.099) ** (1.0 / 0.45))
    if kind == "pq_encode":
        y = x ** m1
        return ((c1 + c2 * y) / (1.0 + c3 * y)) ** m2
    if kind == "pq_decode":
        p = x ** (1.0 / m2)
        return (np.maximum(p - c1, 0.0) / (c2 - c3 * p)) ** (1.0 / m1)
    raise ValueError(kind)


def curve_fill(kind, n, lo=0.0, hi=1.0, param=0.0):
    """htj2k_tensor_curve_fill in float64, not rounded: F(lo + j (hi - lo) / (n - 1))"""
    j = np.arange(n, dtype=np.float64)
    return function(kind, lo + j * (hi - lo) / float(n - 1), param)


def xyz(primaries, scale=1.0):
    """htj2k_tensor_mix_xyz in float64: the 3 x 3 matrix from linear XYZ to linear RGB, times scale"""
    a = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in PRIMARIES[primaries]], np.float64).T
    w = np.array([D65[0] / D65[1], 1.0, (1.0 - D65[0] - D65[1]) / D65[1]], np.float64)
    npm = a * np.linalg.solve(a, w)[None, :]
    return np.linalg.inv(npm) * scale


def dcp_true(s, primaries=709, out="srgb"):
    """float64: 12-bit X'Y'Z' samples s (..., 3) -> the encoded R, G, B a digital cinema package stands for"""
    lin = (np.asarray(s, np.float64) / 4095.0) ** 2.6
    rgb = lin @ xyz(primaries, 52.37 / 48.0).T
    return function(out + "_encode", rgb)


def torch_chain(s, tin, mat, b, tout, x0, inv_dx, gain, offset):
    """the eager chain a caller runs today: s (C, N) integer samples -> (K, N) float32; a gather, the products and sums, a
    clamp, an index and a lerp written out as separate ops"""
    import torch
    g = [tin[s[c].long()] for c in range(s.shape[0])]
    out = []
    for k in range(mat.shape[0]):
        a = torch.mul(g[0], float(mat[k][0]))
        for c in range(1, len(g)):
            a = torch.add(a, torch.mul(g[c], float(mat[k][c])))
        t = torch.add(a, float(b[k]))
        u = torch.mul(torch.sub(t, x0), inv_dx)
        u = torch.clamp(u, 0.0, float(tout.shape[0] - 1))
        i = u.to(torch.int64)
        r = torch.sub(u, i.float())
        lo, hi = tout[i], tout[torch.clamp(i + 1, max=tout.shape[0] - 1)]
        v = torch.add(lo, torch.mul(r, torch.sub(hi, lo)))
        out.append(torch.add(torch.mul(v, float(gain[k])), float(offset[k])))
    return torch.stack(out)
