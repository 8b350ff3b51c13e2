"""numpy restatement of the tensor calls with a colour matrix (include/htj2k_amd.h "frames as tensors, mixed",
csrc/mix_kernels.hpp): K channels of bit patterns from a frame's raw planes.  The source values are tensor_model's (the
sample read and the chroma replication) or resize_model's f; the mix is separate np.float32 multiplications and additions
in the stated order, all C terms, none left out; the stored bits are tensor_model's conversions.  ycbcr() is the float64
restatement of htj2k_tensor_mix_ycbcr."""
import numpy as np

import cmp_model as cm
import resize_model as rm
import tensor_model as tm

KR_KB = {601: (0.299, 0.114), 709: (0.2126, 0.0722), 2020: (0.2627, 0.0593)}


def unpack(mix):
    """(K, m as float32 (4, 4), b as float32 (4,)) of a TensorMix struct, or of an (m, b) pair of arrays (K x C, K)"""
    if hasattr(mix, "nout"):
        return int(mix.nout), np.array([[mix.m[k][c] for c in range(4)] for k in range(4)], np.float32), np.array(list(mix.b), np.float32)
    m, b = mix
    m = np.asarray(m, np.float32)
    full, off = np.zeros((4, 4), np.float32), np.zeros(4, np.float32)
    full[:m.shape[0], :m.shape[1]] = m
    off[:m.shape[0]] = np.zeros(m.shape[0], np.float32) if b is None else np.asarray(b, np.float32)
    return m.shape[0], full, off


def mix_values(f, m, b, nout):
    """the definition: f a list of C float32 arrays -> [t_k] as float32 arrays; a = f_0 * m[k][0]; a = a + (f_c * m[k][c])
    for c = 1 .. C - 1; t = a + b[k]; every operation rounded to binary32 on its own"""
    out = []
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for k in range(nout):
            a = f[0].astype(np.float32) * np.float32(m[k][0])
            for c in range(1, len(f)):
                p = f[c].astype(np.float32) * np.float32(m[k][c])
                a = (a + p).astype(np.float32)
            out.append((a + np.float32(b[k])).astype(np.float32))
    return out


def stored(t, dtype):
    """tensor_model's conversion of float32 values t: t * 1 + (-0) is t bit for bit, signed zeros included"""
    return tm.value_bits(np.asarray(t, np.float32), 1.0, -0.0, dtype)


def _laid_out(f, mix, dtype, layout):
    nout, m, b = unpack(mix)
    out = np.stack([stored(t, dtype) for t in mix_values(f, m, b, nout)])
    return out if layout == "NCHW" else np.ascontiguousarray(out.transpose(1, 2, 0))


def image(planes, fmt, bits, mix, dtype="float32", layout="NCHW", size=None, origin=(0, 0)):
    """one frame's mixed image as bit patterns: shape (K, out_h, out_w) for NCHW, (out_h, out_w, K) for NHWC"""
    comps = cm.components(planes, fmt, bits)
    h, w = comps[0].shape
    out_w, out_h = (w, h) if size is None else size
    ox, oy = origin
    assert 0 <= ox and 0 <= oy and ox + out_w <= w and oy + out_h <= h
    f = [tm.replicate(comps[c], sw, sh, ox, oy, out_w, out_h).astype(np.float32) for c, (sw, sh) in enumerate(tm.chroma_shifts(fmt))]
    return _laid_out(f, mix, dtype, layout)


def batch(frames, fmt, bits, mix, dtype="float32", layout="NCHW", size=None, origins=None):
    return np.stack([image(p, fmt, bits, mix, dtype, layout, size, (0, 0) if origins is None else tuple(origins[i]))
                     for i, p in enumerate(frames)])


def image_resized(planes, fmt, bits, mix, dtype="float32", layout="NCHW", size=None, window=None, filt=rm.TRIANGLE):
    """the resized call with a mix: resize_model's f of every component, then the mix"""
    filt = rm.FILTERS.get(filt, filt)
    comps = cm.components(planes, fmt, bits)
    h, w = comps[0].shape
    ox, oy, ww, wh = (0, 0, w, h) if window is None else window
    out_w, out_h = size
    f = [rm.resample(tm.replicate(comps[c], sw, sh, ox, oy, ww, wh), out_w, out_h, filt) for c, (sw, sh) in enumerate(tm.chroma_shifts(fmt))]
    return _laid_out(f, mix, dtype, layout)


def batch_resized(frames, fmt, bits, mix, dtype="float32", layout="NCHW", size=None, windows=None, filt=rm.TRIANGLE):
    return np.stack([image_resized(p, fmt, bits, mix, dtype, layout, size, None if windows is None else tuple(windows[i]), filt)
                     for i, p in enumerate(frames)])


def identity(nc):
    return np.eye(nc, dtype=np.float32), np.zeros(nc, np.float32)


def ycbcr(standard, full_range, bits, alpha=False, gain=None, offset=None):
    """htj2k_tensor_mix_ycbcr in float64: (m of shape (K, 4), b of shape (K,)), K = 3 or 4"""
    kr, kb = KR_KB[standard]
    kg = 1.0 - kr - kb
    q, peak, mid = float(1 << (bits - 8)), float((1 << bits) - 1), float(1 << (bits - 1))
    ys, y0, cs = (1.0 / peak, 0.0, 1.0 / peak) if full_range else (1.0 / (219.0 * q), 16.0 * q, 1.0 / (224.0 * q))
    # rows R', G', B' over (Y', Pb, Pr)
    w = [[1.0, 0.0, 2.0 * (1.0 - kr)], [1.0, -2.0 * kb * (1.0 - kb) / kg, -2.0 * kr * (1.0 - kr) / kg], [1.0, 2.0 * (1.0 - kb), 0.0]]
    nout = 4 if alpha else 3
    m, b = np.zeros((nout, 4), np.float64), np.zeros(nout, np.float64)
    for k in range(3):
        g = 1.0 if gain is None else float(np.float32(gain[k]))
        o = 0.0 if offset is None else float(np.float32(offset[k]))
        m[k, 0] = g * w[k][0] * ys
        m[k, 1] = g * w[k][1] * cs
        m[k, 2] = g * w[k][2] * cs
        b[k] = g * (-y0 * ys * w[k][0] - mid * cs * (w[k][1] + w[k][2])) + o
    if alpha:
        m[3, 3] = 1.0 / peak
    return m, b
