"""numpy restatement of htj2k_frames_to_tensor_resized (include/htj2k_amd.h, csrc/resize_kernels.hpp): the weights of an
axis in Python integers, and the float image of a frame's resampled window as arrays of bit patterns.  Built on
tensor_model (the replication of chroma, the two rounded operations and the element's rounding) and cmp_model
(components)."""
import numpy as np

import cmp_model as cm
import tensor_model as tm

NEAREST, BILINEAR, TRIANGLE = 0, 1, 2
FILTERS = {"nearest": NEAREST, "bilinear": BILINEAR, "triangle": TRIANGLE}
ONE = 1 << 14
MAX_SIZE, MAX_REDUCTION, MAX_TAPS = 32768, 64, 129


def in_scope(win, out, filt):
    return 1 <= win <= MAX_SIZE and 1 <= out <= MAX_SIZE and (filt != TRIANGLE or win <= MAX_REDUCTION * out)


def weights(win, out, filt, x, seen=None, walk_all=False):
    """the taps of output index x of an axis win -> out: (first source index, [q]).  walk_all: the definition as it is
    written, every X of the window tried; otherwise the walk starts just below the run (the long axes of the tests).
    `seen`, a dict, collects the largest value of every intermediate the header promises to fit 32 bits: "cx", "centre"
    ((2X + 1) out of a tap), "shifted" (a << 14) and "A" """
    def note(name, v):
        if seen is not None:
            seen[name] = max(seen.get(name, 0), v)

    assert in_scope(win, out, filt) and 0 <= x < out
    D = 2 * out
    cx = (2 * x + 1) * win
    note("cx", cx)
    if filt == NEAREST:
        return cx // D, [ONE]
    S = D if filt == BILINEAR else 2 * max(out, win)
    start = 0 if walk_all else max(0, (cx - S - out) // (2 * out) - 1)   # below the first X with (2X + 1) out > cx - S
    first, a = None, []
    for X in range(start, win):
        centre = (2 * X + 1) * out
        v = S - abs(centre - cx)
        if v > 0:
            first = X if first is None else first
            a.append(v)
            note("centre", centre)
            note("shifted", v << 14)
        elif a:
            break                                          # one contiguous run
    A = sum(a)
    note("A", A)
    q = [(v << 14) // A for v in a]
    q[a.index(max(a))] += ONE - sum(q)
    return first, q


def matrix(win, out, filt):
    """the axis as an (out, win) matrix of int64 weights; every row sums to 2^14"""
    W = np.zeros((out, win), np.int64)
    for x in range(out):
        first, q = weights(win, out, filt, x)
        W[x, first:first + len(q)] = q
    return W


def resample(src, out_w, out_h, filt):
    """an integer image (wh, ww) -> f of the definition, float32 (out_h, out_w): acc in int64, one rounding"""
    wh, ww = src.shape
    acc = matrix(wh, out_h, filt) @ (src.astype(np.int64) @ matrix(ww, out_w, filt).T)
    assert acc.min() >= 0 and acc.max() < 1 << 44
    return (acc.astype(np.float64) * 2.0 ** -28).astype(np.float32)


def image(planes, fmt, bits, dtype="float32", layout="NCHW", size=None, window=None, filt=TRIANGLE, scale=None, bias=None):
    """one frame's resampled window as bit patterns: shape (C, out_h, out_w) for NCHW, (out_h, out_w, C) for NHWC;
    window = (ox, oy, ww, wh), None: the frame whole"""
    filt = FILTERS.get(filt, filt)
    comps = cm.components(planes, fmt, bits)
    nc = len(comps)
    h, w = comps[0].shape
    ox, oy, ww, wh = (0, 0, w, h) if window is None else window
    out_w, out_h = size
    assert 0 <= ox and 0 <= oy and ww >= 1 and wh >= 1 and ox + ww <= w and oy + wh <= h
    scale = [1.0] * nc if scale is None else ([scale] * nc if np.isscalar(scale) else list(scale))
    bias = [0.0] * nc if bias is None else ([bias] * nc if np.isscalar(bias) else list(bias))
    chans = [tm.value_bits(resample(tm.replicate(comps[c], sw, sh, ox, oy, ww, wh), out_w, out_h, filt), scale[c], bias[c], dtype)
             for c, (sw, sh) in enumerate(tm.chroma_shifts(fmt))]
    out = np.stack(chans)
    return out if layout == "NCHW" else np.ascontiguousarray(out.transpose(1, 2, 0))


def batch(frames, fmt, bits, dtype="float32", layout="NCHW", size=None, windows=None, filt=TRIANGLE, scale=None, bias=None):
    """n frames (lists of planes) -> (n, ...) bit patterns; windows: None or one (ox, oy, ww, wh) per frame"""
    return np.stack([image(p, fmt, bits, dtype, layout, size, None if windows is None else tuple(windows[i]), filt, scale, bias)
                     for i, p in enumerate(frames)])
