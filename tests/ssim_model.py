"""numpy restatement of htj2k_compare_frames_ssim (include/htj2k_amd.h, csrc/cmp_kernels.hpp: k_frame_ssim), which is
libavfilter's vf_ssim.c (ssim_4x4xn, ssim_end1 / ssim_end1x, ssim_plane) with an integer result: per component the sum
over its 8x8 windows at stride 4 of rint(v * 2^32), v = (A * B) / (C * D) in IEEE doubles on exact integers.  It takes the
raw planes of a layout as cmp_model.compare does and returns q32 and nwin as Python ints."""
import math

import numpy as np

import cmp_model as cm


def constants(bits):
    peak = (1 << bits) - 1
    return (64 * peak * peak + 5000) // 10000, (36288 * peak * peak + 5000) // 10000


def window_sums(x, y):
    """(s1, s2, ss, s12) of every window of one component as int64 arrays of (bh - 1, bw - 1); None without windows"""
    ch, cw = x.shape
    bw, bh = cw >> 2, ch >> 2
    if bw < 2 or bh < 2:
        return None
    x, y = x[:4 * bh, :4 * bw].astype(np.int64), y[:4 * bh, :4 * bw].astype(np.int64)
    out = []
    for v in (x, y, x * x + y * y, x * y):
        blk = v.reshape(bh, 4, bw, 4).sum(axis=(1, 3))
        out.append(blk[:-1, :-1] + blk[:-1, 1:] + blk[1:, :-1] + blk[1:, 1:])
    return out


def window_q(s1, s2, ss, s12, bits):
    """rint(v * 2^32) of windows given by their int64 sums -> int64 array"""
    c1, c2 = constants(bits)
    vars_, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    A, B, C, D = 2 * s1 * s2 + c1, 2 * covar + c2, s1 * s1 + s2 * s2 + c1, vars_ + c2
    for t in (A, B, C, D):
        assert np.all(np.abs(t) < (1 << 53))                  # exact as doubles
    v = (A.astype(np.float64) * B.astype(np.float64)) / (C.astype(np.float64) * D.astype(np.float64))
    return np.rint(v * 4294967296.0).astype(np.int64)


def ssim(a_planes, b_planes, fmt, bits):
    a, b = cm.components(a_planes, fmt, bits), cm.components(b_planes, fmt, bits)
    out = {"q32": [0] * 4, "nwin": [0] * 4, "ssim": [math.nan] * 4}
    num = den = 0.0
    for c, (x, y) in enumerate(zip(a, b)):
        s = window_sums(x, y)
        if s is None:
            continue
        q = window_q(*s, bits)
        out["q32"][c] = sum(int(v) for v in q.ravel())
        out["nwin"][c] = int(q.size)
        out["ssim"][c] = out["q32"][c] / 4294967296.0 / q.size
        num += out["ssim"][c] * float(x.shape[0] * x.shape[1])
        den += float(x.shape[0] * x.shape[1])
    out["all"] = num / den if den else math.nan
    return out


def same(got, want, tol=1e-12):
    """q32 and nwin equal, ssim and all within tol (NaN where the other is NaN)"""
    if list(got["q32"]) != list(want["q32"]) or list(got["nwin"]) != list(want["nwin"]):
        return False
    for g, w in list(zip(got["ssim"], want["ssim"])) + [(got["all"], want["all"])]:
        if math.isnan(g) != math.isnan(w) or (not math.isnan(g) and abs(g - w) > tol):
            return False
    return True
