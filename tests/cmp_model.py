"""numpy restatement of htj2k_compare_frames (include/htj2k_amd.h, csrc/cmp_kernels.hpp): per component sse, ndiff,
max_abs and nsamples as Python ints, and the pooled PSNR.  It takes the raw planes of a layout -- 2-D arrays of uint8 or
uint16, a packed layout's rows holding the interleaved samples -- and applies the shift and the mask itself."""
import math

import numpy as np

# name: (components, planar, log2 chroma w, log2 chroma h, depth, bytes per sample): csrc/j2k_syntax.c layout_table
LAYOUTS = {"rgb24": (3, 0, 0, 0, 8, 1), "rgba": (4, 0, 0, 0, 8, 1), "rgb48le": (3, 0, 0, 0, 16, 2),
           "rgba64le": (4, 0, 0, 0, 16, 2), "gray": (1, 0, 0, 0, 8, 1), "ya8": (2, 0, 0, 0, 8, 1),
           "gray16le": (1, 0, 0, 0, 16, 2), "ya16le": (2, 0, 0, 0, 16, 2), "xyz12le": (3, 0, 0, 0, 12, 2),
           "yuv410p": (3, 1, 2, 2, 8, 1), "yuv411p": (3, 1, 2, 0, 8, 1), "yuv440p": (3, 1, 0, 1, 8, 1)}
for _d, _suffix, _b in [(8, "", 1), (9, "9le", 2), (10, "10le", 2), (12, "12le", 2), (14, "14le", 2), (16, "16le", 2)]:
    for _name, _cw, _ch in [("420p", 1, 1), ("422p", 1, 0), ("444p", 0, 0)]:
        LAYOUTS["yuv" + _name + _suffix] = (3, 1, _cw, _ch, _d, _b)
        if _d in (8, 9, 10, 16):
            LAYOUTS["yuva" + _name + _suffix] = (4, 1, _cw, _ch, _d, _b)
TOP_ALIGNED = ("rgb48le", "rgba64le", "gray16le", "xyz12le")     # 16-bit words that carry the sample at the top


def shift(fmt, bits):
    """what k_enc_unpack shifts a word by: the inverse of the decoder's pack stage"""
    return 8 - bits if bits <= 8 else (16 - bits if fmt in TOP_ALIGNED else 0)


def comp_dims(fmt, w, h):
    nc, _, cw, ch, _, _ = LAYOUTS[fmt]
    return [(-(-w // (1 << cw)), -(-h // (1 << ch))) if c in (1, 2) else (w, h) for c in range(nc)]


def plane_shapes(fmt, w, h):
    """(rows, samples per row) of every plane of the layout"""
    nc, planar = LAYOUTS[fmt][:2]
    return [(ch, cw) for cw, ch in comp_dims(fmt, w, h)] if planar else [(h, w * nc)]


def components(planes, fmt, bits):
    """the layout's components as int64 arrays of `bits`-bit samples"""
    nc, planar = LAYOUTS[fmt][:2]
    sh, mask = shift(fmt, bits), (1 << bits) - 1
    val = [(np.asarray(p).astype(np.int64) >> sh) & mask for p in planes]
    return val if planar else [val[0][:, c::nc] for c in range(nc)]


def compare(a_planes, b_planes, fmt, bits):
    a, b = components(a_planes, fmt, bits), components(b_planes, fmt, bits)
    out = {"sse": [0] * 4, "ndiff": [0] * 4, "nsamples": [0] * 4, "max_abs": [0] * 4}
    for c, (x, y) in enumerate(zip(a, b)):
        d = np.abs(x - y)
        out["sse"][c] = sum(int(v) * int(v) * int(k) for v, k in zip(*np.unique(d, return_counts=True)))
        out["ndiff"][c] = int(np.count_nonzero(d))
        out["nsamples"][c] = int(d.size)
        out["max_abs"][c] = int(d.max()) if d.size else 0
    se, n, peak = sum(out["sse"]), sum(out["nsamples"]), (1 << bits) - 1
    out["psnr"] = math.inf if se == 0 else 10.0 * math.log10(float(peak * peak) * float(n) / float(se))
    return out


def same(got, want, tol=1e-9):
    """every integer equal, psnr within tol dB (both infinite, or both NaN, counts as equal)"""
    if any(list(got[k]) != list(want[k]) for k in ("sse", "ndiff", "nsamples", "max_abs")):
        return False
    g, w = got["psnr"], want["psnr"]
    return (math.isnan(g) and math.isnan(w)) or g == w or abs(g - w) <= tol
