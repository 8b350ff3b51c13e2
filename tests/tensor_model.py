"""numpy restatement of htj2k_frames_to_tensor (include/htj2k_amd.h, csrc/tensor_kernels.hpp): the float image of a
frame's window as arrays of bit patterns (uint32 for float32, uint16 for float16 and bfloat16).  It takes the raw planes
of a layout as cmp_model does -- 2-D arrays of uint8 or uint16, a packed layout's rows holding the interleaved samples --
and applies the shift, the mask and the chroma replication itself."""
import numpy as np

import cmp_model as cm

DTYPES = ("float32", "float16", "bfloat16")
ESIZE = {"float32": 4, "float16": 2, "bfloat16": 2}
BITS_DTYPE = {"float32": np.uint32, "float16": np.uint16, "bfloat16": np.uint16}


def ncomp(fmt):
    return cm.LAYOUTS[fmt][0]


def chroma_shifts(fmt):
    """[(sw, sh)] per component: the layout's chroma shifts for components 1 and 2, 0 for every other"""
    nc, _, cw, ch, _, _ = cm.LAYOUTS[fmt]
    return [(cw, ch) if c in (1, 2) else (0, 0) for c in range(nc)]


def replicate(comp, sw, sh, ox, oy, out_w, out_h):
    """component `comp` (its own, ceilinged size) seen through the window: sample ((ox + x) >> sw, (oy + y) >> sh)"""
    ys = (oy + np.arange(out_h)) >> sh
    xs = (ox + np.arange(out_w)) >> sw
    return comp[np.ix_(ys, xs)]


def value_bits(s, scale, bias, dtype):
    """the stored bits of integer samples s: t = float32(s) * float32(scale) + float32(bias), two rounded binary32
    operations, then the element's rounding to nearest even"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        t = np.asarray(s).astype(np.float32) * np.float32(scale)
        t = (t + np.float32(bias)).astype(np.float32)
        if dtype == "float32":
            return t.view(np.uint32)
        if dtype == "float16":
            return t.astype(np.float16).view(np.uint16)
        assert dtype == "bfloat16"
        u = t.view(np.uint32).astype(np.uint64)
        return (((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16)


def image(planes, fmt, bits, dtype="float32", layout="NCHW", size=None, origin=(0, 0), scale=None, bias=None):
    """one frame's image as bit patterns: shape (C, out_h, out_w) for NCHW, (out_h, out_w, C) for NHWC"""
    comps = cm.components(planes, fmt, bits)
    nc = len(comps)
    h, w = comps[0].shape
    out_w, out_h = (w, h) if size is None else size
    ox, oy = origin
    assert 0 <= ox and 0 <= oy and ox + out_w <= w and oy + out_h <= h
    scale = [1.0] * nc if scale is None else ([scale] * nc if np.isscalar(scale) else list(scale))
    bias = [0.0] * nc if bias is None else ([bias] * nc if np.isscalar(bias) else list(bias))
    chans = [value_bits(replicate(comps[c], sw, sh, ox, oy, out_w, out_h), scale[c], bias[c], dtype)
             for c, (sw, sh) in enumerate(chroma_shifts(fmt))]
    out = np.stack(chans)
    return out if layout == "NCHW" else np.ascontiguousarray(out.transpose(1, 2, 0))


def batch(frames, fmt, bits, dtype="float32", layout="NCHW", size=None, origins=None, scale=None, bias=None):
    """n frames (lists of planes) -> (n, ...) bit patterns; origins: None or one (ox, oy) per frame"""
    return np.stack([image(p, fmt, bits, dtype, layout, size, (0, 0) if origins is None else tuple(origins[i]), scale, bias)
                     for i, p in enumerate(frames)])
