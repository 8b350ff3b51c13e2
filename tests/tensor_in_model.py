"""numpy restatement of tensors as frames (include/htj2k_amd.h, tensor_in_sample in csrc/tensor_kernels.hpp): the frames
that htj2k_tensor_to_frames writes for a float tensor, and that htj2k_encode_tensor encodes.  A tensor comes in as bit
patterns, as tensor_model gives them (uint32 for float32, uint16 for float16 and bfloat16), (n, C, H, W) or (n, H, W, C);
frames go out as cmp_model takes them -- 2-D arrays of uint8 or uint16, a packed layout's rows holding the interleaved
samples -- with the sample shifted to its place in the word and every other bit zero."""
import numpy as np

import cmp_model as cm


def element_values(bits_array, dtype):
    """the elements' values as float32: exact for all three element types"""
    a = np.asarray(bits_array)
    if dtype == "float32":
        return a.astype(np.uint32).view(np.float32)
    if dtype == "float16":
        return a.astype(np.uint16).view(np.float16).astype(np.float32)
    assert dtype == "bfloat16"
    return (a.astype(np.uint32) << np.uint32(16)).view(np.float32)


def samples(values, scale, bias, bits):
    """float32 element values -> integer samples: u = f * scale, then u + bias, two rounded binary32 operations;
    r = rint(u), ties to even; 0 unless r > 0 (NaN, -inf, negatives, -0); 2^bits - 1 where r >= it (+inf)"""
    peak = (1 << bits) - 1
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        u = (np.asarray(values, np.float32) * np.float32(scale)).astype(np.float32)
        u = (u + np.float32(bias)).astype(np.float32)
        r = np.rint(u)
        s = np.zeros(r.shape, np.int64)
        mid = (r > 0) & (r < np.float32(peak))
        s[mid] = r[mid].astype(np.int64)
        s[r >= np.float32(peak)] = peak
    return s


def frame(img_bits, fmt, bits, dtype="float32", layout="NCHW", scale=None, bias=None):
    """one image's bit patterns, (C, H, W) or (H, W, C) -> the planes of its frame"""
    nc, planar, cw, ch, _, nbytes = cm.LAYOUTS[fmt]
    img = np.asarray(img_bits)
    chw = img if layout == "NCHW" else img.transpose(2, 0, 1)
    assert chw.shape[0] == nc
    scale = [1.0] * nc if scale is None else ([scale] * nc if np.isscalar(scale) else list(scale))
    bias = [0.0] * nc if bias is None else ([bias] * nc if np.isscalar(bias) else list(bias))
    word = np.uint8 if nbytes == 1 else np.uint16
    comps = []
    for c in range(nc):
        sw, sh = (cw, ch) if c in (1, 2) else (0, 0)
        e = chw[c][::1 << sh, ::1 << sw]               # the co-sited top-left element of every footprint
        comps.append((samples(element_values(e, dtype), scale[c], bias[c], bits) << cm.shift(fmt, bits)).astype(word))
    if planar:
        return comps
    return [np.ascontiguousarray(np.stack(comps, -1).reshape(chw.shape[1], chw.shape[2] * nc))]


def frames(tensor_bits, fmt, bits, dtype="float32", layout="NCHW", scale=None, bias=None):
    """(n, ...) bit patterns -> n frames (lists of planes)"""
    return [frame(img, fmt, bits, dtype, layout, scale, bias) for img in np.asarray(tensor_bits)]
