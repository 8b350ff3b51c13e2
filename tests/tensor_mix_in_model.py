"""numpy restatement of tensors as frames through a colour matrix and a chroma filter (include/htj2k_amd.h "tensors as
frames, mixed", csrc/mix_in_kernels.hpp): the frames that htj2k_tensor_to_frames_mix writes for a tensor of K channels,
and that htj2k_encode_tensor_mix encodes.  A tensor comes in as bit patterns, as tensor_in_model takes them (uint32 for
float32, uint16 for float16 and bfloat16), (n, K, H, W) or (n, H, W, K); frames go out as cmp_model takes them.  Every
step is a separate np.float32 operation in the stated order: the footprint's elements added in raster order, one
multiplication by the float32 nearest to 1 / N, the K products added in their order, the offset last.  rgb() is the float64
restatement of htj2k_tensor_mix_in_rgb."""
import numpy as np

import cmp_model as cm
import tensor_in_model as tim
from mix_model import KR_KB

COSITED, BOX = 0, 1
CHROMA = {"cosited": COSITED, "box": BOX}


def unpack(mix):
    """(K, chroma, m as float32 (4, 4), b as float32 (4,)) of a TensorMixIn struct, or of an (m, b, chroma) triple with m a
    C x K array"""
    if hasattr(mix, "nin"):
        return (int(mix.nin), int(mix.chroma), np.array([[mix.m[c][k] for k in range(4)] for c in range(4)], np.float32),
                np.array(list(mix.b), np.float32))
    m, b, chroma = mix
    m = np.asarray(m, np.float32)
    full, off = np.zeros((4, 4), np.float32), np.zeros(4, np.float32)
    full[:m.shape[0], :m.shape[1]] = m
    off[:m.shape[0]] = np.zeros(m.shape[0], np.float32) if b is None else np.asarray(b, np.float32)
    return m.shape[1], CHROMA.get(chroma, chroma), full, off


def gather(chan, sw, sh, chroma):
    """one channel's float32 values (H, W) -> g of every footprint, (ceil(H / 2^sh), ceil(W / 2^sw)): the corner element,
    or (box) the footprint's elements added in raster order, rows outer, then times the float32 nearest to 1 / N; the
    last column and row of an odd picture have clipped footprints.  Footprints of one element are the element"""
    f = np.asarray(chan, np.float32)
    h, w = f.shape
    fw, fh = 1 << sw, 1 << sh
    g = f[::fh, ::fw].copy()
    if chroma == COSITED or (fw == 1 and fh == 1):
        return g
    n = np.zeros(g.shape, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for fy in range(fh):
            for fx in range(fw):
                part = f[fy::fh, fx::fw]                      # the footprints that have this element
                rows, cols = part.shape
                if fy or fx:
                    g[:rows, :cols] = (g[:rows, :cols] + part).astype(np.float32)
                n[:rows, :cols] += 1
        rcp = (1.0 / n).astype(np.float32)                    # float64 quotient rounded once: the nearest float32 to 1 / N
        return np.where(n > 1, (g * rcp).astype(np.float32), g)


def mix_rows(g, m_row, b, nin):
    """u of the definition: a = g_0 * m[0]; a = a + (g_k * m[k]) for k = 1 .. K - 1; u = a + b"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a = (g[0] * np.float32(m_row[0])).astype(np.float32)
        for k in range(1, nin):
            a = (a + (g[k] * np.float32(m_row[k])).astype(np.float32)).astype(np.float32)
        return (a + np.float32(b)).astype(np.float32)


def component_u(chw_values, fmt, mix, c):
    """u of every sample of component c, float32, from the image's float32 values (K, H, W)"""
    nc, _, cw, ch, _, _ = cm.LAYOUTS[fmt]
    nin, chroma, m, b = unpack(mix)
    assert chw_values.shape[0] == nin
    sw, sh = (cw, ch) if c in (1, 2) else (0, 0)
    g = [gather(chw_values[k], sw, sh, chroma) for k in range(nin)]
    return mix_rows(g, m[c], b[c], nin)


def frame(img_bits, fmt, bits, mix, dtype="float32", layout="NCHW"):
    """one image's bit patterns, (K, H, W) or (H, W, K) -> the planes of its frame"""
    nc, planar, _, _, _, nbytes = cm.LAYOUTS[fmt]
    img = np.asarray(img_bits)
    chw = tim.element_values(img if layout == "NCHW" else img.transpose(2, 0, 1), dtype)
    word = np.uint8 if nbytes == 1 else np.uint16
    comps = [(tim.samples(component_u(chw, fmt, mix, c), 1.0, -0.0, bits) << cm.shift(fmt, bits)).astype(word) for c in range(nc)]
    if planar:
        return comps
    return [np.ascontiguousarray(np.stack(comps, -1).reshape(chw.shape[1], chw.shape[2] * nc))]


def frames(tensor_bits, fmt, bits, mix, dtype="float32", layout="NCHW"):
    """(n, ...) bit patterns -> n frames (lists of planes)"""
    return [frame(img, fmt, bits, mix, dtype, layout) for img in np.asarray(tensor_bits)]


def averaged(img_bits, fmt, mix, dtype="float32", layout="NCHW"):
    """the image averaged beforehand by the box rule, as float32 bit patterns of the same shape: every element replaced by
    its chroma footprint's g.  The co-sited call on it gives the chroma of the box call on the original"""
    _, _, cw, ch, _, _ = cm.LAYOUTS[fmt]
    img = np.asarray(img_bits)
    chw = tim.element_values(img if layout == "NCHW" else img.transpose(2, 0, 1), dtype)
    out = np.empty(chw.shape, np.float32)
    for k in range(chw.shape[0]):
        g = gather(chw[k], cw, ch, BOX)
        out[k] = np.repeat(np.repeat(g, 1 << ch, 0), 1 << cw, 1)[:chw.shape[1], :chw.shape[2]]
    out = out if layout == "NCHW" else np.ascontiguousarray(out.transpose(1, 2, 0))
    return out.view(np.uint32)


def identity(nc, chroma=COSITED):
    return np.eye(nc, dtype=np.float32), np.zeros(nc, np.float32), chroma


def rgb(standard, full_range, bits, alpha=False, gain=None, offset=None):
    """htj2k_tensor_mix_in_rgb in float64: (m of shape (C, K), b of shape (C,)), C = K = 3, or 4 with alpha"""
    kr, kb = KR_KB[standard]
    kg = 1.0 - kr - kb
    q, peak, mid = float(1 << (bits - 8)), float((1 << bits) - 1), float(1 << (bits - 1))
    ys, y0, cs = (peak, 0.0, peak) if full_range else (219.0 * q, 16.0 * q, 224.0 * q)
    pb, pr = cs / (2.0 * (1.0 - kb)), cs / (2.0 * (1.0 - kr))
    A = [[ys * kr, ys * kg, ys * kb], [-pb * kr, -pb * kg, pb * (1.0 - kb)], [pr * (1.0 - kr), -pr * kg, -pr * kb]]
    o = [y0, mid, mid]
    nc = 4 if alpha else 3
    m, b = np.zeros((nc, nc), np.float64), np.zeros(nc, np.float64)
    for c in range(3):
        b[c] = o[c]
        for k in range(3):
            g = 1.0 if gain is None else float(np.float32(gain[k]))
            off = 0.0 if offset is None else float(np.float32(offset[k]))
            m[c, k] = A[c][k] / g
            b[c] -= A[c][k] * off / g
    if alpha:
        m[3, 3] = peak
    return m, b
