"""numpy restatement of htj2k_resize_frames (include/htj2k_amd.h, csrc/resize_kernels.hpp: k_frame_rescale): a window of a
frame resampled to a frame of another size, every plane on its own grid and in integers.  Built on resize_model (the
weights of an axis, by import) and cmp_model (the layouts and the shift of a sample word).  Planes are what HFrame.arrays()
and the oracle give: 2-D arrays of uint8 or uint16 words, a packed layout's rows holding the interleaved samples."""
import numpy as np

import cmp_model as cm
import resize_model as rm

NEAREST, BILINEAR, TRIANGLE = rm.NEAREST, rm.BILINEAR, rm.TRIANGLE
FILTERS = rm.FILTERS
HALF, SHIFT = 1 << 27, 28


def plane_shifts(fmt):
    """(sw, sh) of every plane: the chroma shifts for planes 1 and 2 of a planar layout, 0 for every other plane"""
    nc, planar, cw, ch = cm.LAYOUTS[fmt][:4]
    return [((cw, ch) if c in (1, 2) else (0, 0)) for c in range(nc)] if planar else [(0, 0)]


def step(fmt):
    """interleaved components of a plane"""
    nc, planar = cm.LAYOUTS[fmt][:2]
    return 1 if planar else nc


def cdiv(v, s):
    return (v + (1 << s) - 1) >> s


def plane_window(window, sw, sh):
    """the frame's window (ox, oy, ww, wh) in a plane of shifts (sw, sh): origin shifted down, size ceilinged"""
    ox, oy, ww, wh = window
    return ox >> sw, oy >> sh, cdiv(ww, sw), cdiv(wh, sh)


def plane_size(size, sw, sh):
    """(dw, dh) of a plane of an out_w x out_h frame: the decoder's ceilinged sizes"""
    return cdiv(size[0], sw), cdiv(size[1], sh)


def grid_ok(fmt, window):
    """the origin is a multiple of the layout's largest 2^sw and 2^sh"""
    sw = max(s for s, _ in plane_shifts(fmt))
    sh = max(s for _, s in plane_shifts(fmt))
    return window[0] % (1 << sw) == 0 and window[1] % (1 << sh) == 0


def rescale(src, dw, dh, filt):
    """an integer image (ph, pw) -> the output samples (dh, dw), int64: acc in int64, r = (acc + 2^27) >> 28"""
    ph, pw = src.shape
    acc = rm.matrix(ph, dh, filt) @ (src.astype(np.int64) @ rm.matrix(pw, dw, filt).T)
    assert acc.min() >= 0 and acc.max() < 1 << 44
    return (acc + HALF) >> SHIFT


def frame(planes, fmt, bits, size, window=None, filt=TRIANGLE):
    """one frame's window resampled to size = (out_w, out_h) -> the destination's planes as arrays of sample words
    (uint8 or uint16; a packed layout's rows interleaved), every bit outside the sample zero"""
    filt = FILTERS.get(filt, filt)
    nbytes = cm.LAYOUTS[fmt][5]
    sh_word, mask, st = cm.shift(fmt, bits), (1 << bits) - 1, step(fmt)
    shifts = plane_shifts(fmt)
    h, w = np.asarray(planes[0]).shape[0], np.asarray(planes[0]).shape[1] // st
    window = (0, 0, w, h) if window is None else tuple(int(v) for v in window)
    ox, oy, ww, wh = window
    assert 0 <= ox and 0 <= oy and ww >= 1 and wh >= 1 and ox + ww <= w and oy + wh <= h and grid_ok(fmt, window)
    out = []
    for p, (sw, sh) in zip(planes, shifts):
        px, py, pw, ph = plane_window(window, sw, sh)
        dw, dh = plane_size(size, sw, sh)
        val = (np.asarray(p).astype(np.int64) >> sh_word) & mask
        assert py + ph <= val.shape[0] and (px + pw) * st <= val.shape[1]
        dst = np.zeros((dh, dw * st), np.int64)
        for c in range(st):
            r = rescale(val[py:py + ph, px * st + c:(px + pw) * st:st], dw, dh, filt)
            assert r.max() <= mask
            dst[:, c::st] = r << sh_word
        out.append(dst.astype(np.uint8 if nbytes == 1 else np.uint16))
    return out


def batch(frames, fmt, bits, size, windows=None, filt=TRIANGLE):
    """n frames (lists of planes) -> n lists of planes; windows: None or one (ox, oy, ww, wh) per frame"""
    return [frame(p, fmt, bits, size, None if windows is None else tuple(windows[i]), filt) for i, p in enumerate(frames)]
