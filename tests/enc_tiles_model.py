"""numpy model of the encoder's stages for tiled frames (test tooling): the tile grid (T.800 B.3), the tile-components'
rectangles, and the coefficient planes of a tiled frame, built tile-component by tile-component: every tile-component's
Mallat layout sits in that tile-component's rectangle of the component plane, as htj2k_enc_layout describes it.

5/3 is the oracle's forward transform (oracle.fdwt with the tile-component's border).  9/7 is a float32 restatement of
the vector factory's fwd97_1d / fwd_dwt for a line that starts at any position, in the style of enc97_model.py: the
samples at even positions are low-pass and come first, the extension reflects about the first and the last sample, a
line of one sample is scaled by 1 / X at an even position and by 2 / K at an odd one.  arbitrate() is enc_opj.arbitrate
for tiled streams: the float64 synthesis of every tile-component at its origin."""
import numpy as np

import enc97_model as e97
import enc_model as em
import enc_opj
import oracle
import rc_model as rc

F = np.float32
TWO_OVER_K97 = F(2) / e97.K97          # `2.0f / K97`, folded in float


def cdiv(a, b):
    return -(-a // b)


def tile_size(w, h, tile):
    """the resolved tile size: 0 in a direction means the image's"""
    return tile[0] or w, tile[1] or h


def grid(w, h, tile):
    """[(x0, y0, x1, y1)] of the tiles on the reference grid, in raster order of the tile index"""
    tw, th = tile_size(w, h, tile)
    return [(tx * tw, ty * th, min((tx + 1) * tw, w), min((ty + 1) * th, h))
            for ty in range(cdiv(h, th)) for tx in range(cdiv(w, tw))]


def sub(fmt):
    """[(dx, dy)] of the layout's components"""
    nc, (sx, sy), _, _ = em.layout(fmt)
    return [(1 << (sx if c in (1, 2) else 0), 1 << (sy if c in (1, 2) else 0)) for c in range(nc)]


def tile_rects(fmt, w, h, tile):
    """per tile, per component: the tile-component's (x0, y0, x1, y1) in the component plane"""
    return [[(cdiv(x0, dx), cdiv(y0, dy), cdiv(x1, dx), cdiv(y1, dy)) for dx, dy in sub(fmt)]
            for x0, y0, x1, y1 in grid(w, h, tile)]


def refused(fmt, w, h, tile):
    """what the encoder must refuse: more than 65535 tiles, an empty tile-component, one beyond 32768 samples"""
    tw, th = tile_size(w, h, tile)
    if cdiv(w, tw) * cdiv(h, th) > 65535:
        return True
    return any(x1 <= x0 or y1 <= y0 or x1 - x0 > 32768 or y1 - y0 > 32768
               for rects in tile_rects(fmt, w, h, tile) for x0, y0, x1, y1 in rects)


def low_count(i0, i1, lev):
    """samples of the line i0 .. i1 - 1 that are low-pass at every level up to lev"""
    return cdiv(i1, 1 << lev) - cdiv(i0, 1 << lev)


def dwt97(x, axis, i0):
    """one forward 9/7 level along `axis` of a line whose first sample is at position i0"""
    x = np.moveaxis(np.asarray(x, dtype=np.float32), axis, 0)
    n, par = x.shape[0], i0 & 1
    if n == 1:
        return np.moveaxis(x * (TWO_OVER_K97 if par else e97.INV_X97), 0, axis)

    def ref(j):
        j = np.abs(j)
        return np.where(j >= n, 2 * (n - 1) - j, j)

    p = x.copy()
    odd, even = np.arange(1 - par, n, 2), np.arange(par, n, 2)
    for c, pos in ((-e97.A97, odd), (-e97.B97, even), (e97.G97, odd), (e97.D97, even)):
        p[pos] = p[pos] + c * (p[ref(pos - 1)] + p[ref(pos + 1)])
    return np.moveaxis(np.concatenate([p[even], p[odd]], 0), 0, axis)


def fdwt97(plane, x0, y0, levels):
    """the forward 9/7 of a tile-component whose first sample is at (x0, y0): vertical then horizontal at each level"""
    p = np.array(plane, dtype=np.float32)
    h, w = p.shape
    for lev in range(levels):
        lw, lh = low_count(x0, x0 + w, lev), low_count(y0, y0 + h, lev)
        if lw < 1 or lh < 1:
            break
        r = dwt97(p[:lh, :lw], 0, cdiv(y0, 1 << lev))
        p[:lh, :lw] = dwt97(r, 1, cdiv(x0, 1 << lev))
    return p


def fdwt53(plane, x0, y0, levels):
    """the oracle's forward 5/3 of a tile-component whose first sample is at (x0, y0)"""
    a = np.ascontiguousarray(plane, dtype=np.int32)
    h, w = a.shape
    return oracle.fdwt(a, ((x0, x0 + w), (y0, y0 + h)), levels, 1)


def band_map(x0, y0, x1, y1, nl):
    """band entry of every sample of the tile-component's Mallat layout"""
    def level(i0, i1):
        x = np.arange(i1 - i0, dtype=np.int64)
        lv = np.full(i1 - i0, nl + 1)
        for l in range(nl, 0, -1):
            lv = np.where(x >= low_count(i0, i1, l), l, lv)
        return lv
    lx, ly = level(x0, x1)[None, :], level(y0, y1)[:, None]
    l = np.minimum(lx, ly)
    g = 3 * (nl - l) + (lx == l) * 1 + (ly == l) * 2
    return np.where(l > nl, 0, g)


def quantise(plane, rect, step_of_band, nl):
    st = np.array([float(s) for s in step_of_band], dtype=np.float64)[band_map(*rect, nl)]
    m = np.minimum(np.floor(np.abs(plane.astype(np.float64)) / st), 2147483000.0).astype(np.int64)
    return np.where(plane < 0, -m, m).astype(np.int32)


def coefficient_planes(comps, fmt, w, h, bits, levels, mct, tile, qstep=None):
    """what the encoder hands the HT block coder for a tiled frame: per component one int32 plane, 5/3 coefficients
    (qstep None) or 9/7 quantisation indices at base step qstep"""
    if qstep is None:
        v = em.components(comps, bits, mct)
    else:
        v = e97.components(comps, bits, mct)
        st = [s for _, _, s in e97.steps(qstep, bits, levels)]
    out = [np.zeros(c.shape, np.int32) for c in v]
    for rects in tile_rects(fmt, w, h, tile):
        for c, (x0, y0, x1, y1) in enumerate(rects):
            part = v[c][y0:y1, x0:x1]
            if qstep is None:
                out[c][y0:y1, x0:x1] = fdwt53(part, x0, y0, levels)
            else:
                out[c][y0:y1, x0:x1] = quantise(fdwt97(part, x0, y0, levels), (x0, y0, x1, y1), st, levels)
    return out


def code_blocks(planes, blocks, at=None):
    """vecgen's cleanup segment of every block of `blocks` (Encoder.layout) -> ([bytes], [max U]); at: None, or per block
    the bit-plane it is coded from (-1: left out)"""
    coded = [rc.code_block(rc.block_view(planes, b), 0 if at is None else at[i]) for i, b in enumerate(blocks)]
    return [c[0] for c in coded], [c[2] for c in coded]


def idwt97_f64(plane, x0, y0, levels, high_scale=1.0):
    """inverse of fdwt97 in float64 (enc_opj.idwt97_f64 for a tile-component whose first sample is at (x0, y0));
    high_scale: a factor on the high-pass samples of every one-dimensional step of two samples or more"""
    p = np.array(plane, dtype=np.float64)
    h, w = p.shape

    def inv(y, axis, i0):
        y = np.moveaxis(y, axis, 0)
        n, par = y.shape[0], i0 & 1
        if n == 1:
            return np.moveaxis(y * (enc_opj.K97 / 2 if par else enc_opj.X97), 0, axis)
        nl = (n + 1 - par) // 2
        even, odd = np.arange(par, n, 2), np.arange(1 - par, n, 2)
        x = np.empty_like(y)
        x[even], x[odd] = y[:nl], y[nl:] * high_scale
        ref = lambda j: np.where(np.abs(j) >= n, 2 * (n - 1) - np.abs(j), np.abs(j))
        for c, pos in ((enc_opj.D97, even), (enc_opj.G97, odd), (-enc_opj.B97, even), (-enc_opj.A97, odd)):
            x[pos] = x[pos] - c * (x[ref(pos - 1)] + x[ref(pos + 1)])
        return np.moveaxis(x, 0, axis)

    for lev in range(levels - 1, -1, -1):
        lw, lh = low_count(x0, x0 + w, lev), low_count(y0, y0 + h, lev)
        if lw >= 1 and lh >= 1:
            p[:lh, :lw] = inv(inv(p[:lh, :lw], 1, cdiv(x0, 1 << lev)), 0, cdiv(y0, 1 << lev))
    return p


def arbitrate(cs, fmt, bits, w, h, tile, orc, oracle_pixels, opj_pixels):
    """enc_opj.arbitrate for a tiled 9/7 stream of one component: the oracle's dequantised coefficients of every
    tile-component through the float64 synthesis at that tile-component's origin, with T.800's constants and with
    OpenJPEG's fixed-point 2 / K.  None when each decoder is within one LSB of its own synthesis, else a string."""
    if em.layout(fmt)[0] != 1:
        return "no arbitration for layouts of several components"
    levels = cs[cs.index(b"\xff\x52") + 9]
    orc.decode_blocks(cs, req_pix_fmt=em.pix(fmt))
    rects = [r[0] for r in tile_rects(fmt, w, h, tile)]
    assert orc.num_tilecomps() == len(rects)
    coef = [np.array(orc.plane(t), np.float32) for t in range(len(rects))]

    def px(scale):
        v = np.zeros((h, w), np.float64)
        for c, (x0, y0, x1, y1) in zip(coef, rects):
            v[y0:y1, x0:x1] = idwt97_f64(c.reshape(y1 - y0, x1 - x0), x0, y0, levels, scale)
        v = np.floor(v + (1 << (bits - 1)) + 0.5)
        return np.clip(v, 0, (1 << bits) - 1).astype(np.int64) << em.shift(fmt, bits)

    d_orc = int(np.abs(oracle_pixels - px(1.0)).max())
    d_opj = int(np.abs(opj_pixels - px(enc_opj.OPJ_TWO_INVK / (2 / enc_opj.K97))).max())
    if d_orc > enc_opj.lsb(fmt, bits):
        return "the oracle is %d from the float64 synthesis of T.800" % d_orc
    if d_opj > enc_opj.lsb(fmt, bits):
        return "OpenJPEG is %d from the float64 synthesis with its own constant" % d_opj
    return None
