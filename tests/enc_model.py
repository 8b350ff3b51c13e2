"""numpy model of the lossless encoder's transform stages (test tooling): sample unpacking as the inverse of the
decoder's pack stage, DC level shift, forward RCT (T.800 G.2.1) and the forward 5/3 transform (T.800 F.4.8.2,
origin 0, symmetric extension) into the Mallat layout.  Block coding and stream writing are vecgen's
(tests/vecgen.py) or the product's; this module has neither."""
import numpy as np

import ffmpeg_ht_amd as m

RGB = ("rgb24", "rgba", "rgb48le", "rgba64le")
SHIFT16 = ("rgb48le", "rgba64le", "gray16le")
PACKED = {"rgb24": 3, "rgba": 4, "rgb48le": 3, "rgba64le": 4, "gray": 1, "ya8": 2, "gray16le": 1, "ya16le": 2}


def layout(fmt):
    """(ncomp, chroma log2 (w, h), bytes per sample, layout depth)"""
    if fmt in PACKED:
        depth = 16 if fmt in ("rgb48le", "rgba64le", "gray16le", "ya16le") else 8
        return PACKED[fmt], (0, 0), 2 if depth == 16 else 1, depth
    base = fmt.replace("le", "")
    nc = 4 if base.startswith("yuva") else 3
    digits = "".join(ch for ch in base.split("p")[-1] if ch.isdigit())
    depth = int(digits) if digits else 8
    sub = base[4:7] if nc == 4 else base[3:6]
    cw, ch = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "440": (0, 1), "411": (2, 0), "410": (2, 2)}[sub]
    return nc, (cw, ch), 2 if depth > 8 else 1, depth


def comp_dims(fmt, w, h):
    nc, (sx, sy), _, _ = layout(fmt)
    return [(-(-w // (1 << (sx if c in (1, 2) else 0))), -(-h // (1 << (sy if c in (1, 2) else 0)))) for c in range(nc)]


def shift(fmt, bits):
    return 8 - bits if bits <= 8 else (16 - bits if fmt in SHIFT16 else 0)


def to_planes(comps, fmt, bits):
    """component arrays (values < 2^bits) -> the layout's planes as the decoder writes them"""
    nc, _, nbytes, _ = layout(fmt)
    dt = np.uint8 if nbytes == 1 else np.uint16
    s = shift(fmt, bits)
    if fmt in PACKED:
        return [np.stack([c.astype(np.int64) << s for c in comps], -1).astype(dt).reshape(comps[0].shape[0], -1)]
    return [(c.astype(np.int64) << s).astype(dt) for c in comps]


def dwt53(x, axis):
    """one forward 5/3 level along `axis`: low-pass outputs first"""
    x = np.moveaxis(np.asarray(x, dtype=np.int64), axis, 0)
    n = x.shape[0]
    if n == 1:
        return np.moveaxis(x, 0, axis)

    def ref(j):
        j = np.abs(j)
        return np.where(j >= n, 2 * (n - 1) - j, j)

    odd = np.arange(1, n, 2)
    d = x[odd] - ((x[odd - 1] + x[ref(odd + 1)]) >> 1)
    even = np.arange(0, n, 2)
    dl, dr = (ref(even - 1) - 1) // 2, (ref(even + 1) - 1) // 2
    s = x[even] + ((d[dl] + d[dr] + 2) >> 2)
    return np.moveaxis(np.concatenate([s, d], 0), 0, axis)


def fdwt(plane, levels):
    p = np.array(plane, dtype=np.int64)
    h, w = p.shape
    for lev in range(levels):
        lw, lh = -(-w // (1 << lev)), -(-h // (1 << lev))
        if lw <= 1 and lh <= 1:
            break
        r = dwt53(p[:lh, :lw], 0)
        p[:lh, :lw] = dwt53(r, 1)
    return p


def components(comps, bits, mct):
    """level shift (+ RCT of components 0..2)"""
    v = [c.astype(np.int64) - (1 << (bits - 1)) for c in comps]
    if mct:
        r, g, b = v[0], v[1], v[2]
        v[0], v[1], v[2] = (r + 2 * g + b) >> 2, b - g, r - g
    return v


def coefficient_planes(comps, fmt, bits, levels, mct):
    return [fdwt(c, levels) for c in components(comps, bits, mct)]


def qcd_guard_bits(cs):
    i = cs.index(b"\xff\x5c")
    return cs[i + 4] >> 5


def vecgen_args(fmt, w, h, bits, levels, cb, mct, guard):
    nc, (sx, sy), _, _ = layout(fmt)
    dx = [1 << (sx if c in (1, 2) else 0) for c in range(nc)]
    dy = [1 << (sy if c in (1, 2) else 0) for c in range(nc)]
    return dict(depth=bits, dx=dx, dy=dy, nlevels=levels, cb=cb, mct=int(mct), guard_bits=guard, rsiz=0x4000,
                width=w, height=h)


def mct_default(fmt):
    return fmt in RGB


def pix(fmt):
    return m.PIX_NAMES.index(fmt)
