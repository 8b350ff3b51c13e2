"""OpenJPEG (through Pillow) as a third decoder of the encoder's streams (test tooling, no tests in it): which layouts
Pillow hands back sample for sample, its pixels and the oracle's / the source's in one arrangement, and the comparison
rule of tests/test_encode_openjpeg.py, shared with tools/gpu_encode_random.py.

Pillow returns `gray` as L, `ya8` as LA, `rgb24` / `yuv444p` as RGB, `rgba` / `yuva444p` as RGBA (raw codestreams carry
no colourspace, so the three components come back as they are) and `gray16le` as I;16, samples below the container's
depth shifted up as the decoder's pack stage shifts them.  Subsampled layouts are upsampled and multi-component
layouts deeper than 8 bits are narrowed to 8 bits, so those are not compared here."""
import io

import numpy as np

import enc_model as em

try:
    from PIL import Image, features
    HAVE_OPJ = bool(features.check("jpg_2000"))
except Exception:  # pragma: no cover
    HAVE_OPJ = False

LAYOUTS = [("gray", 8), ("gray", 5), ("ya8", 8), ("rgb24", 8), ("rgba", 8), ("yuv444p", 8), ("yuva444p", 8),
           ("gray16le", 16), ("gray16le", 12), ("gray16le", 10)]
MODES = {"gray": "L", "ya8": "LA", "rgb24": "RGB", "rgba": "RGBA", "yuv444p": "RGB", "yuva444p": "RGBA", "gray16le": "I;16"}


def exact(fmt, bits):
    return (fmt, bits) in LAYOUTS


def lsb(fmt, bits):
    """one LSB of the coded depth in the container's units"""
    return 1 << em.shift(fmt, bits)


def arrange(planes, fmt, w, h):
    """the layout's planes (em.to_planes, Decoder.decode, OracleDecoder.decode) -> int64 array shaped as Pillow's"""
    nc = em.layout(fmt)[0]
    if fmt in em.PACKED:
        a = np.asarray(planes[0]).reshape(h, w, nc)
    else:
        a = np.stack([np.asarray(p).reshape(h, w) for p in planes], -1)
    return (a[:, :, 0] if nc == 1 else a).astype(np.int64)


def pixels(cs, fmt):
    """OpenJPEG's decode of the codestream; raises when Pillow cannot open it or returns another mode"""
    im = Image.open(io.BytesIO(cs))
    im.load()
    if im.mode != MODES[fmt]:
        raise AssertionError("Pillow returned mode %s for %s" % (im.mode, fmt))
    return np.array(im).astype(np.int64)


# T.800 Table F.4
A97, B97, G97, D97, K97 = 1.586134342059924, 0.052980118572961, 0.882911075530934, 0.443506852043971, 1.230174104914001
X97 = 0.812893066115961                                   # the project's un-normalised lifting scales a line of one sample
OPJ_TWO_INVK = 13318 / 8192                               # what OpenJPEG multiplies the high-pass samples by: 2 / K is 1.6257861...


def idwt97_f64(plane, levels, high_scale=1.0):
    """inverse 9/7 of a Mallat plane of un-normalised coefficients (the inverse of enc97_model.fdwt97) in float64;
    high_scale: a factor on the high-pass samples of every one-dimensional step"""
    p = np.array(plane, dtype=np.float64)
    h, w = p.shape

    def inv(y, axis):
        y = np.moveaxis(y, axis, 0)
        n = y.shape[0]
        if n == 1:
            return np.moveaxis(y * X97, 0, axis)
        nl = (n + 1) // 2
        even, odd = np.arange(0, n, 2), np.arange(1, n, 2)
        x = np.empty_like(y)
        x[even], x[odd] = y[:nl], y[nl:] * high_scale
        ref = lambda j: np.where(np.abs(j) >= n, 2 * (n - 1) - np.abs(j), np.abs(j))
        for c, pos in ((D97, even), (G97, odd), (-B97, even), (-A97, odd)):
            x[pos] = x[pos] - c * (x[ref(pos - 1)] + x[ref(pos + 1)])
        return np.moveaxis(x, 0, axis)

    for lev in range(levels - 1, -1, -1):
        lw, lh = -(-w // (1 << lev)), -(-h // (1 << lev))
        p[:lh, :lw] = inv(inv(p[:lh, :lw], 1), 0)
    return p


def arbitrate(cs, fmt, bits, w, h, orc, oracle_pixels, opj_pixels):
    """OpenJPEG and the oracle are more than one LSB apart on a 9/7 stream of one component: who is right?  The oracle's
    dequantised coefficients go through the inverse 9/7 in float64 twice: with the constants of T.800 Table F.4, and
    with the high-pass samples of every step scaled by 13318 / 8192 over 2 / K -- OpenJPEG multiplies them by the
    fixed-point constant 1.625732422 where 2 / K is 1.625786132, a relative error of 3.3e-5 that reaches several LSB of
    16-bit samples with strong high-pass content and 0.01 LSB of 8-bit ones.  None when the oracle is within one LSB of
    the first and OpenJPEG within one LSB of the second (its difference is that constant and nothing else), else a
    string."""
    if em.layout(fmt)[0] != 1:
        return "no arbitration for layouts of several components"
    levels = cs[cs.index(b"\xff\x52") + 9]
    orc.decode_blocks(cs, req_pix_fmt=em.pix(fmt))
    coef = np.array(orc.plane(0), np.float32).reshape(h, w)

    def px(scale):
        v = np.floor(idwt97_f64(coef, levels, scale) + (1 << (bits - 1)) + 0.5)
        return np.clip(v, 0, (1 << bits) - 1).astype(np.int64) << em.shift(fmt, bits)

    d_orc = int(np.abs(oracle_pixels - px(1.0)).max())
    d_opj = int(np.abs(opj_pixels - px(OPJ_TWO_INVK / (2 / K97))).max())
    if d_orc > lsb(fmt, bits):
        return "the oracle is %d from the float64 synthesis of T.800" % d_orc
    if d_opj > lsb(fmt, bits):
        return "OpenJPEG is %d from the float64 synthesis with its own constant" % d_opj
    return None


def compare(cs, fmt, bits, w, h, oracle_planes, irreversible, source_planes=None, orc=None, arbitrated=None):
    """None when OpenJPEG agrees, else a string that says how it does not: 5/3 pixels equal the oracle's exactly (and the
    source's where `source_planes` is given: a lossless stream), 9/7 pixels within one LSB of the coded depth.  With
    `orc` (an OracleDecoder) a 9/7 difference beyond one LSB goes to arbitrate(); `arbitrated` (a list) records it."""
    got = pixels(cs, fmt)
    want = arrange(oracle_planes, fmt, w, h)
    if got.shape != want.shape:
        return "shape %r against the oracle's %r" % (got.shape, want.shape)
    d = int(np.abs(got - want).max())
    if d > (lsb(fmt, bits) if irreversible else 0):
        why = "differs from the oracle by %d (one LSB is %d)" % (d, lsb(fmt, bits))
        if not irreversible or orc is None:
            return why
        verdict = arbitrate(cs, fmt, bits, w, h, orc, want, got)
        if verdict is not None:
            return why + "; " + verdict
        if arbitrated is not None:
            arbitrated.append((fmt, bits, w, h, d))
    if source_planes is not None and not np.array_equal(got, arrange(source_planes, fmt, w, h)):
        return "lossless stream does not return the source"
    return None
