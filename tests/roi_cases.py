"""Region-of-interest (Maxshift, T.800 Annex H) unit blocks shared by tests/test_roi_streams.py (CPU: the vector factory
and the oracle) and tests/test_roi_gpu.py (the kernels against the oracle).  Test tooling only, no tests in it.

A Maxshift block: every magnitude is below 2^s, the ones inside the region are coded times 2^s, the band in M_b + s
bit-planes.  The decoder (jpeg2000htdec.c:1326-1328, jpeg2000dec.c:2071-2086) shifts every sample that has no bit in the
band's own M_b planes, which is every sample below 2^s, up by s: both kinds are on one scale again.

A hostile block: a descriptor whose shift is more than the word has room for, so that `val << roi_shift` carries
magnitude bits into bit 31 (which the reference then reads as the sign: it ORs the saved sign into the shifted word)
and beyond (lost)."""
import ctypes
import functools

import numpy as np

import oracle
import vecgen

SHAPES = [(64, 64), (32, 32), (63, 61), (1, 1), (3, 5), (1, 40), (40, 1), (128, 32), (1024, 4), (4, 1024), (17, 200)]
KS = [(3, 3), (8, 8), (8, 12), (13, 13), (14, 14)]           # (magnitude bits K, shift s); the last reaches 30 planes
# (flags & 3, f_step, i_step): dequantization_int with step 1 and another one, dequantization_float, dequantization_int_97
BRANCHES = [(1, 1.0, 32768), (1, 1.0, 40000), (0, 0.0123, 32768), (2, 1.0, 23456)]
HOSTILE_SHIFTS = (9, 12, 15)


def region(h, w, rng):
    """blobs of a few samples covering roughly half the block"""
    coarse = rng.random(((h + 2) // 3, (w + 2) // 3)) < 0.5
    return np.repeat(np.repeat(coarse, 3, 0), 3, 1)[:h, :w]


def dequant(t1, M_b, branch):
    """the oracle's dequantisation of a sign-magnitude block -> uint32 bit patterns (int32 samples or float32)"""
    transform, f_step, i_step = branch
    h, w = t1.shape
    t1 = np.ascontiguousarray(t1, dtype=np.int32)
    L, src = oracle.lib(), t1.ctypes.data_as(ctypes.c_void_p)
    if transform == 0:
        out = np.zeros((h, w), dtype=np.float32)
        L.orc_dequant_float(src, w, out.ctypes.data_as(ctypes.c_void_p), w, w, h, M_b, ctypes.c_float(f_step))
    else:
        out = np.zeros((h, w), dtype=np.int32)
        if transform == 1:
            L.orc_dequant_int(src, w, out.ctypes.data_as(ctypes.c_void_p), w, w, h, M_b, i_step)
        else:
            L.orc_dequant_int97(src, w, out.ctypes.data_as(ctypes.c_void_p), w, w, h, i_step)
    return out.view(np.uint32)


def carried_into_sign(t1_unshifted, M_b, shift):
    """fraction of the samples whose up-shift puts a magnitude bit into bit 31.  t1_unshifted: the block decoded with
    the same bit positions but no shift"""
    mag = t1_unshifted.view(np.uint32).astype(np.uint64) & 0x7FFFFFFF
    below = np.uint64(0xFFFFFFFF >> (M_b + 1))
    background = (mag & ~below & np.uint64(0xFFFFFFFF)) == 0
    return float((background & (((mag << np.uint64(shift)) >> np.uint64(31)) & np.uint64(1) == 1)).mean())


class HtBlock:
    """one HT block: coded bytes, the descriptor's numbers, the source values (None where the coding is lossy or the
    descriptor hostile) and the oracle's sign-magnitude output"""

    def __init__(self, vals, scaled, passes, causal, roi, hostile=0, min_planes=0):
        h, w = scaled.shape
        self.w, self.h, self.passes, self.causal, self.roi = w, h, passes, causal, roi
        self.data, self.lcup, self.lref, maxU = vecgen.encode_block(scaled, passes, causal)
        p = 1 if passes > 1 else 0
        # bit-planes the block is coded in; min_planes: a block whose region is empty or all zero still is one of a band of
        # M_b + s planes with M_b > K (else its background would be shifted out of the word)
        self.planes = max(max(maxU + p, 1) + 1, min_planes)
        assert self.planes <= 30
        self.zbp = self.planes - 1 - p
        self.M_b = self.planes - roi
        if hostile:                                              # background = below 2^8; `hostile` bits too far up
            self.M_b, self.roi = self.planes - 8, self.planes - 8 + hostile
            roi = self.roi
        self.vals = vals
        ret, self.t1 = oracle.ht_decode_block(self.data, self.lcup, self.lref, passes, self.zbp, w, h, self.M_b,
                                              roi_shift=roi, vsc=causal)
        assert ret == 1

    def unshifted(self):
        ret, t1 = oracle.ht_decode_block(self.data, self.lcup, self.lref, self.passes, self.zbp, self.w, self.h, self.M_b,
                                         roi_shift=0, vsc=self.causal)
        assert ret == 1
        return t1


@functools.lru_cache(maxsize=None)
def ht_blocks():
    """ROI blocks of every shape, pass count and (K, s), a block without shift after every third of them"""
    rng = np.random.default_rng(4242)
    out = []
    for (w, h) in SHAPES:
        for passes in (1, 2, 3):
            causal = passes == 3 and w % 2 == 0
            for K, s in KS:
                vals = rng.integers(-(1 << K) + 1, 1 << K, (h, w))
                scaled = np.where(region(h, w, rng), vals * (1 << s), vals)
                out.append(HtBlock(vals if passes != 2 else None, scaled, passes, causal, s, min_planes=K + s + 1))
                if len(out) % 4 == 3:
                    v = rng.integers(-200, 201, (h, w))
                    out.append(HtBlock(v if passes != 2 else None, v, passes, causal, 0))
    return out


@functools.lru_cache(maxsize=None)
def ht_hostile_blocks():
    """magnitudes of 14 bits in 16 planes or so, M_b = planes - 8 (about 8), seven samples in ten background (below 2^8),
    shifts 1, 4 and 7 more than the 8 that Maxshift would use (9, 12 and 15 with 16 planes): bit 7, 4 or 1 of a
    background magnitude lands in bit 31"""
    rng = np.random.default_rng(4343)
    out = []
    for (w, h) in [(32, 32), (63, 61), (128, 32)]:
        for passes in (1, 3):
            for extra in (1, 4, 7):
                bg = rng.integers(-255, 256, (h, w))
                fg = rng.integers(1, 64, (h, w)) * 256 * rng.choice([-1, 1], (h, w))
                scaled = np.where(rng.random((h, w)) < 0.3, fg, bg)
                out.append(HtBlock(None, scaled, passes, False, 0, hostile=extra))
    return out


class MqBlock:
    """one Part-1 block, laid out as Tier-2 does; nonzerobits = the planes coded (what a Maxshift stream signals)"""

    def __init__(self, vals, scaled, style, band, roi, M_b=None):
        h, w = scaled.shape
        self.w, self.h, self.style, self.band, self.roi, self.vals = w, h, style, band, roi, vals
        seg, lens, passes, self.K, self.npasses = vecgen.encode_block_p1(scaled, band=band, style=style)
        self.data, self.length, self.starts = oracle.mq_block_layout(seg, lens, passes, style)
        self.M_b = self.K - roi + 2 if M_b is None else M_b
        self.ret, self.t1 = oracle.mq_decode_block(self.data, self.length, self.npasses, self.K, w, h, self.M_b, style, band,
                                                   self.starts, roi_shift=roi)

    def unshifted(self):
        # bpno = nonzerobits - 1 + 31 - M_b - 1 - roi_shift: the same bit positions come from M_b + roi_shift and no shift
        return oracle.mq_decode_block(self.data, self.length, self.npasses, self.K, self.w, self.h, self.M_b + self.roi,
                                      self.style, self.band, self.starts, roi_shift=0)[1]


@functools.lru_cache(maxsize=None)
def mq_blocks():
    rng = np.random.default_rng(4444)
    out = []
    for s in (1, 7, 12):
        for (w, h) in [(32, 32), (128, 32), (5, 3)]:
            for style in (0, 0x2F):
                K = min(s, 9)
                vals = rng.integers(-(1 << K) + 1, 1 << K, (h, w))
                vals[0, 0] = (1 << K) - 1
                scaled = np.where(region(h, w, rng), vals * (1 << s), vals)
                out.append(MqBlock(vals, scaled, style, int(rng.integers(0, 4)), s))
                if s == 7:
                    out.append(MqBlock(vals, vals, style, int(rng.integers(0, 4)), 0))
    return out


@functools.lru_cache(maxsize=None)
def mq_hostile_blocks():
    """M_b = 8 and magnitudes of up to `shift` bits: every sample is background, bit 8 of a magnitude lands in bit 31"""
    rng = np.random.default_rng(4545)
    out = []
    for (w, h) in [(32, 32), (128, 32), (5, 3)]:
        for shift in HOSTILE_SHIFTS:
            vals = rng.integers(-(1 << shift) + 1, 1 << shift, (h, w))
            vals[0, 0] = (1 << shift) - 1
            out.append(MqBlock(None, vals, 0, int(rng.integers(0, 4)), shift, M_b=8))
    return out
