"""The transcoder's block rule for HT source blocks (include/htj2k_amd.h, "transcoding") restated for the
tests.  Test tooling only.

An HT block has n passes, placeholder passes included, and zbp zero bit-planes of its band's M_b.  n = 0: left out.
Otherwise P0 = (n - 1) / 3 placeholder sets, k = n - 3 P0 passes (1 .. 3), S_blk = zbp + P0, and its cleanup pass coded
plane pc = M_b - 1 - S_blk.  The block keeps its k passes: the last at pc - (k > 1).  In the terms of tests/xc_model.py
that is a Part-1 block of K = pc + 1 planes cut after k passes, so the fall-backs and the indices are read there."""
import numpy as np

import xc_model as xm


def split(M_b, zbp, n):
    """-> (pc, k); n > 0"""
    p0 = (n - 1) // 3
    return M_b - 1 - zbp - p0, n - 3 * p0


def as_part1(M_b, zbp, n):
    """-> (K, n') of the Part-1 block with the same cleanup plane and the same passes after it"""
    if n == 0:
        return 0, 0
    pc, k = split(M_b, zbp, n)
    return pc + 1, k


def rule(M_b, zbp, n):
    """-> (plane of the last pass, passes) as the encoder reports them, (-1, 1) for a block without passes; None where
    the passes run below plane 0 (HTJ2K_ERR_INVALIDDATA)"""
    if n == 0:
        return -1, 1
    pc, k = split(M_b, zbp, n)
    if pc - (k > 1) < 0:
        return None
    return pc - (k > 1), k


def raw_index(words, M_b, zbp, n):
    """the signed quantiser indices in ff_jpeg2000_decode_htj2k's sign-magnitude words: the magnitude down from bit
    31 - M_b with every half bit left out -- the cleanup pass's below pc (below pc - 1 where MagRef refined the sample),
    SigProp's below pc - 1"""
    return xm.raw_index(words, M_b, *as_part1(M_b, zbp, n))


def ht_form(idx, M_b, zbp, n):
    """(plane of the last pass, passes) after the fall-backs, or None for a block that is left out"""
    return xm.ht_form(idx, *as_part1(M_b, zbp, n))
