"""The transcoder's block rule (include/htj2k_amd.h, "transcoding") restated for the tests, and what they
read from a codestream's main header.  Test tooling only.

A Part-1 block has K coded bit-planes and n passes; n = 1 + 3 k + r, its last cleanup pass coded plane pc = K - 1 - k.
r = 0: one HT cleanup pass at pc; r = 1: cleanup at pc, SigProp at pc - 1; r = 2: cleanup at pc, SigProp and MagRef at
pc - 1.  Where nothing is significant at pc or the refinement segment would be empty: one cleanup pass at pc."""
import struct

import numpy as np


def rule(K, n):
    """-> (plane of the last pass, passes) as the encoder reports them, (-1, 1) for a block without passes"""
    if n == 0:
        return -1, 1
    k, r = divmod(n - 1, 3)
    pc = K - 1 - k
    return (pc - 1 if r else pc), 1 + r


def raw_index(t1, M_b, K, n):
    """the signed quantiser indices in decode_cblk's sign-magnitude words: the magnitude down from bit 31 - M_b, without
    the half bit below the last plane a sample was coded in"""
    t1 = np.asarray(t1)
    m = ((t1.astype(np.int64) & 0x7FFFFFFF) >> (31 - M_b))
    if n:
        k, r = divmod(n - 1, 3)
        pc = K - 1 - k
        if r == 0:
            m = (m >> pc) << pc
        elif r == 2:
            m = (m >> (pc - 1)) << (pc - 1)
        else:                                              # SigProp alone: the samples it made significant end a plane lower
            m = np.where(m >> pc, (m >> pc) << pc, (m >> (pc - 1)) << (pc - 1))
    return np.where(t1 < 0, -m, m).astype(np.int32)


def ht_form(idx, K, n):
    """what the HT block of these indices is: (plane of the last pass, passes) after the fall-back rule, or None for a
    block that is left out (no passes, or all zero)"""
    p, passes = rule(K, n)
    if n == 0 or not np.any(idx):
        return None
    if passes > 1:
        nsig = np.count_nonzero(np.abs(idx.astype(np.int64)) >> (p + 1))
        if nsig == 0 or (passes == 2 and nsig == idx.size):
            return p + 1, 1
    return p, passes


def shifted(idx, p):
    a = idx.astype(np.int64)
    return (np.sign(a) * (np.abs(a) >> p)).astype(np.int32)


def main_header_quant(cs):
    """-> (ncomp, {component: (style, guard, [exponents], [mantissas])}) from QCD (key -1) and QCC of the main header"""
    assert cs[:2] == b"\xff\x4f"
    pos, out, ncomp = 2, {}, 0
    while cs[pos:pos + 2] != b"\xff\x90":
        mk, ln = struct.unpack(">HH", cs[pos:pos + 4])
        seg = cs[pos + 4:pos + 2 + ln]
        if mk == 0xFF51:
            ncomp = struct.unpack(">H", seg[34:36])[0]
        if mk in (0xFF5C, 0xFF5D):
            comp = -1
            if mk == 0xFF5D:
                comp, seg = (seg[0], seg[1:]) if ncomp < 257 else (struct.unpack(">H", seg[:2])[0], seg[2:])
            style, guard, body = seg[0] & 31, seg[0] >> 5, seg[1:]
            if style == 0:
                expn, mant = [b >> 3 for b in body], [0] * len(body)
            else:
                v = struct.unpack(">%dH" % (len(body) // 2), body)
                expn, mant = [x >> 11 for x in v], [x & 0x7FF for x in v]
            out[comp] = (style, guard, expn, mant)
        pos += 2 + ln
    return ncomp, out


def quant_tables(cs, nbands):
    """-> (guard, expn[c][b], mant[c][b]) of every component, a derived QCD expanded as T.800 E.1.1.1 says"""
    ncomp, q = main_header_quant(cs)
    guard, expn, mant = None, [], []
    for c in range(ncomp):
        style, g, e, m = q.get(c, q[-1])
        if style == 1:
            e, m = [max(e[0] - ((b - 1) // 3 if b else 0), 0) for b in range(nbands)], [m[0]] * nbands
        assert guard in (None, g)
        guard = g
        expn.append(list(e[:nbands]))
        mant.append(list(m[:nbands]))
    return guard, expn, mant
