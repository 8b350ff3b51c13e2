"""One reader of a transcoder source for the tests: per block of the encoder's layout the quantiser indices, what the
block rule gives the block, and the expected output rebuilt byte for byte on the CPU.  Read from the oracle's parse and
block decode (tests/oracle.py); the rule is tests/xc_model.py and, for HT blocks, tests/xc_ht_model.py; the blocks are
coded by the vector factory (tests/rc_passes_model.py) and written by the product's host writer given the source's
quantisation (Encoder.assemble_quant).  No GPU.  Test tooling only."""
import numpy as np

import ffmpeg_ht_amd as m
import rc_passes_model as pm
import xc_ht_model as xh
import xc_model as xm
import xc_rc_model as xrm


def enc_opts(kw):
    """the encoder options that give the layout of a source made with the vector factory's keywords kw"""
    return dict(levels=kw["nlevels"], cb=kw.get("cb", (6, 6)), mct=kw.get("mct", 0), irreversible=kw.get("transform", 1) == 0,
                tile=kw.get("tile", (0, 0)))


def signed_words(word, neg):
    """sign-magnitude words as int32: bit 31 the sign"""
    return (word.astype(np.uint32) | (neg.astype(np.uint32) << 31)).view(np.int32)


def block_rects(orc, src, tiles, ncomp):
    """the oracle's block table of src with every block's place: [(entry, tile-component, x and y in the tile-component's
    plane, component, x and y in the component's plane)].  Leaves the oracle with the source's blocks decoded"""
    tab = orc.plan_blocks(src)
    orc.decode_blocks(src)
    base = [orc.plane_offset(t) for t in range(orc.num_tilecomps())]
    out = []
    for e in tab:
        tc = max(t for t in range(len(base)) if base[t] <= int(e["plane_off"]))
        x0, y0, x1, _ = tiles[tc // ncomp]["rects"][tc % ncomp]
        rel = int(e["plane_off"]) - base[tc]
        bx, by = rel % (x1 - x0), rel // (x1 - x0)
        out.append((e, tc, bx, by, tc % ncomp, x0 + bx, y0 + by))
    return out


class Source:
    """a Part-1, HT or MIXED stream and, per block of the encoder's layout: idx (the quantiser indices, read back off the
    oracle's dequantised planes), rule ((plane of the last pass, passes) of the block rule, each block by the rule of its
    own coder: an HT block as the Part-1 block xh.as_part1 names), ht (xm.ht_form: the rule after the fall-backs, None
    for a block that is left out), form (the finest form a budget may give the block), at (tile-component and rectangle)
    and part1 (the block's coder)"""

    def __init__(self, orc, src, kw):
        self.src, self.opts = src, enc_opts(kw)
        info = orc.probe(src)
        self.w, self.h, self.fmt, self.bits = info.width, info.height, info.pix_fmt, info.bits_per_raw_sample
        self.layout = m.Encoder.layout(self.w, self.h, self.fmt, self.bits, **self.opts)
        self.tiles = m.Encoder.tiles(self.w, self.h, self.fmt, self.bits, **self.opts)
        self.ncomp = 1 + max(b["comp"] for b in self.layout)
        where = {(b["comp"], b["x"], b["y"]): i for i, b in enumerate(self.layout)}
        tab = block_rects(orc, src, self.tiles, self.ncomp)
        n = len(self.layout)
        assert len(tab) == n, (len(tab), n)
        self.idx, self.rule, self.ht, self.form, self.at, self.part1 = ([None] * n for _ in range(6))
        for e, tc, bx, by, comp, x, y in tab:
            w, h, M_b = int(e["w"]), int(e["h"]), int(e["M_b"])
            i = where[(comp, x, y)]
            assert (self.layout[i]["w"], self.layout[i]["h"]) == (w, h) and self.idx[i] is None
            part1 = bool(e["flags"] & 4)
            K, n_p = (int(e["zbp"]), int(e["npasses"])) if part1 else xh.as_part1(M_b, int(e["zbp"]), int(e["npasses"]))
            coef = orc.plane(tc)[by:by + h, bx:bx + w]
            if coef.dtype == np.float32:                   # dequantization_float: the 31-bit word times f_step / 2^(31 - M_b)
                word = np.rint(np.abs(coef.astype(np.float64)) / float(e["f_step"]) * 2.0 ** (31 - M_b)).astype(np.int64)
            else:                                          # dequantization_int with step 1: the word >> (31 - M_b)
                assert int(e["i_step"]) == 32768
                word = np.abs(coef.astype(np.int64)) << (31 - M_b)
            self.idx[i] = xm.raw_index(signed_words(word, coef < 0), M_b, K, n_p)
            self.rule[i] = xm.rule(K, n_p)
            f = self.ht[i] = xm.ht_form(self.idx[i], K, n_p)
            self.form[i] = (self.rule[i][0] + (n_p > 0 and self.rule[i][1] > 1 and f is None), 1) if f is None else f
            self.at[i] = (tc, bx, by, w, h)
            self.part1[i] = part1
        assert all(v is not None for v in self.idx)
        self.guard, self.expn, self.mant = xm.quant_tables(src, 3 * self.opts["levels"] + 1)

    def forms(self):
        """per block (reported plane, reported passes, left out, (pr, k) of the rule): what a transcode without a budget
        reports in last_planes and last_passes"""
        return [(r[0] if f is None else f[0], 1 if f is None else f[1], f is None, r) for f, r in zip(self.ht, self.rule)]

    def stream(self, planes, passes):
        """the stream of the vector factory's blocks of the source's indices at these planes and passes, with the
        source's quantisation, through the product's host writer"""
        coded = [pm.code_block(v, p, k) if p >= 0 else (b"", 0, 0, 0, 1) for v, p, k in zip(self.idx, planes, passes)]
        for c, p, k in zip(coded, planes, passes):
            assert c[4] == k or c[1] == 0, (p, k, c[1:])         # the passes reported are the passes the block has
        return m.Encoder.assemble_quant(self.w, self.h, self.fmt, self.bits, [c[0] for c in coded], [c[2] for c in coded],
                                        [c[4] if c[1] else 1 for c in coded], planes, self.guard, self.expn, self.mant, **self.opts)

    def free(self):
        """the stream a transcode without a budget gives: every block in its source's form"""
        f = self.forms()
        return self.stream([p for p, _, _, _ in f], [k for _, k, _, _ in f])

    def empty(self):
        n = len(self.layout)
        return self.stream([-1] * n, [1] * n)

    def check_not_finer(self, planes, passes):
        for i, (p, k) in enumerate(zip(planes, passes)):
            pr, ks = self.rule[i]
            if pr < 0:
                assert (p, k) == (-1, 1), i
            elif p >= 0:
                assert p >= pr and (p > pr or k in xrm.ALLOWED_AT_0[ks]) and p >= self.form[i][0], (i, p, k, pr, ks)
