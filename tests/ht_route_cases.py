"""Unit HT block tables for every kernel route a job can take (knob "unit_ht" of htj2k_ht_blocks, include/htj2k_amd.h),
shared by tests/test_ht_route_cases.py (CPU: the blocks against the oracle, the tables against the routes' conditions)
and tests/test_ht_routes_gpu.py (the kernels against the oracle).  Test tooling only, no tests in it.

A block is coded once (vecgen.encode_block) and decoded once by the oracle (oracle.ht_decode_block); a table places
blocks, each with a dequantiser of roi_cases.BRANCHES, in a dirty sample buffer: shuffled, so that the blocks of one
wavefront differ in shape, content, M_b, zbp and pass count, every other one with a stride wider than the block, windows
at odd offsets where the route allows, gaps between them.  expected() is the whole buffer as it must come back.

M_b: the cleanup pass's magnitudes sit at bit pLSB = 30 - (P0 + zbp) of the oracle's words and the dequantiser reads from
bit 31 - M_b, so P0 + zbp = M_b - 1 - p (p = 1 with SigProp / MagRef passes) in every descriptor here; the least M_b whose
exponent bound P0 + zbp + 1 admits the block's largest exponent max_U is max(max_U + p, 1)."""
import functools

import numpy as np

import oracle
import roi_cases
import vecgen

# (w, h) by what the width selects: k_ht_vlc2 and four blocks per wave, k_ht_vlc2 and two, k_ht_vlc.  Heights 65, 129 and
# 130: one row past the 64-row register window of the multi-block kernels, twice past it, an odd last row
NARROW = [(1, 1), (2, 2), (3, 5), (1, 40), (31, 33), (32, 32), (17, 200), (2, 130), (32, 65), (31, 129), (16, 256), (4, 1024)]
MID = [(33, 1), (40, 1), (64, 3), (63, 61), (64, 64), (63, 65), (34, 70), (33, 124)]
WIDE = [(65, 7), (128, 32), (1024, 4)]
# more than 4096 samples: no codestream has such a block (jpeg2000htdec.c:1230-1232), the unit entry points refuse them as
# they refuse whatever a job could not hold, and no kernel ever sees one.  The oracle decodes them; (31, 129), (63, 65)
# and (33, 124) above are the nearest shapes a kernel may be given (at 33 columns and more nothing is taller than 124)
OVERSIZE = [(32, 129), (64, 65), (64, 130)]
TALL = {(17, 200), (16, 256), (4, 1024)}                     # in two classes only: the CPU reference is what takes the time
CLASSES = {"ones": (1, 0.05), "threes": (3, 0.5), "dense": (200, 1.0), "top16": (16383, 1.0), "top32": (1 << 28, 1.0)}
BR53 = roi_cases.BRANCHES[0]


class Block:
    """one coded block and what the oracle makes of it.  passes: coded passes (0: a block without any); P0: placeholder
    sets in front of them; extra: M_b above the least that decodes"""

    def __init__(self, shape, cls, vals, passes, P0=0, extra=0, causal=False):
        self.w, self.h = self.shape = shape
        self.cls, self.passes, self.P0, self.causal, self.bad = cls, passes, P0, causal, None
        # the source, where coding is lossless: one pass; three passes of a dense block (SigProp only reaches a sample
        # beside a significant one: the lone +-1 of a sparse block, below the cleanup pass's plane, are lost)
        self.vals = vals if passes == 1 or (passes == 3 and cls in ("dense", "top32")) else None
        if passes == 0:
            self.data, self.lcup, self.lref, self.max_U = b"", 0, 0, 0
            self.M_b, self.zbp, self.npasses, self.ret = 8, 7, 0, 1
            self.t1 = np.zeros((self.h, self.w), dtype=np.int32)
            return
        self.data, self.lcup, self.lref, self.max_U = vecgen.encode_block(vals, passes, causal)
        p = 1 if passes > 1 else 0
        self.least = max(self.max_U + p, 1)
        self.M_b = self.least + extra
        while self.M_b - 1 - p < P0:                         # room for the placeholder sets: zbp >= 0
            self.M_b += 1
        self.zbp = self.M_b - 1 - p - P0
        self.npasses = passes + 3 * P0
        self._decode()

    def _decode(self):
        self.ret, self.t1 = oracle.ht_decode_block(self.data, self.lcup, self.lref, self.npasses, self.zbp, self.w, self.h,
                                                   self.M_b, vsc=self.causal)

    def broken(self, how):
        """the three constructions of test_ht_block_errors_zero_the_block on a copy of this block"""
        b = Block.__new__(Block)
        b.__dict__.update(self.__dict__)
        b.bad, b.vals = how, None
        if how == "lcup":                                    # Lcup < 2
            b.lcup, b.lref = 1, 0
        elif how == "scup":                                  # Scup > Lcup
            d = bytearray(self.data)
            d[self.lcup - 1] = 0xFF
            b.data = bytes(d)
        elif how == "maxbp":                                 # zbp too small for the coded magnitudes: U > maxbp
            b.zbp, b.M_b = 2, 3
        else:
            raise ValueError(how)
        b._decode()
        return b

    @property
    def pcup(self):
        """length of the MagSgn segment (0 where Scup is not valid: the host sizes nothing from such a block)"""
        if self.npasses == 0 or self.lcup < 2:
            return 0
        scup = (self.data[self.lcup - 1] << 4) + (self.data[self.lcup - 2] & 15)
        return self.lcup - scup if 2 <= scup <= self.lcup and scup <= 4079 else 0

    @property
    def coded(self):
        return self.passes


def _values(rng, shape, cls):
    w, h = shape
    amp, density = CLASSES[cls]
    vals = rng.integers(-amp, amp + 1, (h, w))
    if density < 1.0:
        vals = np.where(rng.random((h, w)) < density, vals, 0)
    vals[0, 0] = amp                                         # the class's largest value is there: max_U is the class's own
    vals[-1, -1] = amp if w * h == 1 else -amp
    return vals


def classes_of(shape):
    if shape in OVERSIZE:
        return ["dense"]
    if shape in TALL:
        return ["ones", "dense"]
    return ["ones", "threes", "dense", "top32"] + (["top16"] if shape[0] <= 64 else [])


@functools.lru_cache(maxsize=None)
def blocks():
    """-> {(shape, class, kind): Block}; kind "c": the cleanup pass only, "r": with SigProp (and MagRef) passes, and for the
    oversize shapes "1", "2", "3": that many passes.  Pass counts, placeholder sets and M_b above the least cycle with
    different periods, so that all combinations turn up"""
    rng = np.random.default_rng(20240)
    out, i = {}, 0
    for shape in NARROW + MID + WIDE:
        w, h = shape
        for cls in classes_of(shape):
            vals = _values(rng, shape, cls)
            P0c, P0r = (0, 1, 0, 2, 0)[i % 5], (0, 0, 1, 0, 2, 0, 0)[i % 7]
            passes = 2 + i % 2
            if cls == "top16":                               # +-16383: max_U = 15, M_b = 15 is all the 16-bit routes take
                out[shape, cls, "c"] = Block(shape, cls, vals, 1, P0c, 0)
            elif cls == "top32":                             # +-2^28: max_U = 29; M_b = 29 and 30, the entry refuses more
                out[shape, cls, "c"] = Block(shape, cls, vals, 1, P0c, i % 2)
                out[shape, cls, "r"] = Block(shape, cls, vals, passes, P0r, (i + 1) % 2, causal=passes == 3 and w % 2 == 0)
            else:
                out[shape, cls, "c"] = Block(shape, cls, vals, 1, P0c, i % 4)
                out[shape, cls, "r"] = Block(shape, cls, vals, passes, P0r, (i // 2) % 4, causal=passes == 3 and w % 2 == 0)
            i += 1
    for shape in OVERSIZE:
        vals = _values(rng, shape, "dense")
        for passes in (1, 2, 3):
            out[shape, "dense", str(passes)] = Block(shape, "dense", vals, passes, 0, 1, causal=passes == 3)
    return out


def nopass(shape):
    return Block(shape, "nopass", None, 0)


@functools.lru_cache(maxsize=None)
def broken_blocks():
    """Lcup < 2, a bad Scup, an exponent bound above maxbp (zbp 2 under exponents of 9): on a 32 x 32 block of +-200"""
    base = blocks()[(32, 32), "dense", "c"]
    return tuple(base.broken(how) for how in ("lcup", "scup", "maxbp"))


# ---------------------------------------------------------------- what the host sizes, restated (htj2k_device.hip)
def ms_words(max_pcup):
    """ht_lds_layout: words of a block's un-stuffed MagSgn bits in LDS, from the table's longest segment"""
    return ((max_pcup * 8 + 31) // 32 + 3 + 3) & ~3


def multi_lds(nb, max_pcup):
    """bytes of LDS a wave of k_ht_decode_multi takes for its blocks' MagSgn bits"""
    return nb * (ms_words(max_pcup) + 4) * 4


MULTI_LDS_MAX = 12 * 1024                                    # the default of HTJ2K_MULTI_LDS


def multi_refine_lds(nb, max_lref, rows):
    """ht_multi_refine_lds(nb, ht_nsp(max_lref), rows)"""
    mr = (max_lref * 8 + 31) // 32 + 3
    return nb * (mr + 2 * (1 if nb == 4 else 2) * rows) * 4 + 512


def max_pcup_that_fits(nb):
    p = 0
    while multi_lds(nb, p + 1) <= MULTI_LDS_MAX:
        p += 1
    return p


# ---------------------------------------------------------------- tables
class Entry:
    """a block in a table: its dequantiser and where its window lies"""

    def __init__(self, block, branch, data_off, plane_off, stride):
        self.block, self.branch, self.data_off, self.plane_off, self.stride = block, branch, data_off, plane_off, stride

    @property
    def flags(self):
        return (8 if self.block.causal else 0) | self.branch[0]

    def want(self):
        """uint32 bit patterns of the window; zero for a block without passes and for one the oracle rejects"""
        b = self.block
        if b.npasses == 0 or b.ret != 1:
            return np.zeros((b.h, b.w), dtype=np.uint32)
        return roi_cases.dequant(b.t1, b.M_b, self.branch)


class Table:
    """route: the knob's value the table is built for; nb: blocks per wave it is meant to get there (route 2)"""

    def __init__(self, name, route, picks, seed, nb=0, refine=False, shuffle=True):
        self.name, self.route, self.nb, self.refine = name, route, nb, refine
        rng = np.random.default_rng(seed)
        picks = list(picks)
        if shuffle:
            picks = [picks[k] for k in rng.permutation(len(picks))]
        even = route == 3                                    # k_ht_decode_pair stores dwords: even strides and offsets
        self.entries, pool, offs = [], bytearray(), {}
        off = int(rng.integers(1, 4)) * 2 if even else int(rng.integers(1, 8)) | 1
        for k, (blk, branch) in enumerate(picks):
            if id(blk) not in offs:
                offs[id(blk)] = len(pool)
                pool += blk.data + b"\0" * ((-len(blk.data)) % 16)
            pad = 0 if k % 2 == 0 else (2 * int(rng.integers(1, 4)) if even else int(rng.integers(1, 6)))
            stride = blk.w + pad
            self.entries.append(Entry(blk, branch, offs[id(blk)], off, stride))
            off += (blk.h - 1) * stride + blk.w
            off += 2 * int(rng.integers(0, 3)) if even else int(rng.integers(0, 4))
        self.pool = bytes(pool) if pool else b"\0" * 16
        self.nsamples = off + 8
        self.fill = rng.integers(0, 1 << 32, self.nsamples, dtype=np.uint64).astype(np.uint32)

    @property
    def sixteen(self):
        return self.route in (3, 4)

    def expected(self):
        """the whole buffer after the call: uint32 words, or int16 samples (2 * nsamples of them) on routes 3 and 4"""
        if self.sixteen:
            out = self.fill.copy().view(np.int16)
        else:
            out = self.fill.copy()
        for e in self.entries:
            b, want = e.block, e.want()
            if self.sixteen:
                want = want.view(np.int32).astype(np.int16)
            for y in range(b.h):
                out[e.plane_off + y * e.stride:e.plane_off + y * e.stride + b.w] = want[y]
        return out

    def window(self, buf, e):
        b = e.block
        idx = e.plane_off + np.arange(b.h)[:, None] * e.stride + np.arange(b.w)[None, :]
        return buf[idx]

    def bad_status(self):
        return np.array([e.block.ret != 1 for e in self.entries])


def _pick(kinds, shapes, classes, max_pcup=None, refine_rows=None):
    """(shape, class, kind) blocks of the pool that a table admits: kind "r" blocks only up to refine_rows rows"""
    out = []
    for (shape, cls, kind), b in blocks().items():
        if shape not in shapes or cls not in classes or kind not in kinds:
            continue
        if max_pcup is not None and b.pcup > max_pcup:
            continue
        if kind == "r" and refine_rows is not None and b.h > refine_rows:
            continue
        out.append(b)
    return out


def _with_length(picks, shapes, rem, branch):
    """blocks without passes in between, as many as make the table's length n % 4 == rem (at least two)"""
    k = 0
    picks = list(picks)
    while k < 2 or len(picks) % 4 != rem:
        picks.append((nopass(shapes[(3 * k + rem) % len(shapes)]), branch))
        k += 1
    return picks


C32 = ("ones", "threes", "dense", "top32")
C16 = ("ones", "threes", "dense", "top16")


@functools.lru_cache(maxsize=None)
def route2_tables():
    """k_ht_decode_multi: per dequantiser (one transform per table) cleanup-only (REFINE false) and with blocks of 2 and 3
    passes of at most 64 rows mixed in (REFINE true; the cleanup-only blocks beside them are of any height), all blocks at
    most 32 columns wide (four per wave) and with some of 33 to 64 (two per wave).  A table's longest MagSgn segment sizes
    the LDS of every wave: only blocks whose own segment keeps four resp. two of its size within MULTI_LDS_MAX"""
    out, n = [], 0
    for bi, branch in enumerate(roi_cases.BRANCHES):
        for refine in (False, True):
            for nb, shapes in ((4, NARROW), (2, NARROW + MID)):
                got = _pick(("c", "r") if refine else ("c",), shapes, C32, max_pcup_that_fits(nb), 64)
                picks = _with_length([(b, branch) for b in got], shapes, (1, 2, 3, 0)[n % 4], branch)
                out.append(Table("multi_nb%d_%s_br%d" % (nb, "refine" if refine else "cleanup", bi), 2, picks, 500 + n, nb, refine))
                n += 1
    one = blocks()[(31, 33), "dense", "c"]
    out.append(Table("multi_one_block", 2, [(one, roi_cases.BRANCHES[2])], 599, 4, False))
    return out


@functools.lru_cache(maxsize=None)
def route34_tables():
    """16-bit stores: reversible 5/3 with step 1, cleanup-only, M_b <= 15, at most 64 columns; k_ht_decode_pair (route 3)
    even widths, strides and offsets on top"""
    out = []
    for route, rem in ((3, 3), (4, 1)):
        shapes = [s for s in NARROW + MID if route == 4 or s[0] % 2 == 0]
        got = [b for b in _pick(("c",), shapes, C16) if b.M_b <= 15]
        out.append(Table("c16_route%d" % route, route, _with_length([(b, BR53) for b in got], shapes, rem, BR53), 600 + route))
        out.append(Table("c16_route%d_one_block" % route, route, [(blocks()[(32, 32), "top16", "c"], BR53)], 610 + route))
    return out


@functools.lru_cache(maxsize=None)
def route1_tables():
    """the jobs' column-per-lane route (and, run with route 0, the unit entry's fixed choice): every shape, class and pass
    count, the dequantisers in turn.  With a block wider than 64 columns k_ht_vlc, else k_ht_vlc2; two blocks per wave in
    the un-stuffing kernel, four where no block is wider than 32 columns"""
    out = []
    for name, shapes, rem in (("wide", NARROW + MID + WIDE, 2), ("mid", NARROW + MID, 3), ("narrow", NARROW, 1)):
        got = _pick(("c", "r"), shapes, C32 + ("top16",))
        picks = [(b, roi_cases.BRANCHES[k % 4]) for k, b in enumerate(got)]
        out.append(Table("column_" + name, 1, _with_length(picks, shapes, rem, BR53), 700 + len(out)))
    return out


@functools.lru_cache(maxsize=None)
def broken_tables():
    """the three rejected blocks between good ones, so that every wave of four and of two holds one or two of them beside
    blocks that decode -- and one wave of two holds only rejected ones"""
    E = broken_blocks()
    out = []
    for route, nb in ((2, 4), (2, 2), (3, 2), (4, 1)):
        shapes = [(2, 2), (32, 32), (16, 256), (2, 130), (32, 65)] + ([(64, 64), (34, 70), (40, 1)] if nb != 4 else [(4, 1024), (2, 130), (32, 32)])
        G = [blocks()[s, cls, "c"] for s, cls in zip(shapes, ("dense", "ones", "ones", "threes", "dense", "ones", "dense", "threes"))]
        order = [G[0], E[0], E[1], G[1], G[2], G[3], E[2], E[0], G[4], G[5], E[1], G[6], G[7], E[2]]
        out.append(Table("broken_route%d_nb%d" % (route, nb), route, [(b, BR53) for b in order], 800 + 10 * route + nb, nb, shuffle=False))
    return out


def all_tables():
    return route1_tables() + route2_tables() + route34_tables() + broken_tables()


# the tables' names, for a test to ask for one without building any while the tests are collected
NAMES_ROUTE1 = ["column_wide", "column_mid", "column_narrow"]
NAMES_ROUTE2 = ["multi_nb%d_%s_br%d" % (nb, rf, bi) for bi in range(4) for rf in ("cleanup", "refine") for nb in (4, 2)] + ["multi_one_block"]
NAMES_ROUTE34 = ["c16_route3", "c16_route3_one_block", "c16_route4", "c16_route4_one_block"]
NAMES_BROKEN = ["broken_route2_nb4", "broken_route2_nb2", "broken_route3_nb2", "broken_route4_nb1"]


# ---------------------------------------------------------------- the routes' conditions (the knob's table in the header)
def admits(route, entries, raw=False):
    """does the route take a table of these entries?  -> (yes, blocks per wave of the MagSgn kernel)"""
    B = [e.block for e in entries]
    if route in (0, 1):
        return True, 1
    refining = [b for b in B if b.npasses and b.coded > 1]
    max_p = max([b.pcup for b in B if b.npasses] + [0])
    if route == 2:
        if any(b.w > 64 for b in B) or len({e.branch[0] for e in entries}) != 1:
            return False, 0
        nb = 4 if max(b.w for b in B) <= 32 else 2
        if multi_lds(nb, max_p) > MULTI_LDS_MAX:
            return False, 0
        if refining and (max(b.h for b in refining) > 64 or
                         multi_refine_lds(nb, max(b.lref for b in B if b.npasses), max(b.h for b in refining)) > 24 * 1024):
            return False, 0
        return True, nb
    ok = not raw and all(b.w <= 64 and b.M_b <= 15 and e.branch[0] == 1 and e.branch[2] == 32768 for b, e in zip(B, entries))
    ok = ok and not refining
    if route == 3:
        ok = ok and all(b.w % 2 == 0 and e.stride % 2 == 0 and e.plane_off % 2 == 0 for b, e in zip(B, entries))
    return ok, (2 if route == 3 else 1)
