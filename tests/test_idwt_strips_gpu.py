"""Strip seams of the register-streaming inverse DWT (csrc/dwt_stream.hpp) on small pictures and dirty buffers.

Whether the streaming kernels are right depends on launch geometry: the columns a wave owns (stream_strip_cols: 244, or
224 on long rows), the rows of a strip (stream_strip_rows: 8 or 16), the waves of a workgroup (stream_wpb: min(8, strips
of a row)) and the XCD order in which stream_strip() deals the strips out.  At the defaults a picture has to be
thousands of columns wide to have several strips in a row; the per-launch knobs HTJ2K_TW16 / HTJ2K_TW32 / HTJ2K_TWF,
HTJ2K_STRIP and HTJ2K_WPB put every one of those seams on pictures some 200 columns wide: three and more column strips,
a last strip of 4 or 8 columns, a mirror lane in a strip's first lanes, strips of a workgroup that straddle two rows of
strips (gx % wpb != 0), strips of the grid that lie beyond a narrower plane of the same launch.

Everything is compared bit for bit: frames with the oracle's (and 8-bit lossless RGB with the source picture), planes
with oracle.idwt.

Dirty-buffer rule.  A strip that writes nothing, or skips a column range, leaves in its output whatever the allocator
handed out -- and a hipMalloc after a hipFree of the same size commonly returns the same memory.  So no checked run here
may start on buffers that can hold its own answer:
  * job level: every case has two pictures A and B of one geometry (different seeds, more than half of the samples
    differ -- test_case_geometry); consecutive configurations of a case decode the batch [A, B], then [B, A], ...;
  * plane level (dec.idwt): before each checked call the same call -- geometry, mode, knobs -- runs on other random
    content (the result of which is checked as well);
  * one pass of everything runs in a child process under HTJ2K_POISON=1 (fresh device buffers are 0xA5 bytes).

The path a configuration is meant to take is asserted wherever the ABI can tell (16-bit sub-bands, 16-bit LL bands,
packed arithmetic, the number of IDWT launches): a case that no longer qualifies fails instead of passing by another
route.  Run as a program, the module runs its sweeps on its own decoder (the poison pass)."""
import contextlib
import itertools
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.dirname(HERE)]

import oracle
import vecgen

# ------------------------------------------------------------------ the launch knobs
TW_KNOBS = ("HTJ2K_TW16", "HTJ2K_TW32", "HTJ2K_TWF")
ENV_KNOBS = TW_KNOBS + ("HTJ2K_STRIP", "HTJ2K_WPB", "HTJ2K_X3_TH")
INT_DEFAULTS = dict(idwt_mode=3, bitexact=0, coef16=1, ll16=1, idwt_pk=1, idwt_x3=1, idwt_x2=2, idwt_x2_th=20)


@contextlib.contextmanager
def knobs(dec, tw=None, strip=None, wpb=None, x3_th=None, **ints):
    """the launch geometry of the runs inside: strip width (all three of HTJ2K_TW16 / TW32 / TWF: whichever a launch
    reads), HTJ2K_STRIP, HTJ2K_WPB, HTJ2K_X3_TH (None: unset, the default) and set_int knobs.  The variables are read per
    launch: they are gone, and every set_int knob is back at its default, when the block ends"""
    assert not set(ints) - set(INT_DEFAULTS), ints
    env = dict.fromkeys(TW_KNOBS, tw)
    env.update(HTJ2K_STRIP=strip, HTJ2K_WPB=wpb, HTJ2K_X3_TH=x3_th)
    try:
        for k, v in env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)
        for k, v in ints.items():
            dec.set_int(k, v)
        yield
    finally:
        for k in ENV_KNOBS:
            os.environ.pop(k, None)
        for k in ints:
            dec.set_int(k, INT_DEFAULTS[k])


def thin(axes, n, label, ok=None):
    """a fixed subset of the cross product of `axes` (those that `ok` admits): shuffled with a seed made of `label`,
    then taken greedily until every value of every axis has appeared, then filled up to n in the shuffled order"""
    full = [c for c in itertools.product(*axes) if ok is None or ok(c)]
    np.random.default_rng(zlib.crc32(label.encode())).shuffle(full)
    need = {(i, v) for c in full for i, v in enumerate(c)}
    gain = lambda c: len(need.intersection(enumerate(c)))
    chosen = []
    while need:                                             # of the first 256, the first that brings the most values not yet seen
        best = max(full[:256], key=gain)
        if not gain(best):
            best = next(c for c in full if gain(c))
        chosen.append(best)
        need.difference_update(enumerate(best))
    assert len(chosen) <= n, (label, len(chosen))
    return chosen + list(itertools.islice((c for c in full if c not in chosen), n - len(chosen)))


# ------------------------------------------------------------------ geometry, as htj2k_device.hip decides it
def levels(w, h, nl, x0=0, y0=0):
    """(lh, lv, mh, mv) of the IDWT levels of a w x h plane whose origin is (x0, y0), final level first"""
    bx, by, out = [x0, x0 + w], [y0, y0 + h], []
    for _ in range(nl):
        out.append((bx[1] - bx[0], by[1] - by[0], bx[0] & 1, by[0] & 1))
        bx, by = [(v + 1) >> 1 for v in bx], [(v + 1) >> 1 for v in by]
    return out


def fast_geometry(lh, lv, mh, mv=0):
    return mh % 2 == 0 and lh % 4 == 0 and lh >= 8 and lv >= 2


def strips(n, t):
    """the pieces a line of n samples falls into when a strip takes t"""
    return [min(t, n - i) for i in range(0, n, t)]


TWS = (64, 68, 100, 224, 244)              # 100: no multiple of 64; 224 and 244: the defaults
STRIPS = (8, 10, 16)
WPBS = (1, 2, 3, 8, None)                  # None: unset, min(8, strips of a row)
PER_SWEEP = 24                             # configurations of one job-level sweep (one case on one path)

_420 = dict(dx=[1, 2, 2], dy=[1, 2, 2])
_97 = dict(mct=1, transform=0, qstep=1)
# name: (w, h, components, levels, encode arguments, picture arguments, every level of fast geometry, compare with the source)
CASES = {
    "rgb_2l":     (272, 37, 3, 2, dict(mct=1), {}, True, True),
    "rgb_3l":     (208, 37, 3, 3, dict(mct=1), {}, True, True),
    "rgb_nomct":  (208, 37, 3, 3, {}, {}, True, True),
    "gray":       (272, 37, 1, 2, {}, {}, True, False),
    "yuv420":     (544, 74, 3, 2, dict(width=544, height=74, **_420), _420, True, False),
    "rgb10":      (208, 37, 3, 3, dict(mct=1, depth=10), dict(depth=10), True, False),
    "gray12":     (272, 37, 1, 2, dict(depth=12), dict(depth=12), True, False),
    "rgb97":      (208, 37, 3, 3, _97, {}, True, False),
    "rgb10_97":   (208, 37, 3, 3, dict(depth=10, **_97), dict(depth=10), True, False),
    "odd":        (203, 37, 3, 3, dict(mct=1), {}, False, True),
    "odd_off":    (201, 37, 3, 2, dict(mct=1, offset=(3, 5)), {}, False, True),
    "rgba":       (203, 37, 4, 2, {}, {}, False, False),
    "gray_odd97": (203, 37, 1, 3, dict(transform=0, qstep=1), {}, False, False),
    "x3_4l":      (544, 37, 3, 4, dict(mct=1), {}, True, True),
    "x3_wide":    (992, 37, 3, 4, dict(mct=1), {}, True, True),
    "x3_5l":      (1088, 70, 3, 5, dict(mct=1), {}, True, True),
}
# (lh, lv) of every level, final level first, worked out by hand from the table of the picture sizes
LEVELS = {
    "rgb_2l": [(272, 37), (136, 19)], "gray": [(272, 37), (136, 19)], "gray12": [(272, 37), (136, 19)],
    "rgb_3l": [(208, 37), (104, 19), (52, 10)], "rgb_nomct": [(208, 37), (104, 19), (52, 10)],
    "rgb10": [(208, 37), (104, 19), (52, 10)], "rgb97": [(208, 37), (104, 19), (52, 10)],
    "rgb10_97": [(208, 37), (104, 19), (52, 10)],
    "yuv420": [(544, 74), (272, 37)],                       # luma; the chroma planes: 272 x 37 and 136 x 19
    "odd": [(203, 37), (102, 19), (51, 10)], "gray_odd97": [(203, 37), (102, 19), (51, 10)],
    "odd_off": [(201, 37), (100, 18)],                      # columns [3, 204) -> [2, 102), rows [5, 42) -> [3, 21)
    "rgba": [(203, 37), (102, 19)],
    "x3_4l": [(544, 37), (272, 19), (136, 10), (68, 5)],
    "x3_wide": [(992, 37), (496, 19), (248, 10), (124, 5)],
    "x3_5l": [(1088, 70), (544, 35), (272, 18), (136, 9), (68, 5)],
}
# the seams the cases are named for: (case, level counted from the final one, strip width) -> widths of the strips
SEAMS = {
    ("rgb_2l", 0, 64): [64, 64, 64, 64, 16], ("rgb_2l", 0, 68): [68] * 4, ("rgb_2l", 0, 100): [100, 100, 72],
    ("rgb_2l", 0, 244): [244, 28], ("rgb_2l", 1, 64): [64, 64, 8],
    ("rgb_3l", 0, 64): [64, 64, 64, 16], ("rgb_3l", 0, 68): [68, 68, 68, 4], ("rgb_3l", 0, 100): [100, 100, 8],
    ("rgb_3l", 1, 100): [100, 4], ("rgb_3l", 1, 64): [64, 40],
    ("yuv420", 0, 64): [64] * 8 + [32], ("yuv420", 0, 244): [244, 244, 56], ("yuv420", 1, 64): [64, 64, 64, 64, 16],
    ("odd", 0, 64): [64, 64, 64, 11], ("odd_off", 0, 64): [64, 64, 64, 9], ("odd_off", 1, 68): [68, 32],
    ("x3_4l", 1, 244): [244, 28], ("x3_wide", 1, 244): [244, 244, 8], ("x3_wide", 2, 244): [244, 4],
    ("x3_5l", 2, 244): [244, 28], ("x3_5l", 0, 244): [244] * 4 + [112], ("x3_5l", 0, 224): [224] * 4 + [192],
}


def case_origin(name):
    return CASES[name][4].get("offset", (0, 0))


_pictures = {}


def pictures(orc, name, bitexact=0):
    """{"A": (source picture, codestream, oracle planes), "B": ...} of a case, made once and never changed"""
    key = (name, bitexact)
    if key not in _pictures:
        w, h, nc, nl, enc, pic, _, _ = CASES[name]
        out = {}
        for which, seed in (("A", 11), ("B", 23)):
            img = vecgen.synth_image(w, h, nc, seed=seed + 100 * sorted(CASES).index(name), noise=10, **pic)
            data = vecgen.encode(img, nlevels=nl, **enc)
            planes = orc.decode(data, bitexact=bitexact)[1]
            for p in planes:
                p.setflags(write=False)
            out[which] = (img, data, planes)
        _pictures[key] = out
    return _pictures[key]


# ------------------------------------------------------------------ job-level sweeps
def P(sub16, band16, packed, **ints):
    """a path: what the ABI must say of a job that took it (16-bit sub-bands, htj2k_job_ll16, packed arithmetic) and the
    set_int knobs that select it"""
    return dict(ints=ints, coef16=sub16, ll16=band16, packed=packed)


_INT32 = P(False, 0, False)
# (sweep id, cases of the batch, path, IDWT launches, HTJ2K_X3_TH).  idwt_x2 is 0 unless a sweep is about it: the
# launch counts below are one per level (and kind of final level), minus two where idwt_x3 folds levels 0-2 into one.
JOB_SWEEPS = [
    ("rgb_2l-pk",        ["rgb_2l"], P(True, 1, True, idwt_pk=1), 2, None),
    ("rgb_2l-nopk",      ["rgb_2l"], P(True, 1, False, idwt_pk=0), 2, None),
    ("rgb_3l-pk",        ["rgb_3l"], P(True, 1, True), 3, None),
    ("rgb_3l-nopk",      ["rgb_3l"], P(True, 1, False, idwt_pk=0), 3, None),
    ("rgb_3l-ll32",      ["rgb_3l"], P(True, 0, False, ll16=0), 3, None),          # k_idwt_stream<5/3, fast, C16>, fused level with a 32-bit LL band
    ("rgb_3l-coef32",    ["rgb_3l"], P(False, 0, False, coef16=0), 3, None),       # 32-bit sub-bands: k_idwt_stream<5/3, fast> and the rgb24 fast kernel
    ("rgb_nomct-pk",     ["rgb_nomct"], P(True, 1, True), 3, None),
    ("gray-pk",          ["gray"], P(True, 1, True), 2, None),
    ("gray-nopk",        ["gray"], P(True, 1, False, idwt_pk=0), 2, None),
    ("yuv420-pk",        ["yuv420"], P(True, 1, True), 2, None),
    ("yuv420-nopk",      ["yuv420"], P(True, 1, False, idwt_pk=0), 2, None),
    ("rgb10",            ["rgb10"], P(True, 1, False), 3, None),
    ("gray12",           ["gray12"], P(True, 1, False), 2, None),
    ("rgb97",            ["rgb97"], _INT32, 3, None),
    ("rgb97-bitexact",   ["rgb97"], P(False, 0, False, bitexact=1), 3, None),
    ("rgb10_97",         ["rgb10_97"], _INT32, 3, None),
    ("odd",              ["odd"], _INT32, 3, None),
    ("odd_off",          ["odd_off"], _INT32, 2, None),
    ("rgba",             ["rgba"], _INT32, 2, None),
    ("gray_odd97",       ["gray_odd97"], _INT32, 3, None),
    ("mixed-rgb",        ["rgb_2l", "rgb_3l"], P(True, 1, True), 4, None),          # level 1: a plain launch and a fused one
    ("mixed-planes",     ["gray", "yuv420"], P(True, 1, True), 2, None),            # planes of 544, 272 and 272 columns in one fused launch
]
for _name, _nl in (("x3_4l", 4), ("x3_wide", 4), ("x3_5l", 5)):
    JOB_SWEEPS.append(("%s-levels" % _name, [_name], P(True, 1, True, idwt_x3=0), _nl, None))
    for _th in (8, 12, 24):
        JOB_SWEEPS.append(("%s-x3-th%d" % (_name, _th), [_name], P(True, 1, True, idwt_x3=1), _nl - 2, _th))
JOB_CONFIGS = {s[0]: thin((TWS, STRIPS, WPBS), PER_SWEEP, s[0]) for s in JOB_SWEEPS}

# k_idwt_stream_pack_x2: LDS windows of wpb * tw / 2 + ... columns, so strips of 64 and two waves put a window seam at
# every 128th column.  x3_4l runs with idwt_x3 = 0: where x3 takes the level below the final one, x2 leaves it alone.
X2_SWEEPS = [(name, th) for name in ("rgb_2l", "rgb_3l", "x3_4l") for th in (4, 8, 20)]

_turn = {}


def run_job(dec, pkts):
    job = dec.job().parse_batch(pkts).upload().run().wait()
    try:
        frames = [job.download_frame(f)[1] for f in range(len(pkts))]
        st = dict(coef16=job.coef16(), ll16=job.ll16(), errors=job.block_errors(), packed=job.idwt_packed(),
                  launches=len(job.idwt_launches()))
    finally:
        job.free()
    return frames, st


def next_batch(orc, names, bitexact=0):
    """the next batch of these cases: [A, B] and [B, A] in turn (cases of a mixed batch: A of one with B of the other)"""
    key = tuple(names)
    _turn[key] = t = _turn.get(key, 0) ^ 1
    order = "AB" if t else "BA"
    if len(names) == 1:
        return [(names[0], pictures(orc, names[0], bitexact)[o]) for o in order]
    return [(n, pictures(orc, n, bitexact)[order[i & 1]]) for i, n in enumerate(names)]


def check_path(st, path, nlaunch, tag):
    assert st["errors"] == 0, (tag, st)
    assert st["coef16"] == path["coef16"] and st["ll16"] == path["ll16"], (tag, st)
    assert (10 <= st["packed"] <= 16) if path["packed"] else st["packed"] == 0, (tag, st)
    assert st["launches"] == nlaunch, (tag, st)


def check_frames(frames, batch, tag):
    for f, (planes, (name, (img, _, planes_o))) in enumerate(zip(frames, batch)):
        assert len(planes) == len(planes_o), (tag, f)
        for k, (a, d) in enumerate(zip(planes, planes_o)):
            assert a.dtype == d.dtype and np.array_equal(a, d), (tag, "frame %d (%s) plane %d" % (f, name, k))
        w, h = CASES[name][:2]
        if CASES[name][7]:
            assert np.array_equal(planes[0].reshape(h, w, 3), np.stack(img, -1)), (tag, "frame %d (%s) source" % (f, name))


def job_sweep(dec, orc, sweep):
    sid, names, path, nlaunch, x3_th = sweep
    ints = dict(idwt_x2=0, **path["ints"])
    for tw, strip, wpb in JOB_CONFIGS[sid]:
        batch = next_batch(orc, names, ints.get("bitexact", 0))
        with knobs(dec, tw=tw, strip=strip, wpb=wpb, x3_th=x3_th, **ints):
            frames, st = run_job(dec, [b[1][1] for b in batch])
        tag = (sid, "tw %s strip %s wpb %s" % (tw, strip, wpb))
        check_path(st, path, nlaunch, tag)
        check_frames(frames, batch, tag)


def x2_sweep(dec, orc, name, th):
    nl = CASES[name][3]
    n = {}
    for x2 in (0, 1, 1):                                    # the fused run twice: on [B, A] and on [A, B]
        batch = next_batch(orc, [name])
        with knobs(dec, tw=64, wpb=2, idwt_x2=x2, idwt_x2_th=th, idwt_x3=0):
            frames, st = run_job(dec, [b[1][1] for b in batch])
        check_path(st, P(True, 1, True), nl - x2, (name, "x2", x2, th))
        check_frames(frames, batch, (name, "x2", x2, th))
        n[x2] = st["launches"]
    assert n[1] == n[0] - 1, (name, th, n)


# ------------------------------------------------------------------ plane-level sweeps
X0S, Y0S, PLANE_LEVELS = (0, 2, 1, 3), (0, 1), (1, 2, 3)
WIDTHS4, WIDTHS_ODD = (128, 132, 136, 188, 192, 196, 260), (129, 130, 131, 191, 193)
HEIGHTS = (2, 3, 9, 16, 17, 25)
PLANE_TWS, PLANE_STRIPS, PLANE_WPBS = (64, 68, 244), (8, 16), (1, 3, 8)
PER_PLANE_SWEEP = 96
# transform: 1 5/3, 0 9/7 float, 2 9/7 fixed point; "53full": 5/3 on full-range int32 (the wrap-around of sr_1d53)
PLANE_KINDS = {"53": 1, "97": 0, "97int": 2, "53full": 1}


def _plane_is_fast(c):
    """k_idwt_stream<TYPE, true> at the final level: even origin, a width that is a multiple of 4 (every height here is >= 2)"""
    return c[0] % 2 == 0 and c[1] % 4 == 0


_PLANE_AXES = (X0S, WIDTHS4 + WIDTHS_ODD, HEIGHTS, Y0S, PLANE_LEVELS, PLANE_TWS, PLANE_STRIPS, PLANE_WPBS)
# the fast family takes the even origins and the widths that are multiples of 4, the general family every origin and
# width whose combination is not fast
PLANE_SWEEPS = [(kind, fam) for kind in PLANE_KINDS for fam in ("fast", "general")]
PLANE_CONFIGS = {
    (kind, fam): thin(_PLANE_AXES, PER_PLANE_SWEEP, "plane-%s-%s" % (kind, fam),
                      ok=_plane_is_fast if fam == "fast" else lambda c: not _plane_is_fast(c))
    for kind, fam in PLANE_SWEEPS}
N_CONFIGS = dict(job=sum(len(v) for v in JOB_CONFIGS.values()), x2=3 * len(X2_SWEEPS),
                 plane=2 * sum(len(v) for v in PLANE_CONFIGS.values()))


def plane_input(rng, kind, h, w):
    if kind == "97":
        return (rng.standard_normal((h, w)) * 300).astype(np.float32)
    if kind == "53full":
        return rng.integers(-2**31, 2**31 - 1, (h, w), dtype=np.int64).astype(np.int32)
    return rng.integers(-3000, 3000, (h, w)).astype(np.int32) * (256 if kind == "97int" else 1)


def plane_sweep(dec, kind, fam):
    typ = PLANE_KINDS[kind]
    rng = np.random.default_rng(zlib.crc32(("%s-%s" % (kind, fam)).encode()))
    for cfg in PLANE_CONFIGS[(kind, fam)]:
        x0, w, h, y0, lev, tw, strip, wpb = cfg
        border = [[x0, x0 + w], [y0, y0 + h]]
        with knobs(dec, tw=tw, strip=strip, wpb=wpb, idwt_mode=3):
            for role in ("decoy", "checked"):               # the same call on other content first
                p = plane_input(rng, kind, h, w)
                want = oracle.idwt(p, border, lev, typ)
                got = dec.idwt(p, border, lev, typ)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, fam, cfg, role)


# ------------------------------------------------------------------ the tests
def test_case_geometry(orc):
    for name, (w, h, nc, nl, enc, pic, fast, src) in CASES.items():
        x0, y0 = case_origin(name)
        lev = levels(w, h, nl, x0, y0)
        assert [l[:2] for l in lev] == LEVELS[name], name
        assert all(fast_geometry(*l) for l in lev) == fast, name
        if fast:
            assert (x0, y0) == (0, 0)
        else:
            assert not fast_geometry(*lev[0]), name                        # the fused final level is a general kernel
        pa, pb = pictures(orc, name)["A"], pictures(orc, name)["B"]
        info = orc.decode(pa[1])[0]
        assert (info.width, info.height) == (w, h), name
        a, b = (np.concatenate([p.ravel() for p in x[2]]) for x in (pa, pb))
        assert a.shape == b.shape and np.count_nonzero(a != b) > a.size // 2, name
        if src:
            for img, _, planes in (pa, pb):
                assert np.array_equal(planes[0].reshape(h, w, 3), np.stack(img, -1)), name
        # at least three column strips at the narrowest strip, and rows: at least three strips, the last one short
        assert len(strips(w, 64)) >= 3, name
        for th in STRIPS:
            rows = strips(h, th)
            assert len(rows) >= 3 and (rows[-1] < th or (h, th) == (70, 10)), (name, th)
    for (name, k, tw), want in SEAMS.items():
        assert strips(LEVELS[name][k][0], tw) == want, (name, k, tw)
    assert [w % 4 for w in (203, 201)] == [3, 1]
    # strips of a workgroup that straddle two rows of strips: 4 and 5 strips a row with 3 waves, 5 and 9 with 2 and
    # with the default min(8, gx); a last strip of 4 and of 8 columns; strips beyond the chroma planes of 4:2:0
    assert 4 % 3 and 5 % 3 and 5 % 2 and 9 % 2 and 9 % min(8, 9)
    assert {v[-1] for v in SEAMS.values()} >= {4, 8}
    assert len(SEAMS[("yuv420", 0, 64)]) - len(strips(272, 64)) >= 3 and len(SEAMS[("yuv420", 0, 244)]) - len(strips(272, 244)) >= 1
    assert len(strips(136, 64)) - len(strips(52, 64)) >= 2                 # mixed-rgb, level 0: 136 and 52 columns under one grid
    # the x2 windows: strips of 64 columns, two waves: a workgroup every 128 columns, three of them on the narrowest case
    assert all(len(strips(CASES[n][0], 2 * 64)) >= 2 for n, _ in X2_SWEEPS) and len(strips(544, 128)) >= 3
    # every sweep holds every value of every knob
    for sid, cfgs in JOB_CONFIGS.items():
        assert [set(c) for c in zip(*cfgs)] == [set(TWS), set(STRIPS), set(WPBS)], sid
        assert len(cfgs) == PER_SWEEP, sid
    for (kind, fam), cfgs in PLANE_CONFIGS.items():
        got = [set(c) for c in zip(*cfgs)]
        want = [set(a) for a in _PLANE_AXES]
        if fam == "fast":
            want[0], want[1] = {0, 2}, set(WIDTHS4)
        assert got == want and len(cfgs) == PER_PLANE_SWEEP, (kind, fam)
        assert all(fast_geometry(c[1], c[2], c[0] & 1) == (fam == "fast") for c in cfgs)
    # configurations run (jobs of two frames / x2 jobs / dec.idwt calls, the decoys included)
    assert N_CONFIGS == dict(job=34 * 24, x2=27, plane=2 * 8 * 96)


def test_knobs_do_not_leak():
    class Rec:
        def __init__(self): self.calls = []
        def set_int(self, k, v): self.calls.append((k, v))
    rec = Rec()
    os.environ["HTJ2K_WPB"] = "5"
    with pytest.raises(ZeroDivisionError):
        with knobs(rec, tw=64, strip=10, idwt_pk=0, idwt_x2=1):
            assert [os.environ.get(k) for k in ENV_KNOBS] == ["64", "64", "64", "10", None, None]
            1 / 0
    assert not [k for k in ENV_KNOBS if k in os.environ]
    assert rec.calls == [("idwt_pk", 0), ("idwt_x2", 1), ("idwt_pk", 1), ("idwt_x2", 2)]


@pytest.fixture(scope="module")
def dec():
    import ffmpeg_ht_amd as m
    d = m.Decoder()
    assert d.device_name().startswith("gfx950"), d.device_name()
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sweep", JOB_SWEEPS, ids=[s[0] for s in JOB_SWEEPS])
def test_job_strips(dec, orc, sweep):
    """one case on one path: PER_SWEEP jobs of two frames over strip widths, strip heights and waves per workgroup"""
    job_sweep(dec, orc, sweep)


@pytest.mark.gpu
@pytest.mark.parametrize("name,th", X2_SWEEPS)
def test_x2_window_seams(dec, orc, name, th):
    """k_idwt_stream_pack_x2 at strips of 64 columns, two waves per workgroup and idwt_x2_th rows per band: the frames
    of the two-launch run, one launch fewer"""
    x2_sweep(dec, orc, name, th)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,fam", PLANE_SWEEPS)
def test_plane_strips(dec, kind, fam):
    """dec.idwt against oracle.idwt in idwt_mode 3 over origins, widths, heights, levels and the launch knobs"""
    plane_sweep(dec, kind, fam)


def run_everything(dec, orc):
    """every sweep of this module once (the poison pass: this module as a program)"""
    for sweep in JOB_SWEEPS:
        job_sweep(dec, orc, sweep)
    for name, th in X2_SWEEPS:
        x2_sweep(dec, orc, name, th)
    for kind, fam in PLANE_SWEEPS:
        plane_sweep(dec, kind, fam)


# Measured on an MI355X: this module as a program, all sweeps, takes 4.9 s without HTJ2K_POISON (4.3 s of it the sweeps)
# and 5.2 s with it; the poison fill waits for the device at every allocation, so the child gets five times the former.
POISON_TIMEOUT = 25


@pytest.mark.gpu
def test_everything_on_poisoned_buffers():
    """HTJ2K_POISON=1 (read once per process, so a child): every fresh device buffer starts as 0xA5 bytes, and all the
    sweeps above must still give the oracle's results"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=POISON_TIMEOUT,
                       env=dict(os.environ, HTJ2K_POISON="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "poisoned buffers: ok" in r.stdout, r.stdout[-3000:]


if __name__ == "__main__":
    import ffmpeg_ht_amd as m
    t0 = time.time()
    _dec, _orc = m.Decoder(), oracle.OracleDecoder()
    run_everything(_dec, _orc)
    _dec.close()
    _orc.close()
    print("%s buffers: ok, %.1f s" % ("poisoned" if os.environ.get("HTJ2K_POISON") == "1" else "plain", time.time() - t0))
