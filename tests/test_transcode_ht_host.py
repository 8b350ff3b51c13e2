"""CPU checks of HT and MIXED sources in the transcoder (htj2k_transcode_opts.ht_sources; no GPU): the interface, the
context-free check and the smallest stream, the block rule for HT descriptors pinned with the reference's HT block
decoder, and a stream whose passes run below plane 0."""
import ctypes

import numpy as np
import pytest

import cs_rewrite
import ffmpeg_ht_amd as m
import oracle
import vecgen
import xc_ht_model as xh
import xc_model as xm
from test_transcode_rc_host import empty_stream

PATCHWELCOME, INVALIDDATA, EINVAL = -0x45574150, -0x41444E49, -22


# ---------------------------------------------------------------- 1. the interface
def test_symbols_and_defaults():
    L = m.load_library()
    for name in ("htj2k_ht_blocks_raw", "htj2k_transcode_check_opts"):
        assert hasattr(L, name) and name in m.EXPORTS, name
    o = m.TranscodeOptsHt(77, 5)
    assert ctypes.sizeof(o) == 16
    L.htj2k_transcode_opts_default(ctypes.byref(o))
    assert (o.target_bytes, o.ht_sources) == (0, 0)
    # the view callers declared before the field existed: still 8 bytes, and the whole struct fits behind it
    old = m.TranscodeOpts(77)
    L.htj2k_transcode_opts_default(ctypes.byref(old))
    assert old.target_bytes == 0 and ctypes.sizeof(old) == 8 and ctypes.sizeof(m.TranscodeOpts) == 8
    assert m.TranscodeOpts(12).target_bytes == 12
    for f in ("transcode", "transcode_into", "transcode_check", "transcode_min_size"):
        assert "ht_sources" in getattr(m.Encoder, f).__code__.co_varnames, f


def test_ht_sources_is_0_or_1():
    src = vecgen.encode(vecgen.synth_image(33, 17, 1, seed=1), nlevels=2, cb=(2, 2))
    for f in (m.Encoder.transcode_check, m.Encoder.transcode_min_size):
        for bad in (2, -1):
            with pytest.raises(m.Htj2kError) as e:
                f(src, ht_sources=bad)
            assert e.value.code == EINVAL and "ht_sources" in str(e.value)
    # the C entry with opts == NULL is the old one
    L = m.load_library()
    buf, size = m.packet(src)
    bound, least = ctypes.c_size_t(), ctypes.c_int64()
    assert L.htj2k_transcode_check_opts(buf, size, None, ctypes.byref(bound), ctypes.byref(least), None, None) == PATCHWELCOME
    assert (bound.value, least.value) == (0, 0)
    o = m.TranscodeOptsHt(0, 1)
    assert L.htj2k_transcode_check_opts(buf, size, ctypes.byref(o), ctypes.byref(bound), ctypes.byref(least), None, None) == 0
    assert bound.value == m.Encoder.transcode_check(src, ht_sources=True) > least.value > 0
    assert least.value == m.Encoder.transcode_min_size(src, ht_sources=True)


# ---------------------------------------------------------------- 2. check and min size
SOURCES = {
    "gray_33x17": (lambda: vecgen.synth_image(33, 17, 1, seed=1), dict(nlevels=2, cb=(2, 2), transform=1)),
    "rgb_64x48_97_3p": (lambda: vecgen.synth_image(64, 48, 3, seed=2), dict(mct=1, nlevels=3, cb=(4, 4), transform=0, qstep=1 / 8, passes=3)),
    "rgb_70x50_tiles": (lambda: vecgen.synth_image(70, 50, 3, seed=5), dict(mct=1, nlevels=2, cb=(3, 3), tile=(32, 32))),
}


@pytest.mark.parametrize("mixed", [False, True], ids=["ht", "mixed"])
@pytest.mark.parametrize("name", sorted(SOURCES))
def test_check_and_min_size(name, mixed):
    img, kw = SOURCES[name]
    comps = img()
    src = vecgen.encode(comps, mixed=mixed, **kw)
    bound = m.Encoder.transcode_check(src, ht_sources=True)
    least = m.Encoder.transcode_min_size(src, ht_sources=True)
    want = empty_stream(src, kw, "gray" if len(comps) == 1 else "rgb24", comps[0].shape[1], comps[0].shape[0])
    assert least == len(want) and 0 < least < bound
    # without the keyword: refused as before, by both entries and with the same line
    lines = []
    for f in (m.Encoder.transcode_check, m.Encoder.transcode_min_size):
        with pytest.raises(m.Htj2kError) as e:
            f(src)
        assert e.value.code == PATCHWELCOME and "HT code-blocks already" in str(e.value)
        lines.append(str(e.value).split(": ", 1)[1])
    assert lines[0] == lines[1]


@pytest.mark.parametrize("mixed", [False, True], ids=["ht", "mixed"])
def test_the_rest_of_the_list_is_still_refused(mixed):
    img = vecgen.synth_image(70, 50, 3, seed=2)
    for kw in (dict(roi_shift=12), dict(offset=(3, 1)), dict(sgnd=True), dict(prec=[(4, 4)], cb=(6, 6))):
        cs = vecgen.encode(img, mixed=mixed, nlevels=3, mct=1, **kw)
        with pytest.raises(m.Htj2kError) as e:
            m.Encoder.transcode_check(cs, ht_sources=True)
        assert e.value.code == PATCHWELCOME and "transcode:" in str(e.value) and "HT code-blocks" not in str(e.value), kw


def test_part1_sources_do_not_care():
    src = vecgen.encode(vecgen.synth_image(33, 17, 1, seed=1), part1=True, nlevels=2, cb=(2, 2))
    assert m.Encoder.transcode_check(src, ht_sources=True) == m.Encoder.transcode_check(src)
    assert m.Encoder.transcode_min_size(src, ht_sources=True) == m.Encoder.transcode_min_size(src)


# ---------------------------------------------------------------- 3. the block rule on the reference's HT block decoder
SHAPES = [(1, 1), (3, 5), (4, 4), (17, 9), (64, 64)]


def ht_source_block(vals, passes, causal, extra_bits=0):
    """the factory's HT block of these values -> (words of ff_jpeg2000_decode_htj2k, M_b, zbp)"""
    h, w = vals.shape
    data, lcup, lref, mu = vecgen.encode_block(vals, passes=passes, causal=causal)
    p = 1 if passes > 1 else 0
    M_b = max(mu + p, 1) + 1 + extra_bits
    zbp = M_b - 1 - p - extra_bits                         # extra_bits: the same block in a band with more magnitude bits, pc higher
    r, words = oracle.ht_decode_block(data, lcup, lref, passes, zbp, w, h, M_b, vsc=causal)
    assert r == 1
    return words, M_b, zbp


def check_block(vals, passes, causal, extra_bits=0):
    """-> what became of the block: None (left out) or (plane, passes, fell back)"""
    h, w = vals.shape
    words, M_b, zbp = ht_source_block(vals, passes, causal, extra_bits)
    assert xh.rule(M_b, zbp, passes) == (extra_bits, passes)
    idx = xh.raw_index(words, M_b, zbp, passes)
    form = xh.ht_form(idx, M_b, zbp, passes)
    if form is None:
        assert not words.any()
        return None
    p, k = form
    # the indices have the form (p, k): nothing below the plane of the last pass
    assert not np.any(np.abs(idx.astype(np.int64)) & ((1 << p) - 1))
    data, lcup, lref, mu = vecgen.encode_block(xm.shifted(idx, p), passes=k)          # non-causal, whatever the source was
    cp = p + (k > 1)
    assert mu + cp <= M_b
    r, got = oracle.ht_decode_block(data, lcup, lref, k, M_b - 1 - cp, w, h, M_b)
    assert r == 1 and np.array_equal(got, words), (w, h, passes, causal, extra_bits)
    return p, k, k != passes


@pytest.mark.parametrize("causal", [False, True], ids=["plain", "vsc"])
def test_block_rule(causal):
    """ff_jpeg2000_decode_htj2k's words of an HT block of 1, 2 or 3 passes, vertically causal or not, equal, sample for
    sample, its words of the non-causal HT block the rule makes of the block's indices: at pr = 0 and higher, on both
    fall-backs, and with an all-zero block left out"""
    rng = np.random.default_rng(900 + causal)
    kept, fell = set(), 0
    for (w, h) in SHAPES:
        for passes in (1, 2, 3):
            for amp, density in ((3, 0.3), (200, 0.9), (40, 0.05)):
                for extra in (0, 2):
                    vals = rng.integers(-amp, amp + 1, (h, w)) * (rng.random((h, w)) < density)
                    vals[0, 0] = amp
                    f = check_block(vals, passes, causal, extra)
                    assert f is not None and f[0] == extra + (f[2] and passes > 1)
                    kept.add(f[1])
                    fell += f[2]
            # every sample significant at pc: SigProp has nothing to write -> one cleanup pass at pc; MagRef still has
            dense = rng.integers(2, 60, (h, w)) * rng.choice([-1, 1], (h, w))
            f = check_block(dense, passes, causal)
            assert f == ((0, 1, False) if passes == 1 else (1, 1, True) if passes == 2 else (0, 3, False))
            # nothing significant at pc: with one pass that is a block of +-1, with more the cleanup pass codes nothing and
            # SigProp has no neighbour to start from -- the block decodes to zeros and is left out
            ones = rng.integers(-1, 2, (h, w))
            ones[0, 0] = 1
            f = check_block(ones, passes, causal)
            assert f == ((0, 1, False) if passes == 1 else None)
            # all zero
            assert check_block(np.zeros((h, w), np.int64), passes, causal) is None
    assert kept == {1, 2, 3} and fell > 0


def test_rule_arithmetic():
    """placeholder sets count as zero bit-planes; the passes that remain are 1 .. 3"""
    assert xh.rule(10, 3, 0) == (-1, 1)
    assert [xh.rule(10, 3, n) for n in (1, 2, 3)] == [(6, 1), (5, 2), (5, 3)]
    assert [xh.rule(10, 3, n) for n in (4, 5, 6)] == [(5, 1), (4, 2), (4, 3)]           # one placeholder set
    assert [xh.rule(10, 3, n) for n in (7, 8, 9)] == [(4, 1), (3, 2), (3, 3)]
    assert xh.rule(10, 9, 1) == (0, 1) and xh.rule(10, 9, 2) is None and xh.rule(10, 8, 4) == (0, 1) and xh.rule(10, 8, 5) is None


# ---------------------------------------------------------------- 4. passes below plane 0
@pytest.mark.parametrize("kw", [dict(), dict(passes=3), dict(placeholder_sets=1)], ids=["1p", "3p", "placeholder"])
def test_check_refuses_passes_below_plane_0(orc, kw):
    """every exponent of QCD lowered by one (tests/cs_rewrite.py): the blocks keep their zero bit-planes and their passes
    and their bands lose a magnitude bit, so the blocks that ended on plane 0 end below it.  The parsers accept the
    stream, the rule does not"""
    src = vecgen.encode(vecgen.synth_image(33, 17, 1, seed=1), nlevels=1, cb=(3, 3), sop=True, eph=True, **kw)
    s = cs_rewrite.Stream(src)
    for i, (code, p) in enumerate(s.main):
        if code == cs_rewrite.QCD:
            s.main[i] = (code, bytes([p[0]]) + bytes(x - 8 for x in p[1:]))
    bad = s.build()
    rules = lambda cs: [xh.rule(int(e["M_b"]), int(e["zbp"]), int(e["npasses"])) for e in orc.plan_blocks(cs)]
    assert None not in rules(src) and any(r is not None and r[0] == 0 for r in rules(src))
    assert None in rules(bad)
    assert m.Encoder.transcode_check(src, ht_sources=True) > 0
    with pytest.raises(m.Htj2kError) as e:
        m.Encoder.transcode_check(bad, ht_sources=True)
    assert e.value.code == INVALIDDATA and "passes over" in str(e.value)
