"""CPU checks of the transcoder (no GPU): the block rule it rests on, pinned with the reference's two block decoders;
htj2k_transcode_check on every kind of stream in and out of scope; the host writer given a source's quantisation."""
import ctypes

import numpy as np
import pytest

import cs_rewrite
import ffmpeg_ht_amd as m
import oracle
import vecgen
import xc_model as xm

PATCHWELCOME = -0x45574150

SHAPES = [(1, 1), (3, 5), (4, 4), (17, 9), (64, 64)]
STYLES = [0, 0x01, 0x04, 0x08]                           # none, BYPASS, TERMALL, VSC


def p1_block(rng, w, h, band, style, d, amp, density):
    """a random block through the factory's EBCOT coder with its last d passes dropped -> (words of decode_cblk, K, n, M_b)"""
    vals = rng.integers(-amp, amp + 1, (h, w)) * (rng.random((h, w)) < density)
    vals[0, 0] = amp                                      # never all zero
    seg, lens, passes, K, n = vecgen.encode_block_p1(vals, band=band, style=style, drop_passes=d)
    M_b = K + 1                                           # the least headroom an HT block needs
    data, length, starts = oracle.mq_block_layout(seg, lens, passes, style)
    ret, t1 = oracle.mq_decode_block(data, length, n, K, w, h, M_b, style, band, starts)
    assert ret == 1
    return t1, K, n, M_b


@pytest.mark.parametrize("style", STYLES)
def test_block_rule(style):
    """decode_cblk's words of a Part-1 block cut after any pass equal, sample for sample, ff_jpeg2000_decode_htj2k's words
    of the HT block the rule makes of its indices: d runs over more than two whole planes, so the block ends on a
    cleanup, a SigProp and a MagRef pass (r = 0, 1, 2) several times, and on both fall-backs"""
    rng = np.random.default_rng(700 + style)
    seen, fell = set(), 0
    for (w, h) in SHAPES:
        for band in range(4):
            for d in range(8):
                for amp, density in ((3, 0.3), (200, 0.9), (40, 0.05)):
                    t1, K, n, M_b = p1_block(rng, w, h, band, style, d, amp, density)
                    if n == 0:
                        continue
                    idx = xm.raw_index(t1, M_b, K, n)
                    form = xm.ht_form(idx, K, n)
                    seen.add((n - 1) % 3)
                    if form is None:
                        assert not t1.any()
                        continue
                    p, passes = form
                    fell += passes == 1 and (n - 1) % 3 != 0
                    data, lcup, lref, mu = vecgen.encode_block(xm.shifted(idx, p), passes=passes)
                    cp = p + (passes > 1)
                    assert mu + cp <= M_b                 # K < M_b is headroom enough
                    r, got = oracle.ht_decode_block(data, lcup, lref, passes, M_b - 1 - cp, w, h, M_b)
                    assert r == 1 and np.array_equal(got, t1), (w, h, band, style, d, K, n)
    assert seen == {0, 1, 2} and fell > 0


def test_block_rule_needs_one_bit_of_headroom():
    """with K = M_b (a block that uses every magnitude bit of its band) the HT block the rule makes needs U + pc = M_b + 1:
    the reference's HT block decoder rejects every one of them, whatever pass the source ends on.  Such sources are
    refused (test_check_refuses_a_block_without_headroom), not approximated"""
    rng = np.random.default_rng(9)
    n_rejected = 0
    for d in range(7):
        for (w, h) in ((16, 16), (3, 5)):
            vals = rng.integers(-255, 256, (h, w))
            vals[0, 0] = 255
            seg, lens, passes, K, n = vecgen.encode_block_p1(vals, band=0, style=0, drop_passes=d)
            M_b = K
            data, length, starts = oracle.mq_block_layout(seg, lens, passes, 0)
            ret, t1 = oracle.mq_decode_block(data, length, n, K, w, h, M_b, 0, 0, starts)
            assert ret == 1
            idx = xm.raw_index(t1, M_b, K, n)
            p, k = xm.ht_form(idx, K, n)
            hd, lcup, lref, mu = vecgen.encode_block(xm.shifted(idx, p), passes=k)
            cp = p + (k > 1)
            assert mu + cp == M_b + 1
            r, got = oracle.ht_decode_block(hd, lcup, lref, k, M_b - 1 - cp, w, h, M_b)
            assert r < 0 and not got.any()
            n_rejected += 1
    assert n_rejected == 14


IMG = vecgen.synth_image(70, 50, 3, seed=2)
BASE = dict(part1=True, nlevels=3, mct=1)

ACCEPTED = ([dict(prog=p) for p in range(5)] + [dict(sop=True, eph=True), dict(prec=[(7, 7)]), dict(tile=(32, 32))] +
            [dict(cblk_style=s) for s in (0x01, 0x04, 0x08, 0x3F)] +
            [dict(drop_passes=d, transform=0, qstep=1 / 8) for d in range(6)])


@pytest.mark.parametrize("kw", ACCEPTED, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_check_accepts(kw):
    cs = vecgen.encode(IMG, **dict(BASE, **kw))
    bound = m.Encoder.transcode_check(cs)
    tile = kw.get("tile", (0, 0))
    assert bound >= m.Encoder.bound(70, 50, "rgb24", 8, levels=3, mct=1, tile=tile, ht_passes=3,
                                    irreversible="qstep" in kw, qstep=kw.get("qstep", 1.0)) > len(cs) // 4
    assert m.Encoder.transcode_check(vecgen.jp2_wrap(cs, 70, 50, 3, 8, colourspace=16)) == bound


# roi_shift: the issue names 3, which the factory refuses for 8-bit pictures (tests/test_roi_streams.py); 12 is a Maxshift stream
REFUSED = [("ht", dict(part1=False)), ("mixed", dict(part1=False, mixed=True)), ("roi", dict(roi_shift=12)),
           ("comp_levels", dict(comp=[None, {"nlevels": 2}, None], mct=0)), ("origin", dict(offset=(3, 1))),
           ("signed", dict(sgnd=True)), ("partition", dict(prec=[(4, 4)], cb=(6, 6)))]


@pytest.mark.parametrize("name,kw", REFUSED, ids=[n for n, _ in REFUSED])
def test_check_refuses(name, kw):
    cs = vecgen.encode(IMG, **dict(BASE, **kw))
    with pytest.raises(m.Htj2kError) as e:
        m.Encoder.transcode_check(cs)
    assert e.value.code == PATCHWELCOME and "transcode:" in str(e.value), str(e.value)


def test_check_refuses_a_block_without_headroom(orc):
    """one guard bit and a sample at the end of the range: the LL block has K = M_b coded planes"""
    img = [np.zeros((16, 16), np.int32)]
    img[0][3:9, 2:11] = 255
    cs = vecgen.encode(img, part1=True, nlevels=0, guard_bits=1, cb=(4, 4))
    assert [(int(e["zbp"]), int(e["M_b"])) for e in orc.plan_blocks(cs)] == [(8, 8)]
    with pytest.raises(m.Htj2kError) as e:
        m.Encoder.transcode_check(cs)
    assert e.value.code == PATCHWELCOME and "one more guard bit" in str(e.value)
    # the same picture with two guard bits is in scope
    assert m.Encoder.transcode_check(vecgen.encode(img, part1=True, nlevels=0, guard_bits=2, cb=(4, 4))) > 0


def test_check_refuses_more_passes_than_planes(orc):
    """every exponent of QCD lowered by three (tests/cs_rewrite.py): the blocks keep their passes and lose three
    bit-planes, so passes run below plane 0; the parsers accept the stream, the rule does not"""
    src = vecgen.encode(vecgen.synth_image(33, 17, 1, seed=1), part1=True, nlevels=1, cb=(3, 3), sop=True, eph=True)
    s = cs_rewrite.Stream(src)
    for i, (code, p) in enumerate(s.main):
        if code == cs_rewrite.QCD:
            s.main[i] = (code, bytes([p[0]]) + bytes(x - 8 * 3 for x in p[1:]))
    bad = s.build()
    tab = orc.plan_blocks(bad)
    assert any(int(e["npasses"]) > 3 * int(e["zbp"]) - 2 for e in tab if e["flags"] & 4)
    assert m.Encoder.transcode_check(src) > 0
    with pytest.raises(m.Htj2kError) as e:
        m.Encoder.transcode_check(bad)
    assert e.value.code == -0x41444E49 and "passes over" in str(e.value)


def test_check_refuses_garbage():
    with pytest.raises(m.Htj2kError) as e:
        m.Encoder.transcode_check(b"\xff\x4f\xff\x51" + b"\0" * 40)
    assert e.value.code == -0x41444E49                    # HTJ2K_ERR_INVALIDDATA, from the parser


def product_plan_blocks(data):
    """the product parser's block table (libhtj2k_amd.so exports its host parser)"""
    L = m.load_library()
    L.j2k_parser_new.restype = ctypes.c_void_p
    p = ctypes.c_void_p(L.j2k_parser_new())
    try:
        plan = ctypes.POINTER(oracle.Plan)()              # the two layouts agree up to `blocks`
        buf = ctypes.create_string_buffer(bytes(data) + b"\0" * 64, len(data) + 64)
        o = oracle.make_opts()
        assert L.j2k_parse(p, buf, len(data), ctypes.byref(o), 0, ctypes.byref(plan)) == 0
        n = plan.contents.nblocks
        return np.frombuffer(ctypes.string_at(plan.contents.blocks, n * oracle.BLOCK_DTYPE.itemsize), dtype=oracle.BLOCK_DTYPE).copy()
    finally:
        L.j2k_parser_free(p)


@pytest.mark.parametrize("kw", [dict(transform=1, mct=1), dict(transform=0, qstep=1 / 8, mct=1), dict(transform=1, guard_bits=3),
                                dict(transform=0, qstep=0.37, expn_bias=2, guard_bits=1), dict(transform=1, tile=(32, 32), expn_bias=1)],
                         ids=["53_mct", "97", "53_guard3", "97_bias_guard1", "53_tiles_bias"])
def test_writer_with_the_sources_quantisation(orc, kw):
    """htj2k_enc_assemble_quant with a source's exponents, mantissas and guard bits: both parsers read the same M_b and
    the same step for every block of the output as for that block of the source"""
    levels = 2
    src = vecgen.encode(IMG, part1=True, nlevels=levels, cb=(4, 4), **kw)
    guard, expn, mant = xm.quant_tables(src, 3 * levels + 1)
    opts = dict(levels=levels, cb=(4, 4), mct=kw.get("mct", 0), irreversible=kw["transform"] == 0, tile=kw.get("tile", (0, 0)))
    n = len(m.Encoder.layout(70, 50, "rgb24", 8, **opts))
    out = m.Encoder.assemble_quant(70, 50, "rgb24", 8, [b""] * n, [0] * n, [1] * n, [-1] * n, guard, expn, mant, **opts)
    assert xm.quant_tables(out, 3 * levels + 1) == (guard, expn, mant)
    for parse in (product_plan_blocks, orc.plan_blocks):
        a, b = parse(src), parse(out)
        assert len(a) == len(b) == n
        key = lambda t: {(int(e["tcomp"]), int(e["plane_off"])): (int(e["M_b"]), float(e["f_step"]), int(e["i_step"]), int(e["w"]), int(e["h"]))
                         for e in t}
        assert key(a) == key(b)
    # the derived ladder would have written other exponents where the source was biased: the check is not vacuous
    if kw.get("expn_bias") and kw["transform"] == 1:
        assert expn[0][0] != 8 + kw.get("mct", 0)


def test_writer_refuses_bad_quantisation():
    n = len(m.Encoder.layout(16, 16, "gray", 8, levels=1))
    for guard, e in ((0, 9), (8, 9), (2, 32)):
        with pytest.raises(m.Htj2kError) as err:
            m.Encoder.assemble_quant(16, 16, "gray", 8, [b""] * n, [0] * n, [1] * n, [-1] * n, guard, [[e] * 4], levels=1)
        assert err.value.code == -22
