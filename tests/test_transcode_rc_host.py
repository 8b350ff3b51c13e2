"""CPU checks of the transcoder's byte budget (no GPU): the new entry points, htj2k_transcode_min_size against the host
writer, and the model of the candidates (tests/xc_rc_model.py) pinned with the reference's two block decoders."""
import ctypes

import numpy as np
import pytest

import ffmpeg_ht_amd as m
import oracle
import rc_model as rc
import rc_passes_model as pm
import vecgen
import xc_model as xm
import xc_rc_model as xrm

PATCHWELCOME = -0x45574150

SHAPES = [(1, 1), (3, 5), (4, 4), (17, 9), (64, 64)]


# ---------------------------------------------------------------- 1. the interface
def test_symbols_and_defaults():
    L = m.load_library()
    for name in ("htj2k_transcode_opts_default", "htj2k_transcode_batch_opts", "htj2k_transcode_frame_opts",
                 "htj2k_transcode_min_size", "htj2k_xc_rc_tables"):
        assert hasattr(L, name) and name in m.EXPORTS, name
    o = m.TranscodeOpts(77)
    L.htj2k_transcode_opts_default(ctypes.byref(o))
    assert o.target_bytes == 0 and ctypes.sizeof(o) == 8
    for f in ("transcode_min_size", "xc_rc_tables"):
        assert hasattr(m.Encoder, f)


def test_unit_entry_checks_arguments_before_the_context():
    L = m.load_library()
    plane = np.zeros((8, 8), np.int32)
    tab = (m.EncBlock * 1)()
    tab[0].x, tab[0].y, tab[0].w, tab[0].h = 0, 0, 8, 8
    one = (ctypes.c_int * 1)(1)
    d = np.zeros(16, np.uint64)
    l = np.zeros(16, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(bp, bk, nplanes, dist):
        return L.htj2k_xc_rc_tables(None, vp(plane), 8, 8, tab, 1, bp, bk, nplanes, dist, vp(l), vp(d), vp(d), vp(l), vp(l), vp(l))

    assert call(one, one, 16, vp(d)) == -38                 # HTJ2K_ERR_ENOSYS: the arguments are fine, there is no context
    assert call(one, (ctypes.c_int * 1)(4), 16, vp(d)) == -22
    assert call((ctypes.c_int * 1)(31), one, 16, vp(d)) == -22
    assert call(one, one, 17, vp(d)) == -22
    assert call(one, one, 16, None) == -22


# ---------------------------------------------------------------- 2. the smallest stream
R97 = dict(part1=True, mct=1, nlevels=3, cb=(4, 4), transform=0, qstep=1 / 8)
CASES = {                                                  # the definitions of tests/test_transcode_gpu.py
    "gray_33x17": (lambda: vecgen.synth_image(33, 17, 1, seed=1), dict(part1=True, nlevels=2, cb=(2, 2), transform=1)),
    "rgb_64x48_97": (lambda: vecgen.synth_image(64, 48, 3, seed=2), R97),
    "rgb_70x50_tiles": (lambda: vecgen.synth_image(70, 50, 3, seed=5), dict(part1=True, mct=1, nlevels=2, cb=(3, 3), tile=(32, 32))),
}


def empty_stream(src, kw, fmt, w, h, bits=8):
    """Encoder.assemble_quant of the source's parameters with every block left out"""
    levels = kw["nlevels"]
    opts = dict(levels=levels, cb=kw.get("cb", (6, 6)), mct=kw.get("mct", 0), irreversible=kw.get("transform", 1) == 0,
                tile=kw.get("tile", (0, 0)))
    guard, expn, mant = xm.quant_tables(src, 3 * levels + 1)
    n = len(m.Encoder.layout(w, h, fmt, bits, **opts))
    return m.Encoder.assemble_quant(w, h, fmt, bits, [b""] * n, [0] * n, [1] * n, [-1] * n, guard, expn, mant, **opts)


@pytest.mark.parametrize("name", sorted(CASES))
def test_min_size_is_the_all_empty_stream(name):
    img, kw = CASES[name]
    comps = img()
    fmt = "gray" if len(comps) == 1 else "rgb24"
    src = vecgen.encode(comps, **kw)
    want = empty_stream(src, kw, fmt, comps[0].shape[1], comps[0].shape[0])
    assert m.Encoder.transcode_min_size(src) == len(want)
    assert 0 < len(want) < m.Encoder.transcode_check(src)


@pytest.mark.parametrize("kw", [dict(part1=False), dict(roi_shift=12)], ids=["ht", "rgn"])
def test_min_size_refuses_what_check_refuses(kw):
    cs = vecgen.encode(vecgen.synth_image(70, 50, 3, seed=2), **dict(dict(part1=True, nlevels=3, mct=1), **kw))
    with pytest.raises(m.Htj2kError) as a:
        m.Encoder.transcode_check(cs)
    with pytest.raises(m.Htj2kError) as b:
        m.Encoder.transcode_min_size(cs)
    assert a.value.code == b.value.code == PATCHWELCOME
    assert str(a.value).split(": ", 1)[1] == str(b.value).split(": ", 1)[1]


# ---------------------------------------------------------------- 3. the model against the reference's block decoders
def p1_block(rng, w, h, band, d, amp, density):
    """a random block through the factory's EBCOT coder with its last d passes dropped -> (decode_cblk's words, K, n, M_b)"""
    vals = rng.integers(-amp, amp + 1, (h, w)) * (rng.random((h, w)) < density)
    vals[0, 0] = amp
    seg, lens, passes, K, n = vecgen.encode_block_p1(vals, band=band, style=0, drop_passes=d)
    M_b = K + 1
    data, length, starts = oracle.mq_block_layout(seg, lens, passes, 0)
    ret, t1 = oracle.mq_decode_block(data, length, n, K, w, h, M_b, 0, band, starts)
    assert ret == 1
    return t1, K, n, M_b


def word_mag(t, M_b):
    return (np.asarray(t).astype(np.int64) & 0x7FFFFFFF) >> (31 - M_b)


def coded_from(v_rel, pr, p_rel, passes):
    """per sample the lowest bit-plane of the indices the candidate (p', passes) codes for it, after the fall-back rule"""
    P = pr + p_rel
    if pm.falls_back(v_rel, p_rel, passes):
        return np.full(v_rel.shape, P, dtype=np.int64)
    sig, mem, _ = pm.membership(v_rel, p_rel)
    if passes == 3:
        return np.where(sig | mem, P, P + 1).astype(np.int64)
    return np.where(mem, P, P + 1).astype(np.int64)


def decode_candidate(v_rel, pr, p_rel, passes, M_b):
    data, lcup, lref, mu, coded = pm.code_block(v_rel, p_rel, passes)
    h, w = v_rel.shape
    if lcup == 0:
        return np.zeros((h, w), np.int32)
    cp = pr + p_rel + (coded > 1)
    assert mu + cp <= M_b
    r, got = oracle.ht_decode_block(data, lcup, lref, coded, M_b - 1 - cp, w, h, M_b)
    assert r == 1
    return got


def disagreements(got, t1, q, M_b):
    """samples whose decoded word differs from the source's word in a bit-plane >= q[sample], or in the sign of a sample
    that is not zero there"""
    a, b = word_mag(got, M_b) >> q, word_mag(t1, M_b) >> q
    return int(np.count_nonzero((a != b) | ((a != 0) & ((np.asarray(got) < 0) != (np.asarray(t1) < 0)))))


def source_blocks():
    rng = np.random.default_rng(811)
    for (w, h) in SHAPES:
        for d in range(8):
            for amp, density in ((3, 0.3), (200, 0.9), (40, 0.05)):
                t1, K, n, M_b = p1_block(rng, w, h, int(rng.integers(0, 4)), d, amp, density)
                if n:
                    yield t1, K, n, M_b


def test_model_against_the_block_decoders():
    """own-form distortion; every allowed candidate agrees with the source's word in every bit-plane it codes for the
    sample; the candidates the table disables.

    Disabled candidates, one example each: with k = 2 in the source, "one pass at pr" and "three passes at pr" decode,
    at a sample significant at pc, to a word whose bit pr is the coder's statement where the source's word has its half
    bit: the words differ.  With k = 3, "one pass at pr" decodes to the very words the source has (the samples SigProp
    did not reach are 0 in both): no example of a differing word exists, and the test states instead what is so: the
    words are equal, and the candidate codes plane pr for samples whose source coded nothing below pc."""
    seen_k, shown, checked = set(), set(), 0
    for t1, K, n, M_b in source_blocks():
        pr, k = xm.rule(K, n)
        idx = xm.raw_index(t1, M_b, K, n)
        v = xrm.relative(idx, pr)
        pc = pr + (k > 1)
        seen_k.add(k)
        nsig = int(np.count_nonzero(np.abs(idx.astype(np.int64)) >> pc))
        assert xrm.own_dist(idx, pr, k) == (nsig if k == 2 else 0), (K, n)
        # the own form is the form the rule gives, and it decodes to the source's words
        p0, k0 = xrm.own_form(v, k)
        form = xm.ht_form(idx, K, n)
        if form is not None:
            assert (pr + p0, k0) == form
            assert np.array_equal(decode_candidate(v, pr, p0, k0, M_b), t1)
        kmax = int(np.abs(v.astype(np.int64)).max()).bit_length()
        for p in range(min(kmax, 4)):
            for kk in (1, 2, 3):
                if not xrm.allowed(v, k, p, kk):
                    continue
                got = decode_candidate(v, pr, p, kk, M_b)
                assert disagreements(got, t1, coded_from(v, pr, p, kk), M_b) == 0, (K, n, p, kk)
                checked += 1
        # what the table disables at p' = 0
        for kk in (1, 2, 3):
            if kk in xrm.ALLOWED_AT_0[k] or (k, kk) in shown or nsig in (0, idx.size) or (kk > 1 and pm.falls_back(v, 0, kk)):
                continue
            got = decode_candidate(v, pr, 0, kk, M_b)
            if k == 2:
                assert disagreements(got, t1, coded_from(v, pr, 0, kk), M_b) > 0 and not np.array_equal(got, t1)
            else:
                _, mem, _ = pm.membership(v, 0)
                unreached = (np.abs(idx.astype(np.int64)) >> pc == 0) & ~mem
                if not unreached.any():
                    continue
                assert np.array_equal(got, t1) and (coded_from(v, pr, 0, kk)[unreached] == pr).all()
            shown.add((k, kk))
    assert seen_k == {1, 2, 3} and checked > 300
    assert shown == {(2, 1), (2, 3), (3, 1)}


def test_tables_of_the_model():
    """the restatement itself: the disabled entries, the weight, and the mapping back to planes of the indices"""
    rng = np.random.default_rng(5)
    idx = (rng.integers(-300, 301, (9, 17)) << 3).astype(np.int32)
    for k in (1, 2, 3):
        dist, d2, d3, sp, mr = xrm.tables(idx, 3, k)
        plain = rc.dist_row(xrm.relative(idx, 3))
        assert np.array_equal(dist[1:], plain[1:])
        assert int(dist[0]) == (int(plain[0]) if k == 1 else xrm.DISABLED)
        assert (int(d3[0]) == xrm.DISABLED) == (k == 2) and int(d2[0]) != xrm.DISABLED
    assert xrm.weight(0.5, 3) == 32.0 and xrm.absolute(3, 2) == 5 and xrm.absolute(3, rc.SKIP) == rc.SKIP
