"""CPU checks of HT refinement passes in the encoder (no GPU): the model of tests/rc_passes_model.py against the
reference block decoder, htj2k_enc_assemble_passes (the pass count, the two length fields and the zero bit-planes,
checked byte for byte against vecgen's encode(..., passes=k) and with the oracle's parser and decoders), its refusals,
the option and the bound."""
import ctypes

import numpy as np
import pytest

import enc_model as em
import enc_opj
import enc_tiles_model as tm
import ffmpeg_ht_amd as m
import oracle
import rc_model as rc
import rc_passes_model as pm
import vecgen


def decode_block(v, p, passes):
    """vecgen's block of shifted(v, p) through the reference block decoder -> (twice the magnitudes, negative flags)"""
    data, lcup, lref, mu = vecgen.encode_block(rc.shifted(v, p), passes=passes)
    h, w = v.shape
    Mb = mu + p + 2
    r, got = oracle.ht_decode_block(data, lcup, lref, passes, Mb - 1 - (p + 1), w, h, Mb)
    assert r >= 0
    got = got.astype(np.int64) & 0xFFFFFFFF
    return (got & 0x7FFFFFFF) >> (30 - Mb), (got >> 31) != 0


def test_model_equals_the_reference_block_decoder():
    """random blocks 1 x 1 .. 40 x 40, five amplitudes, planes 0 .. 2, passes 2 and 3: the reconstruction of every
    sample, hence the sum of d^2, and the sign wherever the reconstruction is not 0"""
    rng = np.random.default_rng(2024)
    n = 0
    for amp in (2, 3, 5, 40, 3000):
        for _ in range(24):
            w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
            v = (rng.integers(-amp, amp + 1, size=(h, w)) * (rng.random((h, w)) < rng.choice([0.1, 0.5, 1.0]))).astype(np.int32)
            p = int(rng.integers(0, 3))
            for passes in (2, 3):
                sig, _, _ = pm.membership(v, p)
                if not sig.any():
                    continue                              # vecgen's cleanup pass of an all-zero block: the fallback's case
                mag2, neg = decode_block(v, p, passes)
                # the model without its fallback rule: vecgen codes two passes even where Dref is empty
                want = pm.recon2(v, p, passes) if not pm.falls_back(v, p, passes) else \
                    np.where(sig, 2 * ((np.abs(v.astype(np.int64)) >> (p + 1)) << (p + 1)) + (2 << p), 0)
                assert np.array_equal(mag2, want), (w, h, amp, p, passes)
                assert np.array_equal(neg[want != 0], (v < 0)[want != 0])
                m2 = np.abs(v.astype(np.int64))
                d = np.where(m2 > 0, 2 * m2 + 1 - mag2, 0)
                if not pm.falls_back(v, p, passes):
                    assert int((d * d).sum()) == pm.dist(v, p, passes)
                n += 1
    assert n > 150


def test_membership_chains():
    """a chain of newly significant members runs through the block in scan order, and only forwards"""
    v = np.ones((9, 10), np.int32)
    v[0, 0] = 4
    sig, mem, new = pm.membership(v, 0)
    assert mem.sum() == 89 and new.sum() == 89
    v = np.ones((9, 10), np.int32)
    v[8, 9] = 4                                           # the last sample in scan order: its neighbours, then theirs to come
    sig, mem, new = pm.membership(v, 0)
    assert mem[7, 8] and mem[7, 9] and mem[8, 8] and not mem[0, 0] and mem.sum() < 89
    assert pm.bit_counts(v, 0) == (int(mem.sum()) * 2, 1)


def test_membership_by_whole_array_steps_is_the_definition():
    """pm.membership (array steps, the serial scan only where they do not settle) against the scan, sample by sample"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        w, h, amp = int(rng.integers(1, 41)), int(rng.integers(1, 41)), int(rng.choice([1, 2, 3, 8]))
        v = (rng.integers(-amp, amp + 1, size=(h, w)) * (rng.random((h, w)) < rng.choice([0.1, 0.5, 1.0]))).astype(np.int32)
        for p in (0, 1):
            assert all(np.array_equal(a, b) for a, b in zip(pm.membership(v, p), pm.membership_serial(v, p)))
    v = np.ones((64, 64), np.int32)                       # a chain longer than the array steps follow
    v[0, 0] = 5
    assert all(np.array_equal(a, b) for a, b in zip(pm.membership(v, 0), pm.membership_serial(v, 0)))


def noisy(fmt, w, h, seed):
    """low-amplitude noise about mid-grey: every 16 x 16 block has samples on both sides of 2"""
    rng = np.random.default_rng(seed)
    return [rng.integers(121, 136, size=(ch, cw)).astype(np.int32) for cw, ch in em.comp_dims(fmt, w, h)]


@pytest.mark.parametrize("fmt,w,h", [("gray", 96, 64), ("rgb24", 64, 128)])
@pytest.mark.parametrize("levels", [0, 1, 2])
@pytest.mark.parametrize("passes", [2, 3])
def test_assemble_equals_vecgen(orc, fmt, w, h, levels, passes):
    comps = noisy(fmt, w, h, levels)
    cs, coded, idx, blocks = pm.frame_stream(comps, fmt, w, h, 8, passes, levels=levels, cb=(4, 4))
    # the precondition: no block falls back (vecgen has no fallback rule), so the comparison is not vacuous
    for b, c in zip(blocks, coded):
        assert (np.abs(rc.block_view(idx, b)) >= 2).any() and c[2] > 0 and c[4] == passes
    g = em.qcd_guard_bits(cs)
    ref = vecgen.encode(comps, passes=passes, **em.vecgen_args(fmt, w, h, 8, levels, (4, 4), em.mct_default(fmt), g))
    assert cs == ref
    check_plan_and_blocks(orc, cs, fmt, w, h, idx, blocks, coded, [0] * len(blocks))


def check_plan_and_blocks(orc, cs, fmt, w, h, idx, blocks, coded, planes, tiles=None):
    """what the oracle's parser reads for every block is what went in, and the reference block decoder gives the
    model's reconstruction; the whole stream decodes without block errors.  `tiles`: Encoder.tiles() of a tiled stream,
    whose tile-components the parser numbers tile by tile and lays out one behind the other"""
    g = em.qcd_guard_bits(cs)
    dims = em.comp_dims(fmt, w, h)
    tiles = tiles or [dict(blk0=0, nblk=len(blocks), rects=[(0, 0, cw, ch) for cw, ch in dims])]
    tab = orc.plan_blocks(cs, req_pix_fmt=em.pix(fmt))
    base = {c: min(int(p["plane_off"]) for p in tab if p["tcomp"] == c) for c in {int(p["tcomp"]) for p in tab}}
    plan = {(int(p["tcomp"]), int(p["plane_off"]) - base[int(p["tcomp"])]): p for p in tab}
    tile_of = [t for t, T in enumerate(tiles) for _ in range(T["nblk"])]
    for i, (b, (data, lcup, lref, mu, np_), p) in enumerate(zip(blocks, coded, planes)):
        if not lcup:
            continue
        Mb = b["expn"] + g - 1
        x0, y0, x1, _ = tiles[tile_of[i]]["rects"][b["comp"]]
        e = plan[(tile_of[i] * len(dims) + b["comp"], (b["y"] - y0) * (x1 - x0) + b["x"] - x0)]
        cp = p + (np_ > 1)
        assert (e["zbp"], e["npasses"], e["M_b"], e["lcup"], e["lref"]) == (Mb - 1 - cp, np_, Mb, lcup, lref), (b, p)
        v = rc.block_view(idx, b)
        r, got = oracle.ht_decode_block(data, lcup, lref, np_, Mb - 1 - cp, b["w"], b["h"], Mb)
        got = got.astype(np.int64) & 0xFFFFFFFF
        want = pm.recon2(v, p, np_)
        assert r >= 0 and np.array_equal((got & 0x7FFFFFFF) >> (30 - Mb), want), (b, p, np_)
        assert np.array_equal((got >> 31 != 0)[want != 0], (v < 0)[want != 0])
    orc.decode_blocks(cs, req_pix_fmt=em.pix(fmt))
    assert orc.block_errors() == 0


def synth(fmt, w, h, bits, seed=3):
    return [vecgen.synth_image(cw, ch, 1, depth=bits, seed=seed + c)[0] for c, (cw, ch) in enumerate(em.comp_dims(fmt, w, h))]


@pytest.mark.parametrize("irreversible", [False, True])
def test_mixed_pass_counts_planes_and_tiles(orc, irreversible):
    """blocks of 1, 2 and 3 passes at planes of their own in one precinct, blocks left out, with and without tiles"""
    rng = np.random.default_rng(5 + irreversible)
    for fmt, bits, w, h, tile in [("rgb24", 8, 64, 40, (0, 0)), ("yuv420p10le", 10, 97, 61, (0, 0)), ("gray", 8, 160, 96, (64, 48))]:
        opts = dict(levels=3, cb=(4, 4), irreversible=irreversible, qstep=0.25, tile=tile)
        mct = em.mct_default(fmt)
        comps = synth(fmt, w, h, bits)
        idx = tm.coefficient_planes(comps, fmt, w, h, bits, 3, mct, tile, 0.25 if irreversible else None) if tile != (0, 0) \
            else rc.indices(comps, fmt, bits, 3, mct, irreversible, 0.25)
        blocks = m.Encoder.layout(w, h, fmt, bits, **opts)
        coded, planes = [], []
        for b in blocks:
            v = rc.block_view(idx, b)
            k = int(np.abs(v.astype(np.int64)).max()).bit_length()
            p = -1 if rng.random() < 0.1 else int(rng.integers(0, max(k, 1)))
            coded.append(pm.code_block(v, p, int(rng.integers(1, 4))))
            planes.append(p if coded[-1][1] else (p if rng.random() < 0.5 else -1))
        assert {c[4] for c in coded if c[1]} == {1, 2, 3}
        cs = pm.assemble(coded, w, h, fmt, bits, planes=planes, **opts)
        check_plan_and_blocks(orc, cs, fmt, w, h, idx, blocks, coded, planes,
                              m.Encoder.tiles(w, h, fmt, bits, **opts) if tile != (0, 0) else None)
        info, _, _ = orc.decode(cs, req_pix_fmt=em.pix(fmt))
        assert orc.block_errors() == 0 and (info.width, info.height) == (w, h)


@pytest.mark.skipif(not enc_opj.HAVE_OPJ, reason="Pillow/OpenJPEG not importable")
@pytest.mark.parametrize("irreversible", [False, True])
def test_openjpeg_decodes_the_streams(orc, irreversible):
    for fmt, bits, w, h in [("rgb24", 8, 64, 40), ("gray", 8, 97, 61), ("gray16le", 12, 33, 17)]:
        comps = synth(fmt, w, h, bits)
        for passes in (2, 3):
            cs, coded, _, _ = pm.frame_stream(comps, fmt, w, h, bits, passes, levels=3, cb=(4, 4), irreversible=irreversible,
                                              qstep=0.25)
            assert passes in [c[4] for c in coded]
            _, want, _ = orc.decode(cs, req_pix_fmt=em.pix(fmt))
            assert orc.block_errors() == 0
            bad = enc_opj.compare(cs, fmt, bits, w, h, want, irreversible, orc=orc)
            assert bad is None, (fmt, passes, bad)


def test_lblock_grows_from_either_field():
    """one 64 x 64 block: a long Dcup with a short Dref, and a Dref longer than Dcup; the oracle's parser reads both"""
    orc = oracle.OracleDecoder()
    rng = np.random.default_rng(9)
    long_cup = rng.integers(-(1 << 12), 1 << 12, size=(64, 64)).astype(np.int32)
    long_cup[::2] = 0                                       # rows of zeros: members all over, lref well below lcup
    long_ref = np.where(rng.random((64, 64)) < 0.02, 2, -1).astype(np.int32)   # few significant, every other sample a member
    seen = []
    for v in (long_cup, long_ref):
        for passes in (2, 3):
            c = pm.code_block(v, 0, passes)
            assert c[4] == passes
            seen.append((c[1].bit_length(), c[2].bit_length() - (passes == 3)))
            cs = pm.assemble([c], 64, 64, "gray", 8, levels=0, guard_bits=7)
            tab = orc.plan_blocks(cs, req_pix_fmt=em.pix("gray"))
            assert len(tab) == 1 and (tab[0]["lcup"], tab[0]["lref"], tab[0]["npasses"]) == (c[1], c[2], passes)
    assert any(a > b for a, b in seen) and any(b > a for a, b in seen)
    orc.close()


def _raw(o, lcup, lref, npasses, planes=None, n=None, mu=None):
    L = m.load_library()
    nb = len(m.Encoder.layout(64, 48, "gray", 8, levels=o.levels, cb=(o.cb_w_log2, o.cb_h_log2)))
    n = nb if n is None else n
    buf = ctypes.create_string_buffer(b"\xA5" * 64, 64)
    ptrs = (ctypes.c_void_p * nb)(*[ctypes.cast(buf, ctypes.c_void_p)] * nb)
    arr = lambda v: None if v is None else (ctypes.c_int * nb)(*v)
    out = ctypes.create_string_buffer(b"\x5A" * 65536, 65536)
    ln = ctypes.c_size_t(77)
    r = L.htj2k_enc_assemble_passes(64, 48, em.pix("gray"), 8, ctypes.byref(o), ptrs, arr(lcup), arr(lref), arr(npasses),
                                    arr(mu), arr(planes), n, out, ctypes.c_size_t(65536), ctypes.byref(ln))
    return r, ln.value, out.raw == b"\x5A" * 65536, nb


def test_refusals():
    o = m._enc_opts(levels=1, cb=(6, 6))
    _, _, _, nb = _raw(o, None, None, None, n=0)
    ok = lambda **kw: _raw(o, kw.get("lcup", [20] * nb), kw.get("lref", [5] * nb), kw.get("npasses", [2] * nb), kw.get("planes"))
    assert ok()[0] == 0
    assert ok(npasses=[3] * nb)[0] == 0 and ok(lref=[0] * nb, npasses=[1] * nb)[0] == 0
    for bad in (dict(npasses=[0] + [2] * (nb - 1)), dict(npasses=[4] + [2] * (nb - 1)),     # a pass count outside 1 .. 3
                dict(npasses=[1] + [2] * (nb - 1)),                                      # lref > 0 with one pass
                dict(lref=[0] + [5] * (nb - 1)),                                         # lref = 0 with more than one
                dict(lref=[-1] + [5] * (nb - 1)),
                dict(lcup=[0] + [20] * (nb - 1)),                                        # Dref without Dcup
                dict(planes=[-2] + [0] * (nb - 1)), dict(planes=[-1] + [0] * (nb - 1)),  # the plane refusals
                dict(planes=[31] + [0] * (nb - 1)),                                      # p + 1 beyond 31
                dict(planes=[30] + [0] * (nb - 1))):                                     # p + 1 makes zbp negative
        r, ln, untouched, _ = ok(**bad)
        assert r == -22 and ln == 0 and untouched, bad
    # with one pass plane 31 is as before: refused for zbp, not for the range; plane 8 fits one pass, not two, at G = 2
    one = dict(lref=[0] * nb, npasses=[1] * nb)
    e = m.Encoder.layout(64, 48, "gray", 8, levels=1, cb=(6, 6))[0]["expn"]
    assert ok(planes=[e] + [0] * (nb - 1), **one)[0] == 0
    assert ok(planes=[e] + [0] * (nb - 1))[0] == -22
    assert ok(planes=[e - 1] + [0] * (nb - 1))[0] == 0
    # npasses without lref
    assert _raw(o, [20] * nb, None, [1] * nb)[0] == -22
    for k in (-1, 4, 7):
        bad = m._enc_opts(levels=1, ht_passes=k)
        assert _raw(bad, [20] * nb, [5] * nb, [2] * nb)[0] == -22
        assert m.Encoder.bound(64, 48, "gray", 8, ht_passes=k) == 0
        with pytest.raises(m.Htj2kError) as err:
            m.Encoder.layout(64, 48, "gray", 8, ht_passes=k)
        assert err.value.code == -22


def test_option_default_and_one_pass_bytes():
    L = m.load_library()
    o = m.EncOpts(9, 9, 9, 9, 9, 9, 9.0, 9, 9, 9, 9)
    L.htj2k_enc_opts_default(ctypes.byref(o))
    assert o.ht_passes == 0 and (o.tile_w, o.tile_h, o.target_bytes) == (0, 0, 0)
    assert m.EncOpts(5, 6, 6, -1, 0).ht_passes == 0 and m._enc_opts().ht_passes == 0 and m._enc_opts(ht_passes=3).ht_passes == 3
    for fmt, bits, w, h in [("rgb24", 8, 64, 40), ("gray", 8, 17, 9)]:
        opts = dict(levels=3, cb=(4, 4))
        blocks = m.Encoder.layout(w, h, fmt, bits, **opts)
        idx = rc.indices(synth(fmt, w, h, bits), fmt, bits, 3, em.mct_default(fmt), False, 1.0)
        c = [rc.code_block(rc.block_view(idx, b), 0) for b in blocks]
        data, mu = [x[0] for x in c], [x[2] for x in c]
        ref = m.Encoder.assemble(w, h, fmt, bits, data, max_u=mu, **opts)
        for k in (0, 1, 2, 3):                               # the option does not touch what assemble writes
            assert m.Encoder.assemble(w, h, fmt, bits, data, max_u=mu, ht_passes=k, **opts) == ref
            assert m.Encoder.assemble(w, h, fmt, bits, data, max_u=mu, lref=[0] * len(data), passes=[1] * len(data),
                                      ht_passes=k, **opts) == ref
            assert m.Encoder.layout(w, h, fmt, bits, ht_passes=k, **opts) == blocks


def test_bound_covers_worst_case_blocks():
    """the bound is what it was for ht_passes <= 1, and holds a stream of blocks whose every member is newly significant
    and negative and whose significant samples all have bit 0 set, so that both passes are stuffed throughout"""
    for fmt, w, h, cb in [("gray", 128, 64, (6, 6)), ("gray", 64, 64, (4, 4)), ("rgb24", 33, 17, (5, 5))]:
        opts = dict(levels=1, cb=cb)
        base = m.Encoder.bound(w, h, fmt, 8, **opts)
        assert m.Encoder.bound(w, h, fmt, 8, ht_passes=0, **opts) == base == m.Encoder.bound(w, h, fmt, 8, ht_passes=1, **opts)
        blocks = m.Encoder.layout(w, h, fmt, 8, **opts)
        for passes in (2, 3):
            coded = []
            for b in blocks:
                v = np.full((b["h"], b["w"]), -1, np.int32)
                v[::3, ::3] = -3
                c = pm.code_block(v, 0, passes)
                _, mem, new = pm.membership(v, 0)
                if c[4] > 1:
                    assert mem.sum() == new.sum() and c[2] >= (2 * int(mem.sum())) // 8
                    assert c[2] <= (2 * b["w"] * b["h"] + 6) // 7 + 2
                coded.append(c)
            cs = pm.assemble(coded, w, h, fmt, 8, **opts)
            assert len(cs) <= m.Encoder.bound(w, h, fmt, 8, ht_passes=passes, **opts)
            assert m.Encoder.bound(w, h, fmt, 8, ht_passes=passes, **opts) > base
