"""CPU checks of the lossy (9/7) encoder's host side (no GPU): the step rule and the QCD / CAP / COD it writes, the
refusal of bad base steps, and the numpy model of the float stages (tests/enc97_model.py).  Blocks are coded by vecgen's
encode_block from the model's indices; htj2k_enc_assemble must then give vecgen's own encode(..., transform=0) byte for
byte, which pins the host writer and the model before any GPU run."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import enc97_model as e97
import enc_model as em
import ffmpeg_ht_amd as m
import vecgen

QSTEPS = [1 / 32, 0.25, 1.0, 4.0, 16.0]
PATCHWELCOME = -0x45574150


def synth(fmt, w, h, bits, seed=3):
    return [vecgen.synth_image(cw, ch, 1, depth=bits, seed=seed + c)[0] for c, (cw, ch) in enumerate(em.comp_dims(fmt, w, h))]


def main_header(cs):
    return cs[:cs.index(b"\xff\x90")]


def assemble_from_model(comps, fmt, w, h, bits, levels, cb, qstep, mct=None):
    mct = em.mct_default(fmt) if mct is None else mct
    planes = e97.index_planes(comps, fmt, bits, levels, mct, qstep)
    opts = dict(levels=levels, cb=cb, mct=int(mct), irreversible=True, qstep=qstep)
    blocks = m.Encoder.layout(w, h, fmt, bits, **opts)
    data, mu = [], []
    for b in blocks:
        v = planes[b["comp"]][b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]]
        if not v.any():
            data.append(b"")
            mu.append(0)
            continue
        d, lcup, _, maxu = vecgen.encode_block(v)
        data.append(d[:lcup])
        mu.append(maxu)
    return m.Encoder.assemble(w, h, fmt, bits, data, max_u=mu, **opts)


def check_against_vecgen(comps, fmt, w, h, bits, levels, cb, qstep, mct=None):
    mct = em.mct_default(fmt) if mct is None else mct
    cs = assemble_from_model(comps, fmt, w, h, bits, levels, cb, qstep, mct)
    g = em.qcd_guard_bits(cs)
    ref = vecgen.encode(comps, **e97.vecgen_args(fmt, w, h, bits, levels, cb, mct, g, qstep))
    assert cs == ref, "%s %dx%d %d bits, %d levels, cb %s, qstep %g" % (fmt, w, h, bits, levels, cb, qstep)
    return cs


@pytest.mark.parametrize("fmt,bits", [("gray", 8), ("rgb24", 8), ("rgb48le", 10), ("yuv420p", 8)])
@pytest.mark.parametrize("levels", [0, 1, 5, 32])
def test_main_header_equals_vecgen(fmt, bits, levels):
    w, h = 64, 48
    for q in QSTEPS:
        opts = dict(levels=levels, irreversible=True, qstep=q)
        st = e97.steps(q, bits, levels)
        if not e97.exponents_valid(q, bits, levels):
            with pytest.raises(m.Htj2kError) as e:
                m.Encoder.layout(w, h, fmt, bits, **opts)
            assert e.value.code == -22
            continue
        if max(e for e, _, _ in st) + 2 - 1 > 30:           # M_b beyond 30 bits: refused as for 5/3
            with pytest.raises(m.Htj2kError) as e:
                blocks = m.Encoder.layout(w, h, fmt, bits, **opts)
                m.Encoder.assemble(w, h, fmt, bits, [b""] * len(blocks), **opts)
            assert e.value.code == PATCHWELCOME
            continue
        blocks = m.Encoder.layout(w, h, fmt, bits, **opts)
        cs = m.Encoder.assemble(w, h, fmt, bits, [b""] * len(blocks), **opts)
        comps = [np.zeros((ch, cw), np.int32) for cw, ch in em.comp_dims(fmt, w, h)]
        ref = vecgen.encode(comps, **e97.vecgen_args(fmt, w, h, bits, levels, (6, 6), em.mct_default(fmt), 2, q))
        assert main_header(cs) == main_header(ref), (fmt, bits, levels, q)
        cap = cs.index(b"\xff\x50")
        assert int.from_bytes(cs[cap + 8:cap + 10], "big") & 0x20            # Ccap15 HTIRV
        cod = cs.index(b"\xff\x52")
        assert cs[cod + 13] == 0                                             # 9/7
        qcd = cs.index(b"\xff\x5c")
        assert cs[qcd + 4] == 2 << 5 | 2 and int.from_bytes(cs[qcd + 2:qcd + 4], "big") == 3 + 2 * (3 * levels + 1)
        entries = [int.from_bytes(cs[qcd + 5 + 2 * g:qcd + 7 + 2 * g], "big") for g in range(3 * levels + 1)]
        assert entries == [e << 11 | mnt for e, mnt, _ in st]
        assert b"\xff\x5d" not in main_header(cs)                            # one depth: no QCC


def test_layout_reports_97_exponents():
    for fmt, bits, levels, q in [("rgb24", 8, 5, 1.0), ("gray16le", 12, 3, 0.25), ("yuv420p", 8, 0, 4.0)]:
        blocks = m.Encoder.layout(96, 80, fmt, bits, levels=levels, irreversible=True, qstep=q)
        st = e97.steps(q, bits, levels)
        for b in blocks:
            want = st[e97.band_index(b["res"], b["band"] - (b["res"] > 0))][0]
            assert b["expn"] == want, (fmt, b)
        lossless = m.Encoder.layout(96, 80, fmt, bits, levels=levels)
        assert [(b["x"], b["y"], b["w"], b["h"]) for b in blocks] == [(b["x"], b["y"], b["w"], b["h"]) for b in lossless]


def _assemble_raw(opts, cap=1 << 16):
    """htj2k_enc_assemble of an all-empty 64 x 48 gray frame into a buffer of 0xAB: (result, out_len, untouched)"""
    L = m.load_library()
    n = max(L.htj2k_enc_layout(64, 48, em.pix("gray"), 8, ctypes.byref(m._enc_opts()), None, 0), 1)
    lc = (ctypes.c_int * n)()
    ptrs = (ctypes.c_void_p * n)()
    out = np.full(cap, 0xAB, np.uint8)
    ln = ctypes.c_size_t(12345)
    r = L.htj2k_enc_assemble(64, 48, em.pix("gray"), 8, ctypes.byref(opts), ptrs, lc, None, n,
                             out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap), ctypes.byref(ln))
    return r, ln.value, bool((out == 0xAB).all())


@pytest.mark.parametrize("qstep", [0.0, -1.0, math.nan, math.inf, -math.inf, 1e-7, 1e5])
def test_bad_qstep_refused(qstep):
    """not finite, not positive, or an exponent past 31 (fine steps) or below 0 (coarse ones): EINVAL, nothing written"""
    assert not (0 < qstep < math.inf) or not e97.exponents_valid(qstep, 8, 5)
    r, ln, untouched = _assemble_raw(m._enc_opts(irreversible=True, qstep=qstep))
    assert r == -22 and ln == 0 and untouched
    assert m.Encoder.bound(64, 48, "gray", 8, irreversible=True, qstep=qstep) == 0
    with pytest.raises(m.Htj2kError) as e:
        m.Encoder.layout(64, 48, "gray", 8, irreversible=True, qstep=qstep)
    assert e.value.code == -22


def test_exponent_limits_are_exact():
    """the largest and smallest base steps the 0 .. 31 exponents allow are accepted; a little beyond is not"""
    bits, levels = 8, 5
    # LL has the finest step (d = qstep * 2^-2), the level-1 bands the coarsest (d = qstep)
    fine, coarse = 2.0 ** (bits - 31) * 4, 2.0 ** (bits + 1) * (1 - 2 ** -11)
    # 2^(bits + 1) (1 - 2^-13): a mantissa that rounds to 2048 carries into the exponent, which then falls below 0
    for q, ok in [(fine, True), (fine * (1 - 2 ** -12), False), (coarse, True), (2.0 ** (bits + 1) * (1 - 2 ** -13), False),
                  (2.0 ** (bits + 1), False)]:
        assert e97.exponents_valid(q, bits, levels) == ok, q
        r, _, _ = _assemble_raw(m._enc_opts(levels=levels, irreversible=True, qstep=q))
        if ok:
            assert r == 0 or r == PATCHWELCOME, (q, r)       # accepted by the step rule (M_b may still be too large)
        else:
            assert r == -22, q


def test_bad_irreversible_refused():
    for v in (-1, 2):
        r, ln, untouched = _assemble_raw(m._enc_opts(irreversible=v))
        assert r == -22 and ln == 0 and untouched


def test_lossless_ignores_qstep():
    """irreversible off: qstep is not read, and the old five-field options (a zero tail) mean what they meant"""
    comps = synth("rgb24", 40, 24, 8)
    ref = None
    for q in (0.0, -3.0, math.nan, 1.0):
        blocks = m.Encoder.layout(40, 24, "rgb24", 8, levels=3, qstep=q)
        assert all(b["expn"] == 8 + (b["band"] + 1) // 2 + 1 for b in blocks)
        planes = em.coefficient_planes(comps, "rgb24", 8, 3, True)
        data = []
        for b in blocks:
            v = planes[b["comp"]][b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]]
            d, lcup, _, _ = vecgen.encode_block(v) if v.any() else (b"", 0, 0, 0)
            data.append(d[:lcup])
        cs = m.Encoder.assemble(40, 24, "rgb24", 8, data, levels=3, qstep=q)
        ref = cs if ref is None else ref
        assert cs == ref
    assert ref == vecgen.encode(comps, **em.vecgen_args("rgb24", 40, 24, 8, 3, (6, 6), True, em.qcd_guard_bits(ref)))
    o = m.EncOpts(5, 6, 6, -1, 0)
    assert o.irreversible == 0 and o.qstep == 0.0
    L = m.load_library()
    assert L.htj2k_enc_layout(64, 48, em.pix("gray"), 8, ctypes.byref(o), None, 0) == \
        len(m.Encoder.layout(64, 48, "gray", 8))


def test_model_lifting_matches_closed_checks():
    """the model's 9/7: a line of one sample is scaled by 1 / X in each direction at every level (a 1 x 1 LL too), and
    a constant line gives a zero high band and, un-normalised, a low band of K times the constant, up to rounding"""
    want = np.float32(100)
    for _ in range(2 * 3):
        want = want * e97.INV_X97
    assert e97.fdwt97(np.full((1, 1), 100, np.float32), 3)[0, 0] == want
    y = e97.dwt97(np.full((9,), 10.0, np.float32), 0)
    assert np.abs(y[5:]).max() < 1e-4 and np.abs(y[:5] - 10.0 * e97.K97).max() < 1e-4


SMALL = [(1, 1), (3, 1), (1, 5), (7, 3), (17, 9), (33, 17)]


@pytest.mark.parametrize("fmt", ["gray", "rgb24", "yuv420p"])
@pytest.mark.parametrize("w,h", SMALL)
def test_assemble_equals_vecgen_small(fmt, w, h):
    comps = synth(fmt, w, h, 8)
    for levels, q in itertools.product([0, 1, 5], QSTEPS):
        check_against_vecgen(comps, fmt, w, h, 8, levels, (5, 5), q)


@pytest.mark.parametrize("fmt", ["gray", "rgb24", "yuv420p"])
def test_assemble_equals_vecgen_640x480(fmt):
    comps = synth(fmt, 640, 480, 8)
    for levels, cb, q in [(0, (6, 6), 1.0), (1, (5, 5), 0.25), (5, (6, 6), 1 / 32), (5, (6, 6), 1.0), (5, (7, 5), 4.0),
                          (5, (6, 6), 16.0)]:
        check_against_vecgen(comps, fmt, 640, 480, 8, levels, cb, q)


def test_assemble_equals_vecgen_deep_levels_and_12_bits():
    """levels past a 1 x 1 LL (scaled again at each), and the 12-bit ICT of the decoder's C3 configuration"""
    comps = synth("gray", 19, 11, 8)
    for levels in (6, 9):
        check_against_vecgen(comps, "gray", 19, 11, 8, levels, (4, 4), 1.0)
    comps = synth("rgb48le", 45, 31, 12)
    for q in (0.25, 1.0, 4.0):
        check_against_vecgen(comps, "rgb48le", 45, 31, 12, 4, (5, 5), q)


def test_oracle_decodes_assembled_97_streams(orc):
    """the model's streams decode (oracle, float 9/7) to within a few steps of the source"""
    for fmt, bits, q in [("rgb24", 8, 0.25), ("gray", 8, 1.0), ("yuv420p", 8, 0.25)]:
        comps = synth(fmt, 48, 40, bits)
        cs = check_against_vecgen(comps, fmt, 48, 40, bits, 3, (5, 5), q)
        _, planes, _ = orc.decode(cs, req_pix_fmt=em.pix(fmt))
        want = em.to_planes(comps, fmt, bits)
        for a, b in zip(planes, want):
            d = np.abs(a.reshape(-1).astype(np.int64) - b.reshape(-1).astype(np.int64))
            assert d.max() <= 8 * max(q, 1), (fmt, int(d.max()))
