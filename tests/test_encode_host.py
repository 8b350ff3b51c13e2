"""CPU checks of the encoder's host side (no GPU): the code-block layout, the header and packet writer and the guard
bits.  Blocks are coded by vecgen's encode_block from a numpy model of the transform stages (tests/enc_model.py);
htj2k_enc_assemble must then give vecgen's own encode(...) byte for byte."""
import ctypes
import itertools

import numpy as np
import pytest

import enc_model as em
import ffmpeg_ht_amd as m
import vecgen

SIZES = [(1, 1), (1, 255), (255, 1), (17, 9), (640, 480)]
CBS = [(6, 6), (5, 5), (7, 5), (10, 2)]
FMTS = ["gray", "rgb24", "yuv422p", "yuv420p"]


def levels_for(w, h):
    return [0, 1, 5, int(np.log2(min(w, h))) + 2]


def synth(fmt, w, h, bits, seed=3):
    dims = em.comp_dims(fmt, w, h)
    out = []
    for c, (cw, ch) in enumerate(dims):
        out.append(vecgen.synth_image(cw, ch, 1, depth=bits, seed=seed + c)[0])
    return out


def assemble_from_model(comps, fmt, w, h, bits, levels, cb, mct=None, guard_bits=0):
    mct = em.mct_default(fmt) if mct is None else mct
    planes = em.coefficient_planes(comps, fmt, bits, levels, mct)
    blocks = m.Encoder.layout(w, h, fmt, bits, levels=levels, cb=cb, mct=int(mct), guard_bits=guard_bits)
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
    return m.Encoder.assemble(w, h, fmt, bits, data, max_u=mu, levels=levels, cb=cb, mct=int(mct), guard_bits=guard_bits)


def check_against_vecgen(comps, fmt, w, h, bits, levels, cb, mct=None):
    mct = em.mct_default(fmt) if mct is None else mct
    cs = assemble_from_model(comps, fmt, w, h, bits, levels, cb, mct)
    g = em.qcd_guard_bits(cs)
    ref = vecgen.encode(comps, **em.vecgen_args(fmt, w, h, bits, levels, cb, mct, g))
    assert cs == ref, "%s %dx%d %d bits, %d levels, cb %s" % (fmt, w, h, bits, levels, cb)
    return cs


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("w,h", SIZES[:4])
def test_assemble_equals_vecgen_small(fmt, w, h):
    comps = synth(fmt, w, h, 8)
    for levels, cb in itertools.product(levels_for(w, h), CBS):
        check_against_vecgen(comps, fmt, w, h, 8, levels, cb)


@pytest.mark.parametrize("fmt", FMTS)
def test_assemble_equals_vecgen_640x480(fmt):
    comps = synth(fmt, 640, 480, 8)
    for levels, cb in [(0, (6, 6)), (1, (5, 5)), (5, (6, 6)), (5, (7, 5)), (5, (10, 2)), (11, (6, 6))]:
        check_against_vecgen(comps, fmt, 640, 480, 8, levels, cb)


@pytest.mark.parametrize("bits", [8, 12, 16])
def test_full_range_noise_raises_guard_bits_only_when_needed(bits):
    fmt = "rgb48le" if bits > 8 else "rgb24"
    rng = np.random.default_rng(bits)
    comps = [rng.integers(0, 1 << bits, size=(33, 47)).astype(np.int32) for _ in range(3)]
    cs = check_against_vecgen(comps, fmt, 47, 33, bits, 5, (5, 5))
    g = em.qcd_guard_bits(cs)
    assert g == 2                                # full-range noise fits the default; 2 is also the least G written


def test_guard_bits_raised_exactly_to_what_a_block_needs():
    """G = max(2, max(U - expn + 1)): raised by the largest U of any block, and no further.  (Pixel content cannot get
    there -- a 16-bit HH band with MCT peaks at U = 20 = M_b for G = 2 -- so the blocks' U are given.)"""
    w, h, fmt = 40, 24, "rgb24"
    comps = synth(fmt, w, h, 8)
    blocks = m.Encoder.layout(w, h, fmt, 8, levels=2, cb=(4, 4))
    planes = em.coefficient_planes(comps, fmt, 8, 2, True)
    data = []
    for b in blocks:
        v = planes[b["comp"]][b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]]
        d, lcup, _, _ = vecgen.encode_block(v) if v.any() else (b"", 0, 0, 0)
        data.append(d[:lcup])
    for extra in (0, 1, 3, 5):
        mu = [b["expn"] + 1 for b in blocks]                   # what G = 2 holds
        k = len(blocks) // 2
        mu[k] += extra
        want = max(2, mu[k] - blocks[k]["expn"] + 1)
        cs = m.Encoder.assemble(w, h, fmt, 8, data, max_u=mu, levels=2, cb=(4, 4))
        assert em.qcd_guard_bits(cs) == want == 2 + extra
        if want > 2:
            with pytest.raises(m.Htj2kError):                 # one guard bit fewer does not hold that block
                m.Encoder.assemble(w, h, fmt, 8, data, max_u=mu, levels=2, cb=(4, 4), guard_bits=want - 1)
            assert m.Encoder.assemble(w, h, fmt, 8, data, max_u=mu, levels=2, cb=(4, 4), guard_bits=want) == cs


def test_mct_off_and_mct_flag_in_cod():
    comps = synth("rgb24", 40, 24, 8)
    on = check_against_vecgen(comps, "rgb24", 40, 24, 8, 3, (5, 5), mct=True)
    off = check_against_vecgen(comps, "rgb24", 40, 24, 8, 3, (5, 5), mct=False)
    cod_on, cod_off = on[on.index(b"\xff\x52"):], off[off.index(b"\xff\x52"):]
    assert cod_on[8] == 1 and cod_off[8] == 0


def test_header_markers():
    comps = synth("yuv420p", 33, 17, 8)
    cs = assemble_from_model(comps, "yuv420p", 33, 17, 8, 2, (5, 5))
    assert cs[:2] == b"\xff\x4f" and cs[-2:] == b"\xff\xd9"
    siz = cs[2:]
    assert siz[:2] == b"\xff\x51" and int.from_bytes(siz[4:6], "big") == 0x4000
    cap = cs.index(b"\xff\x50")
    assert int.from_bytes(cs[cap + 4:cap + 8], "big") == 0x00020000
    sot = cs.index(b"\xff\x90")
    psot = int.from_bytes(cs[sot + 6:sot + 10], "big")
    assert sot + psot == len(cs) - 2


def test_all_zero_frame_leaves_every_block_out():
    comps = [np.full((20, 30), 128, np.int32)]
    cs = check_against_vecgen(comps, "gray", 30, 20, 8, 2, (4, 4))
    blocks = m.Encoder.layout(30, 20, "gray", 8, levels=2, cb=(4, 4))
    assert len(blocks) > 1


def test_layout_covers_each_plane_once():
    for fmt, (w, h), levels, cb in [("yuv420p", (101, 57), 3, (4, 5)), ("rgba", (64, 64), 5, (6, 6)),
                                    ("gray16le", (1, 300), 4, (2, 10))]:
        blocks = m.Encoder.layout(w, h, fmt, 12 if "16" in fmt else 8, levels=levels, cb=cb)
        dims = em.comp_dims(fmt, w, h)
        cover = [np.zeros((ch, cw), np.int32) for cw, ch in dims]
        for b in blocks:
            assert 0 < b["w"] <= 1 << cb[0] and 0 < b["h"] <= 1 << cb[1]
            cover[b["comp"]][b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]] += 1
        assert all((c == 1).all() for c in cover), fmt


def test_bound_and_errors():
    n = m.Encoder.bound(64, 48, "rgb24", 8)
    assert n > 64 * 48 * 3
    assert m.Encoder.bound(64, 48, "pal8", 8) == 0
    assert m.Encoder.bound(64, 48, "xyz12le", 12) == 0
    assert m.Encoder.bound(40000, 8, "gray", 8) == 0
    assert m.Encoder.bound(64, 48, "gray", 8, levels=33) == 0
    assert m.Encoder.bound(64, 48, "gray", 8, cb=(7, 6)) == 0
    assert m.Encoder.bound(64, 48, "gray", 8, cb=(1, 6)) == 0
    assert m.Encoder.bound(64, 48, "gray", 9) == 0
    assert m.Encoder.bound(64, 48, "yuv420p", 8, mct=1) == 0
    with pytest.raises(m.Htj2kError) as e:
        m.Encoder.layout(64, 48, "pal8", 8)
    assert e.value.code == -0x45574150           # PATCHWELCOME
    # too small an output buffer: a documented error and nothing past cap
    comps = synth("gray", 32, 32, 8)
    cs = assemble_from_model(comps, "gray", 32, 32, 8, 2, (5, 5))
    planes = em.coefficient_planes(comps, "gray", 8, 2, False)
    blocks = m.Encoder.layout(32, 32, "gray", 8, levels=2, cb=(5, 5))
    data = []
    for b in blocks:
        v = planes[0][b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]]
        d, lcup, _, _ = vecgen.encode_block(v) if v.any() else (b"", 0, 0, 0)
        data.append(d[:lcup])
    assert m.Encoder.assemble(32, 32, "gray", 8, data, levels=2, cb=(5, 5)) == cs
    with pytest.raises(m.Htj2kError) as e:
        m.Encoder.assemble(32, 32, "gray", 8, data, cap=len(cs) - 1, levels=2, cb=(5, 5))
    assert e.value.code == -28                   # ENOSPC
    # guard bits fixed below what the blocks need
    with pytest.raises(m.Htj2kError):
        m.Encoder.assemble(32, 32, "gray", 8, data, max_u=[40] * len(data), levels=2, cb=(5, 5), guard_bits=2)
    # the block count must be the layout's
    with pytest.raises(m.Htj2kError) as e:
        m.Encoder.assemble(32, 32, "gray", 8, data[:-1], levels=2, cb=(5, 5))
    assert e.value.code == -22                   # EINVAL
    with pytest.raises(m.Htj2kError) as e:
        m.Encoder.assemble(32, 32, "gray", 8, data + [b""], levels=2, cb=(5, 5))
    assert e.value.code == -22


def _ht_encode_blocks_no_device(rects, plane_w=1024, plane_h=1024):
    """htj2k_ht_encode_blocks checks its arguments before it needs a device context"""
    L = m.load_library()
    plane = np.zeros((plane_h, plane_w), np.int32)
    tab = (m.EncBlock * len(rects))()
    for i, (x, y, w, h) in enumerate(rects):
        tab[i].x, tab[i].y, tab[i].w, tab[i].h = x, y, w, h
    out = np.zeros(1 << 22, np.uint8)
    offs = (ctypes.c_size_t * (len(rects) + 1))()
    lc, mu = (ctypes.c_int * len(rects))(), (ctypes.c_int * len(rects))()
    return L.htj2k_ht_encode_blocks(None, plane.ctypes.data_as(ctypes.c_void_p), plane_w, plane_h, tab, len(rects),
                                    out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), offs, lc, mu)


def test_ht_encode_blocks_rejects_shapes_beyond_the_kernel():
    for rect in [(0, 0, 5, 819), (0, 0, 819, 5), (0, 0, 5, 818), (0, 0, 65, 63), (0, 0, 2048, 2), (0, 0, 0, 4)]:
        assert _ht_encode_blocks_no_device([rect]) == -22, rect          # EINVAL
    for rect in [(0, 0, 64, 64), (0, 0, 4, 1024), (0, 0, 1024, 4), (0, 0, 3, 1024), (0, 0, 3, 5), (960, 1020, 64, 4)]:
        assert _ht_encode_blocks_no_device([rect]) == -38, rect          # ENOSYS: valid, no context


def test_oracle_decodes_assembled_streams(orc):
    for fmt, bits, (w, h) in [("rgb24", 8, (37, 21)), ("yuv422p10le", 10, (30, 16)), ("gray16le", 12, (19, 33)),
                              ("yuva420p", 8, (21, 13))]:
        comps = synth(fmt, w, h, bits)
        cs = check_against_vecgen(comps, fmt, w, h, bits, 3, (5, 4))
        info, planes, _ = orc.decode(cs, req_pix_fmt=em.pix(fmt))
        want = em.to_planes(comps, fmt, bits)
        assert info.pix_fmt == em.pix(fmt) and len(planes) == len(want)
        for a, b in zip(planes, want):
            assert a.dtype == b.dtype and np.array_equal(a.reshape(-1), b.reshape(-1)), fmt
