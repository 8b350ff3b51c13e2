"""Region of interest (Maxshift, RGN segments) on the CPU: the vector factory's Maxshift option and the oracle are pinned
here before tests/test_roi_gpu.py trusts them on the GPU.
 * lossless round trip of the reversible ROI streams of the catalogue (the oracle, and OpenJPEG for the Part-1 ones)
 * the RGN segment matters: without it, or with another value in it, the stream is refused or decodes differently
 * the factory refuses what is no Maxshift stream; RGN without Ccap15 bit 12 is refused by both parsers
 * unit blocks: encode_block on where(region, v << s, v), the oracle's block decoder with roi_shift = s and
   dequantization_int give v back; hostile descriptors really carry magnitude bits into bit 31
3-pass HT streams and 9/7 streams are not lossless with or without a shift (the catalogue's gray_3passes is 1 off too):
for them, as for the hostile streams, the oracle is the reference and the GPU tests ask for parity with it."""
import shutil
import struct

import numpy as np
import pytest

import cs_rewrite
import enc_opj
import oracle
import roi_cases
import streams
import vecgen
from test_plan_equality import plan_diff                    # noqa: F401  (fixture: the product's host parser next to the oracle's)

# name -> (streams._img arguments, depth)
LOSSLESS = {
    "roi_gray": ((200, 150, 1, 8, 3), 8), "roi_gray_l3_cb256x16": ((300, 90, 1, 8, 13), 8),
    "roi_rgb_mct_cb32": ((190, 131, 3, 8, 5), 8), "roi_rgb_tiles": ((190, 131, 3, 8, 5), 8),
    "roi_gray12": ((160, 120, 1, 12, 7, 40), 12), "p1_roi_gray": ((200, 150, 1, 8, 3), 8),
    "p1_roi_rgb_mct": ((190, 131, 3, 8, 5), 8), "roi_mixed_gray": ((200, 150, 1, 8, 3), 8),
    "roi_rgb_nomct_comp0": ((190, 131, 3, 8, 5), 8),
}


def _pixels(info, planes, depth):
    fmt = oracle.PIX_NAMES[info.pix_fmt]
    shift = 16 - depth if fmt in ("rgb48le", "gray16le") else 0     # write_frame's << (precision - cbps)
    return planes[0].reshape(info.height, info.width, -1).astype(np.int64) >> shift


def _main_header(cs):
    """[(offset, code, payload length)] of the main header's segments"""
    pos, out = 2, []
    while True:
        code, ln = struct.unpack_from(">HH", cs, pos)
        if code == cs_rewrite.SOT:
            return out
        out.append((pos, code, ln - 2))
        pos += 2 + ln


def _without_rgn(cs):
    """the main header's RGN segments cut out (Psot counts a tile-part's own bytes: nothing else moves)"""
    out, last = b"", 0
    for pos, code, n in _main_header(cs):
        if code == cs_rewrite.RGN:
            out += cs[last:pos]
            last = pos + 4 + n
    assert last
    return out + cs[last:]


def _with_sprgn(cs, f):
    cs = bytearray(cs)
    for pos, code, n in _main_header(cs):
        if code == cs_rewrite.RGN:
            cs[pos + 4 + n - 1] = f(cs[pos + 4 + n - 1])
    return bytes(cs)


def test_every_roi_stream_carries_rgn_and_the_capability_bit():
    names = [n for n in streams.CASES if "roi" in n]
    assert len(names) >= 16
    for n in names:
        cs, _ = streams.get(n)
        hdr = _main_header(cs)
        assert any(code == cs_rewrite.RGN for _, code, _ in hdr), n
        cap = [pos for pos, code, _ in hdr if code == 0xFF50]
        assert bool(cap) == (not n.startswith("p1_")), n
        if cap:
            assert struct.unpack_from(">H", cs, cap[0] + 8)[0] & 0x1000, n


@pytest.mark.parametrize("name", sorted(LOSSLESS))
def test_lossless_round_trip(orc, name):
    args, depth = LOSSLESS[name]
    data, kw = streams.get(name)
    info, planes, _ = orc.decode(data, **kw)
    assert orc.block_errors() == 0
    assert np.array_equal(_pixels(info, planes, depth), np.stack(streams._img(*args), -1))


@pytest.mark.skipif(not enc_opj.HAVE_OPJ, reason="Pillow has no JPEG 2000")
@pytest.mark.parametrize("name", ["p1_roi_gray", "p1_roi_rgb_mct"])
def test_openjpeg_decodes_the_part1_roi_streams_to_the_source(name):
    """OpenJPEG refuses HT streams with RGN and MIXED streams: the Part-1 ones are the third opinion"""
    args, depth = LOSSLESS[name]
    img = streams._img(*args)
    got = enc_opj.pixels(streams.get(name)[0], "gray" if len(img) == 1 else "rgb24")
    assert np.array_equal(got, np.stack(img, -1)[:, :, 0] if len(img) == 1 else np.stack(img, -1))


@pytest.mark.parametrize("name", sorted(LOSSLESS))
def test_the_rgn_segment_is_what_decodes_them(orc, name):
    """without RGN the zero-bit-plane counts are out of range for the band (both parsers compute nonzerobits with the
    shift) or the picture differs; with SPrgn one less every background sample comes out at half its value"""
    data, kw = streams.get(name)
    _, want, _ = orc.decode(data, **kw)
    try:
        _, got, _ = orc.decode(_without_rgn(data), **kw)
    except oracle.DecodeError as e:
        assert e.code == -0x41444E49
    else:
        assert not np.array_equal(got[0], want[0])
    _, got, _ = orc.decode(_with_sprgn(data, lambda v: v - 1), **kw)
    assert not np.array_equal(got[0], want[0])


def test_factory_refusals():
    img = streams._img(200, 150, 1, 8, 3)
    with pytest.raises(RuntimeError, match="failed: -6$"):      # coefficients of 8-bit pictures reach 2^3: no Maxshift stream
        vecgen.encode(img, roi_shift=3)
    with pytest.raises(RuntimeError, match="failed: -7$"):      # M_b = 9 .. 11 here
        vecgen.encode(img, roi_shift=20)
    with pytest.raises(RuntimeError, match="failed: -7$"):      # 12 bits: M_b up to 15, and 15 + 16 > 30
        vecgen.encode(streams._img(160, 120, 1, 12, 7, 40), depth=12, nlevels=4, roi_shift=16)
    with pytest.raises(RuntimeError, match="failed: -7$"):
        vecgen.encode(streams._img(190, 131, 3, 8, 5), roi_shift=[0, 0, 21])
    vecgen.encode(img, roi_shift=19)                            # 11 + 19 = 30 planes is the most
    # shifts of zero leave the stream as it was, whatever the other two say
    assert vecgen.encode(img, roi_shift=0, roi_seed=5, rgn_value_bias=2) == vecgen.encode(img)
    assert vecgen.encode(img, roi_shift=12, roi_seed=1) != vecgen.encode(img, roi_shift=12)


def test_callers_built_before_the_maxshift_fields_get_the_streams_of_before():
    """htj2k_encode() takes the parameter block that ended with `mixed` and reads nothing behind it (bindings of before
    allocate no more); htj2k_encode_sized() reads what its caller says it has"""
    import ctypes
    img = [np.ascontiguousarray(c, dtype=np.int32) for c in streams._img(190, 131, 3, 8, 5)]
    want = vecgen.encode(img, mct=1, nlevels=3)
    end = vecgen.EncParams.roi_shift.offset
    size = ctypes.sizeof(vecgen.EncParams)                                 # (the binding's block, with every field appended since)
    room = (ctypes.c_uint8 * size)(*([0xA5] * size))                       # what lies behind the old block is not zero
    assert size >= end + 24
    p = vecgen.EncParams.from_buffer(room)
    ctypes.memset(room, 0, end)
    p.width, p.height, p.ncomp, p.nlevels, p.cb_w_log2, p.cb_h_log2, p.transform, p.mct, p.passes = 190, 131, 3, 3, 6, 6, 1, 1, 1
    p.qstep = 1.0 / 32
    for i in range(3):
        p.depth[i], p.dx[i], p.dy[i] = 8, 1, 1
    assert p.roi_shift[0] == 0xA5A5A5A5 - (1 << 32) and p.rgn_value_bias != 0
    ptrs = (ctypes.POINTER(ctypes.c_int32) * 4)(*[a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) for a in img])
    L = vecgen.lib()
    for call in (lambda o, n: L.htj2k_encode(ctypes.byref(p), ptrs, ctypes.byref(o), ctypes.byref(n)),
                 lambda o, n: L.htj2k_encode_sized(ctypes.byref(p), ctypes.c_size_t(end), ptrs, ctypes.byref(o), ctypes.byref(n))):
        out, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
        assert call(out, n) == 0
        got = ctypes.string_at(out, n.value)
        L.htj2k_enc_free(out)
        assert got == want


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_parsers_agree_on_what_they_refuse(orc, plan_diff, tmp_path):
    """RGN in an HT stream of the RGNFREE set (Ccap15 bit 12 clear): refused.  A shift on another component than the
    first: every block's nonzerobits is computed with component 0's shift (jpeg2000dec.c:1194), which is out of range
    in an HT stream and too small by the shift in a Part-1 one: refused, or decoded with rejected blocks.  The
    product's parser returns what the oracle's returns, on the streams and on damaged copies"""
    data = bytearray(streams.get("roi_gray")[0])
    cap = [pos for pos, code, _ in _main_header(data) if code == 0xFF50][0]
    data[cap + 8] &= ~0x10
    with pytest.raises(oracle.DecodeError) as e:
        orc.decode(bytes(data))
    assert e.value.code == -0x41444E49
    img = streams._img(190, 131, 3, 8, 5)
    second = vecgen.encode(img, roi_shift=[0, 12, 0])
    with pytest.raises(oracle.DecodeError) as e:
        orc.decode(second)
    assert e.value.code == -0x41444E49
    files = []
    for name, cs in (("rgnfree", bytes(data)), ("second", second)):
        files.append(tmp_path / (name + ".j2c"))
        files[-1].write_bytes(cs)
    # each parsed eight ways, same codes from both parsers: only the headers of the second stream are accepted (its
    # packets are what is refused)
    assert plan_diff(files, 0) == (16, 1)
    for name, kw in (("p1_first", dict(roi_shift=[12, 0, 0], part1=True)), ("p1_second", dict(roi_shift=[0, 12, 0], part1=True))):
        files.append(tmp_path / (name + ".j2c"))
        files[-1].write_bytes(vecgen.encode(img, **kw))
    plan_diff(files, 40)


def test_unit_blocks_give_the_source_values_back():
    """HT: passes 1 and 3 are exact (2 is lossy by construction, with or without a shift).  Part-1: every pass coded"""
    seen = set()
    for b in roi_cases.ht_blocks():
        if b.vals is None:
            continue
        got = roi_cases.dequant(b.t1, b.M_b, roi_cases.BRANCHES[0]).view(np.int32)
        assert np.array_equal(got, b.vals), (b.w, b.h, b.passes, b.roi, b.planes)
        seen.add((b.roi, b.planes))
    assert (14, 30) in seen and any(r == 0 for r, _ in seen)
    for b in roi_cases.mq_blocks():
        assert b.ret == 1
        got = roi_cases.dequant(b.t1, b.M_b, roi_cases.BRANCHES[0]).view(np.int32)
        assert np.array_equal(got, b.vals), (b.w, b.h, b.style, b.roi)


def test_hostile_descriptors_overflow_the_word():
    """at least a quarter of a block's samples get a magnitude bit shifted into bit 31, and some of them were positive:
    the word the reference dequantises has a sign that the up-shift made.  Without this the GPU test of the same
    descriptors could pass on input that never overflows"""
    for b in roi_cases.ht_hostile_blocks() + roi_cases.mq_hostile_blocks():
        un = b.unshifted().view(np.uint32)
        assert roi_cases.carried_into_sign(un, b.M_b, b.roi) >= 0.25, (b.w, b.h, b.roi)
        assert ((un >> 31 == 0) & (b.t1.view(np.uint32) >> 31 == 1)).any()
