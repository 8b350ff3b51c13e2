"""Region-of-interest (Maxshift, RGN) decoding on the GPU against the CPU oracle, bit for bit: the up-shift in
ht_dequant() (ht_kernels.hpp, shared by the HT kernels and k_mq_decode), the kernels a block with a shift takes (off
k_ht_refine's list, off the narrow MagSgn path) and the paths a job with such a block loses (16-bit sub-bands, two or
four blocks per wavefront), RGN in main and tile-part headers.  tests/test_roi_streams.py pins the inputs on the CPU:
what is lossless there is compared with the source here as well."""
import os
import struct

import numpy as np
import pytest

import cs_rewrite
import oracle
import roi_cases
import streams
import vecgen

pytestmark = pytest.mark.gpu

ROI_STREAMS = sorted(n for n in streams.CASES if "roi" in n)


@pytest.fixture(scope="module")
def dec():
    import ffmpeg_ht_amd as m
    d = m.Decoder()
    assert d.device_name().startswith("gfx950"), d.device_name()
    yield d
    d.close()


class _Table:
    """descriptor table + byte pool of unit blocks, each block once per dequantisation branch"""

    def __init__(self):
        self.descs, self.pool, self.expect, self.soff = [], b"", [], 0

    def _desc(self, b, branch, data_off):
        import ffmpeg_ht_amd as m
        d = m.BlockDesc()
        d.data_off, d.plane_off, d.w, d.h, d.stride = data_off, self.soff, b.w, b.h, b.w
        d.M_b, d.roi_shift, d.f_step, d.i_step = b.M_b, b.roi, branch[1], branch[2]
        self.descs.append(d)
        want = roi_cases.dequant(b.t1, b.M_b, branch)
        exact = b.vals if b.vals is not None and branch == roi_cases.BRANCHES[0] else None
        self.expect.append((self.soff, want, exact, (b.w, b.h, b.roi, b.M_b, branch)))
        self.soff += b.w * b.h
        return d

    def add_ht(self, b, branches):
        off = len(self.pool)
        self.pool += b.data + b"\0" * ((-len(b.data)) % 16)
        for br in branches:
            d = self._desc(b, br, off)
            d.lcup, d.lref, d.npasses, d.zbp, d.flags = b.lcup, b.lref, b.passes, b.zbp, (8 if b.causal else 0) | br[0]

    def add_mq(self, b, branches):
        off = len(self.pool)
        self.pool += oracle.mq_block_region(b.data, b.length, b.style, b.band, b.starts)
        for br in branches:
            d = self._desc(b, br, off)
            d.lcup, d.lref, d.npasses, d.zbp, d.flags = b.length, len(b.starts), b.npasses, b.K, 4 | br[0]

    def check(self, got, status, tag=""):
        assert not status.any(), tag
        got = got.view(np.uint32)
        for o, want, exact, what in self.expect:
            g = got[o:o + want.size].reshape(want.shape)
            assert np.array_equal(g, want), (tag, what)
            if exact is not None:
                assert np.array_equal(g.view(np.int32), exact), (tag, what)


def _each_unstuff_group(dec, tab):
    try:
        for g in ("1", "2", "4"):                            # blocks per wavefront of the un-stuffing kernel
            os.environ["HTJ2K_UNSTUFF_G"] = g
            got, status = dec.ht_blocks(tab.descs, tab.pool, tab.soff)
            tab.check(got, status, g)
    finally:
        os.environ.pop("HTJ2K_UNSTUFF_G", None)


def test_ht_unit_blocks_with_a_shift(dec):
    """one table of blocks with and without a shift, side by side: 11 shapes x 1, 2, 3 passes (vertically causal where
    the width is even) x shifts 3 to 14 (up to 30 bit-planes), each through dequantization_int (step 1 and another),
    dequantization_float and dequantization_int_97.  The blocks with a shift and SigProp / MagRef passes are not on
    k_ht_refine's list: k_ht_decode runs their passes itself, next to blocks that are on it.  Passes 1 and 3 with step 1
    give the source values back"""
    tab = _Table()
    for b in roi_cases.ht_blocks():
        tab.add_ht(b, roi_cases.BRANCHES)
    assert any(d.roi_shift == 0 and d.npasses > 1 for d in tab.descs) and any(d.roi_shift and d.npasses > 1 for d in tab.descs)
    _each_unstuff_group(dec, tab)


def test_ht_unit_blocks_with_a_shift_beyond_the_word(dec):
    """descriptors whose up-shift carries magnitude bits into bit 31 and past it: the reference shifts the 31-bit magnitude
    in a 32-bit word and ORs the saved sign in, so the carried bit is the sign from there on"""
    tab = _Table()
    for b in roi_cases.ht_hostile_blocks():
        tab.add_ht(b, roi_cases.BRANCHES)
    _each_unstuff_group(dec, tab)


def test_part1_unit_blocks_with_a_shift(dec):
    """decode_cblk + the up-shift + dequantisation: shifts 1, 7 and 12 on a 32 x 32, a 128 x 32 (two 64-column chunks) and
    a 5 x 3 block, no mode switch and all of them, blocks without shift in between; then the shifts beyond the word"""
    tab = _Table()
    for b in roi_cases.mq_blocks() + roi_cases.mq_hostile_blocks():
        assert b.ret == 1
        tab.add_mq(b, roi_cases.BRANCHES)
    got, status = dec.mq_blocks(tab.descs, tab.pool, tab.soff)
    tab.check(got, status)


def _frames(job, n):
    return [job.download_frame(f)[1] for f in range(n)]


def _same(planes, planes_o):
    return len(planes) == len(planes_o) and all(np.array_equal(a, b) for a, b in zip(planes, planes_o))


@pytest.mark.parametrize("name", ROI_STREAMS)
def test_roi_jobs_take_the_paths_for_them(dec, orc, name):
    """a job with a shifted block: 32-bit sub-bands, one block per wavefront, whatever the knobs say; same frames and
    error counts as the oracle with the one-kernel and the split HT decoder, ht_multi and coef16 on and off"""
    data, kw = streams.get(name)
    info_o, planes_o, _ = orc.decode(data, **kw)
    nerr = orc.block_errors()
    dec.set_int("bitexact", kw.get("bitexact", 0))
    try:
        for ht_mode, ht_multi, coef16 in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
            dec.set_int("ht_mode", ht_mode)
            dec.set_int("ht_multi", ht_multi)
            dec.set_int("coef16", coef16)
            job = dec.job().parse_batch([data, data]).upload().run().wait()
            assert job.coef16() == 0, name
            assert job.ht_blocks_per_wave() in (0, 1), name
            assert job.block_errors() == 2 * nerr, name
            for planes in _frames(job, 2):
                assert _same(planes, planes_o), (name, ht_mode, ht_multi, coef16)
            job.free()
    finally:
        for knob in ("ht_mode", "ht_multi", "coef16"):
            dec.set_int(knob, 1)
        dec.set_int("bitexact", 0)


def test_a_roi_frame_demotes_its_own_job_only(dec, orc):
    """8-bit RGB frames of fast geometry qualify for 16-bit sub-bands; the same picture with a region of interest does
    not, alone or between two of them, and the next job without it qualifies again"""
    img = vecgen.synth_image(256, 192, 3, seed=448, noise=10)
    plain = vecgen.encode(img, mct=1, nlevels=4)
    roi = vecgen.encode(img, mct=1, nlevels=4, roi_shift=12)
    source = np.stack(img, -1)
    for pkts, c16 in (([plain], 1), ([roi], 0), ([plain, roi, plain], 0), ([plain], 1)):
        job = dec.job().parse_batch(pkts).upload().run().wait()
        assert job.coef16() == c16, len(pkts)
        if not c16:
            assert job.ht_blocks_per_wave() == 1
        assert job.block_errors() == 0
        for pkt, planes in zip(pkts, _frames(job, len(pkts))):
            assert _same(planes, orc.decode(pkt)[1])
            assert np.array_equal(planes[0].reshape(192, 256, 3), source)      # Maxshift is lossless
        job.free()


def _decode_both(dec, orc, data):
    info_o, planes_o, consumed_o = orc.decode(data)
    info, planes, consumed, st = dec.decode(data)
    assert consumed == consumed_o and st.n_block_errors == orc.block_errors()
    assert _same(planes, planes_o)
    return planes


def test_rgn_in_tile_part_headers(dec, orc):
    """the RGN segments moved from the main header into every tile's first tile-part header: same frames; with another
    value left in the main header the tile's own wins (j2k_tier2.c: the main header's is the default of a tile that
    has none)"""
    img = streams._img(190, 131, 3, 8, 5)
    cs = vecgen.encode(img, roi_shift=12, mct=1, tile=(64, 64), nlevels=3, sop=True, eph=True, cap_extra_bits=0x0800)
    source = np.stack(img, -1)
    assert np.array_equal(_decode_both(dec, orc, cs)[0].reshape(source.shape), source)
    s = cs_rewrite.Stream(cs)
    rgn = [m for m in s.main if m[0] == cs_rewrite.RGN]
    assert len(rgn) == 3 and len(s.order) == 9
    in_tiles = {(isot, 0): rgn for isot in s.order}
    s.main = [m for m in s.main if m[0] != cs_rewrite.RGN]
    moved = s.build(extra_tile_hdr=in_tiles)
    assert moved != cs and len(moved) > len(cs)
    assert np.array_equal(_decode_both(dec, orc, moved)[0].reshape(source.shape), source)
    s.main += [(cs_rewrite.RGN, bytes([c, 0, 13])) for c in range(3)]
    assert np.array_equal(_decode_both(dec, orc, s.build(extra_tile_hdr=in_tiles))[0].reshape(source.shape), source)
    # ... and a tile without a segment of its own takes the main header's: the wrong one here, on both decoders alike
    del in_tiles[(s.order[4], 0)]
    assert not np.array_equal(_decode_both(dec, orc, s.build(extra_tile_hdr=in_tiles))[0].reshape(source.shape), source)


@pytest.mark.parametrize("part1", [False, True], ids=["ht", "part1"])
def test_rewritten_rgn_variants_decode(dec, orc, part1):
    """cs_rewrite's rgn_main / rgn_tile on a base that may carry them (Ccap15 bits 11 and 12): decoded, not refused"""
    img = streams._img(190, 131, 3, 8, 6)
    cs = vecgen.encode(img, sop=True, eph=True, mct=1, tile=(100, 70), nlevels=3, part1=part1, cap_extra_bits=0 if part1 else 0x1800)
    seen = []
    for vn, data in cs_rewrite.variants(cs, not part1):
        if vn.startswith("rgn_"):
            _decode_both(dec, orc, bytes(data))
            seen.append(vn)
    assert seen == ["rgn_main", "rgn_tile"]


def test_a_shift_on_another_component_than_the_first(dec, orc):
    """the reference counts every component's bit-planes with component 0's shift (jpeg2000dec.c:1194, restated in
    j2k_tier2.c): an HT stream with a shift on the second component only is refused, by both with the same code; the
    Part-1 streams decode with blocks short of, or beyond, their bit-planes, to the same frames and error counts"""
    import ffmpeg_ht_amd as m
    img = streams._img(190, 131, 3, 8, 5)
    data = vecgen.encode(img, roi_shift=[0, 12, 0])
    with pytest.raises(oracle.DecodeError) as eo:
        orc.decode(data)
    with pytest.raises(m.Htj2kError) as eg:
        dec.decode(data)
    assert eg.value.code == eo.value.code == -0x41444E49
    for shifts in ([12, 0, 0], [0, 12, 0]):
        data = vecgen.encode(img, roi_shift=shifts, part1=True)
        try:
            orc.decode(data)
        except oracle.DecodeError as e:
            with pytest.raises(m.Htj2kError) as eg:
                dec.decode(data)
            assert eg.value.code == e.code
        else:
            _decode_both(dec, orc, data)


def test_another_signalled_shift_is_another_picture(dec, orc):
    """SPrgn of one component changed in the main header: the picture changes, on both decoders alike"""
    data, _ = streams.get("roi_rgb_nomct_comp0")
    base = _decode_both(dec, orc, data)
    at = data.index(struct.pack(">HHBB", cs_rewrite.RGN, 5, 0, 0))
    other = data[:at + 6] + bytes([data[at + 6] - 1]) + data[at + 7:]
    assert not _same(_decode_both(dec, orc, other), base)
