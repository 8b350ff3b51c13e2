"""Transcoding on the GPU: Part-1 codestreams in, HTJ2K codestreams out that decode to the very same coefficients.
The raw stores of the Part-1 block kernel (htj2k_mq_blocks_raw), whole frames compared after the block stage and as
pixels on the product decoder and through the oracle, the planes and passes every block got against the block rule
(tests/xc_model.py), batches, rounds, device-resident output, the refusals, and the C example."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cs_rewrite
import ffmpeg_ht_amd as m
import oracle
import vecgen
import xc_model as xm
from xc_source import Source

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCHWELCOME, INVALIDDATA, ENOSPC, EINVAL = -0x45574150, -0x41444E49, -28, -22


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def enc():
    e = m.Encoder(device_id=0)
    yield e
    e.close()


# ---------------------------------------------------------------- 1. the raw stores of k_mq_decode
def test_mq_blocks_raw(dec):
    """the shapes, styles and dropped passes of the CPU test of the block rule: the plane htj2k_mq_blocks_raw writes is
    the oracle's sign-magnitude output converted to indices (xm.raw_index), with no difference allowed; beside it the
    dequantising entry still gives what it gave"""
    rng = np.random.default_rng(41)
    descs, pool, expect, soff = [], b"", [], 0
    for style in (0, 0x01, 0x04, 0x08):
        for (w, h) in [(1, 1), (3, 5), (4, 4), (17, 9), (64, 64)]:
            for d in range(8):
                band = int(rng.integers(0, 4))
                amp, density = [(3, 0.3), (200, 0.9), (40, 0.05)][d % 3]
                vals = rng.integers(-amp, amp + 1, (h, w)) * (rng.random((h, w)) < density)
                vals[0, 0] = amp
                seg, lens, passes, K, n = vecgen.encode_block_p1(vals, band=band, style=style, drop_passes=d)
                if n == 0:
                    continue
                M_b = K + 1 + d % 2
                data, length, starts = oracle.mq_block_layout(seg, lens, passes, style)
                ret, t1 = oracle.mq_decode_block(data, length, n, K, w, h, M_b, style, band, starts)
                assert ret == 1
                want53 = np.zeros((h, w), dtype=np.int32)
                oracle.lib().orc_dequant_int(t1.ctypes.data_as(ctypes.c_void_p), w, want53.ctypes.data_as(ctypes.c_void_p), w, w, h, M_b, 32768)
                e = m.BlockDesc()
                e.data_off, e.plane_off, e.lcup, e.lref, e.w, e.h, e.stride = len(pool), soff, length, len(starts), w, h, w
                # the transform bits and the steps are not read by the raw stores: 9/7 descriptors on every other block
                e.npasses, e.zbp, e.M_b, e.flags, e.roi_shift, e.f_step, e.i_step = n, K, M_b, 4 | (d % 2), 0, 0.37, 32768
                descs.append(e)
                pool += oracle.mq_block_region(data, length, style, band, starts)
                expect.append((soff, xm.raw_index(t1, M_b, K, n), want53, d % 2))
                soff += w * h
    got, status = dec.mq_blocks(descs, pool, soff, raw=True)
    assert not status.any()
    for o, want, _, _ in expect:
        assert np.array_equal(got[o:o + want.size].reshape(want.shape), want)
    # a block that fails part-way ("Missing needed termination") is reported by the raw entry as by the other
    vals = rng.integers(-50, 51, (32, 32))
    vals[0, 0] = 50
    seg, lens, passes, K, n = vecgen.encode_block_p1(vals, band=1, style=0x04)
    data, length, starts = oracle.mq_block_layout(seg, lens, passes, 0x04)
    starts = starts[:-3]
    ret, _ = oracle.mq_decode_block(data, length, n, K, 32, 32, K + 2, 0x04, 1, starts)
    assert ret < 0
    e = m.BlockDesc()
    e.data_off, e.plane_off, e.lcup, e.lref, e.w, e.h, e.stride = 0, 0, length, len(starts), 32, 32, 32
    e.npasses, e.zbp, e.M_b, e.flags, e.roi_shift, e.f_step, e.i_step = n, K, K + 2, 4 | 1, 0, 1.0, 32768
    _, st = dec.mq_blocks([e], oracle.mq_block_region(data, length, 0x04, 1, starts), 1024, raw=True)
    assert st[0] != 0
    got, status = dec.mq_blocks(descs, pool, soff)
    for o, _, want53, is53 in expect:
        if is53:
            assert np.array_equal(got[o:o + want53.size].reshape(want53.shape), want53)
    # a ROI shift or more than 31 magnitude bits: refused
    descs[0].roi_shift = 3
    with pytest.raises(m.Htj2kError) as err:
        dec.mq_blocks(descs[:1], pool, soff, raw=True)
    assert err.value.code == EINVAL


# ---------------------------------------------------------------- 2 - 4. whole frames
def yuv420(w, h, seed):
    return vecgen.synth_image(w, h, 3, seed=seed, dx=[1, 2, 2], dy=[1, 2, 2])


R97 = dict(part1=True, mct=1, nlevels=3, cb=(4, 4), transform=0, qstep=1 / 8)
CASES = {
    "gray_33x17": (lambda: vecgen.synth_image(33, 17, 1, seed=1), dict(part1=True, nlevels=2, cb=(2, 2), transform=1)),
    "rgb_64x48_53": (lambda: vecgen.synth_image(64, 48, 3, seed=2), dict(part1=True, mct=1, nlevels=3, cb=(4, 4), transform=1)),
    "rgb_64x48_97": (lambda: vecgen.synth_image(64, 48, 3, seed=2), R97),
    "yuv420p_50x38": (lambda: yuv420(50, 38, 3), dict(part1=True, nlevels=2, cb=(3, 3), dx=[1, 2, 2], dy=[1, 2, 2], width=50, height=38)),
    "gray16_40x24": (lambda: vecgen.synth_image(40, 24, 1, depth=16, seed=4), dict(part1=True, depth=16, nlevels=2, cb=(3, 3))),
    "rgb_70x50_tiles": (lambda: vecgen.synth_image(70, 50, 3, seed=5), dict(part1=True, mct=1, nlevels=2, cb=(3, 3), tile=(32, 32))),
    "style_bypass": (lambda: vecgen.synth_image(64, 48, 3, seed=2), dict(R97, cblk_style=0x01)),
    "style_termall": (lambda: vecgen.synth_image(64, 48, 3, seed=2), dict(R97, cblk_style=0x04, transform=1)),
    "one_sample": (lambda: [np.array([[201]], dtype=np.int32)], dict(part1=True, nlevels=0)),
    "levels_0": (lambda: vecgen.synth_image(37, 21, 1, seed=6), dict(part1=True, nlevels=0, cb=(3, 4))),
    "prog_precincts_sop": (lambda: vecgen.synth_image(70, 50, 3, seed=7), dict(part1=True, mct=1, nlevels=3, prog=2, prec=[(7, 7)], sop=True, eph=True)),
}
def mostly_flat():
    a = np.full((48, 64), 100, dtype=np.int32)
    a[:9, :11] = vecgen.synth_image(11, 9, 1, seed=8)[0]
    return [a]


CASES["mostly_flat"] = (mostly_flat, dict(part1=True, nlevels=2, cb=(3, 3)))      # most blocks have no passes at all
CASES.update({"drop_%d" % d: (lambda: vecgen.synth_image(64, 48, 3, seed=2), dict(R97, drop_passes=d)) for d in range(1, 6)})
CASES["drop_4_53"] = (lambda: vecgen.synth_image(64, 48, 3, seed=2), dict(R97, transform=1, drop_passes=4))
LOSSLESS = {"gray_33x17", "rgb_64x48_53", "yuv420p_50x38", "gray16_40x24", "rgb_70x50_tiles", "style_termall", "one_sample", "levels_0",
            "prog_precincts_sop", "mostly_flat"}


def block_stage_planes(dec, cs):
    job = dec.job().parse(cs).upload().run(1).wait()
    assert job.block_errors() == 0
    planes = [job.plane(t) for t in range(job.num_tilecomps())]
    job.free()
    return planes


def source_forms(orc, src, kw):
    """per block of the encoder's layout what the rule makes of the source: (plane, passes, left out), from the oracle's
    parse and block decode of the source (Source, tests/xc_source.py)"""
    return [f[:3] for f in Source(orc, src, kw).forms()]


@pytest.fixture(scope="module")
def transcoded(dec, enc):
    """every case's source and transcoded stream, made once (one call per case) and shared by the tests below"""
    out = {}
    for name, (img, kw) in CASES.items():
        src = vecgen.encode(img(), **kw)
        cs = enc.transcode(dec, [src])[0]
        out[name] = (src, cs, enc.last_planes(0), enc.last_passes(0), enc.transcode_stage_ms())
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_is_identical_on_the_product_decoder(dec, transcoded, name):
    """the planes after the block stage and the final pixels: 0 differing samples, 5/3 and 9/7 alike"""
    src, cs, _, _, ms = transcoded[name]
    info = dec.probe(cs)
    assert info.is_ht == 1 and dec.probe(src).is_ht == 0
    a, b = block_stage_planes(dec, src), block_stage_planes(dec, cs)
    assert len(a) == len(b)
    for t, (p, q) in enumerate(zip(a, b)):
        assert p.dtype == q.dtype and p.shape == q.shape
        assert np.count_nonzero(p.view(np.uint32) != q.view(np.uint32)) == 0, (name, t)
    ia, pa, _, sa = dec.decode(src)
    ib, pb, _, sb = dec.decode(cs)
    assert sa.n_block_errors == 0 == sb.n_block_errors
    assert (ia.width, ia.height, ia.pix_fmt, ia.bits_per_raw_sample) == (ib.width, ib.height, ib.pix_fmt, ib.bits_per_raw_sample)
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert len(ms) == 4 and all(v >= 0 for v in ms)


@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_is_identical_through_the_oracle(orc, transcoded, name):
    """the oracle's whole-frame decode of the transcoded stream equals its decode of the source; a lossless source also
    gives back the image"""
    src, cs, _, _, _ = transcoded[name]
    ia, pa, _ = orc.decode(src)
    ea = orc.block_errors()
    ib, pb, _ = orc.decode(cs)
    assert ea == 0 == orc.block_errors() and ib.is_ht == 1
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
    if name in LOSSLESS:
        img, kw = CASES[name]
        comps = img()
        shift = 16 - kw["depth"] if kw.get("depth", 8) > 8 and oracle.PIX_NAMES[ib.pix_fmt] in ("gray16le", "rgb48le") else 0
        if len(pb) == 1:
            got = pb[0].reshape(ib.height, ib.width, -1).astype(np.int64) >> shift
            assert np.array_equal(got, np.stack(comps, -1))
        else:
            assert all(np.array_equal(p, c) for p, c in zip(pb, comps))


@pytest.mark.parametrize("name", sorted(CASES))
def test_planes_and_passes_follow_the_rule(orc, transcoded, name):
    src, cs, planes, passes, _ = transcoded[name]
    img, kw = CASES[name]
    forms = source_forms(orc, src, kw)
    assert len(forms) == len(planes) == len(passes)
    for i, (p, k, left_out) in enumerate(forms):
        assert (planes[i], passes[i]) == (p, k), (name, i)
    # and the output's own plan says the same: passes, and the zero bit-planes of the cleanup pass
    out = {(int(e["tcomp"]), int(e["plane_off"])): e for e in orc.plan_blocks(cs)}
    coded = [e for e in out.values() if e["npasses"]]
    assert len(coded) == sum(1 for f in forms if not f[2])
    assert sorted(int(e["npasses"]) for e in coded) == sorted(k for _, k, lo in forms if not lo)
    if name.startswith("drop_"):                           # the sources cut after d passes end on every kind of pass
        want = {1: {3}, 2: {2}, 3: {1}, 4: {3}, 5: {2}}[int(name[5])]
        assert want <= {k for _, k, lo in forms if not lo} | {1}, name


# ---------------------------------------------------------------- 5. batches and limits
def small_sources():
    return [vecgen.encode(vecgen.synth_image(w, h, 1, seed=s), part1=True, nlevels=2, cb=(3, 3), transform=t, qstep=1 / 4, drop_passes=d)
            for w, h, s, t, d in ((33, 17, 1, 1, 0), (24, 20, 2, 0, 2), (50, 9, 3, 1, 1))]


def test_batch_of_different_sizes_and_components(dec, enc):
    srcs = small_sources() + [vecgen.encode(vecgen.synth_image(31, 30, 3, seed=9), part1=True, mct=1, nlevels=1, cb=(3, 3))]
    outs = enc.transcode(dec, srcs)
    assert len(outs) == 4
    singles = [enc.transcode(dec, [s])[0] for s in srcs]
    assert outs == singles
    for s, o in zip(srcs, outs):
        assert all(np.array_equal(a, b) for a, b in zip(dec.decode(s)[1], dec.decode(o)[1]))


def test_rounds(dec, enc):
    """eight 24 x 20 frames with room for three in a round: three rounds, the same bytes as one round"""
    srcs = [vecgen.encode(vecgen.synth_image(24, 20, 1, seed=20 + i), part1=True, nlevels=2, cb=(3, 3), drop_passes=i % 3) for i in range(8)]
    want = enc.transcode(dec, srcs)
    old = os.environ.get("HTJ2K_ENC_ROUND")
    os.environ["HTJ2K_ENC_ROUND"] = str(3 * 24 * 20)
    try:
        small = m.Encoder(device_id=0)
    finally:
        if old is None:
            del os.environ["HTJ2K_ENC_ROUND"]
        else:
            os.environ["HTJ2K_ENC_ROUND"] = old
    try:
        got = small.transcode(dec, srcs)
        assert small.last_rounds() == 3 and enc.last_rounds() == 1
        assert [small.last_planes(i) for i in range(8)] == [enc.last_planes(i) for i in range(8)]
    finally:
        small.close()
    assert got == want


def test_output_on_the_device(dec, enc):
    srcs = small_sources()
    assert enc.transcode(dec, srcs, out_on_device=True) == enc.transcode(dec, srcs)


def test_enospc_leaves_the_buffer_untouched(dec, enc):
    srcs = small_sources()
    outs = enc.transcode(dec, srcs)
    total = sum(len(o) for o in outs)
    assert total <= sum(m.Encoder.transcode_check(s) for s in srcs)        # the bound is honoured
    assert enc.transcode(dec, srcs, cap=total) == outs
    with pytest.raises(m.Htj2kError) as err:
        enc.transcode(dec, srcs, cap=total - 1)
    assert err.value.code == ENOSPC and not enc.last_out.any()


def test_a_batch_with_an_ht_frame_is_refused_whole(dec, enc):
    srcs = small_sources()
    srcs[1] = vecgen.encode(vecgen.synth_image(24, 20, 1, seed=2), nlevels=2, cb=(3, 3))
    with pytest.raises(m.Htj2kError) as err:
        enc.transcode(dec, srcs)
    assert err.value.code == PATCHWELCOME and "HT code-blocks already" in str(err.value) and not enc.last_out.any()


def test_reduction_factor_and_other_device_arguments(dec, enc):
    low = m.Decoder(device_id=0, reduction_factor=1)
    try:
        with pytest.raises(m.Htj2kError) as err:
            enc.transcode(low, small_sources()[:1], cap=100000)
        assert err.value.code == PATCHWELCOME
    finally:
        low.close()
    assert enc.L.htj2k_transcode_batch(None, enc.h, None, None, 1, None, ctypes.c_size_t(0), 0, None) == EINVAL


def test_damaged_source_is_an_error(dec, enc, orc):
    """a code-block body cut short (tests/cs_rewrite.py: the last packet's body loses bytes, Psot follows).  In a Part-1
    stream the lengths in the packet header then point past the tile-part, which the parser refuses for the whole frame
    before any block is decoded: HTJ2K_ERR_INVALIDDATA for the call and nothing written.  (decode_cblk's own two errors,
    too many passes for the bit-planes and a missing termination, cannot be produced by cutting bytes; the first is also
    caught by the rule, the second by the count of failed blocks, htj2k_mq_blocks' status.)"""
    cs = vecgen.encode(vecgen.synth_image(33, 17, 1, seed=1), part1=True, nlevels=2, cb=(2, 2), sop=True, eph=True, cblk_style=0x04)
    s = cs_rewrite.Stream(cs)
    sop, hdr, body = s.tiles[0]["packets"][-1]
    assert len(body) > 8
    s.tiles[0]["packets"][-1] = (sop, hdr, body[:-8])
    bad = s.build()
    with pytest.raises(oracle.DecodeError):
        orc.decode(bad)
    good = enc.transcode(dec, [cs])
    with pytest.raises(m.Htj2kError) as err:
        enc.transcode(dec, [cs, bad], cap=4 * len(good[0]) + 100000)
    assert err.value.code == INVALIDDATA and not enc.last_out.any()
    assert "left in the tile-part" in str(err.value)              # the parser's reason reaches the encoder's log


def test_decoder_opened_with_a_pixel_format_request(enc, dec):
    """the sources are parsed without the request: the same bytes, and transcode_check's bound holds"""
    src = small_sources()[0]
    asked = m.Decoder(device_id=0, req_pix_fmt=m.PIX_NAMES.index("rgb24"))
    try:
        assert enc.transcode(asked, [src]) == enc.transcode(dec, [src])
    finally:
        asked.close()


# ---------------------------------------------------------------- 6. the example
def test_example_program(tmp_path):
    exe = os.path.join(ROOT, "examples", "htj2k_transcode")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", ROOT, "examples/htj2k_transcode"])
    src = tmp_path / "in.j2c"
    src.write_bytes(vecgen.encode(vecgen.synth_image(64, 48, 3, seed=2), **dict(R97, drop_passes=2)))
    out = subprocess.run([exe, str(src), str(tmp_path / "out.jph")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "frames identical" in out.stdout, out.stdout + out.stderr
    assert (tmp_path / "out.jph").read_bytes()[:2] == b"\xff\x4f"
