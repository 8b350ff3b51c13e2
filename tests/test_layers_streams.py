"""Quality layers from the vector factory (streams.LAYERS), pinned on the CPU.  A block's bytes arrive spread over several
packets: first inclusion against the layer index, Lblock and the pass count carried from packet to packet, HT placeholder
passes in one layer and the cleanup segment in a later one, SigProp and MagRef later still, a BYPASS pattern entered in
the middle of a segment, the 0xFF 0xFF trailers of terminated segments per contribution, the layer axis of the five packet
orders, and a gather table in which blocks have second and later pieces at any alignment.
 * every stream decodes to exactly the frame of its one-layer twin (the coefficients are the same, so the arithmetic is the
   same, 9/7 included); the lossless ones to the source picture
 * with layers=1 the factory writes what it wrote before it knew layers: every stream of the catalogue is its own twin
 * Pillow's OpenJPEG reader, where present, decodes the lossless Part-1 cases to the source: the factory's layer syntax
   pinned to a third party.  OpenJPEG reads neither HT nor MIXED streams: for those the oracle's restatement of the
   reference and the round trip are the only references
 * both parsers agree on every case and on seeded byte mutations of it (tests/native/plan_diff.c)
 * the streams really are layered: conditions on the inputs, read from the factory's own counters (vecgen.LAYER_STATS) and
   from the product parser's gather table (plan_diff -S)
 * container variants of three layered bases (tests/cs_rewrite.py), poc_layers among them, decode to the base frame; the PLT
   ones take the sequential packet reader also with packet threads on
tests/test_layers_gpu.py takes the same streams through the device routes."""
import hashlib
import io
import json
import os

import numpy as np
import pytest

import cs_rewrite
import streams
import vecgen
from test_plan_equality import plan_diff  # noqa: F401  (fixture)

try:
    from PIL import Image, features
    HAVE_OPJ = bool(features.check("jpg_2000"))
except Exception:  # pragma: no cover
    HAVE_OPJ = False

NAMES = sorted(streams.LAYERS)


def _kw(name):
    return streams.LAYERS[name][1]


def _lossless(name):
    return _kw(name).get("transform", 1) == 1 and not streams.LAYERS[name][2]


def _stored_shift(name):
    """gray of 8 or 16 bits and rgb24 come back as stored; gray12 comes back in the upper bits of gray16"""
    depth = _kw(name).get("depth", 8)
    return 16 - depth if 8 < depth < 16 else 0


# the group "HT, one pass": a block is one cleanup segment, cuts fall between passes, so it travels in one packet whatever
# the seed.  Every other case has blocks of several passes and must spread them
ONE_PASS = ("lay2_gray", "lay3_gray_cb32", "lay7_rgb_mct", "lay40_gray")


def _passes_per_block(name):
    """more than one coding pass per block: every case but the four of one HT pass and the picture without blocks"""
    kw = _kw(name)
    several = bool(kw.get("part1") or kw.get("mixed") or kw.get("passes", 1) > 1 or kw.get("placeholder_sets"))
    assert several == (name not in ONE_PASS + ("lay2_all_zero",)), name
    return several


@pytest.fixture(scope="module")
def stats():
    """name -> the factory's layer counters of the stream"""
    out = {}
    for n in NAMES:
        out[n] = {}
        streams.layers_encode(n, stats=out[n])
    return out


def test_the_catalogue_is_enrolled():
    assert len(NAMES) >= 39 and all(n in streams.CASES for n in NAMES)
    assert all(_kw(n)["layers"] >= 2 for n in NAMES)
    for n in NAMES:
        img = streams.layers_image(n)
        assert img[0].shape[1] <= 300 and img[0].shape[0] <= 150, n
    kws = [_kw(n) for n in NAMES]
    assert {kw.get("prog", 0) for kw in kws if kw.get("prec")} == {0, 1, 2, 3, 4}
    assert {kw["cblk_style"] for kw in kws if kw.get("part1") and "cblk_style" in kw} >= {0x01, 0x02, 0x04, 0x05, 0x20, 0x2F}
    assert sum(bool(kw.get("mixed")) for kw in kws) >= 2 and any(kw.get("placeholder_sets") for kw in kws)
    assert any(kw.get("tile") for kw in kws) and any(kw.get("comp") for kw in kws) and any(kw.get("roi_shift") for kw in kws)


def test_one_layer_is_what_the_factory_wrote_before():
    """every stream of the catalogue as it was before the factory knew layers (tests/golden/catalogue_sha256.json: SHA-256
    of the 173 streams, written by the factory of that time) comes out byte for byte the same; layers=1 (and any seed) is
    the stream without the keyword, and the twin of a layered case is the case without its layers"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "catalogue_sha256.json")) as f:
        before = json.load(f)
    assert len(before) == 173 and set(before) <= set(streams.CASES) and not set(before) & set(streams.LAYERS)
    for n, digest in before.items():
        assert hashlib.sha256(streams.get(n)[0]).hexdigest() == digest, n
    for n, (args, kw) in {"gray": ((200, 150, 1, 8, 3), {}), "p1_bypass": ((200, 150, 1, 12, 3, 60), dict(depth=12, part1=True, cblk_style=1)),
                          "mixed_3p": ((200, 150, 1, 8, 3), dict(mixed=True, passes=3)),
                          "rpcl": ((190, 131, 3, 8, 5), dict(mct=1, prog=2, prec=[(7, 7), (6, 6)], nlevels=3, placeholder_sets=1))}.items():
        img = streams._img(*args)
        assert vecgen.encode(img, **kw) == vecgen.encode(img, layers=1, layer_seed=77, **kw), n
    for n in NAMES:
        kw = {k: v for k, v in _kw(n).items() if k not in ("layers", "layer_seed")}
        src = streams.LAYERS[n][0]
        if isinstance(src, str) and src in streams.DEPTHS:
            assert streams.layers_twin(n) == streams.depths_encode(src, **kw), n
        else:
            assert streams.layers_twin(n) == vecgen.encode(streams.layers_image(n), **kw), n


@pytest.mark.parametrize("name", NAMES)
def test_decodes_to_the_frame_of_its_one_layer_twin(orc, name):
    dkw = streams.LAYERS[name][2]
    data, twin = streams.layers_encode(name), streams.layers_twin(name)
    assert data != twin
    info, planes, consumed = orc.decode(data, **dkw)
    assert orc.block_errors() == 0 and consumed > 0
    got = [p.copy() for p in planes]
    info_t, planes_t, _ = orc.decode(twin, **dkw)
    assert orc.block_errors() == 0 and bytes(info) == bytes(info_t)
    assert len(got) == len(planes_t) and all(np.array_equal(a, b) for a, b in zip(got, planes_t)), name
    src = streams.LAYERS[name][0]
    if _lossless(name) and _kw(name).get("passes", 1) == 1 and not isinstance(src, str) and not _kw(name).get("dx"):
        # (HT blocks with refinement passes are coded from bit-plane 1 down and come back with the decoder's half-bin offsets;
        # their twin is the reference for those -- the unequal-depth case and the 4:2:0 case are such streams, so no
        # comparison per component is left out here: every lossless case of one pass is packed gray or rgb)
        img = streams.layers_image(name)
        a = got[0].reshape(info.height, info.width, -1).astype(np.int64)
        for c in range(len(img)):
            assert np.array_equal(a[..., c], img[c].astype(np.int64) << _stored_shift(name)), (name, c)


OPJ_NAMES = [n for n in NAMES if _kw(n).get("part1") and _lossless(n)]


@pytest.mark.skipif(not HAVE_OPJ, reason="Pillow without OpenJPEG")
@pytest.mark.parametrize("name", OPJ_NAMES)
def test_openjpeg_decodes_the_part1_cases_to_the_source(name):
    """a third party reads the layers the factory writes: OpenJPEG (through Pillow) returns the source picture of every
    lossless Part-1 case, the Maxshift one included.  It reads neither HT nor MIXED streams: those rest on the oracle's
    restatement and the round trip alone"""
    assert len(OPJ_NAMES) >= 10
    img = streams.layers_image(name)
    im = Image.open(io.BytesIO(streams.layers_encode(name)))
    im.load()
    a = np.array(im).astype(np.int64)
    want = np.stack([c.astype(np.int64) for c in img], axis=-1)
    assert np.array_equal(a.reshape(want.shape), want << _stored_shift(name)), name


def test_both_parsers_agree(plan_diff, tmp_path):
    """return code and plan (block table with Lcup / Lref / pass counts, byte pool, the pool rebuilt from the gather table)
    of every case and of 60 damaged copies of each, and of the streams whose layer count does not fit the 8 bits both
    parsers keep it in, as the reference does"""
    files = []
    for n in NAMES:
        files.append(tmp_path / (n + ".j2c"))
        files[-1].write_bytes(streams.layers_encode(n))
    for n, (args, kw) in streams.LAYERS_WRAP.items():
        files.append(tmp_path / (n + ".j2c"))
        files[-1].write_bytes(vecgen.encode(streams._img(*args), **kw))
    parses, accepted = plan_diff(files, 60)
    assert parses >= 68 * len(files) and accepted > parses // 3


def test_the_streams_really_are_layered(stats, plan_diff, tmp_path):
    """Conditions on the inputs, not on the decoder.  Per case, from the factory's counters: some block is first included
    in a layer > 0, some packet is empty, and at least a quarter of the included blocks have contributions in two or more
    packets -- that one for every case but the four of the group "HT, one pass" (ONE_PASS), and again from the product
    parser's gather table, as blocks whose pieces are not all back to back in the codestream.  The all-zero picture has
    no included block at all; its packets are all empty.  (First inclusion in a later layer, empty packets and where a
    BYPASS contribution begins cannot be read off a plan, which has no packets in it: those are the factory's figures, of
    a factory that the twin comparison, the two parsers and OpenJPEG hold to its word.)
    Over the catalogue, from the product parser's gather table: every (dst & 3, src & 3) among the second and later pieces
    of a block, every piece length 0 .. 7, HT blocks whose Dref comes from another packet than Dcup; and from the factory:
    every way of spreading HT passes, BYPASS contributions that begin inside the ten-pass segment and inside a raw pair,
    blocks that skip a layer and resume, the one-bit 'not included'."""
    total = {}
    for n in NAMES:
        st = stats[n]
        print(n, {k: v for k, v in st.items() if v})
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
        assert st["packets"] > 0 and st["empty_packets"] > 0, (n, st)
        if n == "lay2_all_zero":
            assert st["blocks"] == 0 and st["empty_packets"] == st["packets"]
            continue
        assert st["blocks"] > 0 and 0 < st["first_later"] < st["blocks"], (n, st)
        if _passes_per_block(n):
            assert 4 * st["multi_packet"] >= st["blocks"], (n, st)
    print("catalogue", total)
    for k in vecgen.LAYER_STATS:
        assert total[k] > 0, (k, total)
    assert stats["lay4_placeholder_2_3p"]["ht_placeholders_alone"] > 0
    assert stats["p1_lay3_bypass"]["bypass_in_ten"] > 0 and stats["p1_lay3_bypass"]["bypass_in_raw_pair"] > 0
    files = []
    for n in NAMES:
        files.append(tmp_path / (n + ".j2c"))
        files[-1].write_bytes(streams.layers_encode(n))
    table = plan_diff(files, 0, stats=True)
    assert len(table) == len(files)
    align = lens = split = 0
    for n, f in zip(NAMES, files):
        t = table[str(f)]
        print(n, t)
        align |= t["align"]
        lens |= t["lens"]
        split += t["ht_split"]
        # the parser's blocks with bytes are the factory's included blocks.  multi: blocks whose pieces are not all back to
        # back in the codestream, which is bytes from two or more packets (several pieces of one packet, as behind every
        # terminated segment, lie back to back); a contribution of 0 bytes leaves no piece, so the factory may count more
        assert t["blocks"] == stats[n]["blocks"] and t["multi"] <= stats[n]["multi_packet"], (n, t, stats[n])
        if _passes_per_block(n):
            assert 4 * t["multi"] >= t["blocks"], (n, t)
    assert align == 0xFFFF, hex(align)
    assert lens == 0xFF, hex(lens)
    assert split > 0


# ---- container variants of layered streams
REWRITE_BASES = {
    "lay3_ht_rpcl":     ((190, 131, 3, 8, 5), dict(layers=3, layer_seed=51, mct=1, prog=2, prec=[(7, 7), (6, 6)], nlevels=3, passes=3)),
    "lay3_p1_termall_tiles": ((190, 131, 3, 8, 6), dict(layers=3, layer_seed=52, part1=True, cblk_style=0x05, tile=(64, 64), nlevels=3)),
    "lay4_mixed":       ((190, 131, 3, 8, 5), dict(layers=4, layer_seed=53, mct=1, mixed=True, cb=(5, 5), nlevels=3, passes=3)),
}
VARIANTS = ("plt", "tp3_tlm_plt", "tp_each_packet", "tp3_interleaved", "ppm", "ppm_tp3", "ppt", "ppt_tp3", "poc_layers")
# PPM over several tile-parts: the reference takes the first packet header of a tile-part from the body of the next one
# (j2k_tier2.c: header_stream), so the frame is not the base's; both parsers do the same, which is what is asked of it
SAME_FRAME = tuple(v for v in VARIANTS if v != "ppm_tp3")


def rewrite_base(bn):
    args, kw = REWRITE_BASES[bn]
    return vecgen.encode(streams._img(*args), sop=True, eph=True, cap_extra_bits=0 if kw.get("part1") else 0x1800, **kw)


def rewritten_layered_streams():
    """(name, codestream, base codestream) of every container variant of the layered bases"""
    for bn, (args, kw) in REWRITE_BASES.items():
        cs = rewrite_base(bn)
        made = dict(cs_rewrite.variants(cs, not kw.get("part1")))
        for vn in VARIANTS:
            if vn == "poc_layers" and kw.get("prog", 0) != 0:
                continue                                       # (two layer volumes leave the packets in place for LRCP only)
            yield bn + "." + vn, made[vn], cs


def test_container_variants_decode_to_the_base_frame(orc):
    """tile-parts after every packet, three tile-parts (also interleaved across tiles), PPM, PPT, TLM + PLT, and two
    progression volumes that end at different layers: the picture is the base's"""
    seen = 0
    base_frames = {}
    for name, data, cs in rewritten_layered_streams():
        bn, vn = name.split(".")
        if vn not in SAME_FRAME:
            continue
        if bn not in base_frames:
            _, planes, _ = orc.decode(cs)
            assert orc.block_errors() == 0
            base_frames[bn] = [p.copy() for p in planes]
        info, planes, consumed = orc.decode(data)
        assert orc.block_errors() == 0 and consumed > 0, name
        assert all(np.array_equal(a, b) for a, b in zip(planes, base_frames[bn])), name
        seen += 1
    assert seen == 3 * len(SAME_FRAME) - 1


def test_container_variants_through_both_parsers(plan_diff, tmp_path):
    """both parsers agree on every variant and on 40 damaged copies of each.  A PLT list does not make the packets of a
    layered tile readable in parallel (the state of a block runs from one packet of a precinct to the next): with packet
    threads on, every variant with a list takes the sequential reader -- no tile goes the parallel way -- with the same
    plan"""
    files = []
    for name, data, _ in rewritten_layered_streams():
        files.append(tmp_path / (name + ".j2c"))
        files[-1].write_bytes(data)
    parses, accepted = plan_diff(files, 40)
    assert accepted > parses // 3
    only_plt = [f for f in files if f.name.split(".")[1] in ("plt", "tp3_tlm_plt", "tp_each_packet", "ppm_tp3")]
    assert len(only_plt) == 12
    parses, accepted, ptiles, retries = plan_diff(only_plt, 0, threads=4)
    assert accepted > parses // 2 and (ptiles, retries) == (0, 0)
