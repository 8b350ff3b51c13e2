"""CPU checks of the encoder's tile grid (no GPU): htj2k_enc_layout / htj2k_enc_tiles / htj2k_enc_assemble with
tile=(w, h).  Blocks are coded by vecgen's encode_block from the tiled model planes (tests/enc_tiles_model.py); the
assembled stream must be vecgen's own tiled encode(...) byte for byte, and the oracle must decode it to the source."""
import itertools

import numpy as np
import pytest

import enc_model as em
import enc_tiles_model as tm
import ffmpeg_ht_amd as m
import vecgen
from test_encode_host import synth

FMTS = ["gray", "rgb24", "yuv422p", "yuv420p"]
PICTURES = [(61, 47), (190, 131)]
TILES = [(17, 13), (64, 64), (100, 70), (0, 16), (32, 0), (5, 3)]
LEVELS = [0, 1, 3, 5]
CBS = [(6, 6), (4, 4)]
EINVAL, PATCHWELCOME = -22, -0x45574150


def assemble_tiled(comps, fmt, w, h, bits, levels, cb, tile, planes=None):
    """-> (stream, [block bytes]) from vecgen-coded blocks of the model planes"""
    opts = dict(levels=levels, cb=cb, tile=tile)
    if planes is None:
        planes = tm.coefficient_planes(comps, fmt, w, h, bits, levels, em.mct_default(fmt), tile)
    data, mu = tm.code_blocks(planes, m.Encoder.layout(w, h, fmt, bits, **opts))
    return m.Encoder.assemble(w, h, fmt, bits, data, max_u=mu, **opts), data


def vecgen_tiled(comps, fmt, w, h, bits, levels, cb, tile, cs):
    args = em.vecgen_args(fmt, w, h, bits, levels, cb, em.mct_default(fmt), em.qcd_guard_bits(cs))
    return vecgen.encode(comps, tile=tile, **args)


def decodes_to_source(orc, cs, comps, fmt, bits):
    _, planes, _ = orc.decode(cs, req_pix_fmt=em.pix(fmt))
    want = em.to_planes(comps, fmt, bits)
    return len(planes) == len(want) and all(np.array_equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(planes, want))


@pytest.mark.parametrize("w,h", PICTURES)
@pytest.mark.parametrize("fmt", FMTS)
def test_assembled_tiled_streams_equal_vecgen(orc, fmt, w, h):
    comps = synth(fmt, w, h, 8)
    for tile, levels in itertools.product(TILES, LEVELS):
        planes = tm.coefficient_planes(comps, fmt, w, h, 8, levels, em.mct_default(fmt), tile)
        for cb in CBS:
            what = "%s %dx%d tile %s, %d levels, cb %s" % (fmt, w, h, tile, levels, cb)
            cs, data = assemble_tiled(comps, fmt, w, h, 8, levels, cb, tile, planes)
            assert cs == vecgen_tiled(comps, fmt, w, h, 8, levels, cb, tile, cs), what
            assert decodes_to_source(orc, cs, comps, fmt, 8), what
            # htj2k_encode_bound covers every tile's SOT, SOD and packet headers
            assert m.Encoder.bound(w, h, fmt, 8, levels=levels, cb=cb, tile=tile) >= len(cs), what


def test_one_tile_is_the_untiled_stream():
    for fmt, (w, h) in [("rgb24", (61, 47)), ("yuv420p", (61, 47)), ("gray", (190, 131))]:
        comps = synth(fmt, w, h, 8)
        opts = dict(levels=3, cb=(4, 4))
        planes = em.coefficient_planes(comps, fmt, 8, 3, em.mct_default(fmt))
        blocks = m.Encoder.layout(w, h, fmt, 8, **opts)
        data, mu = tm.code_blocks(planes, blocks)
        plain = m.Encoder.assemble(w, h, fmt, 8, data, max_u=mu, **opts)
        for tile in [(0, 0), (w, h), (w, 0), (0, h)]:
            assert m.Encoder.layout(w, h, fmt, 8, tile=tile, **opts) == blocks
            assert m.Encoder.assemble(w, h, fmt, 8, data, max_u=mu, tile=tile, **opts) == plain, (fmt, tile)
            assert m.Encoder.bound(w, h, fmt, 8, tile=tile, **opts) == m.Encoder.bound(w, h, fmt, 8, **opts)


def code_of(call):
    with pytest.raises(m.Htj2kError) as e:
        call()
    return e.value.code


def test_refusals():
    lay, asm = m.Encoder.layout, m.Encoder.assemble
    for tile in [(-1, 0), (0, -1), (-16, -16)]:
        assert code_of(lambda: lay(61, 47, "gray", 8, tile=tile)) == EINVAL
    assert code_of(lambda: lay(300, 300, "gray", 8, tile=(1, 1))) == EINVAL            # 90000 tiles
    assert len(m.Encoder.tiles(255, 257, "gray", 8, levels=0, tile=(1, 1))) == 65535   # the most Isot can number
    assert code_of(lambda: lay(256, 256, "gray", 8, levels=0, tile=(1, 1))) == EINVAL
    assert code_of(lambda: lay(61, 47, "yuv420p", 8, tile=(1, 1))) == EINVAL           # empty chroma tile-components
    assert code_of(lambda: lay(61, 47, "yuv422p", 8, tile=(1, 4))) == EINVAL
    assert code_of(lambda: lay(61, 47, "yuv420p", 8, tile=(2, 1))) == EINVAL
    assert len(m.Encoder.tiles(61, 47, "yuv420p", 8, tile=(2, 2))) == 31 * 24
    # a tile-component beyond 32768 samples, with and without tiles; the picture may be larger when its tiles are not
    assert code_of(lambda: lay(32769, 8, "gray", 8)) == PATCHWELCOME
    assert code_of(lambda: lay(8, 32769, "gray", 8)) == PATCHWELCOME
    assert code_of(lambda: lay(40000, 8, "gray", 8, tile=(32769, 0))) == PATCHWELCOME
    assert code_of(lambda: lay(40000, 8, "gray", 8, tile=(0, 4))) == PATCHWELCOME
    assert len(m.Encoder.tiles(32769, 8, "gray", 8, levels=2, tile=(16384, 8))) == 3
    assert len(m.Encoder.tiles(70000, 8, "yuv420p", 8, levels=2, tile=(32768, 8))) == 3
    # every refusal writes nothing, and the bound of a refused frame is 0
    for kw in [dict(tile=(-1, 0)), dict(tile=(1, 1))]:
        assert m.Encoder.bound(300, 300, "gray", 8, **kw) == 0
        assert code_of(lambda: asm(300, 300, "gray", 8, [], cap=64, **kw)) == EINVAL


@pytest.mark.parametrize("fmt,w,h,tile,levels,cb", [
    ("gray", 61, 47, (17, 13), 3, (4, 4)), ("yuv420p", 61, 47, (5, 3), 2, (6, 6)), ("rgb24", 190, 131, (100, 70), 5, (4, 4)),
    ("yuv422p", 190, 131, (0, 16), 3, (6, 6)), ("gray", 61, 47, (1, 1), 2, (6, 6))])
def test_tile_report_is_consistent_with_the_layout(fmt, w, h, tile, levels, cb):
    opts = dict(levels=levels, cb=cb, tile=tile)
    blocks = m.Encoder.layout(w, h, fmt, 8, **opts)
    tiles = m.Encoder.tiles(w, h, fmt, 8, **opts)
    nc = len(em.comp_dims(fmt, w, h))
    assert [t["rects"][:nc] for t in tiles] == tm.tile_rects(fmt, w, h, tile)
    # the tiles' block ranges follow each other and cover the layout
    assert tiles[0]["blk0"] == 0 and tiles[-1]["blk0"] + tiles[-1]["nblk"] == len(blocks)
    assert all(a["blk0"] + a["nblk"] == b["blk0"] for a, b in zip(tiles, tiles[1:]))
    cover = [np.zeros((ch, cw), np.int32) for cw, ch in em.comp_dims(fmt, w, h)]
    for t in tiles:
        mine = blocks[t["blk0"]:t["blk0"] + t["nblk"]]
        # packet order inside the tile: resolution, then component
        assert [(b["res"], b["comp"]) for b in mine] == sorted((b["res"], b["comp"]) for b in mine)
        for b in mine:
            x0, y0, x1, y1 = t["rects"][b["comp"]]
            assert x0 <= b["x"] and b["x"] + b["w"] <= x1 and y0 <= b["y"] and b["y"] + b["h"] <= y1
            cover[b["comp"]][b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]] += 1
    assert all((c == 1).all() for c in cover)


def test_stream_shape():
    """SIZ carries the tile size, every tile is one tile-part with its real length, nothing follows the last but EOC"""
    fmt, w, h, tile = "rgb24", 61, 47, (17, 0)
    comps = synth(fmt, w, h, 8)
    cs, _ = assemble_tiled(comps, fmt, w, h, 8, 2, (4, 4), tile)
    siz = cs.index(b"\xff\x51")
    u32 = lambda at: int.from_bytes(cs[at:at + 4], "big")
    assert [u32(siz + 6 + 4 * k) for k in range(8)] == [w, h, 0, 0, 17, h, 0, 0]
    at = cs.index(b"\xff\x90")
    for t in range(4):
        assert cs[at:at + 4] == b"\xff\x90\x00\x0a" and int.from_bytes(cs[at + 4:at + 6], "big") == t
        assert cs[at + 10:at + 14] == b"\x00\x01\xff\x93"
        at += u32(at + 6)
    assert cs[at:] == b"\xff\xd9"
