"""GPU checks of the encoder's tile grid (htj2k_enc_opts.tile_w / tile_h): the forward transform kernels on
tile-components that start anywhere (htj2k_fdwt_regions) against the oracle's forward 5/3, the product's inverse and the
float32 9/7 model; whole tiled frames against vecgen's tiled encode byte for byte, decoded by the product decoder and
the oracle; pictures beyond 32768 samples; batches, padded and device input, device output and several rounds; rate
control over all tiles of a frame; and the C example's tiled round."""
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import enc97_model as e97
import enc_frames as ef
import enc_model as em
import enc_tiles_model as tm
import ffmpeg_ht_amd as m
import vecgen
from test_encode_gpu import _content

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, PATCHWELCOME = -22, -0x45574150
TILES = [(17, 13), (64, 64), (100, 70), (0, 16), (32, 0), (5, 3)]


@pytest.fixture(scope="module")
def enc():
    e = m.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def decoders():
    cache = {}
    yield cache
    for d in cache.values():
        d.close()


def decoder(cache, fmt, bitexact=0):
    key = em.pix(fmt), bitexact
    if key not in cache:
        cache[key] = m.Decoder(device_id=0, req_pix_fmt=key[0], bitexact=bitexact)
    return cache[key]


# ------------------------------------------------------------------ the transform kernels at an origin

SENTINEL = -123456
CELL_W, CELL_H, PER_ROW = 19, 10, 70              # a cell holds a region of up to 17 x 8 and a border of sentinels


def region_cases():
    """(w, h, x0, y0, levels): every combination the origin rules can differ on, and one deeper case"""
    small = list(itertools.product([1, 2, 3, 4, 5, 8, 17], [1, 2, 3, 5, 8], [0, 1, 2, 3, 5, 6, 7], [0, 1, 3, 6], range(5)))
    return small + [(37, 29, 13, 11, 6)]


def region_plane(cases, dtype):
    """one plane holding every case's region with sentinels around it -> (plane, regions for Encoder.fdwt_regions)"""
    rows = -(-(len(cases) - 1) // PER_ROW)
    plane = np.full((rows * CELL_H + 31, PER_ROW * CELL_W), SENTINEL, dtype)
    rng = np.random.default_rng(11)
    regions = []
    for k, (w, h, x0, y0, levels) in enumerate(cases):
        px, py = (1 + (k % PER_ROW) * CELL_W, 1 + (k // PER_ROW) * CELL_H) if k < len(cases) - 1 else (1, rows * CELL_H + 1)
        plane[py:py + h, px:px + w] = rng.integers(-(1 << 15), 1 << 15, size=(h, w))
        regions.append((px, py, w, h, x0, y0, levels))
    return plane, regions


def test_fdwt53_at_any_origin(enc, dec):
    cases = region_cases()
    plane, regions = region_plane(cases, np.int32)
    out = enc.fdwt_regions(plane, regions)
    inside = np.zeros(plane.shape, bool)
    for px, py, w, h, x0, y0, levels in regions:
        inside[py:py + h, px:px + w] = True
        src, got = plane[py:py + h, px:px + w], out[py:py + h, px:px + w]
        assert np.array_equal(got, tm.fdwt53(src, x0, y0, levels)), (w, h, x0, y0, levels)
    assert np.array_equal(out[~inside], plane[~inside])            # nothing outside a region is touched
    # the product's inverse with the same border gives the samples back
    for px, py, w, h, x0, y0, levels in regions:
        back = dec.idwt(np.ascontiguousarray(out[py:py + h, px:px + w]), ((x0, x0 + w), (y0, y0 + h)), levels, m.DWT53)
        assert np.array_equal(back, plane[py:py + h, px:px + w]), (w, h, x0, y0, levels)


def test_fdwt97_at_any_origin(enc):
    cases = region_cases()
    plane, regions = region_plane(cases, np.float32)
    out = enc.fdwt_regions(plane, regions, irreversible=True)
    inside = np.zeros(plane.shape, bool)
    for px, py, w, h, x0, y0, levels in regions:
        inside[py:py + h, px:px + w] = True
        want = tm.fdwt97(plane[py:py + h, px:px + w], x0, y0, levels)
        assert np.array_equal(out[py:py + h, px:px + w].view(np.uint32), want.view(np.uint32)), (w, h, x0, y0, levels)
    assert np.array_equal(out[~inside], plane[~inside])


def test_fdwt_regions_refuses_bad_regions(enc):
    plane = np.zeros((16, 16), np.int32)
    for bad in [(0, 0, 17, 4, 0, 0, 1), (13, 0, 4, 4, 0, 0, 1), (0, 14, 4, 4, 0, 0, 1), (0, 0, 0, 4, 0, 0, 1),
                (0, 0, 4, 4, -1, 0, 1), (0, 0, 4, 4, 0, 0, 33), (-1, 0, 4, 4, 0, 0, 1)]:
        with pytest.raises(m.Htj2kError) as e:
            enc.fdwt_regions(plane, [bad])
        assert e.value.code == EINVAL, bad


# ------------------------------------------------------------------ whole frames

def vecgen_tiled(comps, fmt, w, h, bits, cs, levels, cb, tile, qstep=None):
    g = em.qcd_guard_bits(cs)
    if qstep is None:
        return vecgen.encode(comps, tile=tile, **em.vecgen_args(fmt, w, h, bits, levels, cb, em.mct_default(fmt), g))
    return vecgen.encode(comps, tile=tile, **e97.vecgen_args(fmt, w, h, bits, levels, cb, em.mct_default(fmt), g, qstep))


def lossless_case(enc, orc, cache, fmt, bits, w, h, levels, cb, tile, seed=3, product=True):
    comps = _content("synth", fmt, w, h, bits, seed)
    planes = em.to_planes(comps, fmt, bits)
    what = (fmt, bits, w, h, levels, cb, tile)
    cs = enc.encode(planes, fmt, bits, levels=levels, cb=cb, tile=tile)
    assert cs == vecgen_tiled(comps, fmt, w, h, bits, cs, levels, cb, tile), what
    if product:
        info, got, _, st = decoder(cache, fmt).decode(cs)
        assert st.n_block_errors == 0, what
        assert all(np.array_equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(got, planes)), what
    _, got_o, _ = orc.decode(cs, req_pix_fmt=em.pix(fmt))
    assert all(np.array_equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(got_o, planes)), ("oracle",) + what
    return cs


def lossy_case(enc, orc, cache, fmt, bits, w, h, levels, cb, tile, qstep, seed=3):
    comps = _content("synth", fmt, w, h, bits, seed)
    planes = em.to_planes(comps, fmt, bits)
    what = (fmt, bits, w, h, levels, cb, tile, qstep)
    cs = enc.encode(planes, fmt, bits, levels=levels, cb=cb, tile=tile, irreversible=True, qstep=qstep)
    assert cs == vecgen_tiled(comps, fmt, w, h, bits, cs, levels, cb, tile, qstep), what
    for bitexact in (0, 1):
        _, got, _, st = decoder(cache, fmt, bitexact).decode(cs)
        assert st.n_block_errors == 0, what
        _, want, _ = orc.decode(cs, req_pix_fmt=em.pix(fmt), bitexact=bitexact)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (bitexact,) + what
    return cs


@pytest.mark.parametrize("fmt,bits", [("gray", 8), ("rgb24", 8), ("yuv422p", 8), ("yuv420p", 8), ("yuv422p10le", 10),
                                      ("rgba64le", 16)])
def test_tiled_frames_equal_vecgen_and_decode(enc, orc, decoders, fmt, bits):
    """the host test's grid on the device: every tile shape at every level count on 61 x 47, (4, 4) and (6, 6) blocks in
    turn; 190 x 131 with the two tile shapes that leave it more than one tile of several blocks"""
    for k, (tile, levels) in enumerate(itertools.product(TILES, [0, 1, 3, 5])):
        lossless_case(enc, orc, decoders, fmt, bits, 61, 47, levels, [(4, 4), (6, 6)][k & 1], tile)
    for tile, levels, cb in [((100, 70), 5, (4, 4)), ((64, 64), 3, (6, 6))]:
        lossless_case(enc, orc, decoders, fmt, bits, 190, 131, levels, cb, tile)


def test_one_sample_tiles(enc, orc, decoders):
    """gray 61 x 47 in 2867 tiles of one sample: origins of every parity at both levels, every line of one sample"""
    assert len(m.Encoder.tiles(61, 47, "gray", 8, levels=2, tile=(1, 1))) == 2867
    lossless_case(enc, orc, decoders, "gray", 8, 61, 47, 2, (6, 6), (1, 1))
    lossy_case(enc, orc, decoders, "gray", 8, 61, 47, 2, (6, 6), (1, 1), 1.0)


@pytest.mark.parametrize("fmt,bits", [("rgb24", 8), ("yuv420p", 8), ("yuv422p10le", 10)])
def test_tiled_lossy_frames_equal_vecgen(enc, orc, decoders, fmt, bits):
    for qstep, tile in itertools.product((0.25, 1.0, 4.0), [(17, 13), (64, 64)]):
        lossy_case(enc, orc, decoders, fmt, bits, 61, 47, 3, (4, 4), tile, qstep)
        lossy_case(enc, orc, decoders, fmt, bits, 190, 131, 5, (6, 6), tile, qstep)


def test_one_tile_is_the_untiled_stream(enc):
    for fmt, bits, (w, h) in [("rgb24", 8, (61, 47)), ("yuv420p", 8, (190, 131))]:
        planes = em.to_planes(_content("synth", fmt, w, h, bits, 3), fmt, bits)
        for opts in [dict(levels=3), dict(levels=3, irreversible=True, qstep=0.5)]:
            plain = enc.encode(planes, fmt, bits, **opts)
            for tile in [(0, 0), (w, h), (0, h), (w, 0)]:
                assert enc.encode(planes, fmt, bits, tile=tile, **opts) == plain, (fmt, tile)


# ------------------------------------------------------------------ beyond 32768

@pytest.mark.parametrize("w,h,tile,levels", [(32769, 8, (16384, 8), 2), (5, 32775, (3, 32768), 5)])
def test_pictures_beyond_32768(enc, orc, decoders, w, h, tile, levels):
    planes = em.to_planes(_content("synth", "gray", w, h, 8, 3), "gray", 8)
    for opts in [dict(), dict(irreversible=True, qstep=1.0)]:
        with pytest.raises(m.Htj2kError) as e:
            enc.encode(planes, "gray", 8, levels=levels, **opts)
        assert e.value.code == PATCHWELCOME
    lossless_case(enc, orc, decoders, "gray", 8, w, h, levels, (6, 6), tile)
    lossy_case(enc, orc, decoders, "gray", 8, w, h, levels, (6, 6), tile, 1.0)


def test_a_picture_taller_than_one_unpack_launch(enc, orc, decoders):
    """3 x 65541: more rows than grid.y takes, so the unpack stage reads the frame in bands; the stream is vecgen's and the
    product decoder and the oracle decode it to the source"""
    lossless_case(enc, orc, decoders, "gray", 8, 3, 65541, 1, (6, 6), (0, 32768))


def test_65535_one_sample_tiles(enc, orc, decoders):
    """gray 255 x 257 in tiles of one sample: as many tiles as a codestream can number, and as many pack tiles as one
    grid.z of the decoder takes (tests/test_decode_many_tiles_gpu.py goes beyond)"""
    assert len(m.Encoder.tiles(255, 257, "gray", 8, levels=0, tile=(1, 1))) == 65535
    lossless_case(enc, orc, decoders, "gray", 8, 255, 257, 0, (6, 6), (1, 1))


# ------------------------------------------------------------------ batches and I/O

BATCH_SIZES = [(61, 47), (190, 131), (75, 41)]


@pytest.mark.parametrize("opts", [dict(levels=3, cb=(4, 4)), dict(levels=3, cb=(4, 4), irreversible=True, qstep=0.5)], ids=["53", "97"])
@pytest.mark.parametrize("fmt,bits", [("rgb24", 8), ("yuv420p10le", 10)])
def test_batches_and_io(enc, fmt, bits, opts):
    """frames of three sizes under one tile option: one call == the single calls, from contiguous and padded host rows,
    from device memory with a true stride, and into device memory"""
    opts = dict(opts, tile=(17, 13))
    planes = [em.to_planes(_content("synth", fmt, w, h, bits, 5 + i), fmt, bits) for i, (w, h) in enumerate(BATCH_SIZES)]
    single = [enc.encode(p, fmt, bits, **opts) for p in planes]
    order = [0, 1, 2, 1, 0]
    want = [single[i] for i in order]
    assert enc.encode_batch([planes[i] for i in order], fmt, bits, **opts) == want
    pads = [(1, 13, 64, 1), (13, 64, 1, 13), (64, 1, 13, 64), (0, 0, 0, 0), (7, 7, 7, 7)]
    host = [ef.padded_frame(planes[i], fmt, *BATCH_SIZES[i], pd) for i, pd in zip(order, pads)]
    assert ef.encode_frames(enc, [f for f, _ in host], fmt, bits, **opts) == want
    dev = [ef.device_frame(planes[i], fmt, *BATCH_SIZES[i], pd, torch) for i, pd in zip(order, pads)]
    assert ef.encode_frames(enc, [f for f, _ in dev], fmt, bits, in_on_device=1, **opts) == want
    # device output: the same bytes and offsets, nothing behind the last stream
    frames = [f for f, _ in host]
    cap = sum(m.Encoder.bound(f.width, f.height, fmt, bits, **opts) for f in frames)
    out = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r, offs = ef.call_batch(enc, frames, bits, out.data_ptr(), cap=cap, out_on_device=1, **opts)
    assert r == 0 and offs == np.cumsum([0] + [len(c) for c in want]).tolist()
    back = out.cpu().numpy()
    assert back[:offs[-1]].tobytes() == b"".join(want) and (back[offs[-1]:] == 0xAB).all()


ROUND = 35000                                       # samples: four 61 x 47 rgb24 frames (8601 each) fit, a fifth does not


@pytest.fixture(scope="module")
def enc_small_rounds():
    mp = pytest.MonkeyPatch()
    mp.setenv("HTJ2K_ENC_ROUND", str(ROUND))
    try:
        e = m.Encoder(0)
    finally:
        mp.undo()
    yield e
    e.close()


@pytest.mark.parametrize("opts", [dict(levels=3, cb=(4, 4)), dict(levels=3, cb=(4, 4), irreversible=True, qstep=0.25, target_bytes=4000)],
                         ids=["53", "97-budget"])
def test_sixteen_tiled_frames_in_four_rounds(enc, enc_small_rounds, opts):
    fmt, bits, (w, h) = "rgb24", 8, (61, 47)
    assert 4 * 3 * w * h <= ROUND < 5 * 3 * w * h
    opts = dict(opts, tile=(17, 13))
    distinct = [em.to_planes(_content("synth" if s < 2 else "noise", fmt, w, h, bits, s), fmt, bits) for s in range(4)]
    order = [0, 2, 1, 3, 3, 0, 2, 1, 1, 1, 0, 3, 2, 2, 0, 3]
    single, planes_of = [], []
    for p in distinct:
        single.append(enc.encode(p, fmt, bits, **opts))
        planes_of.append(enc.last_planes(0))
    assert enc_small_rounds.encode_batch([distinct[i] for i in order], fmt, bits, **opts) == [single[i] for i in order]
    for k, i in enumerate(order):
        assert enc_small_rounds.last_planes(k) == planes_of[i], k
        assert enc_small_rounds.rc_info(k)["final_bytes"] == len(single[i]), k


# ------------------------------------------------------------------ rate control

@pytest.mark.parametrize("irreversible", [False, True], ids=["53", "97"])
def test_rate_control_over_all_tiles(enc, orc, decoders, irreversible):
    fmt, bits, w, h, tile = "rgb24", 8, 160, 96, (64, 48)
    comps = _content("synth", fmt, w, h, bits, 2)
    planes = em.to_planes(comps, fmt, bits)
    opts = dict(levels=3, cb=(4, 4), irreversible=irreversible, qstep=0.25, tile=tile)
    blocks = m.Encoder.layout(w, h, fmt, bits, **opts)
    idx = tm.coefficient_planes(comps, fmt, w, h, bits, 3, True, tile, 0.25 if irreversible else None)
    free = enc.encode(planes, fmt, bits, **opts)
    assert enc.last_planes(0) == [0] * len(blocks)
    for share in (0.75, 0.50, 0.25, 0.10):
        target = int(len(free) * share)
        cs = enc.encode(planes, fmt, bits, target_bytes=target, **opts)
        at, info = enc.last_planes(0), enc.rc_info(0)
        print(irreversible, share, len(cs), info)
        assert len(cs) <= target
        assert info["final_bytes"] == len(cs) and info["target_bytes"] == target and info["nblocks"] == len(blocks) == len(at)
        assert 1 <= info["ht_launches"] <= 3 and info["blocks_left_out"] == sum(p < 0 for p in at)
        data, mu = tm.code_blocks(idx, blocks, at)
        assert m.Encoder.assemble(w, h, fmt, bits, data, max_u=mu, planes=at, guard_bits=em.qcd_guard_bits(cs), **opts) == cs, share
        for bitexact in (0, 1):
            _, got, _, st = decoder(decoders, fmt, bitexact).decode(cs)
            assert st.n_block_errors == 0
            _, want, _ = orc.decode(cs, req_pix_fmt=em.pix(fmt), bitexact=bitexact)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (share, bitexact)
    for target in (len(free), len(free) + 1, 10 * len(free)):
        assert enc.encode(planes, fmt, bits, target_bytes=target, **opts) == free
    # the smallest stream holds every tile's SOT, SOD and empty packets; one byte less is refused with nothing written
    smallest = m.Encoder.assemble(w, h, fmt, bits, [b""] * len(blocks), **opts)
    untiled = {k: v for k, v in opts.items() if k != "tile"}
    one = m.Encoder.assemble(w, h, fmt, bits, [b""] * len(m.Encoder.layout(w, h, fmt, bits, **untiled)), **untiled)
    assert len(m.Encoder.tiles(w, h, fmt, bits, **opts)) == 6
    assert len(smallest) == len(one) + 5 * (14 + 4 * 3)            # per tile SOT, SOD and an empty packet per resolution and component
    assert enc.encode(planes, fmt, bits, target_bytes=len(smallest), **opts) == smallest
    fr, keep = m.frame_from_planes(planes, fmt)
    out = np.full(len(free) + 16, 0xAB, np.uint8)
    r, _ = ef.call_batch(enc, [fr], bits, out, target_bytes=len(smallest) - 1, **opts)
    assert r == EINVAL and (out == 0xAB).all()


# ------------------------------------------------------------------ the C example

def test_example_tiled_round_trip():
    exe = os.path.join(ROOT, "examples", "htj2k_encode")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", ROOT, "examples/htj2k_encode"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "round trip ok" in out.stdout and "4 tiles of 1000x1000" in out.stdout and "tiled round trip ok" in out.stdout
