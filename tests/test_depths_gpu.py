"""Components of unequal bit depth (streams.DEPTHS) through the device layer, frame for frame equal to the CPU oracle's.
Every frame goes through a conversion per component -- add 1 << (cbps - 1), clip to [0, 2^cbps - 1], shift left by
precision - cbps -- which the product has in three places (ffmpeg-ht_amd/csrc):
 * pack_value / pack_convert (pack_kernels.hpp): k_mct_pack and the general path of the fused final level
 * the four fast stores of k_idwt_stream_pack (dwt_stream.hpp): constants per component in f_dc / f_hi / f_sh, for the plane
   stores taken from component comp0; stream_fast_outk reads cbps per component to qualify a group
 * the host: the packed 16-bit final level wants cbps == 8 of every component of a fused group, the 16-bit LL check starts
   at cbps + 2 of each tile-component (pk16_eligibility, htj2k_device.hip)
tests/test_depths_streams.py pins the streams and the oracle's conversion on the CPU; test_gpu_parity.py::
test_frames_match_oracle runs every case without a requested layout in the four IDWT modes as well.
Every test decodes pictures of its own (a seed per test): a job's device buffers are not cleared."""
import ctypes

import numpy as np
import pytest

import oracle
import streams
import vecgen
from test_gpu_parity import damaged_bodies_match_the_oracle, stage_planes_match_oracle
from test_hetero_gpu import same_frames
from test_hetero_streams import _oracle_tilecomps
from test_depths_streams import layout_of

pytestmark = pytest.mark.gpu

DEFAULTS = dict(coef16=1, ll16=1, idwt_x3=1, idwt_x2=2, idwt_pk=1, ht_pair=1, ht_multi=1, fuse_pack=1, idwt_mode=3,
                bitexact=0, reduction_factor=0)


@pytest.fixture(scope="module")
def decs():
    """decoders by requested layout (None: the default one), opened when first asked for"""
    import ffmpeg_ht_amd as m
    made = {}

    def get(req=None):
        if req not in made:
            made[req] = m.Decoder(device_id=0, req_pix_fmt=-1 if req is None else m.PIX_NAMES.index(req))
            assert made[req].device_name().startswith("gfx950")
        return made[req]
    yield get
    for d in made.values():
        d.close()


@pytest.fixture()
def dec(decs):
    d = decs()
    yield d
    for knob, value in DEFAULTS.items():
        d.set_int(knob, value)


def case(name, seed):
    """DEPTHS[name] over the picture of another seed -> (codestream, decode keywords for the oracle)"""
    return streams.depths_encode(name, seed=seed), streams.depths_decode_kw(name, oracle.PIX_NAMES)


def decoder_for(decs, name):
    dkw = streams.DEPTHS[name][3]
    d = decs(dkw.get("req_pix_fmt"))
    d.set_int("bitexact", dkw.get("bitexact", 0))
    d.set_int("reduction_factor", dkw.get("reduction_factor", 0))
    return d


# ---------------------------------------------------------------- which store a stream takes
def store_kinds(tcs, info, P):
    """build_descriptors' grouping of a frame's tile-components and stream_fast_geom / stream_fast_outk (dwt_stream.hpp)
    restated over the plan's tile-component table -> the set of stores the fused final level of the frame takes: 0 rgb24,
    1 rgb48, 2 an 8-bit plane, 3 a 16-bit plane, -1 the general path, None a tile that is not fused at all.
    (The frames of a job lie in device buffers of the library's own: lines and planes are aligned.)"""
    nc, out_bytes = info.ncomponents, 1 if P == 8 else 2
    W, H = list(info.plane_width), list(info.plane_height)

    def final(tc):
        lev = int(tc["ndeclevels"]) - 1
        return lev, int(tc["linelen"][lev][0]), int(tc["linelen"][lev][1]), int(tc["mod"][lev][0]), int(tc["mod"][lev][1])

    def same(a, b):
        return (a["w"], a["h"], a["ndeclevels"], a["transform"]) == (b["w"], b["h"], b["ndeclevels"], b["transform"]) and final(a)[3:] == final(b)[3:]

    def placed(C, lh, lv):
        pl = int(C["out_plane"])
        return C["out_x"] >= 0 and not C["out_x"] & 3 and C["out_y"] >= 0 and C["out_x"] + lh <= W[pl] and C["out_y"] + lv <= H[pl]

    def kind(T, g0, ncg, comp0):
        lev, lh, lv, mh, mv = final(T[g0])
        if mh & 1 or lh & 3 or lh < 8 or lv < 2:
            return -1
        k = -1
        if ncg == 3 and nc == 3 and comp0 == 0 and T[0]["pix_step"] == 3 and [int(t["pix_off"]) for t in T] == [0, 1, 2] and placed(T[0], lh, lv):
            if out_bytes == 1 and P == 8 and all(t["cbps"] <= 8 for t in T):
                k = 0
            elif out_bytes == 2 and P <= 16 and all(t["cbps"] <= P for t in T):
                k = 1
        elif ncg == 1:
            C = T[comp0]
            if C["pix_step"] == 1 and C["pix_off"] == 0 and placed(C, lh, lv):
                if out_bytes == 1 and P == 8 and C["cbps"] <= 8:
                    k = 2
                elif out_bytes == 2 and P <= 16 and C["cbps"] <= P:
                    k = 3
        return -1 if k > 0 and T[g0]["transform"] == 2 else k      # rgb48 / plane stores: 5/3 and 9/7 float only

    kinds = set()
    for t0 in range(0, len(tcs), nc):
        T = tcs[t0:t0 + nc]
        ok = all(t["coded"] and t["ndeclevels"] >= 1 and final(t)[1] >= 2 and final(t)[2] >= 2 and
                 (final(t)[1], final(t)[2]) == (t["w"], t["h"]) for t in T)
        groups = []
        if ok and T[0]["pix_step"] > 1:
            ok = nc in (3, 4) and all(same(T[0], t) and t["pix_step"] == T[0]["pix_step"] and t["out_plane"] == T[0]["out_plane"] for t in T[1:])
            groups = [(0, nc, 0)]
        elif ok:
            first = 0
            if T[0]["mct"]:
                ok = nc >= 3 and same(T[0], T[1]) and same(T[0], T[2])
                groups, first = [(0, 3, 0)], 3
            groups += [(c, 1, c) for c in range(first, nc)]
        if not ok:
            kinds.add(None)
            continue
        kinds |= {kind(T, g0, ncg, comp0) for g0, ncg, comp0 in groups}
    return kinds


# what every case is there for: the store its fused final level takes.  None: two packed components are no group of the
# fused plan, k_mct_pack writes the frame in every mode.  (Every case on 53 x 37: the general path, or None likewise)
STORE = {
    "dep_rgb24_583": 0, "dep_rgb24_878_rct": 0, "dep_rgb24_876_rct": 0, "dep_rgb24_876_ict": 0, "p1_dep_rgb24_876_rct": 0,
    "dep_rgb24_583_lowres_1": 0, "dep_clip_rgb24_583": 0,
    "dep_rgb48_8_12_8": 1, "dep_rgb48_8_12_8_rct": 1, "dep_rgb48_8_12_8_rct_qcc": 1, "dep_rgb48_12_10_16": 1,
    "dep_rgb48_12_10_16_rct": 1, "dep_rgb48_10_12_9_ict": 1, "dep_rgb48_8_12_8_sgnd": 1, "dep_clip_rgb48_10_12_9": 1,
    "dep_yuv420p_866": 2, "dep_yuv420p_866_levels_322": 2, "dep_yuv444p_878": 2, "dep_clip_yuv420p_866": 2,
    "dep_yuv422p12_10_12_9": 3, "dep_yuv444p16_8_12_8": 3, "dep_clip_yuv422p12_10_12_9": 3,
    # general path on the fast geometry: the fixed-point transform has the rgb24 store only; two and four components;
    # tiles of 50 columns
    "dep_rgb48_10_12_9_ict_bitexact": -1, "dep_ya16_12_8": None, "dep_ya8_8_1": None, "dep_rgba_8881": -1,
    "dep_rgba64_10_10_10_16": -1, "dep_clip_rgba_8881": -1, "dep_rgb24_583_tiles50": -1, "dep_rgb48_8_12_8_tiles50": -1,
}


def store_of(name):
    return STORE[name] if name in STORE else None if "_ya" in name else -1


def test_every_store_has_its_cases():
    assert set(STORE) == {n for n, v in streams.DEPTHS.items() if v[0][:2] == streams.DEPTHS_FAST}
    by = {k: {tuple(streams.DEPTHS[n][1]) for n in STORE if STORE[n] == k} for k in (0, 1, 2, 3, -1)}
    assert {(5, 8, 3), (8, 7, 8)} <= by[0] and {(8, 12, 8), (10, 12, 9)} <= by[1]
    assert {(8, 6, 6), (8, 7, 8)} <= by[2] and {(10, 12, 9), (8, 12, 8)} <= by[3]
    assert {(8, 8, 8, 1), (10, 10, 10, 16)} <= by[-1] and {(8, 1), (12, 8)} == {tuple(streams.DEPTHS[n][1]) for n in STORE if STORE[n] is None}


@pytest.mark.parametrize("name", sorted(streams.DEPTHS))
def test_every_store_route_fused_and_unfused(decs, dec, orc, name):
    """A job of two frames from different seeds, with the pack stage fused into the final level and without, in the three
    IDWT modes: the oracle's frames.  The case must take the store it is there for: the plan's tile-component table says
    which (store_kinds), and the job of the fused streaming mode shows what it exposes of that -- a fused final launch that
    moves fewer bytes than the plain level would; 16-bit sub-bands, which only jobs whose every fused launch is a fast-store
    one get, exactly when the stream's blocks allow them; no packed 16-bit final level for a group whose components are not
    all of 8 bits"""
    d = decoder_for(decs, name)
    depths, ekw = streams.DEPTHS[name][1], streams.DEPTHS[name][2]
    seed = 1000 + 2 * sorted(streams.DEPTHS).index(name)
    pkts, want = [], []
    for s in (seed, seed + 1):
        data, kw = case(name, s)
        pkts.append(data)
        info_o, planes_o, _ = orc.decode(data, **kw)
        assert orc.block_errors() == 0
        want.append(planes_o)
    assert any(not np.array_equal(a, b) for a, b in zip(*want))
    fmt, bits, P = layout_of(name)
    r, tcs, info_p = _oracle_tilecomps(orc, pkts[0], want_info=True, **kw)
    kinds = store_kinds(tcs, info_p, P)
    assert kinds == {store_of(name)}, (name, kinds)
    blocks = orc.plan_blocks(pkts[0], **kw)
    lossless_ht = ekw.get("transform", 1) == 1 and not ekw.get("part1") and not any((c or {}).get("transform", 1) == 0 for c in ekw.get("comp", []))
    # ht_block_routes + job_ht_eligibility: reversible HT blocks of one cleanup pass, at most 64 columns and M_b <= 15, and
    # every fused launch a fast-store one
    c16 = lossless_ht and kinds <= {0, 1, 2, 3} and int(blocks["M_b"].max()) <= 15 and int(blocks["w"].max()) <= 64
    try:
        for fuse, mode in [(1, 3), (1, 1), (1, 0), (0, 3), (0, 1), (0, 0)]:
            d.set_int("fuse_pack", fuse)
            d.set_int("idwt_mode", mode)
            job = d.job().parse_batch(pkts).upload().run().wait()
            assert job.block_errors() == 0
            for f in range(2):
                info, planes = job.download_frame(f)
                assert (oracle.PIX_NAMES[info.pix_fmt], info.bits_per_raw_sample) == (fmt, bits)
                same_frames(planes, want[f], (name, fuse, mode, f))
            if mode == 3:
                launches, hbm = job.idwt_launches(), job.idwt_hbm_bytes()
                assert len(launches) == len(hbm) > 0
                fused_launch = any(hb < by for (ms, by), hb in zip(launches, hbm))
                assert fused_launch == bool(fuse and None not in kinds), (name, fuse, launches, hbm)
                assert job.coef16() == bool(fuse and c16), (name, fuse, job.coef16(), int(blocks["M_b"].max()))
                assert job.ll16() == (1 if fuse and c16 else 0), (name, fuse, job.ll16())
                if fuse and c16:
                    assert job.ht_blocks_per_wave() == 2, name                   # k_ht_decode_pair
                else:
                    assert job.ht_blocks_per_wave() in ((0,) if ekw.get("part1") else (1, 2, 4)), name
                # the packed level: the luma launch of dep_yuv420p_866_levels_322 alone (test_packed_level_and_yuv420_8_6_6)
                assert (job.idwt_packed() > 0) == (fuse == 1 and name == "dep_yuv420p_866_levels_322"), (name, fuse, job.idwt_packed())
            job.free()
    finally:
        for knob, value in DEFAULTS.items():
            d.set_int(knob, value)


# ---------------------------------------------------------------- the packed 16-bit final level
def _rgb8(seed):
    return vecgen.encode(vecgen.synth_image(*streams.DEPTHS_FAST, 3, seed=seed, noise=10), mct=1, nlevels=3)


def _yuv420_8(seed, **kw):
    img = vecgen.synth_image(*streams.DEPTHS_FAST, 3, seed=seed, noise=10, dx=[1, 2, 2], dy=[1, 2, 2])
    return vecgen.encode(img, nlevels=3, dx=[1, 2, 2], dy=[1, 2, 2], width=streams.DEPTHS_FAST[0], height=streams.DEPTHS_FAST[1], **kw)


def _run(dec, orc, pkts, what):
    want = [orc.decode(p)[1] for p in pkts]
    job = dec.job().parse_batch(pkts).upload().run().wait()
    assert job.block_errors() == 0 and job.coef16(), what
    for f in range(len(pkts)):
        same_frames(job.download_frame(f)[1], want[f], (what, f))
    packed = job.idwt_packed()
    job.free()
    return packed


def test_packed_level_and_rgb_8_7_8(dec, orc):
    """Two 8/8/8 RCT frames on the fast geometry take the packed 16-bit final level (components of 8 bits: DC shift and clip
    there are "clamp to [-128, 127], flip bit 7").  An 8/7/8 frame between them shares their rgb24 launch, and a launch
    keeps the packed level only if every component of every group in it has 8 bits: none does.  (The job keeps its 16-bit
    sub-bands: the rgb24 store takes components of up to 8 bits.)"""
    a, b = _rgb8(2001), _rgb8(2002)
    assert _run(dec, orc, [a, b], "8/8/8") > 0
    assert _run(dec, orc, [a, case("dep_rgb24_878_rct", 2003)[0], b], "8/7/8 between") == 0
    assert _run(dec, orc, [a, case("dep_rgb24_876_rct", 2004)[0], b], "8/7/6 between") == 0


def test_packed_level_and_yuv420_8_6_6(dec, orc):
    """4:2:0 planes are groups of one component each, and the groups of a level, transform and store share a launch
    (build_descriptors): luma and chroma of three levels each lie in one launch of the 8-bit plane store, so an 8/6/6 frame
    takes the packed level from that launch, for its own 8-bit luma and for every 8/8/8 frame next to it: 0.  With chroma of
    two levels (dep_yuv420p_866_levels_322) the chroma planes' final level is a launch of its own, at level 1, which is not
    packed, and the luma launch at level 2 keeps the packed level -- of the 8/6/6 frames alone and next to 8/8/8 frames
    whose chroma has two levels as well"""
    a, b = _yuv420_8(2011), _yuv420_8(2012)
    assert _run(dec, orc, [a, b], "8/8/8") > 0
    assert _run(dec, orc, [a, case("dep_yuv420p_866", 2013)[0], b], "8/6/6 between") == 0
    assert _run(dec, orc, [case("dep_yuv420p_866", 2014)[0], case("dep_yuv420p_866", 2015)[0]], "8/6/6") == 0
    levels = dict(comp=[dict(nlevels=3), dict(nlevels=2), dict(nlevels=2)])
    assert _run(dec, orc, [case("dep_yuv420p_866_levels_322", 2016)[0], case("dep_yuv420p_866_levels_322", 2017)[0]], "8/6/6, levels 3/2/2") > 0
    assert _run(dec, orc, [_yuv420_8(2018, **levels), case("dep_yuv420p_866_levels_322", 2019)[0], _yuv420_8(2020, **levels)],
                "8/6/6 between, levels 3/2/2") > 0


# ---------------------------------------------------------------- knobs
KNOBS = [("coef16", 0), ("ll16", 0), ("idwt_x3", 0), ("idwt_x2", 1), ("idwt_pk", 0), ("ht_pair", 0), ("ht_multi", 0), ("fuse_pack", 0)]


@pytest.mark.parametrize("name", ["dep_rgb24_878_rct", "dep_yuv422p12_10_12_9"])
def test_knobs_leave_mixed_depth_frames_alone(dec, orc, name):
    """every knob at its other value, one at a time: the oracle's frames.  (idwt_x2 1 asks for the last plain level inside
    the packed final-level launch wherever the job allows it: a job with a 7-bit component must not)"""
    pkts = [case(name, 3000 + i)[0] for i in range(2)]
    want = [orc.decode(p)[1] for p in pkts]
    try:
        for knob, value in [(None, None)] + KNOBS:
            if knob:
                dec.set_int(knob, value)
            job = dec.job().parse_batch(pkts).upload().run().wait()
            assert job.block_errors() == 0 and job.idwt_packed() == 0, (name, knob)
            assert job.coef16() == (knob not in ("coef16", "fuse_pack")), (name, knob)
            assert job.ll16() == (0 if knob in ("coef16", "fuse_pack", "ll16") else 1), (name, knob)
            for f in range(2):
                same_frames(job.download_frame(f)[1], want[f], (name, knob, f))
            job.free()
            if knob:
                dec.set_int(knob, DEFAULTS[knob])
    finally:
        for knob, value in DEFAULTS.items():
            dec.set_int(knob, value)


# ---------------------------------------------------------------- stage planes
@pytest.mark.parametrize("name", ["dep_rgb48_8_12_8_rct", "dep_rgb48_10_12_9_ict", "dep_rgb48_10_12_9_ict_bitexact"])
def test_stage_planes_match_oracle(dec, orc, name):
    """dequantised sub-bands and IDWT output of every plane in the three IDWT modes: RCT, ICT float, ICT fixed point over
    components of 8 to 12 bits (guard bits for the deepest)"""
    data, kw = case(name, 4000)
    stage_planes_match_oracle(dec, orc, data, kw)


# ---------------------------------------------------------------- other entry points
ENTRY = ["dep_rgb24_878_rct", "dep_rgb48_8_12_8", "dep_yuv422p12_10_12_9", "dep_yuv420p_866", "dep_odd_rgba_8881", "dep_odd_ya16_12_8",
         "dep_rgb24_583_tiles50"]


def test_one_call_path_and_padded_lines(dec, orc):
    """htj2k_decode into lines of the picture's own length and into lines padded to 64 and 256 bytes, over buffers filled
    with 0xAB: the whole buffer is compared, the padding keeps its 0xAB"""
    import ffmpeg_ht_amd as m
    for i, name in enumerate(ENTRY):
        data, kw = case(name, 5000 + i)
        info_o, want, consumed_o = orc.decode(data, **kw)
        for align in (1, 64, 256):
            info = dec.probe(data)
            planes, fr = m.alloc_frame(info, align)
            expect = []
            for p, a in enumerate(planes):
                a[:] = 0xAB
                e = a.copy()
                row = np.ascontiguousarray(want[p]).view(np.uint8).reshape(info.plane_height[p], -1)
                assert row.shape[1] == info.plane_width[p] * info.plane_bytes_per_sample[p] <= a.shape[1]
                e[:, :row.shape[1]] = row
                expect.append(e)
            st = m.Stats()
            pkt = m.packet(data)
            r = dec.L.htj2k_decode(dec.h, pkt[0], pkt[1], ctypes.byref(fr), ctypes.byref(st))
            assert r == consumed_o and st.n_block_errors == 0, (name, align, r)
            for p in range(info.nplanes):
                assert np.array_equal(planes[p], expect[p]), (name, align, p)


def test_pipe_host_and_device_frames(dec, orc):
    """the pipeline entry points: a mixed-depth frame between equal-depth frames of the same layout, in batches of four,
    received into host frames and as device frames"""
    import ffmpeg_ht_amd as m
    fast = streams.DEPTHS_FAST
    rgb12 = lambda s: vecgen.encode(vecgen.synth_image(*fast, 3, depth=12, seed=s, noise=40), depth=12, nlevels=3)
    yuv422 = lambda s: vecgen.encode(vecgen.synth_image(*fast, 3, depth=12, seed=s, noise=40, dx=[1, 2, 2], dy=[1, 1, 1]), depth=12, nlevels=3,
                                     dx=[1, 2, 2], dy=[1, 1, 1], width=fast[0], height=fast[1])
    pkts = [_rgb8(6001), case("dep_rgb24_878_rct", 6002)[0], _rgb8(6003), case("dep_rgb24_583", 6004)[0],
            rgb12(6005), case("dep_rgb48_8_12_8", 6006)[0], rgb12(6007),
            _yuv420_8(6008), case("dep_yuv420p_866", 6009)[0], _yuv420_8(6010),
            yuv422(6011), case("dep_yuv422p12_10_12_9", 6012)[0], yuv422(6013), case("dep_odd_rgba_8881", 6014)[0]]
    want = [orc.decode(p)[1] for p in pkts]
    for device in (False, True):
        pipe = dec.pipe(batch=4, depth=2)
        try:
            sent = got = 0
            while got < len(pkts):
                while sent < len(pkts) and pipe.send(pkts[sent]):
                    sent += 1
                if sent == len(pkts):
                    pipe.flush()
                if device:
                    info = m.Info()
                    assert dec.L.htj2k_pipe_info(pipe.h, ctypes.byref(info)) >= 0
                    fr = pipe.receive_device()
                    assert fr is not None
                    planes = dec.fetch_device_frame(info, fr)
                else:
                    info, planes = pipe.receive()
                same_frames(planes, want[got], (got, device))
                got += 1
        finally:
            pipe.close()


@pytest.mark.parametrize("name", ["dep_rgb24_878_rct", "dep_rgb48_10_12_9_ict", "dep_yuv422p12_10_12_9", "dep_odd_rgba64_10_10_10_16"])
def test_job_compare_against_the_oracle_frames(dec, orc, name):
    """htj2k_job_compare of a decoded mixed-depth job against the oracle's frames, bits 0, references on the host and on the
    device: every error sum 0, every sample counted"""
    pkts = [case(name, 7000 + i)[0] for i in range(2)]
    want = [orc.decode(p)[1] for p in pkts]
    job = dec.job().parse_batch(pkts).upload().run().wait()
    ref = dec.job().parse_batch(pkts).upload().run().wait()          # the same frames in device memory of their own ...
    for f in range(2):
        same_frames(ref.download_frame(f)[1], want[f], (name, f))    # ... which are the oracle's
    for got in (job.compare(want, bits=0), job.compare([ref.device_frame(f) for f in range(2)], bits=0, on_device=True)):
        assert len(got) == 2
        for f, d in enumerate(got):
            nc = len(streams.DEPTHS[name][1])
            assert d["sse"] == [0] * 4 and d["ndiff"] == [0] * 4 and d["max_abs"] == [0] * 4, (name, f, d)
            assert sum(d["nsamples"]) == sum(int(p.size) for p in want[f]) and all(n > 0 for n in d["nsamples"][:nc]), (name, f, d)
    # and a frame that differs is seen: the references exchanged
    got = job.compare(want[::-1], bits=0)
    assert all(sum(d["ndiff"]) > 0 for d in got)
    job.free()
    ref.free()


def test_damaged_bodies_of_a_mixed_depth_stream(dec, orc):
    """the mutation of test_damaged_ht_bodies_match_the_oracle, with its two carve-outs and no other, on an 8/12/8 RCT
    stream: the same error code, or the same pixels and the same number of rejected blocks"""
    data, kw = case("dep_rgb48_8_12_8_rct", 8000)
    same, carved, rejected = damaged_bodies_match_the_oracle(dec, orc, np.random.default_rng(13), "dep_rgb48_8_12_8_rct", data, kw)
    assert same >= 15 and carved < same // 4, (same, carved, rejected)
