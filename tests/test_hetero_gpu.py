"""Components of one tile coded with parameters of their own (COC / QCC) through the device layer, against the CPU
oracle: 5/3 and fixed point exactly, 9/7 float by the rule of test_stage_planes_match_oracle.

The branches this reaches (ffmpeg-ht_amd/csrc/htj2k_device.hip):
 * build_descriptors: a packed or MCT tile whose components differ in levels or wavelet stays out of the fused plan (plain
   launches at every level, k_mct_pack afterwards) while the other tiles and frames of the job stay in it; the ping-pong
   parity of the final buffer differs per component; a plane without levels is packed from where the block decoder wrote it
 * the pack table carries a transform per component: float and int32 planes in one tile
 * the job-wide gates: 16-bit sub-bands, two blocks per wave, k_ht_decode_multi, the narrow VLC kernel -- one component
   with wide blocks, M_b above 15 or 9/7 demotes exactly its job
tests/test_gpu_parity.py::test_frames_match_oracle runs every streams.HET entry in the four IDWT modes as well.
Every test decodes pictures of its own (a seed per test): a job's device buffers are not cleared, and what an earlier run
of the same pictures left behind holds the right answer (tests/test_decode_many_tiles_gpu.py)."""
import ctypes

import numpy as np
import pytest

import oracle
import streams
import vecgen
from test_gpu_parity import damaged_bodies_match_the_oracle, dec, stage_planes_match_oracle  # noqa: F401  (dec: fixture)

pytestmark = pytest.mark.gpu

YUV = dict(dx=[1, 2, 2], dy=[1, 2, 2])


def het(name, seed, **more):
    """the stream of streams.HET[name] over a picture of the same shape from another seed -> (codestream, decode keywords)"""
    args, kw, dkw = streams.HET[name]
    args = args[:4] + (seed,) + args[5:]
    return streams._enc(args, **dict(kw, **more)), dkw


def same_frames(planes, want, what):
    assert len(planes) == len(want), what
    for a, b in zip(planes, want):
        assert np.array_equal(a, b), what


STAGE = ["het_rgb_levels_530", "het_rgb_mct_levels_424", "het_rgb_ict_levels_424", "het_rgb_ict_levels_424_bitexact",
         "het_yuv420_levels_250", "het_rgba_levels_3331", "het_rgb_deep_vs_none", "het_rgb_53_97_97", "het_rgb_53_97_97_bitexact",
         "het_rgb_mct_flag_wavelets_differ", "het_rgb_guard_125", "het_rgb_97_qsteps", "het_rgb10_expn_bias"]


@pytest.mark.parametrize("name", STAGE)
def test_stage_planes_match_oracle(dec, orc, name):
    """dequantised sub-bands and IDWT output of every plane, in the three IDWT modes: planes of 0 to 8 levels, float next
    to int32 next to fixed point, step sizes and guard bits of their own.  (A plane without levels comes out of the IDWT
    stage as the block decoder left it.)"""
    data, kw = het(name, 100 + STAGE.index(name))
    stage_planes_match_oracle(dec, orc, data, kw)


# ---------------------------------------------------------------- job-wide gates
FAST = (256, 96)                  # every level of three: even origin, widths a multiple of 4 (the fast geometry)


def _fast(seed, **kw):
    return vecgen.encode(vecgen.synth_image(FAST[0], FAST[1], 3, seed=seed, noise=10), **dict(dict(mct=1, nlevels=3), **kw))


# name -> (encode keywords of a frame on the fast geometry, blocks per wave of the HT kernel its job gets with 32-bit
# sub-bands: 2 / 4 = k_ht_decode_multi over blocks of up to 64 / 32 columns, 1 = the kernel of a block per wave)
DEMOTE = {
    # the tile is not fusable (the three components of a packed MCT tile must agree in levels): no 16-bit sub-bands
    "levels_313":  (dict(comp=[None, dict(nlevels=1), None]), 2),
    # M_b = 8 + 1 (RCT) + 2 (HH) + 2 (bias) + 5 - 1 = 17 > 15 in component 2
    "guard_5":     (dict(comp=[None, None, dict(guard_bits=5, expn_bias=2)]), 2),
    # blocks of 128 columns in component 1: neither 16-bit sub-bands nor several blocks per wave nor the narrow VLC kernel
    "cb_256x16":   (dict(comp=[None, dict(cb=(8, 4)), None]), 1),
    # a 9/7 plane between two 5/3 ones (no component transform): blocks of two transforms
    "wavelet_97":  (dict(mct=0, comp=[None, dict(transform=0, qstep=1), None]), 1),
    # 64 x 64 tiles, some components with fewer levels: the unfusable tiles of a job whose other tiles are fused
    # (blocks of 32 columns at most: four per wave)
    "tiles_313":   (dict(tile=(64, 64), comp=[None, dict(nlevels=3), dict(nlevels=1)]), 4),
}


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", sorted(DEMOTE))
def test_heterogeneous_frame_between_homogeneous_frames(dec, orc, case, fuse):
    """Two homogeneous frames alone take 16-bit sub-bands, two blocks per wave and the packed final level (with the fused
    pack stage; without it 32-bit sub-bands and k_ht_decode_multi).  With a heterogeneous frame between them the job is
    demoted -- which way is asserted, so that a case that stops reaching its branch is noticed -- and every frame of it
    equals the oracle's"""
    seed = 200 + 10 * sorted(DEMOTE).index(case) + fuse
    kw, bpw = DEMOTE[case]
    tile = dict(tile=kw["tile"]) if "tile" in kw else {}
    pkts = [_fast(seed, **tile), _fast(seed + 3, **kw), _fast(seed + 6, **tile)]
    want = [orc.decode(p)[1] for p in pkts]
    assert orc.block_errors() == 0
    dec.set_int("fuse_pack", fuse)
    try:
        job = dec.job().parse_batch([pkts[0], pkts[2]]).upload().run().wait()
        alone = 2 if fuse or not tile else 4                    # k_ht_decode_pair, or k_ht_decode_multi by the widest block
        assert job.coef16() == bool(fuse) and job.ht_blocks_per_wave() == alone and job.block_errors() == 0, (job.coef16(), job.ht_blocks_per_wave())
        assert (job.idwt_packed() > 0) == bool(fuse)
        same_frames(job.download_frame(0)[1], want[0], (case, "alone", 0))
        same_frames(job.download_frame(1)[1], want[2], (case, "alone", 1))
        job.free()
        job = dec.job().parse_batch(pkts).upload().run().wait()
        assert job.block_errors() == 0
        assert not job.coef16() and job.ht_blocks_per_wave() == bpw and job.idwt_packed() == 0, (job.coef16(), job.ht_blocks_per_wave())
        for f in range(3):
            same_frames(job.download_frame(f)[1], want[f], (case, fuse, f))
        job.free()
    finally:
        dec.set_int("fuse_pack", 1)


def test_fast_heterogeneous_job_keeps_16_bit_sub_bands(dec, orc):
    """components that differ in levels only, each a group of its own (4:2:0 planes, levels [5, 4, 1]), on the fast geometry:
    nothing demotes the job, the first three levels of the two deep planes run as one launch next to a plane whose only
    level is its final one"""
    img = vecgen.synth_image(256, 128, 3, seed=301, noise=10, **YUV)
    data = vecgen.encode(img, width=256, height=128, comp=[dict(nlevels=5), dict(nlevels=4), dict(nlevels=1)], **YUV)
    want = orc.decode(data)[1]
    launches = {}
    try:
        for x3 in (1, 0):
            dec.set_int("idwt_x3", x3)
            job = dec.job().parse_batch([data, data]).upload().run().wait()
            assert job.coef16() and job.ll16() == 1 and job.ht_blocks_per_wave() == 2 and job.block_errors() == 0
            launches[x3] = len(job.idwt_launches())
            for f in range(2):
                same_frames(job.download_frame(f)[1], want, (x3, f))
            job.free()
    finally:
        dec.set_int("idwt_x3", 1)
    assert launches[1] == launches[0] - 2, launches                         # levels 0-2 of the two deep planes as one launch
    for c in range(3):
        assert np.array_equal(want[c], img[c])


# ---------------------------------------------------------------- knobs
KNOBS = [("coef16", 0), ("ll16", 0), ("idwt_x3", 0), ("idwt_pk", 0), ("ht_pair", 0), ("ht_multi", 0), ("ht_mode", 0), ("device_gather", 0),
         ("idwt_mode", 0), ("idwt_mode", 1), ("fuse_pack", 0)]
DEFAULTS = dict(coef16=1, ll16=1, idwt_x3=1, idwt_pk=1, ht_pair=1, ht_multi=1, ht_mode=1, device_gather=1, idwt_mode=3, fuse_pack=1)


def _knob_streams():
    """(name, codestream, blocks per wave with 32-bit sub-bands): the two catalogue cases (blocks of 64 columns: two per
    wave), both again with 32 x 32 blocks (four per wave), and the 4:2:0 job on the fast geometry that keeps its 16-bit
    sub-bands, so that coef16 / ll16 / idwt_x3 / idwt_pk / ht_pair switch something"""
    out = []
    for i, name in enumerate(("het_rgb_mct_levels_424", "het_yuv420_levels_250")):
        out.append((name, het(name, 400 + i)[0], 2))
        out.append((name + "_cb32", het(name, 410 + i, cb=(5, 5))[0], 4))
    img = vecgen.synth_image(256, 128, 3, seed=420, noise=10, **YUV)
    out.append(("yuv420_fast_levels_541", vecgen.encode(img, width=256, height=128, comp=[dict(nlevels=5), dict(nlevels=4), dict(nlevels=1)], **YUV), 2))
    return out


def test_knobs_leave_heterogeneous_frames_alone(dec, orc):
    """every knob at its other value, one at a time: the oracle's frames.  ht_multi switches between the kernel of a block
    per wave and k_ht_decode_multi with two (64-column blocks) and four (32-column blocks) per wave"""
    try:
        for name, data, nb in _knob_streams():
            want = orc.decode(data)[1]
            fast = name == "yuv420_fast_levels_541"
            for knob, value in [(None, None)] + KNOBS:
                if knob:
                    dec.set_int(knob, value)
                job = dec.job().parse_batch([data, data]).upload().run().wait()
                c16 = fast and knob not in ("coef16", "ht_mode", "idwt_mode", "fuse_pack")
                assert job.coef16() == c16, (name, knob, job.coef16())
                bpw = (2 if knob != "ht_pair" else 1) if c16 else (1 if knob in ("ht_multi", "ht_mode") else nb)
                assert job.ht_blocks_per_wave() == bpw, (name, knob, job.ht_blocks_per_wave(), bpw)
                assert job.block_errors() == 0
                for f in range(2):
                    same_frames(job.download_frame(f)[1], want, (name, knob, f))
                job.free()
                if knob:
                    dec.set_int(knob, DEFAULTS[knob])
    finally:
        for knob, value in DEFAULTS.items():
            dec.set_int(knob, value)


# ---------------------------------------------------------------- other entry points
ENTRY = ["het_rgb_mct_levels_424", "het_rgb_53_97_97", "het_yuv420_levels_250", "het_rgb_cb_64x64_256x16_4x1024"]


def test_one_call_path_and_padded_lines(dec, orc):
    """htj2k_decode into lines of the picture's own length and into lines padded to 64 and 256 bytes"""
    for i, name in enumerate(ENTRY):
        data, kw = het(name, 500 + i)
        info_o, want, consumed_o = orc.decode(data, **kw)
        for align in (1, 64, 256):
            info, planes, consumed, st = dec.decode(data, align=align)
            assert consumed == consumed_o and st.n_block_errors == 0
            same_frames(planes, want, (name, align))


def test_pipe_host_and_device_frames(dec, orc):
    """the pipeline entry points: heterogeneous frames between homogeneous ones in batches of four, received into host
    frames and as device frames"""
    import ffmpeg_ht_amd as m
    names = ENTRY[:3] + ["rgb_mct", "het_rgb_guard_125", "gray_l5_cb64", "het_rgb_tiles_coc_in_tile_hdr", "yuv420p8", "het_rgba_levels_3331"]
    pkts = [het(n, 600 + i)[0] if n in streams.HET else streams.get(n)[0] for i, n in enumerate(names)]
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
                same_frames(planes, want[got], (names[got], device))
                got += 1
        finally:
            pipe.close()


def test_damaged_bodies_of_a_stream_with_three_block_shapes(dec, orc):
    """the mutation of test_damaged_ht_bodies_match_the_oracle, with its two carve-outs and no other, on 64 x 64, 256 x 16
    and 4 x 1024 blocks in one tile: the same error code, or the same pixels and the same number of rejected blocks"""
    data, kw = het("het_rgb_cb_64x64_256x16_4x1024", 700)
    same, carved, rejected = damaged_bodies_match_the_oracle(dec, orc, np.random.default_rng(12), "het_rgb_cb_64x64_256x16_4x1024", data, kw)
    assert same >= 15 and carved < same // 4, (same, carved, rejected)


def test_reduction_factor_up_to_the_smallest_component(dec, orc):
    """levels [4, 2, 3]: reduction_factor 1 and 2 decode as the oracle does (at 2 one plane has no level left), 3 is
    refused with the oracle's code"""
    import ffmpeg_ht_amd as m
    data, _ = het("het_rgb_rlcp_levels_prec", 800)
    try:
        for red in (1, 2):
            dec.set_int("reduction_factor", red)
            info_o, want, _ = orc.decode(data, reduction_factor=red)
            info, planes, _, st = dec.decode(data)
            assert (info.width, info.height) == (info_o.width, info_o.height) and st.n_block_errors == 0
            same_frames(planes, want, red)
        dec.set_int("reduction_factor", 3)
        with pytest.raises(oracle.DecodeError) as eo:
            orc.decode(data, reduction_factor=3)
        with pytest.raises(m.Htj2kError) as eg:
            dec.decode(data)
        assert eo.value.code == eg.value.code == -22
    finally:
        dec.set_int("reduction_factor", 0)
