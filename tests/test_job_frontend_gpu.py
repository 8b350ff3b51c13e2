"""The host front end of a job: htj2k_job_parse_batch_ex's staging paths, its refusals, and the reads of device state that
need an upload ("A job used again", and section 4, "The parse in steps").

A packet reaches the device one of three ways.  The solo path: one pageable packet of at least 4 MiB with the device
gathering, copied in pieces by helper threads and sent on while the caller's thread parses.  The general path: every packet
staged in page-locked memory, sent on, then parsed, a frame per thread.  Host gather: the parser gathers the code-block
bytes itself and no packet travels.  Which host buffer a copy reads (FrameSlot::h2d_own, h2d_src), where it lands
(pkt_base) and whether the upload still has to send it (pkt_h2d_issued) are state of the job, so one job goes through all
of them in turn here.  Every stream is lossless and every frame is compared with the picture that was encoded."""
import functools
import math

import numpy as np
import pytest

import vecgen

pytestmark = pytest.mark.gpu

EINVAL = -22
SOLO_MIN_BYTES = 4 << 20                                   # the threshold of the solo path (htj2k_device.hip)
# 1500 x 1000 rgb24 is 4 500 000 bytes of uniform noise.  The reversible colour and wavelet transforms are bijections, so
# a lossless codestream of it cannot be shorter than about the raw size: 7 % above the threshold, whatever the coder does
SOLO_W, SOLO_H = 1500, 1000


@pytest.fixture(scope="module")
def dec():
    import ffmpeg_ht_amd as m
    d = m.Decoder()
    assert d.device_name().startswith("gfx950"), d.device_name()
    yield d
    d.close()


@pytest.fixture(scope="module")
def solo():
    """(codestream, the rgb24 frame it holds): made once by the GPU encoder"""
    import ffmpeg_ht_amd as m
    frame = np.random.default_rng(4).integers(0, 256, (SOLO_H, SOLO_W * 3), dtype=np.uint8)
    enc = m.Encoder()
    data = enc.encode([frame], "rgb24", 8)
    enc.close()
    return data, frame


def _small(w, h, seed, **kw):
    """(lossless rgb24 stream, the frame it holds)"""
    img = vecgen.synth_image(w, h, 3, seed=seed, noise=10)
    return vecgen.encode(img, mct=1, nlevels=2, **kw), np.stack(img, -1).reshape(h, w * 3).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def small_set():
    """three distinct small frames: [(stream, frame)]"""
    return [_small(64, 48, 1), _small(190, 131, 2), _small(256, 192, 3)]


def host_ms_ok(job):
    ms = job.host_ms()
    assert all(math.isfinite(v) and v >= 0 for v in ms), ms


def frames_ok(job, want, what):
    assert job.num_frames() == len(want)
    for f, frame in enumerate(want):
        planes = job.download_frame(f)[1]
        assert len(planes) == 1 and np.array_equal(planes[0], frame), "frame %d: %s" % (f, what)
    assert job.block_errors() == 0


def decoded(job, datas, want, what):
    (job.parse(datas[0]) if len(datas) == 1 else job.parse_batch(datas)).upload().run().wait()
    host_ms_ok(job)
    frames_ok(job, want, what)


# ------------------------------------------------------------------ 1. the solo path
def test_solo_packet(dec, solo):
    data, frame = solo
    assert len(data) >= SOLO_MIN_BYTES, len(data)
    info, planes, consumed, st = dec.decode(data)           # (a) htj2k_decode: a job of one
    assert st.n_block_errors == 0
    assert len(planes) == 1 and np.array_equal(planes[0], frame)
    job = dec.job()
    decoded(job, [data], [frame], "parse of one")           # (b)
    decoded(job, [data, data], [frame, frame], "batch of two")   # (c) two frames: the general path
    try:
        dec.set_int("device_gather", 0)                     # the parser gathers: no packet travels, no solo path
        decoded(job, [data], [frame], "parse of one, host gather")
        assert job.host_ms()[1] == 0                        # ... and no staging copy
    finally:
        dec.set_int("device_gather", 1)
    job.free()


# ------------------------------------------------------------------ 2. one job through every staging path in turn
def test_one_job_through_every_staging_path(dec, solo):
    data, frame = solo
    assert len(data) >= SOLO_MIN_BYTES, len(data)
    batch, want = [d for d, _ in small_set()], [f for _, f in small_set()]
    job = dec.job()
    try:
        decoded(job, [data], [frame], "solo")
        decoded(job, batch, want, "batch after solo")
        decoded(job, [data], [frame], "solo after a batch")
        dec.set_int("device_gather", 0)
        decoded(job, batch, want, "batch, host gather")
        dec.set_int("device_gather", 1)
        decoded(job, batch, want, "batch, device gather again")
        decoded(job, [data], [frame], "solo at the end")
    finally:
        dec.set_int("device_gather", 1)
    job.free()


# ------------------------------------------------------------------ 3. the first failure in submission order
def code_alone(dec, data):
    import ffmpeg_ht_amd as m
    job = dec.job()
    with pytest.raises(m.Htj2kError) as e:
        job.parse(data)
    job.free()
    return e.value.code


def test_first_failure_in_submission_order(dec):
    import ffmpeg_ht_amd as m
    good, want = [d for d, _ in small_set()], [f for _, f in small_set()]
    many = bytearray(good[1])
    assert many[2:4] == b"\xff\x51"                         # SIZ follows SOC: Csiz is 36 bytes into the segment
    many[40:42] = (100).to_bytes(2, "big")                  # a codestream of 100 components
    many, noise = bytes(many), bytes(range(7, 207))         # and bytes that do not begin one
    code_many, code_noise = code_alone(dec, many), code_alone(dec, noise)
    assert code_many < 0 and code_noise < 0 and code_many != code_noise, (code_many, code_noise)
    job = dec.job()
    try:
        for threads in (1, 4):
            dec.set_int("parse_threads", threads)
            for batch, code in (([good[0], many, noise], code_many), ([good[0], noise, many], code_noise)):
                with pytest.raises(m.Htj2kError) as e:
                    job.parse_batch(batch)
                assert e.value.code == code, (threads, e.value.code, code)
            decoded(job, good, want, "a good batch after refused ones, %d threads" % threads)
    finally:
        dec.set_int("parse_threads", 0)
    job.free()


# ------------------------------------------------------------------ 4. refusals between parse and upload
def refused_before_upload(job):
    import ffmpeg_ht_amd as m
    for call in (lambda: job.plane(0), lambda: job.plane(job.num_tilecomps() - 1), lambda: job.download_frame(0), job.download,
                 job.block_errors, lambda: job.device_frame(0)):
        with pytest.raises(m.Htj2kError) as e:
            call()
        assert e.value.code == EINVAL
    assert not job.dec.L.htj2k_job_device_plane(job.h, 0, None)


def test_reads_of_device_state_need_an_upload(dec):
    small, small_frame = small_set()[0]                           # one tile, three tile-components
    large, large_frame = _small(256, 192, 9, tile=(128, 192))   # two tiles, six
    for used in (True, False):                              # a job that has run the small frame; a fresh one
        job = dec.job()
        if used:
            decoded(job, [small], [small_frame], "the small frame")
            assert job.num_tilecomps() == 3
        job.parse(large)
        refused_before_upload(job)
        info = job.frame_info(0)                            # what the parse answers is there
        assert (info.width, info.height) == (256, 192)
        assert job.num_tilecomps() == 6 and job.num_blocks() > 0 and job.num_frames() == 1
        job.upload().run().wait()
        frames_ok(job, [large_frame], "the large frame, used job: %r" % used)
        assert job.device_frame(0).data[0] and dec.L.htj2k_job_device_plane(job.h, 0, None)
        job.free()
