"""Jobs used more than once: second calls, split stages, changed knobs, re-parses, several jobs in flight.

An htj2k_job remembers what its last run did (16-bit or 32-bit sub-bands, which buffer each plane ended in, whether the
final level was fused with the pack stage, what the LL overflow check said), and the next call decides from that and from
the knobs as they are then which kernel reads which buffer.  The kernels are pinned to the oracle elsewhere, on jobs that
run once; here the same few small streams go through one job again and again, and after every call the frame
(orc.decode), the planes behind the block stage (orc.decode_blocks / orc.plane) or behind the IDWT (orc.idwt) must be the
oracle's, bit for bit -- the 9/7 float path included, as in test_stage_planes_match_oracle.

The rule under test ("A job used again"): a stage call gives the right result or returns
HTJ2K_ERR_EINVAL without launching anything.  Which sequences may take the second way out is MAY_REFUSE below.

Dirty rule.  A call that writes nothing would find the previous call's answer still in the output planes.  Between the
first run and the sequence under test the device planes of every frame (htj2k_job_device_frame) are therefore filled
with 0xA5 bytes (dirty(): hipMemset of the HIP runtime the process has loaded, then hipDeviceSynchronize);
test_dirty_fills_the_frame proves the helper.  One pass of the re-parse cycle also runs in a child process under
HTJ2K_POISON=1, where every fresh device buffer starts as 0xA5 bytes.

Every test first asserts that its job is on the path it is there for (PATHS): 16-bit sub-bands, 16-bit LL bands, the
packed final level, blocks per wave of the MagSgn kernel, the number of IDWT launches.  Run as a program the module runs
the re-parse cycle on a decoder of its own (the poison pass)."""
import contextlib
import ctypes
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.dirname(HERE)]

import oracle
import streams
import vecgen

pytestmark = pytest.mark.gpu

EINVAL = -22
DEFAULTS = dict(idwt_mode=3, fuse_pack=1, coef16=1, ll16=1, idwt_pk=1, idwt_x3=1, idwt_x2=2, ht_mode=1, ht_pair=1, ht_multi=1,
                ll16_test_bits=16)


@contextlib.contextmanager
def knobs(dec, **ints):
    """set_int knobs for the calls inside; all of DEFAULTS are back when the block ends (the body may set more)"""
    assert not set(ints) - set(DEFAULTS), ints
    try:
        for k, v in ints.items():
            dec.set_int(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            dec.set_int(k, v)


# ------------------------------------------------------------------ the streams: the smallest that still take each path
def _rgb(w, h, nl, seed):
    return vecgen.encode(vecgen.synth_image(w, h, 3, seed=seed, noise=10), mct=1, nlevels=nl)


def _yuv420():
    img = vecgen.synth_image(512, 256, 3, seed=12, dx=[1, 2, 2], dy=[1, 2, 2])
    return vecgen.encode(img, nlevels=3, dx=[1, 2, 2], dy=[1, 2, 2], width=512, height=256)


STREAMS = {
    "S1": lambda: _rgb(64, 48, 2, 64 + 48),             # the smallest coef16 + ll16 job of test_gpu_parity._coef16_streams
    "S2": lambda: _rgb(256, 192, 4, 256 + 192),         # + the three-level launch and the packed final level
    "S2b": lambda: _rgb(256, 192, 4, 7),                # S2's geometry, another picture
    "S3": lambda: streams.get("rgb_mct")[0],            # 190 x 131: odd geometry, 32-bit sub-bands, fused
    "S4": lambda: streams.get("rgb_97_ict")[0],         # the float path
    "S5": lambda: streams.get("p1_rgb_mct")[0],         # Part-1 blocks
    "S6": lambda: streams.get("rgb_3passes_cb32")[0],   # the refine kernel
    "S7": _yuv420,                                      # 4:2:0 512 x 256: planes of two sizes, 8-bit plane stores
    "S8": lambda: streams.get("gray16")[0],             # M_b > 15
}

# (coef16(), ll16(), idwt_packed() != 0, ht_blocks_per_wave(), len(idwt_launches())) of a fresh job after run(7) under
# default knobs.  The first three are what test_gpu_parity asserts for these streams (test_coef16_jobs_match_...,
# test_coef16_is_not_used_where_it_does_not_apply, test_ll16_jobs_..., test_final_level_on_pairs_...); launches: one per level,
# levels 0-2 of a job with 16-bit LL bands as one (test_first_three_idwt_levels_in_one_launch: nl - 2), the fused final
# level of S3 / S4 / S5 / S6 one launch, of S8 (a 16-bit plane store) and S7 (three 8-bit planes) one as well; blocks per
# wave: 2 = k_ht_decode_pair with 16-bit sub-bands, 0 = no HT block, else what job_ht_eligibility allows
# k_ht_decode_multi (2 up to 64 columns, 4 up to 32), as htj2k_job_ht_blocks_per_wave documents
PATHS = {
    "S1": (True, 1, True, 2, 2),
    "S2": (True, 1, True, 2, 2),
    "S2b": (True, 1, True, 2, 2),
    "S3": (False, 0, False, 2, 5),
    "S4": (False, 0, False, 2, 5),
    "S5": (False, 0, False, 0, 5),
    "S6": (False, 0, False, 4, 5),
    "S7": (True, 1, True, 2, 3),
    "S8": (False, 0, False, 2, 4),
}


@functools.lru_cache(maxsize=None)
def stream(name):
    return STREAMS[name]()


_REF = {}


def ref(orc, name):
    """the oracle's answers for a stream, computed once: (frame planes, planes behind the block stage, planes behind the IDWT)"""
    if name not in _REF:
        data = stream(name)
        frame = [np.array(p, copy=True) for p in orc.decode(data)[1]]
        orc.decode_blocks(data)
        blocks = [np.array(orc.plane(tc), copy=True) for tc in range(orc.num_tilecomps())]
        orc.idwt()
        planes = [np.array(orc.plane(tc), copy=True) for tc in range(orc.num_tilecomps())]
        _REF[name] = (frame, blocks, planes)
    return _REF[name]


def path_of(job):
    return (job.coef16(), job.ll16(), job.idwt_packed() != 0, job.ht_blocks_per_wave(), len(job.idwt_launches()))


def check_path(job, names):
    """the accessors after run(7) under default knobs; a batch: every frame on the first name's path but for the launches"""
    got, want = path_of(job), PATHS[names[0]]
    assert got == want if len(names) == 1 else got[:3] == want[:3], (names, got, want)


def check_frames(job, orc, names, what=""):
    for f, name in enumerate(names):
        planes = job.download_frame(f)[1]
        want = ref(orc, name)[0]
        assert len(planes) == len(want)
        for p, (a, b) in enumerate(zip(planes, want)):
            assert a.dtype == b.dtype and np.array_equal(a, b), "frame %d (%s) plane %d: %s" % (f, name, p, what)


def check_planes(job, orc, names, which, what=""):
    """every plane(tc) of the job against the oracle's planes behind the block stage (which = 1) or the IDWT (2)"""
    want = [p for name in names for p in ref(orc, name)[which]]
    assert job.num_tilecomps() == len(want)
    for tc, b in enumerate(want):
        a = job.plane(tc)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), "plane %d: %s" % (tc, what)


# ------------------------------------------------------------------ the dirty rule
def _hip():
    """the HIP runtime libhtj2k_amd.so has brought into the process"""
    with open("/proc/self/maps") as fh:
        paths = {line.split()[-1] for line in fh if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths.pop())
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    return hip


def dirty(dec, job, nframes=1):
    """0xA5 into every byte of the device planes of the job's frames; call after wait()"""
    import ffmpeg_ht_amd as m
    hip = _hip()
    for f in range(nframes):
        info, fr = job.frame_info(f), m.Frame()
        assert dec.L.htj2k_job_device_frame(dec.h, job.h, f, ctypes.byref(fr)) == 0
        for p in range(info.nplanes):
            assert hip.hipMemset(fr.data[p], 0xA5, fr.linesize[p] * info.plane_height[p]) == 0
    assert hip.hipDeviceSynchronize() == 0


def is_dirty(job, nframes=1):
    return all((p.view(np.uint8) == 0xA5).all() for f in range(nframes) for p in job.download_frame(f)[1])


@pytest.fixture(scope="module")
def dec():
    import ffmpeg_ht_amd as m
    d = m.Decoder()
    assert d.device_name().startswith("gfx950"), d.device_name()
    yield d
    d.close()


def first_run(dec, orc, names, job=None):
    """parse, upload, run(7), wait under default knobs; the path, the frames; then the planes dirtied"""
    job = job or dec.job()
    (job.parse(stream(names[0])) if len(names) == 1 else job.parse_batch([stream(n) for n in names])).upload().run(7).wait()
    check_path(job, names)
    assert job.block_errors() == 0
    check_frames(job, orc, names, "first run")
    dirty(dec, job, len(names))
    return job


def test_dirty_fills_the_frame(dec, orc):
    for name in ("S1", "S7", "S8"):                      # rgb24, three planes of two sizes, a 16-bit plane
        job = first_run(dec, orc, [name])
        planes = job.download_frame(0)[1]
        assert sum(p.nbytes for p in planes) == sum(p.nbytes for p in ref(orc, name)[0]) > 0
        assert is_dirty(job), name
        job.run(7).wait()
        check_frames(job, orc, [name], "after the dirt")
        job.free()


# ------------------------------------------------------------------ 1. second calls on one job
KNOB_CASES = [("idwt_mode", 0), ("idwt_mode", 1), ("fuse_pack", 0), ("coef16", 0), ("ll16", 0), ("idwt_pk", 0), ("idwt_x3", 0),
              ("idwt_x2", 1), ("ht_mode", 0), ("ht_pair", 0), ("ht_multi", 0)]
SEQUENCES = ["run7_x3", "run6", "run2_run4", "run4", "run5", "run1_run6"] + ["%s_%d" % k for k in KNOB_CASES]
# The sequences that may be refused (HTJ2K_ERR_EINVAL, nothing written) instead of giving the frame: their mask lacks a
# stage that the results of the run before -- a run of 7 whose final level was fused with the pack stage and never wrote the
# final planes -- cannot stand in for.  This set does not grow to make a test pass.
MAY_REFUSE = {"run4", "run5"}


def refused(job, mask, seq):
    import ffmpeg_ht_amd as m
    try:
        job.run(mask)
    except m.Htj2kError as e:
        assert e.code == EINVAL and seq in MAY_REFUSE, (seq, mask, e)
        return True
    return False


@pytest.mark.parametrize("seq", SEQUENCES)
@pytest.mark.parametrize("name", ["S1", "S2", "S3", "S4", "S5", "S7"])
def test_second_call(dec, orc, name, seq):
    names = [name]
    with knobs(dec):
        job = first_run(dec, orc, names)
        if seq == "run7_x3":
            job.run(7).run(7).run(7).wait()
        elif seq == "run6":
            job.run(6).wait()
        elif seq == "run2_run4":
            job.run(2).wait()
            check_planes(job, orc, names, 2, "run(2) after run(7)")
            assert is_dirty(job)                            # the IDWT alone writes no frame
            job.run(4).wait()
        elif seq in ("run4", "run5"):
            if refused(job, int(seq[3]), seq):
                job.wait()
                assert is_dirty(job), "a refused call wrote to the frame"
                job.run(7).wait()
            else:
                job.wait()
        elif seq == "run1_run6":
            job.run(1).wait()
            check_planes(job, orc, names, 1, "run(1) after run(7)")
            assert is_dirty(job)
            job.run(6).wait()
        else:
            knob = next(k for k in KNOB_CASES if "%s_%d" % k == seq)
            dec.set_int(*knob)
            job.run(6).wait()
            check_frames(job, orc, names, "run(6) after %s = %d" % knob)
            dirty(dec, job)
            job.run(7).wait()
        check_frames(job, orc, names, seq)
        assert job.block_errors() == 0
        job.free()


@pytest.mark.parametrize("name", ["S1", "S3"])
def test_split_stages_after_runs_that_were_not_fused(dec, orc, name):
    """the other half of the rule: where the run before left what the mask needs, the call is NOT refused.  The pack stage
    alone after an IDWT run that wrote its planes (fuse_pack 0, idwt_mode 0); with the block stage in front (5) where that
    writes over no plane; the IDWT alone twice in a row under idwt_mode 0, whose kernels transform in place; and the pack
    stage refused once a block stage has run since the planes were made"""
    names = [name]
    with knobs(dec):
        job = first_run(dec, orc, names)
        dec.set_int("fuse_pack", 0)
        for mask in (7, 4, 5, 6):                           # planes in the IDWT's buffers: 5 keeps them
            job.run(mask).wait()
            check_frames(job, orc, names, "fuse_pack 0, run(%d)" % mask)
            dirty(dec, job)
        check_planes(job, orc, names, 2, "fuse_pack 0")
        dec.set_int("idwt_mode", 0)
        for mask in (2, 2, 4, 6):                           # in place: the second IDWT needs the sub-bands back
            job.run(mask).wait()
            check_planes(job, orc, names, 2, "idwt_mode 0, run(%d)" % mask)
            if mask & 4:
                check_frames(job, orc, names, "idwt_mode 0, run(%d)" % mask)
                dirty(dec, job)
        for mask in (5, 1, 4):                              # 5 would write over the planes; after 1 there are none
            if mask == 1:
                job.run(1).wait()
                check_planes(job, orc, names, 1, "idwt_mode 0, run(1)")
                continue
            assert refused(job, mask, "run%d" % mask), mask
            job.wait()
            assert is_dirty(job), "a refused call wrote to the frame"
        job.run(7).wait()
        check_frames(job, orc, names, "idwt_mode 0, run(7)")
        job.free()


# ------------------------------------------------------------------ 2. the overflow re-run
@pytest.mark.parametrize("knob", [("idwt_mode", 0), ("fuse_pack", 0)], ids=["idwt_mode_0", "fuse_pack_0"])
@pytest.mark.parametrize("name", ["S1", "S2"])
def test_overflow_rerun_does_not_follow_knobs_changed_before_wait(dec, orc, name, knob):
    with knobs(dec):
        job = first_run(dec, orc, [name])
        dec.set_int("ll16_test_bits", 6)                   # ordinary LL samples "overflow"
        job.run(7)
        dec.set_int(*knob)
        job.wait()
        check_frames(job, orc, [name], "overflow, then %s = %d before wait()" % knob)
        assert job.ll16() == 2
        job.free()


@pytest.mark.parametrize("name", ["S1", "S2"])
def test_overflow_then_runs_that_do_not(dec, orc, name):
    with knobs(dec):
        job = first_run(dec, orc, [name])
        dec.set_int("ll16_test_bits", 6)
        job.run(7).run(7).wait()
        check_frames(job, orc, [name], "two runs that overflow, one wait")
        assert job.coef16() and job.ll16() == 2
        dirty(dec, job)
        dec.set_int("ll16_test_bits", 16)
        job.run(7).wait()
        check_frames(job, orc, [name], "16 bits again")
        assert path_of(job) == PATHS[name]                 # ll16() == 1: this run did not overflow
        dirty(dec, job)
        dec.set_int("ll16", 0)
        job.run(7).wait()
        check_frames(job, orc, [name], "ll16 = 0")
        assert job.coef16() and job.ll16() == 0            # ... and this one kept no 16-bit LL bands at all
        job.free()


# ------------------------------------------------------------------ 3. one job, many contents
CONTENTS = [(["S2"], {}), (["S4"], {}), (["S5"], {}), (["S1"], {}), (["S8"], {}), (["S7"], {}), (["S6"], {}), (["S1", "S3", "S4"], {}),
            (["S2"], dict(ll16_test_bits=6)), (["S4"], {}), (["S2"], {})]


def one_job_many_contents(dec, orc):
    job = dec.job()
    for step, (names, kn) in enumerate(CONTENTS):
        what = "content %d %r %r" % (step, names, kn)
        with knobs(dec, **kn):
            job.parse(stream(names[0])) if len(names) == 1 else job.parse_batch([stream(n) for n in names])
            job.upload().run(1).wait()
            check_planes(job, orc, names, 1, what + ": run(1)")           # (a stale fused_last used to refuse these planes)
            job.upload().wait()
            dirty(dec, job, len(names))
            job.run(7).wait()
            check_frames(job, orc, names, what + ": run(7)")
            assert job.block_errors() == 0
            fresh = dec.job()
            (fresh.parse(stream(names[0])) if len(names) == 1 else fresh.parse_batch([stream(n) for n in names])).upload().run(7).wait()
            assert path_of(job) == path_of(fresh), what                   # (ll16_fallbacks used to outlive its content)
            if not kn and len(names) == 1:
                assert path_of(fresh) == PATHS[names[0]], what
            if kn:
                assert fresh.ll16() == 2, what
            fresh.free()
    job.free()


def test_one_job_many_contents(dec, orc):
    one_job_many_contents(dec, orc)


# Measured on an MI355X: the cycle takes 0.2 s in the suite's process and the child under HTJ2K_POISON=1 0.9 s from start to
# end (interpreter, library, the fill that waits for the device at every allocation); the child gets many times that
POISON_TIMEOUT = 30


def test_one_job_many_contents_on_poisoned_buffers():
    """HTJ2K_POISON=1 (read once per process, so a child): every fresh device buffer starts as 0xA5 bytes"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=POISON_TIMEOUT,
                       env=dict(os.environ, HTJ2K_POISON="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "poisoned buffers: ok" in r.stdout, r.stdout[-3000:]


# ------------------------------------------------------------------ 4. several jobs of one decoder in flight
def test_several_jobs_in_flight(dec, orc):
    held = ["S1", "S2", "S2b", "S4"]
    with knobs(dec):
        jobs = [first_run(dec, orc, [n]) for n in held]

        def all_waits_then_frames(what):
            for j in jobs:
                j.wait()
            for j, n in zip(jobs, held):
                check_frames(j, orc, [n], what)
                dirty(dec, j)

        for _ in range(3):                                  # three rounds of run(7) on each in turn, no wait
            for j in jobs:
                j.run(7)
        all_waits_then_frames("three rounds of run(7)")
        for j, n in zip(jobs, held):
            assert path_of(j) == PATHS[n], n
        for j in jobs:
            j.run(1)
        for j in jobs:
            j.run(6)
        all_waits_then_frames("run(1) on all, run(6) on all")
        # two of the jobs swap contents by re-parse while the other two have a run outstanding
        jobs[1].run(7)
        jobs[2].run(7)
        held[0], held[3] = held[3], held[0]
        for i in (0, 3):
            jobs[i].parse(stream(held[i])).upload().run(7)
        all_waits_then_frames("S1 and S4 swapped")
        for j in jobs:
            j.free()


def test_two_threads_with_a_decoder_each(orc):
    """two host threads, a Decoder of its own on device 0 and two jobs of different geometry each; the iteration counts
    are fixed: this is no stress loop"""
    import ffmpeg_ht_amd as m
    plan = [["S2", "S1"], ["S7", "S3"]]
    for names in plan:
        for n in names:
            ref(orc, n)                                     # the oracle is not shared between threads: computed here
    errors = []

    def work(names):
        try:
            d = m.Decoder()
            jobs = [d.job().parse(stream(n)).upload() for n in names]
            for rnd in range(3):
                for j in jobs:
                    j.run(7)
                for j, n in zip(jobs, names):
                    j.wait()
                    assert path_of(j) == PATHS[n], (n, path_of(j))
                    check_frames(j, None, [n], "thread round %d" % rnd)
                    dirty(d, j)
            for j in jobs:
                j.free()
            d.close()
        except BaseException as e:                          # noqa: B902 -- handed to the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(names,)) for names in plan]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]


# ------------------------------------------------------------------ 5. refusals that exist today stay refusals
def test_refusals_leave_the_job_usable(dec, orc):
    import ffmpeg_ht_amd as m
    name = "S2"
    with knobs(dec):
        job = dec.job().parse(stream(name))
        with pytest.raises(m.Htj2kError) as e:              # run before upload, on a fresh job ...
            job.run(7)
        assert e.value.code == EINVAL
        job.upload().run(7).wait()
        check_path(job, [name])
        check_frames(job, orc, [name], "after run before upload")
        dirty(dec, job)
        job.parse(stream(name))                             # ... and on one that has run: a parse asks for an upload again
        for mask in (7, 6, 4, 1):
            with pytest.raises(m.Htj2kError) as e:
                job.run(mask)
            assert e.value.code == EINVAL
        job.upload().wait()
        dirty(dec, job)
        job.run(7).wait()
        check_frames(job, orc, [name], "after run before upload on a used job")
        dirty(dec, job)
        for tc in range(job.num_tilecomps()):               # plane() of a fused plane after run(7)
            with pytest.raises(m.Htj2kError) as e:
                job.plane(tc)
            assert e.value.code == EINVAL
        job.run(7).wait()
        check_frames(job, orc, [name], "after plane() of fused planes")
        dirty(dec, job)
        info = job.frame_info(0)                            # download_frame with a short linesize
        planes, fr = m.alloc_frame(info)
        fr.linesize[0] = info.plane_width[0] * info.plane_bytes_per_sample[0] - 1
        assert dec.L.htj2k_job_download_frame(dec.h, job.h, 0, ctypes.byref(fr)) == EINVAL
        assert is_dirty(job)
        job.run(7).wait()
        check_frames(job, orc, [name], "after a short linesize")
        job.free()


if __name__ == "__main__":
    import time
    import ffmpeg_ht_amd as m
    t0 = time.time()
    _dec, _orc = m.Decoder(), oracle.OracleDecoder()
    one_job_many_contents(_dec, _orc)
    _dec.close()
    _orc.close()
    print("%s buffers: ok, %.1f s" % ("poisoned" if os.environ.get("HTJ2K_POISON") == "1" else "plain", time.time() - t0))
