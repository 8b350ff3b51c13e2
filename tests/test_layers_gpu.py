"""Quality layers (streams.LAYERS) through the device layer, frame for frame equal to the CPU oracle's.  Layers are the one
axis of the stream syntax that changes the shape of the gather table the device reads: a block's bytes are second and
later pieces at any alignment of source and destination (k_gather: the head bytes, the shifted dword copy behind a head,
the tail bytes), Lcup and Lref come from different packets, Scup is read from the end of the cleanup piece, and the
0xFF 0xFF trailers of terminated Part-1 segments go by contribution.
 * every case with device_gather 1 and 0, and once per knob that changes the block stage; a frame that differs is taken
   through the stage planes, so that the failure names the block stage or the transform
 * all cases and their one-layer twins in one job (merged plans, gather segments re-based per frame), the same job run
   twice, and the same packets through a pipe
 * container variants of layered streams (tile-parts, PPM, PPT, TLM + PLT with packet threads on, two progression volumes
   that end at different layers)
 * damaged bodies of four layered cases, by the rules of test_gpu_parity.test_damaged_ht_bodies_match_the_oracle
 * layered Part-1, HT and MIXED sources in the transcoder: the output of their one-layer twins
tests/test_layers_streams.py pins the streams, and what is in them, on the CPU."""
import numpy as np
import pytest

import streams
import vecgen
from test_gpu_parity import damaged_bodies_match_the_oracle, stage_planes_match_oracle
from test_hetero_gpu import DEFAULTS, KNOBS, same_frames
from test_layers_streams import SAME_FRAME, rewritten_layered_streams

pytestmark = pytest.mark.gpu

NAMES = sorted(streams.LAYERS)
EXTERNAL = -0x20545845
# the knobs of test_hetero_gpu.KNOBS that change the block stage
BLOCK_KNOBS = [(k, v) for k, v in KNOBS if k in ("ht_multi", "ht_pair", "ht_mode", "coef16")]


@pytest.fixture(scope="module")
def dec():
    import ffmpeg_ht_amd as m
    d = m.Decoder()
    assert d.device_name().startswith("gfx950"), d.device_name()
    yield d
    d.close()


@pytest.fixture(scope="module")
def want(orc):
    """name -> the oracle's frame of the case, computed once"""
    out = {}
    for n in NAMES:
        info, planes, _ = orc.decode(streams.get(n)[0], **streams.LAYERS[n][2])
        assert orc.block_errors() == 0
        out[n] = [p.copy() for p in planes]
    return out


def _gpu(what, fn):
    """fn(); a failure of the HIP runtime ends the session: nothing more is started on a device that has faulted"""
    import ffmpeg_ht_amd as m
    try:
        return fn()
    except m.Htj2kError as e:
        if e.code == EXTERNAL:
            pytest.exit("HIP runtime failure: %r" % (what,), returncode=3)
        raise


def _options(dec, name):
    dkw = streams.LAYERS[name][2]
    dec.set_int("bitexact", dkw.get("bitexact", 0))
    dec.set_int("reduction_factor", dkw.get("reduction_factor", 0))


def _restore(dec):
    dec.set_int("bitexact", 0)
    dec.set_int("reduction_factor", 0)
    for knob, value in DEFAULTS.items():
        dec.set_int(knob, value)


def _frame(dec, data, what):
    def run():
        job = dec.job().parse(data).upload().run().wait()
        out = job.download_frame(0)[1], job.block_errors()
        job.free()
        return out
    return _gpu(what, run)


def _check(dec, orc, name, want, what):
    data = streams.get(name)[0]
    planes, nerr = _frame(dec, data, what)
    if nerr == 0 and len(planes) == len(want[name]) and all(np.array_equal(a, b) for a, b in zip(planes, want[name])):
        return
    # which stage: the dequantised sub-bands after the block stage, then the planes after the IDWT
    if not streams.LAYERS[name][2].get("reduction_factor"):
        _gpu(what, lambda: stage_planes_match_oracle(dec, orc, data, streams.LAYERS[name][2]))
    assert nerr == 0, what
    same_frames(planes, want[name], what)


@pytest.mark.parametrize("gather", [1, 0], ids=["device_gather", "host_gather"])
@pytest.mark.parametrize("name", NAMES)
def test_frames_match_the_oracle(dec, orc, want, name, gather):
    try:
        _options(dec, name)
        dec.set_int("device_gather", gather)
        _check(dec, orc, name, want, (name, "device_gather", gather))
    finally:
        _restore(dec)


@pytest.mark.parametrize("name", NAMES)
def test_block_stage_knobs(dec, orc, want, name):
    """ht_multi, ht_pair, ht_mode, coef16 at their other value, one at a time: every block kernel a job can take reads
    blocks put together from several packets"""
    try:
        for knob, value in BLOCK_KNOBS:
            _options(dec, name)
            dec.set_int(knob, value)
            _check(dec, orc, name, want, (name, knob, value))
            dec.set_int(knob, DEFAULTS[knob])
    finally:
        _restore(dec)


def _plain(name):
    return not streams.LAYERS[name][2]


def test_one_batch_with_the_one_layer_twins(dec, orc, want):
    """every case that needs no decoder option, each next to its one-layer twin, in one job: merged plans, the gather
    segments of every frame re-based into one table, with device_gather 1 and 0.  The job runs twice (the second run reads
    the byte pool the first one left), and the same packets go through a pipe in batches of eight"""
    names = [n for n in NAMES if _plain(n)]
    assert len(names) >= 36
    pkts, frames = [], []
    for n in names:
        pkts += [streams.get(n)[0], streams.layers_twin(n)]
        frames += [want[n], want[n]]
    try:
        for gather in (1, 0):
            dec.set_int("device_gather", gather)

            def run():
                job = dec.job().parse_batch(pkts).upload()
                for again in (0, 1):
                    job.run(7).wait()
                    assert job.block_errors() == 0, (gather, again)
                    for f in range(len(pkts)):
                        same_frames(job.download_frame(f)[1], frames[f], (names[f // 2], "twin" if f & 1 else "layered", gather, again))
                job.free()
            _gpu(("batch", gather), run)

        def piped():
            pipe = dec.pipe(batch=8, depth=2)
            try:
                sent = got = 0
                while got < len(pkts):
                    while sent < len(pkts) and pipe.send(pkts[sent]):
                        sent += 1
                    if sent == len(pkts):
                        pipe.flush()
                    info, planes = pipe.receive()
                    same_frames(planes, frames[got], (names[got // 2], "pipe", got))
                    got += 1
            finally:
                pipe.close()
        _gpu("pipe", piped)
    finally:
        _restore(dec)


def test_container_variants(dec, orc):
    """the rewritten variants of tests/test_layers_streams.py on the device, alone and all in one job; with packet threads
    on for the ones that carry a PLT list (a layered tile takes the sequential packet reader all the same)"""
    items = [(n, d) for n, d, _ in rewritten_layered_streams() if n.split(".")[1] in SAME_FRAME]
    assert len(items) == 3 * len(SAME_FRAME) - 1
    frames = []
    for n, d in items:
        frames.append([p.copy() for p in orc.decode(d)[1]])
        assert orc.block_errors() == 0
    try:
        for threads in (1, 4):
            dec.set_int("packet_threads", threads)
            for (n, d), w in zip(items, frames):
                if threads > 1 and n.split(".")[1] not in ("plt", "tp3_tlm_plt", "tp_each_packet"):
                    continue
                planes, nerr = _frame(dec, d, (n, threads))
                assert nerr == 0, (n, threads)
                same_frames(planes, w, (n, threads))

            def run():
                job = dec.job().parse_batch([d for _, d in items]).upload().run().wait()
                assert job.block_errors() == 0
                for f, (n, _) in enumerate(items):
                    same_frames(job.download_frame(f)[1], frames[f], (n, threads, "batch"))
                job.free()
            _gpu(("variants", threads), run)
    finally:
        dec.set_int("packet_threads", 1)


DAMAGED = ["lay3_gray_3passes", "lay4_placeholder_2_3p", "p1_lay5_bypass_termall", "mixed_lay3_3passes_vsc"]


@pytest.mark.parametrize("name", DAMAGED)
def test_damaged_bodies(dec, orc, name):
    """24 damaged copies of a layered HT stream of three passes, one with placeholder passes, a Part-1 BYPASS + TERMALL
    one and a MIXED one: the same error code, or the same pixels and the same number of rejected blocks; the two corners
    test_gpu_parity carves out, and no other (a carved frame is still compared, outside the blocks the oracle reports).
    How many frames may be carved: the suite asks for fewer than a quarter of the frames that were the same, over streams
    most of whose blocks have one pass.  Both corners need a block with refinement passes (a backward MagRef reader that
    runs dry, a SigProp neighbour outside the block), and in the two HT cases here every block has them: of the 24 copies
    12 carry 64 random bytes or 400 bytes of 0xFF over about 25 blocks, and each of those may hold such a block, so the
    bound for these two is those 12 copies; the 12 copies with one flipped bit or 8 random bytes are left to the suite's
    rule.  A Part-1 stream has neither corner (0), the MIXED one keeps the suite's quarter.  The one-layer twin of each
    case is damaged the same way and held to the same bounds: the figures belong to the kind of stream, not to layers"""
    ht_refinement = name in ("lay3_gray_3passes", "lay4_placeholder_2_3p")
    for what, data in (("layered", streams.get(name)[0]), ("twin", streams.layers_twin(name))):
        rng = np.random.default_rng([17, DAMAGED.index(name)])
        same, carved, rejected = _gpu(name, lambda: damaged_bodies_match_the_oracle(dec, orc, rng, name, data, streams.get(name)[1]))
        print(name, what, "same", same, "carved", carved, "rejected", rejected)
        assert same + carved + rejected == 24, (name, what, same, carved, rejected)
        if ht_refinement:
            assert same + rejected >= 12 and carved <= 12, (name, what, same, carved, rejected)
        elif streams.LAYERS[name][1].get("part1"):
            assert same >= 15 and carved == 0, (name, what, same, carved, rejected)
        else:
            assert same >= 15 and carved < same // 4, (name, what, same, carved, rejected)


# ---------------------------------------------------------------- the transcoder
XC = {
    "p1":    ((64, 48, 3, 8, 2), dict(mct=1, nlevels=3, cb=(4, 4), part1=True, layers=3, layer_seed=61)),
    "p1_bypass": ((150, 40, 1, 12, 8, 60), dict(depth=12, nlevels=1, cb=(6, 6), part1=True, cblk_style=0x01, layers=4, layer_seed=62)),
    "ht_3p": ((64, 48, 3, 8, 2), dict(mct=1, nlevels=3, cb=(4, 4), transform=0, qstep=1 / 8, passes=3, layers=3, layer_seed=63)),
    "ht_placeholder": ((64, 48, 3, 8, 2), dict(mct=1, nlevels=3, cb=(5, 5), placeholder_sets=1, layers=3, layer_seed=64)),
    "mixed": ((64, 48, 3, 8, 2), dict(mct=1, nlevels=3, cb=(4, 4), mixed=True, layers=3, layer_seed=65)),
}


@pytest.mark.parametrize("name", sorted(XC))
def test_transcoder_takes_layered_sources(dec, orc, name):
    """a layered source and its one-layer twin hold the same blocks with the same passes, and the transcoder's output is a
    function of those (indices, planes and passes per block): the codestream bytes are equal, not only the frames"""
    import ffmpeg_ht_amd as m
    args, kw = XC[name]
    img = streams._img(*args)
    src = vecgen.encode(img, **kw)
    twin = vecgen.encode(img, **dict(kw, layers=1))
    assert src != twin
    ht = not kw.get("part1")
    enc = m.Encoder(device_id=0)
    try:
        a, b = _gpu(name, lambda: enc.transcode(dec, [src, twin], ht_sources=ht))
        assert a == b, name
        fa = [p.copy() for p in orc.decode(a)[1]]
        fb = [p.copy() for p in orc.decode(src)[1]]
        assert orc.block_errors() == 0
        same_frames(fa, fb, name)
        planes, nerr = _frame(dec, a, name)
        assert nerr == 0
        same_frames(planes, fb, name)
    finally:
        enc.close()
