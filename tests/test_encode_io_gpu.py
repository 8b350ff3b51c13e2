"""GPU checks of the encoder's input and output paths and of the loops of the batch path that the other encoder tests
never take twice: rows with padding (host input, and device input with a true stride), the bits of a sample outside
`bits`, output into device memory, the refusals of htj2k_encode_batch, htj2k_encode_frame, calls that take several
rounds (HTJ2K_ENC_ROUND, and once at the real 2^30 samples), and launches over more than 65535 planes.

The reference of every comparison is the encoder's own single-frame, contiguous, host-to-host call, which
tests/test_encode_gpu.py, test_encode_lossy_gpu.py and test_encode_rc_gpu.py pin against vecgen and the CPU rebuild."""
import ctypes
import time

import numpy as np
import pytest
import torch

import enc_frames as ef
import enc_model as em
import ffmpeg_ht_amd as m
from test_encode_gpu import _content

pytestmark = pytest.mark.gpu
PADS = (1, 13, 64)
STRIDE_FORMATS = [("rgb24", 8), ("rgba64le", 16), ("gray", 8), ("yuv420p", 8), ("yuv422p10le", 10)]
TRANSFORMS = [dict(irreversible=False), dict(irreversible=True, qstep=0.5)]
OUT_POISON = 0xAB


@pytest.fixture(scope="module")
def enc():
    e = m.Encoder(0)
    yield e
    e.close()


def case(fmt, bits, w, h, kind="synth", seed=3):
    return em.to_planes(_content(kind, fmt, w, h, bits, seed), fmt, bits)


def stride_batch(make, fmt, sizes, planes):
    """frames of both sizes with a different padding each, per plane too; the last one contiguous"""
    pads = [(1, 13, 64, 1), (13, 64, 1, 13), (64, 1, 13, 64), (0, 0, 0, 0)]
    order = [0, 1, 0, 1]
    made = [make(planes[i], fmt, *sizes[i], pd) for i, pd in zip(order, pads)]
    return order, [f for f, _ in made], made


@pytest.mark.parametrize("opts", TRANSFORMS, ids=["53", "97"])
@pytest.mark.parametrize("fmt,bits", STRIDE_FORMATS)
def test_padded_rows_of_host_frames(enc, fmt, bits, opts):
    """linesize above the row by 1, 13 and 64 bytes (16-bit rows then start at odd addresses), the padding poisoned:
    the upload copies rows, so the bytes are those of the contiguous frame"""
    sizes = [(37, 29), (640, 480)]
    planes = [case(fmt, bits, w, h) for w, h in sizes]
    ref = [enc.encode(p, fmt, bits, **opts) for p in planes]
    for i, (w, h) in enumerate(sizes):
        for pad in PADS:
            fr, keep = ef.padded_frame(planes[i], fmt, w, h, [pad] * 4)
            assert ef.encode_frames(enc, [fr], fmt, bits, **opts) == [ref[i]], (fmt, w, h, pad)
    order, frames, keep = stride_batch(ef.padded_frame, fmt, sizes, planes)
    assert ef.encode_frames(enc, frames, fmt, bits, **opts) == [ref[i] for i in order]


@pytest.mark.parametrize("opts", TRANSFORMS + [dict(irreversible=True, qstep=0.5, target_bytes=-2)], ids=["53", "97", "97-budget"])
@pytest.mark.parametrize("fmt,bits", STRIDE_FORMATS)
def test_device_input_with_a_true_stride(enc, fmt, bits, opts):
    """the same frames in device memory, passed with their linesize: here k_enc_unpack itself reads padded rows
    (host input is repacked by the upload).  target_bytes = -2 stands for half of the larger frame's free size."""
    sizes = [(37, 29), (640, 480)]
    planes = [case(fmt, bits, w, h) for w, h in sizes]
    if opts.get("target_bytes"):
        free = enc.encode(planes[1], fmt, bits, **dict(opts, target_bytes=0))
        opts = dict(opts, target_bytes=len(free) // 2)
    ref = [enc.encode(p, fmt, bits, **opts) for p in planes]
    dev = lambda p, f, w, h, pd: ef.device_frame(p, f, w, h, pd, torch)
    for i, (w, h) in enumerate(sizes):
        for pad in PADS:
            fr, keep = dev(planes[i], fmt, w, h, [pad] * 4)
            assert ef.encode_frames(enc, [fr], fmt, bits, in_on_device=1, **opts) == [ref[i]], (fmt, w, h, pad)
    order, frames, keep = stride_batch(dev, fmt, sizes, planes)
    assert ef.encode_frames(enc, frames, fmt, bits, in_on_device=1, **opts) == [ref[i] for i in order]


@pytest.mark.parametrize("opts", TRANSFORMS, ids=["53", "97"])
@pytest.mark.parametrize("fmt,bits", [("gray", 5), ("gray16le", 12), ("rgb48le", 10), ("ya16le", 10), ("yuv420p10le", 10)])
def test_bits_outside_the_sample_are_not_read(enc, fmt, bits, opts):
    """a sample is `bits` bits of its byte or word, from bit precision - bits up (include/htj2k_amd.h): random values in
    the bits below the shift (gray at 5 bits, gray16le at 12, rgb48le at 10) and in the bits above the sample (ya16le
    and yuv420p10le at 10: bits 10 .. 15 of the word) leave the codestream as it is, from host and from device memory"""
    w, h = 200, 120
    planes = case(fmt, bits, w, h)
    ref = enc.encode(planes, fmt, bits, **opts)
    rng = np.random.default_rng(bits)
    field = ((1 << bits) - 1) << em.shift(fmt, bits)
    dirty = []
    for p in planes:
        junk = rng.integers(0, 1 << (8 * p.itemsize), size=p.shape).astype(p.dtype) & p.dtype.type(~field & ((1 << (8 * p.itemsize)) - 1))
        assert junk.any() and not (p & junk).any()
        dirty.append(p | junk)
    assert enc.encode(dirty, fmt, bits, **opts) == ref
    fr, keep = ef.device_frame(dirty, fmt, w, h, [0] * 4, torch)
    assert ef.encode_frames(enc, [fr], fmt, bits, in_on_device=1, **opts) == [ref]


@pytest.mark.parametrize("opts", [dict(levels=3), dict(levels=3, irreversible=True, qstep=0.25),
                                  dict(levels=3, cb=(4, 4), target_bytes=6000),
                                  dict(levels=3, cb=(4, 4), irreversible=True, qstep=0.25, target_bytes=6000)],
                         ids=["53", "97", "53-budget", "97-budget"])
def test_output_into_device_memory(enc, opts):
    """out_on_device = 1: the bytes and offsets of the host-output call, the buffer behind offsets[n] untouched; a cap one
    byte short answers -28 and writes nothing"""
    fmt, bits = "rgb24", 8
    sizes = [(160, 96), (75, 41), (160, 96), (75, 41)]
    made = [m.frame_from_planes(case(fmt, bits, w, h, seed=s), fmt) for s, (w, h) in enumerate(sizes)]
    frames = [f for f, _ in made]
    cap = sum(m.Encoder.bound(w, h, fmt, bits, **opts) for w, h in sizes)
    host = np.full(cap, OUT_POISON, np.uint8)
    r, offs = ef.call_batch(enc, frames, bits, host, **opts)
    assert r == 0 and offs[0] == 0 and all(a < b for a, b in zip(offs, offs[1:]))
    end = offs[-1]
    assert (host[end:] == OUT_POISON).all()
    dev = torch.full((cap + 64,), OUT_POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r, offs_d = ef.call_batch(enc, frames, bits, dev.data_ptr(), cap=cap, out_on_device=1, **opts)
    assert r == 0 and offs_d == offs
    back = dev.cpu().numpy()
    assert back[:end].tobytes() == host[:end].tobytes() and (back[end:] == OUT_POISON).all()
    dev.fill_(OUT_POISON)
    torch.cuda.synchronize()
    r, _ = ef.call_batch(enc, frames, bits, dev.data_ptr(), cap=end - 1, out_on_device=1, **opts)
    assert r == -28 and bool((dev == OUT_POISON).all())
    r, offs_d = ef.call_batch(enc, frames, bits, dev.data_ptr(), cap=end, out_on_device=1, **opts)
    assert r == 0 and offs_d == offs and dev.cpu().numpy()[:end].tobytes() == host[:end].tobytes()


def test_refusals_leave_the_output_and_the_encoder_alone(enc):
    """-22, nothing written, and the next good call is what it was: a NULL plane, a negative linesize, a linesize one byte
    below the row, frames of two layouts in one batch, n = 0"""
    good = case("rgb24", 8, 64, 40)
    ref = enc.encode(good, "rgb24", 8)
    yuv = case("yuv420p", 8, 64, 40)
    ref_yuv = enc.encode(yuv, "yuv420p", 8)
    out = np.full(4 * len(ref) + 4096, OUT_POISON, np.uint8)

    def rgb(**change):
        fr, keep = m.frame_from_planes(good, "rgb24")
        for k, v in change.items():
            if k == "data":
                fr.data[0] = v
            elif k == "linesize":
                fr.linesize[0] = v
            else:
                setattr(fr, k, v)
        return fr, keep

    def yuv_frame(plane, data=0, linesize=None):
        fr, keep = m.frame_from_planes(yuv, "yuv420p")
        if linesize is None:
            fr.data[plane] = data or None
        else:
            fr.linesize[plane] = linesize
        return fr, keep

    gray, keep_gray = m.frame_from_planes(case("gray", 8, 64, 40), "gray")
    ok, keep_ok = rgb()
    bad = [("data NULL", [rgb(data=None)[0]], 8), ("linesize negative", [rgb(linesize=-192)[0]], 8),
           ("linesize short", [rgb(linesize=191)[0]], 8), ("second frame bad", [ok, rgb(linesize=191)[0]], 8),
           ("two layouts", [ok, gray], 8)]
    for name, frames, bits in bad:
        r, _ = ef.call_batch(enc, frames, bits, out)
        assert r == -22 and (out == OUT_POISON).all(), name
        assert enc.encode(good, "rgb24", 8) == ref, name
    for name, fr in [("chroma plane NULL", yuv_frame(2)[0]), ("chroma linesize short", yuv_frame(1, linesize=31)[0]),
                     ("chroma linesize negative", yuv_frame(1, linesize=-32)[0])]:
        r, _ = ef.call_batch(enc, [fr], 8, out)
        assert r == -22 and (out == OUT_POISON).all(), name
        assert enc.encode(yuv, "yuv420p", 8) == ref_yuv, name
    r, _ = ef.call_batch(enc, [ok], 8, out, n=0)
    assert r == -22 and (out == OUT_POISON).all()
    assert enc.encode(good, "rgb24", 8) == ref
    # the same refusals with the planes in device memory
    fr, keep = ef.device_frame(good, "rgb24", 64, 40, [13] * 4, torch)
    for name, change in [("data NULL", dict(data=None)), ("linesize negative", dict(linesize=-205)), ("linesize short", dict(linesize=191))]:
        f2 = m.Frame.from_buffer_copy(fr)
        if "data" in change:
            f2.data[0] = None
        else:
            f2.linesize[0] = change["linesize"]
        r, _ = ef.call_batch(enc, [f2], 8, out, in_on_device=1)
        assert r == -22 and (out == OUT_POISON).all(), name
    assert ef.encode_frames(enc, [fr], "rgb24", 8, in_on_device=1) == [ref]


@pytest.mark.parametrize("opts", [dict(), dict(levels=3, cb=(5, 5), irreversible=True, qstep=0.5),
                                  dict(levels=3, cb=(4, 4), irreversible=True, qstep=0.25, target_bytes=5000)],
                         ids=["53", "97", "97-budget"])
def test_encode_frame_equals_a_batch_of_one(enc, opts):
    fmt, bits, w, h = "yuv422p10le", 10, 150, 90
    planes = case(fmt, bits, w, h)
    ref = enc.encode(planes, fmt, bits, **opts)
    fr, keep = ef.padded_frame(planes, fmt, w, h, [0, 13, 1, 0])
    o = m._enc_opts(**opts)
    out = np.full(len(ref) + 64, OUT_POISON, np.uint8)
    ln = ctypes.c_size_t(777)
    r = enc.L.htj2k_encode_frame(enc.h, ctypes.byref(fr), bits, ctypes.byref(o), out.ctypes.data_as(ctypes.c_void_p),
                                 ctypes.c_size_t(out.size), ctypes.byref(ln))
    assert r == 0 and ln.value == len(ref) and out[:len(ref)].tobytes() == ref and (out[len(ref):] == OUT_POISON).all()
    # refused calls: out_len is 0, nothing is written
    out[:] = OUT_POISON
    for change, code in [("cap", -28), ("linesize", -22)]:
        f2 = m.Frame.from_buffer_copy(fr)
        if change == "linesize":
            f2.linesize[1] = 2 * 75 - 1
        ln = ctypes.c_size_t(777)
        r = enc.L.htj2k_encode_frame(enc.h, ctypes.byref(f2), bits, ctypes.byref(o), out.ctypes.data_as(ctypes.c_void_p),
                                     ctypes.c_size_t(len(ref) - 1 if change == "cap" else out.size), ctypes.byref(ln))
        assert r == code and ln.value == 0 and (out == OUT_POISON).all(), change
    assert enc.encode(planes, fmt, bits, **opts) == ref


# ------------------------------------------------------------------ rounds and launch chunks

def samples(fmt, w, h):
    return sum(cw * ch for cw, ch in em.comp_dims(fmt, w, h))


def rounds_of(fmt, sizes, limit):
    """the frames of every round by the rule of DESIGN.md 3.5: a round takes frames while their samples stay within the
    limit, and at least one"""
    out, cur, ns = [], [], 0
    for k, (w, h) in enumerate(sizes):
        s = samples(fmt, w, h)
        if cur and ns + s > limit:
            out.append(cur)
            cur, ns = [], 0
        cur.append(k)
        ns += s
    return out + [cur]


ROUND = 40000


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


def check_batch_against_singles(enc, e2, distinct, order, fmt, bits, opts):
    """one call of `e2` over distinct[order[k]] against the single-frame calls of `enc`: bytes, offsets as the running
    sum, rc_info and last_planes of every frame"""
    single, info, chosen = [], [], []
    for planes in distinct:
        single.append(enc.encode(planes, fmt, bits, **opts))
        info.append(enc.rc_info(0))
        chosen.append(enc.last_planes(0))
    made = [m.frame_from_planes(p, fmt) for p in distinct]
    frames = [made[i][0] for i in order]
    cap = sum(m.Encoder.bound(f.width, f.height, fmt, bits, **opts) for f in frames)
    out = np.empty(cap, np.uint8)
    r, offs = ef.call_batch(e2, frames, bits, out, **opts)
    assert r == 0
    want = np.cumsum([0] + [len(single[i]) for i in order]).tolist()
    assert offs == want
    for k, i in enumerate(order):
        assert out[offs[k]:offs[k + 1]].tobytes() == single[i], k
    for k in range(len(order)):
        assert e2.rc_info(k) == info[order[k]], (k, e2.rc_info(k), info[order[k]])
        assert e2.last_planes(k) == chosen[order[k]], k
    return offs


@pytest.mark.parametrize("budget", [False, True], ids=["free", "budget"])
@pytest.mark.parametrize("irreversible", [False, True], ids=["53", "97"])
@pytest.mark.parametrize("fmt,bits", [("rgb24", 8), ("yuv420p10le", 10)])
def test_calls_of_several_rounds(enc, enc_small_rounds, fmt, bits, irreversible, budget):
    """HTJ2K_ENC_ROUND = 40 000 samples: 16 frames of 160 x 96 and 75 x 41 in one call go through in four rounds or more
    (counted here from the sizes); every frame is what the single-frame call of an encoder without the knob writes, the
    offsets run on across the rounds, and rc_info / last_planes answer for the frames of every round"""
    sizes = [(160, 96), (160, 96), (75, 41), (75, 41)]
    distinct = [case(fmt, bits, w, h, "synth" if i < 2 else "noise", seed=i) for i, (w, h) in enumerate(sizes)]
    order = [0, 2, 1, 3, 3, 0, 2, 1, 1, 1, 0, 3, 2, 2, 0, 3]
    rounds = rounds_of(fmt, [sizes[i] for i in order], ROUND)
    assert len(rounds) >= 4 and all(rounds), rounds
    if fmt == "rgb24":
        assert samples(fmt, 160, 96) > ROUND          # a frame larger than the knob is a round of its own
    opts = dict(levels=3, cb=(4, 4), irreversible=irreversible, qstep=0.25)
    if budget:
        opts["target_bytes"] = len(enc.encode(distinct[0], fmt, bits, **opts)) // 2
    check_batch_against_singles(enc, enc_small_rounds, distinct, order, fmt, bits, opts)
    first_of_later_rounds = [r[0] for r in rounds[1:]]
    assert first_of_later_rounds and all(enc_small_rounds.rc_info(k)["nblocks"] > 0 for k in first_of_later_rounds)


def test_a_bad_frame_in_a_later_round_is_refused_before_any_round_writes(enc, enc_small_rounds):
    """sixteen frames in four rounds or more, the last one with a linesize one byte below its row: -22 and the output as
    it was, although the rounds before the bad frame's could have run; the next good call is what it was"""
    fmt, bits, w, h = "rgb24", 8, 160, 96
    planes = case(fmt, bits, w, h)
    ref = enc.encode(planes, fmt, bits)
    good, keep = m.frame_from_planes(planes, fmt)
    bad = m.Frame.from_buffer_copy(good)
    bad.linesize[0] = 3 * w - 1
    frames = [good] * 15 + [bad]
    assert len(rounds_of(fmt, [(w, h)] * 16, ROUND)) >= 4
    out = np.full(16 * m.Encoder.bound(w, h, fmt, bits), OUT_POISON, np.uint8)
    r, _ = ef.call_batch(enc_small_rounds, frames, bits, out)
    assert r == -22 and (out == OUT_POISON).all()
    assert enc_small_rounds.encode(planes, fmt, bits) == ref


def test_a_frame_larger_than_the_round(enc, enc_small_rounds):
    planes = case("rgb24", 8, 640, 480)
    assert samples("rgb24", 640, 480) > ROUND
    for opts in TRANSFORMS:
        assert enc_small_rounds.encode(planes, "rgb24", 8, **opts) == enc.encode(planes, "rgb24", 8, **opts)


@pytest.mark.parametrize("opts", [dict(), dict(irreversible=True, qstep=1.0, target_bytes=-2)], ids=["53", "97-budget"])
def test_rounds_at_the_real_size(enc, opts):
    """no knob: 12 frames of 7680 x 4320 rgb48le (two distinct ones alternating) are 1.11 x 2^30 samples and go through as
    10 + 2.  target_bytes = -2 stands for half of the first frame's free size."""
    fmt, bits, w, h = "rgb48le", 16, 7680, 4320
    rounds = rounds_of(fmt, [(w, h)] * 12, 1 << 30)
    assert [len(r) for r in rounds] == [10, 2]
    distinct = [case(fmt, bits, w, h, seed=s) for s in (11, 12)]
    if opts.get("target_bytes"):
        opts = dict(opts, target_bytes=len(enc.encode(distinct[0], fmt, bits, **dict(opts, target_bytes=0))) // 2)
    t0 = time.time()
    check_batch_against_singles(enc, enc, distinct, [k & 1 for k in range(12)], fmt, bits, opts)
    print("12 x 7680 x 4320 rgb48le, %s: two single calls and the call of two rounds took %.1f s" % (opts, time.time() - t0))


@pytest.mark.parametrize("opts", [dict(levels=2), dict(levels=2, irreversible=True, qstep=0.5)], ids=["53", "97"])
def test_more_planes_than_one_launch_takes(enc, opts):
    """22 000 rgba frames of 9 x 7 in one call: 88 000 planes, so every launch over planes (the DWT levels, the quantiser)
    goes out in two chunks of grid.z; frame k is the single-frame stream of its array"""
    fmt, bits, n = "rgba", 8, 22000
    assert 4 * n > 65535
    distinct = [case(fmt, bits, 9, 7, "noise", seed=s) for s in range(4)]
    single = [enc.encode(p, fmt, bits, **opts) for p in distinct]
    made = [m.frame_from_planes(p, fmt) for p in distinct]
    arr = (m.Frame * n)()
    for k in range(n):
        arr[k] = made[k & 3][0]
    cap = n * m.Encoder.bound(9, 7, fmt, bits, **opts)
    out = np.empty(cap, np.uint8)
    offs = (ctypes.c_size_t * (n + 1))()
    t0 = time.time()
    assert enc.encode_into(arr, n, bits, m._enc_opts(**opts), out.ctypes.data_as(ctypes.c_void_p), cap, offs) == 0
    print("%d frames of 9 x 7 rgba in one call: %.1f s" % (n, time.time() - t0))
    offs = np.array(offs[:], np.int64)
    want = np.cumsum([0] + [len(single[k & 3]) for k in range(n)])
    assert np.array_equal(offs, want)
    for k in range(n):
        assert out[offs[k]:offs[k + 1]].tobytes() == single[k & 3], k
