"""GPU checks of the lossless encoder (htj2k_enc_*): the HT cleanup kernel against vecgen's encode_block, the forward
5/3 kernels against the numpy model and the decoder's inverse, whole frames against vecgen's encode and decoded back
by the product decoder and the oracle, batches, device input, and the C example."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import enc_model as em
import ffmpeg_ht_amd as m
import vecgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _blocks():
    rng = np.random.default_rng(7)
    out = []
    for w, h in [(64, 64), (32, 32), (128, 32), (1024, 4), (4, 1024), (3, 5), (1, 1), (7, 2), (2, 1), (5, 1), (33, 17)]:
        out.append(rng.integers(-6, 7, size=(h, w)))
        out.append(rng.integers(-(1 << 20), 1 << 20, size=(h, w)))
    out.append(np.zeros((16, 16), np.int64))
    z = np.zeros((64, 64), np.int64)
    z[63, 63] = -1
    out.append(z)
    out.append(rng.integers(-(1 << 30), 1 << 30, size=(64, 64)))           # M_b up to 31
    big = np.full((32, 32), -(1 << 30), np.int64)                         # |v| = 2^30: 31 magnitude bits
    out.append(big)
    for k in (3, 8, 13):                                                  # MagSgn all ones: 0xFF on every byte
        out.append(np.full((64, 64), -(1 << (k - 1)), np.int64))
    sparse = rng.integers(-3, 4, size=(64, 64)) * (rng.random((64, 64)) < 0.1)
    out.append(sparse)
    alt = np.where((np.indices((64, 64)).sum(0) & 1) == 0, 127, -128)     # dense, VLC-heavy checkerboard
    out.append(alt)
    return [a.astype(np.int32) for a in out]


def test_ht_encode_blocks_equal_vecgen(enc):
    blocks = _blocks()
    for v in blocks:
        h, w = v.shape
        (data, lcup, mu), = enc.ht_encode_blocks(v, [(0, 0, w, h)])
        if not v.any():
            assert lcup == 0
            continue
        ref, rl, _, rmu = vecgen.encode_block(v)
        assert lcup == rl and mu == rmu and data == ref[:rl], (w, h, int(np.abs(v).max()))


def test_ht_encode_blocks_many_in_one_plane(enc):
    rng = np.random.default_rng(1)
    plane = rng.integers(-300, 300, size=(100, 200)).astype(np.int32)
    rects = [(x, y, min(64, 200 - x), min(32, 100 - y)) for y in range(0, 100, 32) for x in range(0, 200, 64)]
    for (data, lcup, mu), (x, y, w, h) in zip(enc.ht_encode_blocks(plane, rects), rects):
        ref, rl, _, rmu = vecgen.encode_block(plane[y:y + h, x:x + w])
        assert (data, lcup, mu) == (ref[:rl], rl, rmu)


@pytest.mark.parametrize("w,h,levels", [(1, 1, 3), (1, 255, 5), (255, 1, 5), (17, 9, 1), (17, 9, 6), (640, 480, 5),
                                        (3840, 2160, 5), (333, 777, 32)])
def test_fdwt_plane_model_and_inverse(enc, dec, w, h, levels):
    rng = np.random.default_rng(w * 31 + h)
    x = rng.integers(-(1 << 15), 1 << 15, size=(h, w)).astype(np.int32)
    y = enc.fdwt_plane(x, levels)
    assert np.array_equal(y, em.fdwt(x, levels))
    back = dec.idwt(y, ((0, w), (0, h)), levels, m.DWT53)
    assert np.array_equal(back, x)


def _content(kind, fmt, w, h, bits, seed):
    dims = em.comp_dims(fmt, w, h)
    rng = np.random.default_rng(seed)
    out = []
    for c, (cw, ch) in enumerate(dims):
        if kind == "synth":
            out.append(vecgen.synth_image(cw, ch, 1, depth=bits, seed=seed + c)[0])
        elif kind == "noise":
            out.append(rng.integers(0, 1 << bits, size=(ch, cw)).astype(np.int32))
        elif kind == "zero":
            out.append(np.zeros((ch, cw), np.int32))
        elif kind == "max":
            out.append(np.full((ch, cw), (1 << bits) - 1, np.int32))
        else:
            out.append(np.where((np.indices((ch, cw)).sum(0) & 1) == 0, (1 << bits) - 1, 0).astype(np.int32))
    return out


def _roundtrip(enc, fmt, bits, comps, w, h, dec_cache, orc, levels=5, cb=(6, 6), mct=None, oracle=True):
    mct_v = em.mct_default(fmt) if mct is None else bool(mct)
    planes = em.to_planes(comps, fmt, bits)
    cs = enc.encode(planes, fmt, bits, levels=levels, cb=cb, mct=-1 if mct is None else int(mct))
    g = em.qcd_guard_bits(cs)
    ref = vecgen.encode(comps, **em.vecgen_args(fmt, w, h, bits, levels, cb, mct_v, g))
    assert cs == ref, (fmt, bits, w, h, levels, cb)
    pf = em.pix(fmt)
    if pf not in dec_cache:
        dec_cache[pf] = m.Decoder(device_id=0, req_pix_fmt=pf)
    info, got, _, st = dec_cache[pf].decode(cs)
    assert info.pix_fmt == pf and st.n_block_errors == 0
    for a, b in zip(got, planes):
        assert np.array_equal(a.reshape(-1), b.reshape(-1)), (fmt, bits, w, h)
    if oracle:
        info_o, got_o, _ = orc.decode(cs, req_pix_fmt=pf)
        for a, b in zip(got_o, planes):
            assert np.array_equal(a.reshape(-1), b.reshape(-1)), ("oracle", fmt, bits, w, h)
    return cs


FORMATS = [("gray", 8), ("gray", 5), ("ya8", 8), ("gray16le", 16), ("gray16le", 12), ("ya16le", 10), ("rgb24", 8),
           ("rgba", 8), ("rgb48le", 16), ("rgb48le", 10), ("rgba64le", 16), ("yuv410p", 8), ("yuv411p", 8),
           ("yuva420p", 8), ("yuv420p", 8), ("yuv422p", 8), ("yuva422p", 8), ("yuv440p", 8), ("yuv444p", 8),
           ("yuva444p", 8), ("yuv420p9le", 9), ("yuv422p9le", 9), ("yuv444p9le", 9), ("yuva420p9le", 9),
           ("yuva422p9le", 9), ("yuva444p9le", 9), ("yuv420p10le", 10), ("yuv422p10le", 10), ("yuv444p10le", 10),
           ("yuva420p10le", 10), ("yuva422p10le", 10), ("yuva444p10le", 10), ("yuv420p12le", 12),
           ("yuv422p12le", 12), ("yuv444p12le", 12), ("yuv420p14le", 14), ("yuv422p14le", 14), ("yuv444p14le", 14),
           ("yuv420p16le", 16), ("yuv422p16le", 16), ("yuv444p16le", 16), ("yuva420p16le", 16),
           ("yuva422p16le", 16), ("yuva444p16le", 16)]


@pytest.mark.parametrize("fmt,bits", FORMATS)
def test_every_layout_round_trips(enc, orc, fmt, bits):
    cache = {}
    for i, ((w, h), kind) in enumerate([((17, 9), "synth"), ((1, 1), "noise"), ((1, 255), "max"), ((255, 1), "zero"),
                                        ((64, 40), "noise"), ((37, 29), "checker")]):
        comps = _content(kind, fmt, w, h, bits, seed=i)
        _roundtrip(enc, fmt, bits, comps, w, h, cache, orc, levels=[5, 0, 1, 5, 3, 8][i], cb=[(6, 6), (5, 5), (7, 5), (10, 2), (4, 4), (5, 5)][i])
    for d in cache.values():
        d.close()


@pytest.mark.parametrize("fmt,bits,levels,cb", [("rgb24", 8, 5, (6, 6)), ("rgb24", 8, 1, (5, 5)), ("gray", 8, 0, (6, 6)),
                                                ("yuv420p", 8, 11, (7, 5)), ("yuv422p", 8, 5, (10, 2))])
def test_640x480_matrix(enc, orc, fmt, bits, levels, cb):
    cache = {}
    for kind in ("synth", "noise"):
        _roundtrip(enc, fmt, bits, _content(kind, fmt, 640, 480, bits, 5), 640, 480, cache, orc, levels, cb)
    for d in cache.values():
        d.close()


def test_rgb_mct_off(enc, orc):
    _roundtrip(enc, "rgb24", 8, _content("synth", "rgb24", 96, 64, 8, 2), 96, 64, {}, orc, mct=0)


@pytest.mark.parametrize("fmt,bits,w,h", [("rgb24", 8, 3840, 2160), ("yuv422p10le", 10, 1920, 1080),
                                          ("gray16le", 16, 7680, 4320), ("rgb48le", 16, 7680, 4320)])
def test_large_frames(enc, orc, fmt, bits, w, h):
    big = w * h > 10_000_000
    _roundtrip(enc, fmt, bits, _content("synth", fmt, w, h, bits, 9), w, h, {}, orc, oracle=not big)


def test_coefficients_equal_decoder_ht_stage(enc):
    """fdwt of the level-shifted + RCT'd components == the decoder's HT-stage planes of the encoded frame"""
    w, h = 150, 90
    comps = _content("synth", "rgb24", w, h, 8, 4)
    cs = enc.encode(em.to_planes(comps, "rgb24", 8), "rgb24", 8, levels=4, cb=(5, 5))
    dec = m.Decoder(device_id=0)
    assert dec.L.htj2k_set_int(dec.h, b"coef16", 0) == 0          # int32 sub-bands in the plane buffer
    job = dec.job().parse(cs).upload().run(stages=1).wait()
    for c, v in enumerate(em.components(comps, 8, True)):
        want = enc.fdwt_plane(v.astype(np.int32), 4)
        assert np.array_equal(job.plane(c), want), c
    job.free()
    dec.close()


def test_batch_equals_single_calls(enc):
    frames = [_content("synth", "rgb24", 160, 96, 8, s) for s in range(3)] + \
             [_content("noise", "rgb24", 75, 41, 8, s) for s in range(3)]
    order = [0, 3, 1, 4, 2, 5]
    planes = [em.to_planes(frames[i], "rgb24", 8) for i in order]
    batch = enc.encode_batch(planes, "rgb24", 8, levels=3)
    single = [enc.encode(p, "rgb24", 8, levels=3) for p in planes]
    assert batch == single


def test_device_input_equals_host_input(enc, dec):
    comps = _content("synth", "yuv420p", 200, 120, 8, 6)
    planes = em.to_planes(comps, "yuv420p", 8)
    src = vecgen.encode(comps, **em.vecgen_args("yuv420p", 200, 120, 8, 4, (6, 6), False, 2))
    job = dec.job().parse(src).upload().run().wait()
    fr = m.Frame()
    assert dec.L.htj2k_job_device_frame(dec.h, job.h, 0, ctypes.byref(fr)) == 0
    fr.width, fr.height = 200, 120
    dev = enc.encode_device([fr], "yuv420p", 8, levels=4)[0]
    host = enc.encode(planes, "yuv420p", 8, levels=4)
    assert dev == host
    job.free()


def test_output_buffer_too_small(enc):
    planes = em.to_planes(_content("synth", "gray", 64, 64, 8, 1), "gray", 8)
    cs = enc.encode(planes, "gray", 8)
    fr, keep = m.frame_from_planes(planes, "gray")
    arr = (m.Frame * 1)(fr)
    out = np.full(len(cs) + 16, 0xAB, np.uint8)
    offs = (ctypes.c_size_t * 2)()
    o = m.EncOpts(5, 6, 6, -1, 0)
    r = enc.L.htj2k_encode_batch(enc.h, arr, 1, 8, ctypes.byref(o), 0, out.ctypes.data_as(ctypes.c_void_p),
                                 ctypes.c_size_t(len(cs) - 1), 0, offs)
    assert r == -28 and (out == 0xAB).all()
    assert enc.encode_into(arr, 1, 8, o, out.ctypes.data_as(ctypes.c_void_p), len(cs), offs) == 0
    assert out[:len(cs)].tobytes() == cs and (out[len(cs):] == 0xAB).all()


def test_example_round_trip():
    exe = os.path.join(ROOT, "examples", "htj2k_encode")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", ROOT, "examples/htj2k_encode"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "round trip ok" in out.stdout


@pytest.mark.parametrize("seed", range(4))
def test_ht_encode_blocks_stuffing_at_every_distance(enc, seed):
    """MagSgn arrays with 0xFF bytes near, far and back to back: values whose sign-magnitude bits are all ones mixed
    with random ones, so the 0xFF pass runs anything from one window to one per byte"""
    rng = np.random.default_rng(100 + seed)
    rects, blocks = [], []
    plane = np.zeros((64, 64 * 8), np.int32)
    for k in range(8):
        share = [0.0, 0.02, 0.2, 0.5, 0.8, 0.95, 0.99, 1.0][k]
        bits = int(rng.integers(2, 20))
        ones = np.full((64, 64), -(1 << (bits - 1)), np.int64)
        rnd = rng.integers(-(1 << bits), 1 << bits, size=(64, 64))
        v = np.where(rng.random((64, 64)) < share, ones, rnd).astype(np.int32)
        plane[:, 64 * k:64 * (k + 1)] = v
        rects.append((64 * k, 0, 64, 64))
    for (data, lcup, mu), (x, y, w, h) in zip(enc.ht_encode_blocks(plane, rects), rects):
        ref, rl, _, rmu = vecgen.encode_block(plane[y:y + h, x:x + w])
        assert (data, lcup, mu) == (ref[:rl], rl, rmu), x // 64


def test_ht_encode_blocks_rejects_oversized_quads(enc):
    plane = np.zeros((1024, 1024), np.int32)
    for rect in [(0, 0, 5, 819), (0, 0, 65, 63)]:
        with pytest.raises(m.Htj2kError) as e:
            enc.ht_encode_blocks(plane, [rect])
        assert e.value.code == -22


def test_phase_stamps_leave_the_bytes_alone(enc, monkeypatch):
    comps = _content("synth", "rgb24", 256, 128, 8, 3)
    planes = em.to_planes(comps, "rgb24", 8)
    monkeypatch.setenv("HTJ2K_ENC_STAMPS", "1")
    e2 = m.Encoder(0)
    try:
        assert e2.encode(planes, "rgb24", 8) == enc.encode(planes, "rgb24", 8)
        n, cyc = e2.ht_cycles()
        assert n > 0 and all(c > 0 for c in cyc[:4])
    finally:
        e2.close()
    assert enc.ht_cycles()[0] == 0
