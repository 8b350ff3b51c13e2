"""GPU checks of the lossy encoder (htj2k_enc_* with irreversible = 1): the forward 9/7 kernels against the float32
model bit for bit and the decoder's inverse, whole frames of every layout against vecgen's encode(..., transform=0) byte
for byte and decoded by the product decoder (float and bitexact 9/7) and the oracle, rate and quality of the synth
frames, batches, device input, the output-buffer limit, guard bits, and lossless output left as it was."""
import ctypes

import numpy as np
import pytest

import enc97_model as e97
import enc_model as em
import ffmpeg_ht_amd as m
import vecgen
from test_encode_gpu import FORMATS, _content

pytestmark = pytest.mark.gpu


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


def _decoder(cache, pf, bitexact):
    if (pf, bitexact) not in cache:
        cache[pf, bitexact] = m.Decoder(device_id=0, req_pix_fmt=pf, bitexact=bitexact)
    return cache[pf, bitexact]


@pytest.mark.parametrize("w,h,levels", [(1, 1, 3), (1, 255, 5), (255, 1, 5), (17, 9, 1), (17, 9, 6), (640, 480, 5),
                                        (3840, 2160, 5), (333, 777, 32)])
def test_fdwt97_plane_model_and_inverse(enc, dec, w, h, levels):
    rng = np.random.default_rng(w * 31 + h)
    x = rng.integers(-(1 << 15), 1 << 15, size=(h, w)).astype(np.float32)
    y = enc.fdwt97_plane(x, levels)
    assert np.array_equal(y.view(np.uint32), e97.fdwt97(x, levels).view(np.uint32))
    back = dec.idwt(y, ((0, w), (0, h)), levels, m.DWT97)
    assert np.abs(back - x).max() < 0.5


def _roundtrip(enc, orc, cache, fmt, bits, comps, w, h, qstep, levels=5, cb=(6, 6), mct=None):
    """product encode == vecgen; product float / bitexact decodes == the oracle's in the same mode"""
    mct_v = em.mct_default(fmt) if mct is None else bool(mct)
    planes = em.to_planes(comps, fmt, bits)
    cs = enc.encode(planes, fmt, bits, levels=levels, cb=cb, mct=-1 if mct is None else int(mct), irreversible=True,
                    qstep=qstep)
    g = em.qcd_guard_bits(cs)
    ref = vecgen.encode(comps, **e97.vecgen_args(fmt, w, h, bits, levels, cb, mct_v, g, qstep))
    assert cs == ref, (fmt, bits, w, h, levels, cb, qstep)
    pf = em.pix(fmt)
    for bitexact in (0, 1):
        info, got, _, st = _decoder(cache, pf, bitexact).decode(cs)
        assert info.pix_fmt == pf and st.n_block_errors == 0
        _, got_o, _ = orc.decode(cs, req_pix_fmt=pf, bitexact=bitexact)
        for a, b in zip(got, got_o):
            assert np.array_equal(a, b), ("oracle", bitexact, fmt, bits, w, h, qstep)
    return cs, got


QSTEPS = (0.25, 1.0, 4.0)


@pytest.mark.parametrize("fmt,bits", FORMATS)
def test_every_layout_round_trips(enc, orc, decoders, fmt, bits):
    for i, ((w, h), kind) in enumerate([((17, 9), "synth"), ((1, 1), "noise"), ((1, 255), "max"), ((255, 1), "zero"),
                                        ((64, 40), "noise"), ((37, 29), "checker")]):
        comps = _content(kind, fmt, w, h, bits, seed=i)
        sizes = []
        for q in QSTEPS:
            cs, _ = _roundtrip(enc, orc, decoders, fmt, bits, comps, w, h, q, levels=[5, 0, 1, 5, 3, 8][i],
                               cb=[(6, 6), (5, 5), (7, 5), (10, 2), (4, 4), (5, 5)][i])
            sizes.append(len(cs))
        if kind == "noise" and w > 1:
            assert sizes[0] > sizes[1] > sizes[2], (fmt, sizes)


# vecgen + oracle on the CPU at 512 x 384, 5 levels, 64 x 64 blocks, G = 2: (bit/pixel, PSNR dB)
TABLE = {("rgb24", 1.0): (7.18, 42.5869), ("rgb24", 4.0): (0.36, 34.2359),
         ("gray", 1.0): (3.26, 47.4863), ("gray", 4.0): (0.60, 35.7485)}


@pytest.mark.parametrize("fmt,qstep", sorted(TABLE))
def test_rate_and_quality_of_synth_frames(enc, decoders, fmt, qstep):
    w, h = 512, 384
    comps = vecgen.synth_image(w, h, 3 if fmt == "rgb24" else 1)
    planes = em.to_planes(comps, fmt, 8)
    cs = enc.encode(planes, fmt, 8, irreversible=True, qstep=qstep)
    _, got, _, st = _decoder(decoders, em.pix(fmt), 0).decode(cs)
    assert st.n_block_errors == 0
    d = got[0].reshape(-1).astype(np.float64) - planes[0].reshape(-1).astype(np.float64)
    psnr = 10 * np.log10(255.0 ** 2 / np.mean(d * d))
    bpp, want_psnr = TABLE[fmt, qstep]
    assert round(8 * len(cs) / (w * h), 2) == bpp
    assert abs(psnr - want_psnr) < 0.01, psnr


def _c2(seed):
    return em.to_planes([vecgen.synth_image(3840, 2160, 1, seed=seed + c)[0] for c in range(3)], "rgb24", 8)


@pytest.mark.parametrize("qstep", [1.0, 4.0])
def test_c2_frame_and_batch(enc, dec, qstep):
    opts = dict(irreversible=True, qstep=qstep)
    frames = [_c2(s) for s in range(4)]
    single = [enc.encode(p, "rgb24", 8, **opts) for p in frames]
    if qstep == 1.0:
        comps = [vecgen.synth_image(3840, 2160, 1, seed=c)[0] for c in range(3)]
        g = em.qcd_guard_bits(single[0])
        assert single[0] == vecgen.encode(comps, **e97.vecgen_args("rgb24", 3840, 2160, 8, 5, (6, 6), True, g, qstep))
    order = [0, 1, 2, 3] * 4
    batch = enc.encode_batch([frames[i] for i in order], "rgb24", 8, **opts)
    assert batch == [single[i] for i in order]
    # the same frame in device memory: decoded from its lossless codestream, as the decoder hands frames to the encoder
    job = dec.job().parse(enc.encode(frames[2], "rgb24", 8)).upload().run().wait()
    fr = m.Frame()
    assert dec.L.htj2k_job_device_frame(dec.h, job.h, 0, ctypes.byref(fr)) == 0
    fr.width, fr.height = 3840, 2160
    assert enc.encode_device([fr], "rgb24", 8, **opts)[0] == single[2]
    job.free()


def test_output_buffer_too_small(enc):
    planes = em.to_planes(_content("synth", "gray", 64, 64, 8, 1), "gray", 8)
    cs = enc.encode(planes, "gray", 8, irreversible=True, qstep=0.5)
    fr, keep = m.frame_from_planes(planes, "gray")
    arr = (m.Frame * 1)(fr)
    out = np.full(len(cs) + 16, 0xAB, np.uint8)
    offs = (ctypes.c_size_t * 2)()
    o = m._enc_opts(irreversible=True, qstep=0.5)
    r = enc.L.htj2k_encode_batch(enc.h, arr, 1, 8, ctypes.byref(o), 0, out.ctypes.data_as(ctypes.c_void_p),
                                 ctypes.c_size_t(len(cs) - 1), 0, offs)
    assert r == -28 and (out == 0xAB).all()
    assert enc.encode_into(arr, 1, 8, o, out.ctypes.data_as(ctypes.c_void_p), len(cs), offs) == 0
    assert out[:len(cs)].tobytes() == cs and (out[len(cs):] == 0xAB).all()


def test_bad_qstep_refused_on_the_device_path(enc):
    planes = em.to_planes(_content("synth", "gray", 32, 32, 8, 1), "gray", 8)
    for q in (0.0, -1.0, float("nan"), float("inf"), 1e-7, 1e5):
        with pytest.raises(m.Htj2kError) as e:
            enc.encode(planes, "gray", 8, irreversible=True, qstep=q)
        assert e.value.code == -22


def test_guard_bits(enc, orc, decoders):
    """16-bit extremes at fine steps: the 9/7 exponents carry no gain term, yet the automatic choice stays at 2 (the
    normalised gains of these contents stay within one bit of the step), and matches vecgen; fixed G above it is
    written as asked and still matches"""
    for fmt, kind, levels in [("gray16le", "max", 5), ("gray16le", "checker", 1), ("rgb48le", "checker", 5),
                              ("yuv444p16le", "max", 8)]:
        comps = _content(kind, fmt, 37, 29, 16, 1)
        cs, _ = _roundtrip(enc, orc, decoders, fmt, 16, comps, 37, 29, 1 / 32, levels=levels)
        assert em.qcd_guard_bits(cs) == 2
    comps = _content("checker", "gray16le", 37, 29, 16, 1)
    planes = em.to_planes(comps, "gray16le", 16)
    for g in (3, 5):
        cs = enc.encode(planes, "gray16le", 16, levels=3, irreversible=True, qstep=1 / 32, guard_bits=g)
        assert em.qcd_guard_bits(cs) == g
        assert cs == vecgen.encode(comps, **e97.vecgen_args("gray16le", 37, 29, 16, 3, (6, 6), False, g, 1 / 32))


def test_lossless_output_unchanged(enc):
    """irreversible off: qstep is not read, and the bytes are the 5/3 encoder's"""
    for fmt, bits, (w, h) in [("rgb24", 8, (160, 96)), ("yuv420p10le", 10, (75, 41)), ("gray16le", 16, (64, 64))]:
        comps = _content("synth", fmt, w, h, bits, 2)
        planes = em.to_planes(comps, fmt, bits)
        base = enc.encode(planes, fmt, bits)
        for q in (0.0, 2.0, float("nan")):
            assert enc.encode(planes, fmt, bits, irreversible=False, qstep=q) == base
        ref = vecgen.encode(comps, **em.vecgen_args(fmt, w, h, bits, 5, (6, 6), em.mct_default(fmt), em.qcd_guard_bits(base)))
        assert base == ref
