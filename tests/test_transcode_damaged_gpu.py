"""Damaged sources on the GPU: bytes no encoder writes through the Part-1 block kernel (htj2k_mq_blocks and its raw stores)
against the oracle's decode_cblk, and the damaged streams of tests/xc_damage.py through Encoder.transcode -- the same
coefficients as the damaged source in no more bytes than htj2k_transcode_check's bound, or a clean error with nothing
written -- with what the encoder / decoder pair does after a refused call, and the same under a byte budget.
tests/test_transcode_damaged_host.py vets the streams on the CPU.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the library, as in tests/test_transcode_rc_gpu.py)

import ffmpeg_ht_amd as m
import oracle
import xc_damage as xd
import xc_model as xm
import xc_rc_model as xrm
from test_transcode_gpu import block_stage_planes

pytestmark = pytest.mark.gpu

INVALIDDATA = xd.INVALIDDATA


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def enc():
    e = m.Encoder(device_id=0)
    yield e
    e.close()


# ---------------------------------------------------------------- 1. garbage through k_mq_decode
SHAPES = [(64, 64), (32, 32), (63, 61), (1, 1), (3, 5), (1, 40), (40, 1), (128, 32), (1024, 4), (4, 1024)]        # (w, h)
STYLES = (0, 0x01, 0x04, 0x08, 0x2F)
PLANES = (1, 2, 9, 16, 29, 30)                             # K; M_b = K + 1, and 30 for K = 30: the first plane is bpno 28 or 29
POPULATIONS = ("uniform", "markers", "zeros", "ones")


def garbage(rng, pop, n):
    """n bytes of a population: uniform; half of them 0xFF, each followed by a byte on either side of the marker
    threshold 0x8F or at an end of the range; all 0x00; all 0xFF"""
    if pop == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if pop == "zeros":
        return b"\x00" * n
    if pop == "ones":
        return b"\xff" * n
    out = bytearray()
    while len(out) < n:
        out += bytes([0xFF, int(rng.choice([0x00, 0x7F, 0x8F, 0x90, 0xFF]))]) if rng.integers(0, 2) else bytes([int(rng.integers(0, 256))])
    return bytes(out[:n])


def garbage_block(rng, w, h, style, K, pop, band, last=2, lengths=None):
    """-> dict: a block of K bit-planes whose passes end on a pass of type `last` (2 cleanup: all 3 K - 2 of them, 1
    refinement, 0 significance), its codeword segments cut where oracle.mq_needs_termination says and filled from the
    population; lengths: the segments' lengths, or a draw from 0 .. 40 for each"""
    M_b = 30 if K == 30 else K + 1
    n = max(3 * K - 2 - {2: 0, 1: 1, 0: 2}[last], 1)
    segpasses, run = [], 0
    for i in range(n):
        run += 1
        if oracle.mq_needs_termination(style, i) or i == n - 1:
            segpasses.append(run)
            run = 0
    lens = [int(rng.integers(0, 41)) for _ in segpasses] if lengths is None else list(lengths)
    assert len(lens) == len(segpasses)
    seg = b"".join(garbage(rng, pop, ln) for ln in lens)
    data, length, starts = oracle.mq_block_layout(seg, lens, segpasses, style)
    return dict(w=w, h=h, style=style, K=K, M_b=M_b, n=n, band=band, data=data, length=length, starts=starts, lens=lens, pop=pop)


def garbage_blocks():
    """256 blocks, four waves of k_mq_decode.  The first 192: every style on every shape but 4 x 1024, each from every
    population, K, band and last pass going round, and twelve more: a single segment of about 2 KB on 64 x 64 from every
    population (the 96-byte window refilled some twenty times while the other lanes sit in their sentinels), and segments
    of 0, 1 and 2 bytes, alone and between others.  The last 64: 4 x 1024 in every style and population among small
    blocks.  (1024 x 4 and 4 x 1024 in one wave make every lane walk 1024 x 1024 positions per pass: they are together
    in tests/test_gpu_parity.py's table, with blocks an encoder wrote.)"""
    rng = np.random.default_rng(20261020)
    first, second, i = [], [], 0
    for style in STYLES:
        for (w, h) in SHAPES:
            for pop in POPULATIONS:
                b = garbage_block(rng, w, h, style, PLANES[i % 6], pop, (i // 6) % 4, last=(2, 2, 1, 0)[(i // 3) % 4])
                (second if (w, h) == (4, 1024) else first).append(b)
                i += 1
    for pop in POPULATIONS:
        first.append(garbage_block(rng, 64, 64, 0, 16, pop, 3, lengths=[2048 + len(first)]))
    for k, lens in enumerate(([0], [1], [2])):             # the whole block in 0, 1 or 2 bytes: nothing but the sentinel
        first.append(garbage_block(rng, 32, 32, 0x08, 9, "uniform", k, lengths=lens))
    nseg = len(garbage_block(rng, 1, 1, 0x04, 9, "zeros", 0)["lens"])
    for k, pop in enumerate(("uniform", "markers", "ones")):           # TERMALL: every pass its own segment, of 0, 1, 2, 0, 1, 2 ... bytes
        first.append(garbage_block(rng, 32, 32, 0x04, 9, pop, k, lengths=[(j + k) % 3 for j in range(nseg)]))
    nseg = len(garbage_block(rng, 1, 1, 0x01, 9, "zeros", 0)["lens"])
    for k in range(2):                                     # BYPASS: the raw segments among them
        first.append(garbage_block(rng, 17, 9, 0x01, 9, "markers", 2 + k, lengths=[(j + k) % 3 for j in range(nseg)]))
    assert len(first) == 192 and len(second) == 20
    small = [s for s in SHAPES if max(s) <= 64]
    while len(second) < 64:
        w, h = small[int(rng.integers(0, len(small)))]
        second.append(garbage_block(rng, w, h, STYLES[int(rng.integers(0, 5))], PLANES[int(rng.integers(0, 6))],
                                    POPULATIONS[int(rng.integers(0, 4))], int(rng.integers(0, 4)), last=int(rng.integers(0, 3))))
    mixed = [first[j] for j in rng.permutation(len(first))] + [second[j] for j in rng.permutation(len(second))]
    lens = [ln for b in mixed for ln in b["lens"]]
    assert {0, 1, 2} <= set(lens) and max(lens) > 2000
    assert {b["n"] % 3 for b in mixed if b["K"] > 1} == {0, 1, 2} and {b["band"] for b in mixed} == {0, 1, 2, 3}
    return mixed


@pytest.fixture(scope="module")
def garbage_reference():
    """the blocks and the oracle's words of each, decoded once: [(block, ret, words)]"""
    out = []
    for b in garbage_blocks():
        ret, t1 = oracle.mq_decode_block(b["data"], b["length"], b["n"], b["K"], b["w"], b["h"], b["M_b"], b["style"], b["band"], b["starts"])
        out.append((b, ret, t1))
    return out


def wave_cost(blocks):
    """positions times passes the lanes of every wave of 64 walk in lockstep, summed: what the table costs on the device"""
    cost = 0
    for i in range(0, len(blocks), 64):
        wv = blocks[i:i + 64]
        cost += -(-max(b["h"] for b in wv) // 4) * 4 * -(-max(b["w"] for b in wv) // 64) * 64 * max(b["n"] for b in wv)
    return cost


@pytest.mark.parametrize("order", ["mixed", "sorted"])
def test_garbage_through_the_part1_block_kernel(dec, garbage_reference, order):
    """bytes no encoder writes as the whole input of k_mq_decode: LPS-heavy renormalisation over two byte boundaries,
    0xFF before a byte on either side of 0x8F in mid-segment, segments of 0, 1 and 2 bytes, raw passes over such bytes,
    the window of a wave refilled while most lanes sit in their sentinels.  The samples of htj2k_mq_blocks equal
    decode_cblk + dequantization_int of the oracle, those of htj2k_mq_blocks_raw its words as indices (xm.raw_index),
    and the status is non-zero exactly where the oracle fails.  mixed: lanes of different shape, pass count and byte
    length in one wave; sorted: by height, width and passes, as a job lays its table out"""
    ref = garbage_reference
    if order == "sorted":
        ref = sorted(ref, key=lambda r: (-r[0]["h"], -r[0]["w"], -r[0]["n"]))
    assert wave_cost([b for b, _, _ in ref]) < 40e6         # tests/test_gpu_parity.py's table of encoded blocks: 135e6
    descs, pool, expect, soff = [], b"", [], 0
    for b, ret, t1 in ref:
        w, h, M_b = b["w"], b["h"], b["M_b"]
        want = np.zeros((h, w), dtype=np.int32)
        oracle.lib().orc_dequant_int(t1.ctypes.data_as(ctypes.c_void_p), w, want.ctypes.data_as(ctypes.c_void_p), w, w, h, M_b, 32768)
        d = m.BlockDesc()
        d.data_off, d.plane_off, d.lcup, d.lref, d.w, d.h, d.stride = len(pool), soff, b["length"], len(b["starts"]), w, h, w
        d.npasses, d.zbp, d.M_b, d.flags, d.roi_shift, d.f_step, d.i_step = b["n"], b["K"], M_b, 4 | 1, 0, 1.0, 32768
        descs.append(d)
        pool += oracle.mq_block_region(b["data"], b["length"], b["style"], b["band"], b["starts"])
        expect.append((soff, want, xm.raw_index(t1, M_b, b["K"], b["n"]), ret))
        soff += w * h
    what = lambda i: {k: v for k, v in ref[i][0].items() if k not in ("data", "starts")}
    assert sum(1 for _, want, _, _ in expect if want.any()) > len(expect) // 2
    for raw in (False, True):
        got, status = dec.mq_blocks(descs, pool, soff, raw=raw)
        for i, (o, want, idx, ret) in enumerate(expect):
            assert (status[i] != 0) == (ret < 0), (raw, i, what(i))
            ref_i = idx if raw else want
            assert np.array_equal(got[o:o + ref_i.size].reshape(ref_i.shape), ref_i), (raw, i, what(i))


# ---------------------------------------------------------------- 2. damaged frames through Encoder.transcode
@pytest.fixture(scope="module")
def goods(dec, enc):
    """name -> (source, its transcode), made before anything fails"""
    cache = {}

    def get(name):
        if name not in cache:
            src = xd.source(name)
            cache[name] = (src, enc.transcode(dec, [src], ht_sources=xd.SOURCES[name][2])[0])
        return cache[name]
    return get


def fails(enc, dec, frames, cap, ht, code):
    """the call raises `code` and writes nothing"""
    with pytest.raises(m.Htj2kError) as err:
        enc.transcode(dec, frames, cap=cap, ht_sources=ht)
    assert err.value.code == code, str(err.value)
    assert not enc.last_out.any()


def same_frame(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def check_draw(orc, dec, enc, good, bad, ht):
    """what one damaged stream must do -> (xd.outcome's kind, noted, the transcoded stream or None, the code of a failure)"""
    o = xd.outcome(orc, bad, ht)
    room = 4 * len(bad) + 100000
    if o[0] == "refused":                                  # A: the check raises, the call raises the same and writes nothing
        fails(enc, dec, [good, bad], m.Encoder.transcode_check(good, ht_sources=ht) + room, ht, o[1])
        return "refused", False, None, o[1]
    bound = o[-1]
    if o[0] == "error":                                    # B, blocks that fail: INVALIDDATA, nothing written
        fails(enc, dec, [bad], bound, ht, INVALIDDATA)
        if o[1] is None:
            with pytest.raises(m.Htj2kError):
                dec.decode(bad)
        else:                                              # (a marked block may fail on one side alone: tests/test_gpu_parity.py's rule)
            assert abs(dec.decode(bad)[3].n_block_errors - o[1]) <= o[2], o
        return "error", False, None, INVALIDDATA
    noted = o[1]                                           # B, compared
    _, oracle_bad, _ = orc.decode(bad)
    out = enc.transcode(dec, [bad], ht_sources=ht)[0]
    assert len(out) <= bound
    assert dec.probe(out).is_ht == 1
    info, oracle_out, _ = orc.decode(out)
    assert orc.block_errors() == 0 and info.is_ht == 1 and not orc.underrun_windows()
    a, b = block_stage_planes(dec, bad), block_stage_planes(dec, out)
    assert len(a) == len(b)
    for t, (p, q) in enumerate(zip(a, b)):
        assert p.dtype == q.dtype and p.shape == q.shape
        assert np.count_nonzero(p.view(np.uint32) != q.view(np.uint32)) == 0, t
    ia, dec_bad, _, sa = dec.decode(bad)
    ib, dec_out, _, sb = dec.decode(out)
    assert sa.n_block_errors == 0 == sb.n_block_errors
    assert (ia.width, ia.height, ia.pix_fmt, ia.bits_per_raw_sample) == (ib.width, ib.height, ib.pix_fmt, ib.bits_per_raw_sample)
    assert same_frame(dec_out, oracle_out)                 # the output is well-formed: both decoders agree on it
    assert same_frame(dec_out, dec_bad)
    if not noted:                                          # (noted: undefined input, the product's own decode is the reference)
        assert same_frame(oracle_out, oracle_bad)
    return "compared", noted, out, 0


@pytest.mark.parametrize("name,cls", xd.CASES, ids=["%s-%s" % c for c in xd.CASES])
def test_damaged_sources(orc, dec, enc, goods, name, cls):
    """every draw of a class on a source: compared, INVALIDDATA or refused as the oracle and the check say, with the
    counts the host test has; then, with the same encoder and decoder, the source comes out as before the failures, a
    batch around a damaged frame that transcodes equals the single calls, and a batch with a failing frame anywhere in
    it fails whole"""
    ht = xd.SOURCES[name][2]
    good, good_out = goods(name)
    kinds, ok_bad, failing, noted = [], None, None, 0
    for bad in xd.draws(name, cls):
        kind, n, out, code = check_draw(orc, dec, enc, good, bad, ht)
        kinds.append(kind)
        noted += n
        if kind == "compared" and ok_bad is None and bad != good:
            ok_bad = (bad, out)
        if kind != "compared" and failing is None:
            failing = (bad, code)
    counts = dict(compared=kinds.count("compared"), errors=kinds.count("error"), refused=kinds.count("refused"), noted=noted)
    print(name, cls, counts)
    if name in xd.PART1 and cls in "abcd":
        assert counts["compared"] == len(kinds)
    if name in xd.HT and cls == "a":
        assert 2 * counts["compared"] >= len(kinds)
    if name in xd.HT and cls == "b":
        assert counts["compared"] >= 2
    if cls in "ef":
        assert ok_bad is not None and failing is not None  # the seeds give every class of these both
    # after the failures
    assert enc.transcode(dec, [good], ht_sources=ht) == [good_out]
    cap = 2 * m.Encoder.transcode_check(good, ht_sources=ht) + 4 * len(good) + 100000
    if ok_bad:
        assert enc.transcode(dec, [good, ok_bad[0], good], ht_sources=ht) == [good_out, ok_bad[1], good_out]
    if failing:
        middle = ok_bad[0] if ok_bad else good
        for at in range(3):
            frames = [good, middle, good]
            frames[at] = failing[0]
            fails(enc, dec, frames, cap, ht, failing[1])
        assert enc.transcode(dec, [good], ht_sources=ht) == [good_out]


@pytest.mark.parametrize("name", sorted(xd.SOURCES))
def test_conditions(orc, name):
    """the conditions that keep check_draw from hiding a failure (xd.conditions), on the draws the test above ran"""
    xd.conditions(name, {cls: xd.census(orc, name, cls)[1] for cls in xd.CLASSES[name]})


# ---------------------------------------------------------------- 3. with a budget
def no_finer(form, free):
    """(plane of the last pass, passes) under a budget against the unbudgeted call's: left out, a higher plane, or the
    same plane with passes the source backs (tests/xc_rc_model.py)"""
    (p, k), (fp, fk) = form, free
    return p < 0 or (fp >= 0 and (p > fp or (p == fp and k in xrm.ALLOWED_AT_0[fk])))


@pytest.mark.parametrize("name,cls", [("p1_rgb_53_cb16", "c"), ("p1_rgb_97_style05", "c"), ("ht_rgb_53_3p", "a")])
def test_damaged_sources_with_a_budget(orc, dec, enc, name, cls):
    """the compared draws again with half their unbudgeted size for a budget: the call succeeds within it, both decoders
    read the stream without a block error and agree, and no block is finer than without the budget"""
    ht = xd.SOURCES[name][2]
    done = 0
    for bad in xd.draws(name, cls):
        if xd.outcome(orc, bad, ht)[0] != "compared":
            continue
        out = enc.transcode(dec, [bad], ht_sources=ht)[0]
        free = list(zip(enc.last_planes(0), enc.last_passes(0)))
        target = max(m.Encoder.transcode_min_size(bad, ht_sources=ht), len(out) // 2)
        cs = enc.transcode(dec, [bad], target_bytes=target, ht_sources=ht)[0]
        forms = list(zip(enc.last_planes(0), enc.last_passes(0)))
        assert len(cs) <= target
        _, got, _, st = dec.decode(cs)
        _, want, _ = orc.decode(cs)
        assert st.n_block_errors == 0 == orc.block_errors()
        assert same_frame(got, want)
        assert len(forms) == len(free)
        worse = [i for i, (f, g) in enumerate(zip(forms, free)) if not no_finer(f, g)]
        assert not worse, (worse[:5], [forms[i] for i in worse[:5]], [free[i] for i in worse[:5]])
        assert forms != free or len(out) <= target
        done += 1
    assert done >= (xd.DRAWS if name in xd.PART1 else xd.DRAWS // 2)
