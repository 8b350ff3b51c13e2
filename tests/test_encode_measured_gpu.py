"""GPU checks of htj2k_encode_batch_measured: the streams of htj2k_encode_batch reported with the error of their own
decode (report only), and the loop that holds target_psnr in decoded pixels (close_loop).

The frames and settings are those of test_encode_cq_gpu.py: four frames x {9/7 q 0.25, 9/7 q 1, 5/3}, levels 3.  Every
measured figure is compared, exactly, with cmp_model of the product decoder's own decode against the input; every stream of
the loop with the single-frame encode at the target the call reports.

Measured on an MI355X with max_rounds = 16, the 24 closed-loop cases take 1 to 7 quality rounds (DESIGN.md 3.5 has the
table; the default, 8, is that worst case plus one) and none falls back.  Two of them, rgb24 over 9/7 with qstep 1 at
44 dB, have a base_psnr below the target: they are the plane-0 stream after round 1 and final by the rule itself, so they
measure short (42.875 and 42.935 dB) with rounds = 1; "a second round exactly when round 1 measured short" is asserted
for every other frame."""
import math

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: device input and output go through it)

import cmp_model as cm
import enc_model as em
import ffmpeg_ht_amd as m
from test_encode_cq_gpu import FRAMES, FS, FS_IDS, LEVELS, SETTINGS
from test_encode_rc_gpu import check_decodes, synth

pytestmark = pytest.mark.gpu

LOOP_TARGETS = (38.0, 44.0)


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
def decs():
    d = {}
    yield d
    for x in d.values():
        x.close()


_frames = {}


def case(fi, si, seed=None):
    """(layout, bits, the frame's planes, the options of setting si)"""
    fmt, bits, w, h, cb = FRAMES[fi]
    key = (fi, fi + 1 if seed is None else seed)
    if key not in _frames:
        _frames[key] = em.to_planes(synth(fmt, w, h, bits, seed=key[1]), fmt, bits)
    return fmt, bits, _frames[key], dict(levels=LEVELS, cb=cb, **SETTINGS[si])


def decoded(decs, fmt, cs, bitexact=0):
    """the product decoder's frame of a stream, in the input's layout"""
    pf = em.pix(fmt)
    if (pf, bitexact) not in decs:
        decs[pf, bitexact] = m.Decoder(device_id=0, req_pix_fmt=pf, bitexact=bitexact)
    _, planes, _, st = decs[pf, bitexact].decode(cs)
    assert st.n_block_errors == 0
    return planes


def check_diff(decs, fmt, bits, planes, cs, info, bitexact=0):
    want = cm.compare(decoded(decs, fmt, cs, bitexact), planes, fmt, bits)
    assert cm.same(info["diff"], want, tol=0), (info, want)
    return want


# ---------------------------------------------------------------------------------------------- 1. report only

VARIANTS = [("plain", {}), ("target_bytes", None), ("ht_passes", dict(ht_passes=3)), ("tile", dict(tile=(64, 64)))]


@pytest.mark.parametrize("fi,si", FS, ids=FS_IDS)
def test_report_only_is_encode_batch_and_measures_its_decode(enc, dec, decs, fi, si):
    fmt, bits, planes, opts = case(fi, si)
    free = enc.encode(planes, fmt, bits, **opts)
    for name, extra in VARIANTS:
        extra = dict(target_bytes=int(len(free) * 0.6)) if extra is None else extra
        want = enc.encode_batch([planes], fmt, bits, **opts, **extra)
        got, info = enc.encode_measured(dec, [planes], fmt, bits, **opts, **extra)
        assert got == want, name
        d = check_diff(decs, fmt, bits, planes, got[0], info[0])
        assert info[0]["rounds"] == 1 and info[0]["fell_back"] == 0 and info[0]["short_measured"] == 0
        assert info[0]["first_psnr"] == info[0]["diff"]["psnr"] and info[0]["target_used"] == 0
        if name in ("plain", "tile") and not opts["irreversible"]:
            assert sum(d["sse"]) == 0 and sum(d["ndiff"]) == 0 and info[0]["diff"]["psnr"] == math.inf      # lossless
        elif name != "ht_passes":              # (three passes over 5/3 may lose nothing on a small frame)
            assert sum(d["sse"]) > 0
        print(FS_IDS[FS.index((fi, si))], name, len(got[0]), "bytes, %.3f dB" % info[0]["diff"]["psnr"])


@pytest.mark.parametrize("si", range(len(SETTINGS)))
def test_report_only_batches_and_a_group_budget(enc, dec, decs, si):
    """the two rgb24 frames in one call: sizes that differ, a budget over the group, a PSNR target that is only reported"""
    fmt, bits, a, opts = case(0, si)
    _, _, b, _ = case(1, si)
    free = enc.encode_batch([a, b], fmt, bits, **opts)
    for extra in ({}, dict(group_bytes=int(sum(len(c) for c in free) * 0.7)), dict(target_psnr=44.0)):
        want = enc.encode_batch([a, b], fmt, bits, **opts, **extra)
        if "group_bytes" in extra:
            assert sum(len(c) for c in want) <= extra["group_bytes"] < sum(len(c) for c in free)
        got, info = enc.encode_measured(dec, [a, b], fmt, bits, **opts, **extra)
        assert got == want
        for planes, cs, i in zip((a, b), got, info):
            check_diff(decs, fmt, bits, planes, cs, i)
            assert i["rounds"] == 1 and i["fell_back"] == 0 and i["target_used"] == extra.get("target_psnr", 0)
            assert i["short_measured"] == int("target_psnr" in extra and i["diff"]["psnr"] < 44.0)


# ---------------------------------------------------------------------------------------------- 2. contexts

def test_the_decoders_pixel_format_request_does_not_matter(enc, dec, decs):
    other = m.Decoder(device_id=0, req_pix_fmt=m.PIX_NAMES.index("yuv444p"))       # fits three 8-bit components as well
    try:
        for fi, si in ((0, 0), (0, 2), (3, 1)):
            fmt, bits, planes, opts = case(fi, si)
            a = enc.encode_measured(dec, [planes], fmt, bits, **opts)
            b = enc.encode_measured(other, [planes], fmt, bits, **opts)
            assert a == b
            check_diff(decs, fmt, bits, planes, b[0][0], b[1][0])
    finally:
        other.close()


def test_a_reduction_factor_is_refused(enc):
    low = m.Decoder(device_id=0, reduction_factor=1)
    try:
        fmt, bits, planes, opts = case(0, 2)
        with pytest.raises(m.Htj2kError) as e:
            enc.encode_measured(low, [planes], fmt, bits, **opts)
        assert e.value.code == -0x45574150
    finally:
        low.close()


def test_bitexact_changes_the_97_figures_only(enc, dec, decs):
    exact = m.Decoder(device_id=0, bitexact=1)
    differ = 0
    try:
        for fi, si in FS:
            fmt, bits, planes, opts = case(fi, si)
            cs, a = enc.encode_measured(dec, [planes], fmt, bits, **opts)
            cs2, b = enc.encode_measured(exact, [planes], fmt, bits, **opts)
            assert cs == cs2
            check_diff(decs, fmt, bits, planes, cs[0], b[0], bitexact=1)
            if opts["irreversible"]:
                differ += a[0]["diff"] != b[0]["diff"]
            else:
                assert a == b
    finally:
        exact.close()
    assert differ > 0


def test_device_input_and_output(enc, dec, decs):
    for fi, si in ((0, 0), (3, 2), (2, 1)):
        fmt, bits, planes, opts = case(fi, si)
        fr, keep = m.frame_from_planes(planes, fmt)
        ts = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes]
        torch.cuda.synchronize()
        for p, t in enumerate(ts):
            fr.data[p] = t.data_ptr()
        for kw in (dict(), dict(close_loop=True, target_psnr=44.0)):
            want = enc.encode_measured(dec, [planes], fmt, bits, **opts, **kw)
            assert enc.encode_measured(dec, [fr], fmt, bits, in_on_device=True, **opts, **kw) == want
            assert enc.encode_measured(dec, [planes], fmt, bits, out_on_device=True, **opts, **kw) == want
            assert enc.encode_measured(dec, [fr], fmt, bits, in_on_device=True, out_on_device=True, **opts, **kw) == want
            check_diff(decs, fmt, bits, planes, want[0][0], want[1][0])


def test_the_output_buffer(enc, dec):
    fmt, bits, planes, opts = case(0, 2)
    for kw in (dict(), dict(close_loop=True, target_psnr=44.0)):
        cs, _ = enc.encode_measured(dec, [planes, planes], fmt, bits, **opts, **kw)
        total = sum(len(c) for c in cs)
        assert enc.encode_measured(dec, [planes, planes], fmt, bits, cap=total, **opts, **kw)[0] == cs
        with pytest.raises(m.Htj2kError) as e:
            enc.encode_measured(dec, [planes, planes], fmt, bits, cap=total - 1, **opts, **kw)
        assert e.value.code == -28


# ---------------------------------------------------------------------------------------------- 3. rounds

def test_sixteen_frames_in_four_rounds(dec, decs, monkeypatch):
    fi = 1
    fmt, bits, w, h, cb = FRAMES[fi]
    monkeypatch.setenv("HTJ2K_ENC_ROUND", str(4 * w * h * 3))
    small = m.Encoder(0)
    try:
        frames = [case(fi, 0, seed=40 + k)[2] for k in range(16)]
        for si, kw in ((0, dict()), (2, dict(close_loop=True, target_psnr=44.0))):
            opts = case(fi, si)[3]
            cs, info = small.encode_measured(dec, frames, fmt, bits, **opts, **kw)
            if not kw:
                assert small.last_rounds() == 4
            q = [small.quality_info(k) for k in range(16)]
            for k in range(16):
                one, i1 = small.encode_measured(dec, [frames[k]], fmt, bits, **opts, **kw)
                assert one[0] == cs[k] and i1[0] == info[k], k
                assert small.quality_info(0) == q[k]
                check_diff(decs, fmt, bits, frames[k], cs[k], info[k])
    finally:
        small.close()


# ---------------------------------------------------------------------------------------------- 4. the closed loop

def check_loop_frame(enc, decs, fmt, bits, planes, opts, target, cs, info, q, extra=()):
    extra = dict(extra)
    check_diff(decs, fmt, bits, planes, cs, info)
    assert info["diff"]["psnr"] >= target or info["short_measured"]
    assert info["short_measured"] == int(info["diff"]["psnr"] < target)
    if info["short_measured"]:
        assert info["fell_back"] or q["short_of_target"] or q["capped"]
    if info["first_psnr"] >= target:
        assert info["rounds"] == 1
    if info["fell_back"]:
        assert info["target_used"] == 0 and cs == enc.encode(planes, fmt, bits, **opts, **extra)
    else:
        assert info["target_used"] >= target and q["target_psnr"] == info["target_used"]
        assert cs == enc.encode(planes, fmt, bits, target_psnr=info["target_used"], **opts, **extra)


@pytest.mark.parametrize("target", LOOP_TARGETS)
@pytest.mark.parametrize("fi,si", FS, ids=FS_IDS)
def test_the_loop_holds_the_target_in_pixels(enc, dec, decs, orc, fi, si, target):
    fmt, bits, planes, opts = case(fi, si)
    cs, info = enc.encode_measured(dec, [planes], fmt, bits, close_loop=True, target_psnr=target, **opts)
    q, planes_final, passes_final = enc.quality_info(0), enc.last_planes(0), enc.last_passes(0)
    i = info[0]
    print("%s target %g: first %.3f dB, final %.3f dB at target_used %.3f, rounds %d, fell_back %d, short %d, %d bytes" %
          (FS_IDS[FS.index((fi, si))], target, i["first_psnr"], i["diff"]["psnr"], i["target_used"], i["rounds"], i["fell_back"],
           i["short_measured"], len(cs[0])))
    check_loop_frame(enc, decs, fmt, bits, planes, opts, target, cs[0], i, q)
    # a frame goes into a second round exactly when round 1 measured short -- unless round 1 was final by the rule itself
    # (the plane-0 stream already, or the budget decided: nothing finer exists to go to)
    if i["rounds"] == 1 and (q["short_of_target"] or q["capped"]):
        assert i["short_measured"] == int(i["first_psnr"] < target)
    else:
        assert (i["rounds"] > 1) == (i["first_psnr"] < target)
    assert i["fell_back"] == 0                 # the default max_rounds is the worst case measured (7 rounds) plus one
    # the records speak of the final round: the single-frame call at target_used reports the same
    assert (planes_final, passes_final) == (enc.last_planes(0), enc.last_passes(0)) and q == enc.quality_info(0)
    if (fi, si, target) == (0, 2, 44.0):
        # the case the loop exists for: over 5/3 with the RCT the model is about 1 dB optimistic at 44 dB
        assert i["first_psnr"] < 44.0 and i["rounds"] >= 2 and i["diff"]["psnr"] >= 44.0
    if fi in (0, 3):
        check_decodes(cs[0], fmt, orc, decs)


def test_the_loop_on_a_batch(enc, dec, decs):
    """the two rgb24 frames in one call, each on its own way through the rounds"""
    for si in range(len(SETTINGS)):
        fmt, bits, a, opts = case(0, si)
        _, _, b, _ = case(1, si)
        cs, info = enc.encode_measured(dec, [a, b], fmt, bits, close_loop=True, target_psnr=44.0, **opts)
        qs = [enc.quality_info(k) for k in range(2)]
        rcs = [enc.rc_info(k) for k in range(2)]
        for k, planes in enumerate((a, b)):
            assert rcs[k]["final_bytes"] == len(cs[k])
            one, i1 = enc.encode_measured(dec, [planes], fmt, bits, close_loop=True, target_psnr=44.0, **opts)
            assert one[0] == cs[k] and i1[0] == info[k] and enc.quality_info(0) == qs[k]
            check_loop_frame(enc, decs, fmt, bits, planes, opts, 44.0, cs[k], info[k], qs[k])


def test_max_rounds_and_the_fall_back(enc, dec, decs):
    """one quality round only: the frame that is short after it is coded without the target and says so"""
    fmt, bits, planes, opts = case(0, 2)
    cs, info = enc.encode_measured(dec, [planes], fmt, bits, close_loop=True, max_rounds=1, target_psnr=44.0, **opts)
    i = info[0]
    assert i["first_psnr"] < 44.0 and i["rounds"] == 1 and i["fell_back"] == 1 and i["target_used"] == 0
    assert cs[0] == enc.encode(planes, fmt, bits, **opts) and i["diff"]["psnr"] == math.inf and i["short_measured"] == 0
    assert enc.quality_info(0)["target_psnr"] == 0
    check_loop_frame(enc, decs, fmt, bits, planes, opts, 44.0, cs[0], i, enc.quality_info(0))
    for bad in (-1, 17):
        with pytest.raises(m.Htj2kError) as e:
            enc.encode_measured(dec, [planes], fmt, bits, close_loop=True, max_rounds=bad, target_psnr=44.0, **opts)
        assert e.value.code == -22
    # a target above what the quantiser allows: the plane-0 stream at once, short and final
    fmt, bits, planes, opts = case(0, 1)
    cs, info = enc.encode_measured(dec, [planes], fmt, bits, close_loop=True, target_psnr=99.0, **opts)
    q = enc.quality_info(0)
    assert q["short_of_target"] == 1 and info[0]["rounds"] == 1 and info[0]["short_measured"] == 1 and info[0]["fell_back"] == 0
    assert cs[0] == enc.encode(planes, fmt, bits, **opts)


def test_a_budget_that_caps_the_frame_is_left_alone(enc, dec, decs):
    for si in range(len(SETTINGS)):
        fmt, bits, planes, opts = case(0, si)
        free = enc.encode(planes, fmt, bits, target_psnr=44.0, **opts)
        budget = int(len(free) * 0.5)
        cs, info = enc.encode_measured(dec, [planes], fmt, bits, close_loop=True, target_psnr=44.0, target_bytes=budget, **opts)
        q, r = enc.quality_info(0), enc.rc_info(0)
        assert q["capped"] == 1 and len(cs[0]) <= budget and r["final_bytes"] == len(cs[0]) and r["target_bytes"] == budget
        assert info[0]["rounds"] == 1 and info[0]["fell_back"] == 0 and info[0]["short_measured"] == 1
        assert cs[0] == enc.encode(planes, fmt, bits, target_psnr=44.0, target_bytes=budget, **opts)
        check_loop_frame(enc, decs, fmt, bits, planes, opts, 44.0, cs[0], info[0], q, extra=dict(target_bytes=budget))


def test_twice_gives_the_same(enc, dec):
    for fi, si in ((0, 2), (3, 0), (2, 1)):
        fmt, bits, planes, opts = case(fi, si)
        for kw in (dict(), dict(close_loop=True, target_psnr=44.0), dict(close_loop=True, target_psnr=38.0, ht_passes=3)):
            assert enc.encode_measured(dec, [planes], fmt, bits, **opts, **kw) == enc.encode_measured(dec, [planes], fmt, bits, **opts, **kw)
