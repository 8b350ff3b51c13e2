"""What htj2k_hash_frames, htj2k_compare_frames and htj2k_compare_frames_ssim have in common: one staged call on the
context's stream, whose pinned staging image, device image, plane table and results region are used again by the next
call whatever its entry size (CmpPlane, HashPlane), slot size (CmpSums, SsimSums, HashSums) and number of planes.

One Decoder takes six calls of unlike shapes, then the same six in reverse order: the staging buffer grows, shrinks in
use and is filled by another metric in between.  Every answer must be the model's (cmp_model, ssim_model, hash_model:
integers and q32 for equality) and, figure for figure, what a fresh Decoder gives for that call alone; compare_ms() is
positive after a call that launched something and 0 after the one that had nothing to launch."""
import math

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: device operands are made through it)

import cmp_model as cm
import ffmpeg_ht_amd as m
import ssim_model as sm
from test_compare_gpu import pair
from test_hash_gpu import HFrame
from test_ssim_gpu import identical

HASHED = [("rgb24", 65, 5), ("yuv422p10le", 17, 9), ("pal8", 33, 9)]


def build_steps():
    """[(name, call(dec) -> results, the models' results, same(got, want), exact(got, other), launches)]"""
    keep = []                                           # what Frames point into, for as long as the steps are used
    rng = np.random.default_rng(31)
    hs = [HFrame(fmt, w, h, rng, ls, off) for (fmt, w, h), ls, off in zip(HASHED, ("row+13", "to64", "row+1"), (1, 0, 2))]
    keep.append(hs)
    h_host = [f.frame() for f in hs]
    h_dev = []
    for f in hs:
        fr, ts = f.on_device()
        h_dev.append(fr)
        keep.append(ts)
    h_want = [f.want() for f in hs]

    def dev(o):
        fr, ts = o.on_device()
        keep.append(ts)
        return fr

    s_a, s_b = pair("gray16le", 257, 12, 12, 41, "row+1", 2, "to64", 0)
    s_fa, s_fb = dev(s_a), dev(s_b)
    mixed = [pair("rgb24", 65, 5, 8, 42, "row+13", 1, "row", 15), pair("yuv422p10le", 17, 9, 10, 43, "to64", 0, "row+1", 2)]
    x_a, x_b = [[a.frame()] for a, _ in mixed], [[dev(b)] for _, b in mixed]
    n_a, n_b = pair("gray", 7, 3, 8, 44, "row+1", 1, "row+13", 2)       # no 8 x 8 window: nothing to launch
    r_a, r_b = pair("rgba64le", 5, 5, 16, 45, "row+13", 1, "to64", 2)

    def mixed_call(dec):                                                # one layout a call: the two pairs one after the other
        out = []
        for (a, _), fa, fb in zip(mixed, x_a, x_b):
            out += dec.compare(fa, fb, a.fmt, a.bits, on_device=(False, True))
        return out

    diff_same = lambda g, w: len(g) == len(w) and all(cm.same(x, y) for x, y in zip(g, w))
    diff_exact = lambda g, w: len(g) == len(w) and all(cm.same(x, y, tol=0) for x, y in zip(g, w))
    ssim_same = lambda g, w: len(g) == len(w) and all(sm.same(x, y) for x, y in zip(g, w))
    equal = lambda g, w: g == w
    steps = [
        ("framecrc host", lambda dec: dec.framecrc(h_host, None), h_want, equal, equal, True),
        ("ssim device", lambda dec: dec.compare_ssim([s_fa], [s_fb], "gray16le", 12, on_device=(True, True)),
         [sm.ssim(s_a.raw_planes(), s_b.raw_planes(), "gray16le", 12)], ssim_same, identical, True),
        ("compare host/device", mixed_call, [cm.compare(a.raw_planes(), b.raw_planes(), a.fmt, a.bits) for a, b in mixed],
         diff_same, diff_exact, True),
        ("ssim no window", lambda dec: dec.compare_ssim([n_a.frame()], [n_b.frame()], "gray", 8),
         [sm.ssim(n_a.raw_planes(), n_b.raw_planes(), "gray", 8)], ssim_same, identical, False),
        ("framecrc device", lambda dec: dec.framecrc(h_dev, None, on_device=True), h_want, equal, equal, True),
        ("compare host", lambda dec: dec.compare([r_a.frame()], [r_b.frame()], "rgba64le", 16),
         [cm.compare(r_a.raw_planes(), r_b.raw_planes(), "rgba64le", 16)], diff_same, diff_exact, True),
    ]
    return steps, keep


@pytest.mark.gpu
def test_one_context_through_calls_of_unlike_shapes():
    steps, keep = build_steps()
    alone = []
    for name, call, want, same, exact, launches in steps:               # every call on a context of its own
        d = m.Decoder(device_id=0)
        try:
            alone.append(call(d))
        finally:
            d.close()
        assert same(alone[-1], want), (name, alone[-1], want)
    none = steps[3][2][0]
    assert none["nwin"] == [0] * 4 and math.isnan(none["all"]) and all(math.isnan(s) for s in none["ssim"])
    dec = m.Decoder(device_id=0)
    try:
        for order in (range(len(steps)), reversed(range(len(steps)))):
            for k in order:
                name, call, want, same, exact, launches = steps[k]
                got = call(dec)
                ms = dec.compare_ms()
                print("%-20s compare_ms %.4f" % (name, ms))
                assert same(got, want), (name, got, want)
                assert exact(got, alone[k]), (name, got, alone[k])
                assert (ms > 0) if launches else (ms == 0), (name, ms)
    finally:
        dec.close()
    del keep
