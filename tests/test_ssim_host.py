"""CPU-only checks of the structural comparison (htj2k_compare_frames_ssim, htj2k_job_compare_ssim,
htj2k_enc_measure_ssim, htj2k_enc_last_ssim): the header's symbols and struct against the binding, the refusals in their
documented order with a NULL context, and the numpy model (ssim_model) against its own definition: the constants, the
window counts, closed forms and a plain loop over windows in exact rationals."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import cmp_model as cm
import ffmpeg_ht_amd as m
import ssim_model as sm
from test_compare_host import frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSYS, PATCHWELCOME = -22, -38, -0x45574150
NEW = ["htj2k_compare_frames_ssim", "htj2k_job_compare_ssim", "htj2k_enc_measure_ssim", "htj2k_enc_last_ssim"]


def test_the_new_symbols_are_exported_and_bound():
    lib = m.load_library()
    header = open(os.path.join(ROOT, "include", "htj2k_amd.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in m.EXPORTS and name + "(" in header, name
    assert hasattr(m, "FrameSsim") and "} htj2k_frame_ssim;" in header
    assert set(m.FrameSsim().as_dict()) == {"q32", "nwin", "ssim", "all"}
    for cls, name in ((m.Decoder, "compare_ssim"), (m.Job, "compare_ssim"), (m.Encoder, "last_ssim")):
        assert hasattr(cls, name)


def test_struct_size_agrees_with_the_binding(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "htj2k_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(htj2k_frame_ssim), '
                   'offsetof(htj2k_frame_ssim, nwin), offsetof(htj2k_frame_ssim, ssim), offsetof(htj2k_frame_ssim, all), '
                   'sizeof(htj2k_frame_diff), sizeof(htj2k_enc_measured)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(m.FrameSsim), m.FrameSsim.nwin.offset, m.FrameSsim.ssim.offset, getattr(m.FrameSsim, "all").offset,
                   ctypes.sizeof(m.FrameDiff), ctypes.sizeof(m.EncMeasured)]
    assert got[:4] == [104, 32, 64, 96] and got[4] == 120        # no struct that existed changed size


def call(a, b, n, bits, out=True, ctx=None):
    L = m.load_library()
    res = (m.FrameSsim * max(n, 1))()
    fa = None if a is None else (m.Frame * len(a))(*a)
    fb = None if b is None else (m.Frame * len(b))(*b)
    return L.htj2k_compare_frames_ssim(ctx, fa, 0, fb, 0, n, bits, res if out else None)


def test_refusals_in_their_order_without_a_context():
    (a, ka), (b, kb) = frame("rgb24", 17, 9), frame("rgb24", 17, 9)
    assert call([a], [b], 1, 8) == ENOSYS                      # valid arguments, no context: ENOSYS comes last
    assert call(None, [b], 1, 8) == EINVAL and call([a], None, 1, 8) == EINVAL and call([a], [b], 1, 8, out=False) == EINVAL
    assert call([a], [b], 0, 8) == EINVAL and call([a], [b], -3, 8) == EINVAL
    for bits in (0, -1, 1, 2, 3, 9, 16):
        assert call([a], [b], 1, bits) == EINVAL               # below 4 bits c1 is 0
    for bits in range(4, 9):
        assert call([a], [b], 1, bits) == ENOSYS
    (p, kp), (q, kq) = frame("pal8", 16, 8), frame("pal8", 16, 8)
    assert call([p], [q], 1, 8) == PATCHWELCOME and call([p], [q], 1, 3) == PATCHWELCOME     # the layout before the depth
    (x, kx), (y, ky) = frame("xyz12le", 9, 9), frame("xyz12le", 9, 9)
    assert call([x], [y], 1, 12) == ENOSYS and call([x], [y], 1, 13) == EINVAL and call([x], [y], 1, 3) == EINVAL
    (g, kg), (g2, kg2) = frame("yuv422p10le", 15, 5), frame("yuv422p10le", 15, 5)
    assert call([g], [g2], 1, 10) == ENOSYS                    # no component has a window: still a valid call
    assert call([g], [g2], 1, 11) == EINVAL
    (c, kc), (d, kd), (e, ke) = frame("rgb24", 16, 9), frame("rgb24", 17, 8), frame("rgba", 17, 9)
    assert call([a], [c], 1, 8) == EINVAL and call([a], [d], 1, 8) == EINVAL and call([a], [e], 1, 8) == EINVAL
    assert call([a, e], [b, frame("rgba", 17, 9)[0]], 2, 8) == EINVAL
    assert call([a, c], [b, frame("rgb24", 16, 9)[0]], 2, 8) == ENOSYS       # sizes may differ from pair to pair
    (s, ks) = frame("rgb24", 17, 9, linesize=50)
    assert call([a], [s], 1, 8) == EINVAL and call([s], [b], 1, 8) == EINVAL
    neg = m.Frame.from_buffer_copy(b)
    neg.linesize[0] = -51
    assert call([a], [neg], 1, 8) == EINVAL
    gone = m.Frame.from_buffer_copy(g2)
    gone.data[2] = None
    assert call([g], [gone], 1, 10) == EINVAL


def test_the_other_entries_refuse_missing_arguments_and_bad_values():
    L = m.load_library()
    out = (m.FrameSsim * 1)()
    fr, keep = frame("gray", 8, 8)
    assert L.htj2k_job_compare_ssim(None, None, ctypes.byref(fr), 0, 0, out) == EINVAL
    # the knob and the switch: no context, no value is accepted; with one, test_ssim_gpu.py checks the ranges
    for v in (-1, 0, 1, 256, 257):
        assert L.htj2k_set_int(None, b"ssim_rows", v) == EINVAL
    for v in (-1, 0, 1, 2):
        assert L.htj2k_enc_measure_ssim(None, v) == EINVAL
    assert L.htj2k_enc_last_ssim(None, 0, out) == EINVAL


def test_the_constants_are_vf_ssims_at_8_bits():
    assert sm.constants(8) == (416, 235963)
    assert sm.constants(3)[0] == 0 and sm.constants(4)[0] == 1           # why fewer than 4 bits are refused
    assert sm.constants(16) == ((64 * 65535 ** 2 + 5000) // 10000, (36288 * 65535 ** 2 + 5000) // 10000)


@pytest.mark.parametrize("bits,fmt", [(4, "gray"), (8, "gray"), (8, "rgb24"), (10, "yuv422p10le"), (12, "xyz12le"), (16, "gray16le")])
def test_window_counts_and_identical_frames(bits, fmt):
    rng = np.random.default_rng(bits)
    sh = cm.shift(fmt, bits)
    dt = np.uint8 if cm.LAYOUTS[fmt][5] == 1 else np.uint16
    for w in (7, 8, 11, 12):
        for h in (7, 8, 11, 12):
            a = [(rng.integers(0, 1 << bits, size=s) << sh).astype(dt) for s in cm.plane_shapes(fmt, w, h)]
            got = sm.ssim(a, a, fmt, bits)
            want = [max((cw >> 2) - 1, 0) * max((ch >> 2) - 1, 0) for cw, ch in cm.comp_dims(fmt, w, h)]
            want += [0] * (4 - len(want))
            assert got["nwin"] == want
            assert got["q32"] == [n << 32 for n in want]                    # v is exactly 1: nwin * 2^32
            assert all(s == 1.0 if n else math.isnan(s) for s, n in zip(got["ssim"], want))
            assert got["all"] == 1.0 if any(want) else math.isnan(got["all"])


@pytest.mark.parametrize("bits", [4, 8, 10, 16])
def test_constant_frames_against_the_closed_form(bits):
    fmt = "gray" if bits <= 8 else "gray16le"
    dt = np.uint8 if bits <= 8 else np.uint16
    sh = cm.shift(fmt, bits)
    c1, _ = sm.constants(bits)
    peak = (1 << bits) - 1
    for x, y in [(0, 0), (0, peak), (peak, peak), (1, peak - 1), (peak // 2, peak // 3), (peak, 0)]:
        a, b = np.full((16, 20), x << sh, dt), np.full((16, 20), y << sh, dt)
        got = sm.ssim([a], [b], fmt, bits)
        # vars = covar = 0, so B = D = c2 and v = A / C up to the roundings of the three operations
        exact = Fraction(2 * 64 * x * 64 * y + c1, (64 * x) ** 2 + (64 * y) ** 2 + c1)
        assert got["nwin"][0] == 12
        assert abs(Fraction(got["q32"][0], 12) - exact * (1 << 32)) <= 0.5 + (1 << 32) * 4 * 2.0 ** -53
        if x == y:
            assert got["q32"][0] == 12 << 32


@pytest.mark.parametrize("bits,w,h,seed", [(8, 20, 20, 1), (8, 13, 9, 2), (10, 20, 12, 3), (10, 9, 17, 4), (16, 20, 20, 5), (16, 8, 8, 6)])
def test_every_window_against_exact_rationals(bits, w, h, seed):
    """a plain loop over windows in fractions.Fraction: every window's q lies within 0.5 (the quantiser) plus
    2^32 * 4 * 2^-53 (three roundings, each at most 2^-53 relative, of a value of magnitude at most 1) of the exact one"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << bits, size=(h, w)).astype(np.int64)
    b = np.where(rng.random((h, w)) < 0.5, a, rng.integers(0, 1 << bits, size=(h, w))).astype(np.int64)
    if seed % 2:
        b = np.clip(a + rng.integers(-1, 2, size=(h, w)), 0, (1 << bits) - 1)
    c1, c2 = sm.constants(bits)
    s = sm.window_sums(a, b)
    q = sm.window_q(*s, bits)
    assert q.shape == ((h >> 2) - 1, (w >> 2) - 1)
    for j in range(q.shape[0]):
        for i in range(q.shape[1]):
            wa = [int(v) for v in a[4 * j:4 * j + 8, 4 * i:4 * i + 8].ravel()]
            wb = [int(v) for v in b[4 * j:4 * j + 8, 4 * i:4 * i + 8].ravel()]
            s1, s2 = sum(wa), sum(wb)
            ss, s12 = sum(x * x for x in wa) + sum(y * y for y in wb), sum(x * y for x, y in zip(wa, wb))
            assert (s1, s2, ss, s12) == tuple(int(t[j, i]) for t in s)
            vars_, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
            exact = Fraction((2 * s1 * s2 + c1) * (2 * covar + c2), (s1 * s1 + s2 * s2 + c1) * (vars_ + c2))
            assert abs(int(q[j, i]) - exact * (1 << 32)) <= 0.5 + (1 << 32) * 4 * 2.0 ** -53, (j, i)
    # the layout path gives the same sum
    fmt = "gray" if bits <= 8 else "gray16le"
    sh = cm.shift(fmt, bits)
    dt = np.uint8 if bits <= 8 else np.uint16
    got = sm.ssim([(a << sh).astype(dt)], [(b << sh).astype(dt)], fmt, bits)
    assert got["q32"][0] == sum(int(v) for v in q.ravel()) and got["nwin"][0] == q.size
