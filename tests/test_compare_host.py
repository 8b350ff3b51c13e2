"""CPU-only checks of the frame comparison (htj2k_compare_frames, htj2k_job_compare, htj2k_encode_batch_measured): the
header's symbols and structs against the binding, the refusals in their documented order with a NULL context, and the
numpy model (cmp_model) against rc_model.psnr."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import cmp_model as cm
import ffmpeg_ht_amd as m
import rc_model as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSYS, PATCHWELCOME = -22, -38, -0x45574150
NEW = ["htj2k_compare_frames", "htj2k_compare_ms", "htj2k_job_compare", "htj2k_encode_batch_measured"]


def test_the_new_symbols_are_exported_and_bound():
    lib = m.load_library()
    header = open(os.path.join(ROOT, "include", "htj2k_amd.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in m.EXPORTS and name + "(" in header, name
    for name in ("FrameDiff", "EncMeasureOpts", "EncMeasured"):
        assert hasattr(m, name), name
    for name in ("htj2k_frame_diff", "htj2k_enc_measure_opts", "htj2k_enc_measured"):
        assert "} %s;" % name in header, name


def test_struct_sizes_agree_with_the_binding(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "htj2k_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(htj2k_frame_diff), '
                   'offsetof(htj2k_frame_diff, max_abs), offsetof(htj2k_frame_diff, psnr), sizeof(htj2k_enc_measure_opts), '
                   'sizeof(htj2k_enc_measured), offsetof(htj2k_enc_measured, first_psnr), '
                   'offsetof(htj2k_enc_measured, short_measured)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(m.FrameDiff), m.FrameDiff.max_abs.offset, m.FrameDiff.psnr.offset,
                   ctypes.sizeof(m.EncMeasureOpts), ctypes.sizeof(m.EncMeasured), m.EncMeasured.first_psnr.offset,
                   m.EncMeasured.short_measured.offset]
    assert got[0] == 120 and got[3] == 8


def frame(fmt, w, h, bits=None, linesize=None):
    """(Frame, arrays) of zeros in the layout"""
    fr, keep = m.Frame(), []
    bytes_ = 1 if fmt == "pal8" else cm.LAYOUTS[fmt][5]
    for p, (rows, cols) in enumerate([(h, w)] if fmt == "pal8" else cm.plane_shapes(fmt, w, h)):
        ls = cols * bytes_ if linesize is None else linesize
        a = np.zeros((rows, max(ls, 1)), np.uint8)
        keep.append(a)
        fr.data[p] = a.ctypes.data
        fr.linesize[p] = ls
    fr.width, fr.height, fr.pix_fmt = w, h, m.PIX_NAMES.index(fmt)
    return fr, keep


def call(a, b, n, bits, out=True, ctx=None):
    L = m.load_library()
    res = (m.FrameDiff * max(n, 1))()
    fa = None if a is None else (m.Frame * len(a))(*a)
    fb = None if b is None else (m.Frame * len(b))(*b)
    return L.htj2k_compare_frames(ctx, fa, 0, fb, 0, n, bits, res if out else None)


def test_refusals_in_their_order_without_a_context():
    (a, ka), (b, kb) = frame("rgb24", 17, 5), frame("rgb24", 17, 5)
    assert call([a], [b], 1, 8) == ENOSYS                      # valid arguments, no context
    assert call(None, [b], 1, 8) == EINVAL and call([a], None, 1, 8) == EINVAL and call([a], [b], 1, 8, out=False) == EINVAL
    assert call([a], [b], 0, 8) == EINVAL and call([a], [b], -3, 8) == EINVAL
    for bits in (0, -1, 9, 16):
        assert call([a], [b], 1, bits) == EINVAL               # EINVAL before ENOSYS
    for bits in range(1, 9):
        assert call([a], [b], 1, bits) == ENOSYS
    (p, kp), (q, kq) = frame("pal8", 16, 4), frame("pal8", 16, 4)
    assert call([p], [q], 1, 8) == PATCHWELCOME                # indices are not samples
    (x, kx), (y, ky) = frame("xyz12le", 9, 3), frame("xyz12le", 9, 3)
    assert call([x], [y], 1, 12) == ENOSYS and call([x], [y], 1, 13) == EINVAL
    (g, kg), (g2, kg2) = frame("yuv422p10le", 15, 5), frame("yuv422p10le", 15, 5)
    assert call([g], [g2], 1, 10) == ENOSYS and call([g], [g2], 1, 9) == ENOSYS and call([g], [g2], 1, 11) == EINVAL
    # frames of a pair that differ in size or layout; a batch of two layouts
    (c, kc) = frame("rgb24", 16, 5)
    (d, kd) = frame("rgb24", 17, 4)
    (e, ke) = frame("rgba", 17, 5)
    assert call([a], [c], 1, 8) == EINVAL and call([a], [d], 1, 8) == EINVAL and call([a], [e], 1, 8) == EINVAL
    (e2, ke2) = frame("rgba", 17, 5)
    assert call([a, e], [b, e2], 2, 8) == EINVAL
    assert call([a, c], [b, frame("rgb24", 16, 5)[0]], 2, 8) == ENOSYS       # sizes may differ from pair to pair
    # a missing plane, a short and a negative linesize
    (s, ks) = frame("rgb24", 17, 5, linesize=50)
    assert call([a], [s], 1, 8) == EINVAL and call([s], [b], 1, 8) == EINVAL
    (l, kl) = frame("rgb24", 17, 5, linesize=52)
    assert call([a], [l], 1, 8) == ENOSYS                      # linesize may exceed the row, by an odd amount too
    (o, ko) = frame("gray16le", 7, 3, linesize=15)             # 16-bit samples on an odd linesize
    assert call([o], [frame("gray16le", 7, 3)[0]], 1, 16) == ENOSYS
    (o2, ko2) = frame("gray16le", 7, 3, linesize=13)
    assert call([o2], [o], 1, 16) == EINVAL
    neg = m.Frame.from_buffer_copy(b)
    neg.linesize[0] = -51
    assert call([a], [neg], 1, 8) == EINVAL
    gone = m.Frame.from_buffer_copy(g2)
    gone.data[2] = None
    assert call([g], [gone], 1, 10) == EINVAL
    zero = m.Frame.from_buffer_copy(b)
    zero.width = 0
    assert call([zero], [zero], 1, 8) == EINVAL


def test_the_other_entries_refuse_missing_arguments():
    L = m.load_library()
    ms = ctypes.c_float()
    assert L.htj2k_compare_ms(None, ctypes.byref(ms)) == EINVAL
    out = (m.FrameDiff * 1)()
    fr, keep = frame("gray", 4, 4)
    assert L.htj2k_job_compare(None, None, ctypes.byref(fr), 0, 0, out) == EINVAL
    offs = (ctypes.c_size_t * 2)()
    res = (m.EncMeasured * 1)()
    buf = ctypes.create_string_buffer(1 << 16)
    o = m._enc_opts(levels=1)
    # arguments before the contexts, then ENOSYS as the encoder's unit entries answer
    assert L.htj2k_encode_batch_measured(None, None, None, 1, 8, ctypes.byref(o), None, 0, buf, ctypes.c_size_t(1 << 16), 0,
                                         offs, res) == EINVAL
    assert L.htj2k_encode_batch_measured(None, None, ctypes.byref(fr), 1, 8, ctypes.byref(o), None, 0, buf,
                                         ctypes.c_size_t(1 << 16), 0, offs, None) == EINVAL
    bad = m.EncMeasureOpts(1, 17)
    assert L.htj2k_encode_batch_measured(None, None, ctypes.byref(fr), 1, 8, ctypes.byref(o), ctypes.byref(bad), 0, buf,
                                         ctypes.c_size_t(1 << 16), 0, offs, res) == EINVAL
    assert L.htj2k_encode_batch_measured(None, None, ctypes.byref(fr), 1, 8, ctypes.byref(o), None, 0, buf,
                                         ctypes.c_size_t(1 << 16), 0, offs, res) == ENOSYS


@pytest.mark.parametrize("fmt,bits", [("gray", 8), ("rgb24", 8), ("ya8", 7), ("rgb48le", 16), ("rgb48le", 12), ("gray16le", 16),
                                      ("yuv420p", 8), ("yuv422p10le", 10), ("yuv422p10le", 9), ("yuva444p16le", 16),
                                      ("xyz12le", 12)])
def test_the_model_against_rc_model_psnr(fmt, bits):
    rng = np.random.default_rng(7)
    w, h = 33, 9
    dt = np.uint8 if cm.LAYOUTS[fmt][5] == 1 else np.uint16
    sh = cm.shift(fmt, bits)
    a = [rng.integers(0, 1 << bits, size=s).astype(dt) << sh for s in cm.plane_shapes(fmt, w, h)]
    b = [rng.integers(0, 1 << bits, size=s).astype(dt) << sh for s in cm.plane_shapes(fmt, w, h)]
    d = cm.compare(a, b, fmt, bits)
    want = rc.psnr([p >> sh for p in a], [p >> sh for p in b], bits)
    assert abs(d["psnr"] - want) < 1e-9
    nc = cm.LAYOUTS[fmt][0]
    assert d["nsamples"][:nc] == [cw * ch for cw, ch in cm.comp_dims(fmt, w, h)] and d["nsamples"][nc:] == [0] * (4 - nc)
    # bits below the shift and above the sample change nothing
    dirt = [p | dt(rng.integers(0, 1 << sh)) if sh else p for p in a]
    if sh + bits < 8 * cm.LAYOUTS[fmt][5]:
        dirt = [p | dt(1 << (sh + bits)) for p in dirt]
    assert cm.compare(dirt, b, fmt, bits) == d
    same = cm.compare(a, a, fmt, bits)
    assert same["psnr"] == math.inf and sum(same["sse"]) == 0 and sum(same["ndiff"]) == 0 and sum(same["max_abs"]) == 0
    assert rc.psnr(a, a, bits) == math.inf
    # by hand: one sample off by 3 in component 0
    c = [p.copy() for p in a]
    v = (int(c[0][0, 0]) >> sh) & ((1 << bits) - 1)
    c[0][0, 0] = dt((v - 3 if v >= 3 else v + 3) << sh)
    one = cm.compare(a, c, fmt, bits)
    assert one["sse"] == [9, 0, 0, 0] and one["ndiff"] == [1, 0, 0, 0] and one["max_abs"] == [3, 0, 0, 0]
