"""CPU-only checks of the frame checksums (htj2k_hash_frames, htj2k_job_hash, htj2k_pipe_receive_hash): the header's
symbols and struct against the binding, the refusals in their documented order with a NULL context, the numpy / zlib
model (hash_model) against oracle.framecrc and the golden framecrcs, and the two steps the device takes -- the grouped
sums of k_frame_adler with 64-bit accumulators, the combination of the planes -- against zlib.adler32(., 0)."""
import ctypes
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import cmp_model as cm
import ffmpeg_ht_amd as m
import hash_model as hm
import oracle
import streams

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL, ENOSYS = -22, -38
NEW = ["htj2k_hash_frames", "htj2k_job_hash", "htj2k_pipe_receive_hash"]
KATS = json.load(open(os.path.join(HERE, "golden", "kats.json")))


def test_the_new_symbols_are_exported_and_bound():
    lib = m.load_library()
    header = open(os.path.join(ROOT, "include", "htj2k_amd.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in m.EXPORTS and name + "(" in header, name
    assert hasattr(m, "FrameHash") and "} htj2k_frame_hash;" in header
    assert all(hasattr(c, n) for c, n in ((m.Decoder, "framecrc"), (m.Job, "framecrc"), (m.Pipe, "receive_crc")))


def test_struct_size_agrees_with_the_binding(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "htj2k_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(htj2k_frame_hash), '
                   'offsetof(htj2k_frame_hash, plane_adler32), offsetof(htj2k_frame_hash, nbytes)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(m.FrameHash), m.FrameHash.plane_adler32.offset, m.FrameHash.nbytes.offset] == [32, 4, 24]


def frame(fmt, w, h, linesize=None):
    """(Frame, arrays) of zeros in the layout"""
    fr, keep = m.Frame(), []
    for p, (rows, rowbytes) in enumerate(hm.plane_geometry(fmt, w, h)):
        ls = rowbytes if linesize is None else linesize
        a = np.zeros((rows, max(ls, 1)), np.uint8)
        keep.append(a)
        fr.data[p] = a.ctypes.data
        fr.linesize[p] = ls
    fr.width, fr.height, fr.pix_fmt = w, h, m.PIX_NAMES.index(fmt)
    return fr, keep


def call(frames, n, out=True, ctx=None):
    L = m.load_library()
    res = (m.FrameHash * max(n, 1))()
    arr = None if frames is None else (m.Frame * len(frames))(*frames)
    return L.htj2k_hash_frames(ctx, arr, 0, n, res if out else None)


def test_refusals_in_their_order_without_a_context():
    (a, ka), (b, kb) = frame("rgb24", 17, 5), frame("yuv422p10le", 15, 5)
    assert call([a], 1) == ENOSYS and call([a, b], 2) == ENOSYS   # valid arguments, layouts and sizes may differ: no context
    assert call(None, 1) == EINVAL and call([a], 1, out=False) == EINVAL
    assert call([a], 0) == EINVAL and call([a], -3) == EINVAL
    for fmt in m.PIX_NAMES:                                      # every layout of the enum is in scope, pal8 and xyz12le too
        f, k = frame(fmt, 9, 3)
        assert call([f], 1) == ENOSYS, fmt
    for bad in (-1, len(m.PIX_NAMES), 1000):
        f = m.Frame.from_buffer_copy(a)
        f.pix_fmt = bad
        assert call([f], 1) == EINVAL and call([a, f], 2) == EINVAL
    for field in ("width", "height"):
        for v in (0, -4):
            f = m.Frame.from_buffer_copy(a)
            setattr(f, field, v)
            assert call([f], 1) == EINVAL
    gone = m.Frame.from_buffer_copy(b)
    gone.data[2] = None
    assert call([gone], 1) == EINVAL and call([a, gone], 2) == EINVAL
    pal, kp = frame("pal8", 16, 4)
    assert call([pal], 1) == ENOSYS
    nopal = m.Frame.from_buffer_copy(pal)
    nopal.data[1] = None
    assert call([nopal], 1) == EINVAL                           # the palette is a plane of the frame
    shortpal = m.Frame.from_buffer_copy(pal)
    shortpal.linesize[1] = 1023
    assert call([shortpal], 1) == EINVAL
    (s, ks), (l, kl) = frame("rgb24", 17, 5, linesize=50), frame("rgb24", 17, 5, linesize=52)
    assert call([s], 1) == EINVAL and call([l], 1) == ENOSYS    # linesize may exceed the row, by an odd amount too
    (o, ko), (o2, ko2) = frame("gray16le", 7, 3, linesize=15), frame("gray16le", 7, 3, linesize=13)
    assert call([o], 1) == ENOSYS and call([o2], 1) == EINVAL
    neg = m.Frame.from_buffer_copy(a)
    neg.linesize[0] = -51
    assert call([neg], 1) == EINVAL
    L = m.load_library()
    out = (m.FrameHash * 1)()
    assert L.htj2k_job_hash(None, None, out) == EINVAL
    assert L.htj2k_pipe_receive_hash(None, None, out) == EINVAL


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_the_model_on_the_known_answers(orc, kat):
    info, planes, _ = orc.decode(bytes.fromhex(kat["hex"]))
    got = hm.frame_hash(planes, info)
    assert got["adler32"] == oracle.framecrc(planes) == int(kat["framecrc"], 16)
    assert got == hm.frame_hash(planes)
    assert got["nbytes"] == sum(np.asarray(p).nbytes for p in planes)
    if len(planes) == 1:
        assert got["plane_adler32"] == [got["adler32"], 0, 0, 0]


@pytest.mark.parametrize("name", ["pal8_jp2", "yuv422p12_97", "rgb_mct", "gray16"])
def test_the_model_on_decoded_layouts(orc, name):
    data, kw = streams.get(name)
    info, planes, _ = orc.decode(data, **kw)
    got = hm.frame_hash(planes, info)
    assert got["adler32"] == oracle.framecrc(planes) and got["nbytes"] == sum(np.asarray(p).nbytes for p in planes)
    fmt = oracle.PIX_NAMES[info.pix_fmt]
    assert hm.info_geometry(info) == hm.plane_geometry(fmt, info.width, info.height)
    # the rows padded with dirt: only the geometry's bytes count
    wide = [np.pad(np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1), ((0, 2), (0, 13)), constant_values=0xAB) for p in planes]
    assert hm.frame_hash(wide, info) == got


LENGTHS = [1, 15, 16, 17, 5552, 5553, 65520, 65521, 65522, 1 << 20]


@pytest.mark.parametrize("n", LENGTHS)
def test_the_grouped_sums_against_zlib(n):
    rng = np.random.default_rng(n)
    for data in (rng.integers(0, 256, size=n, dtype=np.uint8).tobytes(), b"\xff" * n):
        A, B = hm.grouped_sums(data)
        assert hm.adler_of(A, B) == zlib.adler32(data, 0) & 0xFFFFFFFF
        # as rows of a plane: short last groups inside the data, weights that wrap within a row and across rows
        for rowbytes in (1, 7, 16, 17, 48, 49, 5552, 65521):
            if n % rowbytes == 0 and n // rowbytes <= 70000:
                assert hm.grouped_sums(data, rowbytes) [0] == A
                assert hm.adler_of(*hm.grouped_sums(data, rowbytes)) == zlib.adler32(data, 0) & 0xFFFFFFFF, rowbytes


def test_the_accumulator_bounds():
    # a group adds less than 2^29 to B: (2 * 65521 - 1) * 16 * 255; exact below 2^38 bytes a plane, the decoder's largest has 2^33
    assert (2 * hm.MOD - 1) * 16 * 255 < 1 << 29
    assert ((1 << 38) >> 4) * (1 << 29) <= 1 << 64 and 32768 * 32768 * 8 == 1 << 33
    assert (hm.MOD - 1) ** 2 < 1 << 32                           # (rows - y) mod M times rowbytes mod M in 32 bits


@pytest.mark.parametrize("fmt", ["gray", "rgb24", "yuv420p", "yuv422p10le", "yuva444p16le", "pal8", "xyz12le", "ya16le"])
def test_the_planes_combine_to_the_frame(fmt):
    rng = np.random.default_rng(len(fmt))
    for w, h in ((1, 1), (17, 5), (300, 73), (257, 3)):
        geo = hm.plane_geometry(fmt, w, h)
        planes = [rng.integers(0, 256, size=(rows, rb), dtype=np.uint8) for rows, rb in geo]
        want = hm.frame_hash(planes)
        assert want["adler32"] == oracle.framecrc(planes) and want["nbytes"] == sum(r * b for r, b in geo)
        parts = [hm.grouped_sums(p.tobytes(), rb) + (p.size,) for p, (_, rb) in zip(planes, geo)]
        assert [hm.adler_of(a, b) for a, b, _ in parts] + [0] * (4 - len(parts)) == want["plane_adler32"]
        assert hm.combine(parts) == want["adler32"]
    if fmt in cm.LAYOUTS:
        assert [r * b for r, b in hm.plane_geometry(fmt, 9, 7)] == [r * c * cm.LAYOUTS[fmt][5] for r, c in cm.plane_shapes(fmt, 9, 7)]
