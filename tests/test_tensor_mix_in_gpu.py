"""Tensors as frames through a colour matrix and a chroma filter on the GPU: htj2k_tensor_to_frames_mix against the numpy
model (tensor_mix_in_model), every byte of every plane buffer, and htj2k_encode_tensor_mix against the encoder's own
streams of those frames, byte for byte.

Twelve layouts, three element types, two tensor layouts, K = 1 .. 4 and both chroma rules; widths and heights 1, 2, 3 and
5 and the 256-footprint seam of the encoder's kernel; destinations with padded linesizes and bases off the 16-byte
alignment between 0xC3 guard zones.  Run as a program, the module runs the equalities on its own contexts:
test_equalities_on_poisoned_buffers does that in a child process under HTJ2K_POISON=1."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [HERE, ROOT]

import cmp_model as cm
import ffmpeg_ht_amd as m
import tensor_mix_in_model as tmi
import tensor_model as tm
from test_tensor_in_gpu import picture, to_device
from test_tensor_mix_in_host import ROUND_TRIP_LAYOUTS, check_against_torch, random_mix, round_trip_planes, torch_frames

LAYOUTS = ["gray", "ya8", "rgb24", "rgba", "rgb48le", "yuv444p12le", "yuv422p10le", "yuv420p", "yuv411p", "yuv410p", "yuva420p", "xyz12le"]
COMBOS = [(d, l) for d in tm.DTYPES for l in ("NCHW", "NHWC")]
TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
EINVAL, PATCHWELCOME = -22, -0x45574150
GUARD = 0xC3
SMALL = [1, 2, 3, 5]


def seam(fmt):
    """widths around the 256-footprint seam of k_enc_unpack_tensor_mix: 256 footprints of 1 << sw pixels, +- 1"""
    s = 256 << cm.LAYOUTS[fmt][2]
    return [s - 1, s, s + 1]


def shaped(v, layout):
    return v if layout == "NCHW" else np.ascontiguousarray(v.transpose(0, 2, 3, 1))


def a_mix(fmt, K, chroma, rng, bits):
    """weights that keep a picture in [0, 1] mostly inside the range, some of them negative, one of them -0"""
    nc, peak = cm.LAYOUTS[fmt][0], (1 << bits) - 1
    mat = rng.uniform(-0.2, 1.0, size=(nc, K)) * (peak / (0.6 * K))
    mat[rng.integers(nc), rng.integers(K)] = -0.0
    return mat.astype(np.float32), rng.uniform(-2.0, 0.1 * peak, size=nc).astype(np.float32), chroma


def struct_of(mix):
    return m.tensor_mix_in(mix[0], mix[1], mix[2])


# ------------------------------------------------------------------ htj2k_tensor_to_frames_mix against the model

class Guarded:
    """n destination frames in device memory, every plane with a linesize and a base offset of its own inside a buffer of
    0xC3 bytes"""

    def __init__(self, fmt, w, h, n, pad, off):
        self.geo = m.plane_geometry(m.PIX_NAMES.index(fmt), w, h)
        self.off, self.ls = off, [rb + pad for _, rb in self.geo]
        self.bufs = [[torch.full((off + ls * rows + 32,), GUARD, dtype=torch.uint8, device="cuda") for (rows, _), ls in zip(self.geo, self.ls)]
                     for _ in range(n)]
        self.arr = (m.Frame * n)()
        for i in range(n):
            self.arr[i].width, self.arr[i].height, self.arr[i].pix_fmt = w, h, m.PIX_NAMES.index(fmt)
            for p, b in enumerate(self.bufs[i]):
                self.arr[i].data[p] = b.data_ptr() + off
                self.arr[i].linesize[p] = self.ls[p]
        torch.cuda.synchronize()

    def expect(self, want):
        """every byte of every buffer: the model's rows in their places, 0xC3 everywhere else"""
        for i, planes in enumerate(want):
            for p, (rows, rb) in enumerate(self.geo):
                exp = np.full(self.bufs[i][p].numel(), GUARD, np.uint8)
                rows_bytes = np.ascontiguousarray(planes[p]).view(np.uint8).reshape(rows, rb)
                for y in range(rows):
                    exp[self.off + y * self.ls[p]: self.off + y * self.ls[p] + rb] = rows_bytes[y]
                got = self.bufs[i][p].cpu().numpy()
                bad = np.flatnonzero(got != exp)
                assert bad.size == 0, (i, p, len(bad), bad[:6].tolist(), got[bad[:6]].tolist(), exp[bad[:6]].tolist())

    def untouched(self):
        return all(bool((b == GUARD).all()) for bufs in self.bufs for b in bufs)


def to_frames_mix(dec, t, tbits, fmt, bits, dtype, layout, w, h, mix, pad=0, off=0):
    n = t.shape[0]
    dst = Guarded(fmt, w, h, n, pad, off)
    spec, s = m.tensor_spec(dtype, layout), struct_of(mix)
    r = dec.L.htj2k_tensor_to_frames_mix(dec.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * t.element_size()), n, int(bits),
                                         ctypes.byref(spec), ctypes.byref(s), dst.arr)
    what = (fmt, bits, dtype, layout, w, h, n, mix[2], mix[0].shape, pad, off)
    assert r == 0, (r, what)
    want = tmi.frames(tbits, fmt, bits, mix, dtype, layout)
    try:
        dst.expect(want)
    except AssertionError as e:
        raise AssertionError((what, e.args))
    return want


PADS, OFFS = [0, 1, 13, 5], [0, 1, 2, 15]


def check_layout(dec, fmt):
    """every small width and the seam with every element type and tensor layout; heights, K, the chroma rule, paddings,
    offsets and batch sizes change from call to call, so that every K meets both rules on every layout"""
    depth = cm.LAYOUTS[fmt][4]
    rng = np.random.default_rng(LAYOUTS.index(fmt))
    j = LAYOUTS.index(fmt)
    seen = set()
    for w in SMALL + seam(fmt):
        for dtype, layout in COMBOS:
            j += 1
            h, n, K, chroma = SMALL[j % 4], 1 + j % 2, 1 + (j // 2) % 4, (j // 8 + j) % 2
            seen.add((K, chroma))
            t, tbits = to_device(shaped(picture(n, K, h, w, rng), layout), dtype)
            to_frames_mix(dec, t, tbits, fmt, depth, dtype, layout, w, h, a_mix(fmt, K, chroma, rng, depth), PADS[j % 4], OFFS[(j // 4) % 4])
    assert len(seen) == 8, seen


def special_values(bits):
    peak = (1 << bits) - 1
    return [np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, 0.5, 1.5, 2.5, 3.5, 6e-8, 6.1e-5, 1e-40, 3e38, -3e38, peak - 0.5, peak + 0.5, peak,
            65504.0, 1e-45, 7.0]


def check_values(enc, dec):
    """NaN, infinities, -0, ties, subnormals: through the identity, through a weight of -0.0, through inf * 0, and in sums
    that overflow to +inf (the peak) and to -inf (0); box footprints that hold them; the codestreams agree with the frames"""
    f32 = np.float32
    for fmt, bits in (("gray", 8), ("yuv422p10le", 10), ("yuv420p", 8), ("rgb24", 8), ("rgb48le", 16)):
        nc = cm.LAYOUTS[fmt][0]
        vals = np.array(special_values(bits), f32)
        w, h = len(vals), 4
        img = np.stack([np.stack([np.roll(vals, k + 3 * y) for y in range(h)]) for k in range(3)])[None]       # (1, 3, h, w)
        eye = np.zeros((nc, 3), f32)
        eye[np.arange(nc), np.arange(nc) % 3] = 1.0
        minus0 = eye.copy()
        minus0[eye == 0] = -0.0
        mixes = [(eye, None), (minus0, np.full(nc, 0.5, f32)), (np.ones((nc, 3), f32), None), (np.array([[1.0, -1.0, 0.0]] * nc, f32), None),
                 (np.array([[2.0, 2.0, 2.0]] * nc, f32), np.full(nc, -3e38, f32))]
        for ci, (dtype, layout) in enumerate(COMBOS):
            t, tbits = to_device(shaped(img, layout), dtype)
            for mi, (mat, off) in enumerate(mixes):
                chroma = (ci + mi) % 2
                mix = (mat, off, chroma)
                want = to_frames_mix(dec, t, tbits, fmt, bits, dtype, layout, w, h, mix, PADS[ci % 4], OFFS[mi % 4])
                if fmt != "rgb48le" and mi in (0, 2):
                    got = enc.encode_tensor(t, fmt, bits, layout, mix=struct_of(mix), levels=1)
                    assert got == enc.encode_batch(want, fmt, bits, levels=1), (fmt, dtype, layout, mi)
    # what the model says of them, spelled out once: one channel through a weight of 1
    one, obits = to_device(np.array(special_values(8)[:10], f32).reshape(1, 1, 1, 10), "float32")
    want = to_frames_mix(dec, one, obits, "gray", 8, "float32", "NCHW", 10, 1, (np.array([[1.0]], f32), None, 0))
    assert want[0][0].tolist() == [[0, 0, 255, 0, 0, 0, 0, 0, 2, 2]]
    # sums that overflow: 3e38 + 3e38 is +inf (the peak), -3e38 - 3e38 is -inf (0); inf * 0 is NaN (0)
    cols = np.array([[3e38, -3e38, np.inf, 1.0], [3e38, -3e38, 5.0, 1.0]], f32).reshape(1, 2, 1, 4)
    t, tbits = to_device(cols, "float32")
    want = to_frames_mix(dec, t, tbits, "gray", 8, "float32", "NCHW", 4, 1, (np.array([[1.0, 1.0]], f32), None, 0))
    assert want[0][0].tolist() == [[255, 0, 255, 2]]
    want = to_frames_mix(dec, t, tbits, "gray", 8, "float32", "NCHW", 4, 1, (np.array([[0.0, 1.0]], f32), None, 0))
    assert want[0][0].tolist() == [[255, 0, 0, 1]]
    # binary16 subnormals scaled up to samples
    tb = np.array([0x0001, 0x03FF, 0x8001, 0x0200], np.uint16).reshape(1, 1, 2, 2)
    t = torch.from_numpy(tb.view(np.int16)).view(torch.float16).cuda()
    torch.cuda.synchronize()
    want = to_frames_mix(dec, t, tb, "gray16le", 16, "float16", "NCHW", 2, 2, (np.array([[2.0 ** 24]], f32), None, 1))
    assert want[0][0].tolist() == [[1, 1023], [0, 512]]


# ------------------------------------------------------------------ htj2k_encode_tensor_mix against the encoder's own streams

def three_ways(enc, dec, t, tbits, fmt, bits, dtype, layout, mix, opts):
    """encode_tensor(mix=), encode_device(from_tensor(mix=)) and encode_batch(model frames): equal streams"""
    n = t.shape[0]
    s = struct_of(mix)
    got = enc.encode_tensor(t, fmt, bits, layout, mix=s, **opts)
    ms = enc.stage_ms()
    frames, keep = dec.from_tensor(t, fmt, bits, layout, mix=s)
    via = enc.encode_device(list(frames), fmt, bits, **opts)
    model = tmi.frames(tbits, fmt, bits, mix, dtype, layout)
    ref = enc.encode_batch(model, fmt, bits, **opts)
    what = (fmt, bits, dtype, layout, tuple(t.shape), mix[2], opts)
    assert len(got) == n and all(len(x) > 0 for x in got), what
    assert ref == via, ("from_tensor(mix=)'s frames encode differently from the model's", what)
    assert got == via, ("encode_tensor(mix=) differs from the encode of its frames", what, [k for k in range(n) if got[k] != via[k]])
    assert ms[0] > 0, ms
    del keep
    return got


BGR = np.array([[0, 0, 255.0], [0, 255.0, 0], [255.0, 0, 0]], np.float32)
# (layout, bits, w, h, n, element, tensor layout, mix: "bgr" / "rgb" (htj2k_tensor_mix_in_rgb) / K for a random one, chroma, options)
EQUAL = [
    ("rgb24", 8, 257, 3, 1, "float16", "NCHW", "bgr", 0, dict(levels=1)),
    ("rgb24", 8, 255, 5, 3, "float32", "NHWC", "bgr", 0, dict(levels=2, irreversible=True, qstep=0.5)),
    ("rgb24", 8, 64, 48, 3, "bfloat16", "NCHW", "bgr", 1, dict(levels=3, group_bytes="half")),
    ("rgb24", 8, 40, 24, 2, "float32", "NCHW", 4, 0, dict(levels=2, mct=0, tile=(16, 16))),
    ("yuv422p10le", 10, 513, 3, 1, "float32", "NCHW", "rgb", 0, dict(levels=1)),
    ("yuv422p10le", 10, 511, 2, 2, "float16", "NHWC", "rgb", 1, dict(levels=1, irreversible=True)),
    ("yuv422p10le", 10, 64, 48, 2, "float32", "NHWC", "rgb", 1, dict(levels=3, irreversible=True, qstep=0.25, target_psnr=34.0)),
    ("yuv422p10le", 10, 65, 47, 1, "bfloat16", "NCHW", "rgb", 0, dict(levels=3, target_bytes="half")),
    ("yuv420p", 8, 512, 5, 1, "float32", "NHWC", "rgb", 1, dict(levels=1)),
    ("yuv420p", 8, 513, 3, 2, "float16", "NCHW", "rgb", 0, dict(levels=1, irreversible=True, qstep=0.5)),
    ("yuv420p", 8, 65, 47, 1, "float32", "NCHW", "rgb", 1, dict(levels=3, irreversible=True, qstep=0.5, target_bytes="half", ht_passes=3)),
    ("yuv420p", 8, 64, 48, 1, "float16", "NHWC", "rgb", 0, dict(levels=3, ht_passes=3)),
    ("yuv420p", 8, 40, 24, 3, "bfloat16", "NHWC", "rgb", 1, dict(levels=2)),
    ("yuv411p", 8, 1025, 2, 1, "float32", "NCHW", 3, 1, dict(levels=1)),
    ("yuv410p", 8, 1023, 7, 1, "float16", "NHWC", 2, 1, dict(levels=1)),
    ("yuv410p", 8, 11, 7, 3, "float32", "NCHW", 3, 0, dict(levels=1, irreversible=True)),
    ("yuva420p", 8, 5, 5, 2, "float16", "NCHW", 4, 1, dict(levels=1)),
    ("yuv444p12le", 12, 33, 17, 2, "float32", "NHWC", 3, 1, dict(levels=2)),
    ("rgba", 8, 9, 5, 2, "float16", "NHWC", 3, 0, dict(levels=1)),
    ("gray", 8, 257, 2, 2, "bfloat16", "NHWC", 3, 0, dict(levels=1)),
    ("ya8", 8, 2, 1, 3, "float32", "NCHW", 1, 1, dict(levels=0)),
    ("rgb48le", 12, 5, 3, 1, "float32", "NCHW", 2, 0, dict(levels=1, irreversible=True, mct=0)),
]


def case_mix(fmt, bits, how, chroma, rng):
    if how == "bgr":
        return BGR, None, chroma
    if how == "rgb":
        s = m.Decoder.rgb_mix_in(709, bits, chroma=tmi.CHROMA.get(chroma, chroma))
        _, _, mat, off = tmi.unpack(s)
        return mat[:3, :3], off[:3], chroma
    return a_mix(fmt, how, chroma, rng, bits)


def check_equal(enc, dec, case):
    fmt, bits, w, h, n, dtype, layout, how, chroma, opts = case
    rng = np.random.default_rng(EQUAL.index(case))
    mix = case_mix(fmt, bits, how, chroma, rng)
    K = mix[0].shape[1]
    t, tbits = to_device(shaped(picture(n, K, h, w, rng, "NCHW", -0.05, 1.05), layout), dtype)
    opts = dict(opts)
    for key in ("target_bytes", "group_bytes"):
        if opts.get(key) == "half":
            free = enc.encode_tensor(t, fmt, bits, layout, mix=struct_of(mix), **{k: v for k, v in opts.items() if k != key})
            opts[key] = sum(len(s) for s in free) // 2 if key == "group_bytes" else max(len(s) for s in free) // 2
    return three_ways(enc, dec, t, tbits, fmt, bits, dtype, layout, mix, opts)


# ------------------------------------------------------------------ identities, the torch chain, the round trip

def plane_bytes(keep):
    return [k.cpu().numpy().tobytes() for k in keep]


def check_identities(enc, dec):
    rng = np.random.default_rng(11)
    for fmt in ("rgb24", "yuv420p", "yuv422p10le", "yuv410p", "yuva420p", "ya8", "xyz12le"):
        nc, depth = cm.LAYOUTS[fmt][0], cm.LAYOUTS[fmt][4]
        for (dtype, layout), (w, h) in zip(COMBOS, ((5, 3), (8, 4), (1, 1), (3, 5), (6, 2), (2, 2))):
            v = rng.uniform(-3.0, (1 << depth) + 3.0, size=(2, nc, h, w)).astype(np.float32)
            t, tbits = to_device(shaped(v, layout), dtype)
            _, plain = dec.from_tensor(t, fmt, depth, layout)
            _, mixed = dec.from_tensor(t, fmt, depth, layout, mix=m.tensor_mix_in(np.eye(nc)))
            assert plane_bytes(plain) == plane_bytes(mixed), ("the identity mix is not the plain call", fmt, dtype, layout, w, h)
            if fmt != "xyz12le":
                assert enc.encode_tensor(t, fmt, depth, layout, levels=0) == enc.encode_tensor(t, fmt, depth, layout, mix=m.tensor_mix_in(np.eye(nc)),
                                                                                               levels=0)
    # the box call is the co-sited call on the tensor averaged beforehand by the model
    for fmt, bits, w, h in (("yuv420p", 8, 7, 5), ("yuv422p10le", 10, 9, 2), ("yuv411p", 8, 11, 3), ("yuv410p", 8, 11, 7)):
        for dtype, layout in COMBOS[::2] + COMBOS[1::2][:1]:
            t, tbits = to_device(shaped(picture(1, 3, h, w, rng), layout), dtype)
            mat, off, _ = a_mix(fmt, 3, 1, rng, bits)
            pre = torch.from_numpy(tmi.averaged(tbits[0], fmt, (mat, off, 1), dtype, layout).view(np.float32)[None].copy()).cuda()
            torch.cuda.synchronize()
            _, box = dec.from_tensor(t, fmt, bits, layout, mix=m.tensor_mix_in(mat, off, "box"))
            _, cos = dec.from_tensor(pre, fmt, bits, layout, mix=m.tensor_mix_in(mat, off, "cosited"))
            assert plane_bytes(box)[1:] == plane_bytes(cos)[1:], (fmt, dtype, layout)


def device_planes(keep, fmt, w, h, n):
    """from_tensor's tight planes as numpy arrays, per frame"""
    geo = m.plane_geometry(m.PIX_NAMES.index(fmt), w, h)
    two = cm.LAYOUTS[fmt][5] == 2
    out, it = [], iter(keep)
    for _ in range(n):
        planes = []
        for rows, rb in geo:
            a = next(it).cpu().numpy().reshape(rows, rb)
            planes.append(a.view("<u2") if two else a)
        out.append(planes)
    return out


def check_torch_chain(dec):
    """the torch eager chain on the device, in the definition's order, bit for bit"""
    rng = np.random.default_rng(4)
    for fmt, bits, w, h in (("yuv420p", 8, 7, 5), ("yuv422p10le", 10, 9, 3), ("yuv411p", 8, 11, 3), ("yuv410p", 8, 11, 7), ("rgb24", 8, 5, 3),
                            ("yuva420p", 8, 6, 4), ("yuv444p12le", 12, 3, 2)):
        nc = cm.LAYOUTS[fmt][0]
        for j, (dtype, layout) in enumerate(COMBOS):
            K, chroma = 1 + (j + w) % 4, j % 2
            t, tbits = to_device(shaped(picture(2, K, h, w, rng), layout), dtype)
            mix = random_mix(nc, K, chroma, rng, (1 << bits) - 1)
            _, keep = dec.from_tensor(t, fmt, bits, layout, mix=struct_of(mix))
            check_against_torch(device_planes(keep, fmt, w, h, 2), torch_frames(t, fmt, bits, mix, layout), fmt, bits, (fmt, dtype, layout, K, chroma))


def check_round_trip(dec):
    """dec.to_tensor(mix=ycbcr_mix(...), float32) fed to from_tensor(mix=rgb_mix_in(...)) gives the frames back: the cases
    the host test established in the model"""
    for bits in (8, 10, 12, 16):
        for si, standard in enumerate((601, 709, 2020)):
            rng = np.random.default_rng(standard + bits)
            for fmt in ROUND_TRIP_LAYOUTS[bits]:
                planes, w, h = round_trip_planes(fmt, bits, rng)
                for full in (False, True):
                    for li, layout in enumerate(("NCHW", "NHWC")):
                        if (si + li + full) % 2:                   # half of the combinations each way
                            continue
                        t = dec.to_tensor([planes], fmt, bits, "float32", layout, mix=m.Decoder.ycbcr_mix(standard, bits, full))
                        for chroma in ("cosited", "box"):
                            _, keep = dec.from_tensor(t, fmt, bits, layout, mix=m.Decoder.rgb_mix_in(standard, bits, full, chroma=chroma))
                            back = device_planes(keep, fmt, w, h, 1)[0]
                            for c, (a, b) in enumerate(zip(back, planes)):
                                assert np.array_equal(a, b), (standard, bits, fmt, full, layout, chroma, c, int(np.count_nonzero(a != b)))


# ------------------------------------------------------------------ rounds and size limits

ROUND = 40000


def check_rounds(enc, enc_small, dec):
    """HTJ2K_ENC_ROUND = 40 000 samples: twelve images of 80 x 42 as yuv420p (5 040 samples each) go through seven to a
    round; the frames of the later rounds are read at their own place in the tensor"""
    fmt, bits, w, h, n = "yuv420p", 8, 80, 42, 12
    per = w * h * 3 // 2
    assert 7 * per <= ROUND < 8 * per
    rng = np.random.default_rng(5)
    for dtype, layout, chroma, opts in (("float16", "NCHW", 1, dict(levels=2)), ("float32", "NHWC", 0, dict(levels=2, irreversible=True, qstep=0.5))):
        t, tbits = to_device(shaped(picture(n, 3, h, w, rng), layout), dtype)
        s = m.Decoder.rgb_mix_in(601, bits, True, chroma=chroma)
        got = enc_small.encode_tensor(t, fmt, bits, layout, mix=s, **opts)
        assert enc_small.last_rounds() == 2, enc_small.last_rounds()
        assert len(set(got)) == n
        assert got == enc.encode_batch(tmi.frames(tbits, fmt, bits, s, dtype, layout), fmt, bits, **opts)
        assert got[n - 1] == enc.encode_tensor(t[n - 1:], fmt, bits, layout, mix=s, **opts)[0]


def check_tall(enc, dec, fmt, K, w, h, dtype, layout, chroma):
    """a frame of more footprint rows than grid.y takes goes in as bands: the later band reads the tensor and writes every
    component from its own row on"""
    bits = 8
    rng = np.random.default_rng(h)
    rows = (np.arange(h) % 251 / 250.0).reshape(1, 1, h, 1)
    v = np.clip(rows * np.array([1.0, 0.7, 0.4][:K]).reshape(1, K, 1, 1) + 0.1 * rng.random((1, K, h, w)), 0, 1).astype(np.float32)
    t, tbits = to_device(shaped(v, layout), dtype)
    mix = a_mix(fmt, K, chroma, rng, bits)
    opts = dict(levels=1, tile=(0, 4096))
    got = enc.encode_tensor(t, fmt, bits, layout, mix=struct_of(mix), **opts)
    model = tmi.frames(tbits, fmt, bits, mix, dtype, layout)
    assert got == enc.encode_batch(model, fmt, bits, **opts), (fmt, w, h)
    _, keep = dec.from_tensor(t, fmt, bits, layout, mix=struct_of(mix))
    for a, b in zip(device_planes(keep, fmt, w, h, 1)[0], model[0]):
        assert np.array_equal(a, b)


def check_many_frames(enc, n=66000):
    """66 000 frames of 2 x 2 as yuv420p from RGB in one call: the unpack table goes out in two chunks of grid.z; every
    stream is its image's single-image stream"""
    fmt, bits, w, h, opts = "yuv420p", 8, 2, 2, dict(levels=0)
    assert n > 65535
    rng = np.random.default_rng(9)
    s = m.Decoder.rgb_mix_in(601, bits, chroma="box")
    four, fbits = to_device(rng.random((4, 3, h, w)).astype(np.float32), "float16")
    single = [enc.encode_tensor(four[k:k + 1], fmt, bits, "NCHW", mix=s, **opts)[0] for k in range(4)]
    assert single == enc.encode_batch(tmi.frames(fbits, fmt, bits, s, "float16", "NCHW"), fmt, bits, **opts) and len(set(single)) == 4
    idx = torch.arange(n, device="cuda") & 3
    t = four[idx].contiguous()
    t[n - 1] = four[1]                                        # the last frame of the second chunk is not what the pattern says
    torch.cuda.synchronize()
    cap = n * m.Encoder.bound(w, h, fmt, bits, **opts)
    out = np.empty(cap, np.uint8)
    offs = (ctypes.c_size_t * (n + 1))()
    spec, o = m.tensor_spec("float16", "NCHW"), m._enc_opts(**opts)
    t0 = time.time()
    r = enc.L.htj2k_encode_tensor_mix(enc.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * 2), n, w, h, m.PIX_NAMES.index(fmt), bits,
                                      ctypes.byref(spec), ctypes.byref(s), ctypes.byref(o), out.ctypes.data_as(ctypes.c_void_p),
                                      ctypes.c_size_t(cap), 0, offs)
    print("%d images of 2 x 2 in one call: %.1f s" % (n, time.time() - t0))
    assert r == 0
    which = [k & 3 for k in range(n - 1)] + [1]
    offs = np.array(offs[:], np.int64)
    assert np.array_equal(offs, np.cumsum([0] + [len(single[i]) for i in which]))
    data = out.tobytes()
    for k in range(n):
        assert data[offs[k]:offs[k + 1]] == single[which[k]], k


# ------------------------------------------------------------------ refusals

def check_refusals(enc, dec):
    """refused calls on live contexts write nothing: `out`, the destination frames and the info calls are as they were"""
    fmt, bits, w, h = "yuv420p", 8, 20, 10
    t, tbits = to_device(picture(2, 3, h, w, np.random.default_rng(1)), "float16")
    ok_mix = m.Decoder.rgb_mix_in(709, bits, chroma="box")
    good = enc.encode_tensor(t, fmt, bits, "NCHW", mix=ok_mix, levels=2, target_bytes=400)

    def said():
        return repr((enc.stage_ms(), enc.rc_info(0), enc.rc_info(1), enc.last_planes(1), enc.last_passes(0), enc.last_rounds(),
                     enc.quality_info(0), enc.group_info()))

    before = said()
    out = np.full(1 << 16, GUARD, np.uint8)
    offs = (ctypes.c_size_t * 3)(7, 7, 7)
    o = m._enc_opts(levels=2)
    ok = m.tensor_spec("float16", "NCHW")
    nbytes = t.numel() * 2

    def changed_mix(**kw):
        x = m.Decoder.rgb_mix_in(709, bits, chroma="box")
        for k, v in kw.items():
            if k == "m":
                x.m[v[0]][v[1]] = v[2]
            elif k == "b":
                x.b[v[0]] = v[1]
            else:
                setattr(x, k, v)
        return x

    def spec_with(**kw):
        s = m.tensor_spec("float16", "NCHW")
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def enc_call(spec=ok, mix=ok_mix, src=t.data_ptr(), src_bytes=nbytes, n=2, width=w, height=h, pix=fmt, depth=bits, dst=out.ctypes.data,
                 offsets=offs):
        return enc.L.htj2k_encode_tensor_mix(enc.h, ctypes.c_void_p(src), ctypes.c_size_t(src_bytes), n, width, height, m.PIX_NAMES.index(pix),
                                             depth, None if spec is None else ctypes.byref(spec), ctypes.byref(mix), ctypes.byref(o),
                                             ctypes.c_void_p(dst), ctypes.c_size_t(out.size), 0, offsets)

    four = changed_mix(nin=4)                                 # a valid mix of four channels: the tensor has three
    refused = [(dict(src=0), EINVAL), (dict(spec=None), EINVAL), (dict(dst=0), EINVAL), (dict(offsets=None), EINVAL), (dict(n=0), EINVAL),
               (dict(width=0), EINVAL), (dict(pix="pal8"), PATCHWELCOME), (dict(depth=9), EINVAL), (dict(spec=spec_with(dtype=3)), EINVAL),
               (dict(mix=changed_mix(nin=0)), EINVAL), (dict(mix=changed_mix(nin=5)), EINVAL), (dict(mix=changed_mix(chroma=2)), EINVAL),
               (dict(mix=changed_mix(m=(1, 2, float("nan")))), EINVAL), (dict(mix=changed_mix(b=(0, float("inf")))), EINVAL),
               (dict(spec=spec_with(out_w=w, out_h=h)), EINVAL), (dict(mix=four), EINVAL), (dict(src_bytes=nbytes - 1), EINVAL),
               (dict(src=t.data_ptr() + 1), EINVAL)]
    for kw, code in refused:
        assert enc_call(**kw) == code, kw
        assert (out == GUARD).all() and list(offs) == [7, 7, 7], kw
        assert before == said(), kw
    assert enc_call(mix=changed_mix(m=(3, 3, float("nan")))) == 0            # an entry that is not read
    assert enc.encode_tensor(t, fmt, bits, "NCHW", mix=ok_mix, levels=2, target_bytes=400) == good

    # htj2k_tensor_to_frames_mix: the destination frames stay 0xC3, the context's last time stays
    dst = Guarded(fmt, w, h, 2, 1, 1)

    def frames_call(spec=ok, mix=ok_mix, src=t.data_ptr(), src_bytes=nbytes, n=2, depth=bits, frames=dst.arr):
        return dec.L.htj2k_tensor_to_frames_mix(dec.h, ctypes.c_void_p(src), ctypes.c_size_t(src_bytes), n, depth,
                                                None if spec is None else ctypes.byref(spec), ctypes.byref(mix), frames)

    def changed(**kw):
        a = (m.Frame * 2)(*[m.Frame.from_buffer_copy(fr) for fr in dst.arr])
        for k, v in kw.items():
            if k == "plane":
                a[1].data[v] = None
            elif k == "linesize":
                a[1].linesize[v[0]] = v[1]
            else:
                setattr(a[1], k, v)
        return a

    dec.framecrc([dst.arr[0]], fmt, on_device=True)
    ms = dec.compare_ms()
    for kw, code in [(dict(src=0), EINVAL), (dict(spec=None), EINVAL), (dict(frames=None), EINVAL), (dict(n=0), EINVAL), (dict(depth=9), EINVAL),
                     (dict(spec=spec_with(layout=2)), EINVAL), (dict(mix=changed_mix(nin=-1)), EINVAL), (dict(mix=changed_mix(chroma=-1)), EINVAL),
                     (dict(mix=changed_mix(m=(2, 0, float("-inf")))), EINVAL), (dict(spec=spec_with(out_w=1, out_h=1)), EINVAL),
                     (dict(frames=changed(width=w + 1)), EINVAL), (dict(frames=changed(plane=2)), EINVAL),
                     (dict(frames=changed(linesize=(1, w // 2 - 1))), EINVAL), (dict(mix=four), EINVAL), (dict(src_bytes=nbytes - 1), EINVAL),
                     (dict(src=t.data_ptr() + 1), EINVAL)]:
        assert frames_call(**kw) == code, kw
        assert dec.compare_ms() == ms, kw
        assert dst.untouched(), kw
    assert frames_call() == 0 and dec.compare_ms() > 0 and not dst.untouched()

    # the Python entry points: a tensor whose channels are not the mix's, and something that is no mix
    with pytest.raises(ValueError):
        enc.encode_tensor(t, fmt, bits, mix=m.tensor_mix_in(np.ones((3, 4))))
    with pytest.raises(ValueError):
        dec.from_tensor(t, fmt, bits, mix=m.tensor_mix_in(np.ones((3, 2))))
    with pytest.raises(ValueError):
        dec.from_tensor(t, fmt, bits, mix=m.Decoder.ycbcr_mix(709, 8))
    with pytest.raises(ValueError):
        enc.encode_tensor(t.cpu(), fmt, bits, mix=ok_mix)


# ------------------------------------------------------------------ pytest

@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def enc():
    e = m.Encoder(0)
    yield e
    e.close()


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


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_from_tensor_mix_is_the_model(dec, fmt):
    check_layout(dec, fmt)


@pytest.mark.gpu
def test_values_at_the_corners(enc, dec):
    check_values(enc, dec)


@pytest.mark.gpu
@pytest.mark.parametrize("case", EQUAL, ids=lambda c: "%s-%d-%dx%dx%d-%s-%s-%s-%s-%s" % (c[:9] + ("_".join(sorted(c[9])),)))
def test_encode_tensor_mix_is_the_encode_of_its_frames(enc, dec, case):
    check_equal(enc, dec, case)


@pytest.mark.gpu
def test_identity_mix_and_pre_averaged_tensor(enc, dec):
    check_identities(enc, dec)


@pytest.mark.gpu
def test_torch_chain_on_the_device(dec):
    check_torch_chain(dec)


@pytest.mark.gpu
def test_round_trip_on_the_device(dec):
    check_round_trip(dec)


@pytest.mark.gpu
def test_calls_of_several_rounds(enc, enc_small_rounds, dec):
    check_rounds(enc, enc_small_rounds, dec)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,K,w,h,dtype,layout,chroma", [("yuv420p", 3, 2, 131080, "float32", "NHWC", 1), ("yuv420p", 3, 2, 131080, "bfloat16", "NCHW", 0),
                                                           ("gray", 3, 4, 65540, "float16", "NCHW", 0)])
def test_a_frame_of_more_footprint_rows_than_one_launch_covers(enc, dec, fmt, K, w, h, dtype, layout, chroma):
    check_tall(enc, dec, fmt, K, w, h, dtype, layout, chroma)


@pytest.mark.gpu
def test_more_frames_than_one_launch_takes(enc):
    check_many_frames(enc)


@pytest.mark.gpu
def test_refusals_on_live_contexts(enc, dec):
    check_refusals(enc, dec)


def run_equalities(enc, dec):
    """what the poisoned pass runs: every byte against the model on a spread of layouts, and every equality case"""
    for fmt in ("rgb24", "yuv420p", "yuv422p10le", "yuv410p"):
        check_layout(dec, fmt)
    check_values(enc, dec)
    for case in EQUAL:
        check_equal(enc, dec, case)
    check_identities(enc, dec)
    check_tall(enc, dec, "yuv420p", 3, 2, 131080, "float32", "NHWC", 1)


POISON_TIMEOUT = 300


@pytest.mark.gpu
def test_equalities_on_poisoned_buffers():
    """HTJ2K_POISON=1 (read once per process, so a fresh child): every new device buffer of the library starts as 0xA5
    bytes, and the model and equality checks must still hold.  The child's exit status comes first."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True,
                       timeout=POISON_TIMEOUT, env=dict(os.environ, HTJ2K_POISON="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "poisoned buffers: ok" in r.stdout, r.stdout[-3000:]


if __name__ == "__main__":
    t0 = time.time()
    _dec, _enc = m.Decoder(device_id=0), m.Encoder(0)
    run_equalities(_enc, _dec)
    _enc.close()
    _dec.close()
    print("%s buffers: ok (%.1f s)" % ("poisoned" if os.environ.get("HTJ2K_POISON") == "1" else "plain", time.time() - t0))
