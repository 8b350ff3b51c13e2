"""Tensors as frames on the GPU: htj2k_tensor_to_frames against the numpy model (tensor_in_model), every byte of every
plane buffer, and htj2k_encode_tensor against the encoder's own streams of those frames, byte for byte.

Thirteen layouts, three element types and two tensor layouts; widths on both sides of the 256-thread seam, heights 1 to
3, linesizes and plane bases off the 16-byte alignment with 0xAB dirt that must survive, depths below the layout's own,
values at the corners of the number formats.  encode_tensor must equal encode_device(from_tensor(t)) and
encode_batch(model frames) over 5/3 and 9/7, the component transform on and off, budgets, a PSNR target, a group
budget, refinement passes and tiles; in calls of several rounds, on frames taller than one launch covers, and in a call
of more frames than grid.z takes.  Run as a program, the module runs the model and equality checks on its own contexts:
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
import hash_model as hm
import tensor_in_model as tim
import tensor_model as tm
from test_hash_gpu import HFrame

LAYOUTS = ["gray", "ya8", "rgb24", "rgba", "rgb48le", "gray16le", "yuv420p", "yuv422p10le", "yuv444p12le", "yuv411p", "yuv410p",
           "yuva420p", "xyz12le"]
WIDTHS = [1, 2, 3, 255, 256, 257]                        # the 256-thread seam of both kernels' rows
HEIGHTS = [1, 2, 3]
LS_MODES = ["row", "row+1", "row+13", "to64"]
OFFSETS = [0, 1, 2, 15]
COMBOS = [(d, l) for d in tm.DTYPES for l in ("NCHW", "NHWC")]
TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
EINVAL, PATCHWELCOME = -22, -0x45574150
OUT_POISON = 0xC3


def low_bits(fmt):
    """a depth below the layout's own: the sample is then shifted among bits that must stay zero"""
    return {"rgb48le": 12, "yuv422p10le": 9}.get(fmt, cm.LAYOUTS[fmt][4] - 1)


def to_device(values, dtype):
    """float32 values -> (the CUDA tensor of `dtype`, its bit patterns as the model takes them)"""
    t = torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(TORCH[dtype]).contiguous()
    bits = t.view(torch.int32 if dtype == "float32" else torch.int16).numpy().view(tm.BITS_DTYPE[dtype])
    d = t.cuda()
    torch.cuda.synchronize()
    return d, bits


def picture(n, nc, h, w, rng, layout="NCHW", lo=-0.1, hi=1.1):
    """n images in [lo, hi): a ramp across each, a tilt per channel and image, and noise; as (n, C, H, W) or (n, H, W, C)"""
    y, x = np.mgrid[0:h, 0:w]
    base = (x / max(w - 1, 1) + y / max(h - 1, 1)) / 2
    v = np.stack([np.stack([np.clip(base * (0.6 + 0.1 * c) + 0.05 * i, 0, 1) for c in range(nc)]) for i in range(n)])
    v = lo + (hi - lo) * (0.85 * v + 0.15 * rng.random(v.shape))
    return np.ascontiguousarray(v if layout == "NCHW" else v.transpose(0, 2, 3, 1), np.float32)


# ------------------------------------------------------------------ htj2k_tensor_to_frames against the model

def to_frames(dec, t, tbits, fmt, bits, dtype, layout, w, h, scale, bias, ls_mode="row", off=0):
    """the C call into dirty destination frames with a linesize and a base offset of their own; every byte of every plane
    buffer against the model's frames in 0xAB dirt"""
    n = t.shape[0]
    rng = np.random.default_rng(0)
    dst = [HFrame(fmt, w, h, rng, ls_mode, off, value=0xAB) for _ in range(n)]
    made = [f.on_device() for f in dst]
    arr = (m.Frame * n)(*[fr for fr, _ in made])
    spec = m.tensor_spec(dtype, layout, None, scale, bias)
    r = dec.L.htj2k_tensor_to_frames(dec.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * t.element_size()), n, int(bits),
                                     ctypes.byref(spec), arr)
    what = (fmt, bits, dtype, layout, w, h, n, scale, bias, ls_mode, off)
    assert r == 0, (r, what)
    want = tim.frames(tbits, fmt, bits, dtype, layout, scale, bias)
    for i, f in enumerate(dst):
        for p, (rows, rb) in enumerate(f.geo):
            exp = f.bufs[p].copy()
            rows_bytes = np.ascontiguousarray(want[i][p]).view(np.uint8).reshape(rows, rb)
            for y in range(rows):
                exp[f.off + y * f.ls[p]: f.off + y * f.ls[p] + rb] = rows_bytes[y]
            got = made[i][1][p].cpu().numpy()
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (what, i, p, len(bad), bad[:6].tolist(), got[bad[:6]].tolist(), exp[bad[:6]].tolist())
    return want


def check_layout(dec, fmt):
    """every width at the seam with every element type and tensor layout; heights, linesizes, offsets, depths, batch sizes
    and the scale / bias per component change from call to call"""
    nc, depth = cm.LAYOUTS[fmt][0], cm.LAYOUTS[fmt][4]
    rng = np.random.default_rng(LAYOUTS.index(fmt))
    k = LAYOUTS.index(fmt)
    for wi, w in enumerate(WIDTHS):
        for ci, (dtype, layout) in enumerate(COMBOS):
            k += 1
            h, n = HEIGHTS[k % 3], 1 + k % 2
            bits = depth if k % 3 else low_bits(fmt)
            peak = (1 << bits) - 1
            t, tbits = to_device(picture(n, nc, h, w, rng, layout), dtype)
            scale = [peak * s for s in (1.0, 0.5, 1.25, 1.0)][:nc]
            bias = [0.0, 0.25, -3.0, 0.5][:nc]
            to_frames(dec, t, tbits, fmt, bits, dtype, layout, w, h, scale, bias, LS_MODES[k % 4], OFFSETS[(k // 4) % 4])


def special_values(bits):
    peak = (1 << bits) - 1
    ties = [j + 0.5 for j in range(0, min(peak, 9))]
    return [np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, -0.5, 1e-45, -1e-45, 1e-40, 6e-8, 6.1e-5, 1e-38, 9.2e-41, 3e38, -3e38,
            peak - 0.5, peak - 0.499, peak + 0.5, peak, peak + 1, peak - 1, 65504.0, 65536.0] + ties


def check_values(dec):
    """NaN, infinities, -0, subnormals of every element type, ties at k + 0.5 and the values around the peak, with a scale
    of 1 and a bias of 0, and through a scale and a bias that lands them on ties"""
    for fmt, bits in (("gray", 8), ("gray", 1), ("gray16le", 16), ("gray16le", 10), ("yuv422p10le", 10), ("rgb24", 8), ("xyz12le", 12)):
        nc = cm.LAYOUTS[fmt][0]
        vals = np.array(special_values(bits), np.float32)
        w, h = 2 * ((len(vals) + 1) // 2), 2
        img = np.resize(vals, (1, nc, h, w))
        for ci, (dtype, layout) in enumerate(COMBOS):
            v = img if layout == "NCHW" else np.ascontiguousarray(img.transpose(0, 2, 3, 1))
            t, tbits = to_device(v, dtype)
            want = to_frames(dec, t, tbits, fmt, bits, dtype, layout, w, h, None, None, LS_MODES[ci % 4], OFFSETS[ci % 4])
            if fmt == "gray" and bits == 8:                          # what the model says of them, spelled out once
                assert want[0][0][0, :8].tolist() == [0, 0, 255, 0, 0, 0, 0, 0]
            to_frames(dec, t, tbits, fmt, bits, dtype, layout, w, h, 0.5, 0.25, "row+1", 1)
            to_frames(dec, t, tbits, fmt, bits, dtype, layout, w, h, [-1.0, 2.0, 3.0][:nc], [float(1 << bits), -0.0, 0.5][:nc], "row", 0)
    # subnormal elements scaled up to samples: they are values, not zeros
    for dtype, pats, scale in (("float16", [0x0001, 0x03FF, 0x8001, 0x0200], 2.0 ** 24), ("bfloat16", [0x0001, 0x007F, 0x0040, 0x8040], 2.0 ** 127),
                               ("float32", [0x00000001, 0x007FFFFF, 0x00400000, 0x80400000], 2.0 ** 127)):
        tbits = np.array(pats, tm.BITS_DTYPE[dtype]).reshape(1, 1, 2, 2)
        t = torch.from_numpy(tbits.view(np.int16 if tbits.itemsize == 2 else np.int32)).view(TORCH[dtype]).cuda()
        torch.cuda.synchronize()
        want = to_frames(dec, t, tbits, "gray16le", 16, dtype, "NCHW", 2, 2, scale, 0.0)
        assert int(want[0][0].max()) > 0


# ------------------------------------------------------------------ htj2k_encode_tensor against the encoder's own streams

def three_ways(enc, dec, t, tbits, fmt, bits, dtype, layout, scale, bias, opts, infos=True):
    """encode_tensor, encode_device(from_tensor) and encode_batch(model frames): equal streams, and the info calls say of
    the tensor call what they say of the batch call"""
    n = t.shape[0]
    got = enc.encode_tensor(t, fmt, bits, layout, scale, bias, **opts)
    ms = enc.stage_ms()
    said = [(enc.rc_info(k), enc.last_planes(k), enc.last_passes(k)) for k in range(n)] if infos else None
    rounds = enc.last_rounds()
    frames, keep = dec.from_tensor(t, fmt, bits, layout, scale, bias)
    via = enc.encode_device(list(frames), fmt, bits, **opts)
    model = tim.frames(tbits, fmt, bits, dtype, layout, scale, bias)
    ref = enc.encode_batch(model, fmt, bits, **opts)
    what = (fmt, bits, dtype, layout, tuple(t.shape), opts)
    assert len(got) == n and all(len(s) > 0 for s in got), what
    assert ref == via, ("from_tensor's frames encode differently from the model's", what)
    assert got == ref, ("encode_tensor differs from the encode of its frames", what, [k for k in range(n) if got[k] != ref[k]])
    assert ms[0] > 0, ms
    if infos:
        assert said == [(enc.rc_info(k), enc.last_planes(k), enc.last_passes(k)) for k in range(n)], what
        assert rounds == enc.last_rounds()
    del keep
    return got


# (layout, bits, w, h, n, element, tensor layout, options); "half": a budget of half the free stream is filled in
EQUAL = [
    ("rgb24", 8, 257, 3, 1, "float16", "NCHW", dict(levels=1)),
    ("rgb24", 8, 255, 5, 5, "float32", "NHWC", dict(levels=2, irreversible=True, qstep=0.5)),
    ("rgb24", 8, 256, 4, 1, "bfloat16", "NHWC", dict(levels=2, mct=0)),
    ("rgb48le", 12, 33, 17, 5, "float32", "NCHW", dict(levels=2, irreversible=True, mct=0, qstep=0.25)),
    ("rgb48le", 16, 64, 48, 1, "float32", "NHWC", dict(levels=3, mct=1, target_bytes="half")),
    ("rgba", 8, 40, 24, 5, "float16", "NHWC", dict(levels=2, tile=(16, 16))),
    ("rgb24", 8, 64, 48, 5, "float16", "NCHW", dict(levels=3, irreversible=True, qstep=0.25, target_psnr=34.0)),
    ("rgb24", 8, 64, 48, 5, "bfloat16", "NCHW", dict(levels=3, group_bytes="half")),
    ("rgb24", 8, 64, 48, 1, "float32", "NCHW", dict(levels=3, ht_passes=3)),
    ("yuv420p", 8, 9, 5, 5, "float16", "NHWC", dict(levels=1)),
    ("yuv420p", 8, 65, 47, 1, "float32", "NCHW", dict(levels=3, irreversible=True, qstep=0.5, target_bytes="half", ht_passes=3)),
    ("yuv422p10le", 10, 5, 3, 1, "float32", "NCHW", dict(levels=1, irreversible=True)),
    ("yuv422p10le", 9, 257, 2, 5, "float16", "NCHW", dict(levels=1)),
    ("yuv411p", 8, 9, 5, 1, "bfloat16", "NHWC", dict(levels=1)),
    ("yuv410p", 8, 5, 3, 5, "float32", "NHWC", dict(levels=1)),
    ("yuv410p", 8, 9, 5, 1, "float16", "NCHW", dict(levels=1, irreversible=True)),
    ("yuva420p", 8, 3, 3, 5, "float16", "NCHW", dict(levels=1)),
    ("gray16le", 16, 1, 1, 1, "float32", "NCHW", dict(levels=0)),
    ("ya8", 7, 2, 1, 5, "bfloat16", "NHWC", dict(levels=0)),
]


def check_equal(enc, dec, case):
    fmt, bits, w, h, n, dtype, layout, opts = case
    nc = cm.LAYOUTS[fmt][0]
    peak = (1 << bits) - 1
    rng = np.random.default_rng(EQUAL.index(case))
    t, tbits = to_device(picture(n, nc, h, w, rng, layout, -0.05, 1.05), dtype)
    scale, bias = [float(peak)] * nc, [0.0, 0.25, -0.25, 0.0][:nc]
    opts = dict(opts)
    for key in ("target_bytes", "group_bytes"):
        if opts.get(key) == "half":
            free = enc.encode_tensor(t, fmt, bits, layout, scale, bias, **{k: v for k, v in opts.items() if k != key})
            opts[key] = sum(len(s) for s in free) // 2 if key == "group_bytes" else max(len(s) for s in free) // 2
    return three_ways(enc, dec, t, tbits, fmt, bits, dtype, layout, scale, bias, opts)


def check_round_trip(enc, dec):
    """Decoder.to_tensor's output fed straight back (scale 1, bias 0) encodes as the frames it came from do"""
    for fmt, bits, w, h, dtype, layout in (("yuv420p", 8, 9, 5, "float16", "NCHW"), ("yuv422p10le", 10, 33, 3, "float32", "NHWC"),
                                           ("rgb24", 8, 257, 2, "bfloat16", "NHWC"), ("yuv410p", 8, 5, 3, "float32", "NCHW"),
                                           ("rgb48le", 11, 17, 9, "float16", "NCHW")):
        rng = np.random.default_rng(w)
        nbytes = cm.LAYOUTS[fmt][5]
        frames = [[(rng.integers(0, 1 << bits, size=s, dtype=np.int64) << cm.shift(fmt, bits)).astype(np.uint8 if nbytes == 1 else np.uint16)
                   for s in cm.plane_shapes(fmt, w, h)] for _ in range(3)]
        t = dec.to_tensor(frames, fmt, bits, dtype, layout)
        for opts in (dict(levels=1), dict(levels=1, irreversible=True, qstep=0.5)):
            assert enc.encode_tensor(t, fmt, bits, layout, **opts) == enc.encode_batch(frames, fmt, bits, **opts), (fmt, dtype, layout, opts)


ROUND = 40000


def check_rounds(enc, enc_small, dec):
    """HTJ2K_ENC_ROUND = 40 000 samples: sixteen distinct images of 75 x 41 x 3 samples go through four to a round; the
    frames of the later rounds are read at their own place in the tensor, so every stream is its image's single-image stream"""
    fmt, bits, w, h, n = "rgb24", 8, 75, 41, 16
    assert 4 * 3 * w * h <= ROUND < 5 * 3 * w * h
    rng = np.random.default_rng(5)
    for dtype, layout, opts in (("float16", "NCHW", dict(levels=2)), ("float32", "NHWC", dict(levels=2, irreversible=True, qstep=0.5))):
        t, tbits = to_device(picture(n, 3, h, w, rng, layout), dtype)
        got = enc_small.encode_tensor(t, fmt, bits, layout, 255.0, **opts)
        assert enc_small.last_rounds() == 4, enc_small.last_rounds()
        assert len(set(got)) == n
        for k in range(n):
            assert got[k] == enc.encode_tensor(t[k:k + 1], fmt, bits, layout, 255.0, **opts)[0], (dtype, layout, k)
        assert got == enc.encode_batch(tim.frames(tbits, fmt, bits, dtype, layout, 255.0), fmt, bits, **opts)


def check_tall(enc, fmt, w, h, dtype, layout):
    """a frame of more rows than grid.y takes goes in as bands: the later band reads the tensor from its own row on
    (4:2:0 at twice that height: the chroma band's row y is the tensor's row 2 y)"""
    nc, bits = cm.LAYOUTS[fmt][0], 8
    rng = np.random.default_rng(h)
    rows = (np.arange(h) % 251 / 250.0).reshape(1, 1, h, 1)
    v = np.clip(rows * np.array([1.0, 0.7, 0.4][:nc]).reshape(1, nc, 1, 1) + 0.1 * rng.random((1, nc, h, w)), 0, 1).astype(np.float32)
    v = v if layout == "NCHW" else np.ascontiguousarray(v.transpose(0, 2, 3, 1))
    t, tbits = to_device(v, dtype)
    opts = dict(levels=1, tile=(0, 4096))
    got = enc.encode_tensor(t, fmt, bits, layout, 255.0, **opts)
    assert got == enc.encode_batch(tim.frames(tbits, fmt, bits, dtype, layout, 255.0), fmt, bits, **opts), (fmt, w, h)


def check_many_frames(enc, n=66000):
    """66 000 gray frames of 9 x 7 in one call: the unpack table goes out in two chunks of grid.z; every stream is its
    image's single-image stream"""
    fmt, bits, w, h, opts = "gray", 8, 9, 7, dict(levels=2)
    assert n > 65535
    rng = np.random.default_rng(9)
    four, fbits = to_device(picture(4, 1, h, w, rng), "float16")
    single = [enc.encode_tensor(four[k:k + 1], fmt, bits, "NCHW", 255.0, **opts)[0] for k in range(4)]
    assert single == enc.encode_batch(tim.frames(fbits, fmt, bits, "float16", "NCHW", 255.0), fmt, bits, **opts) and len(set(single)) == 4
    idx = torch.arange(n, device="cuda") & 3
    t = four[idx].contiguous()
    t[n - 1] = four[1]                                        # the last frame of the second chunk is not what the pattern says
    torch.cuda.synchronize()
    cap = n * m.Encoder.bound(w, h, fmt, bits, **opts)
    out = np.empty(cap, np.uint8)
    offs = (ctypes.c_size_t * (n + 1))()
    spec, o = m.tensor_spec("float16", "NCHW", None, 255.0), m._enc_opts(**opts)
    t0 = time.time()
    r = enc.L.htj2k_encode_tensor(enc.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * 2), n, w, h, m.PIX_NAMES.index(fmt), bits,
                                  ctypes.byref(spec), ctypes.byref(o), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap), 0, offs)
    print("%d images of 9 x 7 in one call: %.1f s" % (n, time.time() - t0))
    assert r == 0
    which = [k & 3 for k in range(n - 1)] + [1]
    offs = np.array(offs[:], np.int64)
    assert np.array_equal(offs, np.cumsum([0] + [len(single[i]) for i in which]))
    data = out.tobytes()
    for k in range(n):
        assert data[offs[k]:offs[k + 1]] == single[which[k]], k


def check_from_tensor_frames(enc, dec):
    """the frames of from_tensor are frames like any other on the device: checksums against the zlib model, and the
    measured encode takes them as its input"""
    for fmt, bits, w, h, dtype, layout in (("yuv420p", 8, 33, 17, "float16", "NHWC"), ("rgb48le", 12, 40, 24, "float32", "NCHW")):
        nc, peak = cm.LAYOUTS[fmt][0], (1 << bits) - 1
        t, tbits = to_device(picture(2, nc, h, w, np.random.default_rng(3), layout), dtype)
        frames, keep = dec.from_tensor(t, fmt, bits, layout, float(peak))
        model = tim.frames(tbits, fmt, bits, dtype, layout, float(peak))
        assert dec.framecrc(frames, fmt, on_device=True) == [hm.frame_hash(p) for p in model]
        streams, info = enc.encode_measured(dec, frames, fmt, bits, in_on_device=True, levels=2)
        assert streams == enc.encode_tensor(t, fmt, bits, layout, float(peak), levels=2)
        assert all(i["diff"]["sse"] == [0] * 4 and i["diff"]["nsamples"][0] == w * h for i in info)       # 5/3 without a budget: lossless
        lossy, info = enc.encode_measured(dec, frames, fmt, bits, in_on_device=True, levels=2, irreversible=True, qstep=2.0)
        assert lossy == enc.encode_tensor(t, fmt, bits, layout, float(peak), levels=2, irreversible=True, qstep=2.0)
        assert dec.compare(frames, model, fmt, bits, on_device=(True, False))[0]["ndiff"] == [0] * 4


def check_refusals(enc, dec):
    """refused calls on live contexts write nothing: `out`, the destination frames and the info calls are as they were"""
    fmt, bits, w, h = "yuv420p", 8, 20, 10
    t, tbits = to_device(picture(2, 3, h, w, np.random.default_rng(1)), "float16")
    good = enc.encode_tensor(t, fmt, bits, "NCHW", 255.0, levels=2, target_bytes=400)
    def said():
        return repr((enc.stage_ms(), enc.rc_info(0), enc.rc_info(1), enc.last_planes(1), enc.last_passes(0), enc.last_rounds(),
                     enc.quality_info(0), enc.group_info()))

    before = said()
    out = np.full(1 << 16, OUT_POISON, np.uint8)
    offs = (ctypes.c_size_t * 3)(7, 7, 7)
    o = m._enc_opts(levels=2)
    ok = m.tensor_spec("float16", "NCHW", None, 255.0)
    nbytes = t.numel() * 2

    def enc_call(spec=ok, src=t.data_ptr(), src_bytes=nbytes, n=2, width=w, height=h, pix=fmt, depth=bits, dst=out.ctypes.data, offsets=offs):
        return enc.L.htj2k_encode_tensor(enc.h, ctypes.c_void_p(src), ctypes.c_size_t(src_bytes), n, width, height, m.PIX_NAMES.index(pix), depth,
                                         None if spec is None else ctypes.byref(spec), ctypes.byref(o), ctypes.c_void_p(dst),
                                         ctypes.c_size_t(out.size), 0, offsets)

    def spec_with(**kw):
        s = m.tensor_spec("float16", "NCHW", None, 255.0)
        for k, v in kw.items():
            if k in ("scale", "bias"):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return s

    refused = [(dict(src=0), EINVAL), (dict(spec=None), EINVAL), (dict(dst=0), EINVAL), (dict(offsets=None), EINVAL), (dict(n=0), EINVAL),
               (dict(width=0), EINVAL), (dict(height=-1), EINVAL), (dict(pix="pal8"), PATCHWELCOME), (dict(depth=9), EINVAL),
               (dict(spec=spec_with(dtype=3)), EINVAL), (dict(spec=spec_with(layout=2)), EINVAL),
               (dict(spec=spec_with(scale=(1, float("nan")))), EINVAL), (dict(spec=spec_with(bias=(2, float("inf")))), EINVAL),
               (dict(spec=spec_with(out_w=w, out_h=h)), EINVAL), (dict(src_bytes=nbytes - 1), EINVAL), (dict(src=t.data_ptr() + 1), EINVAL)]
    for kw, code in refused:
        assert enc_call(**kw) == code, kw
        assert (out == OUT_POISON).all() and list(offs) == [7, 7, 7], kw
        assert before == said(), kw
    # what the encoder refuses for such frames comes with its code, and writes no stream either
    assert enc.L.htj2k_encode_tensor(enc.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(nbytes), 2, 10, 10, m.PIX_NAMES.index("xyz12le"), 12,
                                     ctypes.byref(ok), ctypes.byref(o), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), 0,
                                     offs) == PATCHWELCOME
    o_bad = m._enc_opts(levels=2, target_bytes=10)            # below the smallest stream
    assert enc.L.htj2k_encode_tensor(enc.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(nbytes), 2, w, h, m.PIX_NAMES.index(fmt), bits,
                                     ctypes.byref(ok), ctypes.byref(o_bad), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), 0,
                                     offs) == EINVAL
    assert (out == OUT_POISON).all()
    with pytest.raises(m.Htj2kError):
        enc.encode_tensor(t, fmt, bits, "NCHW", 255.0, levels=2, target_bytes=10)
    assert "budget" in "".join(enc._logs)
    assert enc.encode_tensor(t, fmt, bits, "NCHW", 255.0, levels=2, target_bytes=400) == good

    # htj2k_tensor_to_frames: the destination frames stay 0xAB
    rng = np.random.default_rng(0)
    dst = [HFrame(fmt, w, h, rng, "row+1", 1, value=0xAB) for _ in range(2)]
    made = [f.on_device() for f in dst]
    arr = (m.Frame * 2)(*[fr for fr, _ in made])
    plain = m.tensor_spec("float16", "NCHW", None, 255.0)

    def frames_call(spec=plain, src=t.data_ptr(), src_bytes=nbytes, n=2, depth=bits, frames=arr):
        return dec.L.htj2k_tensor_to_frames(dec.h, ctypes.c_void_p(src), ctypes.c_size_t(src_bytes), n, depth,
                                            None if spec is None else ctypes.byref(spec), frames)

    def changed(**kw):
        a = (m.Frame * 2)(*[m.Frame.from_buffer_copy(fr) for fr, _ in made])
        for k, v in kw.items():
            if k == "plane":
                a[1].data[v] = None
            elif k == "linesize":
                a[1].linesize[v[0]] = v[1]
            else:
                setattr(a[1], k, v)
        return a

    dec.framecrc([made[0][0]], fmt, on_device=True)
    ms = dec.compare_ms()
    for kw, code in [(dict(src=0), EINVAL), (dict(spec=None), EINVAL), (dict(frames=None), EINVAL), (dict(n=0), EINVAL),
                     (dict(frames=changed(pix_fmt=0)), EINVAL), (dict(depth=0), EINVAL), (dict(depth=9), EINVAL),
                     (dict(spec=spec_with(dtype=-1)), EINVAL), (dict(spec=spec_with(scale=(0, float("-inf")))), EINVAL),
                     (dict(spec=spec_with(out_w=1, out_h=1)), EINVAL), (dict(frames=changed(width=w + 1)), EINVAL),
                     (dict(frames=changed(plane=2)), EINVAL), (dict(frames=changed(linesize=(1, w // 2 - 1))), EINVAL),
                     (dict(src_bytes=nbytes - 1), EINVAL), (dict(src=t.data_ptr() + 1), EINVAL)]:
        assert frames_call(**kw) == code, kw
        assert dec.compare_ms() == ms, kw
        for _, ts in made:
            assert all(bool((x == 0xAB).all()) for x in ts), kw
    pal = changed()
    pal[0].pix_fmt = pal[1].pix_fmt = 0
    assert frames_call(frames=pal) == PATCHWELCOME
    assert frames_call() == 0 and dec.compare_ms() > 0

    # the Python entry points refuse what is not a contiguous CUDA tensor of the right shape and type
    for bad in (t.cpu(), t.double(), t[:, :, :, ::2], t[0], t[:, :2], np.zeros((2, 3, h, w), np.float32)):
        with pytest.raises(ValueError):
            enc.encode_tensor(bad, fmt, bits)
        with pytest.raises(ValueError):
            dec.from_tensor(bad, fmt, bits)
    with pytest.raises(ValueError):
        enc.encode_tensor(t, fmt, bits, "NHWC")               # (2, 3, 10, 20) read as NHWC has 20 channels
    with pytest.raises(ValueError):
        enc.encode_tensor(t, fmt, bits, "CHWN")


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
def test_tensor_to_frames_is_the_model(dec, fmt):
    check_layout(dec, fmt)


@pytest.mark.gpu
def test_values_at_the_corners_of_the_formats(dec):
    check_values(dec)


@pytest.mark.gpu
@pytest.mark.parametrize("case", EQUAL, ids=lambda c: "%s-%d-%dx%dx%d-%s-%s-%s" % (c[:7] + ("_".join(sorted(c[7])),)))
def test_encode_tensor_is_the_encode_of_its_frames(enc, dec, case):
    check_equal(enc, dec, case)


@pytest.mark.gpu
def test_to_tensor_output_fed_straight_back(enc, dec):
    check_round_trip(enc, dec)


@pytest.mark.gpu
def test_calls_of_several_rounds(enc, enc_small_rounds, dec):
    check_rounds(enc, enc_small_rounds, dec)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,w,h,dtype,layout", [("gray", 4, 65540, "float16", "NCHW"), ("yuv420p", 2, 131080, "float32", "NHWC"),
                                                  ("yuv420p", 2, 131080, "bfloat16", "NCHW")])
def test_a_frame_taller_than_one_launch_covers(enc, fmt, w, h, dtype, layout):
    check_tall(enc, fmt, w, h, dtype, layout)


@pytest.mark.gpu
def test_more_frames_than_one_launch_takes(enc):
    check_many_frames(enc)


@pytest.mark.gpu
def test_from_tensor_frames_are_frames(enc, dec):
    check_from_tensor_frames(enc, dec)


@pytest.mark.gpu
def test_refusals_on_live_contexts(enc, dec):
    check_refusals(enc, dec)


def run_equalities(enc, dec):
    """what the poisoned pass runs: every byte against the model on a spread of layouts, and every equality case"""
    for fmt in ("rgb24", "yuv420p", "yuv422p10le", "xyz12le"):
        check_layout(dec, fmt)
    check_values(dec)
    for case in EQUAL:
        check_equal(enc, dec, case)
    check_round_trip(enc, dec)
    check_tall(enc, "gray", 4, 65540, "float16", "NCHW")
    check_from_tensor_frames(enc, dec)


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
