"""Tensors as frames with transfer curves on the device: every byte of every plane buffer that htj2k_tensor_to_frames_curves
writes against the numpy model (curve_in_model) between guard zones, htj2k_encode_tensor_curves byte for byte against the
encode of those frames, the corners of the definition, the identity against the _mix call, the torch chain, the X'Y'Z'
chain through the decoder, rounds, size limits, the grid knobs and the refusals on live contexts.  No tolerance appears
here: the device equals the model."""
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
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cmp_model as cm
import curve_in_model as cim
import ffmpeg_ht_amd as m
import tensor_mix_in_model as tmi
import tensor_model as tm
from test_curves_in_host import random_curves, special_values, struct_of as curves_struct
from test_tensor_in_gpu import picture, to_device
from test_tensor_mix_in_gpu import COMBOS, GUARD, OFFS, PADS, Guarded, a_mix, device_planes, plane_bytes, shaped, struct_of as mix_struct

EINVAL, ENOSYS, PATCHWELCOME = -22, -38, -0x45574150
LAYOUTS = ["xyz12le", "rgb48le", "rgb24", "gray", "ya8", "yuv444p12le", "yuv422p10le", "yuv420p", "yuv411p", "yuv410p", "yuva420p"]
BITS = {"xyz12le": 12, "rgb48le": 12, "yuv444p12le": 12, "yuv422p10le": 10}
WIDTHS, HEIGHTS = [1, 2, 3, 5, 63, 64, 65, 255, 257], [1, 2, 3, 4, 5]
ROOTS = [(0, 0), (1, 2), (3, None), (None, 3), (2, 1), (None, 0), (0, None), (3, 3), (None, 1), (2, None), (1, 0), (None, 2)]
GRID = 4                        # HTJ2K_ENC_CURVES_GRID of the second encoder; the cases marked "both" size their tables to it (fit_knots)
FACTORS = [2, GRID, 1, 4096]    # of the four encoders of `encs`: the default, GRID, a workgroup per 256 footprints, one workgroup a frame
KNOBS = [0, 1, 4096, 16]        # curves_grid of the decoder, call by call: the default, a workgroup per 256 samples, one workgroup, between


def scaled_curves(rng, K, nc, bits, roots, knots=(17, 9)):
    """random_curves whose out-curve, gain and offset land the samples mostly inside the range of `bits` bits"""
    q = random_curves(rng, K, nc, roots, knots)
    peak = (1 << bits) - 1
    q["gain"] = (rng.uniform(0.7, 1.1, 4) * peak).astype(np.float32)
    q["offset"] = rng.uniform(-0.02, 0.05, 4).astype(np.float32) * peak
    return q


def unit_mix(fmt, K, chroma, rng):
    """weights that keep curved values in 0 .. 1 mostly inside 0 .. 1, some negative, one of them -0"""
    nc = cm.LAYOUTS[fmt][0]
    mat = rng.uniform(-0.2, 1.0, size=(nc, K)) / (0.6 * K)
    mat[rng.integers(nc), rng.integers(K)] = -0.0
    return mat.astype(np.float32), rng.uniform(-0.05, 0.1, size=nc).astype(np.float32), chroma


def to_frames_curves(dec, t, tbits, fmt, bits, dtype, layout, w, h, mix, q, pad=0, off=0):
    n = t.shape[0]
    q = cim.unpack(q)
    dst = Guarded(fmt, w, h, n, pad, off)
    spec, s, cs = m.tensor_spec(dtype, layout), mix_struct(mix), curves_struct(q)
    r = dec.L.htj2k_tensor_to_frames_curves(dec.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * t.element_size()), n, int(bits),
                                            ctypes.byref(spec), ctypes.byref(s), ctypes.byref(cs), dst.arr)
    what = (fmt, bits, dtype, layout, w, h, n, mix[2], mix[0].shape, q["in"] and q["in"][3], q["out"] and q["out"][3], q["in_mask"], q["out_mask"], pad, off)
    assert r == 0, (r, what)
    want = cim.frames(tbits, fmt, bits, mix, q, dtype, layout)
    try:
        dst.expect(want)
    except AssertionError as e:
        raise AssertionError((what, e.args))
    return want


def check_layout(dec, fmt):
    """every width with every element type and tensor layout; heights, K, the chroma rule, the roots, which curves there
    are, the grid knob, paddings, offsets and batch sizes change from call to call"""
    bits = BITS.get(fmt, 8)
    rng = np.random.default_rng(100 + LAYOUTS.index(fmt))
    j = LAYOUTS.index(fmt)
    seen_k, seen_r = set(), set()
    try:
        for w in WIDTHS:
            for dtype, layout in COMBOS:
                j += 1
                h, n, K, chroma = HEIGHTS[j % 5], 1 + j % 2, 1 + (j // 2) % 4, (j // 8 + j) % 2
                roots = ROOTS[j % len(ROOTS)]
                seen_k.add((K, chroma))
                seen_r.add(roots)
                dec.set_int("curves_grid", KNOBS[(j // 3) % 4])
                t, tbits = to_device(shaped(picture(n, K, h, w, rng), layout), dtype)
                q = scaled_curves(rng, K, cm.LAYOUTS[fmt][0], bits, roots, (17, 9) if j % 5 else (4097, 2))
                to_frames_curves(dec, t, tbits, fmt, bits, dtype, layout, w, h, unit_mix(fmt, K, chroma, rng), q, PADS[j % 4], OFFS[(j // 4) % 4])
    finally:
        dec.set_int("curves_grid", 0)
    assert len(seen_k) == 8 and len(seen_r) == len(ROOTS), (seen_k, seen_r)


def check_values(enc, dec):
    """NaN, infinities, -0, negatives under a root, arguments beyond both ends of a table, subnormals under sqrtf: on every
    element type, with tables of 2 and 4097 knots, each curve alone and both; the codestreams agree with the frames"""
    f32 = np.float32
    vals = np.array(special_values() + [0.3, 0.7, 0.04, 0.96, 1.5, -0.5, 0.999, 1e-20], f32)
    w, h = len(vals), 4
    img = np.stack([np.stack([np.roll(vals, k + 3 * y) for y in range(h)]) for k in range(3)])[None]           # (1, 3, h, w)
    rng = np.random.default_rng(21)
    for fi, (fmt, bits) in enumerate((("gray", 8), ("yuv422p10le", 10), ("yuv420p", 8), ("rgb48le", 12), ("xyz12le", 12))):
        nc = cm.LAYOUTS[fmt][0]
        eye = np.zeros((nc, 3), f32)
        eye[np.arange(nc), np.arange(nc) % 3] = 1.0
        mixes = [(eye, None), (np.ones((nc, 3), f32), None), (np.array([[1.0, -1.0, 0.0]] * nc, f32), None),
                 (np.array([[2.0, 2.0, 2.0]] * nc, f32), np.full(nc, -3e38, f32))]
        for ci, (dtype, layout) in enumerate(COMBOS):
            t, tbits = to_device(shaped(img, layout), dtype)
            for mi, (mat, off) in enumerate(mixes):
                roots = ROOTS[(fi + ci + mi) % len(ROOTS)]
                q = scaled_curves(rng, 3, nc, bits, roots, (2, 4097) if (ci + mi) % 2 else (4097, 2))
                q["in_mask"], q["out_mask"] = 7, (1 << nc) - 1
                mix = (mat, off, (ci + mi) % 2)
                want = to_frames_curves(dec, t, tbits, fmt, bits, dtype, layout, w, h, mix, q, PADS[ci % 4], OFFS[mi % 4])
                if fmt != "xyz12le" and mi < 2:
                    opts = dict(levels=1, mct=0) if fmt == "rgb48le" else dict(levels=1)
                    got = enc.encode_tensor(t, fmt, bits, layout, mix=mix_struct(mix), curves=curves_struct(q), **opts)
                    assert got == enc.encode_batch(want, fmt, bits, **opts), (fmt, dtype, layout, mi)
    # what the model says of them, spelled out once: one channel, the table { 10, 20 } over 0 .. 1 indexed by the square root
    one, obits = to_device(np.array([np.nan, -np.inf, -4.0, -0.0, 0.0, 0.25, 1.0, 4.0, np.inf, 1e-40], f32).reshape(1, 1, 1, 10), "float32")
    q = {"in": (np.array([10.0, 20.0], f32), 0.0, 1.0, 1), "in_mask": 1, "out_mask": 0}
    want = to_frames_curves(dec, one, obits, "gray", 8, "float32", "NCHW", 10, 1, (np.array([[1.0]], f32), None, 0), q)
    assert want[0][0].tolist() == [[10, 10, 10, 10, 10, 15, 20, 20, 20, 10]]
    # the same table without a root: a NaN takes knot 0 through E's own clamp, and 0.25 is a quarter of the way
    q = {"in": (np.array([10.0, 20.0], f32), 0.0, 1.0, 0), "in_mask": 1, "out_mask": 0}
    want = to_frames_curves(dec, one, obits, "gray", 8, "float32", "NCHW", 10, 1, (np.array([[1.0]], f32), None, 0), q)
    assert want[0][0].tolist() == [[10, 10, 10, 10, 10, 12, 20, 20, 20, 10]]
    # subnormals under three roots: 2^-149 ^ (1/8) = 2^-18.625, times 2^18 through the table { 0, 2^18 }
    tiny, tb = to_device(np.array([1e-45, 1e-40, 1.1754944e-38, 5e-324], f32).reshape(1, 1, 2, 2), "float32")
    q = {"out": (np.array([0.0, 2.0 ** 18], f32), 0.0, 1.0, 3), "in_mask": 0, "out_mask": 1, "gain": 100.0}
    want = to_frames_curves(dec, tiny, tb, "gray16le", 16, "float32", "NCHW", 2, 2, (np.array([[1.0]], f32), None, 0), q)
    assert want[0][0].tolist() == [[65, 262], [476, 0]]


# ------------------------------------------------------------------ htj2k_encode_tensor_curves against the encoder's own streams

def three_ways(encs, dec, t, tbits, fmt, bits, dtype, layout, mix, q, opts):
    """encode_tensor(curves=) under every grid factor, encode_device(from_tensor(curves=)) and encode_batch(model frames):
    equal streams"""
    n = t.shape[0]
    s, cs = mix_struct(mix), curves_struct(q)
    enc = encs[0]
    got = enc.encode_tensor(t, fmt, bits, layout, mix=s, curves=cs, **opts)
    ms = enc.stage_ms()
    frames, keep = dec.from_tensor(t, fmt, bits, layout, mix=s, curves=cs)
    via = enc.encode_device(list(frames), fmt, bits, **opts)
    model = cim.frames(tbits, fmt, bits, mix, q, dtype, layout)
    ref = enc.encode_batch(model, fmt, bits, **opts)
    what = (fmt, bits, dtype, layout, tuple(t.shape), mix[2], opts)
    assert len(got) == n and all(len(x) > 0 for x in got), what
    assert ref == via, ("from_tensor(curves=)'s frames encode differently from the model's", what)
    assert got == via, ("encode_tensor(curves=) differs from the encode of its frames", what, [k for k in range(n) if got[k] != via[k]])
    for other in encs[1:]:
        assert other.encode_tensor(t, fmt, bits, layout, mix=s, curves=cs, **opts) == got, ("the grid factor changes the streams", what)
    assert ms[0] > 0, ms
    del keep
    return got


def table_bytes(knots, roots):
    """bytes of both tables as a workgroup stages them: n + 1 floats each, padded to 16 bytes; a curve that is not there has none"""
    return 4 * sum((n + 1 + 3) & ~3 for n, r in zip(knots, roots) if r is not None)


def unpack_grid(fmt, w, h, n, K, dtype, knots, roots, factor):
    """(workgroups a frame gets in k_enc_unpack_tensor_curves, strides the busiest of them makes): round_unpack_tensor_curves'
    rule (htj2k_encode.hip, curve_grid) restated: a workgroup per 256 footprints, but no more than leave each `factor` times
    the tables' bytes of tensor to read, and never fewer than one"""
    sw, sh = cm.LAYOUTS[fmt][2], cm.LAYOUTS[fmt][3]
    blocks = -(-((-(-w >> sw)) * (-(-h >> sh))) // 256)
    cap = K * w * h * (4 if dtype == "float32" else 2) // (factor * table_bytes(knots, roots))
    gx = max(1, min(blocks, 256 if n >= 64 else 2048, cap))
    return gx, -(-blocks // gx)


def fit_knots(fmt, w, h, n, K, dtype, roots):
    """knots for which the encoder of factor GRID gives the frame several workgroups that each make several strides: the
    last curve's table grows until half the blocks (two at the least) are what the tensor's bytes allow"""
    for last in range(9, 4098):
        knots = (33, last) if roots[1] is not None else (last, 9)
        gx, strides = unpack_grid(fmt, w, h, n, K, dtype, knots, roots, GRID)
        _, blocks = unpack_grid(fmt, w, h, n, K, dtype, knots, roots, 4096)       # one workgroup: its strides are the blocks
        if 2 <= gx and 2 * gx <= blocks:
            return knots
    raise AssertionError(("no table size gives several workgroups and several strides", fmt, w, h))


# (layout, bits, w, h, n, element, tensor layout, K, chroma, roots, options, grid)
# grid "both": under the encoder of factor GRID a frame takes several workgroups of several strides each (asserted; the
#              sub-sampled ones have clipped footprints in the last column and row);
#      "split": under factor 1 several workgroups, under factor 4096 one workgroup of several strides (asserted);
#      "big": tables of 33 and 4097 knots, which leave these small frames one workgroup under every factor
EQUAL = [
    ("rgb48le", 12, 257, 5, 1, "float32", "NCHW", 3, 0, (0, 2), dict(levels=1, mct=0), "both"),
    ("rgb48le", 12, 255, 3, 2, "float16", "NHWC", 3, 0, (None, 2), dict(levels=2, mct=0, irreversible=True, qstep=0.5), "split"),
    ("rgb48le", 12, 64, 48, 2, "bfloat16", "NCHW", 4, 0, (0, 3), dict(levels=3, mct=0, target_bytes="half"), "big"),
    ("rgb24", 8, 65, 4, 2, "float32", "NHWC", 3, 0, (1, 1), dict(levels=1), "split"),
    ("rgb24", 8, 40, 24, 2, "float16", "NCHW", 2, 1, (2, None), dict(levels=2, irreversible=True, tile=(16, 16)), "split"),
    ("yuv422p10le", 10, 257, 5, 1, "float32", "NCHW", 3, 1, (2, 0), dict(levels=1), "split"),
    ("yuv422p10le", 10, 257, 11, 2, "float16", "NCHW", 3, 1, (0, 2), dict(levels=1), "both"),
    ("yuv422p10le", 10, 63, 2, 2, "float16", "NHWC", 3, 0, (0, 0), dict(levels=1, irreversible=True), ""),
    ("yuv420p", 8, 257, 5, 1, "float32", "NHWC", 3, 1, (3, 1), dict(levels=1), "split"),
    ("yuv420p", 8, 257, 21, 1, "float32", "NHWC", 3, 1, (1, 3), dict(levels=2), "both"),
    ("yuv420p", 8, 255, 23, 2, "bfloat16", "NCHW", 3, 0, (2, None), dict(levels=2, irreversible=True), "both"),
    ("yuv420p", 8, 65, 47, 1, "bfloat16", "NCHW", 3, 0, (None, 0), dict(levels=3, irreversible=True, qstep=0.5, target_bytes="half"), "split"),
    ("yuv420p", 8, 64, 48, 3, "float16", "NCHW", 4, 1, (2, 2), dict(levels=3, tile=(32, 32)), "big"),
    ("yuv411p", 8, 255, 3, 1, "float32", "NCHW", 3, 1, (1, None), dict(levels=1), ""),
    ("yuv411p", 8, 1025, 7, 1, "float16", "NHWC", 3, 1, (1, 0), dict(levels=1), "both"),
    ("yuv410p", 8, 257, 5, 1, "float16", "NHWC", 2, 1, (0, 3), dict(levels=1), ""),
    ("yuv410p", 8, 1029, 21, 1, "float32", "NCHW", 3, 1, (3, 2), dict(levels=1), "both"),
    ("yuva420p", 8, 5, 5, 2, "float32", "NCHW", 4, 1, (2, 2), dict(levels=1), ""),
    ("yuva420p", 8, 255, 13, 1, "float16", "NHWC", 4, 1, (0, 1), dict(levels=1), "both"),
    ("yuv444p12le", 12, 33, 17, 2, "float32", "NHWC", 3, 1, (3, 0), dict(levels=2), "split"),
    ("gray", 8, 257, 2, 2, "bfloat16", "NHWC", 3, 0, (1, 2), dict(levels=1), "split"),
    ("ya8", 8, 2, 1, 3, "float32", "NCHW", 1, 1, (None, 1), dict(levels=0), ""),
]


def case_knots(case):
    """the case's table sizes, and what its `grid` word promises of them, held to the launch rule"""
    fmt, bits, w, h, n, dtype, layout, K, chroma, roots, opts, grid = case
    if grid == "both":
        knots = fit_knots(fmt, w, h, n, K, dtype, roots)
        gx, strides = unpack_grid(fmt, w, h, n, K, dtype, knots, roots, GRID)
        assert gx >= 2 and strides >= 2, (case, knots, gx, strides)
        if cm.LAYOUTS[fmt][2] or cm.LAYOUTS[fmt][3]:           # sub-sampled: the last column or row of footprints is clipped
            assert w % (1 << cm.LAYOUTS[fmt][2]) or h % (1 << cm.LAYOUTS[fmt][3]), case
        return knots
    knots = (33, 4097) if grid == "big" else (17, 9)
    if grid == "split":
        many, _ = unpack_grid(fmt, w, h, n, K, dtype, knots, roots, 1)
        one, strides = unpack_grid(fmt, w, h, n, K, dtype, knots, roots, 4096)
        assert many >= 2 and one == 1 and strides >= 2, (case, many, one, strides)
    return knots


def check_equal(encs, dec, case):
    fmt, bits, w, h, n, dtype, layout, K, chroma, roots, opts, grid = case
    rng = np.random.default_rng(300 + EQUAL.index(case))
    mix = unit_mix(fmt, K, chroma, rng)
    q = scaled_curves(rng, K, cm.LAYOUTS[fmt][0], bits, roots, case_knots(case))
    t, tbits = to_device(shaped(picture(n, K, h, w, rng, "NCHW", -0.05, 1.05), layout), dtype)
    opts = dict(opts)
    if opts.get("target_bytes") == "half":
        free = encs[0].encode_tensor(t, fmt, bits, layout, mix=mix_struct(mix), curves=curves_struct(q), **{k: v for k, v in opts.items() if k != "target_bytes"})
        opts["target_bytes"] = max(len(s) for s in free) // 2
    return three_ways(encs, dec, t, tbits, fmt, bits, dtype, layout, mix, q, opts)


# ------------------------------------------------------------------ the identity, the torch chain, the cinema chain

def check_identity(enc, dec):
    """the two-knot table { 0, 1 } before the mix, no out-curve, gain 1 and offset 0 on elements in 0 .. 1: the _mix call"""
    rng = np.random.default_rng(12)
    ident = lambda K: m.tensor_curves_in(m.tensor_curve_in([0.0, 1.0], 0.0, 1.0), None, (1 << K) - 1, 0, 1.0, 0.0)
    for fmt in ("rgb24", "yuv420p", "yuv422p10le", "yuv410p", "yuva420p", "ya8", "xyz12le"):
        nc, bits = cm.LAYOUTS[fmt][0], BITS.get(fmt, 8)
        for (dtype, layout), (w, h) in zip(COMBOS, ((5, 3), (8, 4), (1, 1), (3, 5), (6, 2), (2, 2))):
            K, chroma = 1 + (w + h) % 4, w % 2
            v = rng.uniform(0.0, 1.0, size=(2, K, h, w)).astype(np.float32)
            v[0, 0, 0, 0] = -0.0
            t, _ = to_device(shaped(v, layout), dtype)
            mat, off, _ = a_mix(fmt, K, chroma, rng, bits)
            s = m.tensor_mix_in(mat, off, chroma)
            _, mixed = dec.from_tensor(t, fmt, bits, layout, mix=s)
            _, curved = dec.from_tensor(t, fmt, bits, layout, mix=s, curves=ident(K))
            assert plane_bytes(mixed) == plane_bytes(curved), ("the identity curve is not the mix call", fmt, dtype, layout, w, h)
            if fmt != "xyz12le":
                assert enc.encode_tensor(t, fmt, bits, layout, mix=s, levels=0) == enc.encode_tensor(t, fmt, bits, layout, mix=s, curves=ident(K), levels=0)


def check_default_masks(enc, dec):
    """masks left to the call are cut to the mix's K channels and the layout's C components: one channel to gray and to ya8,
    two channels to rgb24, equal to the calls with the masks written out"""
    rng = np.random.default_rng(13)
    cv = lambda: m.tensor_curve_in(rng.uniform(0, 1, 9).astype(np.float32), 0.0, 8.0, 1)
    for fmt, K in (("gray", 1), ("ya8", 1), ("rgb24", 2), ("yuv420p", 4)):
        nc = cm.LAYOUTS[fmt][0]
        t, _ = to_device(picture(1, K, 4, 6, rng), "float32")
        mix = m.tensor_mix_in(rng.uniform(0, 1, (nc, K)))
        a, b = cv(), cv()
        auto = m.tensor_curves_in(a, b, gain=255.0)
        said = m.tensor_curves_in(a, b, min(7, (1 << K) - 1), min(7, (1 << nc) - 1), gain=255.0)
        assert auto.auto_masks == (True, True) and said.auto_masks == (False, False) and (auto.in_mask, auto.out_mask) == (7, 7)
        _, x = dec.from_tensor(t, fmt, 8, mix=mix, curves=auto)
        _, y = dec.from_tensor(t, fmt, 8, mix=mix, curves=said)
        assert plane_bytes(x) == plane_bytes(y), fmt
        assert enc.encode_tensor(t, fmt, 8, mix=mix, curves=auto, levels=0) == enc.encode_tensor(t, fmt, 8, mix=mix, curves=said, levels=0)
    # a mask that was given is passed as it is, and refused where it names what is not there
    with pytest.raises(m.Htj2kError):
        dec.from_tensor(t, "gray", 8, mix=m.tensor_mix_in(np.ones((1, 4))), curves=m.tensor_curves_in(cv(), cv(), 7, 7))


def check_torch_chain(dec):
    """the torch eager chain on the device, in the definition's order, bit for bit.  torch.sqrt on the device is held to
    numpy's first: the chain can only be the definition where torch's square root is correctly rounded too"""
    rng = np.random.default_rng(4)
    probe = np.concatenate([rng.uniform(0, 1, 200000), rng.uniform(0, 1, 20000) ** 8, [1e-45, 1e-40, 1.1754944e-38, 0.0]]).astype(np.float32)
    exact = np.array_equal(torch.sqrt(torch.from_numpy(probe).cuda()).cpu().numpy().view(np.uint32), np.sqrt(probe).view(np.uint32))
    assert exact, "torch.sqrt on the device is not correctly rounded: the eager chain is then not the definition, and this test says nothing"
    for fmt, bits, w, h in (("rgb48le", 12, 65, 5), ("rgb24", 8, 5, 3), ("gray", 8, 257, 2), ("yuv444p12le", 12, 33, 4), ("xyz12le", 12, 64, 3)):
        nc = cm.LAYOUTS[fmt][0]
        for j, dtype in enumerate(tm.DTYPES):
            K = 1 + (j + w) % 4
            roots = ROOTS[(j + w) % len(ROOTS)]
            t, tbits = to_device(picture(2, K, h, w, rng), dtype)
            mix = unit_mix(fmt, K, 0, rng)
            q = scaled_curves(rng, K, nc, bits, roots, (257, 33))
            _, keep = dec.from_tensor(t, fmt, bits, "NCHW", mix=mix_struct(mix), curves=curves_struct(q))
            got = device_planes(keep, fmt, w, h, 2)
            want = cim.torch_chain(t, mix, q, bits, nc, cm.shift(fmt, bits)).cpu().numpy()
            for i in range(2):
                comps = got[i] if cm.LAYOUTS[fmt][1] else [got[i][0].reshape(h, w, nc)[:, :, c] for c in range(nc)]
                for c in range(nc):
                    assert np.array_equal(comps[c].astype(np.int64), want[i, c]), (fmt, dtype, roots, i, c)


def check_cinema_chain(enc, dec):
    """an sRGB tensor to an X'Y'Z' codestream (rgb48le at 12 bits, mct = 0), decoded under a pixel-format request of
    xyz12le: the frames from_tensor(..., "xyz12le", curves=) writes; and the model's"""
    rng = np.random.default_rng(8)
    xyz = m.Decoder(device_id=0, req_pix_fmt=m.PIX_NAMES.index("xyz12le"))
    try:
        for primaries, source, dtype, layout, (w, h) in ((709, "srgb", "float16", "NCHW", (65, 33)), (2020, "pq", "float32", "NHWC", (33, 17)),
                                                        (m.PRIMARIES_P3D65, "linear", "bfloat16", "NCHW", (17, 9)), (709, "bt709", "float32", "NCHW", (5, 3))):
            mix, q = m.Decoder.dcp_curves_in(primaries, source)
            t, tbits = to_device(shaped(picture(2, 3, h, w, rng, "NCHW", 0.0, 1.0), layout), dtype)
            frames, keep = dec.from_tensor(t, "xyz12le", 12, layout, mix=mix, curves=q)
            direct = device_planes(keep, "xyz12le", w, h, 2)
            model = cim.frames(tbits, "xyz12le", 12, mix, q, dtype, layout)
            streams = enc.encode_tensor(t, "rgb48le", 12, layout, mix=mix, curves=q, levels=3, mct=0)
            assert streams == enc.encode_batch(cim.frames(tbits, "rgb48le", 12, mix, q, dtype, layout), "rgb48le", 12, levels=3, mct=0)
            for i in range(2):
                info, planes, consumed, st = xyz.decode(streams[i])
                assert m.PIX_NAMES[info.pix_fmt] == "xyz12le" and (info.width, info.height) == (w, h) and st.n_block_errors == 0
                got = np.asarray(planes[0]).view("<u2").reshape(h, 3 * w)
                assert np.array_equal(got, direct[i][0]), (primaries, source, i)
                assert np.array_equal(got, model[i][0]), (primaries, source, i)
            assert len(np.unique(direct[0][0])) > 20
    finally:
        xyz.close()


# ------------------------------------------------------------------ rounds and size limits

ROUND = 40000


def check_rounds(enc, enc_small, dec):
    """HTJ2K_ENC_ROUND = 40 000 samples: twelve images of 80 x 42 as yuv420p go through seven to a round; the tables are
    uploaded again for the second round, and its frames are read at their own place in the tensor"""
    fmt, bits, w, h, n = "yuv420p", 8, 80, 42, 12
    rng = np.random.default_rng(5)
    for dtype, layout, chroma, roots, opts in (("float16", "NCHW", 1, (2, 0), dict(levels=2)),
                                               ("float32", "NHWC", 0, (0, 3), dict(levels=2, irreversible=True, qstep=0.5))):
        t, tbits = to_device(shaped(picture(n, 3, h, w, rng), layout), dtype)
        mix, q = unit_mix(fmt, 3, chroma, rng), scaled_curves(rng, 3, 3, bits, roots)
        s, cs = mix_struct(mix), curves_struct(q)
        got = enc_small.encode_tensor(t, fmt, bits, layout, mix=s, curves=cs, **opts)
        assert enc_small.last_rounds() == 2, enc_small.last_rounds()
        assert len(set(got)) == n
        assert got == enc.encode_batch(cim.frames(tbits, fmt, bits, mix, q, dtype, layout), fmt, bits, **opts)
        assert got[n - 1] == enc.encode_tensor(t[n - 1:], fmt, bits, layout, mix=s, curves=cs, **opts)[0]


def check_tall(encs, dec, fmt, K, w, h, dtype, layout, chroma, roots):
    """a frame of more rows than a launch's grid.y or grid.z takes: the footprints are walked by index, not by grid row"""
    bits = 8
    rng = np.random.default_rng(h)
    rows = (np.arange(h) % 251 / 250.0).reshape(1, 1, h, 1)
    v = np.clip(rows * np.array([1.0, 0.7, 0.4][:K]).reshape(1, K, 1, 1) + 0.1 * rng.random((1, K, h, w)), 0, 1).astype(np.float32)
    t, tbits = to_device(shaped(v, layout), dtype)
    mix, q = unit_mix(fmt, K, chroma, rng), scaled_curves(rng, K, cm.LAYOUTS[fmt][0], bits, roots)
    opts = dict(levels=1, tile=(0, 4096))
    model = cim.frames(tbits, fmt, bits, mix, q, dtype, layout)
    want = encs[0].encode_batch(model, fmt, bits, **opts)
    for e in encs:
        assert e.encode_tensor(t, fmt, bits, layout, mix=mix_struct(mix), curves=curves_struct(q), **opts) == want, (fmt, w, h)
    _, keep = dec.from_tensor(t, fmt, bits, layout, mix=mix_struct(mix), curves=curves_struct(q))
    for a, b in zip(device_planes(keep, fmt, w, h, 1)[0], model[0]):
        assert np.array_equal(a, b)


def check_many_frames(enc, n=66000):
    """66 000 frames of 2 x 2 as yuv420p in one call: the unpack table goes out in two chunks of grid.z; every stream is its
    image's single-image stream"""
    fmt, bits, w, h, opts = "yuv420p", 8, 2, 2, dict(levels=0)
    rng = np.random.default_rng(9)
    mix, q = unit_mix(fmt, 3, 1, rng), scaled_curves(rng, 3, 3, bits, (1, 2))
    s, cs = mix_struct(mix), curves_struct(q)
    four, fbits = to_device(rng.random((4, 3, h, w)).astype(np.float32), "float16")
    single = [enc.encode_tensor(four[k:k + 1], fmt, bits, "NCHW", mix=s, curves=cs, **opts)[0] for k in range(4)]
    assert single == enc.encode_batch(cim.frames(fbits, fmt, bits, mix, q, "float16", "NCHW"), fmt, bits, **opts) and len(set(single)) == 4
    idx = torch.arange(n, device="cuda") & 3
    t = four[idx].contiguous()
    t[n - 1] = four[1]                                        # the last frame of the second chunk is not what the pattern says
    torch.cuda.synchronize()
    cap = n * m.Encoder.bound(w, h, fmt, bits, **opts)
    out = np.empty(cap, np.uint8)
    offs = (ctypes.c_size_t * (n + 1))()
    spec, o = m.tensor_spec("float16", "NCHW"), m._enc_opts(**opts)
    t0 = time.time()
    r = enc.L.htj2k_encode_tensor_curves(enc.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * 2), n, w, h, m.PIX_NAMES.index(fmt), bits,
                                         ctypes.byref(spec), ctypes.byref(s), ctypes.byref(cs), ctypes.byref(o), out.ctypes.data_as(ctypes.c_void_p),
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
    rng = np.random.default_rng(1)
    t, tbits = to_device(picture(2, 3, h, w, rng), "float16")
    ok_mix = mix_struct(unit_mix(fmt, 3, 1, rng))
    base = scaled_curves(rng, 3, 3, bits, (1, 2))
    ok_q = curves_struct(base)
    good = enc.encode_tensor(t, fmt, bits, "NCHW", mix=ok_mix, curves=ok_q, levels=2, target_bytes=400)

    def said():
        return repr((enc.stage_ms(), enc.rc_info(0), enc.rc_info(1), enc.last_planes(1), enc.last_passes(0), enc.last_rounds()))

    def changed(**kw):
        q = curves_struct(base)
        for k, v in kw.items():
            if k in ("in_", "out"):
                for field, x in v.items():
                    setattr(getattr(q, k), field, x)
            elif k in ("gain", "offset"):
                getattr(q, k)[v[0]] = v[1]
            else:
                setattr(q, k, v)
        return q

    nan_tab = m.tensor_curve_in(np.array([0.0, np.nan, 1.0], np.float32))
    refused = [m.tensor_curves_in(None, None), changed(out=dict(n=1)), changed(in_=dict(n=4098)), changed(out=dict(root=4)), changed(in_=dict(root=-1)),
               changed(in_=dict(t=None)), changed(out=dict(x0=float("nan"))), changed(in_=dict(inv_dx=0.0)), changed(in_=dict(inv_dx=float("inf"))),
               m.tensor_curves_in(nan_tab, None), changed(in_mask=8), changed(out_mask=8), changed(gain=(2, float("inf"))), changed(offset=(0, float("nan")))]
    before = said()
    out = np.full(1 << 16, GUARD, np.uint8)
    offs = (ctypes.c_size_t * 3)(7, 7, 7)
    o = m._enc_opts(levels=2)
    spec = m.tensor_spec("float16", "NCHW")
    nbytes = t.numel() * 2

    def enc_call(q, mix=ok_mix, pix=fmt):
        return enc.L.htj2k_encode_tensor_curves(enc.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(nbytes), 2, w, h, m.PIX_NAMES.index(pix), bits,
                                                ctypes.byref(spec), None if mix is None else ctypes.byref(mix), ctypes.byref(q), ctypes.byref(o),
                                                ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(out.size), 0, offs)

    dst = Guarded(fmt, w, h, 2, 1, 1)

    def frames_call(q, mix=ok_mix):
        return dec.L.htj2k_tensor_to_frames_curves(dec.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(nbytes), 2, bits, ctypes.byref(spec),
                                                   None if mix is None else ctypes.byref(mix), ctypes.byref(q), dst.arr)

    dec.framecrc([dst.arr[0]], fmt, on_device=True)
    ms = dec.compare_ms()
    for i, q in enumerate(refused + [ok_q]):
        mix = None if i == len(refused) else ok_mix            # the last: valid curves without a mix
        assert enc_call(q, mix) == EINVAL, i
        assert (out == GUARD).all() and list(offs) == [7, 7, 7] and before == said(), i
        assert frames_call(q, mix) == EINVAL, i
        assert dec.compare_ms() == ms and dst.untouched(), i
    assert enc_call(ok_q, pix="pal8") == PATCHWELCOME and (out == GUARD).all()
    assert enc_call(changed(out_mask=3, gain=(3, float("nan")))) == 0        # an entry that is not read
    assert frames_call(ok_q) == 0 and dec.compare_ms() > 0 and not dst.untouched()
    assert enc.encode_tensor(t, fmt, bits, "NCHW", mix=ok_mix, curves=ok_q, levels=2, target_bytes=400) == good
    # the encoder does not take the XYZ12 layout, with curves or without
    with pytest.raises(m.Htj2kError):
        enc.encode_tensor(t, "xyz12le", 12, "NCHW", mix=ok_mix, curves=ok_q)
    # the Python entry points: curves without a mix, and something that is no TensorCurvesIn
    with pytest.raises(ValueError):
        enc.encode_tensor(t, fmt, bits, curves=ok_q)
    with pytest.raises(ValueError):
        dec.from_tensor(t, fmt, bits, mix=ok_mix, curves=m.Decoder.dcp_curves()[1])


# ------------------------------------------------------------------ pytest

@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


def _encoder(**env):
    mp = pytest.MonkeyPatch()
    for k, v in env.items():
        mp.setenv(k, str(v))
    try:
        return m.Encoder(0)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def encs():
    """encoders of the grid factors FACTORS: the default; GRID, under which the cases marked "both" take several workgroups of
    several strides; a workgroup per 256 footprints; one workgroup a frame"""
    made = [m.Encoder(0)] + [_encoder(HTJ2K_ENC_CURVES_GRID=f) for f in FACTORS[1:]]
    yield made
    for e in made:
        e.close()


@pytest.fixture(scope="module")
def enc(encs):
    return encs[0]


@pytest.fixture(scope="module")
def enc_small_rounds():
    e = _encoder(HTJ2K_ENC_ROUND=ROUND, HTJ2K_ENC_CURVES_GRID=GRID)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_from_tensor_curves_is_the_model(dec, fmt):
    check_layout(dec, fmt)


@pytest.mark.gpu
def test_values_at_the_corners(enc, dec):
    check_values(enc, dec)


@pytest.mark.gpu
@pytest.mark.parametrize("case", EQUAL, ids=lambda c: "%s-%d-%dx%dx%d-%s-%s-%d-%d-%s-%s-%s" % (c[:9] + ("r%s%s" % c[9], "_".join(sorted(c[10])), c[11])))
def test_encode_tensor_curves_is_the_encode_of_its_frames(encs, dec, case):
    check_equal(encs, dec, case)


@pytest.mark.gpu
def test_identity_curve_is_the_mix_call(enc, dec):
    check_identity(enc, dec)


@pytest.mark.gpu
def test_masks_left_to_the_call(enc, dec):
    check_default_masks(enc, dec)


@pytest.mark.gpu
def test_torch_chain_on_the_device(dec):
    check_torch_chain(dec)


@pytest.mark.gpu
def test_srgb_tensor_to_an_xyz_codestream_and_back(enc, dec):
    check_cinema_chain(enc, dec)


@pytest.mark.gpu
def test_calls_of_several_rounds(enc, enc_small_rounds, dec):
    check_rounds(enc, enc_small_rounds, dec)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,K,w,h,dtype,layout,chroma,roots", [("yuv420p", 3, 2, 65540, "float32", "NHWC", 1, (2, 0)),
                                                                 ("yuv420p", 3, 2, 131080, "bfloat16", "NCHW", 0, (None, 3)),
                                                                 ("gray", 3, 4, 65540, "float16", "NCHW", 0, (1, 1))])
def test_a_frame_of_more_rows_than_a_grid_dimension_takes(encs, dec, fmt, K, w, h, dtype, layout, chroma, roots):
    check_tall(encs[:2], dec, fmt, K, w, h, dtype, layout, chroma, roots)


@pytest.mark.gpu
def test_more_frames_than_one_launch_takes(enc):
    check_many_frames(enc)


@pytest.mark.gpu
def test_refusals_on_live_contexts(enc, dec):
    check_refusals(enc, dec)


def run_equalities(encs, dec):
    """what the poisoned pass runs: every byte against the model on a spread of layouts, and every equality case"""
    for fmt in ("xyz12le", "rgb24", "yuv420p", "yuv422p10le", "yuv410p"):
        check_layout(dec, fmt)
    check_values(encs[0], dec)
    for case in EQUAL:
        check_equal(encs, dec, case)
    check_identity(encs[0], dec)
    check_cinema_chain(encs[0], dec)
    check_tall(encs, dec, "yuv420p", 3, 2, 65540, "float32", "NHWC", 1, (2, 0))


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
    _dec = m.Decoder(device_id=0)
    os.environ["HTJ2K_ENC_CURVES_GRID"] = str(GRID)
    _grid = m.Encoder(0)
    del os.environ["HTJ2K_ENC_CURVES_GRID"]
    _encs = [m.Encoder(0), _grid]
    run_equalities(_encs, _dec)
    for _e in _encs:
        _e.close()
    _dec.close()
    print("%s buffers: ok (%.1f s)" % ("poisoned" if os.environ.get("HTJ2K_POISON") == "1" else "plain", time.time() - t0))
