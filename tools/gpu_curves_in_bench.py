#!/usr/bin/env python3
"""Tensors as frames with transfer curves (htj2k_encode_tensor_curves, k_enc_unpack_tensor_curves;
htj2k_tensor_to_frames_curves, k_tensor_frame_curves): what the encoder's first stage costs when it decodes an sRGB tensor
to linear light, mixes it to XYZ and encodes it by the 1 / 2.6 law itself, beside the stage with the matrix alone, beside
k_enc_unpack on ready-made frames, beside the torch eager chain that builds the same frames, and beside the copy kernel.

    python tools/gpu_curves_in_bench.py [--frames 64] [--iters 5] [--dtype float16]

For 64 device-resident 2048 x 1080 RGB images in [0, 1] (NCHW), one process, --iters rounds after a warm-up, every figure a
median with its range:
  xyz      sRGB to X'Y'Z' (rgb48le at 12 bits, mct = 0; Decoder.dcp_curves_in): the unpack stage with curves
           (htj2k_enc_stage_ms' first figure), the stage with the matrix alone (htj2k_encode_tensor_mix with the same matrix
           times 4095: other samples, the same traffic), k_enc_unpack on the frames htj2k_tensor_to_frames_curves wrote, the
           torch eager chain (tests/curve_in_model.torch_chain, the definition's order) plus k_enc_unpack on its frames,
           k_tensor_frame_curves, and the copy kernel's rate (htj2k_copy_bench)
  grid     the same stage under HTJ2K_ENC_CURVES_GRID = 1, 2, 4, 8, 16 (an encoder each)
  bt709    linear RGB to yuv422p10le: the BT.709 OETF as an in-curve of 4097 knots uniform in the fourth root, the BT.709
           matrix, the box chroma rule; beside the matrix alone
  pq2020   linear RGB to yuv420p10le: the PQ inverse EOTF as an in-curve of 4097 knots uniform in the eighth root, the
           BT.2020 matrix, the box chroma rule; beside the matrix alone
Before anything is timed the streams of the curves call, of the chain's frames and of htj2k_tensor_to_frames_curves'
frames are compared byte for byte.  No figure is fixed in advance.  One JSON line a row and one at the end."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import curve_in_model as cim  # noqa: E402
import ffmpeg_ht_amd as m  # noqa: E402
import gpu_compare_bench as cb  # noqa: E402

W, H = 2048, 1080


def images(torch, n, dtype):
    """n images in [0, 1]: a ramp, a tilt per channel and noise, made on the device; one picture in every slot"""
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.linspace(0, 1, H, device="cuda").view(1, H, 1)
    x = torch.linspace(0, 1, W, device="cuda").view(1, 1, W)
    tilt = torch.tensor([0.9, 0.7, 0.5], device="cuda").view(3, 1, 1)
    img = ((x + y) / 2 * tilt + 0.1 * torch.rand((3, H, W), device="cuda", generator=g)).clamp(0, 1)
    return img.to(getattr(torch, dtype)).unsqueeze(0).repeat(n, 1, 1, 1).contiguous()


def encoder(grid=None):
    if grid is None:
        return m.Encoder(0)
    os.environ["HTJ2K_ENC_CURVES_GRID"] = str(grid)
    try:
        return m.Encoder(0)
    finally:
        del os.environ["HTJ2K_ENC_CURVES_GRID"]


class Call:
    """one encode call on prepared arguments; run() -> the first stage's device ms"""

    def __init__(self, enc, t, n, fmt, bits, spec, mix, curves, o):
        self.enc, self.t, self.n, self.fmt, self.bits, self.spec, self.mix, self.curves, self.o = enc, t, n, fmt, bits, spec, mix, curves, o
        self.cap = n * m.Encoder.bound(W, H, fmt, bits, mct=0)
        self.out = np.empty(self.cap, np.uint8)
        self.offs = (ctypes.c_size_t * (n + 1))()

    def run(self):
        e, t = self.enc, self.t
        r = e.L.htj2k_encode_tensor_curves(e.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * t.element_size()), self.n, W, H,
                                           m.PIX_NAMES.index(self.fmt), self.bits, ctypes.byref(self.spec), ctypes.byref(self.mix),
                                           None if self.curves is None else ctypes.byref(self.curves), ctypes.byref(self.o),
                                           self.out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(self.cap), 0, self.offs)
        if r < 0:
            raise m.Htj2kError(r, "htj2k_encode_tensor_curves")
        return e.stage_ms()[0]

    def frames(self, arr):
        self.enc.encode_into(arr, self.n, self.bits, self.o, self.out.ctypes.data_as(ctypes.c_void_p), self.cap, self.offs, in_on_device=1)
        return self.enc.stage_ms()[0]

    def same(self, other):
        total = self.offs[self.n]
        return list(self.offs) == list(other.offs) and np.array_equal(self.out[:total], other.out[:total])


def scaled(mix, k):
    """the mix with every weight times k: the matrix alone lands in the sample range as the curves' gain does"""
    out = m.TensorMixIn.from_buffer_copy(mix)
    for c in range(4):
        for j in range(4):
            out.m[c][j] = mix.m[c][j] * k
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--dtype", default="float16", choices=["float16", "float32", "bfloat16"])
    a = ap.parse_args()
    import torch
    n = a.frames
    dec, enc = m.Decoder(device_id=0), encoder()
    copy_gbs = dec.copy_bench()
    res = {"metric": "htj2k_encode_tensor_curves", "frames": n, "size": [W, H], "device": dec.device_name(), "iters": a.iters, "dtype": a.dtype,
           "date": time.strftime("%Y-%m-%d"), "copy_gbs": round(copy_gbs, 1)}
    t = images(torch, n, a.dtype)
    es = t.element_size()
    spec = m.tensor_spec(a.dtype, "NCHW")
    o = m._enc_opts(mct=0)

    # ---- sRGB to X'Y'Z'
    fmt, bits = "rgb48le", 12
    mix, q = m.Decoder.dcp_curves_in(709, "srgb")
    curved, alone, ready = (Call(enc, t, n, fmt, bits, spec, mix, q, o), Call(enc, t, n, fmt, bits, spec, scaled(mix, 4095.0), None, o),
                            Call(enc, t, n, fmt, bits, spec, mix, q, o))
    fr, keep = dec.from_tensor(t, fmt, bits, "NCHW", mix=mix, curves=q)

    def chain():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        words = cim.torch_chain(t, mix, q, bits, 3, 4)                       # (n, 3, H, W) int32, the sample words
        packed = words.permute(0, 2, 3, 1).to(torch.int16).contiguous()
        e1.record()
        torch.cuda.synchronize()
        arr = (m.Frame * n)()
        for i in range(n):
            arr[i].data[0], arr[i].linesize[0] = packed.data_ptr() + i * H * W * 6, W * 6
            arr[i].width, arr[i].height, arr[i].pix_fmt = W, H, m.PIX_NAMES.index(fmt)
        return e0.elapsed_time(e1), ready.frames(arr)

    def frame_kernel_ms():
        r = dec.L.htj2k_tensor_to_frames_curves(dec.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * es), n, bits, ctypes.byref(spec),
                                                ctypes.byref(mix), ctypes.byref(q), fr)
        if r < 0:
            raise m.Htj2kError(r, "htj2k_tensor_to_frames_curves")
        return dec.compare_ms()

    curved.run()
    alone.run()
    chain()
    if not curved.same(ready):
        sys.exit("gpu_curves_in_bench: encode_tensor(curves=) differs from the encode of the chain's frames")
    ready.frames(fr)
    if not curved.same(ready):
        sys.exit("gpu_curves_in_bench: encode_tensor(curves=) differs from the encode of tensor_to_frames_curves' frames")
    ta, tm_, tc, tch, tcu, tk = [], [], [], [], [], []
    for _ in range(a.iters):
        ta.append(curved.run())
        tm_.append(alone.run())
        tc.append(ready.frames(fr))
        c, u = chain()
        tch.append(c)
        tcu.append(u)
        tk.append(frame_kernel_ms())
    moved = n * (3 * W * H * es + 3 * W * H * 4)                             # the stage reads the tensor and writes three int32 planes
    row = {"unpack_curves_ms": cb.spread(ta), "unpack_mix_alone_ms": cb.spread(tm_), "unpack_ready_frames_ms": cb.spread(tc),
           "chain_ms": cb.spread(tch), "chain_unpack_ms": cb.spread(tcu), "chain_plus_unpack_ms": cb.spread([x + y for x, y in zip(tch, tcu)]),
           "k_tensor_frame_curves_ms": cb.spread(tk), "stream_bytes": int(curved.offs[n])}
    row["unpack_curves_gbs"] = round(moved / (row["unpack_curves_ms"]["median"] * 1e6), 1)
    row["unpack_curves_over_copy"] = round(row["unpack_curves_gbs"] / copy_gbs, 3)
    row["curves_over_mix_alone"] = round(row["unpack_curves_ms"]["median"] / row["unpack_mix_alone_ms"]["median"], 2)
    row["chain_plus_unpack_over_curves"] = round(row["chain_plus_unpack_ms"]["median"] / row["unpack_curves_ms"]["median"], 1)
    res["xyz"] = row
    print("xyz", json.dumps(row), flush=True)
    del fr, keep
    torch.cuda.empty_cache()

    # ---- the grid factor
    grid = {}
    for factor in (1, 2, 4, 8, 16):
        e = encoder(factor)
        call = Call(e, t, n, fmt, bits, spec, mix, q, o)
        call.run()
        if not call.same(curved):
            sys.exit("gpu_curves_in_bench: the grid factor %d changes the streams" % factor)
        grid[str(factor)] = cb.spread([call.run() for _ in range(a.iters)])
        e.close()
    res["grid"] = grid
    print("grid", json.dumps(grid), flush=True)

    # ---- linear RGB to Y'CbCr: the transfer function before the matrix and the chroma rule
    for name, out_fmt, standard, kind, root in (("bt709", "yuv422p10le", 709, "bt709_encode", 2), ("pq2020", "yuv420p10le", 2020, "pq_encode", 3)):
        ymix = m.Decoder.rgb_mix_in(standard, 10, chroma="box")
        yq = m.tensor_curves_in(m.tensor_curve_in(m.curve_table(kind, 4097, 0.0, 1.0, root=root), 0.0, 4096.0, root), None, 7, 0)
        oy = m._enc_opts()
        with_curve, without = Call(enc, t, n, out_fmt, 10, spec, ymix, yq, oy), Call(enc, t, n, out_fmt, 10, spec, ymix, None, oy)
        with_curve.run()
        without.run()
        row = {"unpack_curves_ms": cb.spread([with_curve.run() for _ in range(a.iters)]),
               "unpack_mix_alone_ms": cb.spread([without.run() for _ in range(a.iters)])}
        row["curves_over_mix_alone"] = round(row["unpack_curves_ms"]["median"] / row["unpack_mix_alone_ms"]["median"], 2)
        res[name] = row
        print(name, json.dumps(row), flush=True)
    print(json.dumps(res))
    enc.close()
    dec.close()


if __name__ == "__main__":
    main()
