#!/usr/bin/env python3
"""Tensors as frames (htj2k_encode_tensor, k_enc_unpack_tensor; htj2k_tensor_to_frames, k_tensor_frame): what the
encoder's first stage costs when it reads a float tensor itself, beside the torch eager chain that builds the packed frame
from the same tensor for htj2k_encode_batch(in_on_device = 1), and beside k_enc_unpack alone on ready-made frames.

    python tools/gpu_tensor_encode_bench.py [--frames 64] [--iters 7]

For 64 device-resident 3840 x 2160 images in [0, 1] -- as a float16 and a float32 NCHW tensor and a float16 NHWC one --
encoded as rgb24 and as rgb48le (lossless 5/3, the defaults), three legs alternate in one process, --iters rounds after
a warm-up, every figure a median with its spread:
  (a) encode_tensor; htj2k_enc_stage_ms' first figure is k_enc_unpack_tensor
  (b) the chain a user writes today -- multiply, add, round, clamp, convert, permute().contiguous() -- timed between two
      events on torch's stream, then encode_device on its buffer; stage_ms' first figure is k_enc_unpack
  (c) encode_device on the frames htj2k_tensor_to_frames made of the same tensor: k_enc_unpack alone, the stage as it
      was; the device time of k_tensor_frame (htj2k_compare_ms) stands beside the chain's
Before anything is timed (a)'s streams are compared with (b)'s byte for byte.  The byte ratio is (element bytes read +
4 bytes written per sample) over (sample bytes read + the same written), what (a) / (c) would be if both ran at one
rate.  The one condition, checked at the end: on every row (a)'s stage takes no longer than (b)'s chain plus stage.

One JSON line a row and one at the end."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import cmp_model as cm  # noqa: E402
import ffmpeg_ht_amd as m  # noqa: E402
import gpu_compare_bench as cb  # noqa: E402

W, H = cb.W, cb.H
ROWS = [(fmt, bits, dtype, layout) for fmt, bits in (("rgb24", 8), ("rgb48le", 16))
        for dtype, layout in (("float16", "NCHW"), ("float32", "NCHW"), ("float16", "NHWC"))]


def images(torch, n, dtype, layout):
    """n images in [0, 1]: a ramp, a tilt per channel and noise, made on the device; one picture in every slot"""
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.linspace(0, 1, H, device="cuda").view(1, H, 1)
    x = torch.linspace(0, 1, W, device="cuda").view(1, 1, W)
    tilt = torch.tensor([0.9, 0.7, 0.5], device="cuda").view(3, 1, 1)
    img = ((x + y) / 2 * tilt + 0.1 * torch.rand((3, H, W), device="cuda", generator=g)).clamp(0, 1)
    if layout == "NHWC":
        img = img.permute(1, 2, 0)
    return img.to(getattr(torch, dtype)).unsqueeze(0).repeat(n, 1, 1, 1).contiguous()


def chain(torch, t, layout, bits, size):
    """the packed frames of the tensor, built the eager way: (n, H, W, 3) of uint8, or of int16 holding the 16-bit words"""
    peak = (1 << bits) - 1
    x = t.to(torch.float32) * float(peak)
    x = x + 0.0
    x = torch.round(x).clamp(0, peak)
    x = x.to(torch.uint8) if size == 1 else x.to(torch.int32).to(torch.int16)
    if layout == "NCHW":
        x = x.permute(0, 2, 3, 1)
    return x.contiguous()


def frames_of(buf, n, fmt, size):
    arr = (m.Frame * n)()
    for i in range(n):
        arr[i].data[0] = buf.data_ptr() + i * H * W * 3 * size
        arr[i].linesize[0] = W * 3 * size
        arr[i].width, arr[i].height, arr[i].pix_fmt = W, H, m.PIX_NAMES.index(fmt)
    return arr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=7)
    a = ap.parse_args()
    import torch
    n = a.frames
    dec, enc = m.Decoder(device_id=0), m.Encoder(0)
    res = {"metric": "htj2k_encode_tensor", "frames": n, "size": [W, H], "device": dec.device_name(), "iters": a.iters,
           "date": time.strftime("%Y-%m-%d"), "rows": {}}
    o = m._enc_opts()
    ok = True
    for fmt, bits, dtype, layout in ROWS:
        size, peak = cm.LAYOUTS[fmt][5], (1 << bits) - 1
        t = images(torch, n, dtype, layout)
        es = t.element_size()
        spec = m.tensor_spec(dtype, layout, None, float(peak), 0.0)
        cap = n * m.Encoder.bound(W, H, fmt, bits)
        out = [np.empty(cap, np.uint8) for _ in range(2)]
        offs = [(ctypes.c_size_t * (n + 1))() for _ in range(2)]
        torch.cuda.synchronize()

        def leg_a(k=0):
            t0 = time.perf_counter()
            r = enc.L.htj2k_encode_tensor(enc.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * es), n, W, H,
                                          m.PIX_NAMES.index(fmt), bits, ctypes.byref(spec), ctypes.byref(o),
                                          out[k].ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap), 0, offs[k])
            if r < 0:
                raise m.Htj2kError(r, "htj2k_encode_tensor")
            return enc.stage_ms()[0], (time.perf_counter() - t0) * 1e3

        def leg_b(k=1):
            t0 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            buf = chain(torch, t, layout, bits, size)
            e1.record()
            torch.cuda.synchronize()
            enc.encode_into(frames_of(buf, n, fmt, size), n, bits, o, out[k].ctypes.data_as(ctypes.c_void_p), cap, offs[k], in_on_device=1)
            return e0.elapsed_time(e1), enc.stage_ms()[0], (time.perf_counter() - t0) * 1e3

        fr, keep = dec.from_tensor(t, fmt, bits, layout, float(peak))

        def leg_c(k=1):
            enc.encode_into(fr, n, bits, o, out[k].ctypes.data_as(ctypes.c_void_p), cap, offs[k], in_on_device=1)
            return enc.stage_ms()[0]

        def tensor_frame_ms():
            r = dec.L.htj2k_tensor_to_frames(dec.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * es), n, bits, ctypes.byref(spec), fr)
            if r < 0:
                raise m.Htj2kError(r, "htj2k_tensor_to_frames")
            return dec.compare_ms()

        # equal first, and the warm-up: the first calls allocate
        leg_a()
        leg_b()
        total = offs[0][n]
        if list(offs[0]) != list(offs[1]) or not np.array_equal(out[0][:total], out[1][:total]):
            sys.exit("gpu_tensor_encode_bench: %s %s %s: encode_tensor differs from the encode of the chain's frames" % (fmt, dtype, layout))
        leg_c()
        if list(offs[0]) != list(offs[1]) or not np.array_equal(out[0][:total], out[1][:total]):
            sys.exit("gpu_tensor_encode_bench: %s %s %s: encode_tensor differs from the encode of tensor_to_frames' frames" % (fmt, dtype, layout))
        ta, tb_chain, tb_unpack, tc, tk, wa, wb = [], [], [], [], [], [], []
        for _ in range(a.iters):
            s, whole = leg_a()
            ta.append(s)
            wa.append(whole)
            c, s, whole = leg_b()
            tb_chain.append(c)
            tb_unpack.append(s)
            wb.append(whole)
            tc.append(leg_c())
            tk.append(tensor_frame_ms())
        ratio = (3 * es + 12) / (3 * size + 12)
        row = {"a_unpack_tensor_ms": cb.spread(ta), "b_chain_ms": cb.spread(tb_chain), "b_unpack_ms": cb.spread(tb_unpack),
               "b_chain_plus_unpack_ms": cb.spread([x + y for x, y in zip(tb_chain, tb_unpack)]), "c_unpack_ms": cb.spread(tc),
               "k_tensor_frame_ms": cb.spread(tk), "a_whole_call_ms": cb.spread(wa), "b_whole_call_ms": cb.spread(wb),
               "byte_ratio": round(ratio, 3), "stream_bytes": int(total)}
        row["a_over_c"] = round(row["a_unpack_tensor_ms"]["median"] / row["c_unpack_ms"]["median"], 3)
        row["c_spread"] = round(row["c_unpack_ms"]["max"] / row["c_unpack_ms"]["min"], 3)
        row["chain_plus_unpack_over_a"] = round(row["b_chain_plus_unpack_ms"]["median"] / row["a_unpack_tensor_ms"]["median"], 2)
        row["holds"] = row["a_unpack_tensor_ms"]["median"] <= row["b_chain_plus_unpack_ms"]["median"]
        ok = ok and row["holds"]
        name = "%s_%s_%s" % (fmt, dtype, layout)
        res["rows"][name] = row
        print(name, json.dumps(row), flush=True)
        del t, fr, keep
        torch.cuda.empty_cache()
    res["condition_holds"] = ok
    print(json.dumps(res))
    enc.close()
    dec.close()
    if not ok:
        sys.exit("gpu_tensor_encode_bench: encode_tensor's unpack stage is slower than the chain plus k_enc_unpack on some row")


if __name__ == "__main__":
    main()
