#!/usr/bin/env python3
"""Frames as tensors (htj2k_frames_to_tensor, k_frame_tensor / k_frame_tensor_any): what a launch costs beside the copy
kernel of the same box and beside the torch eager chain that makes the same tensor from the same device buffer, and what a
pipe delivers when frames come back as tensors.

    python tools/gpu_tensor_bench.py [--frames 64] [--iters 7] [--pipe-frames 240] [--window 1.0]

Kernel legs.  For 64 device-resident C2-sized frames (3840 x 2160) of rgb24, rgb48le and yuv422p10le: the full frame to
float16 NCHW and to float32 NCHW, a 224 x 224 window of every frame that starts on a group boundary (the fast route where
the plane allows it) and one that does not (the general route), and the full frame on the general route alone
(tensor_path 1).  The torch chain is the one a user writes today: view the bytes, mask, de-interleave with
permute().contiguous() or replicate chroma with repeat_interleave, convert, multiply, add, convert.  Before anything is
timed the chain's tensor and the library's are compared with torch.equal.  After a warm-up, --iters rounds alternate the
library call, the chain and htj2k_copy_bench in one process; each figure is the median with its spread.  The library's
time is the device time of its launches (htj2k_compare_ms), the chain's is between two events on torch's stream.  GB/s is
sample bytes read plus element bytes written per second; the copy kernel's figure counts the same two.

Pipe legs.  --pipe-frames distinct 4K rgb24 frames (bench.py's generator) through a pipe of 8 x 3, received as float16
NCHW tensors into one destination (htj2k_pipe_receive_tensor) and as device pointers (htj2k_pipe_receive_device):
Gpixel/s over a window of at least --window seconds after 48 warm-up frames, the legs alternating, twice.

One JSON line at the end.  There is no gate."""
import argparse
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
import gpu_hash_bench as hb  # noqa: E402

W, H = cb.W, cb.H
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def torch_chain(torch, tensors, fmt, bits, n, dtype, scale, bias, window):
    """the eager chain: the planes' bytes (one tensor a plane, n slots) -> (n, 3, h, w) of dtype"""
    size = cm.LAYOUTS[fmt][5]
    shift, mask = cm.shift(fmt, bits), (1 << bits) - 1
    planes = []
    for t, (rows, cols) in zip(tensors, cm.plane_shapes(fmt, W, H)):
        v = t.view(n, -1)[:, : rows * cols * size]
        if size == 2:
            v = v.view(torch.int16)
        planes.append(v.view(n, rows, cols))
    if len(planes) == 1:                                   # interleaved: (n, H, W, 3) -> channels first
        x = planes[0].view(n, H, W, 3)
        if window:
            (ow, oh), (ox, oy) = window
            x = x[:, oy:oy + oh, ox:ox + ow]
        x = x.permute(0, 3, 1, 2).contiguous()
    else:                                                   # 4:2:2: chroma replicated to the luma's width
        y, u, v = planes
        (ow, oh), (ox, oy) = window if window else ((W, H), (0, 0))
        c0, c1 = ox >> 1, ((ox + ow - 1) >> 1) + 1        # crop first, as a user would, then replicate
        y = y[:, oy:oy + oh, ox:ox + ow]
        u, v = (c[:, oy:oy + oh, c0:c1].repeat_interleave(2, dim=2)[:, :, (ox & 1):(ox & 1) + ow] for c in (u, v))
        x = torch.stack([y, u, v], dim=1)
    if size == 2 or shift or mask != 0xFF:
        x = (x.to(torch.int32) >> shift) & mask
    x = x.to(torch.float32) * scale.view(1, 3, 1, 1)
    x = x + bias.view(1, 3, 1, 1)
    return x.to(dtype)


def kernel_legs(dec, torch, n, iters):
    rng = np.random.default_rng(1)
    rows = {}
    for fmt, bits in cb.LAYOUTS:
        fa, ta = cb.device_frames(torch, fmt, bits, n, rng)
        peak = (1 << bits) - 1
        scale_l, bias_l = [1 / (peak * s) for s in STD], [-a / s for a, s in zip(MEAN, STD)]
        scale = torch.tensor(scale_l, dtype=torch.float32, device="cuda")
        bias = torch.tensor(bias_l, dtype=torch.float32, device="cuda")
        size = cm.LAYOUTS[fmt][5]
        variants = [("full_f16", "float16", None, 0), ("full_f32", "float32", None, 0), ("full_f16_general", "float16", None, 1),
                    ("win224_on_f16", "float16", ((224, 224), (1808, 968)), 0), ("win224_off_f16", "float16", ((224, 224), (1801, 969)), 0)]
        outs, times = {}, {}
        for name, dtype, window, path in variants:
            ow, oh = window[0] if window else (W, H)
            outs[name] = torch.empty((n, 3, oh, ow), dtype=getattr(torch, dtype), device="cuda")
            times[name] = {"lib": [], "torch": []}
        times["copy"] = []

        def lib_ms(name, dtype, window, path):
            dec.set_int("tensor_path", path)
            try:
                dec.to_tensor(fa, fmt, bits, dtype, "NCHW", size=window[0] if window else None, origins=window[1] if window else None,
                              scale=scale_l, bias=bias_l, on_device=True, out=outs[name])
            finally:
                dec.set_int("tensor_path", 0)
            return dec.compare_ms(), dec.tensor_last_route()

        def chain_ms(dtype, window):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            x = torch_chain(torch, ta, fmt, bits, n, getattr(torch, dtype), scale, bias, window)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), x

        routes = {}
        for name, dtype, window, path in variants:          # equal first, and the warm-up: the first calls allocate
            _, routes[name] = lib_ms(name, dtype, window, path)
            _, x = chain_ms(dtype, window)
            if not torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32),
                               outs[name].view(torch.int16 if x.element_size() == 2 else torch.int32)):
                sys.exit("gpu_tensor_bench: %s %s differs from the torch chain" % (fmt, name))
            del x
        dec.copy_bench(512, 2)
        for _ in range(iters):
            for name, dtype, window, path in variants:
                times[name]["lib"].append(lib_ms(name, dtype, window, path)[0])
                if path == 0:
                    times[name]["torch"].append(chain_ms(dtype, window)[0])
            times["copy"].append(dec.copy_bench(512, 5))
        copy = cb.spread(times["copy"])
        row = {"copy_gb_s_read_plus_written": copy}
        for name, dtype, window, path in variants:
            ow, oh = window[0] if window else (W, H)
            es = 4 if dtype == "float32" else 2
            # samples read: a window's luma-sized share of every component (replicated chroma is read once per sample)
            read = n * sum((ow >> (cm.LAYOUTS[fmt][2] if c in (1, 2) else 0)) * oh for c in range(3)) * size
            moved = float(read + n * 3 * ow * oh * es)
            lib = cb.spread(times[name]["lib"])
            r = {"route": routes[name], "ms": lib, "gb_s_read_plus_written": cb.spread([moved / x / 1e6 for x in times[name]["lib"]])}
            r["share_of_copy_rate"] = round(r["gb_s_read_plus_written"]["median"] / copy["median"], 3)
            if times[name]["torch"]:
                r["torch_chain_ms"] = cb.spread(times[name]["torch"])
                r["torch_over_lib"] = round(r["torch_chain_ms"]["median"] / lib["median"], 2)
            row[name] = r
        rows[fmt] = row
        print(fmt, json.dumps(row), flush=True)
        del ta, outs
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--pipe-frames", type=int, default=240)
    ap.add_argument("--window", type=float, default=1.0, help="seconds a pipe leg's clock runs at least")
    a = ap.parse_args()
    import torch
    dec = m.Decoder(device_id=0)
    res = {"metric": "htj2k_frames_to_tensor", "frames": a.frames, "size": [W, H], "device": dec.device_name(), "iters": a.iters,
           "date": time.strftime("%Y-%m-%d"), "layouts": kernel_legs(dec, torch, a.frames, a.iters)}
    if a.pipe_frames > 0:
        t0 = time.perf_counter()
        pkts, _ = hb.make_packets(a.pipe_frames)
        print("made %d packets in %.1f s" % (len(pkts), time.perf_counter() - t0), flush=True)
        out = torch.empty((1, 3, H, W), dtype=torch.float16, device="cuda")
        legs = {"receive_tensor_f16": lambda p: p.receive_tensor("float16", "NCHW", scale=1 / 255, out=out),
                "receive_device": lambda p: p.receive_device()}
        rates = {k: [] for k in legs}
        for _ in range(2):
            for name, fn in legs.items():
                rate, nfr, first = hb.pipe_leg(dec, pkts, fn, a.window)
                rates[name].append(round(rate, 2))
                print(name, round(rate, 2), "Gpixel/s over", nfr, "frames", flush=True)
        res["pipe_4k_rgb24_x%d_gpixel_s" % a.pipe_frames] = rates
    print(json.dumps(res))
    dec.close()


if __name__ == "__main__":
    main()
