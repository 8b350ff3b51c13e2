#!/usr/bin/env python3
"""Resized frames (htj2k_resize_frames, k_frame_rescale): what a launch costs beside the resized tensor call at the same
size, beside the torch chain that builds the same frames from that call's float tensor, and beside the copy kernel of
the same box; and what a proxy costs as a whole.

    python tools/gpu_rescale_bench.py [--frames 64] [--iters 7] [--filter triangle] [--proxy-frames 8]

For 64 device-resident C2-sized frames (3840 x 2160) of rgb24, rgb48le and yuv422p10le, to 1920 x 1080 and to 1280 x 720:
  rescale   htj2k_resize_frames into frames allocated once; the device time of its launch (htj2k_compare_ms)
  tensor    htj2k_frames_to_tensor_resized to float16 NCHW at the same size, scale 1 / peak; the same clock
  chain     the route to a resized frame before this call: the tensor call in float32 at scale 1, then torch: round,
            clamp, cast, shift, re-interleave or sub-sample chroma.  The library's device time plus the chain's, between
            two events on torch's stream.  Its frames are not the new call's bit for bit where chroma is sub-sampled (it
            resamples replicated chroma and takes every other column); the largest difference in samples is printed
  copy      htj2k_copy_bench
After a warm-up, --iters rounds alternate all four in one process; each figure is the median with its range.  GB/s is
the source planes' sample bytes read once plus the bytes written per second; the copy kernel's figure counts the same two.
Then a proxy as a whole, on the wall clock: --proxy-frames lossless 4K rgb24 codestreams as one job -- run, resize to
1080p, htj2k_encode_batch from the device -- beside run and encode at full size.

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

W, H = cb.W, cb.H
SIZES = [("to_1080p", (1920, 1080)), ("to_720p", (1280, 720))]


def chain_frames(torch, t, fmt, bits):
    """(n, C, oh, ow) float32 samples -> the planes of n frames of the layout, as the torch chain a user writes"""
    size, shift = cm.LAYOUTS[fmt][5], cm.shift(fmt, bits)
    x = t.round().clamp_(0, (1 << bits) - 1).to(torch.int32)
    if shift:
        x = x << shift
    x = x.to(torch.uint8 if size == 1 else torch.int16)      # 16-bit words as their bit patterns
    if not cm.LAYOUTS[fmt][1]:
        return [x.permute(0, 2, 3, 1).contiguous()]
    cw, ch = cm.LAYOUTS[fmt][2:4]
    return [x[:, 0].contiguous()] + [x[:, c, ::1 << ch, ::1 << cw].contiguous() for c in (1, 2)]


def proxy(dec, torch, frames, iters):
    """the whole call on the wall clock: a job of `frames` lossless 4K rgb24 streams run, resized to 1080p and encoded
    from the device, beside the same job run and encoded at full size"""
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(7)
    img = np.stack([(xx * (3 + c) // 16 + yy * (5 - c) // 16) & 0xFF for c in range(3)], axis=-1).astype(np.int32)
    img = np.clip(img + rng.integers(-4, 5, img.shape), 0, 255).astype(np.uint8).reshape(H, W * 3)
    enc = m.Encoder(device_id=0)
    src = enc.encode(([img]), "rgb24", 8)
    job = dec.job()
    pk = [m.packet(src)] * frames
    out = {"frames": frames, "source_bytes_a_frame": len(src)}
    times = {"proxy_1080p": [], "full_size": []}
    sizes = {}
    for it in range(iters + 1):                             # the first round allocates
        for name in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            job.parse_batch(pk).upload().run()
            if name == "proxy_1080p":
                arr, keep, status = job.resized_frames((1920, 1080))
                streams = enc.encode_device(list(arr), "rgb24", 8)
            else:
                job.wait()
                streams = enc.encode_device([job.device_frame(i) for i in range(frames)], "rgb24", 8)
            dt = (time.perf_counter() - t0) * 1e3
            sizes[name] = len(streams[0])
            if it:
                times[name].append(dt)
    for name in times:
        out[name] = {"ms": cb.spread(times[name]), "fps": round(frames / cb.spread(times[name])["median"] * 1e3, 1), "bytes_a_frame": sizes[name]}
    job.free()
    enc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--filter", default="triangle", choices=m.RESIZE_FILTERS)
    ap.add_argument("--proxy-frames", type=int, default=8, help="0: no proxy leg")
    a = ap.parse_args()
    import torch
    n = a.frames
    flt = m.RESIZE_FILTERS.index(a.filter)
    dec = m.Decoder(device_id=0)
    rng = np.random.default_rng(1)
    res = {"metric": "htj2k_resize_frames", "frames": n, "size": [W, H], "device": dec.device_name(), "iters": a.iters,
           "filter": a.filter, "date": time.strftime("%Y-%m-%d"), "layouts": {}}
    for fmt, bits in cb.LAYOUTS:
        fa, ta = cb.device_frames(torch, fmt, bits, n, rng)
        nc, size, peak = cm.LAYOUTS[fmt][0], cm.LAYOUTS[fmt][5], (1 << bits) - 1
        read = float(sum(r * c for r, c in cm.plane_shapes(fmt, W, H)) * size * n)
        dsts, halves, floats = {}, {}, {}
        for name, (ow, oh) in SIZES:
            dsts[name] = dec.resize_frames(fa, fmt, bits, (ow, oh), None, a.filter, on_device=True)       # allocates the frames; a warm-up
            halves[name] = torch.empty((n, nc, oh, ow), dtype=torch.float16, device="cuda")
            floats[name] = torch.empty((n, nc, oh, ow), dtype=torch.float32, device="cuda")

        def rescale_ms(name):
            r = dec.L.htj2k_resize_frames(dec.h, fa, 1, n, bits, None, flt, dsts[name][0])
            if r < 0:
                raise m.Htj2kError(r, "htj2k_resize_frames")
            return dec.compare_ms()

        def tensor_ms(name, size_):
            dec.to_tensor_resized(fa, fmt, bits, size_, None, a.filter, "float16", "NCHW", 1 / peak, 0.0, on_device=True, out=halves[name])
            return dec.compare_ms()

        def chain_ms(name, size_):
            dec.to_tensor_resized(fa, fmt, bits, size_, None, a.filter, "float32", "NCHW", 1.0, 0.0, on_device=True, out=floats[name])
            lib = dec.compare_ms()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            planes = chain_frames(torch, floats[name], fmt, bits)
            e1.record()
            torch.cuda.synchronize()
            return lib + e0.elapsed_time(e1), planes

        times = {name: {"rescale": [], "tensor": [], "chain": []} for name, _ in SIZES}
        times["copy"] = []
        diffs = {}
        for name, size_ in SIZES:                           # the warm-up, and how far the chain's frames are from the call's
            rescale_ms(name)
            tensor_ms(name, size_)
            _, planes = chain_ms(name, size_)
            keep, worst = dsts[name][1], 0
            for p, cp in enumerate(planes):
                mine = torch.stack([keep[i * len(planes) + p] for i in range(min(n, 4))])
                if size == 2:
                    mine = mine.view(torch.int16)
                a_, b_ = mine.view(cp[:4].shape).to(torch.int32) & 0xFFFF, cp[:4].to(torch.int32) & 0xFFFF
                worst = max(worst, int((a_ - b_).abs().max()) >> cm.shift(fmt, bits))
            diffs[name] = worst
            del planes
        dec.copy_bench(512, 2)
        for _ in range(a.iters):
            for name, size_ in SIZES:
                times[name]["rescale"].append(rescale_ms(name))
                times[name]["tensor"].append(tensor_ms(name, size_))
                times[name]["chain"].append(chain_ms(name, size_)[0])
            times["copy"].append(dec.copy_bench(512, 5))
        copy = cb.spread(times["copy"])
        row = {"copy_gb_s_read_plus_written": copy}
        for name, (ow, oh) in SIZES:
            written = float(sum(r * b for r, b in zip(*m.Decoder.plane_sizes(fmt, ow, oh)[2:])) * n)
            t = times[name]
            r = {"rescale_ms": cb.spread(t["rescale"]), "tensor_f16_ms": cb.spread(t["tensor"]), "torch_chain_ms": cb.spread(t["chain"]),
                 "rescale_gb_s_read_plus_written": cb.spread([(read + written) / x / 1e6 for x in t["rescale"]]),
                 "tensor_gb_s_read_plus_written": cb.spread([(read + n * nc * ow * oh * 2.0) / x / 1e6 for x in t["tensor"]]),
                 "largest_difference_from_the_chain_in_samples": diffs[name]}
            r["share_of_copy_rate"] = round(r["rescale_gb_s_read_plus_written"]["median"] / copy["median"], 3)
            r["tensor_over_rescale"] = round(r["tensor_f16_ms"]["median"] / r["rescale_ms"]["median"], 2)
            r["chain_over_rescale"] = round(r["torch_chain_ms"]["median"] / r["rescale_ms"]["median"], 2)
            row[name] = r
        res["layouts"][fmt] = row
        print(fmt, json.dumps(row), flush=True)
        del ta, dsts, halves, floats
        torch.cuda.empty_cache()
    if a.proxy_frames > 0:
        res["proxy"] = proxy(dec, torch, a.proxy_frames, max(2, a.iters // 2))
        print("proxy", json.dumps(res["proxy"]), flush=True)
    print(json.dumps(res))
    dec.close()


if __name__ == "__main__":
    main()
