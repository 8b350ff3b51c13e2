#!/usr/bin/env python3
"""Resized windows (htj2k_frames_to_tensor_resized, k_frame_resize): what a launch costs beside the copy kernel of the same
box and beside the torch eager chain that makes the nearest equivalent tensor from the same device buffer.

    python tools/gpu_resize_bench.py [--frames 64] [--iters 7] [--filter triangle]

For 64 device-resident C2-sized frames (3840 x 2160) of rgb24, rgb48le and yuv422p10le, to float16 NCHW with ImageNet's
scale and bias: the whole frame to 224 x 224, the whole frame to 1920 x 1080, and a random window of 8 to 100 % of the
frame's area (aspect 3/4 to 4/3, as a random-resized-crop draws it; one window per frame, drawn once) to 224 x 224.  The
torch chain is the one a user writes today: view the bytes, mask, crop, de-interleave or replicate chroma, .float(),
F.interpolate(mode="bilinear", antialias=True), multiply, add, .half(); where the windows differ it runs frame by frame.
The two tensors are not equal bit for bit -- the library's weights are 14-bit integers -- so before anything is timed
their largest difference is printed.  After a warm-up, --iters rounds alternate the library call, the chain and
htj2k_copy_bench in one process; each figure is the median with its spread.  The library's time is the device time of its
launch (htj2k_compare_ms), the chain's is between two events on torch's stream.  GB/s is the windows' sample bytes read
once plus element bytes written per second; the copy kernel's figure counts the same two.

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
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def random_windows(rng, n):
    """one (ox, oy, ww, wh) per frame: 8 to 100 % of the area, aspect 3/4 to 4/3 in log space, clipped to the frame"""
    out = []
    for _ in range(n):
        area = rng.uniform(0.08, 1.0) * W * H
        aspect = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
        ww = int(min(W, max(1, round(np.sqrt(area * aspect)))))
        wh = int(min(H, max(1, round(np.sqrt(area / aspect)))))
        out.append((int(rng.integers(0, W - ww + 1)), int(rng.integers(0, H - wh + 1)), ww, wh))
    return out


def samples(torch, tensors, fmt, bits, n, i0, i1, window):
    """frames i0 .. i1 - 1 of the planes' bytes (one tensor a plane, n slots) -> (i1 - i0, 3, wh, ww) integer samples of
    the window, chroma replicated"""
    size = cm.LAYOUTS[fmt][5]
    shift, mask = cm.shift(fmt, bits), (1 << bits) - 1
    ox, oy, ww, wh = window
    planes = []
    for t, (rows, cols) in zip(tensors, cm.plane_shapes(fmt, W, H)):
        v = t.view(n, -1)[i0:i1, : rows * cols * size]
        if size == 2:
            v = v.view(torch.int16)
        planes.append(v.view(i1 - i0, rows, cols))
    if len(planes) == 1:
        x = planes[0].view(i1 - i0, H, W, 3)[:, oy:oy + wh, ox:ox + ww].permute(0, 3, 1, 2)
    else:
        y, u, v = planes
        c0, c1 = ox >> 1, ((ox + ww - 1) >> 1) + 1
        y = y[:, oy:oy + wh, ox:ox + ww]
        u, v = (c[:, oy:oy + wh, c0:c1].repeat_interleave(2, dim=2)[:, :, (ox & 1):(ox & 1) + ww] for c in (u, v))
        x = torch.stack([y, u, v], dim=1)
    if size == 2 or shift or mask != 0xFF:
        x = (x.to(torch.int32) >> shift) & mask
    return x


def torch_chain(torch, F, tensors, fmt, bits, n, windows, size, scale, bias):
    """-> (n, 3, out_h, out_w) float16; one interpolate where the frames share a window, else one a frame"""
    ow, oh = size

    def one(i0, i1, window):
        x = samples(torch, tensors, fmt, bits, n, i0, i1, window).float()
        x = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False, antialias=True)
        return ((x * scale.view(1, 3, 1, 1)) + bias.view(1, 3, 1, 1)).half()

    if windows is None:
        return one(0, n, (0, 0, W, H))
    return torch.cat([one(i, i + 1, w) for i, w in enumerate(windows)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--filter", default="triangle", choices=m.RESIZE_FILTERS)
    ap.add_argument("--share", type=int, default=0, help="knob resize_share: 0 the library's choice, 1 .. 6: 1 .. 32 lanes a horizontal sum")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    n = a.frames
    dec = m.Decoder(device_id=0)
    dec.set_int("resize_share", a.share)
    rng = np.random.default_rng(1)
    wins = random_windows(np.random.default_rng(2), n)
    cases = [("whole_to_224", None, (224, 224)), ("whole_to_1080p", None, (1920, 1080)), ("random_window_to_224", wins, (224, 224))]
    res = {"metric": "htj2k_frames_to_tensor_resized", "frames": n, "size": [W, H], "device": dec.device_name(), "iters": a.iters,
           "filter": a.filter, "resize_share": a.share, "date": time.strftime("%Y-%m-%d"), "layouts": {}}
    for fmt, bits in cb.LAYOUTS:
        fa, ta = cb.device_frames(torch, fmt, bits, n, rng)
        peak = (1 << bits) - 1
        scale_l, bias_l = [1 / (peak * s) for s in STD], [-x / s for x, s in zip(MEAN, STD)]
        scale = torch.tensor(scale_l, dtype=torch.float32, device="cuda")
        bias = torch.tensor(bias_l, dtype=torch.float32, device="cuda")
        size = cm.LAYOUTS[fmt][5]
        outs = {name: torch.empty((n, 3, oh, ow), dtype=torch.float16, device="cuda") for name, _, (ow, oh) in cases}
        times = {name: {"lib": [], "torch": []} for name, _, _ in cases}
        times["copy"] = []

        def lib_ms(name, windows, out_size):
            dec.to_tensor_resized(fa, fmt, bits, out_size, windows, a.filter, "float16", "NCHW", scale_l, bias_l, on_device=True, out=outs[name])
            return dec.compare_ms()

        def chain_ms(windows, out_size):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            x = torch_chain(torch, F, ta, fmt, bits, n, windows, out_size, scale, bias)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), x

        diffs = {}
        for name, windows, out_size in cases:               # the warm-up (the first calls allocate), and how far apart the two are
            lib_ms(name, windows, out_size)
            _, x = chain_ms(windows, out_size)
            diffs[name] = float((x.float() - outs[name].float()).abs().max())
            del x
        dec.copy_bench(512, 2)
        for _ in range(a.iters):
            for name, windows, out_size in cases:
                times[name]["lib"].append(lib_ms(name, windows, out_size))
                times[name]["torch"].append(chain_ms(windows, out_size)[0])
            times["copy"].append(dec.copy_bench(512, 5))
        copy = cb.spread(times["copy"])
        row = {"copy_gb_s_read_plus_written": copy}
        cw = cm.LAYOUTS[fmt][2]
        for name, windows, (ow, oh) in cases:
            ws = windows if windows is not None else [(0, 0, W, H)] * n
            # a window's samples read once: chroma columns at their own width
            read = sum(sum((((ox + ww - 1) >> s) - (ox >> s) + 1) * wh for s in (0, cw, cw)) for ox, oy, ww, wh in ws) * size
            moved = float(read + n * 3 * ow * oh * 2)
            lib = cb.spread(times[name]["lib"])
            r = {"ms": lib, "gb_s_read_plus_written": cb.spread([moved / x / 1e6 for x in times[name]["lib"]]),
                 "torch_chain_ms": cb.spread(times[name]["torch"]), "largest_difference_from_the_chain": diffs[name]}
            r["share_of_copy_rate"] = round(r["gb_s_read_plus_written"]["median"] / copy["median"], 3)
            r["torch_over_lib"] = round(r["torch_chain_ms"]["median"] / lib["median"], 2)
            row[name] = r
        res["layouts"][fmt] = row
        print(fmt, json.dumps(row), flush=True)
        del ta, outs
        torch.cuda.empty_cache()
    print(json.dumps(res))
    dec.close()


if __name__ == "__main__":
    main()
