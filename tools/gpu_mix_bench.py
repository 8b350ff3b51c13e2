#!/usr/bin/env python3
"""The tensor calls with a colour matrix (htj2k_frames_to_tensor_mix, k_frame_mix / k_frame_mix_any; the resized call's
scratch pass, k_tensor_mix): what a launch costs beside the torch eager chain that makes the same tensor from the same
device buffer, beside the plain call that reads the same bytes, and beside the copy kernel of the same box.

    python tools/gpu_mix_bench.py [--frames 64] [--iters 7]

For 64 device-resident 3840 x 2160 frames, after a warm-up, --iters rounds alternate in one process:
  (a) the library call with a mix: yuv422p10le to RGB float16 and float32 NCHW (BT.709 limited range, ImageNet gain and
      offset folded in), yuv420p to RGB float16, rgb24 to BGR float16 NHWC, rgb24 to one luma channel; and the first row
      on the general route alone (tensor_path 1)
  (b) the torch eager chain a user writes today: view the bytes, mask, repeat_interleave the chroma, .float(), a multiply
      and an add kernel per term, stack, convert; timed between two events on torch's stream.  Its tensor and the
      library's are compared with torch.equal before anything is timed
  (c) htj2k_frames_to_tensor without a mix on the same frames (it reads the same bytes; a channel per component)
  (d) htj2k_copy_bench
  (e) one resized row: whole yuv422p10le frames to 224 x 224 float16 with and without a mix: what the scratch pass adds
Each figure is the median with its spread.  The library's time is the device time of its launches (htj2k_compare_ms).
GB/s is sample bytes read plus element bytes written per second; the copy kernel's figure counts the same two.

One JSON line at the end.  The one condition is (a) < (b) on every row: the exit status is 1 where it does not hold."""
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
import mix_model as mm  # noqa: E402

W, H = cb.W, cb.H
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
# (row, layout, bits, mix, dtype, tensor layout)
ROWS = [("yuv422p10le_rgb_f16", "yuv422p10le", 10, "ycbcr", "float16", "NCHW"),
        ("yuv422p10le_rgb_f32", "yuv422p10le", 10, "ycbcr", "float32", "NCHW"),
        ("yuv420p_rgb_f16", "yuv420p", 8, "ycbcr", "float16", "NCHW"),
        ("rgb24_bgr_f16_nhwc", "rgb24", 8, "bgr", "float16", "NHWC"),
        ("rgb24_luma_f16", "rgb24", 8, "luma", "float16", "NCHW")]


def make_mix(kind, bits):
    if kind == "ycbcr":
        return m.Decoder.ycbcr_mix(709, bits, gain=[1 / s for s in STD], offset=[-a / s for a, s in zip(MEAN, STD)])
    if kind == "bgr":
        return m.tensor_mix(np.eye(3)[::-1] / 255.0, [-0.5, -0.5, -0.5])
    return m.tensor_mix([[0.2126 / 255, 0.7152 / 255, 0.0722 / 255]])


def torch_chain(torch, tensors, fmt, bits, n, mix, dtype, layout):
    """the eager chain: the planes' bytes (one tensor a plane, n slots) -> (n, K, H, W) or (n, H, W, K) of dtype"""
    nc, planar, cw, ch, _, size = cm.LAYOUTS[fmt]
    shift, mask = cm.shift(fmt, bits), (1 << bits) - 1
    nout, mat, b = mm.unpack(mix)
    planes = []
    for t, (rows, cols) in zip(tensors, cm.plane_shapes(fmt, W, H)):
        v = t.view(n, -1)[:, : rows * cols * size]
        if size == 2:
            v = v.view(torch.int16)
        planes.append(v.view(n, rows, cols))
    if planar:
        comps = [planes[0]]
        for c in planes[1:]:
            if cw:
                c = c.repeat_interleave(1 << cw, dim=2)[:, :, :W]
            if ch:
                c = c.repeat_interleave(1 << ch, dim=1)[:, :H]
            comps.append(c)
    else:
        x = planes[0].view(n, H, W, nc)
        comps = [x[..., c] for c in range(nc)]
    if size == 2 or shift or mask != 0xFF:
        comps = [(c.to(torch.int32) >> shift) & mask for c in comps]
    comps = [c.float() for c in comps]
    out = []
    for k in range(nout):
        a = torch.mul(comps[0], float(mat[k][0]))
        for c in range(1, nc):
            a = torch.add(a, torch.mul(comps[c], float(mat[k][c])))
        out.append(torch.add(a, float(b[k])))
    return torch.stack(out, dim=1 if layout == "NCHW" else 3).to(dtype)


def bits_view(torch, t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=7)
    a = ap.parse_args()
    import torch
    n = a.frames
    dec = m.Decoder(device_id=0)
    rng = np.random.default_rng(1)
    res = {"metric": "htj2k_frames_to_tensor_mix", "frames": n, "size": [W, H], "device": dec.device_name(), "iters": a.iters,
           "date": time.strftime("%Y-%m-%d"), "rows": {}}
    frames = {}
    ok = True
    for name, fmt, bits, kind, dtype, layout in ROWS:
        if fmt not in frames:
            frames.clear()
            torch.cuda.empty_cache()
            frames[fmt] = cb.device_frames(torch, fmt, bits, n, rng)
        fa, ta = frames[fmt]
        mix = make_mix(kind, bits)
        k, es, size = mix.nout, (4 if dtype == "float32" else 2), cm.LAYOUTS[fmt][5]
        tdt = getattr(torch, dtype)
        out = torch.empty((n, k, H, W) if layout == "NCHW" else (n, H, W, k), dtype=tdt, device="cuda")
        plain = torch.empty((n, 3, H, W) if layout == "NCHW" else (n, H, W, 3), dtype=tdt, device="cuda")

        def lib_ms(path=0):
            dec.set_int("tensor_path", path)
            try:
                dec.to_tensor(fa, fmt, bits, dtype, layout, on_device=True, out=out, mix=mix)
            finally:
                dec.set_int("tensor_path", 0)
            return dec.compare_ms(), dec.tensor_last_route()

        def plain_ms():
            dec.to_tensor(fa, fmt, bits, dtype, layout, scale=1 / ((1 << bits) - 1), bias=-0.5, on_device=True, out=plain)
            return dec.compare_ms(), dec.tensor_last_route()

        def chain_ms():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            x = torch_chain(torch, ta, fmt, bits, n, mix, tdt, layout)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), x

        general = name == ROWS[0][0]
        _, route = lib_ms()                                  # equal first, and the warm-up: the first calls allocate
        _, x = chain_ms()
        if not torch.equal(bits_view(torch, x), bits_view(torch, out)):
            sys.exit("gpu_mix_bench: %s differs from the torch chain" % name)
        if general:
            out.zero_()
            lib_ms(1)
            if not torch.equal(bits_view(torch, x), bits_view(torch, out)):
                sys.exit("gpu_mix_bench: %s on the general route differs from the torch chain" % name)
        del x
        _, plain_route = plain_ms()
        dec.copy_bench(512, 2)
        t = {"lib": [], "torch": [], "plain": [], "copy": [], "general": []}
        for _ in range(a.iters):
            t["lib"].append(lib_ms()[0])
            t["torch"].append(chain_ms()[0])
            t["plain"].append(plain_ms()[0])
            if general:
                t["general"].append(lib_ms(1)[0])
            t["copy"].append(dec.copy_bench(512, 5))
        read = n * sum(rows * cols for rows, cols in cm.plane_shapes(fmt, W, H)) * size
        moved, moved_plain = float(read + n * k * W * H * es), float(read + n * 3 * W * H * es)
        lib, chain, pl, copy = cb.spread(t["lib"]), cb.spread(t["torch"]), cb.spread(t["plain"]), cb.spread(t["copy"])
        row = {"route": route, "K": k, "ms": lib, "torch_chain_ms": chain, "torch_over_lib": round(chain["median"] / lib["median"], 2),
               "faster_than_chain": max(t["lib"]) < min(t["torch"]), "plain_route": plain_route, "plain_ms": pl,
               "lib_over_plain": round(lib["median"] / pl["median"], 3),
               "gb_s_read_plus_written": round(moved / lib["median"] / 1e6, 1), "plain_gb_s": round(moved_plain / pl["median"] / 1e6, 1),
               "copy_gb_s_read_plus_written": copy, "share_of_copy_rate": round(moved / lib["median"] / 1e6 / copy["median"], 3)}
        ok = ok and lib["median"] < chain["median"]
        if general:
            g = cb.spread(t["general"])
            row["general_route_ms"] = g
            row["general_share_of_copy_rate"] = round(moved / g["median"] / 1e6 / copy["median"], 3)
            ok = ok and g["median"] < chain["median"]
        res["rows"][name] = row
        print(name, json.dumps(row), flush=True)
        del out, plain
    # (e) whole frames to 224 x 224 with and without a mix
    frames.clear()
    torch.cuda.empty_cache()
    fa, ta = cb.device_frames(torch, "yuv422p10le", 10, n, rng)
    mix = make_mix("ycbcr", 10)
    small = torch.empty((n, 3, 224, 224), dtype=torch.float16, device="cuda")
    t = {"mix": [], "plain": []}
    for it in range(a.iters + 1):
        dec.to_tensor_resized(fa, "yuv422p10le", 10, (224, 224), None, "triangle", "float16", "NCHW", on_device=True, out=small, mix=mix)
        ms_mix, route = dec.compare_ms(), dec.tensor_last_route()
        dec.to_tensor_resized(fa, "yuv422p10le", 10, (224, 224), None, "triangle", "float16", "NCHW", scale=1 / 1023, on_device=True, out=small)
        if it:                                               # the first round allocates
            t["mix"].append(ms_mix)
            t["plain"].append(dec.compare_ms())
    res["resized_224_yuv422p10le_f16"] = {"route": route, "mix_ms": cb.spread(t["mix"]), "plain_ms": cb.spread(t["plain"]),
                                          "mix_over_plain": round(cb.spread(t["mix"])["median"] / cb.spread(t["plain"])["median"], 3)}
    res["lib_faster_than_chain_on_every_row"] = ok
    print(json.dumps(res))
    dec.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
