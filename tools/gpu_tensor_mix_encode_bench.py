#!/usr/bin/env python3
"""Tensors as frames through a colour matrix (htj2k_encode_tensor_mix, k_enc_unpack_tensor_mix; htj2k_tensor_to_frames_mix,
k_tensor_frame_mix): what the encoder's first stage costs when it reads an RGB tensor, mixes it to Y'CbCr and decimates the
chroma itself, beside the torch eager chain that builds the same frames for htj2k_encode_batch(in_on_device = 1), and beside
k_enc_unpack alone on ready-made frames.

    python tools/gpu_tensor_mix_encode_bench.py [--frames 64] [--iters 7] [--dtype float16]

For 64 device-resident 3840 x 2160 RGB images in [0, 1] (NCHW) encoded as yuv422p10le and yuv420p (BT.709, limited range)
with both chroma rules, and as rgb24 from BGR (lossless 5/3, the defaults), three legs alternate in one process, --iters
rounds after a warm-up, every figure a median with its range:
  (a) encode_tensor(mix=); htj2k_enc_stage_ms' first figure is k_enc_unpack_tensor_mix
  (b) the torch eager chain that builds the same frames -- written in the definition's order, strided slices and
      elementwise operations, so that its frames are the kernel's bit for bit -- timed between two events on torch's
      stream, then encode_device on its planes; stage_ms' first figure is k_enc_unpack
  (c) encode_device on the frames htj2k_tensor_to_frames_mix made of the same tensor: k_enc_unpack alone; the device
      time of k_tensor_frame_mix (htj2k_compare_ms) and its rate stand beside the copy kernel's (htj2k_copy_bench)
Before anything is timed the streams of (a), (b) and (c) are compared byte for byte.  No ratio is fixed in advance: the
number to hold (a) against is (b)'s chain plus unpack, measured in the same run; "a_below_b" says per row how it came out.

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
import gpu_tensor_encode_bench as tb  # noqa: E402

W, H = cb.W, cb.H
ROWS = [("yuv422p10le", 10, "rgb", "cosited"), ("yuv422p10le", 10, "rgb", "box"), ("yuv420p", 8, "rgb", "cosited"), ("yuv420p", 8, "rgb", "box"),
        ("rgb24", 8, "bgr", "cosited")]


def the_mix(how, bits, chroma):
    if how == "bgr":
        return m.tensor_mix_in(np.array([[0, 0, 255.0], [0, 255.0, 0], [255.0, 0, 0]], np.float32), None, chroma)
    return m.Decoder.rgb_mix_in(709, bits, chroma=chroma)


def chain(torch, t, fmt, bits, mix):
    """the planes of the frames, built the eager way in the definition's order: per component the gathered channels (the
    corner element, or the footprint's elements added in raster order times 1 / N), the three products added in their
    order, the offset, round, clamp, convert.  t is (n, 3, H, W) -> a list of contiguous planes (n, rows, samples)"""
    nc, planar, cw, ch, _, size = cm.LAYOUTS[fmt]
    peak = (1 << bits) - 1
    x = t.to(torch.float32)
    comps = []
    for c in range(nc):
        fw, fh = (1 << cw, 1 << ch) if c in (1, 2) else (1, 1)
        g = []
        for k in range(3):
            f = x[:, k]
            gk = f[:, ::fh, ::fw]
            if mix.chroma == 1 and fw * fh > 1:
                for fy in range(fh):
                    for fx in range(fw):
                        if fy or fx:
                            gk = gk + f[:, fy::fh, fx::fw]
                gk = gk * (1.0 / (fw * fh))
            g.append(gk)
        a = g[0] * float(mix.m[c][0])
        a = a + g[1] * float(mix.m[c][1])
        a = a + g[2] * float(mix.m[c][2])
        u = a + float(mix.b[c])
        s = torch.round(u).clamp(0, peak)
        comps.append(s.to(torch.uint8) if size == 1 else s.to(torch.int32).to(torch.int16))
    if planar:
        return [c.contiguous() for c in comps]
    return [torch.stack(comps, -1).contiguous()]


def frames_of(planes, n, fmt):
    size = cm.LAYOUTS[fmt][5]
    arr = (m.Frame * n)()
    for i in range(n):
        for p, pl in enumerate(planes):
            rowbytes = pl[0][0].numel() * size
            arr[i].data[p] = pl.data_ptr() + i * pl.shape[1] * rowbytes
            arr[i].linesize[p] = rowbytes
        arr[i].width, arr[i].height, arr[i].pix_fmt = W, H, m.PIX_NAMES.index(fmt)
    return arr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--dtype", default="float16", choices=["float16", "float32", "bfloat16"])
    a = ap.parse_args()
    import torch
    n = a.frames
    dec, enc = m.Decoder(device_id=0), m.Encoder(0)
    copy_gbs = dec.copy_bench()
    res = {"metric": "htj2k_encode_tensor_mix", "frames": n, "size": [W, H], "device": dec.device_name(), "iters": a.iters, "dtype": a.dtype,
           "date": time.strftime("%Y-%m-%d"), "copy_gbs": round(copy_gbs, 1), "rows": {}}
    o = m._enc_opts()
    t = tb.images(torch, n, a.dtype, "NCHW")
    es = t.element_size()
    spec = m.tensor_spec(a.dtype, "NCHW")
    below = True
    for fmt, bits, how, chroma in ROWS:
        mix = the_mix(how, bits, chroma)
        cap = n * m.Encoder.bound(W, H, fmt, bits)
        out = [np.empty(cap, np.uint8) for _ in range(2)]
        offs = [(ctypes.c_size_t * (n + 1))() for _ in range(2)]
        torch.cuda.synchronize()

        def leg_a(k=0):
            t0 = time.perf_counter()
            r = enc.L.htj2k_encode_tensor_mix(enc.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * es), n, W, H,
                                              m.PIX_NAMES.index(fmt), bits, ctypes.byref(spec), ctypes.byref(mix), ctypes.byref(o),
                                              out[k].ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap), 0, offs[k])
            if r < 0:
                raise m.Htj2kError(r, "htj2k_encode_tensor_mix")
            return enc.stage_ms()[0], (time.perf_counter() - t0) * 1e3

        def leg_b(k=1):
            t0 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            planes = chain(torch, t, fmt, bits, mix)
            e1.record()
            torch.cuda.synchronize()
            enc.encode_into(frames_of(planes, n, fmt), n, bits, o, out[k].ctypes.data_as(ctypes.c_void_p), cap, offs[k], in_on_device=1)
            return e0.elapsed_time(e1), enc.stage_ms()[0], (time.perf_counter() - t0) * 1e3

        fr, keep = dec.from_tensor(t, fmt, bits, "NCHW", mix=mix)

        def leg_c(k=1):
            enc.encode_into(fr, n, bits, o, out[k].ctypes.data_as(ctypes.c_void_p), cap, offs[k], in_on_device=1)
            return enc.stage_ms()[0]

        def tensor_frame_ms():
            r = dec.L.htj2k_tensor_to_frames_mix(dec.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel() * es), n, bits,
                                                 ctypes.byref(spec), ctypes.byref(mix), fr)
            if r < 0:
                raise m.Htj2kError(r, "htj2k_tensor_to_frames_mix")
            return dec.compare_ms()

        def same():
            total = offs[0][n]
            return list(offs[0]) == list(offs[1]) and np.array_equal(out[0][:total], out[1][:total])

        # equal first, and the warm-up: the first calls allocate
        leg_a()
        leg_b()
        if not same():
            sys.exit("gpu_tensor_mix_encode_bench: %s %s: encode_tensor(mix=) differs from the encode of the chain's frames" % (fmt, chroma))
        leg_c()
        if not same():
            sys.exit("gpu_tensor_mix_encode_bench: %s %s: encode_tensor(mix=) differs from the encode of tensor_to_frames_mix's frames" % (fmt, chroma))
        total = offs[0][n]
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
        frame_bytes = sum(rows * rb for rows, rb in m.plane_geometry(m.PIX_NAMES.index(fmt), W, H))
        moved = n * (3 * W * H * es + frame_bytes)                 # what k_tensor_frame_mix has to read and write
        row = {"a_unpack_tensor_mix_ms": cb.spread(ta), "b_chain_ms": cb.spread(tb_chain), "b_unpack_ms": cb.spread(tb_unpack),
               "b_chain_plus_unpack_ms": cb.spread([x + y for x, y in zip(tb_chain, tb_unpack)]), "c_unpack_ms": cb.spread(tc),
               "k_tensor_frame_mix_ms": cb.spread(tk), "a_whole_call_ms": cb.spread(wa), "b_whole_call_ms": cb.spread(wb),
               "stream_bytes": int(total)}
        row["k_tensor_frame_mix_gbs"] = round(moved / (row["k_tensor_frame_mix_ms"]["median"] * 1e6), 1)
        row["k_tensor_frame_mix_over_copy"] = round(row["k_tensor_frame_mix_gbs"] / copy_gbs, 3)
        row["chain_plus_unpack_over_a"] = round(row["b_chain_plus_unpack_ms"]["median"] / row["a_unpack_tensor_mix_ms"]["median"], 2)
        row["a_below_b"] = row["a_unpack_tensor_mix_ms"]["median"] <= row["b_chain_plus_unpack_ms"]["median"]
        below = below and row["a_below_b"]
        name = "%s_%s_%s" % (fmt, how, chroma)
        res["rows"][name] = row
        print(name, json.dumps(row), flush=True)
        del fr, keep
        torch.cuda.empty_cache()
    res["a_below_b_everywhere"] = below
    print(json.dumps(res))
    enc.close()
    dec.close()


if __name__ == "__main__":
    main()
