#!/usr/bin/env python3
"""Frame comparison on the device (htj2k_compare_frames, k_frame_diff): GB/s on device-resident frames beside the copy
ceiling of the same box, and what measuring costs an encode.

    python tools/gpu_compare_bench.py [--frames 64] [--iters 5] [--target-psnr 44]

For 64 device-resident C2-sized frames (3840 x 2160) of rgb24, rgb48le and yuv422p10le it prints the device ms of one
comparison launch (htj2k_compare_ms, best of --iters) and the GB/s of the bytes the kernel reads: both operands, once;
it writes nothing but 96 bytes of sums per pair.  htj2k_copy_bench runs in the same process: its figure counts bytes
read + written, so the two are the same kind of number, HBM traffic per second.  The operands differ in every
eighth byte; a second figure has them equal (no atomics at all), a third has planes that miss the 16-byte alignment by
one byte (the narrower path).

Then a 64-frame encode_measured call on C2 rgb24 (device input, device output): wall ms of encode_batch alone, of the
measured call in report-only mode, the difference (parse + decode + compare, the codestreams' trip to the host included)
as a share of the measured call, and with --target-psnr the closed loop's ms and rounds.

With --ssim the structural comparison instead (htj2k_compare_frames_ssim, k_frame_ssim): on the same frames, after a
warm-up, --iters repeats that alternate k_frame_ssim, k_frame_diff and the copy kernel, each figure as the median with
its spread (min .. max): device ms per launch and GB/s of operand bytes read; k_frame_diff reads exactly the same bytes,
so the ratio of the two is what the windows cost.  Beside the measured ratio stands the one that the kernel's re-reads
alone predict: (R + 1) / R for strips of R block rows times 64 / 63 for the group a wave shares with the next.  Then
a sweep of "ssim_rows", and what htj2k_enc_measure_ssim adds to the 64-frame measured encode.

One JSON line at the end.  There is no gate."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cmp_model as cm  # noqa: E402
import enc_model as em  # noqa: E402
import ffmpeg_ht_amd as m  # noqa: E402
import vecgen  # noqa: E402

W, H = 3840, 2160
LAYOUTS = [("rgb24", 8), ("rgb48le", 16), ("yuv422p10le", 10)]


def device_frames(torch, fmt, bits, n, rng, like=None, off=0):
    """(Frame * n) of device planes: one tensor per plane holds all n frames (random bytes; the frames repeat one slot);
    like: another set's tensors, copied with every eighth byte changed; off: every plane starts `off` bytes into its slot"""
    size = cm.LAYOUTS[fmt][5]
    tensors, arr = [], (m.Frame * n)()
    for p, (rows, cols) in enumerate(cm.plane_shapes(fmt, W, H)):
        slot = rows * cols * size + 64
        if like is None:
            t = torch.from_numpy(rng.integers(0, 256, size=slot, dtype=np.uint8)).cuda().repeat(n)
        else:
            t = like[p].clone()
            t[::8] ^= 0x55
        tensors.append(t)
        for i in range(n):
            arr[i].data[p] = t.data_ptr() + i * slot + off
            arr[i].linesize[p] = cols * size
    for i in range(n):
        arr[i].width, arr[i].height, arr[i].pix_fmt = W, H, m.PIX_NAMES.index(fmt)
    torch.cuda.synchronize()
    return arr, tensors


def best_ms(dec, a, b, n, bits, iters):
    out = (m.FrameDiff * n)()
    best = None
    for _ in range(iters + 1):                          # the first call allocates
        r = dec.L.htj2k_compare_frames(dec.h, a, 1, b, 1, n, bits, out)
        if r < 0:
            raise m.Htj2kError(r, "htj2k_compare_frames")
        ms = dec.compare_ms()
        best = ms if best is None else min(best, ms)
    return best, out


SSIM_ROWS_DEFAULT = 16                  # csrc/htj2k_device.hip
SSIM_SWEEP = (1, 2, 4, 8, 16, 32, 64, 128)


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def main_ssim(a):
    import torch
    n = a.frames
    dec, enc = m.Decoder(device_id=0), m.Encoder(0)
    rng = np.random.default_rng(1)
    res = {"metric": "htj2k_compare_frames_ssim", "frames": n, "size": [W, H], "device": dec.device_name(), "iters": a.iters,
           "layouts": {}}
    sout, dout = (m.FrameSsim * n)(), (m.FrameDiff * n)()

    def ssim_ms(fa, fb, bits):
        r = dec.L.htj2k_compare_frames_ssim(dec.h, fa, 1, fb, 1, n, bits, sout)
        if r < 0:
            raise m.Htj2kError(r, "htj2k_compare_frames_ssim")
        return dec.compare_ms()

    def diff_ms(fa, fb, bits):
        r = dec.L.htj2k_compare_frames(dec.h, fa, 1, fb, 1, n, bits, dout)
        if r < 0:
            raise m.Htj2kError(r, "htj2k_compare_frames")
        return dec.compare_ms()

    for fmt, bits in LAYOUTS:
        fa, ta = device_frames(torch, fmt, bits, n, rng)
        fb, tb = device_frames(torch, fmt, bits, n, rng, like=ta)
        nbytes = 2.0 * n * sum(r * c for r, c in cm.plane_shapes(fmt, W, H)) * cm.LAYOUTS[fmt][5]
        ssim_ms(fa, fb, bits), diff_ms(fa, fb, bits), dec.copy_bench(512, 2)          # warm-up: the first calls allocate
        t = {"ssim": [], "diff": [], "copy": []}
        for _ in range(a.iters):
            t["ssim"].append(ssim_ms(fa, fb, bits))
            t["diff"].append(diff_ms(fa, fb, bits))
            t["copy"].append(dec.copy_bench(512, 5))
        row = {"bytes_read": int(nbytes), "ssim_ms": spread(t["ssim"]), "diff_ms": spread(t["diff"]),
               "ssim_gb_s_read": spread([nbytes / x / 1e6 for x in t["ssim"]]),
               "diff_gb_s_read": spread([nbytes / x / 1e6 for x in t["diff"]]),
               "copy_gb_s_read_plus_written": spread(t["copy"]), "ssim_all_frame0": round(sout[0].all, 6)}
        row["ssim_over_diff_ms"] = round(row["ssim_ms"]["median"] / row["diff_ms"]["median"], 3)
        row["re_read_ratio_expected"] = round((SSIM_ROWS_DEFAULT + 1) / SSIM_ROWS_DEFAULT * 64 / 63, 3)
        sweep = {}
        for rows in SSIM_SWEEP:
            dec.set_int("ssim_rows", rows)
            ssim_ms(fa, fb, bits)
            sweep[rows] = spread([ssim_ms(fa, fb, bits) for _ in range(3)])["median"]
        dec.set_int("ssim_rows", 0)
        row["ssim_rows_sweep_ms"] = sweep
        res["layouts"][fmt] = row
        print(fmt, row, flush=True)
        del ta, tb
    # what the switch adds to a measured encode: 64 C2 rgb24 frames, device in, device out, report only
    fmt, bits = "rgb24", 8
    comps = [vecgen.synth_image(W, H, 1, depth=bits, seed=c)[0] for c in range(3)]
    planes = em.to_planes(comps, fmt, bits)
    dev = torch.from_numpy(planes[0]).cuda()
    fr = m.Frame()
    fr.data[0], fr.linesize[0] = dev.data_ptr(), planes[0].strides[0]
    fr.width, fr.height, fr.pix_fmt = W, H, em.pix(fmt)
    arr = (m.Frame * n)(*([fr] * n))
    bound = m.Encoder.bound(W, H, fmt, bits)
    out = torch.empty(bound * n, dtype=torch.uint8, device="cuda")
    offs = (ctypes.c_size_t * (n + 1))()
    info = (m.EncMeasured * n)()
    torch.cuda.synchronize()
    o, mo = m._enc_opts(target_psnr=a.target_psnr), m.EncMeasureOpts(0, 0)

    def measured(on):
        enc.L.htj2k_enc_measure_ssim(enc.h, on)
        t0 = time.perf_counter()
        r = enc.L.htj2k_encode_batch_measured(dec.h, enc.h, arr, n, bits, ctypes.byref(o), ctypes.byref(mo), 1,
                                              ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(bound * n), 1, offs, info)
        if r < 0:
            raise m.Htj2kError(r, "htj2k_encode_batch_measured")
        return (time.perf_counter() - t0) * 1e3

    measured(0), measured(1)
    t = {0: [], 1: []}
    for _ in range(max(a.iters // 2, 3)):
        for on in (0, 1):
            t[on].append(measured(on))
    s = m.FrameSsim()
    enc.L.htj2k_enc_last_ssim(enc.h, 0, ctypes.byref(s))
    res["encode_measured_C2_x%d_target_psnr_%g" % (n, a.target_psnr)] = {
        "switch_off_ms": spread(t[0]), "switch_on_ms": spread(t[1]),
        "added_ms": round(spread(t[1])["median"] - spread(t[0])["median"], 2), "ssim_kernel_ms": round(dec.compare_ms(), 3),
        "psnr_frame0": round(info[0].diff.psnr, 3), "ssim_all_frame0": round(s.all, 6)}
    print(json.dumps(res))
    enc.close()
    dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--target-psnr", type=float, default=44.0)
    ap.add_argument("--ssim", action="store_true", help="k_frame_ssim beside k_frame_diff and the copy kernel")
    a = ap.parse_args()
    if a.ssim:
        return main_ssim(a)
    import torch
    n = a.frames
    dec, enc = m.Decoder(device_id=0), m.Encoder(0)
    rng = np.random.default_rng(1)
    res = {"metric": "htj2k_compare_frames", "frames": n, "size": [W, H], "device": dec.device_name(),
           "copy_bench_gb_s_read_plus_written": round(dec.copy_bench(512, 10), 1), "compare": {}}
    for fmt, bits in LAYOUTS:
        fa, ta = device_frames(torch, fmt, bits, n, rng)
        fb, tb = device_frames(torch, fmt, bits, n, rng, like=ta)
        nbytes = 2.0 * n * sum(r * c for r, c in cm.plane_shapes(fmt, W, H)) * cm.LAYOUTS[fmt][5]
        ms, out = best_ms(dec, fa, fb, n, bits, a.iters)
        ms_eq, _ = best_ms(dec, fa, fa, n, bits, a.iters)
        fu, tu = device_frames(torch, fmt, bits, n, rng, like=ta, off=1)
        ms_un, _ = best_ms(dec, fu, fa, n, bits, max(a.iters // 2, 1))
        res["compare"][fmt] = {"bytes_read": int(nbytes), "ms": round(ms, 3), "gb_s_read": round(nbytes / ms / 1e6, 1),
                               "ms_equal_frames": round(ms_eq, 3), "gb_s_read_equal_frames": round(nbytes / ms_eq / 1e6, 1),
                               "ms_unaligned": round(ms_un, 3), "gb_s_read_unaligned": round(nbytes / ms_un / 1e6, 1),
                               "psnr_frame0": round(out[0].psnr, 3)}
        print(fmt, res["compare"][fmt], flush=True)
        del ta, tb, tu
    # what measuring costs an encode: 64 C2 rgb24 frames, device in, device out
    fmt, bits = "rgb24", 8
    comps = [vecgen.synth_image(W, H, 1, depth=bits, seed=c)[0] for c in range(3)]
    planes = em.to_planes(comps, fmt, bits)
    dev = torch.from_numpy(planes[0]).cuda()
    fr = m.Frame()
    fr.data[0], fr.linesize[0] = dev.data_ptr(), planes[0].strides[0]
    fr.width, fr.height, fr.pix_fmt = W, H, em.pix(fmt)
    arr = (m.Frame * n)(*([fr] * n))
    bound = m.Encoder.bound(W, H, fmt, bits)
    out = torch.empty(bound * n, dtype=torch.uint8, device="cuda")
    offs = (ctypes.c_size_t * (n + 1))()
    info = (m.EncMeasured * n)()
    torch.cuda.synchronize()

    def timed(fn):
        fn()
        t = []
        for _ in range(max(a.iters // 2, 2)):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return min(t) * 1e3

    def measured(o, mo):
        r = enc.L.htj2k_encode_batch_measured(dec.h, enc.h, arr, n, bits, ctypes.byref(o), ctypes.byref(mo), 1,
                                              ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(bound * n), 1, offs, info)
        if r < 0:
            raise m.Htj2kError(r, "htj2k_encode_batch_measured")

    row = {}
    for name, o in (("lossless", m._enc_opts()), ("target_psnr_%g" % a.target_psnr, m._enc_opts(target_psnr=a.target_psnr))):
        plain = timed(lambda: enc.encode_into(arr, n, bits, o, ctypes.c_void_p(out.data_ptr()), bound * n, offs, 1, 1))
        rep = timed(lambda: measured(o, m.EncMeasureOpts(0, 0)))
        row[name] = {"encode_batch_ms": round(plain, 2), "encode_measured_ms": round(rep, 2),
                     "decode_and_compare_ms": round(rep - plain, 2), "share_of_measured_call": round((rep - plain) / rep, 3),
                     "compare_kernel_ms": round(dec.compare_ms(), 3), "psnr_frame0": round(info[0].diff.psnr, 3)
                     if np.isfinite(info[0].diff.psnr) else "inf"}
        if "target" in name:
            loop = timed(lambda: measured(o, m.EncMeasureOpts(1, 0)))
            row[name].update(closed_loop_ms=round(loop, 2), rounds=int(info[0].rounds), final_psnr=round(info[0].diff.psnr, 3),
                             target_used=round(info[0].target_used, 3), fell_back=int(info[0].fell_back))
        print(name, row[name], flush=True)
    res["encode_measured_C2_x%d" % n] = row
    print(json.dumps(res))
    enc.close()
    dec.close()


if __name__ == "__main__":
    main()
