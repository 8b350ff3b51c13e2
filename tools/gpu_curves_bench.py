#!/usr/bin/env python3
"""The tensor calls with transfer curves (htj2k_frames_to_tensor_curves, k_frame_curves / k_frame_curves_any; the resized
call's scratch pass, k_tensor_curves): what a launch costs beside the matrix alone (htj2k_frames_to_tensor_mix) on the same
frames, beside the torch eager chain that makes the same tensor from the same device buffer, and beside the copy kernel of
the same box.

    python tools/gpu_curves_bench.py [--frames 64] [--iters 7]

For 64 device-resident 2048 x 1080 (DCI 2K) xyz12le frames and Decoder.dcp_curves(709, "srgb", 4097), to float16 NCHW,
after a warm-up, --iters rounds alternate in one process:
  (a) the library call with curves, on smooth frames (a diagonal gradient plus noise of a few codes: lanes of a wave look up
      neighbouring knots) and on uniformly random ones (every lookup of a wave somewhere else in the table)
  (b) the same call on the general route alone (tensor_path 1)
  (c) htj2k_frames_to_tensor_mix with the same matrix on the same frames: the launch without its LDS gathers
  (d) the torch eager chain a user writes today (curve_model.torch_chain: shift, gather, a multiply and an add kernel per
      term, clamp, index, lerp, convert), timed between two events on torch's stream.  Its tensor and the library's are
      compared with torch.equal before anything is timed
  (e) htj2k_copy_bench
  (f) whole frames resized to 224 x 224 with curves and with the matrix alone: what k_tensor_curves adds to k_tensor_mix
  (h) (a) under knob "curves_grid" = 1 .. 256: the source bytes a workgroup reads for every byte of tables it stages
  (i) (a) with one curve only, with a 256-knot out-table, and with the masks down to one component and one channel: the
      launch with half its gathers, with less LDS a workgroup, and with a sixth of its gathers under the full tables
  (g) yuv422p10le to linear-light RGB: the BT.709 matrix, then the BT.709 decode as an out-curve of 4097 knots, beside the
      matrix alone
Each figure is the median with its spread.  The library's time is the device time of its launches (htj2k_compare_ms).
GB/s is sample bytes read plus element bytes written per second; the copy kernel's figure counts the same two.

One JSON line at the end.  No figure is a pass mark: the exit status is 1 only where a tensor differs from the chain's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import cmp_model as cm  # noqa: E402
import curve_model as cvm  # noqa: E402
import ffmpeg_ht_amd as m  # noqa: E402
import mix_model as mm  # noqa: E402
from gpu_compare_bench import spread  # noqa: E402

W, H = 2048, 1080


def device_frames(torch, fmt, n, planes):
    """(Frame * n) of device planes from one frame's host planes (arrays of bytes or words): a tensor per plane holds the n
    frames one behind the other, every slot the same content at its own address"""
    tensors, arr = [], (m.Frame * n)()
    for p, a in enumerate(planes):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        slot = (raw.size + 63) // 64 * 64
        t = torch.from_numpy(np.pad(raw, (0, slot - raw.size))).cuda().repeat(n)
        tensors.append(t)
        for i in range(n):
            arr[i].data[p] = t.data_ptr() + i * slot
            arr[i].linesize[p] = a.shape[1] * a.itemsize
    for i in range(n):
        arr[i].width, arr[i].height, arr[i].pix_fmt = W, H, m.PIX_NAMES.index(fmt)
    return arr, tensors


def xyz_planes(rng, smooth):
    """one xyz12le frame: a diagonal gradient over the 4096 codes plus noise of +-8 codes, or uniformly random codes"""
    if smooth:
        y, x = np.mgrid[0:H, 0:W]
        base = ((x + y) * (4095.0 / (W + H - 2)))[..., None] + rng.integers(-8, 9, (H, W, 3))
        s = np.clip(base, 0, 4095).astype(np.uint16)
    else:
        s = rng.integers(0, 4096, (H, W, 3)).astype(np.uint16)
    return [(s << 4).reshape(H, W * 3)]


def chain_xyz(torch, t, n, mix, q, dtype):
    """the eager chain from the frames' bytes -> (n, 3, H, W) of dtype"""
    words = t.view(n, -1)[:, : H * W * 6].view(torch.int16).view(n, H, W, 3)
    s = ((words.to(torch.int32) >> 4) & 4095).permute(3, 0, 1, 2)
    _, mat, b = mm.unpack(mix)
    tin, tout = torch.from_numpy(q.tables[0]).cuda(), torch.from_numpy(q.tables[1]).cuda()
    v = cvm.torch_chain(s, tin, mat[:3], b, tout, float(q.out.x0), float(q.out.inv_dx), list(q.gain), list(q.offset))
    return v.permute(1, 0, 2, 3).to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=7)
    a = ap.parse_args()
    import torch
    n = a.frames
    dec = m.Decoder(device_id=0)
    rng = np.random.default_rng(1)
    res = {"metric": "htj2k_frames_to_tensor_curves", "frames": n, "size": [W, H], "device": dec.device_name(), "iters": a.iters,
           "date": time.strftime("%Y-%m-%d"), "rows": {}}
    mix, q = m.Decoder.dcp_curves(709, "srgb", 4097)
    out = torch.empty((n, 3, H, W), dtype=torch.float16, device="cuda")
    same = True

    def timed(call):
        call()
        return dec.compare_ms(), dec.tensor_last_route()

    for name, smooth in (("xyz12le_dcp_srgb_f16_smooth", True), ("xyz12le_dcp_srgb_f16_random", False)):
        fa, ta = device_frames(torch, "xyz12le", n, xyz_planes(rng, smooth))

        def lib(path=0):
            dec.set_int("tensor_path", path)
            try:
                return timed(lambda: dec.to_tensor(fa, "xyz12le", 12, "float16", "NCHW", on_device=True, out=out, mix=mix, curves=q))
            finally:
                dec.set_int("tensor_path", 0)

        def chain_ms():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            x = chain_xyz(torch, ta[0], n, mix, q, torch.float16)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), x

        _, route = lib()                                     # equal first, and the warm-up: the first calls allocate
        _, x = chain_ms()
        for path in (0, 1):
            out.zero_()
            lib(path)
            if not torch.equal(x.view(torch.int16), out.view(torch.int16)):
                same = False
                print("gpu_curves_bench: %s differs from the torch chain (tensor_path %d)" % (name, path), file=sys.stderr)
        del x
        timed(lambda: dec.to_tensor(fa, "xyz12le", 12, "float16", "NCHW", on_device=True, out=out, mix=mix))
        dec.copy_bench(512, 2)
        t = {"lib": [], "general": [], "mix": [], "torch": [], "copy": []}
        for _ in range(a.iters):
            t["lib"].append(lib()[0])
            t["general"].append(lib(1)[0])
            t["mix"].append(timed(lambda: dec.to_tensor(fa, "xyz12le", 12, "float16", "NCHW", on_device=True, out=out, mix=mix))[0])
            t["torch"].append(chain_ms()[0])
            t["copy"].append(dec.copy_bench(512, 5))
        moved = float(n * H * W * 6 + n * 3 * H * W * 2)
        s = {k: spread(v) for k, v in t.items()}
        gbs = lambda ms: round(moved / ms / 1e6, 1)
        res["rows"][name] = {"route": route, "ms": s["lib"], "general_route_ms": s["general"], "mix_alone_ms": s["mix"], "torch_chain_ms": s["torch"],
                             "copy_gb_s_read_plus_written": s["copy"], "gb_s_read_plus_written": gbs(s["lib"]["median"]),
                             "share_of_copy_rate": round(gbs(s["lib"]["median"]) / s["copy"]["median"], 3),
                             "general_share_of_copy_rate": round(gbs(s["general"]["median"]) / s["copy"]["median"], 3),
                             "mix_alone_share_of_copy_rate": round(gbs(s["mix"]["median"]) / s["copy"]["median"], 3),
                             "curves_over_mix_alone": round(s["lib"]["median"] / s["mix"]["median"], 3),
                             "torch_over_lib": round(s["torch"]["median"] / s["lib"]["median"], 2)}
        print(name, json.dumps(res["rows"][name]), flush=True)
        # (h), (i): the grid's factor under knob "curves_grid", and the launch with fewer gathers and smaller tables
        sweep = {}
        for factor in (1, 2, 4, 8, 16, 64, 256):
            dec.set_int("curves_grid", factor)
            try:
                sweep[str(factor)] = spread([lib()[0] for _ in range(a.iters + 1)][1:])["median"]
            finally:
                dec.set_int("curves_grid", 0)
        res["rows"][name]["ms_by_curves_grid"] = sweep
        t_in, t_out = q.tables
        small_out = m.tensor_curve(m.curve_table("srgb_encode", 256), 0.0, 255.0)
        coded = m.tensor_mix(mm.unpack(mix)[1][:3, :3] / 4095.0)           # without an in-curve: t spread over 0 .. 1 all the same
        variants = {"in_curve_only_4096": (mix, m.tensor_curves(m.tensor_curve(t_in), None)),
                    "out_curve_only_4097": (coded, m.tensor_curves(None, m.tensor_curve(t_out, 0.0, 4096.0))),
                    "out_curve_only_256": (coded, m.tensor_curves(None, small_out)),
                    "both_4096_256": (mix, m.tensor_curves(m.tensor_curve(t_in), small_out)),
                    "one_channel_each_4096_4097": (mix, m.tensor_curves(m.tensor_curve(t_in), m.tensor_curve(t_out, 0.0, 4096.0), 1, 1))}
        res["rows"][name]["ms_by_curves"] = {
            k: spread([timed(lambda: dec.to_tensor(fa, "xyz12le", 12, "float16", "NCHW", on_device=True, out=out, mix=vm, curves=vq))[0]
                       for _ in range(a.iters + 1)][1:])["median"] for k, (vm, vq) in variants.items()}
        print(name, "sweeps", json.dumps({"grid": sweep, "curves": res["rows"][name]["ms_by_curves"]}), flush=True)
        if not smooth:                                       # (f) on the random frames
            small = torch.empty((n, 3, 224, 224), dtype=torch.float16, device="cuda")
            r = {"curves": [], "mix": []}
            for it in range(a.iters + 1):
                ms_q, route = timed(lambda: dec.to_tensor_resized(fa, "xyz12le", 12, (224, 224), None, "triangle", "float16", "NCHW", on_device=True,
                                                                  out=small, mix=mix, curves=q))
                ms_m, _ = timed(lambda: dec.to_tensor_resized(fa, "xyz12le", 12, (224, 224), None, "triangle", "float16", "NCHW", on_device=True,
                                                              out=small, mix=mix))
                if it:                                       # the first round allocates
                    r["curves"].append(ms_q)
                    r["mix"].append(ms_m)
            res["resized_224_xyz12le_f16"] = {"route": route, "curves_ms": spread(r["curves"]), "mix_ms": spread(r["mix"]),
                                              "curves_over_mix": round(spread(r["curves"])["median"] / spread(r["mix"])["median"], 3)}
            print("resized", json.dumps(res["resized_224_xyz12le_f16"]), flush=True)
        del fa, ta
        torch.cuda.empty_cache()
    # (g) yuv422p10le to linear-light RGB, out-curve only
    planes = [rng.integers(64, 941, (rows, cols)).astype(np.uint16) for rows, cols in cm.plane_shapes("yuv422p10le", W, H)]
    fa, ta = device_frames(torch, "yuv422p10le", n, planes)
    ymix = m.Decoder.ycbcr_mix(709, 10)
    lin = m.tensor_curves(None, m.tensor_curve(m.curve_table("bt709_decode", 4097), 0.0, 4096.0))
    t = {"curves": [], "mix": []}
    for it in range(a.iters + 1):
        ms_q, route = timed(lambda: dec.to_tensor(fa, "yuv422p10le", 10, "float16", "NCHW", on_device=True, out=out, mix=ymix, curves=lin))
        ms_m, _ = timed(lambda: dec.to_tensor(fa, "yuv422p10le", 10, "float16", "NCHW", on_device=True, out=out, mix=ymix))
        if it:
            t["curves"].append(ms_q)
            t["mix"].append(ms_m)
    moved = float(n * H * W * 2 * 2 + n * 3 * H * W * 2)
    res["yuv422p10le_linear_rgb_f16"] = {"route": route, "ms": spread(t["curves"]), "mix_alone_ms": spread(t["mix"]),
                                         "gb_s_read_plus_written": round(moved / spread(t["curves"])["median"] / 1e6, 1),
                                         "curves_over_mix_alone": round(spread(t["curves"])["median"] / spread(t["mix"])["median"], 3)}
    res["equal_to_the_torch_chain"] = same
    print(json.dumps(res))
    dec.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
