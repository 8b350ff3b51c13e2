#!/usr/bin/env python3
"""Frame checksums on the device (htj2k_hash_frames, k_frame_adler): what a launch costs beside k_frame_diff and the
copy kernel of the same box, and what a pipe delivers when frames come back as checksums.

    python tools/gpu_hash_bench.py [--frames 64] [--iters 9] [--pipe-frames 240] [--window 1.0]

Kernel legs.  For 64 device-resident C2-sized frames (3840 x 2160) of rgb24, rgb48le and yuv422p10le, after a warm-up,
--iters rounds that alternate four launches in one process: k_frame_adler over the frames, k_frame_diff of the same
frames against themselves (the same launch shape; every byte asked for twice, the second time out of the caches), k_frame_diff
against a copy of them that differs in every eighth byte (two operands from memory), and htj2k_copy_bench.  Each figure is
the median of the device ms (htj2k_compare_ms: device events around the launches) with its spread, and GB/s of operand
bytes read; the copy kernel's figure counts bytes read + written, so all are HBM traffic per second.

Pipe legs.  --pipe-frames distinct 4K rgb24 frames (bench.py's generator), sent by reference through a pipe of 8 x 3,
received as checksums (htj2k_pipe_receive_hash), as frames in page-locked host memory (htj2k_pipe_receive) and as device
pointers (htj2k_pipe_receive_device): Gpixel/s over a window of at least --window seconds that starts after 48 warm-up
frames, the three legs alternating, twice.  The first checksums are compared with zlib over the source pictures.

One JSON line at the end.  There is no gate."""
import argparse
import concurrent.futures
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import cmp_model as cm  # noqa: E402
import ffmpeg_ht_amd as m  # noqa: E402
import gpu_compare_bench as cb  # noqa: E402
import vecgen  # noqa: E402

W, H = cb.W, cb.H


def kernel_legs(dec, torch, n, iters):
    rng = np.random.default_rng(1)
    hout, dout = (m.FrameHash * n)(), (m.FrameDiff * n)()

    def hash_ms(fa):
        r = dec.L.htj2k_hash_frames(dec.h, fa, 1, n, hout)
        if r < 0:
            raise m.Htj2kError(r, "htj2k_hash_frames")
        return dec.compare_ms()

    def diff_ms(fa, fb, bits):
        r = dec.L.htj2k_compare_frames(dec.h, fa, 1, fb, 1, n, bits, dout)
        if r < 0:
            raise m.Htj2kError(r, "htj2k_compare_frames")
        return dec.compare_ms()

    rows = {}
    for fmt, bits in cb.LAYOUTS:
        fa, ta = cb.device_frames(torch, fmt, bits, n, rng)
        fb, tb = cb.device_frames(torch, fmt, bits, n, rng, like=ta)
        nbytes = float(n * sum(r * c for r, c in cm.plane_shapes(fmt, W, H)) * cm.LAYOUTS[fmt][5])
        hash_ms(fa), diff_ms(fa, fa, bits), diff_ms(fa, fb, bits), dec.copy_bench(512, 2)      # warm-up: the first calls allocate
        t = {"adler": [], "diff_self": [], "diff_pair": [], "copy": []}
        for _ in range(iters):
            t["adler"].append(hash_ms(fa))
            t["diff_self"].append(diff_ms(fa, fa, bits))
            t["diff_pair"].append(diff_ms(fa, fb, bits))
            t["copy"].append(dec.copy_bench(512, 5))
        # the frames repeat one slot of random bytes: every frame's checksum is that of frame 0, computed on the host
        host = [np.asarray(x[: rws * cols * cm.LAYOUTS[fmt][5]].cpu()) for x, (rws, cols) in zip(ta, cm.plane_shapes(fmt, W, H))]
        want = 0
        for p in host:
            want = zlib.adler32(p.tobytes(), want)
        if any(hout[i].adler32 != want & 0xFFFFFFFF for i in range(n)):
            sys.exit("gpu_hash_bench: %s checksums differ from zlib's" % fmt)
        row = {"bytes_hashed": int(nbytes), "adler_ms": cb.spread(t["adler"]), "diff_self_ms": cb.spread(t["diff_self"]),
               "diff_pair_ms": cb.spread(t["diff_pair"]),
               "adler_gb_s_read": cb.spread([nbytes / x / 1e6 for x in t["adler"]]),
               "diff_self_gb_s_asked": cb.spread([2 * nbytes / x / 1e6 for x in t["diff_self"]]),
               "diff_pair_gb_s_read": cb.spread([2 * nbytes / x / 1e6 for x in t["diff_pair"]]),
               "copy_gb_s_read_plus_written": cb.spread(t["copy"])}
        row["adler_over_diff_self_ms"] = round(row["adler_ms"]["median"] / row["diff_self_ms"]["median"], 3)
        row["adler_over_diff_pair_ms"] = round(row["adler_ms"]["median"] / row["diff_pair_ms"]["median"], 3)
        row["adler_read_over_copy_rate"] = round(row["adler_gb_s_read"]["median"] / row["copy_gb_s_read_plus_written"]["median"], 3)
        rows[fmt] = row
        print(fmt, row, flush=True)
        del ta, tb
        torch.cuda.empty_cache()
    return rows


def make_packets(nframes):
    """distinct synthetic 4K rgb24 frames as bench.py makes them -> (packets, zlib's checksum of frame 0 and 1)"""
    def make(i):
        img = vecgen.synth_image(W, H, 3, depth=8, seed=2 + i, noise=8)
        crc = zlib.adler32(np.stack(img, -1).astype(np.uint8).tobytes(), 0) & 0xFFFFFFFF if i < 2 else None
        if i % 40 == 0:
            print("making frame", i, flush=True)
        return vecgen.encode(img, mct=1, nlevels=5, cb=(6, 6), transform=1), crc
    made = [make(0)]
    with concurrent.futures.ThreadPoolExecutor(16) as ex:
        made += list(ex.map(make, range(1, nframes)))
    return [m.packet(d) for d, _ in made], [c for _, c in made[:2]]


def pipe_leg(dec, pkts, receive, window, nwarm=48):
    """Gpixel/s of a pipe that cycles through the packets: the clock starts after nwarm frames and stops once at least
    len(pkts) frames and `window` seconds have passed"""
    pipe = dec.pipe(batch=8, depth=3)
    sent = got = 0
    t0 = None
    first = []
    while True:
        while pipe.send(pkts[sent % len(pkts)]):
            sent += 1
        r = receive(pipe)
        if r is None:
            sys.exit("gpu_hash_bench: the pipe ran dry")
        if got < 2:
            first.append(r)
        got += 1
        if got == nwarm:
            t0 = time.perf_counter()
        elif got > nwarm:
            dt = time.perf_counter() - t0
            if got - nwarm >= len(pkts) and dt >= window:
                break
    pipe.close()
    return (got - nwarm) * W * H / dt / 1e9, got - nwarm, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--pipe-frames", type=int, default=240)
    ap.add_argument("--window", type=float, default=1.0, help="seconds a pipe leg's clock runs at least")
    a = ap.parse_args()
    import torch
    dec = m.Decoder(device_id=0)
    res = {"metric": "htj2k_hash_frames", "frames": a.frames, "size": [W, H], "device": dec.device_name(), "iters": a.iters,
           "date": time.strftime("%Y-%m-%d"), "layouts": kernel_legs(dec, torch, a.frames, a.iters)}
    if a.pipe_frames > 0:
        t0 = time.perf_counter()
        pkts, crcs = make_packets(a.pipe_frames)
        print("made %d packets in %.1f s" % (len(pkts), time.perf_counter() - t0), flush=True)
        info0 = dec.probe(bytes(pkts[0][0][:pkts[0][1]]))
        pinned, ptrs = dec.alloc_frame_pinned(info0)
        legs = {"receive_hash": lambda p: p.receive_crc(), "receive": lambda p: p.receive(into=pinned),
                "receive_device": lambda p: p.receive_device()}
        rates = {k: [] for k in legs}
        for _ in range(2):
            for name, fn in legs.items():
                rate, nfr, first = pipe_leg(dec, pkts, fn, a.window)
                rates[name].append(round(rate, 2))
                if name == "receive_hash" and [h["adler32"] for _, h in first] != crcs:
                    sys.exit("gpu_hash_bench: the pipe's checksums differ from zlib's over the sources")
                print(name, round(rate, 2), "Gpixel/s over", nfr, "frames", flush=True)
        dec.free_frame_pinned(ptrs)
        res["pipe_4k_rgb24_x%d_gpixel_s" % a.pipe_frames] = rates
    print(json.dumps(res))
    dec.close()


if __name__ == "__main__":
    main()
