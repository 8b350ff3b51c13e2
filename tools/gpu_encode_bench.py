"""Device-resident lossless encode rate of the HTJ2K encoder (htj2k_encode_batch with input and output in device
memory), one JSON line: Gpixel/s for C1 (1920x1080 rgb24), C2 (3840x2160 rgb24) and C4 (7680x4320 gray16 and rgb48)
at 1, 16 and 64 frames per call; the host->host rate of C2; bits per pixel; the stage split of the largest C2 call;
and the reference vector factory's single-core rate for scale.  Frames: vecgen.synth_image.

    python tools/gpu_encode_bench.py [--iters N] [--counts 1,16,64] [--cases C1,C2,C4g,C4] [--qstep Q] [--target-bpp B[,B..]]
                                      [--tile WxH] [--ht-passes N[,N..]] [--target-psnr P[,P..]] [--group-bpp B[,B..]]

--qstep Q encodes lossy (irreversible 9/7, base step Q) and adds, for the largest C2 call, the bytes per frame, the same
call's lossless stage split (the 5/3 forward on the same frames, same process), and the forward 9/7 + quantiser slot as
TB/s of the bytes it moves (from shapes) next to the copy ceiling of the device.

--tile WxH encodes every frame as a tile grid (0 in a direction: one tile spans the image there; 0x128 gives strips).

--target-bpp B adds, in the same process, the same calls under a byte budget of B * pixels / 8 per frame (rate
control): Gpixel/s, size and fill of the budget, the stage times with the two rate-control kernels and the correction
rounds, and the counters of htj2k_enc_rc_info summed over the frames of the largest call.

--ht-passes N[,N..] runs every budgeted call once per N (htj2k_enc_opts.ht_passes: the most passes a block may get) and
adds the times of k_ht_refine_plan + k_ht_refine_encode and of k_rc_stats_passes, the share of coded blocks per pass
count and, from a separate encoder with HTJ2K_ENC_STAMPS=1, where k_ht_refine_encode's cycles go in a 16-frame call under
the first budget.  Without the option the budgeted calls are the default ones.

--target-psnr P[,P..] adds, for the largest C2 call, the same call at constant quality (htj2k_enc_opts.target_psnr): bits
per pixel, the model's PSNR and the PSNR of the decoded first frame (measured on the device: Job.compare), Gpixel/s, the stage times with k_rc_base97 and the
quality select next to k_rc_stats and the HT launch, the HT launches taken (always 1), and the Gpixel/s of the budgeted
call whose target_bytes is the size the quality call came out at.

--group-bpp B[,B..] adds, for the largest C2 call, the same call under one budget over all its frames
(htj2k_enc_opts.group_bytes = B * pixels / 8 * frames): Gpixel/s, the fill of the group budget, the HT launches, the device
ms of the group kernels (htj2k_enc_group_stage_ms), the per-frame sizes and, for the same frames in the same process, the
call with that mean as every frame's own budget (target_bytes) with k_rc_select's ms.
"""
import argparse
import ctypes
import json
import os
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import enc_model as em  # noqa: E402
import ffmpeg_ht_amd as m  # noqa: E402
import vecgen  # noqa: E402

CASES = [("C1", "rgb24", 8, 1920, 1080), ("C2", "rgb24", 8, 3840, 2160), ("C4g", "gray16le", 16, 7680, 4320),
         ("C4", "rgb48le", 16, 7680, 4320)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--counts", default="1,16,64")
    ap.add_argument("--cases", default="C1,C2,C4g,C4")
    ap.add_argument("--qstep", type=float, default=None, help="lossy: irreversible 9/7 with this base step")
    ap.add_argument("--target-bpp", default="", help="also encode under a budget of B * pixels / 8 bytes per frame (comma list)")
    ap.add_argument("--tile", default="", help="WxH: nominal tile size (0: the image's in that direction)")
    ap.add_argument("--ht-passes", default="", help="budgeted calls: the most passes a block may get (comma list of 1 .. 3)")
    ap.add_argument("--target-psnr", default="", help="also encode at constant quality, dB (comma list)")
    ap.add_argument("--group-bpp", default="", help="also encode under one budget of B * pixels / 8 * frames bytes per call (comma list)")
    a = ap.parse_args()
    lossy = {} if a.qstep is None else dict(irreversible=True, qstep=a.qstep)
    tile = tuple(int(v) for v in a.tile.lower().split("x")) if a.tile else (0, 0)
    opts = dict(lossy, tile=tile)
    counts = [int(x) for x in a.counts.split(",")]
    import torch
    enc = m.Encoder(0)
    res = {"metric": "htj2k_lossy_encode" if lossy else "htj2k_lossless_encode", "device_resident_gpix_s": {}, "bpp": {},
           "stage_ms": {}}
    if lossy:
        res["qstep"] = a.qstep
    if a.tile:
        res["tile"] = list(tile)
    for name, fmt, bits, w, h in CASES:
        if name not in a.cases.split(","):
            continue
        comps = [vecgen.synth_image(w, h, 1, depth=bits, seed=c)[0] for c in range(em.layout(fmt)[0])]
        planes = em.to_planes(comps, fmt, bits)
        cs = enc.encode(planes, fmt, bits, **opts)
        res["bpp"][name] = round(8.0 * len(cs) / (w * h), 4)
        dev = torch.from_numpy(planes[0]).cuda()
        o = m._enc_opts(**opts)
        bound = m.Encoder.bound(w, h, fmt, bits, **opts)
        for n in counts:
            fr = m.Frame()
            fr.data[0] = dev.data_ptr()
            fr.linesize[0] = planes[0].strides[0]
            fr.width, fr.height, fr.pix_fmt = w, h, em.pix(fmt)
            arr = (m.Frame * n)(*([fr] * n))
            out = torch.empty(bound * n, dtype=torch.uint8, device="cuda")
            offs = (ctypes.c_size_t * (n + 1))()
            enc.encode_into(arr, n, bits, o, ctypes.c_void_p(out.data_ptr()), bound * n, offs, 1, 1)   # warm-up
            t = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                enc.encode_into(arr, n, bits, o, ctypes.c_void_p(out.data_ptr()), bound * n, offs, 1, 1)
                t.append(time.perf_counter() - t0)
            res["device_resident_gpix_s"]["%s_x%d" % (name, n)] = round(n * w * h / min(t) / 1e9, 3)
            if name == "C2" and n == max(counts):
                res["stage_ms"]["C2_x%d" % n] = [round(x, 3) for x in enc.stage_ms()]
                if lossy or a.tile:
                    res["bytes_per_frame_C2"] = int(offs[1] - offs[0])
                if lossy:
                    dwt_ms = enc.stage_ms()[1]
                    o53 = m._enc_opts(tile=tile)
                    enc.encode_into(arr, n, bits, o53, ctypes.c_void_p(out.data_ptr()), bound * n, offs, 1, 1)
                    res["stage_ms_lossless_same_frames"] = [round(x, 3) for x in enc.stage_ms()]
                    # per level: vertical reads + writes and horizontal reads + writes 4 bytes of each LL sample;
                    # the quantiser reads and writes 4 bytes of every sample
                    ns = 3 * w * h * n
                    moved = sum(16.0 * ns / 4 ** lv for lv in range(5)) + 8.0 * ns
                    res["fdwt97_quant_tb_s"] = round(moved / (dwt_ms * 1e-3) / 1e12, 3)
                    dec = m.Decoder(device_id=0)
                    res["copy_ceiling_tb_s"] = round(dec.copy_bench(512, 10) / 1e3, 3)
                    dec.close()
                for bpp, hp in [(float(x), int(k)) for x in a.target_bpp.split(",") if x for k in (a.ht_passes or "0").split(",")]:
                    target = int(bpp * w * h / 8)
                    ob = m._enc_opts(target_bytes=target, ht_passes=hp, **opts)
                    enc.encode_into(arr, n, bits, ob, ctypes.c_void_p(out.data_ptr()), bound * n, offs, 1, 1)   # warm-up
                    t = []
                    for _ in range(a.iters):
                        t0 = time.perf_counter()
                        enc.encode_into(arr, n, bits, ob, ctypes.c_void_p(out.data_ptr()), bound * n, offs, 1, 1)
                        t.append(time.perf_counter() - t0)
                    info = [enc.rc_info(i) for i in range(n)]
                    row = {
                        "gpix_s": round(n * w * h / min(t) / 1e9, 3), "target_bytes": target,
                        "bytes_per_frame": int(offs[1] - offs[0]), "fill": round((offs[1] - offs[0]) / target, 4),
                        "stage_ms": [round(x, 3) for x in enc.stage_ms()],
                        "rc_stage_ms_stats_select_recode": [round(x, 3) for x in enc.rc_stage_ms()],
                        "ht_launches_max": max(i["ht_launches"] for i in info),
                        "blocks": sum(i["nblocks"] for i in info), "blocks_recoded": sum(i["blocks_recoded"] for i in info),
                        "blocks_left_out": sum(i["blocks_left_out"] for i in info),
                        "trial_frames": sum(i["trial"] for i in info), "last_resort_frames": sum(i["last_resort"] for i in info)}
                    if a.ht_passes:
                        planes0, passes0 = enc.last_planes(0), enc.last_passes(0)
                        coded = [k for p, k in zip(planes0, passes0) if p >= 0]
                        row["ref_stage_ms_refine_stats"] = [round(x, 3) for x in enc.ref_stage_ms()]
                        row["share_of_coded_blocks_by_passes"] = [round(coded.count(k) / max(len(coded), 1), 4) for k in (1, 2, 3)]
                    key = "%s_x%d_bpp%g" % (name, n, bpp) + ("_passes%d" % hp if a.ht_passes else "")
                    res.setdefault("rate_control", {})[key] = row
                for psnr in [float(x) for x in a.target_psnr.split(",") if x]:
                    def timed(o2):
                        enc.encode_into(arr, n, bits, o2, ctypes.c_void_p(out.data_ptr()), bound * n, offs, 1, 1)   # warm-up
                        t = []
                        for _ in range(a.iters):
                            t0 = time.perf_counter()
                            enc.encode_into(arr, n, bits, o2, ctypes.c_void_p(out.data_ptr()), bound * n, offs, 1, 1)
                            t.append(time.perf_counter() - t0)
                        return round(n * w * h / min(t) / 1e9, 3)
                    gpix = timed(m._enc_opts(target_psnr=psnr, **opts))
                    size, q = int(offs[1] - offs[0]), enc.quality_info(0)
                    info = [enc.rc_info(i) for i in range(n)]
                    # the decoded PSNR is measured where the frames are: the job's planes against the device-resident input
                    # (htj2k_job_compare), nothing downloaded
                    dec = m.Decoder(device_id=0, req_pix_fmt=em.pix(fmt))
                    job = dec.job().parse_batch([out[:size].cpu().numpy().tobytes()]).upload().run()
                    diff, nerr = job.compare([fr], bits, on_device=True)[0], job.block_errors()
                    job.free()
                    dec.close()
                    row = {"gpix_s": gpix, "bytes_per_frame": size, "bpp": round(8.0 * size / (w * h), 4),
                           "model_psnr": round(q["model_psnr"], 3), "base_psnr": round(q["base_psnr"], 3),
                           "decoded_psnr": round(diff["psnr"], 3),
                           "short_of_target": q["short_of_target"], "stage_ms": [round(x, 3) for x in enc.stage_ms()],
                           "quality_stage_ms_base_select": [round(x, 3) for x in enc.quality_stage_ms()],
                           "rc_stage_ms_stats_select_recode": [round(x, 3) for x in enc.rc_stage_ms()],
                           "ht_launches_max": max(i["ht_launches"] for i in info), "block_errors": int(nerr)}
                    row["budget_call_same_size_gpix_s"] = timed(m._enc_opts(target_bytes=size, **opts))
                    row["budget_call_bytes_per_frame"] = int(offs[1] - offs[0])
                    res.setdefault("constant_quality", {})["%s_x%d_psnr%g" % (name, n, psnr)] = row
                for bpp in [float(x) for x in a.group_bpp.split(",") if x]:
                    def timed_call(o2):
                        enc.encode_into(arr, n, bits, o2, ctypes.c_void_p(out.data_ptr()), bound * n, offs, 1, 1)   # warm-up
                        t = []
                        for _ in range(a.iters):
                            t0 = time.perf_counter()
                            enc.encode_into(arr, n, bits, o2, ctypes.c_void_p(out.data_ptr()), bound * n, offs, 1, 1)
                            t.append(time.perf_counter() - t0)
                        return round(n * w * h / min(t) / 1e9, 3)
                    mean = int(bpp * w * h / 8)
                    gpix = timed_call(m._enc_opts(group_bytes=mean * n, **opts))
                    g = enc.group_info()
                    sizes = [int(offs[i + 1] - offs[i]) for i in range(n)]
                    row = {"gpix_s": gpix, "group_bytes": mean * n, "bytes": g["final_bytes"], "fill": round(g["final_bytes"] / (mean * n), 4),
                           "ht_launches": g["ht_launches"], "trial": g["trial"], "last_resort": g["last_resort"], "lambda": g["lambda"],
                           "blocks": g["nblocks"], "group_stage_ms": round(enc.group_stage_ms(), 3),
                           "stage_ms": [round(x, 3) for x in enc.stage_ms()],
                           "rc_stage_ms_stats_select_recode": [round(x, 3) for x in enc.rc_stage_ms()],
                           "frame_bytes_min_max": [min(sizes), max(sizes)], "frame_bytes": sizes[:8]}
                    row["per_frame_budget_gpix_s"] = timed_call(m._enc_opts(target_bytes=mean, **opts))
                    sizes = [int(offs[i + 1] - offs[i]) for i in range(n)]
                    row["per_frame_budget_bytes"] = sum(sizes)
                    row["per_frame_budget_frame_bytes_min_max"] = [min(sizes), max(sizes)]
                    row["per_frame_budget_rc_stage_ms_stats_select_recode"] = [round(x, 3) for x in enc.rc_stage_ms()]
                    res.setdefault("group_budget", {})["%s_x%d_bpp%g" % (name, n, bpp)] = row
            del out
        if name == "C2":
            t = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                enc.encode(planes, fmt, bits, **opts)
                t.append(time.perf_counter() - t0)
            res["host_to_host_C2_gpix_s"] = round(w * h / min(t) / 1e9, 4)
            t0 = time.perf_counter()
            vecgen.encode(comps, depth=8, nlevels=5, cb=(6, 6), mct=1, rsiz=0x4000, tile=tile,
                          **(dict(transform=0, qstep=a.qstep) if lossy else {}))
            res["vecgen_single_core_C2_gpix_s"] = round(w * h / (time.perf_counter() - t0) / 1e9, 5)
    enc.close()
    if "C2" in a.cases.split(","):
        # where the HT cleanup kernel's cycles go (clock64 stamps at its phase boundaries; a separate encoder, as the
        # stamps cost a little): one 16-frame C2 call
        os.environ["HTJ2K_ENC_STAMPS"] = "1"
        enc = m.Encoder(0)
        comps = [vecgen.synth_image(3840, 2160, 1, depth=8, seed=c)[0] for c in range(3)]
        planes = em.to_planes(comps, "rgb24", 8)
        enc.encode_batch([planes] * 16, "rgb24", 8, **opts)
        n, cyc = enc.ht_cycles()
        names = ["exponents_contexts", "magsgn_pack", "ff_pass", "mel_vlc", "copy_out"]
        res["ht_cycles_per_block_C2"] = {k: round(c / max(n, 1)) for k, c in zip(names, cyc)}
        res["ht_cycle_share_C2"] = {k: round(c / max(sum(cyc), 1), 4) for k, c in zip(names, cyc)}
        bpps = [float(x) for x in a.target_bpp.split(",") if x]
        for hp in [int(k) for k in a.ht_passes.split(",") if k and int(k) > 1 and bpps]:
            enc.encode_batch([planes] * 16, "rgb24", 8, target_bytes=int(bpps[0] * 3840 * 2160 / 8), ht_passes=hp, **opts)
            n, cyc = enc.ref_cycles()
            names = ["map", "membership", "sigprop_bits", "ff_pass", "magref_bits", "magref_bytes_copy_out"]
            res.setdefault("ref_cycles_per_block_C2", {})["passes%d" % hp] = dict(
                {k: round(c / max(n, 1)) for k, c in zip(names, cyc)}, blocks=n, ht_blocks=enc.ht_cycles()[0])
        enc.close()
        del os.environ["HTJ2K_ENC_STAMPS"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
