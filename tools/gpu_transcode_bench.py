"""Rate of the transcoder (htj2k_transcode_batch, output in device memory), one JSON line: Gpixel/s for Part-1 sources
C1 (1920x1080 rgb24) and C2 (3840x2160 rgb24) from the vector factory, lossless 5/3 and 9/7, at 1 and 16 frames per
call, best of --iters; next to two references measured in the same process on the same frames:

  stage_sum   the Part-1 block stage alone (htj2k_job_stage_ms of a job run with mask 1) plus the encoder's HT and
              gather stages alone (htj2k_enc_stage_ms of the frames' encode): what a transcode call should cost
  decode_then_encode   the full decode to pixels in device memory followed by htj2k_encode_batch from there: what a user
              had to do before

and how fast the transcoded stream decodes against its source (whole frames to pixels, the same job calls).

--target-bpp a,b adds, for each budget of so many bits per pixel and frame (htj2k_transcode_batch_opts), the fill (bytes
written over the budget, worst frame), the HT launches, the call's time and the device ms the budget adds to the
unbudgeted call: both statistics kernels with k_xc_limit, the selections, the correction launches.

--ht-sources builds the sources as HT streams instead (htj2k_transcode_opts.ht_sources): lossless 5/3 with one pass per
block ("ht1") and 9/7 with three ("ht3").

    python tools/gpu_transcode_bench.py [--iters N] [--counts 1,16] [--cases C1,C2] [--qstep Q] [--drop-passes D]
                                        [--target-bpp a,b] [--ht-sources]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ffmpeg_ht_amd as m  # noqa: E402
import vecgen  # noqa: E402

CASES = [("C1", 1920, 1080), ("C2", 3840, 2160)]


def best(fn, iters):
    fn()                                                  # warm-up: buffers grow, code objects load
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--counts", default="1,16")
    ap.add_argument("--cases", default="C1,C2")
    ap.add_argument("--qstep", type=float, default=1.0, help="base step of the 9/7 sources")
    ap.add_argument("--drop-passes", type=int, default=0, help="passes cut off every block of the 9/7 sources")
    ap.add_argument("--target-bpp", default="", help="budgets in bits per pixel, comma separated")
    ap.add_argument("--ht-sources", action="store_true", help="HT sources: one pass (5/3) and three passes (9/7)")
    a = ap.parse_args()
    hs = a.ht_sources
    bpps = [float(x) for x in a.target_bpp.split(",") if x]
    import torch
    dec, enc = m.Decoder(device_id=0), m.Encoder(0)
    res = {"metric": "htj2k_transcode", "ht_sources": int(hs), "gpix_s": {}, "stage_ms": {}, "bytes_per_frame": {}, "budget": {}}
    for name, w, h in CASES:
        if name not in a.cases.split(","):
            continue
        comps = [vecgen.synth_image(w, h, 1, seed=c)[0] for c in range(3)]
        kinds = ((("ht1", dict(transform=1, passes=1), dict()),
                  ("ht3", dict(transform=0, qstep=a.qstep, passes=3), dict(irreversible=True, qstep=a.qstep))) if hs else
                 (("53", dict(transform=1), dict()),
                  ("97", dict(transform=0, qstep=a.qstep, drop_passes=a.drop_passes), dict(irreversible=True, qstep=a.qstep))))
        for kind, kw, eo in kinds:
            src = vecgen.encode(comps, part1=not hs, mct=1, nlevels=5, cb=(6, 6), **kw)
            bound = m.Encoder.transcode_check(src, ht_sources=hs)
            pk = m.packet(src)
            for n in [int(x) for x in a.counts.split(",")]:
                key = "%s_%s_x%d" % (name, kind, n)
                ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(pk[0], ctypes.c_void_p)] * n)
                sizes = (ctypes.c_int * n)(*[pk[1]] * n)
                out = torch.empty(bound * n, dtype=torch.uint8, device="cuda")
                offs = (ctypes.c_size_t * (n + 1))()
                dst = ctypes.c_void_p(out.data_ptr())
                t_xc = best(lambda: enc.transcode_into(dec, ptrs, sizes, n, dst, bound * n, offs, 1, ht_sources=hs), a.iters)
                xc_ms = enc.transcode_stage_ms()
                ht = out[:offs[1]].cpu().numpy().tobytes()
                for bpp in bpps:
                    target = max(int(bpp * w * h / 8), m.Encoder.transcode_min_size(pk, ht_sources=hs))
                    t_b = best(lambda: enc.transcode_into(dec, ptrs, sizes, n, dst, bound * n, offs, 1, target_bytes=target, ht_sources=hs), a.iters)
                    info = [enc.rc_info(f) for f in range(n)]
                    rc_ms, ref_ms = enc.rc_stage_ms(), enc.ref_stage_ms()
                    res["budget"]["%s_bpp%g" % (key, bpp)] = {
                        "target_bytes": target, "fill": round(min(i["final_bytes"] for i in info) / target, 4),
                        "ht_launches": max(i["ht_launches"] for i in info), "last_resort": max(i["last_resort"] for i in info),
                        "blocks_recoded": sum(i["blocks_recoded"] for i in info), "call_ms": round(t_b * 1e3, 3),
                        "unbudgeted_call_ms": round(t_xc * 1e3, 3),
                        "extra_device_ms_stats_passes_select_recode": [round(x, 3) for x in (rc_ms[0], ref_ms[1], rc_ms[1], rc_ms[2])]}
                # reference 1: the stages alone
                job = dec.job()
                job.parse_batch([pk] * n).upload().run(1).wait()
                p1_ms = job.stage_ms()[0]
                # reference 2: decode to pixels on the device, encode from there
                fr = (m.Frame * n)()
                o = m._enc_opts(levels=5, cb=(6, 6), mct=1, **eo)
                ebound = m.Encoder.bound(w, h, "rgb24", 8, levels=5, cb=(6, 6), mct=1, **eo)
                eout = torch.empty(ebound * n, dtype=torch.uint8, device="cuda")

                def decode_then_encode():
                    job.parse_batch([pk] * n).upload().run().wait()
                    for f in range(n):
                        m._check(dec.L.htj2k_job_device_frame(dec.h, job.h, f, ctypes.byref(fr[f])), "htj2k_job_device_frame")
                    enc.encode_into(fr, n, 8, o, ctypes.c_void_p(eout.data_ptr()), ebound * n, offs, 1, 1)
                t_de = best(decode_then_encode, a.iters)
                enc_ms = enc.stage_ms()
                # how fast each stream decodes (parse, upload, all stages)
                t_src = best(lambda: job.parse_batch([pk] * n).upload().run().wait(), a.iters)
                hk = m.packet(ht)
                t_ht = best(lambda: job.parse_batch([hk] * n).upload().run().wait(), a.iters)
                job.free()
                px = n * w * h
                res["gpix_s"][key] = {"transcode": round(px / t_xc / 1e9, 3), "decode_then_encode": round(px / t_de / 1e9, 3),
                                      "decode_source": round(px / t_src / 1e9, 3), "decode_transcoded": round(px / t_ht / 1e9, 3)}
                res["stage_ms"][key] = {"transcode_p1_scatter_ht_gather": [round(x, 3) for x in xc_ms], "transcode_call": round(t_xc * 1e3, 3),
                                        "stage_sum_p1_plus_enc_ht_gather": round(p1_ms + enc_ms[2] + enc_ms[3], 3),
                                        "p1_stage_alone": round(p1_ms, 3), "enc_unpack_dwt_ht_gather": [round(x, 3) for x in enc_ms]}
                res["bytes_per_frame"][key] = {"source": len(src), "htj2k": len(ht)} if hs else {"part1": len(src), "htj2k": len(ht)}
                del out, eout
    enc.close()
    dec.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
