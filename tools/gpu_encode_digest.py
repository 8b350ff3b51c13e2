"""What the encoder's selection modes write for a fixed, seeded matrix of small calls, as digests: one JSON line per case,
to compare two builds of the library byte for byte (run it from each tree and compare the outputs).

    python tools/gpu_encode_digest.py [OUTFILE]

A case is one call of 4 frames (hand-built, padded rows: tests/enc_frames.py).  The matrix: 160 x 96 and 75 x 41; rgb24 at
8 bits and gray16le at 12; 5/3 and 9/7 (qstep 0.25), 3 levels; one tile and tile=(64, 48); ht_passes 1 and 3; and the modes
none, target_bytes at 50 % and 10 % of the unconstrained mean size and at the smallest stream + 40 bytes, target_psnr 35
alone and under a cap of 25 %, group_bytes at 50 % and 10 % of the unconstrained sum, alone and with per-frame caps of 30 %.
The frames are small on purpose: tight budgets on few blocks are where the correction launches and the last resort happen.

A line holds the sha256 of the concatenated streams, the offsets, sha256 of last_planes and last_passes of all frames, and
every field of rc_info, quality_info and group_info.  The last line counts the cases that reported blocks coded again
and the last resort, so that the reader knows which paths a comparison covered, and holds the sha256 of all lines above
it: two outputs are identical when their last lines are.  (An output is half a megabyte; profiles/ keeps the last lines.)"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import enc_frames as ef  # noqa: E402
import enc_model as em  # noqa: E402
import ffmpeg_ht_amd as m  # noqa: E402
import vecgen  # noqa: E402

NFRAMES = 4


def sha(ints):
    return hashlib.sha256(",".join(str(v) for v in ints).encode()).hexdigest()


def modes(mean, total, smallest):
    yield "none", {}
    for name, t in (("tb50", mean // 2), ("tb10", mean // 10), ("tbmin40", smallest + 40)):
        yield name, dict(target_bytes=t)
    yield "psnr35", dict(target_psnr=35.0)
    yield "psnr35_cap25", dict(target_psnr=35.0, target_bytes=mean // 4)
    for pct in (50, 10):
        g = max(total * pct // 100, NFRAMES * smallest)
        yield "gb%d" % pct, dict(group_bytes=g)
        yield "gb%d_cap30" % pct, dict(group_bytes=g, target_bytes=max(mean * 3 // 10, smallest))


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    lines = hashlib.sha256()

    def emit(row):
        text = json.dumps(row, sort_keys=True)
        lines.update(text.encode() + b"\n")
        print(text, file=out)

    enc = m.Encoder(0)
    count = {"cases": 0, "refused": 0, "blocks_recoded": 0, "last_resort": 0, "group_last_resort": 0, "blocks_left_out": 0}
    for w, h in ((160, 96), (75, 41)):
        for fmt, bits in (("rgb24", 8), ("gray16le", 12)):
            frames, keep = [], []
            for i in range(NFRAMES):
                comps = [vecgen.synth_image(cw, ch, 1, depth=bits, seed=17 * i + c)[0]
                         for c, (cw, ch) in enumerate(em.comp_dims(fmt, w, h))]
                fr, arrays = ef.padded_frame(em.to_planes(comps, fmt, bits), fmt, w, h, [5 + i])
                frames.append(fr)
                keep.append(arrays)
            for wavelet in (dict(), dict(irreversible=True, qstep=0.25)):
                for tile in ((0, 0), (64, 48)):
                    base = dict(wavelet, levels=3, tile=tile)
                    free = [len(cs) for cs in ef.encode_frames(enc, frames, fmt, bits, **base)]
                    nblk = len(m.Encoder.layout(w, h, fmt, bits, **base))
                    smallest = len(m.Encoder.assemble(w, h, fmt, bits, [b""] * nblk, **base))
                    for hp in (1, 3):
                        for name, mode in modes(sum(free) // NFRAMES, sum(free), smallest):
                            row = {"case": "%dx%d_%s_%s_tile%dx%d_passes%d_%s" % (w, h, fmt, "97" if wavelet else "53", tile[0],
                                                                                tile[1], hp, name), "opts": mode}
                            count["cases"] += 1
                            try:
                                cs = ef.encode_frames(enc, frames, fmt, bits, ht_passes=hp, **dict(base, **mode))
                            except m.Htj2kError as e:
                                row["refused"] = e.code
                                count["refused"] += 1
                                emit(row)
                                continue
                            rc = [enc.rc_info(i) for i in range(NFRAMES)]
                            row.update(
                                sha256=hashlib.sha256(b"".join(cs)).hexdigest(),
                                offsets=[sum(len(c) for c in cs[:i]) for i in range(NFRAMES + 1)],
                                last_planes=sha([p for i in range(NFRAMES) for p in enc.last_planes(i)]),
                                last_passes=sha([p for i in range(NFRAMES) for p in enc.last_passes(i)]),
                                rc_info=rc, quality_info=[enc.quality_info(i) for i in range(NFRAMES)],
                                group_info=enc.group_info())
                            count["blocks_recoded"] += any(r["blocks_recoded"] > 0 for r in rc)
                            count["last_resort"] += any(r["last_resort"] for r in rc)
                            count["blocks_left_out"] += any(r["blocks_left_out"] > 0 for r in rc)
                            count["group_last_resort"] += row["group_info"]["last_resort"] != 0
                            emit(row)
    print(json.dumps({"cases_that_reported": count, "sha256_of_the_lines_above": lines.hexdigest()}, sort_keys=True), file=out)
    enc.close()


if __name__ == "__main__":
    main()
