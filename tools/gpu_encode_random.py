"""random encoder configurations (layout, sizes, levels, block shape, MCT, 5/3 or 9/7 and its step, content, guard bits,
batches of frames of different sizes with padded rows, byte budgets) through htj2k_encode_batch, every frame checked
against references: vecgen's bytes (no budget) or the CPU rebuild from the planes the encoder reports (budget), the
product decoder against the oracle, the source for lossless streams, and OpenJPEG where Pillow returns the layout
sample for sample (a 9/7 difference beyond one LSB is settled by enc_opj.arbitrate and counted, `opj_arbitrated` frames).
The encoder's counterpart of tools/gpu_random_configs.py.  With --tiles every draw also takes a random tile size (a strip
in one draw of four), drawn again where the encoder must refuse the grid for one of the draw's frames.  With --ht-passes
every draw also takes a pass limit 0 .. 3 (htj2k_enc_opts.ht_passes); streams with blocks of several passes are checked
against the CPU rebuild from the planes and passes the encoder reports (tests/rc_passes_model.py), budget or not.
usage: python tools/gpu_encode_random.py [--tiles] [--ht-passes] [count] [seed]     (ONLY=3,17 in the environment: those draws alone)"""
import os, sys, time, traceback
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ffmpeg_ht_amd as m
import enc97_model as e97, enc_frames as ef, enc_model as em, enc_opj, enc_tiles_model as tm, oracle, vecgen
import rc_model as rc, rc_passes_model as pm
from test_encode_gpu import FORMATS, _content

TILES = "--tiles" in sys.argv[1:]
PASSES = "--ht-passes" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a not in ("--tiles", "--ht-passes")]
N = int(ARGS[0]) if len(ARGS) > 0 else 200
SEED = int(ARGS[1]) if len(ARGS) > 1 else 1
ONLY = set(int(v) for v in os.environ["ONLY"].split(",")) if os.environ.get("ONLY") else None
KINDS = ["synth", "noise", "zero", "max", "checker"]


def draw_size(rng):
    """1 .. 700 each way: a third of the widths above 256 (the unpack, DWT and quantiser kernels take 256 columns per
    workgroup), four in ten of those above 512; one size in ten is 1, 2 or 3 in one direction"""
    w = int(rng.integers(257, 701)) if rng.random() < 1 / 3 else int(rng.integers(1, 257))
    h = int(rng.integers(1, 701))
    if rng.random() < 0.1:
        if rng.random() < 0.5:
            w = int(rng.integers(1, 4))
        else:
            h = int(rng.integers(1, 4))
    return w, h


def max_expn(qstep, bits, levels):
    return max(e for e, _, _ in e97.steps(qstep, bits, levels))


def draw_tile(rng, fmt, sizes):
    """a tile size the encoder accepts for every frame of the draw: 1 .. 300 each way, log-uniform (small tiles are the
    ones with odd origins at deep levels and empty resolutions), 0 in one direction in one draw of four"""
    while True:
        tile = [int(2.0 ** rng.uniform(0, np.log2(300))), int(2.0 ** rng.uniform(0, np.log2(300)))]
        if rng.random() < 0.25:
            tile[int(rng.integers(0, 2))] = 0
        # at most 400 tiles a frame: the CPU references take their time per tile
        if not any(tm.refused(fmt, w, h, tile) or len(tm.grid(w, h, tile)) > 400 for w, h in sizes):
            return tuple(tile)


def draw_config(rng):
    pool = enc_opj.LAYOUTS if rng.random() < 0.5 else FORMATS
    fmt, bits = pool[int(rng.integers(0, len(pool)))]
    levels = int(rng.choice([11, 32])) if rng.random() < 0.1 else int(rng.integers(0, 9))
    cbw = int(rng.integers(2, 11))
    cbh = int(rng.integers(2, min(10, 12 - cbw) + 1))
    mct = int(rng.choice([-1, 0, 1] if fmt in em.RGB else [-1, 0]))
    irrev = bool(rng.random() < 0.5)
    qstep = float(2.0 ** rng.uniform(-6, 3)) if irrev else 1.0
    # deep transforms of deep samples at fine steps: the encoder takes M_b = exponent + G - 1 up to 30, and G may be 5 here
    while irrev and not (e97.exponents_valid(qstep, bits, levels) and max_expn(qstep, bits, levels) + 4 <= 30):
        levels -= 1
    nf = int(rng.integers(1, 5))
    sizes = []
    while len(sizes) < nf:
        s = draw_size(rng)
        if s not in sizes:
            sizes.append(s)
    frames = [dict(w=w, h=h, kind=KINDS[int(rng.integers(0, len(KINDS)))], seed=int(rng.integers(0, 1000)),
                   pads=[int(rng.integers(0, 64)) for _ in range(4)]) for w, h in sizes]
    guard_plus = int(rng.integers(0, 4)) if rng.random() < 0.3 else None
    budget = (float(rng.uniform(0.05, 0.95)), int(rng.integers(0, nf))) if rng.random() < 1 / 3 else None
    tile = draw_tile(rng, fmt, sizes) if TILES else (0, 0)      # drawn last: without --tiles the draws are what they were
    passes = int(rng.integers(0, 4)) if PASSES else 0           # and this after it
    return dict(fmt=fmt, bits=bits, levels=levels, cb=(cbw, cbh), mct=mct, irrev=irrev, qstep=qstep, frames=frames,
                guard_plus=guard_plus, budget=budget, tile=tile, passes=passes)


class Fatal(Exception):
    """the device or the runtime failed: nothing more is started on it"""


def encode(enc, frames, fmt, bits, **opts):
    try:
        return ef.encode_frames(enc, frames, fmt, bits, **opts)
    except m.Htj2kError as e:
        if e.code == -0x20545845:                             # a HIP call failed
            raise Fatal(str(e))
        raise


def run_draw(enc, orc, cfg, stat):
    fmt, bits, irrev = cfg["fmt"], cfg["bits"], cfg["irrev"]
    mct_v = em.mct_default(fmt) if cfg["mct"] < 0 else bool(cfg["mct"])
    opts = dict(levels=cfg["levels"], cb=cfg["cb"], mct=cfg["mct"], irreversible=irrev, qstep=cfg["qstep"])
    tiled = cfg["tile"] != (0, 0)
    if tiled:
        opts["tile"] = cfg["tile"]
    comps = [_content(f["kind"], fmt, f["w"], f["h"], bits, f["seed"]) for f in cfg["frames"]]
    planes = [em.to_planes(c, fmt, bits) for c in comps]
    made = [ef.padded_frame(p, fmt, f["w"], f["h"], f["pads"]) for p, f in zip(planes, cfg["frames"])]
    frames = [fr for fr, _ in made]

    def reference(k, guard):
        f = cfg["frames"][k]
        if irrev:
            return vecgen.encode(comps[k], tile=cfg["tile"], **e97.vecgen_args(fmt, f["w"], f["h"], bits, cfg["levels"], cfg["cb"], mct_v, guard, cfg["qstep"]))
        return vecgen.encode(comps[k], tile=cfg["tile"], **em.vecgen_args(fmt, f["w"], f["h"], bits, cfg["levels"], cfg["cb"], mct_v, guard))

    def rebuild(k, guard, ro):
        """the budgeted stream again on the CPU from the planes (and passes) the encoder reports"""
        f = cfg["frames"][k]
        if multi:
            o = {x: y for x, y in ro.items() if x not in ("guard_bits", "ht_passes")}
            idx = tm.coefficient_planes(comps[k], fmt, f["w"], f["h"], bits, cfg["levels"], mct_v, cfg["tile"], cfg["qstep"] if irrev else None) \
                if tiled else rc.indices(comps[k], fmt, bits, cfg["levels"], mct_v, irrev, cfg["qstep"])
            blocks = m.Encoder.layout(f["w"], f["h"], fmt, bits, **o)
            coded = [pm.code_block(rc.block_view(idx, b), p, n) for b, p, n in zip(blocks, chosen[k], npass[k])]
            assert [c[4] for c in coded] == npass[k], ("passes differ from the model's fallback rule", k)
            return pm.assemble(coded, f["w"], f["h"], fmt, bits, planes=chosen[k], guard_bits=guard, **o)
        if not tiled:
            return ef.rebuild(comps[k], fmt, bits, f["w"], f["h"], chosen[k], guard, **ro)
        idx = tm.coefficient_planes(comps[k], fmt, f["w"], f["h"], bits, cfg["levels"], mct_v, cfg["tile"], cfg["qstep"] if irrev else None)
        o = {x: y for x, y in ro.items() if x != "guard_bits"}
        data, mu = tm.code_blocks(idx, m.Encoder.layout(f["w"], f["h"], fmt, bits, **o), chosen[k])
        return m.Encoder.assemble(f["w"], f["h"], fmt, bits, data, max_u=mu, planes=chosen[k], guard_bits=guard, **o)

    # guard bits: automatic, or fixed at the largest automatic value of the call's frames plus 0 .. 3
    fixed = None
    if cfg["guard_plus"] is not None:
        auto = encode(enc, frames, fmt, bits, **opts)
        fixed = min(7, max(em.qcd_guard_bits(cs) for cs in auto) + cfg["guard_plus"])
        if irrev:
            fixed = min(fixed, 31 - max_expn(cfg["qstep"], bits, cfg["levels"]))
        opts["guard_bits"] = fixed
    multi = cfg["passes"] > 1
    target = 0
    if cfg["budget"]:
        share, k = cfg["budget"]
        free = reference(k, fixed if fixed else em.qcd_guard_bits(encode(enc, [frames[k]], fmt, bits, **opts)[0]))
        lay = {x: y for x, y in opts.items() if x != "guard_bits"}
        smallest = max(len(m.Encoder.assemble(f["w"], f["h"], fmt, bits, [b""] * len(m.Encoder.layout(f["w"], f["h"], fmt, bits, **lay)),
                                              guard_bits=fixed or 0, **lay)) for f in cfg["frames"])
        target = max(int(len(free) * share), smallest)
        opts["target_bytes"] = target
    if PASSES:
        opts["ht_passes"] = cfg["passes"]
    got = encode(enc, frames, fmt, bits, **opts)
    infos = [enc.rc_info(k) for k in range(len(frames))]
    chosen = [enc.last_planes(k) for k in range(len(frames))]
    npass = [enc.last_passes(k) for k in range(len(frames))]
    assert all(1 <= n <= max(cfg["passes"], 1) for v in npass for n in v), "passes beyond the limit"

    pf = em.pix(fmt)
    dec = m.Decoder(device_id=0, req_pix_fmt=pf)
    try:
        for k, (cs, f) in enumerate(zip(got, cfg["frames"])):
            w, h = f["w"], f["h"]
            g = em.qcd_guard_bits(cs)
            assert fixed is None or g == fixed, ("guard bits", k, g, fixed)
            info = infos[k]
            assert info["final_bytes"] == len(cs) and info["target_bytes"] == target and info["nblocks"] == len(chosen[k]), ("rc_info", k, info)
            lossless = not irrev
            if target:
                assert len(cs) <= target, ("over budget", k, len(cs), target)
                assert 1 <= info["ht_launches"] <= 3 and info["blocks_left_out"] == sum(p < 0 for p in chosen[k]), ("rc_info", k, info)
                ro = {x: y for x, y in opts.items() if x != "target_bytes"}
                assert rebuild(k, g, ro) == cs, ("rebuild from last_planes", k)
                stat["multi_blocks"] += sum(n > 1 for n in npass[k])
                lossless = lossless and not any(chosen[k]) and max(npass[k]) == 1
            elif multi:
                assert rebuild(k, g, dict(opts)) == cs, ("rebuild from last_passes", k, w, h)
                assert not any(chosen[k]), ("planes without a budget", k)
                lossless = lossless and max(npass[k]) == 1
                stat["multi_blocks"] += sum(n > 1 for n in npass[k])
            else:
                assert cs == reference(k, g), ("bytes differ from vecgen", k, w, h)
                assert not any(chosen[k]), ("planes without a budget", k)
            want = None
            for bitexact in (0, 1):
                dec.set_int("bitexact", bitexact)
                info_d, pg, _, st = dec.decode(cs)
                assert info_d.pix_fmt == pf and st.n_block_errors == 0, ("product decode", k, bitexact)
                _, po, _ = orc.decode(cs, req_pix_fmt=pf, bitexact=bitexact)
                assert all(np.array_equal(a, b) for a, b in zip(pg, po)), ("product decoder differs from the oracle", k, bitexact)
                want = po if bitexact == 0 else want
            if lossless:
                assert all(np.array_equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(want, planes[k])), ("lossless round trip", k)
            if enc_opj.exact(fmt, bits):
                arb = []
                # (enc_opj's own arbitration reads one tile-component per component: tiled streams go to tm.arbitrate)
                bad = enc_opj.compare(cs, fmt, bits, w, h, want, irrev, planes[k] if lossless else None, orc=None if tiled else orc, arbitrated=arb)
                if tiled and irrev and bad and bad.startswith("differs from the oracle"):
                    bad = tm.arbitrate(cs, fmt, bits, w, h, cfg["tile"], orc, enc_opj.arrange(want, fmt, w, h), enc_opj.pixels(cs, fmt))
                    arb.extend([(fmt, bits, w, h)] if bad is None else [])
                assert bad is None, ("OpenJPEG", k, bad)
                if arb:
                    stat["opj_arbitrated"] += 1
                    print("OpenJPEG beyond one LSB, settled by the float64 synthesis (tests/enc_opj.py):", arb[0], flush=True)
            stat["frames"] += 1
    finally:
        dec.close()
    stat["budget"] += bool(target)
    stat["opj"] += bool(enc_opj.exact(fmt, bits))
    stat["fixed_guard"] += fixed is not None
    stat["tiled"] += tiled
    stat["strips"] += tiled and 0 in cfg["tile"]


def main():
    if not enc_opj.HAVE_OPJ:
        print("Pillow / OpenJPEG is not importable: the OpenJPEG leg cannot run")
        print("done", dict(draws=0, ok=0, bad=1, skipped=N))
        return 1
    enc = m.Encoder(0)
    orc = oracle.OracleDecoder()
    stat = dict(draws=0, ok=0, bad=0, skipped=0, frames=0, opj=0, opj_arbitrated=0, budget=0, fixed_guard=0, wide=0, tiled=0, strips=0,
                multi_blocks=0)
    t0 = time.time()
    for it in range(N):
        cfg = draw_config(np.random.default_rng([SEED, it]))
        if ONLY is not None and it not in ONLY:
            continue
        stat["draws"] += 1
        stat["wide"] += any(f["w"] > 256 for f in cfg["frames"])
        try:
            run_draw(enc, orc, cfg, stat)
            stat["ok"] += 1
        except Fatal as e:
            stat["bad"] += 1
            stat["skipped"] += N - it - 1
            print("FATAL", it, cfg, e, flush=True)
            break
        except Exception as e:
            stat["bad"] += 1
            print("MISMATCH", it, cfg, flush=True)
            traceback.print_exc(file=sys.stdout)
        if it % 25 == 24:
            print(it + 1, stat, "%.0fs" % (time.time() - t0), flush=True)
    stat["wall_s"] = round(time.time() - t0, 1)
    print("done", stat, flush=True)
    return 1 if stat["bad"] or stat["skipped"] else 0


if __name__ == "__main__":
    sys.exit(main())
