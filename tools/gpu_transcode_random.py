"""seeded random sources (tests/xc_random.py: layout, size, Part-1 / HT / MIXED, levels, block shape, 5/3 or 9/7, mode
switches, passes, dropped passes, progression, precincts, layers, SOP / EPH, tiles, guard bits, content, container
variants, budgets; one draw in eight out of scope on purpose) through htj2k_transcode_batch_opts with ht_sources.
Consecutive draws in scope go into calls of 1 .. 4 sources.  Per call: the bytes against the CPU rebuild from the
source's indices (tests/xc_source.py), frame by frame, and the planes and passes the encoder reports against the block
rule; one call in four again source by source; the block-stage planes of source and output bit for bit, the decoded
frames against each other and against the oracle's frame of the source; the output transcoded again; in one call of four
the decoder's block routes (ht_multi 0, ht_mode 0, device_gather 0).  A draw with a budget share: within the target, the
CPU rebuild from the reported planes and passes, no block finer than its source, no block error in the oracle.  A draw
out of scope: refused with the predicted code and word alone and in the middle of a call of good sources, a device
buffer filled with 0xA5 untouched, the good sources alone their bytes again.  With --rounds every call is repeated on an
encoder opened under a small HTJ2K_ENC_ROUND: the same bytes in the rounds the frames' samples make.  The transcoder's
counterpart of tools/gpu_encode_random.py.
usage: python tools/gpu_transcode_random.py [--rounds] [count] [seed] [first]     (draws first .. first + count - 1 of the seed)"""
import ctypes, os, sys, time, traceback
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401  (before the library: the device buffers go through it)
import ffmpeg_ht_amd as m
import enc_model as em, oracle, xc_random as xr
from test_transcode_gpu import block_stage_planes

ROUNDS = "--rounds" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a != "--rounds"]
N = int(ARGS[0]) if len(ARGS) > 0 else 200
SEED = int(ARGS[1]) if len(ARGS) > 1 else 1
FIRST = int(ARGS[2]) if len(ARGS) > 2 else 0
EXTERNAL = -0x20545845                                    # a HIP call failed
ROUND_SAMPLES = 2000                                      # --rounds: most calls of several frames take several rounds
KNOBS = ("ht_multi", "ht_mode", "device_gather")


class Fatal(Exception):
    """the device or the runtime failed: nothing more is started on it"""


def refusal(call):
    """-> (code, text) of the Htj2kError the call raises, (0, "") where it raises none"""
    try:
        call()
    except m.Htj2kError as e:
        if e.code == EXTERNAL:
            raise Fatal(str(e))
        return e.code, str(e)
    return 0, ""


def expected_rounds(draws, limit):
    """the rounds of a call on an encoder whose rounds take `limit` samples: frames in order, a round holds frames of one
    component count, ends before the frame that would take its samples beyond the limit, and holds at least one"""
    rounds, ns, nc = 0, 0, None
    for d in draws:
        dims = em.comp_dims(d["fmt"], d["w"], d["h"])
        s = sum(cw * ch for cw, ch in dims)
        if nc != len(dims) or ns + s > limit:
            rounds, ns, nc = rounds + 1, 0, len(dims)
        ns += s
    return rounds


def equal_frames(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def run_call(enc, small, dec, orc, group, rng, stat):
    """group: [(draw, prepared)] of draws in scope -> the call's output streams"""
    draws, srcs, srcs_s = [d for d, _ in group], [p["src"] for _, p in group], [p["s"] for _, p in group]
    n = len(group)
    want = [s.free() for s in srcs_s]
    got = enc.transcode(dec, srcs, ht_sources=True)
    assert enc.last_rounds() == expected_rounds(draws, 1 << 30), (enc.last_rounds(), expected_rounds(draws, 1 << 30))
    reported = [(enc.last_planes(i), enc.last_passes(i)) for i in range(n)]
    for i, s in enumerate(srcs_s):
        forms = s.forms()
        assert reported[i] == ([f[0] for f in forms], [f[1] for f in forms]), ("planes and passes differ from the rule", i)
        assert got[i] == want[i], ("bytes differ from the CPU rebuild", i, len(got[i]), len(want[i]))
        stat["blocks"] += len(forms)
        stat["multi_blocks"] += sum(f[1] > 1 and not f[2] for f in forms)
    if n > 1 and rng.random() < 0.25:
        assert [enc.transcode(dec, [x], ht_sources=True)[0] for x in srcs] == got, "source by source"
        stat["singly"] += 1
    # the product decoder and the oracle
    for i, (src, cs) in enumerate(zip(srcs, got)):
        a, b = block_stage_planes(dec, src), block_stage_planes(dec, cs)
        assert len(a) == len(b)
        for t, (p, q) in enumerate(zip(a, b)):
            assert p.dtype == q.dtype and p.shape == q.shape and np.array_equal(p.view(np.uint32), q.view(np.uint32)), ("block stage", i, t)
        ia, pa, _, sa = dec.decode(src)
        ib, pb, _, sb = dec.decode(cs)
        assert sa.n_block_errors == 0 == sb.n_block_errors and ib.is_ht == 1, ("product decode", i)
        assert (ia.width, ia.height, ia.pix_fmt, ia.bits_per_raw_sample) == (ib.width, ib.height, ib.pix_fmt, ib.bits_per_raw_sample)
        assert equal_frames(pa, pb), ("the output's frame differs from the source's", i)
        _, po, _ = orc.decode(src)
        assert orc.block_errors() == 0 and equal_frames(pa, po), ("the product's frame differs from the oracle's", i)
    # the output is a source like any other
    assert enc.transcode(dec, got, ht_sources=True) == got, "the output transcoded again"
    if rng.random() < 0.25:
        try:
            for knob in KNOBS:
                dec.set_int(knob, 0)
                assert enc.transcode(dec, srcs, ht_sources=True) == got, knob
                dec.set_int(knob, 1)
        finally:
            for knob in KNOBS:
                dec.set_int(knob, 1)
        stat["knobs"] += 1
    if small is not None:
        assert small.transcode(dec, srcs, ht_sources=True) == got, "rounds"
        assert small.last_rounds() == expected_rounds(draws, ROUND_SAMPLES), (small.last_rounds(), expected_rounds(draws, ROUND_SAMPLES))
        stat["calls_of_rounds"] += small.last_rounds() > expected_rounds(draws, 1 << 30)      # more rounds than the component counts make
    # budgets
    for i, (d, s) in enumerate(zip(draws, srcs_s)):
        if d["share"] is None:
            continue
        target = max(int(d["share"] * len(got[i])), m.Encoder.transcode_min_size(s.src, ht_sources=True))
        cs = (small or enc).transcode(dec, [s.src], target_bytes=target, ht_sources=True)[0]
        planes, passes = (small or enc).last_planes(0), (small or enc).last_passes(0)
        assert len(cs) <= target, ("over budget", i, len(cs), target)
        assert cs == s.stream(planes, passes), ("budget: bytes differ from the CPU rebuild", i)
        s.check_not_finer(planes, passes)
        orc.decode(cs)
        assert orc.block_errors() == 0, ("budget: the oracle fails blocks", i)
        stat["budget"] += 1
        stat["budget_coarser"] += (planes, passes) != reported[i]
    stat["calls"] += 1
    return got


def run_refused(enc, dec, plain, p, good, code, word, ht_sources, stat):
    """a source out of scope (or asked for in a way that is: dec opened with a reduction factor, ht_sources off): alone,
    and in the middle of the good sources of the last call, which then give their bytes again on the decoder `plain`"""
    got, text = refusal(lambda: enc.transcode(dec, [p["src"]], cap=1 << 20, ht_sources=ht_sources))
    assert got == code and word in text and not enc.last_out.any(), ("refused alone", got, text)
    if good is None:
        return
    srcs, outs = good
    if len(srcs) == 1:
        srcs, outs = srcs * 2, outs * 2
    half = len(srcs) // 2
    mid = srcs[:half] + [p["src"]] + srcs[half:]
    got, text = refusal(lambda: enc.transcode(dec, mid, cap=sum(len(o) for o in outs) + (1 << 20), ht_sources=ht_sources))
    assert got == code and word in text and not enc.last_out.any(), ("refused in a call", got, text)
    cap = sum(len(o) for o in outs) + (1 << 20)
    dev = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pk = [m.packet(x) for x in mid]
    ptrs = (ctypes.c_void_p * len(pk))(*[ctypes.cast(b, ctypes.c_void_p) for b, _ in pk])
    sizes = (ctypes.c_int * len(pk))(*[sz for _, sz in pk])
    offs = (ctypes.c_size_t * (len(pk) + 1))()
    got, _ = refusal(lambda: enc.transcode_into(dec, ptrs, sizes, len(pk), ctypes.c_void_p(dev.data_ptr()), cap, offs, out_on_device=1,
                                                ht_sources=ht_sources))
    torch.cuda.synchronize()
    assert got == code and bool((dev == 0xA5).all()), ("the device buffer of a refused call", got)
    assert enc.transcode(plain, srcs, ht_sources=True) == outs, "the good sources after a refused call"
    stat["refused_in_a_call"] += 1


def fatal(e):
    return isinstance(e, Fatal) or (isinstance(e, m.Htj2kError) and e.code == EXTERNAL) or \
        (isinstance(e, RuntimeError) and not isinstance(e, m.Htj2kError) and "HIP error" in str(e))


def main():
    enc, dec, orc = m.Encoder(0), m.Decoder(device_id=0), oracle.OracleDecoder()
    small = None
    if ROUNDS:
        old = os.environ.get("HTJ2K_ENC_ROUND")
        os.environ["HTJ2K_ENC_ROUND"] = str(ROUND_SAMPLES)
        try:
            small = m.Encoder(0)
        finally:
            if old is None:
                del os.environ["HTJ2K_ENC_ROUND"]
            else:
                os.environ["HTJ2K_ENC_ROUND"] = old
    stat = dict(draws=N, ok=0, bad=0, skipped=0, left_out=0, refused=0, refused_in_a_call=0, calls=0, singly=0, knobs=0, budget=0,
                budget_coarser=0, calls_of_rounds=0, blocks=0, multi_blocks=0)
    rng = np.random.default_rng([SEED, FIRST, 77])         # the calls' sizes and what is repeated
    state = dict(group=[], size=int(rng.integers(1, 5)), good=None)
    t0 = time.time()

    def checked(what, draws, work, count=True):
        """work() with its draws counted: ok (count) or bad with a MISMATCH line -> did it pass?  A failure of the device
        goes up as Fatal"""
        try:
            work()
        except Exception as e:
            if fatal(e):
                raise Fatal("%s %s: %s" % (what, [i for i, _ in draws], e))
            stat["bad"] += len(draws)
            print("MISMATCH", what, [(i, xr.describe(d)) for i, d in draws], flush=True)
            traceback.print_exc(file=sys.stdout)
            return False
        stat["ok"] += len(draws) if count else 0
        return True

    def flush():
        g, state["group"], state["size"] = state["group"], [], int(rng.integers(1, 5))
        if g:
            def work():
                outs = run_call(enc, small, dec, orc, [(d, p) for _, d, p in g], rng, stat)
                state["good"] = ([p["src"] for _, _, p in g], outs)
            checked("call", [(i, d) for i, d, _ in g], work)

    def left_out(p):
        if p["status"] == "headroom":                      # left out of the comparison, and refused by the product too
            got, text = refusal(lambda: enc.transcode(dec, [p["src"]], cap=1 << 20, ht_sources=True))
            assert got == xr.PATCHWELCOME and "fills all" in text and not enc.last_out.any(), (got, text)
        stat["left_out"] += 1

    def out_of_scope(d, p):
        if p["status"] == "refused":
            run_refused(enc, dec, dec, p, state["good"], p["code"], p["word"], True, stat)
        elif d["out"] == "no_opt_in":
            run_refused(enc, dec, dec, p, state["good"], *xr.predicted(d, ht_sources=False), False, stat)
        else:
            low = m.Decoder(device_id=0, reduction_factor=1)
            try:
                run_refused(enc, low, dec, p, state["good"], *xr.predicted(d, reduced=True), True, stat)
            finally:
                low.close()
        stat["refused"] += 1

    try:
        for it in range(FIRST, FIRST + N):
            d = xr.draw(np.random.default_rng([SEED, it]))
            made = {}
            if not checked("the CPU reference", [(it, d)], lambda: made.update(xr.prepare(orc, d)), count=False):
                continue
            p = made
            if p["status"] in ("factory", "headroom"):
                checked("left out", [(it, d)], lambda: left_out(p), count=False)
            elif p["status"] == "refused":
                flush()
                checked("out of scope", [(it, d)], lambda: out_of_scope(d, p))
            elif d["out"] in ("no_opt_in", "reduce"):      # refused only for how it is asked for: the source then goes on as one in scope
                flush()
                if checked("out of scope", [(it, d)], lambda: out_of_scope(d, p), count=False):
                    state["group"].append((it, d, p))
            else:
                state["group"].append((it, d, p))
            if len(state["group"]) >= state["size"]:
                flush()
        flush()
    except Fatal as e:
        stat["bad"] += 1
        print("FATAL", e, flush=True)
    stat["skipped"] = N - stat["ok"] - stat["bad"] - stat["left_out"]
    stat["wall_s"] = round(time.time() - t0, 1)
    print("done", stat, flush=True)
    return 1 if stat["bad"] or stat["skipped"] else 0


if __name__ == "__main__":
    sys.exit(main())
