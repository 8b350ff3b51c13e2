"""GPU checks of HT refinement passes in the encoder (ht_passes 2 and 3): k_ht_refine_plan / k_ht_refine_encode byte for
byte against vecgen's encode_block of the shifted indices, whole frames against the CPU model's stream
(tests/rc_passes_model.py) and decoded by the product decoder and the oracle, and the paths around them."""
import numpy as np
import pytest

import enc_model as em
import ffmpeg_ht_amd as m
import rc_model as rc
import rc_passes_model as pm
import vecgen

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (4, 4), (5, 9), (33, 31), (64, 64), (128, 32), (1024, 4), (4, 1024)]


@pytest.fixture(scope="module")
def enc():
    e = m.Encoder(0)
    yield e
    e.close()


def _contents(w, h, p, rng):
    """(name, block) for refinement plane p: random ones and the blocks that reach every corner of the two passes"""
    one, big = 1 << p, 5 << p
    out = [("sparse", rng.integers(-4 * one, 4 * one + 1, size=(h, w)) * (rng.random((h, w)) < 0.15)),
           ("dense", rng.integers(-8 * one, 8 * one + 1, size=(h, w))),
           ("wide", rng.integers(-(1 << 20), 1 << 20, size=(h, w)) * (rng.random((h, w)) < 0.5))]
    chain = np.full((h, w), one, np.int64)            # one significant sample, every other magnitude exactly 2^p
    chain[0, 0] = big
    out.append(("chain from the top-left", chain))
    back = np.full((h, w), one, np.int64)             # nothing before it in scan order joins unless it touches it
    back[h - 1, w - 1] = -big
    out.append(("significant at the bottom-right", back))
    if h > 4:                                         # last row of a stripe, members in the first row of the next
        s = np.zeros((h, w), np.int64)
        s[3, w // 2] = big
        s[4:, :] = -one
        out.append(("across a stripe boundary", s))
    neg = np.full((h, w), -one, np.int64)             # every member newly significant and negative: runs of 1 bits
    neg[::7, ::5] = big
    out.append(("all new and negative", neg))
    out.append(("all significant, bit p set", np.full((h, w), -(3 << p), np.int64)))
    out.append(("falls back: nothing at p + 1", rng.integers(-(2 * one - 1), 2 * one, size=(h, w))))
    return [(n, a.astype(np.int32)) for n, a in out]


@pytest.mark.parametrize("w,h", SHAPES)
def test_blocks_equal_vecgen(enc, w, h):
    """bytes, lcup, lref and max_u of every block equal vecgen's encode_block(shifted(v, p), passes); a block that falls
    back has the bytes of one pass at p"""
    rng = np.random.default_rng(w * 1031 + h)
    fell = coded = 0
    for p in range(4):
        cases = _contents(w, h, p, rng)
        for passes in (2, 3):
            n = len(cases)
            plane = np.concatenate([v for _, v in cases], axis=0)
            got = enc.ht_encode_blocks(plane, [(0, i * h, w, h) for i in range(n)], planes=[p] * n, passes=[passes] * n)
            for (name, v), (data, lcup, lref, mu) in zip(cases, got):
                want, wl, wr, wu, wp = pm.code_block(v, p, passes)
                assert (lcup, lref, mu) == (wl, wr, wu), (name, w, h, p, passes)
                assert data == want, (name, w, h, p, passes)
                fell += wp == 1
                coded += wp > 1
    assert fell and (coded or (w, h) == (1, 1))


def test_one_by_one_with_two_passes_falls_back(enc):
    v = np.array([[-6]], np.int32)
    (data, lcup, lref, mu), = enc.ht_encode_blocks(v, [(0, 0, 1, 1)], planes=[0], passes=[2])
    d1, l1, _, u1 = vecgen.encode_block(v)
    assert (data, lcup, lref, mu) == (d1[:l1], l1, 0, u1)
    (data, lcup, lref, mu), = enc.ht_encode_blocks(v, [(0, 0, 1, 1)], planes=[0], passes=[3])
    d3, l3, r3, u3 = vecgen.encode_block(v, passes=3)
    assert r3 > 0 and (data, lcup, lref, mu) == (d3[:l3 + r3], l3, r3, u3)


def test_mixed_pass_counts_in_one_call(enc):
    """blocks of 1, 2 and 3 passes side by side in one plane, each with its own plane, equal single calls"""
    rng = np.random.default_rng(11)
    plane = rng.integers(-40, 41, size=(64, 192)).astype(np.int32)
    rects = [(0, 0, 64, 64), (64, 0, 64, 64), (128, 0, 64, 64), (3, 5, 33, 31), (70, 1, 5, 9)]
    passes, planes = [1, 2, 3, 3, 2], [1, 0, 2, 1, 3]
    got = enc.ht_encode_blocks(plane, rects, planes=planes, passes=passes)
    for (x, y, w, h), k, p, (data, lcup, lref, mu) in zip(rects, passes, planes, got):
        want, wl, wr, wu, _ = pm.code_block(plane[y:y + h, x:x + w], p, k)
        assert (data, lcup, lref, mu) == (want, wl, wr, wu), (x, y, k, p)
    with pytest.raises(m.Htj2kError):
        enc.ht_encode_blocks(plane, rects[:1], planes=[0], passes=[4])
    with pytest.raises(m.Htj2kError):
        enc.ht_encode_blocks(plane, rects[:1], planes=[31], passes=[2])


def synth(fmt, w, h, bits, seed=1):
    return [vecgen.synth_image(cw, ch, 1, depth=bits, seed=seed + c)[0] for c, (cw, ch) in enumerate(em.comp_dims(fmt, w, h))]


def check_decodes(cs, fmt, orc, decs):
    """product float / bitexact decodes == the oracle's in the same mode, no block errors"""
    pf = em.pix(fmt)
    for bitexact in (0, 1):
        if (pf, bitexact) not in decs:
            decs[pf, bitexact] = m.Decoder(device_id=0, req_pix_fmt=pf, bitexact=bitexact)
        _, got, _, st = decs[pf, bitexact].decode(cs)
        assert st.n_block_errors == 0
        _, want, _ = orc.decode(cs, req_pix_fmt=pf, bitexact=bitexact)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (fmt, bitexact)


FRAMES = [("gray", 8), ("rgb24", 8), ("yuv420p10le", 10), ("gray16le", 16)]


@pytest.mark.parametrize("irreversible", [False, True])
@pytest.mark.parametrize("fmt,bits", FRAMES)
def test_frames_without_a_budget(enc, orc, fmt, bits, irreversible):
    """the stream is the model's (coefficient model -> vecgen blocks with the fallback rule -> Encoder.assemble), the
    passes reported are the model's, and the product decoder agrees with the oracle"""
    w, h = 160, 96
    comps = synth(fmt, w, h, bits)
    planes = em.to_planes(comps, fmt, bits)
    opts = dict(levels=3, cb=(4, 4), irreversible=irreversible, qstep=0.25)
    decs = {}
    one = enc.encode(planes, fmt, bits, **opts)
    for passes in (2, 3):
        cs = enc.encode(planes, fmt, bits, ht_passes=passes, **opts)
        want, coded, _, blocks = pm.frame_stream(comps, fmt, w, h, bits, passes, **opts)
        assert cs == want, (fmt, passes, irreversible)
        got = enc.last_passes(0)
        assert got == [c[4] for c in coded] and enc.last_planes(0) == [0] * len(blocks)
        assert passes in got
        assert cs != one
        check_decodes(cs, fmt, orc, decs)
        assert enc.ref_stage_ms()[0] > 0 and enc.ref_stage_ms()[1] == 0      # no budget: no statistics
    for d in decs.values():
        d.close()


def test_one_pass_is_the_default_call(enc):
    """ht_passes 0 and 1 give the default call's bytes, with and without a budget"""
    comps = synth("rgb24", 160, 96, 8)
    planes = em.to_planes(comps, "rgb24", 8)
    for opts in (dict(levels=3, cb=(4, 4)), dict(levels=3, cb=(4, 4), irreversible=True, qstep=0.25)):
        free = enc.encode(planes, "rgb24", 8, **opts)
        for budget in (0, len(free) // 2):
            ref = enc.encode(planes, "rgb24", 8, target_bytes=budget, **opts)
            for k in (0, 1):
                assert enc.encode(planes, "rgb24", 8, target_bytes=budget, ht_passes=k, **opts) == ref
                assert enc.last_passes(0) == [1] * len(enc.last_planes(0))
                assert enc.ref_stage_ms() == [0, 0]
    for k in (4, -1):                                        # refused with EINVAL and a log line
        del enc._logs[:]
        with pytest.raises(m.Htj2kError) as err:
            enc.encode(planes, "rgb24", 8, ht_passes=k)
        assert err.value.code == -22 and any("ht_passes %d is not 0 .. 3" % k in line for line in enc._logs), enc._logs


def _model(c, fmt, w, h, bits, opts):
    return pm.frame_stream(c, fmt, w, h, bits, opts["ht_passes"], **{k: v for k, v in opts.items() if k != "ht_passes"})[0]


def test_further_paths(enc, orc, monkeypatch):
    """a batch of frames of different sizes, determinism over two calls, several rounds, a tile grid, device input and
    output: the model's streams throughout"""
    import torch
    import enc_frames as ef
    fmt, bits = "rgb24", 8
    sizes = [(160, 96), (97, 61), (33, 140)]
    frames = [(synth(fmt, w, h, bits, seed=3 + i), w, h) for i, (w, h) in enumerate(sizes)]
    planes = [em.to_planes(c, fmt, bits) for c, _, _ in frames]
    opts = dict(levels=3, cb=(4, 4), irreversible=True, qstep=0.25, ht_passes=3)
    want = [_model(c, fmt, w, h, bits, opts) for c, w, h in frames]
    batch = enc.encode_batch(planes, fmt, bits, **opts)
    assert batch == want
    assert enc.encode_batch(planes, fmt, bits, **opts) == batch
    monkeypatch.setenv("HTJ2K_ENC_ROUND", "20000")              # every frame a round of its own
    e2 = m.Encoder(0)
    try:
        assert e2.encode_batch(planes, fmt, bits, **opts) == batch
        assert [e2.last_passes(i) for i in range(3)] == [enc.last_passes(i) for i in range(3)]
    finally:
        e2.close()
    c, w, h = frames[0]
    tiled = dict(opts, tile=(64, 48), ht_passes=2)
    cs = enc.encode(planes[0], fmt, bits, **tiled)
    assert cs == _model(c, fmt, w, h, bits, tiled)
    decs = {}
    check_decodes(cs, fmt, orc, decs)
    for d in decs.values():
        d.close()
    # device input, device output
    made = [ef.device_frame(p, fmt, w, h, [0] * 4, torch) for p, (w, h) in zip(planes, sizes)]
    cap = sum(m.Encoder.bound(w, h, fmt, bits, **opts) for w, h in sizes)
    dev = torch.zeros((cap,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r, offs = ef.call_batch(enc, [f for f, _ in made], bits, dev.data_ptr(), cap=cap, in_on_device=1, out_on_device=1, **opts)
    back = dev.cpu().numpy()
    assert r == 0 and [back[offs[i]:offs[i + 1]].tobytes() for i in range(3)] == batch


# ---------------------------------------------------------------------------------------------- statistics

def grid(w, h, bw, bh):
    return [(x, y, min(bw, w - x), min(bh, h - y)) for y in range(0, h, bh) for x in range(0, w, bw)]


def stat_planes():
    """(name, int32 plane, rects): index planes of the 160 x 96 frames, and synthetic extremes"""
    out = []
    for fmt, bits, irrev in [("gray", 8, True), ("rgb24", 8, False), ("yuv420p10le", 10, True), ("gray16le", 16, False)]:
        idx = rc.indices(synth(fmt, 160, 96, bits), fmt, bits, 3, em.mct_default(fmt), irrev, 0.25)
        for c, p in enumerate(idx):
            out.append(("%s c%d" % (fmt, c), p, grid(p.shape[1], p.shape[0], 16, 16)))
    rng = np.random.default_rng(5)
    wide = rng.integers(-5000, 5000, size=(8, 2048)).astype(np.int32)
    out.append(("1024x4", wide, grid(2048, 8, 1024, 4)))
    out.append(("4x1024", np.ascontiguousarray(wide.T), grid(8, 2048, 4, 1024)))
    chain = np.ones((64, 128), np.int32)
    chain[0, 0], chain[63, 127] = 9, -9
    out.append(("chains", chain, grid(128, 64, 64, 64) + [(1, 1, 33, 31)]))
    sparse = (rng.integers(-40, 41, size=(96, 96)) * (rng.random((96, 96)) < 0.05)).astype(np.int32)
    out.append(("sparse", sparse, grid(96, 96, 64, 64) + [(1, 1, 3, 5), (5, 7, 1, 1), (0, 0, 33, 17)]))
    out.append(("zeros", np.zeros((16, 16), np.int32), [(0, 0, 16, 16)]))
    return out


def test_rc_stats_passes_are_exact(enc):
    """dist2 / dist3 and the bit counts of the two passes equal the model's wherever the block has such a candidate, and
    are 0 where nothing is significant at p + 1"""
    seen = 0
    for name, plane, rects in stat_planes():
        for nplanes in (16, 3):
            d2, d3, sp, mr = enc.rc_stats_passes(plane, rects, nplanes)
            for i, (x, y, w, h) in enumerate(rects):
                v = plane[y:y + h, x:x + w]
                kmax = int(np.abs(v.astype(np.int64)).max()).bit_length()
                for p in range(nplanes):
                    if p + 1 >= kmax:                         # nothing significant at p + 1
                        assert (d2[i][p], d3[i][p], sp[i][p], mr[i][p]) == (0, 0, 0, 0), (name, rects[i], p)
                        continue
                    sig, mem, new = pm.membership(v, p)
                    assert (int(sp[i][p]), int(mr[i][p])) == pm.bit_counts(v, p), (name, rects[i], p)
                    # the distortions without the fallback rule: that is the allocation's business
                    mag = np.abs(v.astype(np.int64))
                    for k, got in ((2, d2), (3, d3)):
                        q = p if k == 3 else p + 1
                        r2 = np.where(sig, 2 * ((mag >> q) << q) + (1 << q), np.where(new, 3 << p, 0))
                        d = np.where(mag > 0, 2 * mag + 1 - r2, 0)
                        assert int(got[i][p]) == int((d * d).sum()), (name, rects[i], p, k)
                    seen += 1
    assert seen > 500


def estimator_ratios(enc):
    """estimated / exact Lcup + Lref over the blocks (Encoder.layout's, 16 x 16) and planes of the 160 x 96 frames, 2 and 3
    passes -> (all ratios, those of candidates above 200 bytes); the estimate is k_rc_select's: len_est[p + 1] and the
    two bit counts in bytes"""
    allr, big = [], []
    for fmt, bits, irrev in [("gray", 8, True), ("rgb24", 8, True), ("yuv420p10le", 10, True), ("gray16le", 16, True),
                             ("gray", 8, False), ("rgb24", 8, False), ("yuv420p10le", 10, False), ("gray16le", 16, False)]:
        opts = dict(levels=3, cb=(4, 4), irreversible=irrev, qstep=0.25)
        idx = rc.indices(synth(fmt, 160, 96, bits), fmt, bits, 3, em.mct_default(fmt), irrev, 0.25)
        blocks = m.Encoder.layout(160, 96, fmt, bits, **opts)
        for c, plane in enumerate(idx):
            rects = [(b["x"], b["y"], b["w"], b["h"]) for b in blocks if b["comp"] == c]
            _, ln = enc.rc_stats(plane, rects, 16)
            _, _, sp, mr = enc.rc_stats_passes(plane, rects, 16)
            for i, (x, y, w, h) in enumerate(rects):
                v = plane[y:y + h, x:x + w]
                for p in range(15):
                    for k in (2, 3):
                        if not mr[i][p] or pm.falls_back(v, p, k):
                            continue
                        est = int(ln[i][p + 1]) + (int(sp[i][p]) + 7) // 8 + ((int(mr[i][p]) + 7) // 8 if k == 3 else 0)
                        _, lcup, lref, _, _ = pm.code_block(v, p, k)
                        allr.append(est / (lcup + lref))
                        if lcup + lref > 200:
                            big.append(est / (lcup + lref))
    return np.array(allr), np.array(big)


# extremes of estimated / exact Lcup + Lref over the candidates above 200 bytes (table in DESIGN.md 3.5), measured
# with this test on an MI355X
EST_MIN, EST_MAX = 0.9966, 1.0048


def test_estimator_accuracy_with_passes(enc):
    """the measured extremes for candidates above 200 bytes, each widened by a quarter of its distance from 1"""
    allr, big = estimator_ratios(enc)
    for name, a in (("all", allr), ("above 200 bytes", big)):
        print(name, len(a), [round(float(x), 4) for x in np.percentile(a, [0, 5, 50, 95, 100])])
    assert len(big) >= 50
    assert big.min() >= 1 - 1.25 * (1 - EST_MIN) and big.max() <= 1 + 1.25 * (EST_MAX - 1), (big.min(), big.max())


# ---------------------------------------------------------------------------------------------- under a budget

BUDGETS = (0.75, 0.50, 0.25, 0.10)


def rebuild(enc, comps, fmt, bits, w, h, opts, cs):
    """the stream again on the CPU from the planes and passes the encoder reports -> (stream, coded blocks)"""
    o = {k: v for k, v in opts.items() if k not in ("ht_passes", "target_bytes")}
    idx = rc.indices(comps, fmt, bits, o["levels"], em.mct_default(fmt), bool(o.get("irreversible")), o.get("qstep", 1.0))
    blocks = m.Encoder.layout(w, h, fmt, bits, **o)
    planes, passes = enc.last_planes(0), enc.last_passes(0)
    assert len(planes) == len(blocks) == len(passes)
    coded = [pm.code_block(rc.block_view(idx, b), p, k) for b, p, k in zip(blocks, planes, passes)]
    assert [c[4] for c in coded] == passes                   # the allocation never picks a candidate that falls back
    return pm.assemble(coded, w, h, fmt, bits, planes=planes, guard_bits=em.qcd_guard_bits(cs), **o), coded, blocks


def parsed_passes(orc, cs, fmt, w, h, blocks):
    """what the oracle's parser reads per block of layout(): (zero bit-planes, passes), None for a block left out"""
    dims = em.comp_dims(fmt, w, h)
    tab = orc.plan_blocks(cs, req_pix_fmt=em.pix(fmt))
    base = {c: min(int(p["plane_off"]) for p in tab if p["tcomp"] == c) for c in range(len(dims))}
    plan = {(int(p["tcomp"]), int(p["plane_off"]) - base[int(p["tcomp"])]): p for p in tab}
    out = []
    for b in blocks:
        e = plan.get((b["comp"], b["y"] * dims[b["comp"]][0] + b["x"]))
        out.append(None if e is None or not e["lcup"] else (int(e["zbp"]), int(e["npasses"])))
    return out


def budget_case(enc, orc, decs, fmt, bits, w, h, levels, cb, irreversible, passes):
    comps = synth(fmt, w, h, bits)
    planes = em.to_planes(comps, fmt, bits)
    opts = dict(levels=levels, cb=cb, irreversible=irreversible, qstep=0.25)
    free = enc.encode(planes, fmt, bits, **opts)
    multi = 0
    for share in BUDGETS:
        target = int(len(free) * share)
        cs = enc.encode(planes, fmt, bits, target_bytes=target, ht_passes=passes, **opts)
        info = enc.rc_info(0)
        assert len(cs) <= target and info["final_bytes"] == len(cs) and 1 <= info["ht_launches"] <= 3
        again, coded, blocks = rebuild(enc, comps, fmt, bits, w, h, opts, cs)
        assert again == cs, (fmt, share, passes)
        g = em.qcd_guard_bits(cs)
        want = [None if not c[1] else (b["expn"] + g - 2 - p - (k > 1), k)
                for b, c, p, k in zip(blocks, coded, enc.last_planes(0), enc.last_passes(0))]
        assert parsed_passes(orc, cs, fmt, w, h, blocks) == want
        assert max(enc.last_passes(0)) <= passes
        multi += sum(k > 1 for k in enc.last_passes(0))
        check_decodes(cs, fmt, orc, decs)
    for target in (len(free), len(free) + 100):
        assert enc.encode(planes, fmt, bits, target_bytes=target, ht_passes=passes, **opts) == free
    return multi


@pytest.mark.parametrize("irreversible", [False, True])
@pytest.mark.parametrize("fmt,bits", FRAMES)
def test_160x96_under_a_budget(enc, orc, fmt, bits, irreversible):
    decs = {}
    multi = sum(budget_case(enc, orc, decs, fmt, bits, 160, 96, 3, (4, 4), irreversible, k) for k in (2, 3))
    assert multi > 0                                          # the allocation does take the new candidates
    for d in decs.values():
        d.close()


@pytest.mark.parametrize("irreversible", [False, True])
@pytest.mark.parametrize("fmt,bits", [("gray", 8), ("rgb24", 8)])
def test_512x384_under_a_budget(enc, orc, fmt, bits, irreversible):
    decs = {}
    multi = sum(budget_case(enc, orc, decs, fmt, bits, 512, 384, 5, (6, 6), irreversible, k) for k in (2, 3))
    assert multi > 0
    for d in decs.values():
        d.close()


@pytest.mark.parametrize("irreversible", [False, True])
def test_correction_round_recodes_blocks_of_several_passes(enc, orc, irreversible):
    """one byte below the unconstrained size: a trial at plane 0 and one pass, one byte over, selected again with the
    passes among the candidates; the stream must be what its planes and passes say"""
    decs = {}
    for fmt, bits, w, h, levels, cb in [("rgb24", 8, 160, 96, 3, (4, 4)), ("gray", 8, 512, 384, 5, (6, 6))]:
        comps = synth(fmt, w, h, bits)
        planes = em.to_planes(comps, fmt, bits)
        opts = dict(levels=levels, cb=cb, irreversible=irreversible, qstep=0.25)
        free = enc.encode(planes, fmt, bits, **opts)
        cs = enc.encode(planes, fmt, bits, target_bytes=len(free) - 1, ht_passes=3, **opts)
        info = enc.rc_info(0)
        print(fmt, irreversible, info, sorted(set(zip(enc.last_planes(0), enc.last_passes(0)))))
        assert len(cs) < len(free) and info["trial"] == 1 and info["ht_launches"] >= 2 and info["blocks_recoded"] > 0
        assert rebuild(enc, comps, fmt, bits, w, h, opts, cs)[0] == cs
        check_decodes(cs, fmt, orc, decs)
    for d in decs.values():
        d.close()


def test_budgeted_batch_rounds_tiles_and_determinism(enc, orc, monkeypatch):
    fmt, bits = "rgb24", 8
    sizes = [(160, 96), (97, 61), (33, 140)]
    planes = [em.to_planes(synth(fmt, w, h, bits, seed=3 + i), fmt, bits) for i, (w, h) in enumerate(sizes)]
    opts = dict(levels=3, cb=(4, 4), irreversible=True, qstep=0.25, ht_passes=3)
    singles = []
    for p in planes:
        free = enc.encode(p, fmt, bits, **dict(opts, ht_passes=1))
        singles.append(free)
    target = min(len(s) for s in singles) // 2
    one = [enc.encode(p, fmt, bits, target_bytes=target, **opts) for p in planes]
    batch = enc.encode_batch(planes, fmt, bits, target_bytes=target, **opts)
    assert batch == one and all(len(b) <= target for b in batch)
    assert enc.encode_batch(planes, fmt, bits, target_bytes=target, **opts) == batch
    assert any(k > 1 for i in range(3) for k in enc.last_passes(i))
    monkeypatch.setenv("HTJ2K_ENC_ROUND", "20000")
    e2 = m.Encoder(0)
    try:
        assert e2.encode_batch(planes, fmt, bits, target_bytes=target, **opts) == batch
    finally:
        e2.close()
    decs = {}
    cs = enc.encode(planes[0], fmt, bits, target_bytes=target, tile=(64, 48), **opts)
    assert len(cs) <= target and max(enc.last_passes(0)) <= 3
    check_decodes(cs, fmt, orc, decs)
    for d in decs.values():
        d.close()


# ---------------------------------------------------------------------------------------------- fill and quality

def psnr_of(dec, cs, planes, bits):
    _, got, _, st = dec.decode(cs)
    assert st.n_block_errors == 0
    return rc.psnr(got, planes, bits)


def model_stream(lens, dists, cands, idx, blocks, room, target, w, h, fmt, bits, opts):
    """the model's allocation as a stream that keeps the budget (tests/test_encode_rc_gpu.py: fill_and_quality)"""
    for _ in range(8):
        mp, mk = pm.chosen(rc.allocate(lens, dists, room), cands)
        coded = [pm.code_block(rc.block_view(idx, b), p, k) for b, p, k in zip(blocks, mp, mk)]
        mcs = pm.assemble(coded, w, h, fmt, bits, planes=mp, **opts)
        if len(mcs) <= target:
            break
        room -= len(mcs) - target
    assert len(mcs) <= target
    return mcs


def fill_and_quality(enc, fmt, w, h, levels, cb, irreversible, q):
    """product against the extended model and against the product's own one-pass call at the four budgets -> rows"""
    bits = 8
    comps = synth(fmt, w, h, bits)
    planes = em.to_planes(comps, fmt, bits)
    mct = em.mct_default(fmt)
    dec = m.Decoder(device_id=0, req_pix_fmt=em.pix(fmt))
    opts = dict(levels=levels, cb=cb, irreversible=irreversible, qstep=q)
    free = enc.encode(planes, fmt, bits, **opts)
    blocks = m.Encoder.layout(w, h, fmt, bits, **opts)
    idx = rc.indices(comps, fmt, bits, levels, mct, irreversible, q)
    wts = rc.weights(fmt, w, h, bits, levels, mct, irreversible, q)
    tabs = {k: pm.tables(idx, blocks, wts, k) for k in (1, 2, 3)}
    rows = []
    for share in BUDGETS:
        target = int(len(free) * share)
        res = {}
        for k in (1, 2, 3):
            cs = enc.encode(planes, fmt, bits, target_bytes=target, ht_passes=k, **opts)
            segs = sum(sum(pm.code_block(rc.block_view(idx, b), p, kk)[1:3])
                       for b, p, kk in zip(blocks, enc.last_planes(0), enc.last_passes(0)))
            mcs = model_stream(*tabs[k], idx, blocks, target - (len(cs) - segs), target, w, h, fmt, bits, opts)
            res[k] = dict(size=len(cs), fill=len(cs) / target, psnr=psnr_of(dec, cs, planes, bits), model_fill=len(mcs) / target,
                          model_psnr=psnr_of(dec, mcs, planes, bits), launches=enc.rc_info(0)["ht_launches"],
                          share=[sum(x == j for x in enc.last_passes(0)) for j in (1, 2, 3)])
        rows.append(dict(fmt=fmt, w=w, irreversible=irreversible, q=q, share=share, target=target, res=res))
    dec.close()
    return rows


# the worst shortfall of the product's fill against the extended model's, and of its PSNR (dB), over the cases below (table
# in DESIGN.md 3.5), measured with this test on an MI355X: fill at the 10 % budget of gray 512 x 384 at qstep 1, PSNR at the 50 % budget of rgb24 160 x 96
FILL_SHORTFALL, PSNR_GAP = 0.0509, 0.1930

QUALITY = [("gray", 512, 384, 5, (6, 6), True, 0.25), ("gray", 512, 384, 5, (6, 6), True, 1.0),
           ("gray", 512, 384, 5, (6, 6), False, 1.0), ("rgb24", 160, 96, 3, (4, 4), True, 0.25)]


@pytest.mark.parametrize("fmt,w,h,levels,cb,irreversible,q", QUALITY)
def test_fill_and_quality_against_the_model(enc, fmt, w, h, levels, cb, irreversible, q):
    rows = fill_and_quality(enc, fmt, w, h, levels, cb, irreversible, q)
    fill_tol, psnr_tol = max(1.25 * FILL_SHORTFALL, 0.01), max(1.25 * PSNR_GAP, 0.1)
    for r in rows:
        print(r["fmt"], r["w"], "9/7 %g" % r["q"] if r["irreversible"] else "5/3", r["share"], r["target"])
        for k in (1, 2, 3):
            print("   ", k, {a: (round(b, 4) if isinstance(b, float) else b) for a, b in r["res"][k].items()})
    for r in rows:
        one = r["res"][1]
        for k in (2, 3):
            x = r["res"][k]
            assert x["size"] <= r["target"] and x["launches"] <= 3
            assert x["model_fill"] - x["fill"] <= fill_tol, (r["share"], k, x)
            assert x["model_psnr"] - x["psnr"] <= psnr_tol, (r["share"], k, x)
            # against one pass: never worse by more than the model itself loses in this case, plus 0.1 dB
            deficit = max(0.0, one["model_psnr"] - x["model_psnr"])
            assert one["psnr"] - x["psnr"] <= deficit + 0.1, (r["share"], k, one, x)
