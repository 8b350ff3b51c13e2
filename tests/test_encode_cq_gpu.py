"""GPU checks of the encoder's constant-quality mode (htj2k_enc_opts.target_psnr): k_rc_base97 against the numpy model,
the guarantee D <= D_target recomputed exactly from the planes and passes the encoder reports, the stream rebuilt on the
CPU, decoding by the product and the oracle, the bytes spent against the reference allocation of tests/cq_model.py,
the decoded PSNR against the model's, passes and tiles, the budget as a cap, batches, rounds, determinism and I/O.

The reference data of a frame (coefficients, indices, weights, the quantiser's own error, the candidates' tables) is
computed once and shared; so is every encode that several tests look at."""
import ctypes
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

import cq_model as cq
import enc_model as em
import ffmpeg_ht_amd as m
import rc_model as rc
import rc_passes_model as pm
import vecgen
from test_encode_rc_gpu import check_decodes, synth

pytestmark = pytest.mark.gpu

LEVELS = 3
# (layout, bits, w, h, code-block log2): the last one has more blocks (1476) than k_rc_select_q has threads
FRAMES = [("rgb24", 8, 160, 96, (4, 4)), ("rgb24", 8, 75, 41, (4, 4)), ("gray", 8, 200, 136, (4, 4)),
          ("yuv420p10le", 10, 160, 96, (2, 2))]
SETTINGS = [dict(irreversible=True, qstep=0.25), dict(irreversible=True, qstep=1.0), dict(irreversible=False)]
ABOVE = 99.0                                 # above the base PSNR of every 9/7 case here (5/3 has none and is never short)
TARGETS = (32.0, 38.0, 44.0, ABOVE)
FS = [(fi, si) for fi in range(len(FRAMES)) for si in range(len(SETTINGS))]
FS_IDS = ["%s-%dx%d-%s" % (FRAMES[fi][0], FRAMES[fi][2], FRAMES[fi][3],
                           "53" if not SETTINGS[si]["irreversible"] else "97q%g" % SETTINGS[si]["qstep"]) for fi, si in FS]


@pytest.fixture(scope="module")
def enc():
    e = m.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def decs():
    d = {}
    yield d
    for x in d.values():
        x.close()


@functools.lru_cache(maxsize=None)
def ref(fi, si, tile=(0, 0)):
    """everything the checks need of frame fi under setting si, from the models"""
    fmt, bits, w, h, cb = FRAMES[fi]
    st = SETTINGS[si]
    irrev, q, mct = st["irreversible"], st.get("qstep", 1.0), em.mct_default(fmt)
    opts = dict(levels=LEVELS, cb=cb, **st)
    if tile != (0, 0):
        opts["tile"] = tile
    comps = synth(fmt, w, h, bits, seed=fi + 1)
    blocks = m.Encoder.layout(w, h, fmt, bits, **opts)
    wts = m.Encoder.band_weights(w, h, fmt, bits, **opts)
    bases = [0.0] * len(blocks)
    if irrev:
        bases = cq.frame_base(cq.float_planes(comps, fmt, w, h, bits, LEVELS, mct, tile), blocks,
                              cq.block_steps(blocks, q, bits, LEVELS))
    return SimpleNamespace(fmt=fmt, bits=bits, w=w, h=h, opts=opts, comps=comps, planes=em.to_planes(comps, fmt, bits),
                           idx=cq.index_planes(comps, fmt, w, h, bits, LEVELS, mct, irrev, q, tile), blocks=blocks,
                           wts=wts, bases=bases, dbase=float(sum(a * b for a, b in zip(wts, bases))))


@functools.lru_cache(maxsize=None)
def tables(fi, si):
    """(lens, dists) of the reference allocation: exact bytes, and w d / 4 with the product's weights"""
    r = ref(fi, si)
    wd = {(b["comp"], rc.band_entry(b)): float(x) for b, x in zip(r.blocks, r.wts)}
    lens, dists = rc.tables(r.idx, r.blocks, wd)
    return lens, [[d / 4.0 for d in row] for row in dists]


_runs = {}


def run(enc, fi, si, target, tile=(0, 0), **extra):
    """the quality call of a case (once): bytes and what the encoder reports of it"""
    key = (fi, si, target, tile, tuple(sorted(extra.items())))
    if key not in _runs:
        r = ref(fi, si, tile)
        cs = enc.encode(r.planes, r.fmt, r.bits, target_psnr=target, **r.opts, **extra)
        _runs[key] = SimpleNamespace(cs=cs, planes=enc.last_planes(0), passes=enc.last_passes(0), q=enc.quality_info(0),
                                     rc=enc.rc_info(0))
    return _runs[key]


def same_db(a, b):
    return (math.isinf(a) and math.isinf(b) and a > 0 and b > 0) or abs(a - b) <= 1e-6


def check_guarantee(r, out, target):
    """D recomputed from the reported planes and passes, the product's weights and the models' distortions"""
    d = cq.frame_d(r.idx, r.blocks, r.wts, r.bases, out.planes, out.passes)
    dt = cq.d_target(target, r.fmt, r.w, r.h, r.bits)
    q = out.q
    print("%s %dx%d %s target %g: D %.6g D_target %.6g base %.3f dB model %.3f dB lambda %.4g short %d bytes %d" %
          (r.fmt, r.w, r.h, r.opts, target, d, dt, q["base_psnr"], q["model_psnr"], q["lambda"], q["short_of_target"], len(out.cs)))
    if q["short_of_target"]:
        assert r.dbase > dt and out.planes == [0] * len(r.blocks) and out.passes == [1] * len(r.blocks) and q["lambda"] == 0
    else:
        assert d <= dt * (1 + 1e-9)
    assert q["target_psnr"] == target and q["capped"] == 0
    assert same_db(q["model_psnr"], cq.psnr(d, r.fmt, r.w, r.h, r.bits)), (q, d)
    assert same_db(q["base_psnr"], cq.psnr(r.dbase, r.fmt, r.w, r.h, r.bits)), (q, r.dbase)
    return d


def rebuild(r, out):
    """the stream again on the CPU from the planes and passes the encoder reports"""
    coded = []
    for b, p, k in zip(r.blocks, out.planes, out.passes):
        if k > 1:
            coded.append(pm.code_block(rc.block_view(r.idx, b), p, k))
        else:
            data, lcup, mu = rc.code_block(rc.block_view(r.idx, b), p)
            coded.append((data, lcup, 0, mu, 1))
    assert [c[4] for c in coded] == out.passes               # the selection never picks a candidate that falls back
    return pm.assemble(coded, r.w, r.h, r.fmt, r.bits, planes=out.planes, guard_bits=em.qcd_guard_bits(out.cs), **r.opts)


# ---------------------------------------------------------------------------------------------- 1. k_rc_base97

def base_cases():
    """(name, float32 plane, rects): the block shapes the kernel's loop takes differently, at offsets that are no multiple
    of 4; magnitudes up to 2^23 steps, exact multiples of the step, +-0 and values just under one step among them"""
    rng = np.random.default_rng(17)

    def fill(h, w, step):
        scale = 2.0 ** rng.integers(-6, 23, size=(h, w))
        v = (rng.standard_normal((h, w)) * scale).clip(-2.0 ** 23, 2.0 ** 23) * step
        kind = rng.integers(0, 8, size=(h, w))
        v = np.where(kind == 0, np.round(v / step) * step, v)                       # multiples of the step
        v = np.where(kind == 1, 0.0, v)
        v = np.where(kind == 2, -0.0, v)
        v = np.where(kind == 3, np.sign(v) * step * (1 - 2.0 ** -20), v)            # just under one step
        return v.astype(np.float32)

    out = []
    for step in (1 / 32, 1.0, 3.7):
        out.append(("96x96 step %g" % step, fill(96, 96, step), step,
                    [(5, 7, 1, 1), (9, 2, 1, 7), (13, 11, 3, 5), (41, 3, 33, 17), (31, 29, 64, 64), (1, 1, 7, 1), (0, 0, 96, 42)]))
        out.append(("1024x4 step %g" % step, fill(8, 2048, step), step, [(5, 3, 1024, 4), (1021, 1, 1024, 4), (0, 0, 1024, 4)]))
        out.append(("4x1024 step %g" % step, fill(2048, 8, step), step, [(3, 5, 4, 1024), (1, 1021, 4, 1024), (0, 0, 4, 1024)]))
    return out


def test_rc_base_against_the_model(enc):
    tol = 4096 * 2.0 ** -52              # the order of a double sum of at most 4096 non-negative terms, nothing else
    for name, plane, step, rects in base_cases():
        assert float(np.abs(plane).max()) / step < 2.0 ** 24
        got = enc.rc_base(plane, rects, [step] * len(rects))
        for g, (x, y, w, h) in zip(got, rects):
            want = cq.base(plane[y:y + h, x:x + w], step)
            assert abs(g - want) <= tol * want, (name, (x, y, w, h), g, want)
    # every block with its own step
    name, plane, _, rects = base_cases()[0]
    steps = [1 / 32, 1.0, 3.7, 0.5, 0.25, 17.0, 2.0]
    got = enc.rc_base(plane, rects, steps)
    for g, (x, y, w, h), s in zip(got, rects, steps):
        want = cq.base(plane[y:y + h, x:x + w], s)
        assert abs(g - want) <= tol * want, ((x, y, w, h), s)
    z = np.zeros((8, 8), np.float32)
    assert enc.rc_base(z, [(0, 0, 8, 8)], [1.0]).tolist() == [0.0]


def test_rc_base_refuses_what_rc_stats_refuses(enc):
    z = np.zeros((8, 8), np.float32)
    for rect in [(0, 0, 9, 8), (1, 0, 8, 8), (0, 0, 0, 4), (-1, 0, 4, 4)]:
        with pytest.raises(m.Htj2kError) as e:
            enc.rc_base(z, [rect], [1.0])
        assert e.value.code == -22, rect
    for step in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(m.Htj2kError) as e:
            enc.rc_base(z, [(0, 0, 8, 8)], [step])
        assert e.value.code == -22, step
    tab = (m.EncBlock * 1)()
    tab[0].w = tab[0].h = 8
    st, out = (ctypes.c_float * 1)(1.0), (ctypes.c_double * 1)()
    p = z.ctypes.data_as(ctypes.c_void_p)
    assert enc.L.htj2k_enc_rc_base(None, p, 8, 8, tab, 1, st, out) == -38          # fine arguments, no context
    assert enc.L.htj2k_enc_rc_base(enc.h, None, 8, 8, tab, 1, st, out) == -22
    assert enc.L.htj2k_enc_rc_base(enc.h, p, 8, 8, tab, 1, None, out) == -22
    assert enc.L.htj2k_enc_rc_base(enc.h, p, 8, 8, tab, 1, st, None) == -22
    assert enc.L.htj2k_enc_rc_base(enc.h, p, 8, 8, None, 0, None, None) == 0


def test_the_quantiser_is_unchanged(enc):
    """k_rc_base97 reads the floats ahead of k_quant97 and writes none: the indices of a quality call are the model's (the
    stream of a call that is short of its target is the CPU rebuild from rc.indices at plane 0, and the plain call's)"""
    for fi in range(len(FRAMES)):
        for si in (0, 1):
            r, out = ref(fi, si), run(enc, fi, si, ABOVE)
            assert out.q["short_of_target"] == 1 and out.planes == [0] * len(r.blocks)
            assert rebuild(r, out) == out.cs == enc.encode(r.planes, r.fmt, r.bits, **r.opts)


# ---------------------------------------------------------------------------------------------- 2. the guarantee

@pytest.mark.parametrize("fi,si", FS, ids=FS_IDS)
def test_the_guarantee_exactly(enc, orc, decs, fi, si):
    r = ref(fi, si)
    shorts = 0
    for target in TARGETS:
        out = run(enc, fi, si, target)
        check_guarantee(r, out, target)
        shorts += out.q["short_of_target"]
        assert out.rc["target_bytes"] == 0 and out.rc["ht_launches"] == 1 and out.rc["final_bytes"] == len(out.cs)
        assert out.rc["est_bytes"] > 0 and out.rc["trial"] == 0 and out.rc["blocks_recoded"] == 0 and out.rc["last_resort"] == 0
        assert out.rc["blocks_left_out"] == sum(p < 0 for p in out.planes)
        assert rebuild(r, out) == out.cs, (fi, si, target)
        check_decodes(out.cs, r.fmt, orc, decs)
    # short of the target exactly where the quantiser's own error is beyond it: at ABOVE in every 9/7 case (at 44 dB too
    # with qstep 1 on the rgb24 frames); 5/3 has no base error and is never short
    assert shorts == sum(r.dbase > cq.d_target(t, r.fmt, r.w, r.h, r.bits) for t in TARGETS)
    assert shorts >= 1 if SETTINGS[si]["irreversible"] else shorts == 0
    if not SETTINGS[si]["irreversible"]:
        out = run(enc, fi, si, 400.0)                        # D_target below what dropping any one plane of any block costs
        check_guarantee(r, out, 400.0)
        assert math.isinf(out.q["base_psnr"]) and math.isinf(out.q["model_psnr"]) and out.planes == [0] * len(r.blocks)
        assert out.cs == enc.encode(r.planes, r.fmt, r.bits, **r.opts)             # lossless


# ---------------------------------------------------------------------------------------------- 3. it does not overspend

def reference_stream(fi, si, target):
    """the reference allocation's stream: exact lengths, the same constraint -> (bytes, D)"""
    r = ref(fi, si)
    lens, dists = tables(fi, si)
    dt = cq.d_target(target, r.fmt, r.w, r.h, r.bits)
    sel = cq.allocate(lens, dists, dt - r.dbase)
    planes = [0] * len(r.blocks) if sel is None else rc.planes_of(sel, lens)
    coded = [rc.code_block(rc.block_view(r.idx, b), p) for b, p in zip(r.blocks, planes)]
    cs = m.Encoder.assemble(r.w, r.h, r.fmt, r.bits, [c[0] for c in coded], max_u=[c[2] for c in coded], planes=planes, **r.opts)
    d = cq.frame_d(r.idx, r.blocks, r.wts, r.bases, planes, [1] * len(planes))
    assert sel is None or d <= dt * (1 + 1e-9)               # the reference itself meets the target
    return cs, d


# measured on the MI355X (table in DESIGN.md 3.5, "Constant quality"): the worst size / reference size - 1 over the 48 cases
OVERSPEND = 0.0326


@pytest.mark.parametrize("fi,si", FS, ids=FS_IDS)
def test_bytes_against_the_reference_allocation(enc, fi, si):
    r = ref(fi, si)
    tol = max(1.25 * OVERSPEND, 0.01)
    outs = [run(enc, fi, si, t) for t in TARGETS]
    overs = []
    for target, out in zip(TARGETS, outs):
        mcs, md = reference_stream(fi, si, target)
        over = len(out.cs) / len(mcs) - 1
        print("%s %dx%d %s target %g: %d bytes, reference %d, over %.4f; model %.3f dB, reference %.3f dB" %
              (r.fmt, r.w, r.h, FS_IDS[FS.index((fi, si))], target, len(out.cs), len(mcs), over, out.q["model_psnr"],
               cq.psnr(md, r.fmt, r.w, r.h, r.bits)))
        overs.append(over)
    assert max(overs) <= tol, overs
    # the bisection is monotone on exact sums: no tolerance
    for a, b in zip(outs, outs[1:]):
        assert len(a.cs) <= len(b.cs) and a.q["model_psnr"] <= b.q["model_psnr"] and a.q["lambda"] >= b.q["lambda"]


# ---------------------------------------------------------------------------------------------- 4. decoded PSNR

# measured on the MI355X ("Constant quality"): the worst model_psnr - decoded PSNR (dB) over the 8-bit cases
# at 32, 38 and 44 dB
PSNR_GAP = 1.0424


@pytest.mark.parametrize("fi,si", [x for x in FS if FRAMES[x[0]][1] == 8], ids=[i for x, i in zip(FS, FS_IDS) if FRAMES[x[0]][1] == 8])
def test_decoded_psnr_against_the_model(enc, decs, fi, si):
    r = ref(fi, si)
    pf = em.pix(r.fmt)
    if (pf, 0) not in decs:
        decs[pf, 0] = m.Decoder(device_id=0, req_pix_fmt=pf, bitexact=0)
    gaps = []
    for target in (32.0, 38.0, 44.0):
        out = run(enc, fi, si, target)
        _, got, _, st = decs[pf, 0].decode(out.cs)
        assert st.n_block_errors == 0
        decoded = rc.psnr(got, r.planes, r.bits)
        gap = 0.0 if math.isinf(out.q["model_psnr"]) and math.isinf(decoded) else out.q["model_psnr"] - decoded
        print("%s target %g: model %.3f dB decoded %.3f dB gap %.3f" % (FS_IDS[FS.index((fi, si))], target, out.q["model_psnr"], decoded, gap))
        gaps.append(gap)
    assert max(gaps) <= max(1.25 * PSNR_GAP, 0.1), gaps


# ---------------------------------------------------------------------------------------------- 5. passes and tiles

@pytest.mark.parametrize("si", [0, 2], ids=["97q0.25", "53"])
def test_passes(enc, orc, decs, si):
    r = ref(0, si)
    out = run(enc, 0, si, 38.0, ht_passes=3)
    check_guarantee(r, out, 38.0)
    assert max(out.passes) <= 3 and sum(k > 1 for k in out.passes) >= 1
    assert rebuild(r, out) == out.cs
    check_decodes(out.cs, r.fmt, orc, decs)
    one = run(enc, 0, si, 38.0)
    print("ht_passes 3: %d bytes, %d blocks of several passes; ht_passes 1: %d bytes" % (len(out.cs), sum(k > 1 for k in out.passes), len(one.cs)))
    assert len(out.cs) <= len(one.cs) * (1 + max(1.25 * OVERSPEND, 0.01))
    assert run(enc, 0, si, 38.0, ht_passes=1).cs == one.cs == run(enc, 0, si, 38.0, ht_passes=0).cs


@pytest.mark.parametrize("tile", [(64, 64), (0, 32)])
@pytest.mark.parametrize("si", [0, 2], ids=["97q0.25", "53"])
def test_tiles(enc, orc, decs, si, tile):
    r = ref(0, si, tile)
    assert len(m.Encoder.tiles(r.w, r.h, r.fmt, r.bits, **r.opts)) in (6, 3)
    for target in (38.0, ABOVE):
        out = run(enc, 0, si, target, tile)
        check_guarantee(r, out, target)
        assert rebuild(r, out) == out.cs
        check_decodes(out.cs, r.fmt, orc, decs)


# ---------------------------------------------------------------------------------------------- 6. the budget as a cap

@pytest.mark.parametrize("si", [0, 2], ids=["97q0.25", "53"])
@pytest.mark.parametrize("passes", [1, 3])
def test_the_budget_is_a_cap(enc, si, passes):
    r = ref(0, si)
    kw = dict(r.opts, ht_passes=passes)
    free = enc.encode(r.planes, r.fmt, r.bits, target_psnr=44.0, **kw)
    qfree = enc.quality_info(0)
    assert qfree["capped"] == 0 and qfree["short_of_target"] == 0
    # a cap the quality selection stays under: the quality-only frame
    assert enc.encode(r.planes, r.fmt, r.bits, target_psnr=44.0, target_bytes=2 * len(free), **kw) == free
    q, info = enc.quality_info(0), enc.rc_info(0)
    assert q == qfree and info["target_bytes"] == 2 * len(free) and info["ht_launches"] == 1 and info["final_bytes"] == len(free)
    # a cap below it: the frame of the call with the budget alone, and its rc_info
    for budget in (len(free) // 2, len(free) - 1):
        alone = enc.encode(r.planes, r.fmt, r.bits, target_bytes=budget, **kw)
        info_alone, planes_alone, passes_alone = enc.rc_info(0), enc.last_planes(0), enc.last_passes(0)
        cs = enc.encode(r.planes, r.fmt, r.bits, target_psnr=44.0, target_bytes=budget, **kw)
        q = enc.quality_info(0)
        assert len(cs) <= budget and cs == alone and q["capped"] == 1 and q["target_psnr"] == 44.0
        assert enc.rc_info(0) == info_alone and enc.last_planes(0) == planes_alone and enc.last_passes(0) == passes_alone
        # what the budget left is below the target, and the record says so in the model's terms
        out = SimpleNamespace(planes=planes_alone, passes=passes_alone)
        d = cq.frame_d(r.idx, r.blocks, r.wts, r.bases, out.planes, out.passes)
        assert same_db(q["model_psnr"], cq.psnr(d, r.fmt, r.w, r.h, r.bits))
        assert budget > len(free) // 2 or q["model_psnr"] < qfree["model_psnr"]
        assert same_db(q["base_psnr"], qfree["base_psnr"])
    # a budget below the smallest stream is still refused, the output untouched
    smallest = m.Encoder.assemble(r.w, r.h, r.fmt, r.bits, [b""] * len(r.blocks), **r.opts)
    fr, keep = m.frame_from_planes(r.planes, r.fmt)
    arr = (m.Frame * 1)(fr)
    buf = np.full(len(free) + 16, 0xAB, np.uint8)
    offs = (ctypes.c_size_t * 2)()
    for bad in (len(smallest) - 1, 1, -5):
        o = m._enc_opts(target_bytes=bad, target_psnr=44.0, **kw)
        ret = enc.L.htj2k_encode_batch(enc.h, arr, 1, r.bits, ctypes.byref(o), 0, buf.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.c_size_t(buf.size), 0, offs)
        assert ret == -22 and (buf == 0xAB).all(), bad
    for bad in (-1.0, float("nan"), float("inf")):
        o = m._enc_opts(target_psnr=bad, **kw)
        enc._logs.clear()
        ret = enc.L.htj2k_encode_batch(enc.h, arr, 1, r.bits, ctypes.byref(o), 0, buf.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.c_size_t(buf.size), 0, offs)
        assert ret == -22 and (buf == 0xAB).all() and any("PSNR target" in line for line in enc._logs), (bad, enc._logs)


# ---------------------------------------------------------------------------------------------- 7. batches, rounds, I/O

ROUND = 40000


@pytest.fixture(scope="module")
def enc_small_rounds():
    mp = pytest.MonkeyPatch()
    mp.setenv("HTJ2K_ENC_ROUND", str(ROUND))
    try:
        e = m.Encoder(0)
    finally:
        mp.undo()
    yield e
    e.close()


@pytest.mark.parametrize("kw", [dict(irreversible=True, qstep=0.25), dict(irreversible=False),
                                dict(irreversible=True, qstep=0.25, ht_passes=3, tile=(64, 64))], ids=["97", "53", "97-passes-tiles"])
def test_batches_rounds_and_determinism(enc, enc_small_rounds, kw):
    fmt, bits = "rgb24", 8
    sizes = [(160, 96), (160, 96), (75, 41), (75, 41)]
    frames = [em.to_planes(synth(fmt, w, h, bits, seed=10 + i), fmt, bits) for i, (w, h) in enumerate(sizes)]
    opts = dict(levels=LEVELS, cb=(4, 4), target_psnr=40.0, **kw)
    single, info, chosen = [], [], []
    for f in frames:
        single.append(enc.encode(f, fmt, bits, **opts))
        info.append((enc.quality_info(0), enc.rc_info(0)))
        chosen.append((enc.last_planes(0), enc.last_passes(0)))
    assert len(set(single)) == 4 and all(q["capped"] == 0 and q["short_of_target"] == 0 for q, _ in info)
    # one call of four frames of two sizes, in three rounds: 160 x 96 x 3 samples are beyond the knob, the small two share one
    assert 3 * 160 * 96 > ROUND >= 2 * 3 * 75 * 41
    assert enc_small_rounds.encode_batch(frames, fmt, bits, **opts) == single
    assert enc_small_rounds.last_rounds() >= 3
    for k in range(4):
        assert (enc_small_rounds.quality_info(k), enc_small_rounds.rc_info(k)) == info[k]
        assert (enc_small_rounds.last_planes(k), enc_small_rounds.last_passes(k)) == chosen[k]
    # shuffled, repeated three times, in one round and in several
    order = [2, 0, 3, 1, 1, 3, 0, 2]
    for e in (enc, enc_small_rounds):
        for _ in range(3):
            assert e.encode_batch([frames[i] for i in order], fmt, bits, **opts) == [single[i] for i in order]
            for k, i in enumerate(order):
                assert e.quality_info(k) == info[i][0]
    e2 = m.Encoder(0)
    try:
        assert [e2.encode(f, fmt, bits, **opts) for f in frames] == single
    finally:
        e2.close()


def test_device_input_equals_host_input(enc):
    comps = synth("yuv420p", 200, 120, 8, seed=6)
    planes = em.to_planes(comps, "yuv420p", 8)
    src = vecgen.encode(comps, **em.vecgen_args("yuv420p", 200, 120, 8, 4, (6, 6), False, 2))
    dec = m.Decoder(device_id=0)
    job = dec.job().parse(src).upload().run().wait()
    fr = m.Frame()
    assert dec.L.htj2k_job_device_frame(dec.h, job.h, 0, ctypes.byref(fr)) == 0
    fr.width, fr.height = 200, 120
    for irrev in (False, True):
        opts = dict(levels=4, cb=(4, 4), irreversible=irrev, qstep=0.5, target_psnr=36.0)
        host = enc.encode(planes, "yuv420p", 8, **opts)
        q = enc.quality_info(0)
        assert enc.encode_device([fr], "yuv420p", 8, **opts)[0] == host and enc.quality_info(0) == q
        assert q["short_of_target"] == 0 and sum(p != 0 for p in enc.last_planes(0)) > 0
    job.free()
    dec.close()


def test_target_zero_is_the_call_without_the_keyword(enc):
    for fi, si in [(0, 0), (0, 2), (3, 0)]:
        r = ref(fi, si)
        free = enc.encode(r.planes, r.fmt, r.bits, **r.opts)
        assert enc.encode(r.planes, r.fmt, r.bits, target_psnr=0, **r.opts) == free
        q = enc.quality_info(0)
        assert q == dict(target_psnr=0.0, base_psnr=0.0, model_psnr=0.0, short_of_target=0, capped=0, **{"lambda": 0.0})
        assert enc.quality_stage_ms() == [0.0, 0.0]
        budget = len(free) // 2
        alone = enc.encode(r.planes, r.fmt, r.bits, target_bytes=budget, **r.opts)
        info = enc.rc_info(0)
        assert enc.encode(r.planes, r.fmt, r.bits, target_bytes=budget, target_psnr=0.0, **r.opts) == alone
        assert enc.rc_info(0) == info and enc.quality_info(0) == q
        for k in (2, 3):
            alone = enc.encode(r.planes, r.fmt, r.bits, ht_passes=k, **r.opts)
            assert enc.encode(r.planes, r.fmt, r.bits, ht_passes=k, target_psnr=0.0, **r.opts) == alone


def test_stage_times_are_reported(enc):
    r = ref(2, 0)
    enc.encode(r.planes, r.fmt, r.bits, target_psnr=38.0, **r.opts)
    base_ms, select_ms = enc.quality_stage_ms()
    assert base_ms > 0 and select_ms > 0
    assert enc.rc_stage_ms()[0] > 0 and enc.rc_stage_ms()[1] == 0 and enc.rc_stage_ms()[2] == 0       # one HT launch, no budget runs
    r = ref(2, 2)
    enc.encode(r.planes, r.fmt, r.bits, target_psnr=38.0, **r.opts)
    assert enc.quality_stage_ms()[0] == 0 and enc.quality_stage_ms()[1] > 0                             # 5/3: no base kernel
