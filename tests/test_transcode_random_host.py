"""The seeded random sources of the transcoder (tests/xc_random.py) on the CPU, no GPU: the verdict of
htj2k_transcode_check on every draw, and the reference tools/gpu_transcode_random.py compares the GPU with -- the output
rebuilt from the source's indices (tests/xc_source.py) -- pinned before the GPU relies on it: it decodes to the source's
frame, keeps the check's bound, reads the same in both parsers, and does not depend on the source's container.  The
seeds and the draws per seed are the ones tests/test_transcode_random_gpu.py runs."""
import shutil
from collections import Counter

import numpy as np
import pytest

import cs_rewrite
import ffmpeg_ht_amd as m
import vecgen
import xc_random as xr
from test_plan_equality import plan_diff  # noqa: F401  (the fixture: both parsers on a list of files)
from xc_source import Source

SEEDS = (40, 104)
DRAWS = 200
CAP = 0.05                                                 # of a seed's draws may be left out


_runs = {}


@pytest.fixture(scope="module", params=SEEDS)
def run(request, orc):
    """a seed's draws, each prepared once -> (seed, [(draw, prepared)])"""
    seed = request.param
    if seed not in _runs:
        draws = [xr.draw(np.random.default_rng([seed, i])) for i in range(DRAWS)]
        _runs[seed] = [(d, xr.prepare(orc, d)) for d in draws]
    return seed, _runs[seed]


def answer(call, src, ht_sources):
    try:
        return 0, call(src, ht_sources=ht_sources)
    except m.Htj2kError as e:
        return e.code, str(e)


def test_verdict(run, orc):
    """htj2k_transcode_check, with and without ht_sources, and htj2k_transcode_min_size give every draw the code, and a
    refused one a word of the log line, that predicted() reads off the draw's parameters"""
    seed, items = run
    seen = Counter()
    for i, (d, p) in enumerate(items):
        if p["status"] == "factory":
            continue
        for ht in (True, False):
            code, word = xr.predicted(d, ht_sources=ht, orc=orc, src=p["src"])
            if not code and p["status"] == "headroom":
                code, word = xr.PATCHWELCOME, "fills all"
            for call in (m.Encoder.transcode_check, m.Encoder.transcode_min_size):
                got, what = answer(call, p["src"], ht)
                assert got == code, (seed, i, ht, xr.describe(d), what)
                assert code == 0 or word in what, (seed, i, ht, xr.describe(d), what)
            seen[word] += 1
    assert set(seen) >= set(xr.WORDS.values()) - {xr.WORDS["reduce"]}, seen        # (the reduction factor is the decoder's)


def test_the_reference(run, orc, plan_diff, tmp_path):
    """the rebuilt output of every draw in scope: the oracle decodes it without a block error to exactly the source's
    frame (9/7: bitexact 0 and 1), it is no longer than the check's bound, the stream with every block left out has the
    length htj2k_transcode_min_size reports, and both parsers read the same plan from it"""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    seed, items = run
    files = []
    for i, (d, p) in enumerate(items):
        if p["status"] != "ok":
            continue
        s = p["s"]
        ref = s.free()
        for bitexact in ((0, 1) if s.opts["irreversible"] else (0,)):
            _, want, _ = orc.decode(s.src, bitexact=bitexact)
            assert orc.block_errors() == 0
            info, got, _ = orc.decode(ref, bitexact=bitexact)
            assert orc.block_errors() == 0 and info.is_ht == 1, (seed, i)
            assert len(want) == len(got) and all(np.array_equal(a, b) for a, b in zip(want, got)), (seed, i, xr.describe(d))
        assert len(ref) <= m.Encoder.transcode_check(s.src, ht_sources=True), (seed, i)
        assert len(s.empty()) == m.Encoder.transcode_min_size(s.src, ht_sources=True), (seed, i)
        f = tmp_path / ("%d_%d.j2c" % (seed, i))
        f.write_bytes(ref)
        files.append(f)
    parses, accepted = plan_diff(files, 0)                  # (asserts that no plan differs)
    assert parses >= accepted >= 2 * len(files)             # every file as it is under several options; bitexact 0 and 1 always parse


def test_a_variant_gives_the_streams_of_its_source(run, orc):
    """the output rebuilt from a container variant equals the one rebuilt from the stream the variant was made of"""
    seed, items = run
    n = 0
    for i, (d, p) in enumerate(items):
        if p["status"] == "ok" and d["variant"] is not None:
            plain = Source(orc, xr.make(d, rewritten=False), d["kw"])
            assert plain.src != p["src"] or d["variant"] == "same", (seed, i)
            assert plain.free() == p["s"].free() and plain.empty() == p["s"].empty(), (seed, i, d["variant"])
            n += 1
    assert n >= 2 * len(xr.IN_VARIANTS)


def test_draws_left_out(run, orc):
    """a draw is left out only where the vector factory refuses it, or where the oracle's block table has a Part-1
    block with zbp >= M_b and the check says so; at most 5 % of a seed's draws"""
    seed, items = run
    left = [(d, p) for d, p in items if p["status"] in ("factory", "headroom")]
    for d, p in left:
        if p["status"] == "factory":
            assert "htj2k_encode failed" in p["why"], xr.describe(d)
        else:
            assert xr.headroom(orc.plan_blocks(p["src"]))
            code, what = answer(m.Encoder.transcode_check, p["src"], True)
            assert code == xr.PATCHWELCOME and "fills all" in what and "one more guard bit" in what, what
    print(seed, Counter(p["status"] for _, p in items), Counter(d["kind"] for d, p in items if p["status"] == "ok"))
    assert len(left) <= CAP * DRAWS, len(left)


def test_a_draw_without_headroom(orc):
    """the second reason met on purpose (the chosen seeds may hold none): among another seed's Part-1 draws with one guard
    bit, the first whose oracle table has a block that fills its band; the check says so with and without ht_sources"""
    for i in range(DRAWS):
        d = xr.draw(np.random.default_rng([11, i]))
        if d["out"] is None and d["kind"] == "p1" and d["kw"]["guard_bits"] == 1:
            p = xr.prepare(orc, d)
            if p["status"] == "headroom":
                for ht in (True, False):
                    code, what = answer(m.Encoder.transcode_check, p["src"], ht)
                    assert code == xr.PATCHWELCOME and "fills all" in what, what
                return
    assert False, "no such draw"


def test_tlm_of_more_than_255_tile_parts(orc):
    """found by a draw (seed 13, draw 127: 288 tiles in three tile-parts each): the reference counts a TLM segment's
    records in a byte, so the rewriter writes segments of at most 255; 180 tiles in three tile-parts read as their source"""
    kw = dict(part1=True, nlevels=2, cb=(2, 2), tile=(8, 8), sop=True, eph=True)
    src = vecgen.encode(vecgen.synth_image(120, 96, 1, seed=3), **kw)
    v = dict(cs_rewrite.variants(src, False))["tp3_tlm_plt"]
    assert v.count(b"\xff\x55") >= 3 and m.Encoder.transcode_check(v) == m.Encoder.transcode_check(src)
    assert Source(orc, v, kw).free() == Source(orc, src, kw).free()


def test_coverage(run):
    """what a seed's draws must hold, so that a later edit of the generator cannot empty the net"""
    seed, items = run
    draws = [d for d, _ in items]
    ok = [(d, p["s"]) for d, p in items if p["status"] == "ok"]
    n = len(draws)
    share = lambda f, of=draws: sum(1 for d in of if f(d)) / len(of)
    for kind in ("p1", "ht", "mixed"):
        assert share(lambda d: d["kind"] == kind) >= 0.2, kind
    styles = Counter(d["kw"]["cblk_style"] for d in draws if d["kind"] == "p1")
    assert all(styles[v] >= 2 for v in set(xr.STYLES)), styles
    progs = Counter(d["kw"]["prog"] for d in draws)
    assert all(progs[v] >= 2 for v in range(5)), progs
    names = Counter(d["variant"] for d in draws)
    assert all(names[v] >= 2 for v in xr.IN_VARIANTS) and all(names[v] >= 1 for v in xr.OUT_VARIANTS), names
    assert share(lambda d: d["kw"]["tile"] != (0, 0)) >= 0.15
    assert share(lambda d: d["kw"].get("layers", 1) > 1) >= 0.15
    assert share(lambda d: any(v > 1 for v in d["kw"]["dx"] + d["kw"]["dy"])) >= 0.15
    assert share(lambda d: d["kw"]["transform"] == 0) >= 0.15
    wide = sum(1 for _, s in ok if any(b["w"] > 64 for b in s.layout))
    assert wide >= 0.1 * len(ok), (wide, len(ok))
    forms = [f for _, s in ok for f in s.forms()]
    assert any(k > 1 and not lo for _, k, lo, _ in forms) and any(lo for _, _, lo, _ in forms)
    assert len({d["bits"] for d in draws}) >= 5
    assert len(ok) >= 0.75 * n                              # one draw in eight is out of scope on purpose
    print(seed, dict(draws=n, in_scope=len(ok), wide=wide, blocks=len(forms), multi_pass=sum(k > 1 and not lo for _, k, lo, _ in forms),
                     left_out_blocks=sum(lo for _, _, lo, _ in forms), depths=sorted({d["bits"] for d in draws}),
                     out=Counter(d["out"] for d in draws if d["out"])))
