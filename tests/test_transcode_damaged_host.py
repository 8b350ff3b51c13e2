"""CPU checks of the damaged sources the transcoder tests use (tests/xc_damage.py; no GPU): what the oracle and
htj2k_transcode_check make of every draw, the conditions that keep tests/test_transcode_damaged_gpu.py from passing on
draws that are all refused, the two parsers' agreement on every draw, and that the check gives no bound for a stream the
oracle's parser refuses.  The seeds of tests/xc_damage.py were chosen against this file."""
import pytest

import cs_rewrite
import ffmpeg_ht_amd as m
import oracle
import xc_damage as xd
from test_plan_equality import plan_diff  # noqa: F401  (the fixture: both parsers on a list of files, no difference allowed)


@pytest.mark.parametrize("name", sorted(xd.SOURCES))
def test_sources(orc, name):
    """every source is in scope, decodes without a block error, and has packets whose headers and bodies are found"""
    src = xd.source(name)
    ht = xd.SOURCES[name][2]
    assert xd.outcome(orc, src, ht)[0] == "compared"
    assert orc.probe(src).is_ht == (1 if ht else 0)
    if ht:
        with pytest.raises(m.Htj2kError):
            m.Encoder.transcode_check(src)
        coders = {bool(e["flags"] & 4) for e in orc.plan_blocks(src) if e["npasses"]}
        assert coders == ({False, True} if name.startswith("mixed") else {False})
    heads, bodies, first_sod = xd._spans(src)
    assert len(bodies) >= xd.SOURCES[name][1]["nlevels"] + 1 and len(heads) >= len(bodies) and first_sod < bodies[0][0]
    assert cs_rewrite.Stream(src).build() == src


@pytest.mark.parametrize("name", sorted(xd.SOURCES))
def test_draws(name):
    """a draw has the source's length and differs from it, in the bytes its class names and in no others; the draws of
    a pair are the same on every call"""
    src = xd.source(name)
    heads, bodies, first_sod = xd._spans(src)
    inside = lambda p, spans: any(a <= p < b for a, b in spans)
    nbody = sum(b - a for a, b in bodies)
    for cls in xd.CLASSES[name]:
        got = xd.draws(name, cls)
        assert got == xd.draws(name, cls) and len(got) == (2 if cls == "d" else xd.DRAWS)
        for bad in got:
            assert len(bad) == len(src)
            diff = [p for p in range(len(src)) if src[p] != bad[p]]
            assert len(diff) <= {"a": 1, "b": 10, "c": nbody, "d": nbody, "e": 3, "f": 10}[cls]
            if cls in "abcd":
                assert all(inside(p, bodies) for p in diff)
            elif cls == "e":
                assert all(inside(p, heads) for p in diff)
            else:
                assert all(first_sod <= p < len(src) - 2 for p in diff)
            if cls in "cd":                                # nothing of the bodies is left: what stays equal is chance
                assert len(diff) > nbody // 2
        assert sum(bad != src for bad in got) >= len(got) - (cls in "ae")      # a byte may be set to the value it had


@pytest.mark.parametrize("name", sorted(xd.SOURCES))
def test_conditions(orc, name):
    """the counts of compared, failed, refused and noted draws per class meet xd.conditions; a stream the oracle's parser
    refuses never gets a bound from the check"""
    ht = xd.SOURCES[name][2]
    counts = {}
    for cls in xd.CLASSES[name]:
        outs, counts[cls] = xd.census(orc, name, cls)
        print(name, cls, counts[cls])
        for bad, o in zip(xd.draws(name, cls), outs):
            try:
                orc.parse(bad)
            except oracle.DecodeError:
                assert o[0] == "refused", (name, cls, o)
            if o[0] != "refused":
                assert o[-1] >= m.Encoder.transcode_min_size(bad, ht_sources=ht) > 0
    xd.conditions(name, counts)


def test_both_parsers_agree_on_every_draw(plan_diff, tmp_path):
    """both accept, with an equal plan, or both refuse (tests/native/plan_diff.c on every draw as it is)"""
    files = []
    for name, cls in xd.CASES:
        for i, bad in enumerate(xd.draws(name, cls)):
            p = tmp_path / ("%s.%s.%d.j2c" % (name, cls, i))
            p.write_bytes(bad)
            files.append(p)
    parses, accepted = plan_diff(files, 0)
    assert parses >= len(files) and 0 < accepted < parses
