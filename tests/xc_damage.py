"""Damaged sources for the transcoder tests (tests/test_transcode_damaged_host.py, tests/test_transcode_damaged_gpu.py):
the sources, the seeded damage of every class, and what the oracle and htj2k_transcode_check make of a draw.  One module
for both files, so that the GPU test runs exactly the streams the host test has vetted.  Test tooling only.

Every source carries SOP and EPH markers, so tests/cs_rewrite.py finds packet headers and bodies without decoding them.
Damage never changes a length: a draw is the source with some bytes replaced."""
import zlib

import numpy as np

import cs_rewrite
import ffmpeg_ht_amd as m
import oracle
import vecgen

INVALIDDATA = -0x41444E49
DRAWS = 12

RGB = lambda: vecgen.synth_image(64, 48, 3, seed=2)
R97 = dict(mct=1, nlevels=3, cb=(4, 4), transform=0, qstep=1 / 8)
# name -> (image, factory keywords, ht_sources)
SOURCES = {
    "p1_rgb_53_cb16": (RGB, dict(part1=True, mct=1, nlevels=3, cb=(4, 4), transform=1), False),
    "p1_rgb_97_style05": (RGB, dict(R97, part1=True, cblk_style=0x05), False),
    "p1_gray_style2f_cb8": (lambda: vecgen.synth_image(64, 48, 1, seed=1), dict(part1=True, nlevels=2, cb=(3, 3), cblk_style=0x2F), False),
    "p1_yuv420p_50x38": (lambda: vecgen.synth_image(50, 38, 3, seed=3, dx=[1, 2, 2], dy=[1, 2, 2]),
                         dict(part1=True, nlevels=2, cb=(3, 3), dx=[1, 2, 2], dy=[1, 2, 2], width=50, height=38), False),
    "p1_gray16_40x24": (lambda: vecgen.synth_image(40, 24, 1, depth=16, seed=4), dict(part1=True, depth=16, nlevels=2, cb=(3, 3)), False),
    "p1_rgb_70x50_tiles": (lambda: vecgen.synth_image(70, 50, 3, seed=5), dict(part1=True, mct=1, nlevels=2, cb=(3, 3), tile=(32, 32)), False),
    "p1_rgb_97_drop2": (RGB, dict(R97, part1=True, drop_passes=2), False),
    "ht_rgb_53_3p": (RGB, dict(mct=1, nlevels=3, cb=(4, 4), transform=1, passes=3), True),
    "ht_rgb_97_1p": (RGB, dict(R97, passes=1), True),
    "mixed_rgb_97_3p": (RGB, dict(R97, mixed=True, passes=3), True),
}
PART1 = sorted(n for n in SOURCES if not SOURCES[n][2])
HT = sorted(n for n in SOURCES if SOURCES[n][2])
# (a) one body byte, (b) ten body bytes, (c) every body byte random, (d) every body byte 0xFF / 0x00, (e) one to three bytes
# of packet headers, (f) ten bytes anywhere behind the first SOD; (c) and (d) on Part-1 sources only
CLASSES = {n: ("a", "b", "c", "d", "e", "f") if n in PART1 else ("a", "b", "e", "f") for n in SOURCES}
CASES = [(n, c) for n in sorted(SOURCES) for c in CLASSES[n]]

# The seed of a (source, class) pair is crc32("source/class") + SEED.get(pair, 0).  The entries here were chosen on the CPU,
# with the oracle and htj2k_transcode_check alone, as the first offsets for which the conditions of the host test hold.
SEED = {
    ("ht_rgb_53_3p", "b"): 3, ("ht_rgb_53_3p", "e"): 388, ("ht_rgb_53_3p", "f"): 2, ("ht_rgb_97_1p", "b"): 2, ("ht_rgb_97_1p", "e"): 58,
    ("mixed_rgb_97_3p", "e"): 12, ("p1_rgb_53_cb16", "e"): 2, ("p1_rgb_53_cb16", "f"): 1, ("p1_rgb_70x50_tiles", "e"): 1,
    ("p1_rgb_97_drop2", "e"): 1, ("p1_yuv420p_50x38", "e"): 1,
}

_cache = {}


def source(name):
    """the undamaged stream"""
    if name not in _cache:
        img, kw, _ = SOURCES[name]
        _cache[name] = vecgen.encode(img(), sop=True, eph=True, **kw)
    return _cache[name]


def _spans(cs):
    """-> (header spans, body spans, offset behind the first SOD) of the packets: [(first, end)] in the stream's bytes"""
    s = cs_rewrite.Stream(cs)
    assert s.build() == cs                                 # the offsets below are those of the stream itself
    heads, bodies, first_sod = [], [], None
    pos = 2 + sum(4 + len(p) for _, p in s.main)
    for isot in s.order:
        t = s.tiles[isot]
        pos += 12 + sum(4 + len(p) for _, p in t["hdr"]) + 2
        first_sod = pos if first_sod is None else first_sod
        for sop, hdr, body in t["packets"]:
            pos += len(sop)
            if len(hdr) > 2:
                heads.append((pos, pos + len(hdr) - 2))    # without the EPH marker
            pos += len(hdr)
            if body:
                bodies.append((pos, pos + len(body)))
            pos += len(body)
    assert pos + 2 == len(cs)
    return heads, bodies, first_sod


def _positions(spans):
    return np.concatenate([np.arange(a, b) for a, b in spans])


def draws(name, cls):
    """-> [damaged stream]: the DRAWS draws of a class on a source (class d: two), the same on every call"""
    cs = source(name)
    heads, bodies, first_sod = _spans(cs)
    rng = np.random.default_rng(zlib.crc32(("%s/%s" % (name, cls)).encode()) + SEED.get((name, cls), 0))
    body, head = _positions(bodies), _positions(heads)
    value = lambda: int(rng.integers(0, 256)) if rng.integers(0, 2) else 0xFF
    out = []
    for i in range(2 if cls == "d" else DRAWS):
        bad = bytearray(cs)
        if cls == "a":
            bad[int(rng.choice(body))] = value()
        elif cls == "b":
            for pos in rng.choice(body, 10, replace=False):
                bad[int(pos)] = value()
        elif cls == "c":
            for pos, v in zip(body, rng.integers(0, 256, len(body))):
                bad[int(pos)] = int(v)
        elif cls == "d":
            for pos in body:
                bad[int(pos)] = 0x00 if i else 0xFF
        elif cls == "e":
            for pos in rng.choice(head, int(rng.integers(1, 4)), replace=False):
                bad[int(pos)] = value()
        elif cls == "f":                                   # as test_part1_corrupt_bodies_match_oracle draws them
            for pos in rng.integers(first_sod, len(bad) - 2, 10):
                bad[int(pos)] = value()
        else:
            raise ValueError(cls)
        out.append(bytes(bad))
    return out


def outcome(orc, bad, ht):
    """what a draw has to do, from htj2k_transcode_check and the oracle alone:
    ("refused", code)                  the check raises
    ("error", errors | None, marked, bound)   the check gives a bound; the oracle fails that many blocks, or (None) refuses
                                       the frame; marked: the blocks of undefined input it marked, by which
                                       the device's count of failed blocks may differ from the oracle's
    ("compared", noted, bound)         the oracle decodes every block; noted: it marked a block of undefined input
    After "compared" the oracle holds its decode of `bad`."""
    try:
        bound = m.Encoder.transcode_check(bad, ht_sources=ht)
    except m.Htj2kError as e:
        return ("refused", e.code)
    try:
        orc.decode(bad)
    except oracle.DecodeError:
        return ("error", None, 0, bound)
    if orc.block_errors():
        return ("error", orc.block_errors(), len(orc.underrun_windows()) if ht else 0, bound)
    return ("compared", bool(ht and orc.underrun_windows()), bound)


def census(orc, name, cls):
    """-> ([outcome of every draw], counts): compared, errors, refused and noted draws, and refused_invalid, the draws the
    check refuses with HTJ2K_ERR_INVALIDDATA"""
    ht = SOURCES[name][2]
    outs = [outcome(orc, bad, ht) for bad in draws(name, cls)]
    kinds = [o[0] for o in outs]
    return outs, dict(compared=kinds.count("compared"), errors=kinds.count("error"), refused=kinds.count("refused"),
                      noted=sum(1 for o in outs if o[0] == "compared" and o[1]),
                      refused_invalid=sum(1 for o in outs if o[0] == "refused" and o[1] == INVALIDDATA))


def conditions(name, counts):
    """the conditions that keep the helper from hiding a failure; counts: {class: census counts} of one source.

    Over classes (e) and (f) every source has a refusal by the check, a draw that is HTJ2K_ERR_INVALIDDATA and two
    compared draws.  On an HT or MIXED source the INVALIDDATA draw is one the check gives a bound for and the block
    decoder fails.  A Part-1 source has no such draw: decode_cblk fails on a block only when its passes run out of
    bit-planes or a termination is missing; the first the check's own block rule refuses ("passes over ..."), the second
    no packet header can express, the parser cuts the segments by the passes.  Not one of 36 000 draws of (e) and (f) on
    each Part-1 source got a bound and a block error, so there the draw is one the check refuses with that code, and
    that a bound never comes with a block error is asserted as well."""
    if name in PART1:
        for c in "abcd":                                   # the Part-1 block decoder is total: every draw is compared
            assert counts[c]["compared"] == (2 if c == "d" else DRAWS), (name, c, counts[c])
        assert sum(v["errors"] for v in counts.values()) == 0, (name, counts)
    else:
        assert 2 * counts["a"]["compared"] >= DRAWS, (name, counts["a"])
        assert counts["b"]["compared"] >= 2, (name, counts["b"])
        compared = sum(v["compared"] for v in counts.values())
        assert 4 * sum(v["noted"] for v in counts.values()) <= compared, (name, counts)
    ef = {k: counts["e"][k] + counts["f"][k] for k in ("compared", "errors", "refused", "refused_invalid")}
    assert ef["refused"] >= 1 and ef["compared"] >= 2, (name, ef)
    assert ef["errors"] >= 1 if name in HT else ef["refused_invalid"] >= 1, (name, ef)
