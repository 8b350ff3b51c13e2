"""HT and MIXED sources in the transcoder (htj2k_transcode_opts.ht_sources) on the GPU: the raw stores of the HT block
kernels (htj2k_ht_blocks_raw) against the reference's block decoder, whole frames compared on the product decoder and
through the oracle, the planes and passes every block got against the block rule (tests/xc_ht_model.py, tests/xc_model.py),
the kernel routes, batches and rounds, budgets, a damaged source, and the C example."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library, as in tests/test_transcode_rc_gpu.py)

import ffmpeg_ht_amd as m
import oracle
import vecgen
import xc_ht_model as xh
import xc_rc_model as xrm
from test_transcode_gpu import block_stage_planes
from xc_source import Source

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCHWELCOME, INVALIDDATA, EINVAL = -0x45574150, -0x41444E49, -22


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def enc():
    e = m.Encoder(device_id=0)
    yield e
    e.close()


# ---------------------------------------------------------------- 5. the raw stores of the HT kernels
def raw_table():
    """-> (descs, pool, [(sample offset, expected indices)], samples): the shapes of the CPU test of the rule and a block
    wider than 64 columns, 1 .. 3 passes, without and with a placeholder set, sparse and dense; every one-pass block has
    pc = 0 (its half bit lies below the index's LSB), and the last blocks have S_blk = 0"""
    rng = np.random.default_rng(55)
    descs, pool, expect, soff = [], b"", [], 0

    def add(vals, passes, plhd, causal=False, top=False):
        nonlocal pool, soff
        h, w = vals.shape
        data, lcup, lref, mu = vecgen.encode_block(vals, passes, causal)
        p = 1 if passes > 1 else 0
        M_b = max(mu + p, 1) + 1 + (1 if plhd else 0)
        zbp, n = M_b - 1 - p - plhd, passes + 3 * plhd
        if top:                                            # the cleanup pass on the band's highest plane: U <= 1
            assert mu <= 1 and not plhd
            M_b, zbp = 6, 0
        ret, t1 = oracle.ht_decode_block(data, lcup, lref, n, zbp, w, h, M_b, vsc=causal)
        assert ret == 1
        d = m.BlockDesc()
        d.data_off, d.plane_off, d.lcup, d.lref, d.w, d.h, d.stride = len(pool), soff, lcup, lref, w, h, w
        # the transform bits and the steps are not read by the raw stores: 9/7 descriptors on every other block
        d.npasses, d.zbp, d.M_b, d.flags, d.roi_shift, d.f_step, d.i_step = n, zbp, M_b, (8 if causal else 0) | (len(descs) % 2), 0, 0.37, 32768
        descs.append(d)
        pool += data + b"\0" * ((-len(data)) % 16)
        want = xh.raw_index(t1, M_b, zbp, n)
        assert xh.rule(M_b, zbp, n) == ((M_b - 1 if top else 0), passes)
        expect.append((soff, want))
        soff += w * h

    for (w, h) in [(1, 1), (3, 5), (4, 4), (17, 9), (64, 64), (128, 32)]:
        for passes in (1, 2, 3):
            for plhd in (0, 1):
                for amp, density in ((3, 0.3), (200, 0.9)):
                    vals = rng.integers(-amp, amp + 1, (h, w)) * (rng.random((h, w)) < density)
                    vals[0, 0] = amp
                    add(vals, passes, plhd, causal=(passes == 3 and plhd == 1))
        ones = rng.integers(-1, 2, (h, w))
        ones[0, 0] = -1
        add(ones, 1, 0, top=True)
    assert any(w.any() for _, w in expect[-1:])
    return descs, pool, expect, soff


@pytest.mark.parametrize("ht_mode", [1, 0])
def test_ht_blocks_raw(dec, ht_mode):
    """the plane htj2k_ht_blocks_raw writes is the oracle's sign-magnitude output with the half bits stripped
    (xh.raw_index), no difference allowed: through k_ht_vlc and k_ht_decode_raw<true> (ht_mode 1; the narrow blocks on its
    row loop, the 128-column ones on the column-per-lane stages) and through k_ht_decode_raw<false> (ht_mode 0)"""
    descs, pool, expect, soff = raw_table()
    dec.set_int("ht_mode", ht_mode)
    try:
        got, status = dec.ht_blocks(descs, pool, soff, raw=True)
        assert not status.any()
        bad = [i for i, (o, want) in enumerate(expect) if not np.array_equal(got[o:o + want.size].reshape(want.shape), want)]
        assert not bad, [(i, descs[i].w, descs[i].h, descs[i].npasses) for i in bad]
        # a ROI shift or 32 magnitude bits: refused
        for field, value in (("roi_shift", 3), ("M_b", 32)):
            d = m.BlockDesc.from_buffer_copy(descs[0])
            setattr(d, field, value)
            with pytest.raises(m.Htj2kError) as err:
                dec.ht_blocks([d], pool, soff, raw=True)
            assert err.value.code == EINVAL
    finally:
        dec.set_int("ht_mode", 1)


# ---------------------------------------------------------------- whole frames
def yuv420(w, h, seed):
    return vecgen.synth_image(w, h, 3, seed=seed, dx=[1, 2, 2], dy=[1, 2, 2])


RGB = lambda: vecgen.synth_image(64, 48, 3, seed=2)
R97 = dict(mct=1, nlevels=3, cb=(4, 4), transform=0, qstep=1 / 8)
CASES = {"gray_33x17": (lambda: vecgen.synth_image(33, 17, 1, seed=1), dict(nlevels=2, cb=(2, 2), transform=1))}
for p in (1, 2, 3):
    CASES["rgb_97_cb16_%dp" % p] = (RGB, dict(R97, passes=p))
    CASES["rgb_97_cb32_%dp" % p] = (RGB, dict(R97, cb=(5, 5), passes=p))         # 32 columns: four blocks per wave
    CASES["rgb_97_cb64_%dp" % p] = (RGB, dict(R97, cb=(6, 6), passes=p))         # two per wave
    CASES["rgb_97_cb128x8_%dp" % p] = (RGB, dict(R97, cb=(7, 3), passes=p))      # 128 columns: no multi kernel
# (the bands of a 64 x 48 picture are at most 32 columns wide, whatever cb says: these three are wide enough for blocks of
# 64 columns, two per wave, and of more than 64, which take k_ht_vlc and the column-per-lane kernel)
WIDE = lambda: vecgen.synth_image(150, 40, 1, seed=8)
for p in (1, 2, 3):
    CASES["wide_cb64_%dp" % p] = (WIDE, dict(nlevels=1, cb=(6, 6), transform=0, qstep=1 / 8, passes=p))
    CASES["wide_cb128x8_%dp" % p] = (WIDE, dict(nlevels=1, cb=(7, 3), transform=0, qstep=1 / 8, passes=p))
CASES.update({
    "yuv420p_64x48": (lambda: yuv420(64, 48, 3), dict(nlevels=2, cb=(3, 3), dx=[1, 2, 2], dy=[1, 2, 2], width=64, height=48)),
    "gray16_40x24": (lambda: vecgen.synth_image(40, 24, 1, depth=16, seed=4), dict(depth=16, nlevels=2, cb=(3, 3))),
    "rgb_70x50_tiles": (lambda: vecgen.synth_image(70, 50, 3, seed=5), dict(mct=1, nlevels=2, cb=(3, 3), tile=(32, 32))),
    "levels_0": (lambda: vecgen.synth_image(37, 21, 1, seed=6), dict(nlevels=0, cb=(3, 4))),
    "prog_precincts_sop": (lambda: vecgen.synth_image(70, 50, 3, seed=7), dict(mct=1, nlevels=3, prog=2, prec=[(7, 7)], sop=True, eph=True)),
    "placeholder_1": (RGB, dict(R97, transform=1, placeholder_sets=1)),
    "vsc_3p": (RGB, dict(R97, passes=3, vsc=True)),
})
HT_CASES = sorted(CASES)
for t, kw in (("53", dict(transform=1)), ("97", dict())):
    for d in (0, 2):
        CASES["mixed_%s_drop%d" % (t, d)] = (RGB, dict(R97, mixed=True, drop_passes=d, **kw))
MIXED_CASES = sorted(set(CASES) - set(HT_CASES))


def source_forms(orc, src, kw):
    """per block of the encoder's layout what the rule makes of the source, each block by the rule of its own coder:
    (reported plane, reported passes, left out, (pr, k) of the rule), from the oracle's parse and block decode of the
    source (Source, tests/xc_source.py)"""
    return Source(orc, src, kw).forms()


@pytest.fixture(scope="module")
def transcoded(dec, enc):
    """every case's source and transcoded stream, made once and shared by the tests below"""
    cache = {}

    def get(name):
        if name not in cache:
            img, kw = CASES[name]
            src = vecgen.encode(img(), **kw)
            cs = enc.transcode(dec, [src], ht_sources=True)[0]
            cache[name] = (src, cs, enc.last_planes(0), enc.last_passes(0))
        return cache[name]
    return get


def check_frame(orc, dec, enc, transcoded, name):
    src, cs, planes, passes = transcoded(name)
    img, kw = CASES[name]
    # the product decoder: the planes after the block stage and the pixels
    assert dec.probe(cs).is_ht == 1
    a, b = block_stage_planes(dec, src), block_stage_planes(dec, cs)
    assert len(a) == len(b)
    for t, (p, q) in enumerate(zip(a, b)):
        assert p.dtype == q.dtype and p.shape == q.shape
        assert np.count_nonzero(p.view(np.uint32) != q.view(np.uint32)) == 0, (name, t)
    ia, pa, _, sa = dec.decode(src)
    ib, pb, _, sb = dec.decode(cs)
    assert sa.n_block_errors == 0 == sb.n_block_errors
    assert (ia.width, ia.height, ia.pix_fmt, ia.bits_per_raw_sample) == (ib.width, ib.height, ib.pix_fmt, ib.bits_per_raw_sample)
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
    # the oracle
    _, oa, _ = orc.decode(src)
    ea = orc.block_errors()
    oi, ob, _ = orc.decode(cs)
    assert ea == 0 == orc.block_errors() and oi.is_ht == 1
    assert all(np.array_equal(x, y) for x, y in zip(oa, ob))
    # the rule
    forms = source_forms(orc, src, kw)
    assert len(forms) == len(planes) == len(passes)
    for i, (p, k, left_out, _) in enumerate(forms):
        assert (planes[i], passes[i]) == (p, k), (name, i)
    out = [e for e in orc.plan_blocks(cs) if e["npasses"]]
    assert len(out) == sum(1 for f in forms if not f[2]) and not any(e["flags"] & (4 | 8) for e in out)      # HT, not causal
    assert sorted(int(e["npasses"]) for e in out) == sorted(k for _, k, lo, _ in forms if not lo)
    # the output is a source like any other: it comes back byte for byte
    assert enc.transcode(dec, [cs], ht_sources=True) == [cs]
    assert (enc.last_planes(0), enc.last_passes(0)) == (planes, passes)
    # every route through the HT kernels stores the same indices
    try:
        for knob, value in (("ht_multi", 0), ("ht_mode", 0)):
            dec.set_int(knob, value)
            assert enc.transcode(dec, [src], ht_sources=True) == [cs], (name, knob)
            dec.set_int(knob, 1)
    finally:
        dec.set_int("ht_multi", 1)
        dec.set_int("ht_mode", 1)
    return forms


@pytest.mark.parametrize("name", HT_CASES)
def test_ht_frames(orc, dec, enc, transcoded, name):
    """6. an HT source and its transcode are the same frame, block for block in the source's form"""
    forms = check_frame(orc, dec, enc, transcoded, name)
    kw = CASES[name][1]
    if kw.get("passes", 1) > 1:                           # the sources of two and three passes keep them somewhere
        assert kw["passes"] in {k for _, k, lo, _ in forms if not lo}, name
    per_wave = {"rgb_97_cb32": 4, "wide_cb64": 2, "wide_cb128x8": 1}.get(name[:-3])
    if per_wave:                                          # the route this layout takes, read off the decoder's own block stage
        job = dec.job().parse(transcoded(name)[0]).upload().run(1).wait()
        assert job.ht_blocks_per_wave() == per_wave, name
        job.free()


@pytest.mark.parametrize("name", MIXED_CASES)
def test_mixed_frames(orc, dec, enc, transcoded, name):
    """7. a MIXED source: every block by the rule of its own coder"""
    forms = check_frame(orc, dec, enc, transcoded, name)
    tab = orc.plan_blocks(transcoded(name)[0])
    assert {bool(e["flags"] & 4) for e in tab if e["npasses"]} == {False, True}
    if name.endswith("drop2"):
        assert {k for _, k, lo, _ in forms if not lo} >= {1, 2}


# ---------------------------------------------------------------- 8. batches
def batch_sources():
    return [vecgen.encode(vecgen.synth_image(33, 17, 1, seed=1), part1=True, nlevels=2, cb=(3, 3), drop_passes=1),
            vecgen.encode(vecgen.synth_image(24, 20, 1, seed=2), nlevels=2, cb=(3, 3), transform=0, qstep=1 / 4, passes=3),
            vecgen.encode(vecgen.synth_image(50, 9, 1, seed=3), nlevels=1, cb=(3, 3), mixed=True, drop_passes=2)]


def test_batch_of_part1_ht_and_mixed(dec, enc):
    srcs = batch_sources()
    singles = [enc.transcode(dec, [s], ht_sources=True)[0] for s in srcs]
    assert singles[0] == enc.transcode(dec, srcs[:1])[0]                 # the Part-1 frame does not care
    got = enc.transcode(dec, srcs, ht_sources=True)
    assert got == singles and enc.last_rounds() == 1
    for s, o in zip(srcs, got):
        assert all(np.array_equal(a, b) for a, b in zip(dec.decode(s)[1], dec.decode(o)[1]))
    old = os.environ.get("HTJ2K_ENC_ROUND")
    os.environ["HTJ2K_ENC_ROUND"] = str(33 * 17 + 10)
    try:
        small = m.Encoder(device_id=0)
    finally:
        if old is None:
            del os.environ["HTJ2K_ENC_ROUND"]
        else:
            os.environ["HTJ2K_ENC_ROUND"] = old
    try:
        assert small.transcode(dec, srcs, ht_sources=True) == singles
        assert small.last_rounds() == 3
    finally:
        small.close()
    # without the keyword the batch is refused whole
    with pytest.raises(m.Htj2kError) as err:
        enc.transcode(dec, srcs, cap=sum(m.Encoder.transcode_check(s, ht_sources=True) for s in srcs))
    assert err.value.code == PATCHWELCOME and "HT code-blocks already" in str(err.value) and not enc.last_out.any()
    with pytest.raises(m.Htj2kError) as err:
        enc.transcode(dec, srcs, cap=100000, ht_sources=2)
    assert err.value.code == EINVAL and "ht_sources" in str(err.value) and not enc.last_out.any()


# ---------------------------------------------------------------- 9. budgets
@pytest.mark.parametrize("name", ["rgb_97_cb16_3p", "mixed_97_drop2"])
def test_budgets(orc, dec, enc, transcoded, name):
    src, free, free_planes, free_passes = transcoded(name)
    forms = source_forms(orc, src, CASES[name][1])
    least = m.Encoder.transcode_min_size(src, ht_sources=True)
    assert least < len(free)
    coarser = 0
    for target in (len(free), len(free) - 1, (len(free) + least) // 2, least):
        cs = enc.transcode(dec, [src], target_bytes=target, ht_sources=True)[0]
        info, planes, passes = enc.rc_info(0), enc.last_planes(0), enc.last_passes(0)
        print(name, target, len(cs), info)
        assert len(cs) <= target
        assert (info["target_bytes"], info["final_bytes"], info["nblocks"]) == (target, len(cs), len(forms)) and 1 <= info["ht_launches"] <= 3
        if target >= len(free):
            assert cs == free and (planes, passes) == (free_planes, free_passes)
            assert (info["trial"], info["ht_launches"], info["est_bytes"]) == (1, 1, 0)
        else:
            assert len(cs) < len(free) and info["trial"] == 0
        _, _, _, st = dec.decode(cs)
        assert st.n_block_errors == 0
        orc.decode(cs)
        assert orc.block_errors() == 0
        for i, (p, k) in enumerate(zip(planes, passes)):
            fp, fk, left_out, (pr, ks) = forms[i]
            if pr < 0:
                assert (p, k) == (-1, 1), i
            elif p >= 0:
                assert p >= pr and (p > pr or k in xrm.ALLOWED_AT_0[ks]) and p >= fp, (i, p, k, pr, ks)
                coarser += (p, k) != (fp, fk)
        assert enc.transcode(dec, [src], target_bytes=target, ht_sources=True) == [cs]       # deterministic
        if target == least:
            assert planes == [-1] * len(forms)
    assert coarser > 0


# ---------------------------------------------------------------- 10. a damaged HT block
def test_damaged_ht_block_is_an_error(dec, enc, orc):
    """a byte of the one block's body set to 0xFF (the stream of tests/test_gpu_parity.py's corrupt-block test): the
    parsers take the frame, the reference's HT block decoder rejects the block, and so do the raw kernels -- the call
    is HTJ2K_ERR_INVALIDDATA and nothing is written"""
    good = vecgen.encode(vecgen.synth_image(64, 64, 1, seed=3), nlevels=0)
    bad = bytearray(good)
    bad[-3] = 0xFF
    bad = bytes(bad)
    orc.decode(bad)
    assert orc.block_errors() == 1
    assert m.Encoder.transcode_check(bad, ht_sources=True) > 0
    want = enc.transcode(dec, [good], ht_sources=True)
    for knob, value in ((None, 1), ("ht_multi", 0), ("ht_mode", 0)):
        try:
            if knob:
                dec.set_int(knob, value)
            with pytest.raises(m.Htj2kError) as err:
                enc.transcode(dec, [good, bad], cap=4 * len(good) + 100000, ht_sources=True)
            assert err.value.code == INVALIDDATA and not enc.last_out.any(), knob
            assert "failed to decode" in str(err.value)
        finally:
            if knob:
                dec.set_int(knob, 1)
    assert enc.transcode(dec, [good], ht_sources=True) == want


# ---------------------------------------------------------------- 11. the example
def test_example_program_with_ht_sources(tmp_path):
    exe = os.path.join(ROOT, "examples", "htj2k_transcode")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", ROOT, "examples/htj2k_transcode"])
    src = tmp_path / "in.jph"
    src.write_bytes(vecgen.encode(RGB(), **dict(R97, passes=3)))
    out = subprocess.run([exe, str(src), str(tmp_path / "no.jph")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "HT code-blocks already" in out.stderr and not (tmp_path / "no.jph").exists()
    out = subprocess.run([exe, "--ht-sources", str(src), str(tmp_path / "free.jph")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "frames identical" in out.stdout and "of HTJ2K ->" in out.stdout, out.stdout + out.stderr
    free = len((tmp_path / "free.jph").read_bytes())
    budget = free // 2
    out = subprocess.run([exe, "--ht-sources", str(src), str(tmp_path / "out.jph"), str(budget)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 block errors" in out.stdout, out.stdout + out.stderr
    assert 0 < len((tmp_path / "out.jph").read_bytes()) <= budget
