"""knob "idwt_x2": the last plain 5/3 level of a reversible 8-bit RGB job runs inside the final-level launch
(k_idwt_stream_pack_x2): its output, the largest LL band, stays in LDS windows instead of making a round trip through
memory.  Every case decodes the same job with the knob at 0 and at 1: both results must be the oracle's planes and the
source picture bit for bit, and the fused run must record exactly one IDWT launch fewer -- otherwise a case would pass
without running the kernel.

Shapes are the smallest at which each boundary exists.  Every level of every picture has fast geometry (width a
multiple of 4 and at least 8, at least 2 rows), which jobs with 16-bit sub-bands need; test_case_geometry checks that on
the CPU.  The three-level picture is 496 x 203, not 488 x 203: 488 / 4 = 122 is not a multiple of 4, so level 0 of a
488-wide picture is not of fast geometry and the job would never have 16-bit sub-bands; 496 is the next width that keeps
the odd row counts (203, 102) at the two fused levels."""
import numpy as np
import pytest

import vecgen

W_WG = 8 * 244                     # output columns of one workgroup: 8 waves of 244


def _levels(w, h, nl):
    """(lh, lv) of the IDWT levels of a picture at the origin, final level first"""
    out = []
    for _ in range(nl):
        out.append((w, h))
        w, h = (w + 1) // 2, (h + 1) // 2
    return out


def _fast(lh, lv):
    return lh % 4 == 0 and lh >= 8 and lv >= 2


# name: (width, height, levels)
SHAPES = {"one_band": (16, 5, 2), "seam": (2000, 70, 2), "odd_rows": (496, 203, 3), "with_x3": (256, 72, 5), "auto": (256, 192, 5)}


def test_case_geometry():
    for name, (w, h, nl) in SHAPES.items():
        assert all(_fast(lh, lv) for lh, lv in _levels(w, h, nl)), name
    assert _levels(16, 5, 2)[0][1] < 20                       # one band of the default 20 rows, odd height
    assert 2000 > W_WG and 70 % 20 != 0                       # the window seam inside the picture, a short last band
    (_, lv1), (_, lv0) = _levels(496, 203, 3)[:2]
    assert lv1 % 2 == 1 and lv0 == 102                        # odd rows at the final level, 102 at the one fused into it
    assert 3 * 3 * 2 * 128 * 96 < 16 << 20                    # three 256 x 192 frames: far below any auto threshold


@pytest.fixture(scope="module")
def dec():
    import ffmpeg_ht_amd as m
    d = m.Decoder()
    assert d.device_name().startswith("gfx950"), d.device_name()
    yield d
    d.close()


_cache = {}


def _stream(orc, name):
    """(source picture, codestream, oracle planes) of a shape, made once"""
    if name not in _cache:
        w, h, nl = SHAPES[name]
        img = vecgen.synth_image(w, h, 3, seed=w + h + nl, noise=10)
        data = vecgen.encode(img, mct=1, nlevels=nl, transform=1)
        _cache[name] = (img, data, orc.decode(data)[1])
    return _cache[name]


DEFAULTS = dict(idwt_x2=2, idwt_x2_th=20, idwt_x2_min_bytes=20 << 20, idwt_x3=1, idwt_pk=1, ll16_test_bits=16)


def _restore(dec):
    for k, v in DEFAULTS.items():
        dec.set_int(k, v)


def _run(dec, pkts):
    job = dec.job().parse_batch(pkts).upload().run().wait()
    frames = [job.download_frame(f)[1] for f in range(len(pkts))]
    st = dict(coef16=job.coef16(), ll16=job.ll16(), errors=job.block_errors(), launches=len(job.idwt_launches()))
    hbm = job.idwt_hbm_bytes()
    assert all(0 < hb <= by for (ms, by), hb in zip(job.idwt_launches(), hbm))
    job.free()
    return frames, st


def _check_frames(frames, refs, tag):
    for f, (planes, (img, planes_o)) in enumerate(zip(frames, refs)):
        assert all(np.array_equal(a, d) for a, d in zip(planes, planes_o)), (tag, f)
        h, w = img[0].shape
        assert np.array_equal(planes[0].reshape(h, w, 3), np.stack(img, -1)), (tag, f)


def _both_ways(dec, orc, names, tag, nlaunch=None):
    """the job with idwt_x2 0 and 1: same frames as the oracle and the source, one launch fewer when fused"""
    srcs = [_stream(orc, n) for n in names]
    pkts = [s[1] for s in srcs]
    refs = [(s[0], s[2]) for s in srcs]
    n = {}
    for x2 in (0, 1):
        dec.set_int("idwt_x2", x2)
        frames, st = _run(dec, pkts)
        assert st["coef16"] and st["ll16"] == 1 and st["errors"] == 0, (tag, x2, st)
        _check_frames(frames, refs, (tag, x2))
        n[x2] = st["launches"]
    assert n[1] == n[0] - 1, (tag, n)
    if nlaunch is not None:
        assert n[1] == nlaunch, (tag, n)
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_band", "seam", "odd_rows"])
def test_fused_level_matches_two_launches(dec, orc, name):
    """16 x 5, 2 levels: one band, one strip, odd height, the fused plain level is level 0 (LL band from the block decoder);
    2000 x 70, 2 levels: wider than one workgroup, bands with a short last one; 496 x 203, 3 levels: odd row counts at both
    fused levels, a plain launch in front, the LL band read from the scratch buffer"""
    try:
        nl = SHAPES[name][2]
        _both_ways(dec, orc, [name] * (3 if name == "one_band" else 2), name, nlaunch=nl - 1)
    finally:
        _restore(dec)


@pytest.mark.gpu
def test_together_with_x3(dec, orc):
    """256 x 72, 5 levels: levels 0-2 as one launch (idwt_x3) and levels 3-4 as one (idwt_x2): 2 launches, 5 with both off"""
    try:
        _both_ways(dec, orc, ["with_x3"] * 2, "x3+x2", nlaunch=2)
        dec.set_int("idwt_x3", 0)
        dec.set_int("idwt_x2", 0)
        frames, st = _run(dec, [_stream(orc, "with_x3")[1]] * 2)
        assert st["launches"] == 5
        dec.set_int("idwt_x2", 1)                                 # without x3: the fused launch still takes levels 3 and 4
        frames, st = _run(dec, [_stream(orc, "with_x3")[1]] * 2)
        assert st["launches"] == 4
        s = _stream(orc, "with_x3")
        _check_frames(frames, [(s[0], s[2])] * 2, "x2 without x3")
    finally:
        _restore(dec)


@pytest.mark.gpu
def test_mixed_job(dec, orc):
    """16 x 5 and 2000 x 70 in one job: windows and grid sized by the job's maxima, used by a smaller plane"""
    try:
        _both_ways(dec, orc, ["one_band", "seam", "one_band"], "mixed", nlaunch=1)
    finally:
        _restore(dec)


@pytest.mark.gpu
@pytest.mark.parametrize("th", [4, 20, 256])
def test_rows_per_band(dec, orc, th):
    """idwt_x2_th: the smallest value the knob allows, the default, one above the picture height (clamped to what fits LDS)"""
    try:
        dec.set_int("idwt_x2_th", th)
        _both_ways(dec, orc, ["odd_rows"] * 2, ("th", th), nlaunch=2)
    finally:
        _restore(dec)


@pytest.mark.gpu
def test_without_packed_arithmetic(dec, orc):
    """idwt_pk = 0: the frames are the oracle's, whichever launches that takes"""
    try:
        dec.set_int("idwt_pk", 0)
        s = _stream(orc, "odd_rows")
        for x2 in (0, 1):
            dec.set_int("idwt_x2", x2)
            frames, st = _run(dec, [s[1]] * 2)
            assert st["coef16"] and st["ll16"] == 1 and st["errors"] == 0
            _check_frames(frames, [(s[0], s[2])] * 2, ("pk0", x2))
    finally:
        _restore(dec)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["with_x3", "seam"])
def test_range_check_of_the_band_in_lds(dec, orc, name):
    """ll16_test_bits = 6: an LL sample "overflows" beyond [-32, 31]; the check on what stage A stores into LDS fires and the
    transform runs again with 32-bit LL bands.  In the two-level picture the band in LDS is the only one that is checked."""
    try:
        dec.set_int("idwt_x2", 1)
        dec.set_int("ll16_test_bits", 6)
        s = _stream(orc, name)
        frames, st = _run(dec, [s[1]] * 2)
        assert st["ll16"] == 2 and st["errors"] == 0
        _check_frames(frames, [(s[0], s[2])] * 2, ("ovf", name))
    finally:
        _restore(dec)


@pytest.mark.gpu
def test_auto_mode(dec, orc):
    """idwt_x2 = 2 (default): small jobs, whose LL band makes its round trip in the last-level cache, keep their launches;
    with the threshold (idwt_x2_min_bytes) at 0 the same job fuses"""
    try:
        _restore(dec)
        s = _stream(orc, "auto")
        frames, st = _run(dec, [s[1]] * 3)
        assert st["coef16"] and st["ll16"] == 1 and st["launches"] == 3          # x3 + level 3 + final level
        _check_frames(frames, [(s[0], s[2])] * 3, "auto, default threshold")
        dec.set_int("idwt_x2", 2)
        dec.set_int("idwt_x2_min_bytes", 0)
        frames, st = _run(dec, [s[1]] * 3)
        assert st["coef16"] and st["ll16"] == 1 and st["launches"] == 2
        _check_frames(frames, [(s[0], s[2])] * 3, "auto, threshold 0")
    finally:
        _restore(dec)
