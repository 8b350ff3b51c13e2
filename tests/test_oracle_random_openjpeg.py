"""Random reversible codestreams from the test-vector factory, decoded by the oracle (+ shared host parser) and by
OpenJPEG 2.5.4 (via Pillow): every conforming decoder must return the same pixels, whatever the encoder did.
A third-party pin of the oracle across geometry (sizes, levels, block shapes, tiles, offsets, precincts, progression
orders), HT pass counts and every Part-1 mode switch, also with parameters that differ between the components of a stream
(COC / QCC) -- CPU only."""
import io

import numpy as np
import pytest

import vecgen

try:
    from PIL import Image, features
    HAVE_OPJ = bool(features.check("jpg_2000"))
except Exception:  # pragma: no cover
    HAVE_OPJ = False


def _draw(rng, it):
    w, h = int(rng.integers(1, 300)), int(rng.integers(1, 220))
    nc = int(rng.choice([1, 1, 3, 4]))
    depth = int(rng.choice([8, 8, 12, 16])) if nc == 1 else 8             # Pillow keeps more than 8 bits for grey only
    nl = int(rng.integers(0, 6))
    cbw = int(rng.integers(2, 8))
    cbh = int(rng.integers(2, min(10, 12 - cbw) + 1))
    kw = dict(nlevels=nl, cb=(cbw, cbh), depth=depth)
    if rng.random() < 0.45:
        kw.update(part1=True, cblk_style=int(rng.choice([0, 0, 1, 2, 4, 8, 0x20, 5, 9, 0x2F])))
    elif rng.random() < 0.4:
        kw["passes"] = int(rng.choice([2, 3]))
        if rng.random() < 0.4:
            kw["vsc"] = True
    if nc >= 3 and rng.random() < 0.6:
        kw["mct"] = 1
    if rng.random() < 0.25:
        kw["tile"] = (int(rng.choice([32, 64, 96, 100])), int(rng.choice([32, 48, 64, 70])))
    if rng.random() < 0.2:
        kw["offset"] = (int(rng.integers(0, 9)), int(rng.integers(0, 9)))
    if rng.random() < 0.25:
        kw["prog"] = int(rng.integers(0, 5))
    if rng.random() < 0.15:
        kw["prec"] = [(int(rng.integers(5, 9)), int(rng.integers(5, 9))), (int(rng.integers(4, 8)), int(rng.integers(4, 8)))]
    if rng.random() < 0.1:
        kw.update(sop=True, eph=bool(rng.integers(0, 2)))
    img = vecgen.synth_image(w, h, nc, depth=depth, seed=it + 3, noise=int(rng.choice([0, 4, 20])))
    return (w, h, nc, depth), kw, img


@pytest.mark.skipif(not HAVE_OPJ, reason="Pillow/OpenJPEG not importable")
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_reversible_streams_agree_with_openjpeg(orc, seed):
    rng = np.random.default_rng(seed)
    compared = 0
    for it in range(80):
        key, kw, img = _draw(rng, 100 * seed + it)
        try:
            data = vecgen.encode(img, **kw)
        except RuntimeError:
            continue                                                       # e.g. not enough guard bits for this draw
        info, planes, _ = orc.decode(data)
        assert orc.block_errors() == 0, (key, kw)
        im = Image.open(io.BytesIO(data))
        im.load()
        a = np.array(im)
        got = planes[0].reshape(a.shape)
        assert np.array_equal(got.astype(np.int64), a.astype(np.int64)), (key, kw)
        compared += 1
    assert compared >= 60


def _effective(kw, c, key, default):
    return ((kw.get("comp") or [None] * 4)[c] or {}).get(key, kw.get(key, default))


@pytest.mark.skipif(not HAVE_OPJ, reason="Pillow/OpenJPEG not importable")
@pytest.mark.parametrize("seed", [31, 32])
def test_random_streams_with_per_component_parameters(orc, seed):
    """the draws of above with COC / QCC: every component may have its own levels, block shape, guard bits, wavelet and step
    size, passes or mode switches, precincts (vecgen.draw_comp_overrides).  Components coded completely with 5/3 come back
    from the oracle as they went in; OpenJPEG agrees sample for sample on 5/3 components and within one LSB on 9/7 ones.
    OpenJPEG takes a component transform only over three components of one wavelet and one level count
    (opj_tcd_mct_decode), so a draw that signals one over unequal levels or wavelets is checked against the source alone"""
    rng = np.random.default_rng(seed)
    by_opj = by_source = mct_unequal = 0
    for it in range(80):
        key, kw, img = _draw(rng, 100 * seed + it)
        nc = key[2]
        kw["comp"] = vecgen.draw_comp_overrides(rng, nc, kw)
        if nc == 1 and kw["comp"][0] and "transform" in kw["comp"][0]:
            kw["comp"][0].pop("transform")                                 # (more than 8 bits and 9/7: one LSB is not the rule there)
        try:
            data = vecgen.encode(img, **kw)
        except RuntimeError:
            continue                                                       # e.g. not enough guard bits for this draw
        info, planes, _ = orc.decode(data)
        assert orc.block_errors() == 0, (key, kw)
        wavelets = [_effective(kw, c, "transform", 1) for c in range(nc)]
        levels = [_effective(kw, c, "nlevels", 0) for c in range(nc)]
        mct = bool(kw.get("mct")) and len(set(wavelets[:3])) == 1
        got = planes[0].reshape(info.height, info.width, -1).astype(np.int64)
        if info.bits_per_raw_sample > 8:
            got >>= 16 - info.bits_per_raw_sample
        complete = [wavelets[c] == 1 and (bool(kw.get("part1")) or _effective(kw, c, "passes", 1) == 1) for c in range(nc)]
        for c in range(nc):
            # (HT blocks with refinement passes start the cleanup pass one bit-plane up and can lose an isolated 1)
            if all(complete[:3]) if (mct and c < 3) else complete[c]:
                assert np.array_equal(got[..., c], img[c]), (key, kw, c)
                by_source += 1
        if kw.get("mct") and (len(set(levels[:3])) > 1 or len(set(wavelets[:3])) > 1):
            mct_unequal += 1
            continue
        im = Image.open(io.BytesIO(data))
        im.load()
        a = np.array(im).astype(np.int64).reshape(info.height, info.width, -1)
        full = planes[0].reshape(a.shape).astype(np.int64)
        lsb = 1 << (16 - key[3]) if key[3] > 8 else 1
        for c in range(nc):
            d = int(np.abs(full[..., c] - a[..., c]).max())
            assert d <= (lsb if (wavelets[c] == 0 or (mct and wavelets[0] == 0)) else 0), (key, kw, c, d)
        by_opj += 1
    assert by_opj >= 50 and by_source >= 60 and mct_unequal >= 3, (by_opj, by_source, mct_unequal)


def _draw_97(rng, it):
    """irreversible 9/7 draws: 8-bit (Pillow keeps more only for grey), optional ICT, HT or Part-1 blocks"""
    w, h = int(rng.integers(8, 300)), int(rng.integers(8, 220))
    nc = int(rng.choice([1, 3]))
    depth = int(rng.choice([8, 12])) if nc == 1 else 8
    cbw = int(rng.integers(2, 7))
    kw = dict(nlevels=int(rng.integers(0, 6)), cb=(cbw, int(rng.integers(2, min(10, 12 - cbw) + 1))), depth=depth,
              transform=0, qstep=float(rng.choice([1.0 / 64, 1.0 / 16, 0.25, 1.0])))
    if rng.random() < 0.4:
        kw.update(part1=True)
    if nc == 3 and rng.random() < 0.6:
        kw["mct"] = 1
    if rng.random() < 0.2:
        kw["tile"] = (int(rng.choice([64, 96, 100])), int(rng.choice([48, 64, 70])))
    if rng.random() < 0.2:
        kw["prog"] = int(rng.integers(0, 5))
    img = vecgen.synth_image(w, h, nc, depth=depth, seed=it + 11, noise=int(rng.choice([0, 4, 20])))
    return (w, h, nc, depth), kw, img


@pytest.mark.skipif(not HAVE_OPJ, reason="Pillow/OpenJPEG not importable")
@pytest.mark.parametrize("seed", [11, 12])
def test_random_irreversible_streams_agree_with_openjpeg_within_one_lsb(orc, seed):
    """9/7 + ICT: two float implementations of the same synthesis may round a sample differently, by one LSB at most
    (the tolerance north_star states for the irreversible path)"""
    rng = np.random.default_rng(seed)
    compared = worst = 0
    for it in range(60):
        key, kw, img = _draw_97(rng, 100 * seed + it)
        try:
            data = vecgen.encode(img, **kw)
        except RuntimeError:
            continue
        info, planes, _ = orc.decode(data)
        assert orc.block_errors() == 0, (key, kw)
        im = Image.open(io.BytesIO(data))
        im.load()
        a = np.array(im)
        got = planes[0].reshape(a.shape)
        d = int(np.abs(got.astype(np.int64) - a.astype(np.int64)).max())
        lsb = 1 << (16 - key[3]) if key[3] > 8 else 1                      # both write 12-bit samples << 4 into 16-bit words
        assert d <= lsb, (key, kw, d)
        worst = max(worst, d // lsb)
        compared += 1
    assert compared >= 45


def _analysis_low(x, odd0):
    """low-pass half of one reversible 5/3 analysis step (T.800 F.4.8) of the samples x, the first of which sits on an odd
    (odd0) or even absolute position"""
    n = len(x)
    x = x.astype(np.int64)
    if n == 1:
        return x.copy() if not odd0 else np.zeros(0, np.int64)
    ref = lambda i: -i if i < 0 else (2 * (n - 1) - i if i >= n else i)
    par = 1 if odd0 else 0
    y = x.copy()
    for i in range(par ^ 1, n, 2):
        y[i] = x[i] - ((x[ref(i - 1)] + x[ref(i + 1)]) >> 1)
    z = y.copy()
    for i in range(par, n, 2):
        z[i] = y[i] + ((y[ref(i - 1)] + y[ref(i + 1)] + 2) >> 2)
    return z[par::2]


def _reduced_by_analysis(img, key, kw, red):
    """what a decoder must return at `red` resolutions less: the LL band of `red` forward 5/3 levels of every tile (columns
    first, then rows, as the encoder ran them), through the forward / inverse RCT where the stream has one"""
    w, h, nc, depth = key
    dc = 1 << (depth - 1)
    comps = [c.astype(np.int64) - dc for c in img]
    if kw.get("mct"):
        r, g, b = comps[:3]
        comps = [(r + 2 * g + b) >> 2, b - g, r - g] + comps[3:]
    tw, th = kw.get("tile", (w, h))
    up = lambda v: (v + (1 << red) - 1) >> red
    out = [np.zeros((up(h), up(w)), np.int64) for _ in comps]
    for ty in range(0, h, th):
        for tx in range(0, w, tw):
            for ci, c in enumerate(comps):
                a, x0, y0 = c[ty:ty + th, tx:tx + tw], tx, ty
                for _ in range(red):
                    a = np.stack([_analysis_low(col, y0 & 1) for col in a.T]).T if a.size else a
                    a = np.stack([_analysis_low(row, x0 & 1) for row in a]) if a.size else a
                    x0, y0 = (x0 + 1) >> 1, (y0 + 1) >> 1
                if a.size:
                    out[ci][up(ty):up(ty) + a.shape[0], up(tx):up(tx) + a.shape[1]] = a
    if kw.get("mct"):
        y, cb, cr = out[:3]
        g = y - ((cb + cr) >> 2)
        out = [cr + g, g, cb + g] + out[3:]
    ref = np.clip(np.stack(out, -1) + dc, 0, (1 << depth) - 1)
    return ref << (16 - depth) if depth > 8 else ref


@pytest.mark.parametrize("seed", [21, 22])
def test_random_reversible_streams_at_reduced_resolution(orc, seed):
    """`lowres` (jpeg2000dec.c:2913-2917, reduction_factor): the lower resolution of a reversible stream is an exact integer
    reconstruction too -- the LL band the encoder's analysis left at that level.  Checked against that band computed
    independently here (cleanup-only streams), and against OpenJPEG's `reduce` where Pillow's build accepts the size; where
    the two decoders differ the analysis says who is right"""
    rng = np.random.default_rng(seed)
    by_analysis = by_opj = 0
    for it in range(90):
        key, kw, img = _draw(rng, 100 * seed + it)
        kw.pop("offset", None)
        if kw["nlevels"] < 2:
            continue
        red = int(rng.integers(1, kw["nlevels"]))                          # (Pillow's OpenJPEG refuses reduce == levels)
        try:
            data = vecgen.encode(img, **kw)
        except RuntimeError:
            continue
        info, planes, _ = orc.decode(data, reduction_factor=red)
        assert orc.block_errors() == 0, (key, kw, red)
        ref = None
        if "passes" not in kw:                                             # (streams with refinement passes: OpenJPEG only)
            ref = _reduced_by_analysis(img, key, kw, red)
            assert np.array_equal(planes[0].reshape(ref.shape).astype(np.int64), ref), (key, kw, red)
            by_analysis += 1
        if not HAVE_OPJ:
            continue
        im = Image.open(io.BytesIO(data))
        im.reduce = red
        try:
            im.load()
        except (OSError, ValueError):
            continue                                                       # Pillow's OpenJPEG gives up on some reduced sizes
        a = np.array(im)
        diff = int(np.abs(planes[0].reshape(a.shape).astype(np.int64) - a.astype(np.int64)).max())
        same = diff == 0
        # ref is not None: the oracle equals the analysis band, OpenJPEG is the one that is off.  passes == 2 (cleanup +
        # SigProp, no MagRef: a truncated, lossy stream): a line of ONE sample at an odd position is halved with an
        # arithmetic shift by the reference (jpeg2000dwt.c:313-317, `(int)p[1] >> 1`) and with a division by OpenJPEG --
        # the same for the even values a complete stream holds there, one apart for negative odd ones
        assert same or ref is not None or (kw.get("passes") == 2 and diff <= 2), (key, kw, red, diff)
        by_opj += same
    assert by_analysis >= 20 and (by_opj >= 20 or not HAVE_OPJ), (by_analysis, by_opj)
