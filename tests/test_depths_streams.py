"""Components of unequal bit depth (streams.DEPTHS), pinned on the CPU.  Every frame the decoder returns goes through a
conversion per component (write_frame_8 / _16, jpeg2000dec.c:2301-2364): add 1 << (cbps - 1), clip to [0, 2^cbps - 1],
shift left by precision - cbps, where precision is 8 for the 8-bit layouts, 16 for the layouts that are always full-range
and the deepest component otherwise (jpeg2000dec.c:2383-2392).
 * the layout and the precision every case lands in, written out
 * lossless round trip: img[c] << (P - depth[c])
 * the conversion restated in numpy over the oracle's planes after the IDWT, equal to the oracle's frame
 * the clip cases do clip: samples strictly past both ends of every component's range, counted
 * the product's parser against the oracle's: return code, layout, tile-component table, cbps, also on damaged copies
tests/test_depths_gpu.py takes the same streams through the device routes; the catalogue's shared tests
(test_oracle_streams.py, test_plan_equality.py, test_gpu_parity.py) run every case that needs no decoder option of its own."""
import numpy as np
import pytest

import oracle
import streams
from test_hetero_streams import TILECOMP_DTYPE, _oracle_tilecomps, host_parser  # noqa: F401  (fixture)
from test_plan_equality import plan_diff  # noqa: F401  (fixture)

# name prefix -> (pix_fmt, bits_per_raw_sample, P): the layout of every case and the precision its samples are shifted up to
LAYOUT = {
    "dep_rgb24":     ("rgb24", 8, 8),
    "dep_yuv420p":   ("yuv420p", 8, 8),
    "dep_yuv444p_":  ("yuv444p", 8, 8),
    "dep_ya8":       ("ya8", 8, 8),
    "dep_rgba_":     ("rgba", 8, 8),
    "dep_rgb48_8_12_8": ("rgb48le", 12, 16),               # always full-range: 16
    "dep_rgb48_10_12_9": ("rgb48le", 12, 16),
    "dep_rgb48_12_10_16": ("rgb48le", 16, 16),
    "dep_rgba64":    ("rgba64le", 16, 16),
    "dep_yuv422p12": ("yuv422p12le", 12, 12),              # the deepest component
    "dep_yuv444p16": ("yuv444p16le", 12, 12),              # the layout has 16 bits, the deepest component 12
    "dep_ya16":      ("ya16le", 12, 12),
}


def layout_of(name):
    key = name.replace("p1_", "").replace("_clip", "").replace("_odd", "")
    hits = [v for k, v in LAYOUT.items() if key.startswith(k)]
    assert len(hits) == 1, name
    return hits[0]


def components(info, planes):
    """the frame as one (h, w) array of stored samples per component"""
    if len(planes) > 1:
        return [p.astype(np.int64) for p in planes]
    a = planes[0].reshape(info.height, info.width, -1).astype(np.int64)
    return [a[..., c] for c in range(a.shape[2])]


def decode(orc, name):
    data = streams.depths_encode(name)
    kw = streams.depths_decode_kw(name, oracle.PIX_NAMES)
    info, planes, consumed = orc.decode(data, **kw)
    assert orc.block_errors() == 0 and consumed > 0
    return data, kw, info, planes


def test_the_catalogue_covers_what_it_says():
    """the twelve depth / layout combinations, each on the fast geometry; every kind of packed three-component case (layout,
    shape, component transform, fixed point) has an entry with pairwise different depths; every case but the ones with a
    requested layout is enrolled in streams.CASES"""
    seen, kinds = set(), {}
    for name, (pic, depths, kw, dkw) in streams.DEPTHS.items():
        fmt = layout_of(name)[0]
        if pic[:2] == streams.DEPTHS_FAST:
            seen.add((tuple(depths), fmt))
        if fmt in ("rgb24", "rgb48le"):
            kind = (fmt, pic[:2], bool(kw.get("mct")), kw.get("transform", 1), dkw.get("bitexact", 0))
            kinds[kind] = kinds.get(kind, False) or len(set(depths)) == 3
        assert len(set(depths)) > 1, name
        assert (name in streams.CASES) == ("req_pix_fmt" not in dkw), name
    assert len(kinds) >= 12 and all(kinds.values()), kinds
    assert seen >= {((8, 7, 8), "rgb24"), ((5, 8, 3), "rgb24"), ((8, 12, 8), "rgb48le"), ((12, 10, 16), "rgb48le"),
                    ((10, 12, 9), "yuv422p12le"), ((8, 6, 6), "yuv420p"), ((12, 8), "ya16le"), ((8, 1), "ya8"),
                    ((8, 8, 8, 1), "rgba"), ((10, 10, 10, 16), "rgba64le"), ((8, 7, 8), "yuv444p"), ((8, 12, 8), "yuv444p16le")}
    kws = [(kw, dkw) for _, _, kw, dkw in streams.DEPTHS.values()]
    assert any(kw.get("mct") and kw.get("transform", 1) == 1 for kw, _ in kws)                    # RCT
    assert any(kw.get("mct") and kw.get("transform", 1) == 0 and not d for kw, d in kws)          # ICT float
    assert any(kw.get("mct") and kw.get("transform", 1) == 0 and d.get("bitexact") for kw, d in kws)
    assert any(kw.get("tile") and kw["tile"][0] % 4 and not kw.get("mct") for kw, _ in kws)
    assert any(kw.get("part1") for kw, _ in kws) and any(kw.get("sgnd") for kw, _ in kws)
    assert any(d.get("reduction_factor") == 1 for _, d in kws)


@pytest.mark.parametrize("name", sorted(streams.DEPTHS))
def test_layout_and_precision(orc, name):
    data, kw, info, planes = decode(orc, name)
    fmt, bits, P = layout_of(name)
    assert (oracle.PIX_NAMES[info.pix_fmt], info.bits_per_raw_sample) == (fmt, bits)
    depths = streams.DEPTHS[name][1]
    assert bits == max(depths) and P == (8 if bits <= 8 else 16 if fmt in ("rgb48le", "rgba64le") else bits)
    for c, a in enumerate(components(info, planes)):
        # nothing below the shift, nothing above the component's own range
        assert not (a & ((1 << (P - depths[c])) - 1)).any() and int(a.max()) <= ((1 << depths[c]) - 1) << (P - depths[c]), (name, c)


def _lossless(name):
    pic, depths, kw, dkw = streams.DEPTHS[name]
    return kw.get("transform", 1) == 1 and not dkw.get("reduction_factor")


@pytest.mark.parametrize("name", sorted(n for n in streams.DEPTHS if _lossless(n)))
def test_lossless_round_trip(orc, name):
    """img[c] << (P - depth[c]); a signed component comes back moved up by half its range (the reference ignores the sign
    bit of SIZ and adds the DC shift all the same)"""
    data, kw, info, planes = decode(orc, name)
    pic, depths, ekw, _ = streams.DEPTHS[name]
    P = layout_of(name)[2]
    img = streams.depths_image(name)
    got = components(info, planes)
    assert len(got) == len(img) == len(depths)
    for c, d in enumerate(depths):
        want = img[c].astype(np.int64) + ((1 << (d - 1)) if ekw.get("sgnd") else 0)
        assert 0 <= int(want.min()) and int(want.max()) < (1 << d)
        assert np.array_equal(got[c], want << (P - d)), (name, c)


def restated_frame(orc, data, kw, depths, P, shape_of):
    """the conversion over the oracle's planes after the IDWT, placed by the plan's tile-component table ->
    ([array per component], [the values before the clip per component, flattened])"""
    r, tcs = _oracle_tilecomps(orc, data, **kw)
    assert r >= 0
    orc.decode_blocks(data, **kw)
    orc.idwt()
    assert orc.num_tilecomps() == len(tcs)
    out = [np.zeros(shape_of(c), dtype=np.int64) for c in range(len(depths))]
    raw = [[] for _ in depths]
    for t, tc in enumerate(tcs):
        c, d = int(tc["comp"]), depths[int(tc["comp"])]
        assert int(tc["cbps"]) == d
        p = orc.plane(t)
        v = (np.rint(p) if p.dtype == np.float32 else p).astype(np.int64) + (1 << (d - 1))
        raw[c].append(v.reshape(-1))
        v = np.clip(v, 0, (1 << d) - 1) << (P - d)
        y, x = int(tc["out_y"]), int(tc["out_x"])
        h, w = min(v.shape[0], out[c].shape[0] - y), min(v.shape[1], out[c].shape[1] - x)
        out[c][y:y + h, x:x + w] = v[:h, :w]
    return out, [np.concatenate(r) for r in raw]


@pytest.mark.parametrize("name", sorted(n for n in streams.DEPTHS if not streams.DEPTHS[n][2].get("mct")))
def test_numpy_restatement_of_the_conversion(orc, name):
    """np.rint of float planes (integers as they are), add 1 << (d - 1), clip, shift: the oracle's frame sample for sample.
    This pins the oracle's own write_frame for unequal depths on something that is not it.  The clip cases must clip: at
    least 20 samples strictly below 0 and 20 strictly above 2^d - 1 in every component, before the clip"""
    data, kw, info, planes = decode(orc, name)
    depths = streams.DEPTHS[name][1]
    want = components(info, planes)
    got, raw = restated_frame(orc, data, kw, depths, layout_of(name)[2], lambda c: want[c].shape)
    for c in range(len(depths)):
        assert np.array_equal(got[c], want[c]), (name, c)
    if "_clip_" in name:
        for c, d in enumerate(depths):
            below, above = int((raw[c] < 0).sum()), int((raw[c] > (1 << d) - 1).sum())
            print(name, "component", c, "depth", d, "below 0:", below, "above the range:", above)
            assert below >= 20 and above >= 20, (name, c, below, above)


def test_clip_cases_are_enough():
    names = [n for n in streams.DEPTHS if "_clip_" in n]
    assert all(streams.DEPTHS[n][2].get("transform") == 0 and not streams.DEPTHS[n][2].get("mct") for n in names)
    assert {layout_of(n)[0] for n in names} >= {"rgb24", "rgb48le", "yuv420p", "yuv422p12le", "rgba", "ya8", "ya16le", "rgba64le"}
    for n in names:
        q, bits = streams.DEPTHS[n][2]["qstep"], layout_of(n)[1]
        assert q == 0.5 if bits <= 8 else 1.0 <= q <= 2.0, n


def test_both_parsers_agree(orc, host_parser, plan_diff, tmp_path):
    """return code, pix_fmt, bits_per_raw_sample, tile-component table and cbps per tile-component of every case, with its
    decode keywords; then every stream and 30 damaged copies of each through both parsers (tests/native/plan_diff.c)"""
    files = []
    for name in sorted(streams.DEPTHS):
        data = streams.depths_encode(name)
        kw = streams.depths_decode_kw(name, oracle.PIX_NAMES)
        depths = streams.DEPTHS[name][1]
        r, tcs, log, info = host_parser(data, want_info=True, **kw)
        ro, tco, info_o = _oracle_tilecomps(orc, data, want_info=True, **kw)
        assert r == ro and r >= 0, (name, r, ro, log)
        fmt, bits, _ = layout_of(name)
        for i in (info, info_o):
            assert (oracle.PIX_NAMES[i.pix_fmt], i.bits_per_raw_sample, i.ncomponents) == (fmt, bits, len(depths)), name
        assert bytes(info) == bytes(info_o), name
        assert tcs.tobytes() == tco.tobytes(), name
        assert len(tcs) % len(depths) == 0 and [int(v) for v in tcs["cbps"]] == [depths[int(c)] for c in tcs["comp"]], name
        files.append(tmp_path / (name + ".j2c"))
        files[-1].write_bytes(data)
    parses, accepted = plan_diff(files, 30)
    assert parses >= 30 * len(files) and accepted > parses // 3
