"""CPU checks of the encoder's constant-quality option (htj2k_enc_opts.target_psnr): what the context-free calls refuse,
that the field changes no header, the product's band weights (htj2k_enc_band_weights) against the impulse responses
of tests/rc_model.py, and the numpy model of the quantiser's own error (tests/cq_model.py) against sums done by hand."""
import ctypes

import numpy as np
import pytest

import cq_model as cq
import enc_model as em
import ffmpeg_ht_amd as m
import rc_model as rc

LAYOUTS = [("gray", 8), ("rgb24", 8), ("yuv420p10le", 10)]
# (w, h, levels, tile)
SHAPES = [(200, 136, 3, (0, 0)), (160, 96, 5, (0, 0)), (160, 96, 3, (64, 64))]


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -float("inf")])
def test_bad_targets_are_refused_without_a_context(bad):
    for opts in (dict(), dict(irreversible=True, qstep=0.5), dict(tile=(64, 64), ht_passes=3)):
        assert m.Encoder.bound(64, 48, "rgb24", 8, target_psnr=bad, **opts) == 0
        with pytest.raises(m.Htj2kError) as e:
            m.Encoder.layout(64, 48, "rgb24", 8, target_psnr=bad, **opts)
        assert e.value.code == -22
        with pytest.raises(m.Htj2kError) as e:
            m.Encoder.band_weights(64, 48, "rgb24", 8, target_psnr=bad, **opts)
        assert e.value.code == -22
        with pytest.raises(m.Htj2kError) as e:
            m.Encoder.tiles(64, 48, "rgb24", 8, target_psnr=bad, **opts)
        assert e.value.code == -22
        nblk = len(m.Encoder.layout(64, 48, "rgb24", 8, **opts))
        with pytest.raises(m.Htj2kError) as e:
            m.Encoder.assemble(64, 48, "rgb24", 8, [b""] * nblk, cap=1 << 16, target_psnr=bad, **opts)
        assert e.value.code == -22


def test_the_field_is_the_zero_tail_and_changes_no_header():
    o = m.EncOpts()
    m.load_library().htj2k_enc_opts_default(ctypes.byref(o))
    assert o.target_psnr == 0.0 and m._enc_opts().target_psnr == 0.0 and m._enc_opts(target_psnr=40).target_psnr == 40.0
    assert m.EncOpts(5, 6, 6, -1, 0).target_psnr == 0.0
    assert m.EncOpts.target_psnr.offset + ctypes.sizeof(ctypes.c_double) == ctypes.sizeof(m.EncOpts)     # the last field
    rng = np.random.default_rng(3)
    for fmt, bits in LAYOUTS:
        for opts in (dict(levels=3, cb=(4, 4)), dict(levels=3, cb=(4, 4), irreversible=True, qstep=0.25),
                     dict(levels=2, cb=(5, 3), tile=(64, 48), ht_passes=2)):
            w, h = 150, 90
            blocks = m.Encoder.layout(w, h, fmt, bits, **opts)
            assert m.Encoder.layout(w, h, fmt, bits, target_psnr=40, **opts) == blocks
            assert m.Encoder.bound(w, h, fmt, bits, target_psnr=40, **opts) == m.Encoder.bound(w, h, fmt, bits, **opts) > 0
            assert m.Encoder.tiles(w, h, fmt, bits, target_psnr=40, **opts) == m.Encoder.tiles(w, h, fmt, bits, **opts)
            data = [bytes(rng.integers(0, 255, size=int(rng.integers(0, 40)), dtype=np.uint8)) for _ in blocks]
            assert m.Encoder.assemble(w, h, fmt, bits, data, target_psnr=40, **opts) == m.Encoder.assemble(w, h, fmt, bits, data, **opts)
            assert np.array_equal(m.Encoder.band_weights(w, h, fmt, bits, target_psnr=40, **opts),
                                  m.Encoder.band_weights(w, h, fmt, bits, **opts))


def weight_differences():
    """{case: worst relative difference of the product's block weights from rc_model.weights}, and the check that the
    blocks of one band of a component have one weight"""
    out = {}
    for fmt, bits in LAYOUTS:
        for irrev in (False, True):
            for w, h, levels, tile in SHAPES:
                opts = dict(levels=levels, cb=(4, 4), irreversible=irrev, qstep=0.25, tile=tile)
                blocks = m.Encoder.layout(w, h, fmt, bits, **opts)
                got = m.Encoder.band_weights(w, h, fmt, bits, **opts)
                assert got.shape == (len(blocks),) and got.dtype == np.float64 and (got > 0).all()
                want = rc.weights(fmt, w, h, bits, levels, em.mct_default(fmt), irrev, 0.25)
                per_band = {}
                for g, b in zip(got, blocks):
                    assert per_band.setdefault((b["comp"], rc.band_entry(b)), g) == g        # equal, not close
                assert set(per_band) == set(want)
                out[fmt, irrev, w, h, levels, tile] = max(abs(per_band[k] / want[k] - 1.0) for k in want)
    return out


# computed here on the CPU (table in DESIGN.md 3.5, "Constant quality"): the worst relative difference over the cases of
# weight_differences().  The product takes the norm of the band's synthesis response in free space, rc_model.weights
# sends an impulse through the oracle's inverse transform of the frame itself: at 3 levels the two agree to 2.3e-6, at
# 5 levels of a 160 x 96 frame (a chroma band of 3 x 2 samples) the frame's edges fold the response back.
WEIGHT_DIFF = 0.63681


def test_band_weights_against_the_impulse_model():
    diffs = weight_differences()
    for k, v in diffs.items():
        print(k, "%.3e" % v)
    assert max(diffs.values()) <= 1.25 * WEIGHT_DIFF
    # where the bands are large against the filters' reach the two constructions are the same number
    assert all(v < 1e-5 for k, v in diffs.items() if k[4] == 3 and k[5] == (0, 0))


def test_band_weights_cap_and_count():
    L = m.load_library()
    o = m._enc_opts(levels=3, irreversible=True, qstep=0.5)
    n = L.htj2k_enc_band_weights(200, 136, 1, 8, ctypes.byref(o), None, 0)
    assert n == L.htj2k_enc_layout(200, 136, 1, 8, ctypes.byref(o), None, 0) > 4
    w = np.full(n + 2, -7.0)
    assert L.htj2k_enc_band_weights(200, 136, 1, 8, ctypes.byref(o), w.ctypes.data_as(ctypes.c_void_p), 3) == n
    assert (w[:3] > 0).all() and (w[3:] == -7.0).all()
    full = m.Encoder.band_weights(200, 136, "rgb24", 8, levels=3, irreversible=True, qstep=0.5)
    assert np.array_equal(full[:3], w[:3])
    assert L.htj2k_enc_band_weights(0, 136, 1, 8, ctypes.byref(o), None, 0) == -22


def test_the_model_of_the_quantiser_error_by_hand():
    f = np.float32
    # exact multiples of the step: c = m, e = -1/2 each (m > 0); a zero is no error
    assert cq.base(np.array([[3.0, 1.5, 0.0, 4.5]], f), 1.5) == 3 * 0.25
    # negative values count by magnitude
    assert cq.base(np.array([[-3.0, -1.5, -0.0]], f), 1.5) == 2 * 0.25
    # below one step: the index is 0 and the whole magnitude is the error
    assert cq.base(np.array([[0.25, -0.5, 0.75]], f), 1.0) == 0.25 ** 2 + 0.5 ** 2 + 0.75 ** 2
    # mixed, step 1/32: 0.5 -> c 16, e -1/2; 0.515625 -> c 16.5, e 0; 0.03 -> c 0.96 (of the float32 0.03), e c; -1/64 -> c 1/2
    c3 = float(f(0.03)) * 32
    assert cq.base(np.array([[0.5, 0.515625], [0.03, -1 / 64]], f), 1 / 32) == 0.25 + 0.0 + c3 * c3 + 0.25
    # a step that is no power of two divides in float64 by the float32 step, as the quantiser does
    st = float(f(3.7))
    want = sum(((v / st) - (np.floor(v / st) + 0.5)) ** 2 if v >= st else (v / st) ** 2 for v in (10.0, 3.5, 7.5))
    assert cq.base(np.array([[10.0, -3.5, 7.5]], f), 3.7) == pytest.approx(want, rel=1e-15)
    m_, e = cq.quant_error(np.array([7.5, -3.5], f), 3.7)
    assert m_.tolist() == [2.0, 0.0] and e[1] == 3.5 / st
    # the clamp of the quantiser
    m_, e = cq.quant_error(np.array([3.0e9], f), 1.0)
    assert m_[0] == cq.M_MAX and e[0] == float(f(3.0e9)) - (cq.M_MAX + 0.5)


def test_the_reference_allocation_on_a_toy():
    # two blocks; candidates by decreasing bytes, the last one "left out"
    lens = [[10, 6, 0], [8, 3, 0]]
    dists = [[0.0, 4.0, 20.0], [0.0, 1.0, 10.0]]             # slopes 1 and 16 / 6; 0.2 and 3
    assert cq.allocate(lens, dists, -1.0) is None
    assert cq.allocate(lens, dists, 0.0) == [0, 0]
    assert cq.allocate(lens, dists, 1.0) == [0, 1]              # 5 bytes for 1: slope 0.2, the cheapest step
    assert cq.allocate(lens, dists, 5.0) == [1, 1]
    assert cq.allocate(lens, dists, 20.9) == [1, 1]             # ending on the feasible side
    assert cq.allocate(lens, dists, 21.0) == [2, 1] == cq.allocate(lens, dists, 29.9)
    assert cq.allocate(lens, dists, 30.0) == [2, 2] == cq.allocate(lens, dists, 1e9)
    for room in (0.0, 0.5, 1.0, 4.9, 5.0, 12.0, 13.0, 21.0, 29.0, 100.0):
        sel = cq.allocate(lens, dists, room)
        assert sum(d[s] for s, d in zip(sel, dists)) <= room
