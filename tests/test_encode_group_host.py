"""CPU checks of the budget over a group of frames (htj2k_enc_opts.group_bytes): the option reaches the context-free
calls and a negative one is refused there, group_bytes = 0 changes nothing, and the numpy restatement of the selection
(tests/rc_group_model.py) keeps its own promises: a group of one is its per-frame form, the order of the frames does not
matter, and a frame's floor above the group's slope is kept."""
import numpy as np
import pytest

import ffmpeg_ht_amd as m
import rc_group_model as gm

OPTS = dict(levels=3, cb=(4, 4), irreversible=True, qstep=0.25)


def test_the_keyword_reaches_the_context_free_calls():
    w, h, fmt, bits = 75, 41, "rgb24", 8
    blocks = m.Encoder.layout(w, h, fmt, bits, group_bytes=5000, **OPTS)
    assert blocks == m.Encoder.layout(w, h, fmt, bits, **OPTS)
    assert m.Encoder.bound(w, h, fmt, bits, group_bytes=5000, **OPTS) == m.Encoder.bound(w, h, fmt, bits, **OPTS)
    assert np.array_equal(m.Encoder.band_weights(w, h, fmt, bits, group_bytes=5000, **OPTS), m.Encoder.band_weights(w, h, fmt, bits, **OPTS))
    assert m.Encoder.tiles(w, h, fmt, bits, group_bytes=5000, **OPTS) == m.Encoder.tiles(w, h, fmt, bits, **OPTS)
    assert m._enc_opts(group_bytes=7).group_bytes == 7 and m._enc_opts().group_bytes == 0


def test_a_negative_group_budget_is_refused_without_a_context():
    w, h, fmt, bits = 75, 41, "rgb24", 8
    nblk = len(m.Encoder.layout(w, h, fmt, bits, **OPTS))
    for call in (lambda: m.Encoder.layout(w, h, fmt, bits, group_bytes=-1, **OPTS),
                 lambda: m.Encoder.band_weights(w, h, fmt, bits, group_bytes=-1, **OPTS),
                 lambda: m.Encoder.tiles(w, h, fmt, bits, group_bytes=-1, **OPTS),
                 lambda: m.Encoder.assemble(w, h, fmt, bits, [b""] * nblk, group_bytes=-1, **OPTS)):
        with pytest.raises(m.Htj2kError) as e:
            call()
        assert e.value.code == -22
    assert m.Encoder.bound(w, h, fmt, bits, group_bytes=-1, **OPTS) == 0


def test_group_bytes_zero_is_the_call_without_it():
    w, h, fmt, bits = 75, 41, "rgb24", 8
    nblk = len(m.Encoder.layout(w, h, fmt, bits, **OPTS))
    assert m.Encoder.assemble(w, h, fmt, bits, [b""] * nblk, group_bytes=0, **OPTS) == m.Encoder.assemble(w, h, fmt, bits, [b""] * nblk, **OPTS)


def test_the_unit_entry_checks_its_arguments_before_the_context():
    import ctypes
    L = m.load_library()
    t = gm.random_tables(np.random.default_rng(1), [3])
    a = [np.ascontiguousarray(x, dt) for x, dt in [([3], np.int32), (t.kmax, np.int32), (t.dist, np.uint64), (t.lens, np.uint32),
                                                    (t.dskip, np.float64), (t.low0, np.uint32), (t.weight, np.float64)]]
    planes = np.zeros(3, np.int32)
    lam, est, trial = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_int()

    def call(nframes=1, kmax=a[1], room=10):
        p = [x.ctypes.data_as(ctypes.c_void_p) for x in (a[0], kmax, *a[2:])]
        return L.htj2k_enc_rc_group_select(None, nframes, *p, None, None, ctypes.c_int64(room), 1,
                                           planes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(lam), ctypes.byref(est), ctypes.byref(trial))

    assert call() == -38                                      # valid arguments, no context
    assert call(nframes=0) == -22 and call(room=-1) == -22
    assert call(kmax=np.array([0, 17, 3], np.int32)) == -22


def test_a_group_of_one_is_its_per_frame_form():
    rng = np.random.default_rng(3)
    t = gm.random_tables(rng, [90])
    full = int(gm.est_frames(t, np.zeros(90)).sum())
    for room, trial in ((0, False), (full // 2, True), (full // 7, False), (full - 1, True), (full - 1, False), (10 * full, True)):
        g, f = gm.group_select(t, room, [0.0], trial), gm.frame_select(t, room, trial)
        assert np.array_equal(g[0], f[0]) and g[1:] == f[1:], room


def test_permuting_the_frames_permutes_the_result():
    rng = np.random.default_rng(4)
    t = gm.random_tables(rng, [300, 1, 520, 77])
    floors = np.array([0.0, 0.0, 3.0e4, 0.0])
    full = int(gm.est_frames(t, np.zeros(898)).sum())
    for room in (full // 3, full // 20):
        planes, lam, est, trial = gm.group_select(t, room, floors, False)
        for order in ([3, 2, 1, 0], [2, 0, 3, 1]):
            t2, ix = t.permuted(order)
            p2, lam2, est2, trial2 = gm.group_select(t2, room, floors[order], False)
            assert np.array_equal(p2, planes[ix]) and (lam2, est2, trial2) == (lam, est, trial)


def test_floors_above_the_group_slope_are_kept():
    rng = np.random.default_rng(5)
    t = gm.random_tables(rng, [400, 400])
    full = int(gm.est_frames(t, np.zeros(800)).sum())
    free = gm.group_select(t, full // 2, None, False)
    floor = 64.0 * max(free[1], 1.0)
    planes, lam, est, _ = gm.group_select(t, full // 2, [floor, 0.0], False)
    assert lam < floor and est <= full // 2
    own = gm.selection(t, np.full(800, floor))[0]
    assert np.array_equal(planes[:400], own[:400])            # frame 0 sits at its own slope
    assert np.array_equal(planes[400:], gm.selection(t, np.full(800, lam))[0][400:])
    assert lam <= free[1]                                     # what frame 0 gave up goes to frame 1
