"""CPU check of the choice rate control's last resort makes (no GPU): enc_drop_take of j2k_enc.c, called through ctypes,
against a numpy restatement written here.  The candidates are (gain, block, bytes); the least gain goes first, among equal
gains the smaller block index; a call takes entries from `next` on while the bytes they save are below `excess`.  Gains
come from 8 values, so ties are the rule."""
import ctypes

import numpy as np
import pytest

import ffmpeg_ht_amd as m

DROP = np.dtype([("gain", "<f8"), ("block", "<i4"), ("bytes", "<i4")])
GAINS = np.array([-3.5, -1.0, 0.0, 1e-300, 0.125, 0.1250000000000001, 7.0, 1e30])


def candidates(n, seed):
    rng = np.random.default_rng(seed)
    e = np.zeros(n, DROP)
    e["gain"] = GAINS[rng.integers(0, len(GAINS), n)]
    e["block"] = rng.permutation(3 * n)[:n]            # distinct, in no order
    e["bytes"] = rng.integers(1, 4001, n)
    return e


def take(e, nxt, excess):
    L = m.load_library()
    L.enc_drop_take.restype = ctypes.c_size_t
    L.enc_drop_take.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int64,
                                ctypes.POINTER(ctypes.c_int64)]
    saved = ctypes.c_int64(-1)
    nxt = L.enc_drop_take(e.ctypes.data if len(e) else None, len(e), nxt, int(excess), ctypes.byref(saved))
    return int(nxt), int(saved.value)


def model_order(e):
    return e[np.lexsort((e["block"], e["gain"]))]      # by gain, then by block


def model_take(ordered, nxt, excess):
    """-> (new next, saved): entries from nxt on while the bytes saved are below excess"""
    csum = np.cumsum(ordered["bytes"][nxt:].astype(np.int64))
    k = 0 if excess <= 0 else min(int(np.searchsorted(csum, excess, side="left")) + 1, len(csum))
    return nxt + k, int(csum[k - 1]) if k else 0


@pytest.mark.parametrize("n", (0, 1, 2, 1000))
def test_one_call(n):
    src = candidates(n, 11 + n)
    want = model_order(src)
    total = int(src["bytes"].sum())
    for excess in (0, 1, total - 1, total, total + 1):
        e = src.copy()
        got = take(e, 0, excess)
        assert e.tobytes() == want.tobytes(), (n, excess)
        assert got == model_take(want, 0, excess), (n, excess)
        if excess >= total:
            assert got == (n, total)


@pytest.mark.parametrize("n", (0, 1, 2, 1000))
def test_calls_that_resume(n):
    src = candidates(n, 23 + n)
    want = model_order(src)
    rng = np.random.default_rng(5 + n)
    e, nxt, calls = src.copy(), 0, 0
    while True:
        excess = int(rng.choice((0, 1, 3999, 4000, 4001, 60000)))
        got = take(e, nxt, excess)
        assert got == model_take(want, nxt, excess), (n, calls, nxt, excess)
        assert e.tobytes() == want.tobytes()
        assert got[0] >= nxt and (got[0] > nxt) == (excess > 0 and nxt < n)
        nxt, calls = got[0], calls + 1
        if nxt == n and calls > 3:
            break
    assert take(e, n, 10 ** 12) == (n, 0)              # nothing left to take
