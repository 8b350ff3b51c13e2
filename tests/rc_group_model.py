"""numpy float64 restatement of the group selection (htj2k_enc_opts.group_bytes; test tooling, no tests in it), written
from the definition in include/htj2k_amd.h, not from the kernels: the candidate a block takes at a slope (single-pass
candidates), the scaled length, the header bits, est_f and the bisection on E(lambda) = sum of est_f(max(lambda,
floor_f)).  Every product is rounded on its own (numpy does not fuse), integers are summed as integers, and uint64
distortions go to float64 by round-to-nearest, as a C cast does: the result is meant to match the device bit for bit.

Next to it the group's reference allocation: rc_model.allocate over the concatenated exact tables of all frames."""
import numpy as np

import rc_model as rc

NPLANES, SKIP, STEPS = 16, -1, 64


def scaled(lens, scale):
    """bytes an estimate of `lens` stands for at `scale`: 0 stays 0, else floor(l * scale + 0.5) in 1 .. 10^9"""
    v = np.floor(lens.astype(np.float64) * scale + 0.5)
    return np.where(lens == 0, 0, np.clip(v, 1.0, 1.0e9)).astype(np.int64)


def bit_length(v):
    out = np.zeros(v.shape, np.int64)
    v = v.copy()
    while (v > 0).any():
        out += v > 0
        v >>= 1
    return out


def hdr_bits(L):
    """bits of the packet header a block of L bytes accounts for: 8 + 2 * bit length; nothing for L = 0"""
    return np.where(L > 0, 8 + 2 * bit_length(L), 0)


class Tables:
    """per block of a group: kmax, dist[16], len[16], dskip, low0, weight, scale; nblk[f] blocks per frame, concatenated"""

    def __init__(self, nblk, kmax, dist, lens, dskip, low0, weight, scale=None):
        self.nblk = np.asarray(nblk, np.int64)
        self.kmax = np.asarray(kmax, np.int64)
        self.dist = np.asarray(dist, np.uint64).reshape(-1, NPLANES)
        self.lens = np.asarray(lens, np.int64).reshape(-1, NPLANES)
        self.dskip = np.asarray(dskip, np.float64)
        self.low0 = np.asarray(low0, np.int64)
        self.weight = np.asarray(weight, np.float64)
        self.scale = np.ones(len(self.kmax)) if scale is None else np.asarray(scale, np.float64)
        self.frame = np.repeat(np.arange(len(self.nblk)), self.nblk)
        assert len(self.kmax) == self.nblk.sum() == len(self.dist) == len(self.lens)
        # what does not depend on the slope
        self.L = scaled(self.lens, self.scale[:, None])
        self.cost = (self.L + ((hdr_bits(self.L) + 7) >> 3)).astype(np.float64)
        self.wd = self.weight[:, None] * self.dist.astype(np.float64)

    def permuted(self, order):
        """the same group with its frames in another order"""
        start = np.concatenate([[0], np.cumsum(self.nblk)])
        ix = np.concatenate([np.arange(start[f], start[f + 1]) for f in order]).astype(np.int64)
        return Tables(self.nblk[list(order)], self.kmax[ix], self.dist[ix], self.lens[ix], self.dskip[ix], self.low0[ix],
                      self.weight[ix], self.scale[ix]), ix


def pick(t, lam):
    """per block the candidate of least weight * dist + lambda * (scaled length + header bytes) among the planes below
    kmax (at most 16) and "left out" (SKIP): planes from the highest down with <=, so ties go to the smaller plane and
    "left out" loses every tie.  lam: one slope per block.  -> (plane, scaled length)"""
    n = np.minimum(t.kmax, NPLANES)
    best = t.weight * t.dskip
    at = np.full(len(n), SKIP, np.int64)
    L = np.zeros(len(n), np.int64)
    for p in range(NPLANES - 1, -1, -1):
        J = t.wd[:, p] + lam * t.cost[:, p]
        take = (p < n) & (J <= best)
        best = np.where(take, J, best)
        at = np.where(take, p, at)
        L = np.where(take, t.L[:, p], L)
    return at, L


def selection(t, lam, trial=False):
    """what every block gets at per-block slopes `lam`: an all-zero block (kmax 0), and every block of a trial, keeps
    plane 0 at its plane-0 length -> (plane, scaled length)"""
    at, L = pick(t, lam)
    zero = (t.kmax == 0) | trial
    return np.where(zero, 0, at), np.where(zero, t.L[:, 0], L)


def est_frames(t, lam, trial=False):
    """est_f per frame: the scaled lengths plus the header bits, rounded up to bytes per frame"""
    _, L = selection(t, lam, trial)
    nf = len(t.nblk)
    lens = np.zeros(nf, np.int64)
    np.add.at(lens, t.frame, L)
    bits = np.zeros(nf, np.int64)
    np.add.at(bits, t.frame, hdr_bits(L))
    return lens + ((bits + 7) >> 3)


def group_select(t, room, floors=None, allow_trial=True):
    """-> (planes per block, lambda_g, est (the sum of est_f), trial).  floors: lambda_f per frame (None: 0)"""
    fl = np.zeros(len(t.nblk)) if floors is None else np.asarray(floors, np.float64)
    flb = fl[t.frame]

    def E(lam):
        return int(est_frames(t, np.maximum(lam, flb)).sum())

    if allow_trial and not (fl > 0).any() and int(t.low0.sum()) <= room:
        at, _ = selection(t, flb, True)
        return at, 0.0, int(est_frames(t, flb, True).sum()), 1
    lam = 0.0
    if E(0.0) > room:
        lo, hi = 0.0, 1.0 + float(np.max(t.weight * t.dskip))
        for _ in range(STEPS):
            mid = 0.5 * (lo + hi)
            if E(mid) <= room:
                hi = mid
            else:
                lo = mid
        lam = hi
    at, _ = selection(t, np.maximum(lam, flb))
    return at, lam, E(lam), 0


def frame_select(t, budget, allow_trial=True):
    """the per-frame form for a group of one frame, block by block in plain Python as "rate control" states it (slow:
    small tables only) -> as group_select"""
    assert len(t.nblk) == 1
    n = len(t.kmax)

    def _hdr(L):
        return 8 + 2 * L.bit_length() if L else 0

    def one(b, lam):
        best, at, L = float(t.weight[b] * t.dskip[b]), SKIP, 0
        for p in range(min(int(t.kmax[b]), NPLANES) - 1, -1, -1):
            Lp = int(t.L[b, p])
            J = float(t.weight[b] * np.float64(t.dist[b, p])) + lam * float(Lp + ((_hdr(Lp) + 7) >> 3))
            if J <= best:
                best, at, L = J, p, Lp
        return at, L

    def est(lam, final=False, trial=False):
        planes, total, bits = [], 0, 0
        for b in range(n):
            at, L = (0, int(t.L[b, 0])) if trial or (final and t.kmax[b] == 0) else one(b, lam)
            planes.append(at)
            total += L
            bits += _hdr(L)
        return planes, total + ((bits + 7) >> 3)

    if allow_trial and int(t.low0.sum()) <= budget:
        planes, e = est(0.0, True, True)
        return np.array(planes), 0.0, e, 1
    lam = 0.0
    if est(0.0)[1] > budget:
        lo, hi = 0.0, 1.0 + max(float(t.weight[b] * t.dskip[b]) for b in range(n))
        for _ in range(STEPS):
            mid = 0.5 * (lo + hi)
            if est(mid)[1] <= budget:
                hi = mid
            else:
                lo = mid
        lam = hi
    planes, e = est(lam, True)
    return np.array(planes), lam, e, 0


def random_tables(rng, nblk):
    """tables no picture would produce: kmax 0 .. 16, distortions that fall with the plane count only loosely, some
    lengths 0, scales other than 1 for some blocks"""
    n = int(np.sum(nblk))
    kmax = rng.integers(0, NPLANES + 1, n)
    dist = rng.integers(0, 1 << 40, (n, NPLANES)).astype(np.uint64)
    dist.sort(axis=1)
    lens = rng.integers(1, 5000, (n, NPLANES)).astype(np.uint32)
    lens = -np.sort(-lens.astype(np.int64), axis=1)
    lens[rng.random((n, NPLANES)) < 0.05] = 0
    lens[np.arange(NPLANES)[None, :] >= kmax[:, None]] = 0
    dskip = dist[:, -1].astype(np.float64) + rng.integers(0, 1 << 30, n)
    low0 = (lens[:, 0] * rng.uniform(0.8, 1.0, n)).astype(np.uint32)
    weight = 2.0 ** rng.uniform(-8, 4, n)
    scale = np.where(rng.random(n) < 0.3, rng.uniform(0.5, 1.5, n), 1.0)
    return Tables(nblk, kmax, dist, lens.astype(np.uint32), dskip, low0, weight, scale)


def reference_allocation(lens_frames, dists_frames, room):
    """rc_model.allocate over the concatenated exact tables (rc_model.tables) of all frames -> per frame the planes"""
    lens = [l for fr in lens_frames for l in fr]
    dists = [d for fr in dists_frames for d in fr]
    planes = rc.planes_of(rc.allocate(lens, dists, room), lens)
    out, at = [], 0
    for fr in lens_frames:
        out.append(planes[at:at + len(fr)])
        at += len(fr)
    return out
