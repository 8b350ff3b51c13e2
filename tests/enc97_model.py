"""numpy model of the lossy encoder's stages (test tooling): the forward ICT (T.800 G.3) in float32, the un-normalised
forward 9/7 lifting in float32 into the Mallat layout, the step rule of the QCD exponents and mantissas, the decoder's
f_stepsize (jpeg2000.c:214-272, as j2k_tier2.c's band_step restates it) and the float64 dead-zone quantiser.

Every float32 operation is one numpy ufunc on float32 operands, so each rounds once, as C does on x86-64 without
FMA: the vector factory's results (tools/vecgen/htj2k_enc.c) are expected bit for bit, not within a tolerance."""
import math

import numpy as np

import enc_model as em

F = np.float32
A97, B97, G97, D97 = F(1.586134342059924), F(0.052980118572961), F(0.882911075530934), F(0.443506852043971)
K97, X97 = F(1.230174104914001), F(0.812893066115961)
INV_X97 = F(1) / X97                 # `1.0f / X97`, folded in float


def components(comps, bits, mct):
    """level shift to float32 (+ ICT of components 0..2, the factory's constants and operand order)"""
    v = [(c.astype(np.int64) - (1 << (bits - 1))).astype(np.float32) for c in comps]
    if mct:
        r, g, b = v[0], v[1], v[2]
        v[0] = F(0.299) * r + F(0.587) * g + F(0.114) * b
        v[1] = F(-0.168736) * r - F(0.331264) * g + F(0.5) * b
        v[2] = F(0.5) * r - F(0.418688) * g - F(0.081312) * b
    return v


def dwt97(x, axis):
    """one forward 9/7 level along `axis`: every lifting step x + c * (left + right) on whole-sample symmetric
    extension, low-pass outputs first; a line of one sample is scaled by 1 / X"""
    x = np.moveaxis(np.asarray(x, dtype=np.float32), axis, 0)
    n = x.shape[0]
    if n == 1:
        return np.moveaxis(x * INV_X97, 0, axis)

    def ref(j):
        j = np.abs(j)
        return np.where(j >= n, 2 * (n - 1) - j, j)

    p = x.copy()
    odd, even = np.arange(1, n, 2), np.arange(0, n, 2)
    for c, pos in ((-A97, odd), (-B97, even), (G97, odd), (D97, even)):
        p[pos] = p[pos] + c * (p[ref(pos - 1)] + p[ref(pos + 1)])
    return np.moveaxis(np.concatenate([p[even], p[odd]], 0), 0, axis)


def fdwt97(plane, levels):
    """vertical then horizontal at each level, on the LL region; no early stop at a 1 x 1 region (it is scaled)"""
    p = np.array(plane, dtype=np.float32)
    h, w = p.shape
    for lev in range(levels):
        lw, lh = -(-w // (1 << lev)), -(-h // (1 << lev))
        r = dwt97(p[:lh, :lw], 0)
        p[:lh, :lw] = dwt97(r, 1)
    return p


def band_index(r, b):
    """QCD entry of band b (0 LL; 0 HL, 1 LH, 2 HH above resolution 0) of resolution r"""
    return 3 * (r - 1) + 1 + b if r else 0


def step_rule(qstep, bits, nl, g):
    """(exponent, mantissa) of band entry g: d = qstep * 2^-((l - 1) / 2) at level l (LL: l = NL)"""
    r = (g - 1) // 3 + 1 if g else 0
    lvl = nl - r + 1 if r else nl
    d = qstep * math.pow(2.0, -0.5 * (lvl - 1))
    e = math.floor(math.log2(d))
    mant = math.floor((d / math.pow(2.0, e) - 1.0) * 2048.0 + 0.5)
    if mant >= 2048:
        mant, e = 0, e + 1
    return bits - e, mant


def fstep(bits, nl, g, expn, mant):
    """the decoder's f_stepsize of band entry g, rounded where the reference's float assignments round"""
    r = (g - 1) // 3 + 1 if g else 0
    orient = (g - 1) % 3 + 1 if g else 0
    step = F(math.ldexp(1.0, bits - expn))
    step = F(float(step) * (mant / 2048.0 + 1.0))
    lowpass = 0
    if orient in (1, 2):
        step = step * (X97 * F(2))
        lowpass = 1
    elif orient == 3:
        step = step * (X97 * X97 * F(4))
    return F(float(step) * math.pow(float(K97), 2 * (nl + 1 - r) + lowpass - 2))


def steps(qstep, bits, nl):
    """[(exponent, mantissa, decoder step)] of every band entry"""
    out = []
    for g in range(3 * nl + 1):
        e, mnt = step_rule(qstep, bits, nl, g)
        out.append((e, mnt, fstep(bits, nl, g, e, mnt)))
    return out


def band_map(w, h, nl):
    """band entry of every sample of a w x h Mallat plane"""
    def level(n):
        x = np.arange(n, dtype=np.int64)
        lv = np.full(n, nl + 1)
        for l in range(nl, 0, -1):
            lv = np.where((x << l) >= n, l, lv)
        return lv
    lx, ly = level(w)[None, :], level(h)[:, None]
    l = np.minimum(lx, ly)
    g = 3 * (nl - l) + (lx == l) * 1 + (ly == l) * 2
    return np.where(l > nl, 0, g)


def quantise(plane, step_of_band, nl):
    """float64 dead zone: floor(|v| / step), clamped at 2147483000, with the sign of v"""
    h, w = plane.shape
    st = np.array([float(s) for s in step_of_band], dtype=np.float64)[band_map(w, h, nl)]
    m = np.minimum(np.floor(np.abs(plane.astype(np.float64)) / st), 2147483000.0).astype(np.int64)
    return np.where(plane < 0, -m, m).astype(np.int32)


def index_planes(comps, fmt, bits, levels, mct, qstep):
    """the quantisation indices of every component plane, as the encoder hands them to the HT block coder"""
    st = steps(qstep, bits, levels)
    return [quantise(fdwt97(c, levels), [s for _, _, s in st], levels) for c in components(comps, bits, mct)]


def vecgen_args(fmt, w, h, bits, levels, cb, mct, guard, qstep):
    a = em.vecgen_args(fmt, w, h, bits, levels, cb, mct, guard)
    a.update(transform=0, qstep=qstep)
    return a


def exponents_valid(qstep, bits, nl):
    return all(0 <= e <= 31 for e, _, _ in steps(qstep, bits, nl))
