"""numpy model of the encoder's constant-quality mode (test tooling, no tests in it), stated from the definition in
include/htj2k_amd.h ("constant quality"): the error of the 9/7 quantiser itself per block (base), the frame's distortion
D = sum of w (base + d / 4) for given planes and passes, the model PSNR, and the reference allocation: the fewest exact
bytes whose D meets the target, by bisection on the slope over the hull points, ending on the feasible side.

The reference allocates with perfect knowledge of the lengths; the product works from estimates, so it may need more
bytes but never more distortion than the target.  Everything that exists already is imported, not restated: the
candidates' distortions and lengths are rc_model's and rc_passes_model's, the coefficients enc97_model's."""
import math

import numpy as np

import enc97_model as e97
import enc_model as em
import enc_tiles_model as tm
import rc_model as rc
import rc_passes_model as pm

M_MAX = 2147483000.0                                       # the quantiser's clamp (k_quant97)


def float_planes(comps, fmt, w, h, bits, levels, mct, tile=(0, 0)):
    """the 9/7 coefficients of every component plane as the quantiser gets them (float32, Mallat layout per tile-component)"""
    v = e97.components(comps, bits, mct)
    if tuple(tile) == (0, 0):
        return [e97.fdwt97(c, levels) for c in v]
    out = [np.zeros(c.shape, np.float32) for c in v]
    for rects in tm.tile_rects(fmt, w, h, tile):
        for c, (x0, y0, x1, y1) in enumerate(rects):
            out[c][y0:y1, x0:x1] = tm.fdwt97(v[c][y0:y1, x0:x1], x0, y0, levels)
    return out


def index_planes(comps, fmt, w, h, bits, levels, mct, irreversible, qstep, tile=(0, 0)):
    """what the block coder gets: 5/3 coefficients or 9/7 indices, tiled or not"""
    if tuple(tile) != (0, 0):
        return tm.coefficient_planes(comps, fmt, w, h, bits, levels, mct, tile, qstep if irreversible else None)
    return rc.indices(comps, fmt, bits, levels, mct, irreversible, qstep)


def block_steps(blocks, qstep, bits, levels):
    """the decoder's step of every block's band (float32)"""
    st = e97.steps(qstep, bits, levels)
    return np.array([st[rc.band_entry(b)][2] for b in blocks], dtype=np.float32)


def quant_error(v, step):
    """(m, e) per sample of float32 coefficients v at `step`: c = |v| / step in float64 (the quantiser's own division),
    m = floor(c) clamped as the quantiser clamps it, e = c - (m + 1/2) where m > 0 and e = c where m = 0"""
    c = np.abs(np.asarray(v, dtype=np.float32).astype(np.float64)) / np.float64(np.float32(step))
    m = np.minimum(np.floor(c), M_MAX)
    return m, np.where(m > 0, c - (m + 0.5), c)


def base(v, step):
    """base_b: the sum of e^2 over the block, in index units"""
    e = quant_error(v, step)[1].reshape(-1)
    return float((e * e).sum())


def frame_base(fplanes, blocks, steps):
    return [base(rc.block_view(fplanes, b), s) for b, s in zip(blocks, steps)]


def cand_dist(v, plane, passes):
    """d_b of block v coded as (plane, passes) (plane -1: left out), in the units of htj2k_enc_rc_stats, as an integer"""
    if plane < 0:
        return rc.dist_skip(v)
    if passes > 1:
        return pm.dist(v, plane, passes)
    return int(rc.dist_row(v, plane + 1)[plane])


def frame_d(idx, blocks, wts, bases, planes, passes):
    """D = sum over the blocks, in their order, of w (base + d / 4)"""
    return float(sum(w * (b0 + cand_dist(rc.block_view(idx, b), p, k) / 4.0)
                     for b, w, b0, p, k in zip(blocks, wts, bases, planes, passes)))


def nsamples(fmt, w, h):
    return sum(cw * ch for cw, ch in em.comp_dims(fmt, w, h))


def psnr(d, fmt, w, h, bits):
    peak = float((1 << bits) - 1)
    return float("inf") if d <= 0 else 10.0 * math.log10(peak * peak * nsamples(fmt, w, h) / d)


def d_target(target_psnr, fmt, w, h, bits):
    peak = float((1 << bits) - 1)
    return peak * peak * nsamples(fmt, w, h) / 10.0 ** (target_psnr / 10.0)


def allocate(lens, dists, room, steps=100):
    """lens[b], dists[b]: per block the candidates' exact bytes and their share of D (w d / 4, float64), as rc.tables /
    rc_passes_model.tables list them.  -> per block the candidate of the selection with the fewest bytes whose summed
    dists stay within `room` (D_target less the sum of w base), by bisection on the slope over the hull points,
    ending on the feasible side; None when slope 0 (the least distortion every block has) is beyond `room`."""
    hulls = [rc.hull(list(l), list(d)) for l, d in zip(lens, dists)]

    def pick(lam):
        sel = [min(hp, key=lambda i: (d[i] + lam * l[i], i)) for hp, l, d in zip(hulls, lens, dists)]
        return sel, sum(d[s] for s, d in zip(sel, dists))

    sel, total = pick(0.0)
    if total > room:
        return None
    lo, hi = 0.0, max(max(d) for d in dists) + 1.0
    sel_hi, total = pick(hi)
    if total <= room:
        return sel_hi
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        if pick(mid)[1] <= room:
            lo = mid
        else:
            hi = mid
    return pick(lo)[0]
