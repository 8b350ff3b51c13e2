"""numpy model of the encoder's rate control (test tooling, no tests in it): block rectangles from first principles
(T.800 Annex B, one tile, maximal precincts), the distortion of dropping bit-planes as the product defines it, exact
cleanup lengths from vecgen's encode_block of the shifted indices, band weights from impulse responses through the
oracle's inverse transform and inverse component transform, and the allocation itself: per block the lower convex hull
of (length, weighted distortion) over "plane 0 .. 15" and "left out", and a bisection on the slope in float64.

The model allocates with perfect knowledge of the lengths.  The product works from estimates and corrects afterwards,
so it can approach the model but is not compared with it byte for byte."""
import numpy as np

import enc97_model as e97
import enc_model as em
import oracle
import vecgen

NPLANES = 16
SKIP = -1


def ceil_div(a, b):
    return -(-a // b)


def block_rects(fmt, w, h, levels, cb):
    """the code-blocks of a frame in packet order (LRCP, one precinct per resolution): dicts comp/res/band/x/y/w/h with
    the rectangle in the component's Mallat plane.  Band b of resolution r > 0 covers
    ceil((tc - 2^(nb-1) xo) / 2^nb) (T.800 B-15) with nb = levels - r + 1; the block grid is anchored at 0."""
    out = []
    dims = em.comp_dims(fmt, w, h)
    for r in range(levels + 1):
        for c, (cw, ch) in enumerate(dims):
            nb = levels - r + 1 if r else levels
            for band in ([0] if r == 0 else [1, 2, 3]):
                xo, yo = band & 1, band >> 1
                if r == 0:
                    bw, bh = ceil_div(cw, 1 << nb), ceil_div(ch, 1 << nb)
                else:
                    bw = max(0, ceil_div(cw - (xo << (nb - 1)), 1 << nb))
                    bh = max(0, ceil_div(ch - (yo << (nb - 1)), 1 << nb))
                if bw == 0 or bh == 0:
                    continue
                # the low-pass part of the next lower resolution sits first in the Mallat layout
                lw, lh = ceil_div(cw, 1 << nb), ceil_div(ch, 1 << nb)
                sx, sy = (lw if xo else 0), (lh if yo else 0)
                bx, by = 1 << cb[0], 1 << cb[1]
                for y0 in range(0, bh, by):
                    for x0 in range(0, bw, bx):
                        out.append(dict(comp=c, res=r, band=band, x=sx + x0, y=sy + y0, w=min(bx, bw - x0), h=min(by, bh - y0)))
    return out


def indices(comps, fmt, bits, levels, mct, irreversible, qstep):
    """the quantisation indices of every component plane (Mallat layout), as the block coder gets them"""
    if irreversible:
        return e97.index_planes(comps, fmt, bits, levels, mct, qstep)
    return [p.astype(np.int32) for p in em.coefficient_planes(comps, fmt, bits, levels, mct)]


def shifted(v, p):
    """sign(v) * (|v| >> p)"""
    v = np.asarray(v, dtype=np.int64)
    return (np.sign(v) * (np.abs(v) >> p)).astype(np.int32)


def recon(v, p):
    """the decoder's mid-point reconstruction of shifted(v, p), in index units: sign * (((|v| >> p) << p) + 2^(p-1))"""
    v = np.asarray(v, dtype=np.int64)
    s = np.abs(v) >> p
    half = (1 << (p - 1)) if p >= 1 else 0
    return np.sign(v) * np.where(s > 0, (s << p) + half, 0)


def dist_row(v, nplanes=NPLANES):
    """sum of d^2 per plane, d twice the error of the mid-point reconstruction against m + 1/2 (uint64)"""
    m = np.abs(np.asarray(v, dtype=np.int64)).reshape(-1)
    m = m[m > 0]
    out = np.zeros(nplanes, dtype=np.uint64)
    for p in range(nplanes):
        s = m >> p
        d = np.where(s == 0, 2 * m + 1, 2 * m + 1 - 2 * (s << p) - (1 << p))
        if m.size and int(m.max()) < (1 << 24):            # |d| < 2^26 and at most 4096 samples: int64 is exact
            out[p] = np.uint64(int((d * d).sum()))
        elif m.size:
            out[p] = np.uint64(int((d.astype(object) ** 2).sum()))
    return out


def dist_skip(v):
    """distortion of leaving the block out, as a Python integer"""
    m = np.abs(np.asarray(v, dtype=np.int64)).reshape(-1)
    return int(((2 * m[m > 0] + 1).astype(object) ** 2).sum()) if (m > 0).any() else 0


def code_block(v, p=0):
    """(bytes, lcup, max_u) of vecgen's cleanup pass of shifted(v, p); (b"", 0, 0) when it is all zero or p < 0"""
    if p < 0:
        return b"", 0, 0
    s = shifted(v, p)
    if not s.any():
        return b"", 0, 0
    d, lcup, _, mu = vecgen.encode_block(s)
    return d[:lcup], lcup, mu


def len_row(v, nplanes=NPLANES):
    """exact cleanup bytes per plane"""
    return np.array([code_block(v, p)[1] for p in range(nplanes)], dtype=np.int64)


def block_view(planes, b):
    return planes[b["comp"]][b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]]


def band_entry(b):
    return 3 * (b["res"] - 1) + b["band"] if b["res"] else 0


def weights(fmt, w, h, bits, levels, mct, irreversible, qstep):
    """{(comp, band entry): squared error of the output pixels per unit of squared index error}: a unit impulse in the
    middle of the band through oracle.idwt, times the decoder's step (9/7), times the squared column norm of the
    inverse component transform measured through oracle.mct"""
    out = {}
    dims = em.comp_dims(fmt, w, h)
    col = [1.0, 1.0, 1.0]
    if mct:
        for k in range(3):
            dt = np.float32 if irreversible else np.int32
            amp = 1 if irreversible else 64             # the RCT floors: a larger impulse keeps its linear part
            p = [np.zeros(4, dt) for _ in range(3)]
            p[k][:] = amp
            r = oracle.mct(0 if irreversible else 1, *p)
            col[k] = float(sum((x.astype(np.float64)[0] / amp) ** 2 for x in r))
    steps = e97.steps(qstep, bits, levels) if irreversible else None
    rects = block_rects(fmt, w, h, levels, (6, 6))
    for c, (cw, ch) in enumerate(dims):
        bands = {}
        for b in rects:
            if b["comp"] != c:
                continue
            g = band_entry(b)
            x0, y0, x1, y1 = bands.get(g, (1 << 30, 1 << 30, 0, 0))
            bands[g] = (min(x0, b["x"]), min(y0, b["y"]), max(x1, b["x"] + b["w"]), max(y1, b["y"] + b["h"]))
        for g, (x0, y0, x1, y1) in bands.items():
            plane = np.zeros((ch, cw), np.float32 if irreversible else np.int32)
            amp = 1.0 if irreversible else 1024
            plane[(y0 + y1) // 2, (x0 + x1) // 2] = amp
            y = oracle.idwt(plane, ((0, cw), (0, ch)), levels, 0 if irreversible else 1).astype(np.float64) / amp
            gain = float((y ** 2).sum())
            st = float(steps[g][2]) if irreversible else 1.0
            out[(c, g)] = gain * st * st * (col[c] if mct and c < 3 else 1.0)
    return out


def hull(lens, dists):
    """indices of the candidates on the lower convex hull of (length, distortion), by decreasing length"""
    order = sorted(range(len(lens)), key=lambda i: (-lens[i], dists[i], i))
    pts = []
    for i in order:
        if pts and lens[i] == lens[pts[-1]]:
            continue                                     # same length, not less distortion
        if pts and dists[i] <= dists[pts[-1]]:
            while pts and dists[i] <= dists[pts[-1]]:
                pts.pop()                                # shorter and no worse: the longer one is never taken
        while len(pts) >= 2:
            a, b = pts[-2], pts[-1]
            # slope from a to b must be less steep than from b to i (convexity), else b is above the hull
            if (dists[b] - dists[a]) * (lens[b] - lens[i]) >= (dists[i] - dists[b]) * (lens[a] - lens[b]):
                pts.pop()
            else:
                break
        pts.append(i)
    return pts


def allocate(lens, dists, budget, steps=100, moves=64):
    """lens[b], dists[b]: per block the candidates' exact bytes and weighted distortions (float64), candidate k < NPLANES
    = plane k, the last = left out.  -> per block the plane (SKIP: left out) of the selection with the least total
    distortion whose bytes fit `budget`, by bisection on the slope over the hull points (ties to the longer code),
    ending on the feasible side; what the last step of the bisection leaves of the budget then goes, steepest slope
    first, to blocks that have a longer candidate with less distortion that still fits (on the hull or not: with a
    few dozen blocks the hull points alone leave a visible part of a small budget unused; at most `moves` of them)."""
    hulls = [hull(list(l), list(d)) for l, d in zip(lens, dists)]

    def pick(lam):
        sel, total = [], 0
        for hp, l, d in zip(hulls, lens, dists):
            best = min(hp, key=lambda i: (d[i] + lam * l[i], i))
            sel.append(best)
            total += int(l[best])
        return sel, total

    sel, total = pick(0.0)
    if total <= budget:
        return sel
    lo, hi = 0.0, max(max(d) for d in dists) + 1.0
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        if pick(mid)[1] <= budget:
            hi = mid
        else:
            lo = mid
    sel, total = pick(hi)
    for _ in range(moves):
        best = None
        for k, (hp, l, d) in enumerate(zip(hulls, lens, dists)):
            for nxt in range(len(l)):
                if l[nxt] <= l[sel[k]] or d[nxt] >= d[sel[k]] or total + l[nxt] - l[sel[k]] > budget:
                    continue
                slope = (d[sel[k]] - d[nxt]) / (l[nxt] - l[sel[k]])
                if best is None or slope > best[0]:
                    best = (slope, k, nxt)
        if best is None:
            return sel
        total += lens[best[1]][best[2]] - lens[best[1]][sel[best[1]]]
        sel[best[1]] = best[2]
    return sel


def _rows(job):
    v, wt, nplanes = job
    kmax = int(np.abs(v.astype(np.int64)).max()).bit_length()
    n = min(kmax, nplanes)
    if n == 0:                                            # all zero: plane 0, nothing to code
        return [0], [0.0]
    l = [int(x) for x in len_row(v, n)] + [0]
    d = [wt * float(int(x)) for x in dist_row(v, n)] + [wt * float(dist_skip(v))]
    return l, d


def tables(idx_planes, blocks, wts, nplanes=NPLANES):
    """(lens, dists) for allocate(): exact lengths and weighted distortions of every block's candidates (the last one
    "left out" unless the block is all zero)"""
    rows = [_rows((block_view(idx_planes, b), wts[(b["comp"], band_entry(b))], nplanes)) for b in blocks]
    return [r[0] for r in rows], [r[1] for r in rows]


def planes_of(sel, lens):
    """candidate indices of allocate() -> planes (SKIP for the last candidate of a block that has coded ones)"""
    return [SKIP if (len(l) > 1 and s == len(l) - 1) else s for s, l in zip(sel, lens)]


def psnr(a_planes, b_planes, bits):
    se, n = 0.0, 0
    for a, b in zip(a_planes, b_planes):
        d = a.reshape(-1).astype(np.float64) - b.reshape(-1).astype(np.float64)
        se += float((d * d).sum())
        n += d.size
    peak = float((1 << bits) - 1)
    return float("inf") if se == 0 else 10.0 * np.log10(peak * peak * n / se)
