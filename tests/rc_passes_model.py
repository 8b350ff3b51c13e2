"""numpy model of HT refinement passes in the encoder (test tooling, no tests in it): which samples the SigProp pass
visits, what the decoder reconstructs from a block coded as "cleanup at plane p + 1, SigProp (and MagRef) at plane p",
the exact bit counts of the two passes, the fallback rule, exact bytes from vecgen's encode_block of the shifted
indices, and whole streams through Encoder.assemble.  Everything is stated from the definition (T.814 7.4, 7.5), on the
CPU; the product is compared with it, never the other way round."""
import numpy as np

import ffmpeg_ht_amd as m
import rc_model as rc
import vecgen


def scan_order(w, h):
    """the samples (x, y) of a w x h block in SigProp order: stripes of 4 rows, groups of 4 columns, columns first"""
    for y0 in range(0, h, 4):
        for x0 in range(0, w, 4):
            for x in range(x0, min(x0 + 4, w)):
                for y in range(y0, min(y0 + 4, h)):
                    yield x, y


def membership_serial(v, p):
    """the definition, sample by sample in scan order"""
    mag = np.abs(np.asarray(v, dtype=np.int64))
    h, w = mag.shape
    sig = np.zeros((h + 2, w + 2), dtype=bool)
    sig[1:-1, 1:-1] = (mag >> (p + 1)) != 0
    new = np.zeros_like(sig)
    mem = np.zeros_like(sig)
    one = (mag >> p) == 1
    for x, y in scan_order(w, h):
        if sig[y + 1, x + 1]:
            continue
        nb = sig[y:y + 3, x:x + 3] | new[y:y + 3, x:x + 3]     # the centre itself is neither yet
        if nb.any():
            mem[y + 1, x + 1] = True
            new[y + 1, x + 1] = bool(one[y, x])
    return sig[1:-1, 1:-1], mem[1:-1, 1:-1], new[1:-1, 1:-1]


def membership(v, p):
    """(sigma, member, newsig) bool arrays of block v for refinement plane p: sigma = (|v| >> (p + 1)) != 0; a sample
    with sigma = 0 is a member when, at its visit, one of its 8 neighbours has sigma = 1 or is a member visited earlier
    whose bit (|v| >> p) == 1; newsig = member with that bit.  Whole-array steps while they settle quickly (a step adds
    the members whose cause is already known; the relation is acyclic, so the fixed point is the definition's), else the
    definition sample by sample."""
    mag = np.abs(np.asarray(v, dtype=np.int64))
    h, w = mag.shape
    ys, xs = np.mgrid[0:h, 0:w]
    order = np.full((h + 2, w + 2), -1, dtype=np.int64)
    order[1:-1, 1:-1] = (ys // 4) * (4 * w) + xs * np.minimum(4, h - (ys // 4) * 4) + ys % 4
    sig = np.zeros((h + 2, w + 2), dtype=bool)
    sig[1:-1, 1:-1] = (mag >> (p + 1)) != 0
    one = np.zeros_like(sig)
    one[1:-1, 1:-1] = (mag >> p) == 1
    mem = np.zeros_like(sig)
    me = order[1:-1, 1:-1]
    for _ in range(24):
        new = mem & one
        hit = np.zeros((h, w), dtype=bool)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if dy == 1 and dx == 1:
                    continue
                hit |= sig[dy:dy + h, dx:dx + w] | (new[dy:dy + h, dx:dx + w] & (order[dy:dy + h, dx:dx + w] < me))
        nxt = hit & ~sig[1:-1, 1:-1]
        if np.array_equal(nxt, mem[1:-1, 1:-1]):
            return sig[1:-1, 1:-1], nxt, nxt & one[1:-1, 1:-1]
        mem[1:-1, 1:-1] = nxt
    return membership_serial(v, p)


def falls_back(v, p, passes):
    """the block keeps one pass at plane p: nothing significant at p + 1, or Dref would be empty (only SigProp asked
    for, and it has no member: every sample is significant)"""
    sig, mem, _ = membership(v, p)
    return passes < 2 or not sig.any() or (passes == 2 and not mem.any())


def recon2(v, p, passes):
    """twice the magnitude the decoder reconstructs for every sample (0: the sample decodes to 0), after the fallback
    rule.  One pass at p: 2 ((m >> p) << p) + 2^p where m >> p != 0."""
    mag = np.abs(np.asarray(v, dtype=np.int64))
    if falls_back(v, p, passes):
        return np.where(mag >> p, 2 * ((mag >> p) << p) + (1 << p), 0)
    sig, _, new = membership(v, p)
    q = p if passes == 3 else p + 1
    return np.where(sig, 2 * ((mag >> q) << q) + (1 << q), np.where(new, 3 << p, 0))


def dist(v, p, passes):
    """sum of d^2, d = 2 m + 1 - recon2 where m != 0 (the units of htj2k_enc_rc_stats), as a Python integer"""
    mag = np.abs(np.asarray(v, dtype=np.int64))
    d = np.where(mag > 0, 2 * mag + 1 - recon2(v, p, passes), 0)
    return int((d.astype(object) ** 2).sum())


def bit_counts(v, p):
    """(SigProp bits, MagRef bits) of the refinement passes at plane p: a bit per member and a sign per newly significant
    one; a bit per significant sample"""
    sig, mem, new = membership(v, p)
    return int(mem.sum()) + int(new.sum()), int(sig.sum())


def code_block(v, p, passes):
    """(bytes Dcup || Dref, lcup, lref, max_u, passes coded) of block v with refinement plane p, by vecgen's
    encode_block of the shifted indices, after the fallback rule; (b"", 0, 0, 0, 1) when nothing is coded"""
    if p < 0:
        return b"", 0, 0, 0, 1
    if falls_back(v, p, passes):
        d, lcup, mu = rc.code_block(v, p)
        return d, lcup, 0, mu, 1
    d, lcup, lref, mu = vecgen.encode_block(rc.shifted(v, p), passes=passes)
    assert lref > 0
    return d[:lcup + lref], lcup, lref, mu, passes


def frame_blocks(idx_planes, blocks, passes, plane=0):
    """code_block of every block of a frame (blocks: Encoder.layout's) at one refinement plane"""
    return [code_block(rc.block_view(idx_planes, b), plane, passes) for b in blocks]


def assemble(coded, w, h, fmt, bits, planes=None, **opts):
    """the stream of blocks coded by code_block, through the product's host writer"""
    opts = {k: v for k, v in opts.items() if k != "ht_passes"}
    return m.Encoder.assemble(w, h, fmt, bits, [c[0] for c in coded], max_u=[c[3] for c in coded],
                              planes=[0] * len(coded) if planes is None else planes, lref=[c[2] for c in coded],
                              passes=[c[4] for c in coded], **opts)


def frame_stream(comps, fmt, w, h, bits, passes, levels=5, cb=(6, 6), mct=None, irreversible=False, qstep=1.0, **opts):
    """what the encoder writes for a frame without a budget and ht_passes = passes: coefficient model -> vecgen blocks
    with the fallback rule -> Encoder.assemble.  opts: tile, guard_bits.  -> (stream, coded blocks, index planes, layout)"""
    import enc_model as em
    import enc_tiles_model as tm
    mct = em.mct_default(fmt) if mct is None else mct
    if opts.get("tile", (0, 0)) != (0, 0):
        idx = tm.coefficient_planes(comps, fmt, w, h, bits, levels, mct, opts["tile"], qstep if irreversible else None)
    else:
        idx = rc.indices(comps, fmt, bits, levels, mct, irreversible, qstep)
    kw = dict(levels=levels, cb=cb, mct=int(mct), irreversible=irreversible, qstep=qstep, **opts)
    blocks = m.Encoder.layout(w, h, fmt, bits, **kw)
    coded = frame_blocks(idx, blocks, passes)
    return assemble(coded, w, h, fmt, bits, **kw), coded, idx, blocks


def tables(idx_planes, blocks, wts, maxpass, nplanes=rc.NPLANES):
    """(lens, dists, cands) for rc.allocate(): per block the candidates' exact bytes (Lcup + Lref), weighted distortions
    and what they are, (plane, passes): one pass at every plane below the block's highest, then for every plane p with
    something significant at p + 1 the candidates of 2 .. maxpass passes that do not fall back, then (rc.SKIP, 1), "left
    out" (an all-zero block has the one candidate (0, 1))"""
    lens, dists, cands = [], [], []
    for b in blocks:
        v = rc.block_view(idx_planes, b)
        wt = wts[(b["comp"], rc.band_entry(b))]
        n = min(int(np.abs(v.astype(np.int64)).max()).bit_length(), nplanes)
        if n == 0:
            lens.append([0]); dists.append([0.0]); cands.append([(0, 1)])
            continue
        c = [(p, 1) for p in range(n)]
        l = [int(x) for x in rc.len_row(v, n)]
        d = [wt * float(int(x)) for x in rc.dist_row(v, n)]
        for p in range(min(n - 1, nplanes - 1)):
            for k in range(2, maxpass + 1):
                if falls_back(v, p, k):
                    continue
                _, lcup, lref, _, _ = code_block(v, p, k)
                c.append((p, k)); l.append(lcup + lref); d.append(wt * float(dist(v, p, k)))
        c.append((rc.SKIP, 1)); l.append(0); d.append(wt * float(rc.dist_skip(v)))
        lens.append(l); dists.append(d); cands.append(c)
    return lens, dists, cands


def chosen(sel, cands):
    """rc.allocate's candidate indices -> (planes, passes)"""
    return [c[s][0] for s, c in zip(sel, cands)], [c[s][1] for s, c in zip(sel, cands)]
