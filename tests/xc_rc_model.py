"""numpy model of the transcoder's byte budget (include/htj2k_amd.h, "transcoding"), test tooling with no
tests in it: a restatement on top of xc_model (the block rule), rc_model (distortions, exact cleanup lengths, the
allocation) and rc_passes_model (the refinement passes).

A source block comes with (pr, k): the plane of its last pass and its HT passes.  Under a budget it is seen as
m' = |index| >> pr, in planes p' = p - pr, and its candidates are what an encoder call with ht_passes = 3 offers on m',
less what the source cannot back at p' = 0:  k = 1 nothing;  k = 2 one pass and three passes;  k = 3 one pass.  The
weight is the band's times 4^pr.  Everything is stated from the definition, on the CPU; the product is compared with it,
never the other way round."""
import numpy as np

import rc_model as rc
import rc_passes_model as pm

DISABLED = (1 << 64) - 1                                   # the distortion of a candidate the source cannot back
ALLOWED_AT_0 = {1: (1, 2, 3), 2: (2,), 3: (2, 3)}          # passes a candidate at p' = 0 may have, by the source's k


def relative(idx, pr):
    """sign * (|index| >> pr): the block as the budget sees it"""
    return rc.shifted(idx, pr)


def weight(band_weight, pr):
    return band_weight * 4.0 ** pr


def absolute(pr, p_rel):
    """a selection's relative plane back to a plane of the indices (rc.SKIP stays)"""
    return rc.SKIP if p_rel < 0 else pr + p_rel


def own_form(v_rel, k):
    """(relative plane of the last pass, passes) of the source's own form: k passes at p' = 0, or, where the refinement
    falls back (nothing significant at pc, or SigProp alone would write nothing), one pass at p' = 1"""
    if k > 1 and pm.falls_back(v_rel, 0, k):
        return 1, 1
    return 0, k


def allowed(v_rel, k, p_rel, passes):
    """is (p', passes) a candidate of a block whose source had k passes?  Coded candidates only; p' >= 0"""
    if p_rel == 0 and passes not in ALLOWED_AT_0[k]:
        return False
    kmax = int(np.abs(v_rel.astype(np.int64)).max()).bit_length()
    if passes == 1:
        return p_rel < max(kmax, 1)
    return p_rel + 1 < kmax and not pm.falls_back(v_rel, p_rel, passes)


def pass_rows(v, nplanes):
    """(dist2, dist3, sp_bits, mr_bits) of block v as htj2k_enc_rc_stats_passes states them: no fall-back rule in the
    distortions, zeros where nothing is significant at p + 1"""
    mag = np.abs(v.astype(np.int64))
    kmax = int(mag.max()).bit_length()
    d2, d3 = np.zeros(nplanes, np.uint64), np.zeros(nplanes, np.uint64)
    sp, mr = np.zeros(nplanes, np.uint32), np.zeros(nplanes, np.uint32)
    for p in range(min(nplanes, max(kmax - 1, 0))):
        sig, _, new = pm.membership(v, p)
        sp[p], mr[p] = pm.bit_counts(v, p)
        for k, out in ((2, d2), (3, d3)):
            q = p if k == 3 else p + 1
            r2 = np.where(sig, 2 * ((mag >> q) << q) + (1 << q), np.where(new, 3 << p, 0))
            d = np.where(mag > 0, 2 * mag + 1 - r2, 0)
            out[p] = np.uint64(int((d.astype(object) ** 2).sum()))
    return d2, d3, sp, mr


def tables(idx, pr, k, nplanes=rc.NPLANES):
    """(dist, dist2, dist3, sp_bits, mr_bits) of a source block as the selection sees them: the statistics of
    relative(idx, pr), with DISABLED in dist[0] (k > 1) and dist3[0] (k = 2)"""
    v = relative(idx, pr)
    dist = rc.dist_row(v, nplanes)
    d2, d3, sp, mr = pass_rows(v, nplanes)
    if k > 1:
        dist[0] = np.uint64(DISABLED)
    if k == 2:
        d3[0] = np.uint64(DISABLED)
    return dist, d2, d3, sp, mr


def own_len(len_est, sp, mr, form):
    """the estimate of the own form from the estimates of the cleanup lengths (len_est[p'], the product's) and the two
    bit counts at p' = 0"""
    p, k = form
    if k == 1:
        return int(len_est[p])
    return int(len_est[1]) + (int(sp[0]) + 7) // 8 + ((int(mr[0]) + 7) // 8 if k == 3 else 0)


def own_dist(idx, pr, k):
    """the model's distortion of the own form"""
    v = relative(idx, pr)
    p, kk = own_form(v, k)
    return pm.dist(v, p, kk)


def alloc_tables(idx_blocks, blocks, forms, wts, nplanes=rc.NPLANES):
    """(lens, dists, cands) for rc.allocate() over the blocks of a frame (blocks: Encoder.layout's; idx_blocks[i]: the
    indices of block i) whose source forms are forms[i] = (pr, k) (pr < 0:
    the source left the block out): per block the allowed candidates' exact bytes, weighted distortions and what they
    are, (absolute plane of the last pass, passes); the last is (rc.SKIP, 1).  A block that is empty at its own form has
    that form alone"""
    lens, dists, cands = [], [], []
    for b, idx, (pr, k) in zip(blocks, idx_blocks, forms):
        if pr < 0:
            lens.append([0]); dists.append([0.0]); cands.append([(rc.SKIP, 1)])
            continue
        v = relative(idx, pr)
        wt = weight(wts[(b["comp"], rc.band_entry(b))], pr)
        p0, k0 = own_form(v, k)
        if not rc.shifted(v, p0 + (k0 > 1)).any():
            lens.append([0]); dists.append([0.0]); cands.append([(absolute(pr, p0), 1)])
            continue
        kmax = min(int(np.abs(v.astype(np.int64)).max()).bit_length(), nplanes)
        c, l, d = [], [], []
        for p in range(kmax):
            for kk in (1, 2, 3):
                if not allowed(v, k, p, kk) or (kk > 1 and p + 1 >= nplanes):
                    continue
                _, lcup, lref, _, _ = pm.code_block(v, p, kk)
                c.append((absolute(pr, p), kk)); l.append(lcup + lref); d.append(wt * float(pm.dist(v, p, kk)))
        c.append((rc.SKIP, 1)); l.append(0); d.append(wt * float(rc.dist_skip(v)))
        lens.append(l); dists.append(d); cands.append(c)
    return lens, dists, cands
