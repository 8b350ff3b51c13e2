/*
 * ht_decode_block.hpp -- the body of k_ht_decode / k_ht_decode_raw, included twice by ht_kernels.hpp.
 *
 * HT_DECODE_KERNEL names the kernel, HT_DECODE_RAW (0 / 1) says whether its stores are the decoder's dequantised samples
 * or the transcoder's quantiser indices (blocks that carry J2K_DWT_RAW: htj2k_xc_run_, htj2k_ht_blocks_raw).  The choice
 * is made at compile time and the text is compiled once per kernel, so that k_ht_decode keeps its name and, instruction
 * for instruction, the code it had before the raw stores existed.  No include guard, on purpose.
 */
template <bool EXTERNAL_VLC>
__global__ void __launch_bounds__(64)
HT_DECODE_KERNEL(const J2kBlock *__restrict__ blocks, int nblocks, const uint8_t *__restrict__ bytes,
                 uint32_t *__restrict__ coef, const uint16_t *__restrict__ g_tables,
                 int *__restrict__ status, HtLds L, const ht_sym_t *__restrict__ qsym, const uint32_t *__restrict__ qoff,
                 uint32_t *__restrict__ sink, const uint64_t *__restrict__ refbits, const uint32_t *__restrict__ roff,
                 int coef16 = 0)
{
    constexpr bool RAW = HT_DECODE_RAW != 0;
    extern __shared__ __align__(16) uint8_t smem[];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= nblocks) return;
    const J2kBlock b = blocks[blockIdx.x];
    const int w = b.w, h = b.h, stride = b.stride;
    const int qw = (w + 1) >> 1, qh = (h + 1) >> 1;
    const int transform = b.flags & 3;
    /* coef16 (host-checked: every block of the job is a reversible 5/3 cleanup-only block of at most 64 columns
     * with M_b <= 15 and no ROI shift): the planes are written as int16_t, same element offsets */
    uint16_t *dst16 = (uint16_t *)coef + b.plane_off;
    uint32_t *dst = coef16 ? (uint32_t *)dst16 : coef + b.plane_off;

    if (b.npasses == 0) {                              /* not coded: the reference plane is calloc'ed */
        if (coef16) ht_zero_window16(dst16, w, h, stride, lane); else ht_zero_window(dst, w, h, stride, lane);
        return;
    }
    /* pass bookkeeping, jpeg2000htdec.c:1240-1264 */
    const int rem = b.npasses % 3;
    const int num_plhd = rem ? b.npasses - rem : b.npasses - 3;
    const int p0 = num_plhd / 3;
    const int z_blk = b.npasses - num_plhd;
    const uint32_t Lcup = b.lcup, Lref = b.lref;
    const uint8_t *D = bytes + b.data_off;
    const int S_blk = (p0 + b.zbp) & 0xFF;
    const int pLSB = (30 - S_blk) & 0xFF;
    const int maxbp = S_blk + 1;                       /* (S_blk - 1) + 2, :605,:1263 */
    int err = 0;
    uint32_t Scup = 0, Pcup = 0;
    if (Lcup < 2) err = HT_ERR_INVALID;                /* :1252 */
    if (!err) {
        Scup = ((uint32_t)D[Lcup - 1] << 4) + (D[Lcup - 2] & 0x0F);
        if (Scup < 2 || Scup > Lcup || Scup > 4079) err = HT_ERR_INVALID;   /* :1268 */
        Pcup = Lcup - Scup;
    }
    if (!err && maxbp >= 32) err = HT_ERR_INVALID;     /* :617 */
    /* LDS capacity is sized by the host from the same fields; never index past it */
    if (!err && ((Pcup * 8 + 31) / 32 + 3 > L.ms_words || (uint32_t)qw > L.max_qw ||
                 (!EXTERNAL_VLC && ((Scup * 8 + 31) / 32 + 2 > L.vlc_words || Scup > L.suf_bytes))))
        err = HT_ERR_INVALID;
    if (err) {
        if (coef16) ht_zero_window16(dst16, w, h, stride, lane); else ht_zero_window(dst, w, h, stride, lane);
        if (lane == 0) status[blockIdx.x] = err;
        return;
    }

    uint16_t *tbl  = (uint16_t *)smem;
    uint32_t *ms   = (uint32_t *)(smem + L.off_ms);
    uint32_t *vlcw = (uint32_t *)(smem + L.off_vlc);
    uint8_t  *suf  = smem + L.off_suf;
    uint32_t *qinfo = (uint32_t *)(smem + L.off_qinfo);
    uint8_t  *Earr = smem + L.off_E;
    uint32_t *bm   = (uint32_t *)(smem + L.off_bm);
    const int Estride = 2 * (int)L.max_qw + 8;
    const uint32_t nms = (Pcup * 8 + 31) / 32 + 2, nvl = (Scup * 8 + 31) / 32 + 2;

    /* ---- stage 0: tables, zero, un-stuff ---- */
    if (!EXTERNAL_VLC) {
        for (int i = lane; i < 1024; i += 64)
            ((uint32_t *)tbl)[i] = ((const uint32_t *)g_tables)[i];
        for (uint32_t i = lane; i < nvl; i += 64) vlcw[i] = 0;
    }
    const bool fast = EXTERNAL_VLC && 2 * qw <= 64 && b.roi_shift == 0;   /* ht_magsgn_rows_narrow: no LDS exponent rows */
    for (uint32_t i = lane; i <= nms; i += 64) ms[i] = 0;
    if (!fast) {
        for (int i = lane; i < 2 * Estride; i += 64) Earr[i] = 0;
        for (uint32_t i = lane; i < 2 * L.max_qw; i += 64) qinfo[i] = 0;
    }
    if (z_blk > 1 && !fast)
        for (uint32_t i = lane; i < 4 * L.bm_words; i += 64) bm[i] = 0;
    __syncthreads();

    /* MagSgn: un-stuffed here in both modes, straight into LDS */
    const uint32_t ms_total = ht_unstuff_magsgn(D, Pcup, ms, lane);
    if (!EXTERNAL_VLC) {   /* VLC: backward from Dcup[Lcup-2]; Dcup[Lcup-1] counts as 0xFF and the low nibble of
         * Dcup[Lcup-2] as 0xF (:1277-1278); a byte with 7 LSBs set below a byte > 0x8F loses its MSB */
        uint32_t base = 0;
        const uint32_t nv = Scup - 1;                 /* bytes Lcup-2 .. Pcup */
        for (uint32_t k0 = 0; k0 < nv; k0 += 64) {
            const uint32_t k = k0 + lane;
            const bool act = k < nv;
            uint32_t v = 0, above = 0xFF;
            if (act) {
                const uint32_t j = Lcup - 2 - k;
                v = D[j];
                if (k == 0) v |= 0x0F;
                else { above = D[j + 1]; if (k == 1) above |= 0x0F; }
            }
            const uint32_t nb = act ? ((above > 0x8F && (v & 0x7F) == 0x7F) ? 7u : 8u) : 0u;
            v &= (1u << nb) - 1;
            const uint32_t incl = wave_incl_scan_u32(nb, lane);
            const uint32_t off = base + incl - nb;
            if (act) {
                atomicOr(&vlcw[off >> 5], v << (off & 31));
                if ((off & 31) > 24) atomicOr(&vlcw[(off >> 5) + 1], v >> (32 - (off & 31)));
            }
            base += wave_last(incl);
        }
    }
    for (uint32_t i = lane; !EXTERNAL_VLC && i < Scup; i += 64) {       /* MEL reads the (patched) suffix bytes */
        uint32_t v = D[Pcup + i];
        if (Pcup + i == Lcup - 1) v = 0xFF;
        else if (Pcup + i == Lcup - 2) v |= 0x0F;
        suf[i] = (uint8_t)v;
    }
    __syncthreads();
    for (uint32_t i = lane; i <= nms; i += 64) {                        /* past the end the MagSgn stream is all ones */
        if (i * 32 >= ms_total) ms[i] = 0xFFFFFFFFu;
        else if (i * 32 + 32 > ms_total) ms[i] |= 0xFFFFFFFFu << (ms_total & 31);
    }
    __syncthreads();

    HtSerial S;
    S.vbuf = 0; S.vbits = 0; S.vword = 0; S.vlc = vlcw; S.vlc_words = nvl;
    S.suf = suf; S.mel_pos = 0; S.mel_len = Scup; S.mel_tmp = 0; S.mel_bits = 0;
    S.mel_k = 0; S.mel_run = 0; S.mel_one = 0;
    if (!EXTERNAL_VLC && lane == 0) S.vdrop(0), S.vfill(), S.vdrop(4);   /* jpeg2000_init_vlc drops the Scup nibble, :283-295 */
    const ht_sym_t *qglob = EXTERNAL_VLC ? qsym + qoff[blockIdx.x] : nullptr;

    float fscale = b.f_step;
    fscale /= (float)(1 << (31 - b.M_b));              /* jpeg2000dec.c:2104-2106 */
    const int i_step = b.i_step, M_b = b.M_b, roi_shift = b.roi_shift;

    uint32_t ms_pos = 0;                               /* bit position in the un-stuffed MagSgn stream */
    int ctx_run = 0;                                   /* first-row context carried along the row */
    const int bmW = w + 2;                             /* bitmap row pitch (1-cell border) */

    const uint64_t *rbits = (fast && z_blk > 1 && refbits) ? refbits + roff[blockIdx.x] : nullptr;
    if (fast && RAW) {
        if (z_blk > 1) err = ht_magsgn_rows_narrow<J2K_DWT_RAW, true>(qglob, ms, dst, lane, w, h, stride, pLSB, maxbp, M_b, fscale, i_step, nms - 2, sink, rbits, z_blk);
        else err = ht_magsgn_rows_narrow<J2K_DWT_RAW, false>(qglob, ms, dst, lane, w, h, stride, pLSB, maxbp, M_b, fscale, i_step, nms - 2, sink, rbits, z_blk);
    } else if (fast) {
        if (z_blk > 1) {
            if (transform == J2K_DWT53) err = ht_magsgn_rows_narrow<J2K_DWT53, true>(qglob, ms, dst, lane, w, h, stride, pLSB, maxbp, M_b, fscale, i_step, nms - 2, sink, rbits, z_blk);
            else if (transform == J2K_DWT97) err = ht_magsgn_rows_narrow<J2K_DWT97, true>(qglob, ms, dst, lane, w, h, stride, pLSB, maxbp, M_b, fscale, i_step, nms - 2, sink, rbits, z_blk);
            else err = ht_magsgn_rows_narrow<J2K_DWT97_INT, true>(qglob, ms, dst, lane, w, h, stride, pLSB, maxbp, M_b, fscale, i_step, nms - 2, sink, rbits, z_blk);
        } else if (EXTERNAL_VLC && coef16) {
            err = ht_magsgn_rows_narrow<J2K_DWT53, false, true>(qglob, ms, dst, lane, w, h, stride, pLSB, maxbp, M_b, fscale, i_step, nms - 2, sink, rbits, z_blk);
        } else {
            if (transform == J2K_DWT53) err = ht_magsgn_rows_narrow<J2K_DWT53, false>(qglob, ms, dst, lane, w, h, stride, pLSB, maxbp, M_b, fscale, i_step, nms - 2, sink, rbits, z_blk);
            else if (transform == J2K_DWT97) err = ht_magsgn_rows_narrow<J2K_DWT97, false>(qglob, ms, dst, lane, w, h, stride, pLSB, maxbp, M_b, fscale, i_step, nms - 2, sink, rbits, z_blk);
            else err = ht_magsgn_rows_narrow<J2K_DWT97_INT, false>(qglob, ms, dst, lane, w, h, stride, pLSB, maxbp, M_b, fscale, i_step, nms - 2, sink, rbits, z_blk);
        }
    }
    for (int row = 0; row < qh && !err && !fast; row++) {
        uint32_t *qcur = qinfo + (row & 1) * L.max_qw, *qprev = qinfo + ((row & 1) ^ 1) * L.max_qw;
        uint8_t *Ecur = Earr + (row & 1) * Estride + 4, *Eprev = Earr + ((row & 1) ^ 1) * Estride + 4;

        /* ---- stage 1: serial quad-row decode on lane 0 ---- */
        if (EXTERNAL_VLC) {
            /* symbols are read straight from global in stage 2 */
        } else if (lane == 0) {
            const uint16_t *table = tbl + (row ? 1024 : 0);
            int rho_left = 0;
            for (int qx = 0; qx < qw; qx += 2) {
                const int npair = (qx + 1 < qw) ? 2 : 1;
                int rho[2] = { 0, 0 }, uoff[2] = { 0, 0 }, ek[2] = { 0, 0 }, e1[2] = { 0, 0 }, u[2] = { 0, 0 };
                for (int k = 0; k < npair; k++) {
                    const int q = qx + k;
                    int ctx;
                    if (row == 0) {
                        ctx = ctx_run;
                    } else {
                        const int ra  = qprev[q] & 0xF;
                        const int ral = q > 0 ? (qprev[q - 1] & 0xF) : 0;
                        const int rar = q + 1 < qw ? (qprev[q + 1] & 0xF) : 0;
                        const int rl  = q > 0 ? rho_left : 0;
                        ctx = (((ra >> 1) | (ral >> 3)) & 1) | ((((rl >> 2) | (rl >> 3)) & 1) << 1) |
                              ((((ra >> 3) | (rar >> 1)) & 1) << 2);
                    }
                    if (ctx != 0 || S.mel_sym() != 0) {
                        const uint32_t e = table[(ctx << 7) | S.vpeek(7)];
                        S.vdrop((e >> 1) & 7);
                        uoff[k] = e & 1; rho[k] = (e >> 4) & 0xF; ek[k] = (e >> 8) & 0xF; e1[k] = (e >> 12) & 0xF;
                    }
                    rho_left = rho[k];
                    if (row == 0)
                        ctx_run = ((rho[k] | (rho[k] >> 1)) & 1) | (((rho[k] >> 2) & 1) << 1) | (((rho[k] >> 3) & 1) << 2);
                }
                if (npair == 2 && uoff[0] && uoff[1]) {
                    if (row == 0) {
                        if (S.mel_sym()) {
                            const int p1 = S.upfx(), p2 = S.upfx();
                            const int s1 = S.usfx(p1), s2 = S.usfx(p2);
                            const int x1 = S.uext(s1), x2 = S.uext(s2);
                            u[0] = 2 + p1 + s1 + 4 * x1;
                            u[1] = 2 + p2 + s2 + 4 * x2;
                        } else {
                            const int p1 = S.upfx();
                            if (p1 > 2) {
                                u[1] = (int)S.vget(1) + 1;
                                const int s1 = S.usfx(p1), x1 = S.uext(s1);
                                u[0] = p1 + s1 + 4 * x1;
                            } else {
                                const int p2 = S.upfx();
                                const int s1 = S.usfx(p1), s2 = S.usfx(p2);
                                const int x1 = S.uext(s1), x2 = S.uext(s2);
                                u[0] = p1 + s1 + 4 * x1;
                                u[1] = p2 + s2 + 4 * x2;
                            }
                        }
                    } else {
                        const int p1 = S.upfx(), p2 = S.upfx();
                        const int s1 = S.usfx(p1), s2 = S.usfx(p2);
                        const int x1 = S.uext(s1), x2 = S.uext(s2);
                        u[0] = p1 + s1 + 4 * x1;
                        u[1] = p2 + s2 + 4 * x2;
                    }
                } else {
                    for (int k = 0; k < npair; k++)
                        if (uoff[k]) {
                            const int p = S.upfx(), s = S.usfx(p), x = S.uext(s);
                            u[k] = p + s + 4 * x;
                        }
                }
                for (int k = 0; k < npair; k++)
                    qcur[qx + k] = (uint32_t)rho[k] | ((uint32_t)ek[k] << 4) | ((uint32_t)e1[k] << 8) | ((uint32_t)u[k] << 16);
            }
        }
        if (!EXTERNAL_VLC) __syncthreads();

        /* ---- stage 2: MagSgn of the quad row, lanes = sample columns ---- */
        const int ncols = 2 * qw;
        int row_err = 0;
        for (int c0 = 0; c0 < ncols; c0 += 64) {
            const int col = c0 + lane;
            const bool act = col < ncols;
            const int q = col >> 1;
            const uint32_t qi = act ? (EXTERNAL_VLC ? ht_sym_unpack(qglob[row * (int)ht_qsym_pitch((uint32_t)w) + q]) : qcur[q]) : 0;
            const int rho = qi & 0xF, ekq = (qi >> 4) & 0xF, e1q = (qi >> 8) & 0xF, uq = (qi >> 16) & 0xFF;
            int kappa = 1;
            if (row > 0 && act) {                      /* :855-885; Eprev[-1] and Eprev[ncols] are 0 */
                const int x2 = 2 * q;
                int me = max(max((int)Eprev[x2 - 1], (int)Eprev[x2]), max((int)Eprev[x2 + 1], (int)Eprev[x2 + 2]));
                const int gamma = (rho & (rho - 1)) != 0;           /* more than one significant sample */
                kappa = max(1, gamma * (me - 1));
            }
            const int U = kappa + uq;
            if (act && U > maxbp) row_err = 1;         /* :715,756,889,961 */
            const int sh = (col & 1) * 2;              /* samples 0,1 (left column) or 2,3 (right column) */
            const int s_t = (rho >> sh) & 1, s_b = (rho >> (sh + 1)) & 1;
            int m_t = act ? s_t * U - ((ekq >> sh) & 1) : 0;
            int m_b = act ? s_b * U - ((ekq >> (sh + 1)) & 1) : 0;
            /* a negative m (e_k outside rho: not in the Annex C tables) reads no bits */
            const uint32_t nb = (uint32_t)(max(m_t, 0) + max(m_b, 0));
            const uint32_t incl = wave_incl_scan_u32(nb, lane);
            uint32_t pos = ms_pos + incl - nb;
            uint32_t smag[2] = { 0, 0 };
            int Ebot = 0;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const int m = r ? m_b : m_t;
                const int e1b = (e1q >> (sh + r)) & 1;
                if (m != 0) {
                    uint32_t v = 0;
                    if (m > 0) {
                        const uint32_t wi = min(pos >> 5, nms - 1), wj = min((pos >> 5) + 1, nms - 1);
                        const uint64_t two = ((uint64_t)ms[wj] << 32) | ms[wi];
                        v = (uint32_t)(two >> (pos & 31)) & (uint32_t)((1ull << m) - 1);
                        v += (uint32_t)e1b << m;
                        pos += m;
                    }
                    const int E = 32 - __clz((int)(v | 1));
                    uint32_t mu = (v >> 1) + 1;
                    mu <<= pLSB;
                    mu |= 1u << ((pLSB - 1) & 31);
                    mu |= (v & 1) << 31;
                    smag[r] = mu;
                    if (r) Ebot = E;
                }
            }
            if (act) Ecur[col] = (uint8_t)Ebot;
            ms_pos += wave_last(incl);

            /* raster positions of this lane's two samples; odd sizes: the outside half of the
             * border quads is discarded (:976-1007) */
            const int y0 = 2 * row;
            if (act && col < w) {
#pragma unroll
                for (int r = 0; r < 2; r++) {
                    const int y = y0 + r;
                    if (y >= h) continue;
                    if (z_blk > 1) {
                        dst[(size_t)y * stride + col] = smag[r];          /* raw, finished in stage 3 */
                        if (((rho >> (sh + r)) & 1))
                            atomicOr(&bm[((y + 1) * bmW + col + 1) >> 5], 1u << (((y + 1) * bmW + col + 1) & 31));
                    } else {
                        dst[(size_t)y * stride + col] = RAW ? ht_raw_index(smag[r] & ht_raw_mask(true, pLSB, 1), M_b)
                                                            : ht_dequant(smag[r], transform, M_b, roi_shift, fscale, i_step);
                    }
                }
            }
        }
        if (__any(row_err)) err = HT_ERR_INVALID;
        if (EXTERNAL_VLC) wave_lds_fence(); else __syncthreads();
    }

    if (err) {
        __syncthreads();
        if (coef16) ht_zero_window16(dst16, w, h, stride, lane); else ht_zero_window(dst, w, h, stride, lane);
        if (lane == 0) status[blockIdx.x] = err;
        return;
    }
    if (z_blk <= 1 || fast) return;                    /* the fast path applied k_ht_refine's decisions in its row loop */

    /* ---- stage 3: refinement passes on bitmaps (bit index = (y+1)*(w+2) + x+1) ---- */
    uint32_t *bm_sig = bm, *bm_ref = bm + L.bm_words, *bm_sgn = bm + 2 * L.bm_words, *bm_mr = bm + 3 * L.bm_words;
    const uint8_t *Dref = D + Lcup;
    const int causal = b.flags & J2K_CBLK_VSC;
    __syncthreads();
    if (lane == 0) {
        /* SigProp, jpeg2000htdec.c:1016-1131: forward LSB-first reader, 7 bits after 0xFF, zeros past Lref */
        uint32_t pos = 0, tmp = 0, last = 0; int bits = 0;
        auto rdbit = [&]() -> int {
            if (bits == 0) {
                bits = (last == 0xFF) ? 7 : 8;
                if (pos < Lref) { tmp = Dref[pos]; pos++; } else tmp = 0;
                last = tmp;
            }
            int bit = tmp & 1; tmp >>= 1; bits--;
            return bit;
        };
        for (int i0 = 0; i0 < h; i0 += 4) {
            const int gh = min(4, h - i0);
            for (int j0 = 0; j0 < w; j0 += 4) {
                const int gw = min(4, w - j0);
                for (int j = j0; j < j0 + gw; j++)
                    for (int i = i0; i < i0 + gh; i++) {
                        const int c = (i + 1) * bmW + (j + 1);
                        if (bm_get(bm_sig, c)) continue;
                        const int below_ok = !causal || (i != i0 + gh - 1);
                        int mbr = bm_get(bm_sig, c - bmW - 1) | bm_get(bm_sig, c - bmW) | bm_get(bm_sig, c - bmW + 1) |
                                  bm_get(bm_sig, c - 1) | bm_get(bm_sig, c + 1) |
                                  bm_get(bm_ref, c - bmW - 1) | bm_get(bm_ref, c - bmW) | bm_get(bm_ref, c - bmW + 1) |
                                  bm_get(bm_ref, c - 1) | bm_get(bm_ref, c + 1);
                        if (below_ok)
                            mbr |= bm_get(bm_sig, c + bmW - 1) | bm_get(bm_sig, c + bmW) | bm_get(bm_sig, c + bmW + 1) |
                                   bm_get(bm_ref, c + bmW - 1) | bm_get(bm_ref, c + bmW) | bm_get(bm_ref, c + bmW + 1);
                        if (mbr && rdbit())
                            bm_ref[c >> 5] |= 1u << (c & 31);
                    }
                for (int j = j0; j < j0 + gw; j++)
                    for (int i = i0; i < i0 + gh; i++) {
                        const int c = (i + 1) * bmW + (j + 1);
                        if (bm_get(bm_ref, c) && rdbit())
                            bm_sgn[c >> 5] |= 1u << (c & 31);
                    }
            }
        }
        if (z_blk > 2) {
            /* MagRef, :1137-1185: backward reader over Dref with the VLC un-stuffing rule; the byte
             * after the segment counts as 0xFF (:1260), bytes below Dref[0] read as zero bits */
            int rpos = (int)Lref - 1; uint32_t above = 0xFF, cur = 0; int nb = 0;
            auto rdback = [&]() -> int {
                if (nb == 0) {
                    if (rpos >= 0) {
                        cur = Dref[rpos];
                        nb = (above > 0x8F && (cur & 0x7F) == 0x7F) ? 7 : 8;
                        above = cur;
                        rpos--;
                    } else { cur = 0; nb = 8; }
                }
                int bit = cur & 1; cur >>= 1; nb--;
                return bit;
            };
            for (int i0 = 0; i0 < h; i0 += 4)
                for (int j = 0; j < w; j++)
                    for (int i = i0; i < min(i0 + 4, h); i++) {
                        const int c = (i + 1) * bmW + (j + 1);
                        if (bm_get(bm_sig, c) && rdback())
                            bm_mr[c >> 5] |= 1u << (c & 31);
                    }
        }
    }
    __syncthreads();
    {
        const int qq = (pLSB - 1) & 31;                /* both passes are called with pLSB - 1, :1309-1315 */
        for (int y = 0; y < h; y++)
            for (int x = lane; x < w; x += 64) {
                const int c = (y + 1) * bmW + (x + 1);
                uint32_t v = dst[(size_t)y * stride + x];
                if (bm_get(bm_ref, c)) {
                    v |= 1u << qq;
                    v |= 1u << ((qq - 1) & 31);
                    v |= (uint32_t)bm_get(bm_sgn, c) << 31;
                }
                if (z_blk > 2 && bm_get(bm_sig, c)) {
                    v &= (0xFFFFFFFEu | (uint32_t)bm_get(bm_mr, c)) << qq;
                    v |= 1u << ((qq - 1) & 31);
                }
                if (RAW) v &= ht_raw_mask(bm_get(bm_sig, c) != 0, pLSB, z_blk);
                dst[(size_t)y * stride + x] = RAW ? ht_raw_index(v, M_b) : ht_dequant(v, transform, M_b, roi_shift, fscale, i_step);
            }
    }
}
