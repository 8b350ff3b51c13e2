/*
 * j2k_enc.c -- host side of the HTJ2K encoder: scope checks, code-block layout, the band
 * exponents (and, for 9/7, the quantiser's steps), the main header and packet writer, the
 * guard-bit choice, the choice of rate control's last resort (enc_drop_take), and the context-free
 * entry points htj2k_encode_bound / htj2k_enc_layout / htj2k_enc_assemble.
 *
 * What j2kenc.c does in put_siz / put_cap / put_cod / put_qcd / encode_packet / tag_tree_code
 * (SURVEY.md section 2), for the one stream shape this encoder writes: a regular tile grid from
 * origin 0 (by default one tile equal to the image), one tile-part per tile, one layer, LRCP,
 * maximal precincts, HT code-blocks of one cleanup pass each, or of up to three passes (SigProp,
 * MagRef: one refinement segment behind the cleanup segment, two length fields in the packet header).
 *
 * Geometry.  The band, precinct and code-block rectangles are not derived here: the frame's
 * main header is written first, with an empty tile-part for every tile, and read back by the
 * decoder's own header parser and geometry code (j2k_syntax.c, j2k_tier2.c), so the layout the
 * encoder codes, in every tile, is by construction the one the product decoder expects.
 */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include "j2k_host.h"
#include "j2k_enc.h"
#include "ht_cxtvlc_rows.h"

static void elog(enc_log_fn log, void *opaque, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
static void elog(enc_log_fn log, void *opaque, const char *fmt, ...)
{
    char msg[256];
    va_list ap;
    if (!log)
        return;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    log(opaque, LOGL_ERROR, msg);
}

/* ------------------------------------------------------------------ CxtVLC encode table
 * Built from the T.814 Annex C rows the decoder uses: a row (ctx, rho, u_off, e_k, e_1) codes
 * "pattern rho, exponent bound exceeded by the samples eps" when e_1 == eps & e_k.  Of those
 * the one that saves the most MagSgn bits (most e_k bits) wins, then the shortest codeword. */
static void tab_consider(uint16_t *tab, int t, int ctx, int rho, int uoff, int ek, int e1, int cwd, int len)
{
    int eps;
    for (eps = 0; eps < 16; eps++) {
        uint16_t *e = &tab[((t * 8 + ctx) * 16 + rho) * 16 + eps];
        const int have = *e >> 15, hek = (*e >> 11) & 15, hlen = (*e >> 8) & 7, k = uoff ? ek : 0;
        if (uoff ? (!eps || (eps & ~rho) || (eps & ek) != e1) : eps != 0)
            continue;
        if (!have || __builtin_popcount(k) > __builtin_popcount(hek) ||
            (__builtin_popcount(k) == __builtin_popcount(hek) && len < hlen))
            *e = (uint16_t)(1u << 15 | (uint32_t)k << 11 | (uint32_t)len << 8 | (uint32_t)cwd);
    }
}

void enc_cxtvlc_table(uint16_t tab[2 * 8 * 16 * 16])
{
    memset(tab, 0, 2 * 8 * 16 * 16 * sizeof(uint16_t));
#define ROW0(c, r, u, k, o, w, l) tab_consider(tab, 0, c, r, u, k, o, w, l);
#define ROW1(c, r, u, k, o, w, l) tab_consider(tab, 1, c, r, u, k, o, w, l);
    HT_CXTVLC_ROWS0(ROW0)
    HT_CXTVLC_ROWS1(ROW1)
#undef ROW0
#undef ROW1
}

/* ------------------------------------------------------------------ options and scope */
void htj2k_enc_opts_default(htj2k_enc_opts *o)
{
    o->levels = 5;
    o->cb_w_log2 = 6;
    o->cb_h_log2 = 6;
    o->mct = -1;
    o->guard_bits = 0;
    o->irreversible = 0;
    o->qstep = 1.0;
    o->target_bytes = 0;
    o->tile_w = 0;
    o->tile_h = 0;
    o->ht_passes = 0;
    o->target_psnr = 0;
    o->group_bytes = 0;
}

void enc_opts_resolve(const htj2k_enc_opts *in, htj2k_enc_opts *out)
{
    if (in)
        *out = *in;
    else
        htj2k_enc_opts_default(out);
}

static int is_rgb_family(int fmt)
{
    return fmt == HTJ2K_PIX_RGB24 || fmt == HTJ2K_PIX_RGBA || fmt == HTJ2K_PIX_RGB48 || fmt == HTJ2K_PIX_RGBA64;
}

/* ------------------------------------------------------------------ byte writer */
typedef struct Wr { uint8_t *p; size_t n, cap; int oom; } Wr;
static void wr_put(Wr *w, const void *src, size_t n)
{
    if (w->n + n > w->cap) {
        size_t nc = w->cap ? w->cap * 2 : 1024;
        uint8_t *np;
        while (nc < w->n + n)
            nc *= 2;
        np = (uint8_t *)realloc(w->p, nc);
        if (!np) {
            w->oom = 1;
            return;
        }
        w->p = np;
        w->cap = nc;
    }
    memcpy(w->p + w->n, src, n);
    w->n += n;
}
static void wr_u8(Wr *w, unsigned v)  { uint8_t c = (uint8_t)v; wr_put(w, &c, 1); }
static void wr_u16(Wr *w, unsigned v) { uint8_t c[2] = { (uint8_t)(v >> 8), (uint8_t)v }; wr_put(w, c, 2); }
static void wr_u32(Wr *w, uint32_t v) { wr_u16(w, v >> 16); wr_u16(w, v & 0xFFFF); }

/* the main header, SOC .. QCC (put_siz, put_cap, put_cod, put_qcd) */
static void write_main_header(const EncFrame *f, int guard, Wr *w)
{
    const int nb = 3 * f->nl + 1;
    int c, g, maxMb = 1, pm;
    wr_u16(w, 0xFF4F);                                         /* SOC */
    wr_u16(w, 0xFF51); wr_u16(w, 38 + 3 * f->ncomp);           /* SIZ */
    wr_u16(w, 0x4000);                                         /* Rsiz: HTJ2K (T.814 A.2) */
    wr_u32(w, (uint32_t)f->w); wr_u32(w, (uint32_t)f->h);
    wr_u32(w, 0); wr_u32(w, 0);
    wr_u32(w, (uint32_t)f->tw); wr_u32(w, (uint32_t)f->th);    /* XTsiz, YTsiz; the tile grid starts at 0 */
    wr_u32(w, 0); wr_u32(w, 0);
    wr_u16(w, (unsigned)f->ncomp);
    for (c = 0; c < f->ncomp; c++) {
        wr_u8(w, (unsigned)(f->bits - 1));
        wr_u8(w, (unsigned)f->dx[c]);
        wr_u8(w, (unsigned)f->dy[c]);
    }
    for (c = 0; c < f->ncomp; c++)
        for (g = 0; g < nb; g++)
            maxMb = max32(maxMb, f->expn[c][g] + guard - 1);
    pm = maxMb <= 8 ? 0 : (maxMb < 28 ? maxMb - 8 : 13 + (maxMb >> 2));
    wr_u16(w, 0xFF50); wr_u16(w, 8); wr_u32(w, 0x00020000);    /* CAP: Part 15 */
    wr_u16(w, (unsigned)((f->irrev ? 0x20 : 0) | (min32(pm, 31) & 0x1F)));   /* Ccap15: HTONLY, HTIRV, MAGB */
    wr_u16(w, 0xFF52); wr_u16(w, 12);                          /* COD */
    wr_u8(w, 0);                                               /* maximal precincts, no SOP / EPH */
    wr_u8(w, 0);                                               /* LRCP */
    wr_u16(w, 1);                                              /* one layer */
    wr_u8(w, (unsigned)f->mct);
    wr_u8(w, (unsigned)f->nl);
    wr_u8(w, (unsigned)(f->cbw - 2)); wr_u8(w, (unsigned)(f->cbh - 2));
    wr_u8(w, 0x40);                                            /* HT code-blocks only */
    wr_u8(w, f->irrev ? 0 : 1);                                /* 9/7 or 5/3 */
    for (c = 0; c < f->ncomp; c++) {
        const int per = f->irrev ? 2 : 1;                      /* bytes per band */
        if (c > 0) {
            int same = 1;
            for (g = 0; g < nb; g++)
                same &= f->expn[c][g] == f->expn[0][g] && f->mant[c][g] == f->mant[0][g];
            if (same)
                continue;
            wr_u16(w, 0xFF5D); wr_u16(w, (unsigned)(4 + per * nb)); wr_u8(w, (unsigned)c);     /* QCC */
        } else {
            wr_u16(w, 0xFF5C); wr_u16(w, (unsigned)(3 + per * nb));                             /* QCD */
        }
        wr_u8(w, (unsigned)(guard << 5 | (f->irrev ? 2 : 0)));  /* no quantisation, or scalar expounded */
        for (g = 0; g < nb; g++) {
            if (f->irrev)
                wr_u16(w, (unsigned)(f->expn[c][g] << 11 | f->mant[c][g]));
            else
                wr_u8(w, (unsigned)(f->expn[c][g] << 3));
        }
    }
}

/* the 9/7 step of band g (0 LL, then HL LH HH from the lowest resolution up) as exponent and mantissa, for samples of
 * `bits`: d = qstep * 2^-((l - 1) / 2) at level l (LL: l = NL), e = floor(log2 d), mantissa the 11-bit fraction of
 * d / 2^e, rounded (a carry into e on 2048), exponent bits - e (the rule of the vector factory's band_quant).
 * 0, or HTJ2K_ERR_EINVAL when the exponent leaves 0 .. 31. */
static int step_rule(double qstep, int bits, int nl, int g, int *expn, int *mant)
{
    const int r = g ? (g - 1) / 3 + 1 : 0, lvl = r ? nl - r + 1 : nl;
    const double d = qstep * pow(2.0, -0.5 * (lvl - 1));
    int e, m;
    if (!(d > 0) || !isfinite(d))
        return HTJ2K_ERR_EINVAL;
    e = (int)floor(log2(d));
    m = (int)floor((d / pow(2.0, e) - 1.0) * 2048.0 + 0.5);
    if (m >= 2048) {
        m = 0;
        e++;
    }
    if (bits - e < 0 || bits - e > 31)
        return HTJ2K_ERR_EINVAL;
    *expn = bits - e;
    *mant = m;
    return 0;
}

/* ------------------------------------------------------------------ rate-control weights
 * What one unit of a band's quantisation index is worth in the output pixels, squared: the decoder's step of the band,
 * times the L2 norm of the band's 2-D synthesis response under the inverse lifting exactly as the decoder runs it
 * (un-normalised 9/7: the K factors are in the step; 5/3 taken as its linear part), times the column norm of the
 * inverse ICT / RCT.  The 1-D norms are measured: a unit impulse in the middle of the low (high) half of a line goes
 * through `l` inverse levels in plain C, for l = 1 .. RC_LV; deeper levels continue geometrically (by then the
 * response no longer changes shape).  Doubles, evaluated in a fixed order: part of the determinism contract. */
#define RC_LV 8
static void rc_inv_level(double *x, int n, int irrev)
{
    static const double c97[4] = { -0.443506852043971, -0.882911075530934, 0.052980118572961, 1.586134342059924 };
    static const double c53[2] = { -0.25, 0.5 };
    const double *c = irrev ? c97 : c53;
    const int ns = irrev ? 4 : 2;
    int s, j;
    for (s = 0; s < ns; s++)
        for (j = s & 1; j < n; j += 2) {              /* even positions (low-pass) first, then odd, alternating */
            const int l = j ? j - 1 : 1, r = j + 1 < n ? j + 1 : n - 2;
            x[j] += c[s] * (x[l] + x[r]);
        }
}
/* gl[l], gh[l], l = 1 .. RC_LV: norm at full resolution of a unit low-pass (high-pass) sample of level l */
static int rc_gains(int irrev, double *gl, double *gh)
{
    const int n0 = 64;
    double *a = (double *)calloc((size_t)n0 << RC_LV, sizeof(double)), *b = (double *)calloc((size_t)n0 << RC_LV, sizeof(double));
    int l, hp, k, i;
    if (!a || !b) {
        free(a); free(b);
        return HTJ2K_ERR_ENOMEM;
    }
    for (l = 1; l <= RC_LV; l++) {
        for (hp = 0; hp < 2; hp++) {
            int n = n0;
            double e = 0;
            memset(a, 0, ((size_t)n0 << RC_LV) * sizeof(double));
            a[n0 / 2 + hp] = 1.0;                     /* interleaved: even = low-pass, odd = high-pass */
            for (k = 0; k < l; k++) {
                rc_inv_level(a, n, irrev);
                if (k + 1 < l) {                      /* the line is the low-pass half of the next finer level */
                    memset(b, 0, (size_t)2 * n * sizeof(double));
                    for (i = 0; i < n; i++)
                        b[2 * i] = a[i];
                    memcpy(a, b, (size_t)2 * n * sizeof(double));
                    n *= 2;
                }
            }
            for (i = 0; i < n; i++)
                e += a[i] * a[i];
            (hp ? gh : gl)[l] = sqrt(e);
        }
    }
    free(a); free(b);
    return 0;
}
static double rc_gl[2][RC_LV + 1], rc_gh[2][RC_LV + 1];     /* measured once per transform */
static int rc_gains_err;
static pthread_once_t rc_once = PTHREAD_ONCE_INIT;
static void rc_gains_init(void)
{
    if ((rc_gains_err = rc_gains(0, rc_gl[0], rc_gh[0])) == 0)
        rc_gains_err = rc_gains(1, rc_gl[1], rc_gh[1]);
}
/* only frames with a budget or a PSNR target have weights (htj2k_enc_band_weights asks for them itself; the other
 * context-free calls and plain encodes never read them) */
static int rc_weights(EncFrame *f)
{
    static const double ict[3] = { 3.0, 0.344136 * 0.344136 + 1.772 * 1.772, 1.402 * 1.402 + 0.714136 * 0.714136 };
    static const double rct[3] = { 3.0, 0.6875, 0.6875 };
    const double *gl = rc_gl[f->irrev != 0], *gh = rc_gh[f->irrev != 0];
    int c, g;
    pthread_once(&rc_once, rc_gains_init);
    if (rc_gains_err)
        return rc_gains_err;
    for (c = 0; c < f->ncomp; c++)
        for (g = 0; g < 3 * f->nl + 1; g++) {
            const int r = g ? (g - 1) / 3 + 1 : 0, lvl = r ? f->nl - r + 1 : f->nl, kind = g ? 1 + (g - 1) % 3 : 0;
            double lo = 1.0, hi = 1.0, w;
            if (lvl >= 1) {
                const int k = lvl < RC_LV ? lvl : RC_LV;
                lo = gl[k] * pow(gl[RC_LV] / gl[RC_LV - 1], lvl - k);
                hi = gh[k] * pow(gh[RC_LV] / gh[RC_LV - 1], lvl - k);
            }
            w = (kind == 0 ? lo * lo : kind == 3 ? hi * hi : lo * hi) * (double)f->fstep[c][g];
            w *= w;
            if (f->mct && c < 3)
                w *= f->irrev ? ict[c] : rct[c];
            f->wgt[c][g] = w;
        }
    return 0;
}

int enc_rc_weights(EncFrame *f) { return rc_weights(f); }

/* ------------------------------------------------------------------ frame layout */
static void parser_log(void *opaque, int level, const char *msg)
{
    (void)opaque; (void)level; (void)msg;
}

/* tile t of the frame: its rectangles, packets and blocks appended to f->pkt, f->pb and f->blk at *ki, *pi and *bi */
static void tile_blocks(EncFrame *f, const GeomCache *g, int t, int *bi, int *pi, int *ki)
{
    EncTile *et = &f->tile[t];
    int c, r, b;
    et->t.blk0 = *bi;
    et->pkt0 = *ki;
    for (c = 0; c < f->ncomp; c++) {
        const TcGeom *tc = &g->tc[t * f->ncomp + c];
        et->t.x0[c] = tc->ox0; et->t.x1[c] = tc->ox1;
        et->t.y0[c] = tc->oy0; et->t.y1[c] = tc->oy1;
    }
    for (r = 0; r <= f->nl; r++)
        for (c = 0; c < f->ncomp; c++) {
            const TcGeom *tc = &g->tc[t * f->ncomp + c];
            const ResGeom *rg = &tc->res[r];
            EncPacket *pk;
            if (rg->npx * rg->npy == 0)
                continue;
            pk = &f->pkt[(*ki)++];
            pk->pb0 = *pi;
            for (b = 0; b < rg->nbands; b++) {
                const BandGeom *bg = &rg->band[b];
                const PrecBand *pb = &g->pb[rg->pb0 + (uint32_t)b];
                const int orient = b + (r > 0);
                /* where the band sits in the tile-component's Mallat layout (as layout_rows places it for the decoder) */
                const int32_t sx = (orient & 1) ? tc->res[r - 1].x1 - tc->res[r - 1].x0 : 0;
                const int32_t sy = (orient & 2) ? tc->res[r - 1].y1 - tc->res[r - 1].y0 : 0;
                const int32_t ax = (bg->x0 >> bg->cbw) << bg->cbw, ay = (bg->y0 >> bg->cbh) << bg->cbh;
                int i, j;
                if (bg->x0 == bg->x1 || bg->y0 == bg->y1)
                    continue;
                f->pb[*pi].blk0 = *bi;
                f->pb[*pi].ncw = pb->ncw;
                f->pb[*pi].nch = pb->nch;
                (*pi)++;
                pk->npb++;
                for (j = 0; j < pb->nch; j++)
                    for (i = 0; i < pb->ncw; i++) {
                        EncBlock *e = &f->blk[(*bi)++];
                        const int32_t cx0 = ax + (i << bg->cbw), cy0 = ay + (j << bg->cbh);
                        const int32_t x0 = max32(cx0, bg->x0), x1 = min32(cx0 + (1 << bg->cbw), bg->x1);
                        const int32_t y0 = max32(cy0, bg->y0), y1 = min32(cy0 + (1 << bg->cbh), bg->y1);
                        e->comp = c; e->res = r; e->band = orient;
                        e->x = tc->ox0 + x0 + sx - bg->x0; e->y = tc->oy0 + y0 + sy - bg->y0;
                        e->w = x1 - x0; e->h = y1 - y0;
                        e->expn = f->expn[c][r ? 3 * (r - 1) + b + 1 : 0];
                    }
            }
        }
    et->t.nblk = *bi - et->t.blk0;
    et->npkt = *ki - et->pkt0;
}

/* the tile grid of a w x h frame (f->tw, th, ntx, nty, ntiles) and what it must satisfy: at most 65535 tiles (Isot), no
 * tile-component without samples (the decoder refuses those) and none beyond 32768 samples in a direction.  A direction
 * is checked tile column by tile column (row by row): a tile-component's extent there depends on nothing else. */
static int tile_grid(EncFrame *f, int w, int h, const J2kPixDesc *pd, const htj2k_enc_opts *o, enc_log_fn log, void *opaque)
{
    int dir, c, far = 0;
    if (o->tile_w < 0 || o->tile_h < 0) {
        elog(log, opaque, "encoder: a tile size of %dx%d is negative\n", o->tile_w, o->tile_h);
        return HTJ2K_ERR_EINVAL;
    }
    f->tw = o->tile_w ? o->tile_w : w;
    f->th = o->tile_h ? o->tile_h : h;
    f->ntx = (int)(((int64_t)w + f->tw - 1) / f->tw);
    f->nty = (int)(((int64_t)h + f->th - 1) / f->th);
    if ((int64_t)f->ntx * f->nty > 65535) {
        elog(log, opaque, "encoder: %dx%d tiles of %dx%d are more than the 65535 a codestream can number\n",
             f->ntx, f->nty, f->tw, f->th);
        return HTJ2K_ERR_EINVAL;
    }
    f->ntiles = f->ntx * f->nty;
    for (dir = 0; dir < 2; dir++) {
        const int n = dir ? f->nty : f->ntx, size = dir ? f->th : f->tw, full = dir ? h : w;
        int t;
        for (t = 0; t < n; t++) {
            const int64_t a = (int64_t)t * size, b = a + size < full ? a + size : full;
            for (c = 0; c < pd->nb_components; c++) {
                const int chroma = c == 1 || c == 2, d = 1 << (chroma ? (dir ? pd->log2_chroma_h : pd->log2_chroma_w) : 0);
                const int64_t ca = (a + d - 1) / d, cb = (b + d - 1) / d;
                if (ca == cb) {
                    elog(log, opaque, "encoder: tiles of %dx%d leave component %d without samples in some tile\n", f->tw, f->th, c);
                    return HTJ2K_ERR_EINVAL;
                }
                far |= cb - ca > 32768;
            }
        }
    }
    if (far) {
        elog(log, opaque, "encoder: tile-components beyond 32768 samples are not supported (use smaller tiles)\n");
        return HTJ2K_ERR_PATCHWELCOME;
    }
    return 0;
}

int enc_frame_init(EncFrame *f, int w, int h, int pix_fmt, int bits, const htj2k_enc_opts *opts_in, enc_log_fn log, void *opaque)
{
    return enc_frame_init_q(f, w, h, pix_fmt, bits, opts_in, NULL, log, opaque);
}

int enc_frame_init_q(EncFrame *f, int w, int h, int pix_fmt, int bits, const htj2k_enc_opts *opts_in, const htj2k_enc_quant *q,
                     enc_log_fn log, void *opaque)
{
    htj2k_enc_opts o;
    const J2kPixDesc *pd = j2k_pix_desc(pix_fmt);
    J2kParser *ps = NULL;
    Wr hw = { 0 };
    int c, r, b, t, ret = 0, nb;
    htj2k_opts dopts;

    memset(f, 0, sizeof *f);
    enc_opts_resolve(opts_in, &o);
    if (!pd || pd->pal || pix_fmt == HTJ2K_PIX_XYZ12) {
        elog(log, opaque, "encoder: pixel format %d is not supported\n", pix_fmt);
        return HTJ2K_ERR_PATCHWELCOME;
    }
    if (w < 1 || h < 1 || bits < 1 || bits > pd->depth[0]) {
        elog(log, opaque, "encoder: %dx%d at %d bits does not fit %s\n", w, h, bits, pd->name);
        return HTJ2K_ERR_EINVAL;
    }
    if ((ret = tile_grid(f, w, h, pd, &o, log, opaque)) < 0)
        return ret;
    if (o.levels < 0 || o.levels > 32 || o.cb_w_log2 < 2 || o.cb_w_log2 > 10 || o.cb_h_log2 < 2 || o.cb_h_log2 > 10 ||
        o.cb_w_log2 + o.cb_h_log2 > 12 || o.mct < -1 || o.mct > 1 || o.guard_bits < 0 || o.guard_bits > 7 ||
        o.irreversible < 0 || o.irreversible > 1) {
        elog(log, opaque, "encoder: options out of range (levels %d, block %dx%d log2, mct %d, guard bits %d, irreversible %d)\n",
             o.levels, o.cb_w_log2, o.cb_h_log2, o.mct, o.guard_bits, o.irreversible);
        return HTJ2K_ERR_EINVAL;
    }
    if (o.irreversible && !(isfinite(o.qstep) && o.qstep > 0)) {
        elog(log, opaque, "encoder: the quantiser's base step %g is not a finite positive number\n", o.qstep);
        return HTJ2K_ERR_EINVAL;
    }
    if (o.target_bytes < 0) {
        elog(log, opaque, "encoder: a byte budget of %lld is negative\n", (long long)o.target_bytes);
        return HTJ2K_ERR_EINVAL;
    }
    if (!(o.target_psnr >= 0) || !isfinite(o.target_psnr)) {
        elog(log, opaque, "encoder: a PSNR target of %g dB is not a finite number >= 0\n", o.target_psnr);
        return HTJ2K_ERR_EINVAL;
    }
    if (o.group_bytes < 0) {
        elog(log, opaque, "encoder: a group budget of %lld bytes is negative\n", (long long)o.group_bytes);
        return HTJ2K_ERR_EINVAL;
    }
    if (o.ht_passes < 0 || o.ht_passes > 3) {
        elog(log, opaque, "encoder: ht_passes %d is not 0 .. 3\n", o.ht_passes);
        return HTJ2K_ERR_EINVAL;
    }
    if (o.mct == 1 && !is_rgb_family(pix_fmt)) {
        elog(log, opaque, "encoder: the component transform applies to the RGB family only\n");
        return HTJ2K_ERR_PATCHWELCOME;
    }
    f->w = w; f->h = h; f->pix_fmt = pix_fmt; f->bits = bits;
    f->ncomp = pd->nb_components;
    f->nl = o.levels;
    f->cbw = o.cb_w_log2; f->cbh = o.cb_h_log2;
    f->mct = o.mct < 0 ? is_rgb_family(pix_fmt) : o.mct;
    f->guard_opt = q ? q->guard_bits : o.guard_bits;
    f->qgiven = q != NULL;
    if (q && (q->guard_bits < 1 || q->guard_bits > 7)) {
        elog(log, opaque, "encoder: %d guard bits given with the quantisation are not 1 .. 7\n", q->guard_bits);
        return HTJ2K_ERR_EINVAL;
    }
    f->irrev = o.irreversible;
    f->target = o.target_bytes;
    f->quality = o.target_psnr;
    f->group = o.group_bytes;
    f->passes = o.ht_passes > 1 ? o.ht_passes : 1;
    f->planar = pd->planar;
    f->step = pd->planar ? 1 : pd->nb_components;
    f->bytes = pd->bytes;
    /* the inverse of write_frame's `<< (precision - cbps)` (j2k_plan.c: out_shift_precision) */
    f->shift = bits <= 8 ? 8 - bits
             : (pix_fmt == HTJ2K_PIX_RGB48 || pix_fmt == HTJ2K_PIX_RGBA64 || pix_fmt == HTJ2K_PIX_GRAY16) ? 16 - bits : 0;
    nb = 3 * f->nl + 1;
    for (c = 0; c < f->ncomp; c++) {
        const int chroma = c == 1 || c == 2;
        f->dx[c] = 1 << (chroma ? pd->log2_chroma_w : 0);
        f->dy[c] = 1 << (chroma ? pd->log2_chroma_h : 0);
        f->cw[c] = (w + f->dx[c] - 1) / f->dx[c];
        f->ch[c] = (h + f->dy[c] - 1) / f->dy[c];
        for (b = 0; b < nb; b++) {
            static const int gain[4] = { 0, 1, 1, 2 };
            const int kind = b ? 1 + (b - 1) % 3 : 0;       /* 0 LL, 1 HL, 2 LH, 3 HH */
            int e, m;
            if (q) {                                        /* as given: a transcoded stream keeps its source's steps */
                if (q->expn[c][b] > 31 || q->mant[c][b] > 2047) {
                    elog(log, opaque, "encoder: the quantisation given for band %d of component %d is out of range\n", b, c);
                    return HTJ2K_ERR_EINVAL;
                }
                f->expn[c][b] = q->expn[c][b];
                f->mant[c][b] = f->irrev ? q->mant[c][b] : 0;
                continue;
            }
            if (!f->irrev) {
                f->expn[c][b] = (uint8_t)(bits + gain[kind] + (f->mct ? 1 : 0));     /* band_quant: +1 on every component */
                continue;
            }
            if (step_rule(o.qstep, bits, f->nl, b, &e, &m) < 0) {
                elog(log, opaque, "encoder: base step %g at %d bits and %d levels gives band %d an exponent outside 0 .. 31\n",
                     o.qstep, bits, f->nl, b);
                return HTJ2K_ERR_EINVAL;
            }
            f->expn[c][b] = (uint8_t)e;
            f->mant[c][b] = (uint16_t)m;
        }
    }

    /* the decoder reads the header back and lays out the blocks (an empty tile-part per tile follows the main header) */
    write_main_header(f, 2, &hw);
    for (t = 0; t < f->ntiles; t++) {
        wr_u16(&hw, 0xFF90); wr_u16(&hw, 10); wr_u16(&hw, (unsigned)t); wr_u32(&hw, 14); wr_u8(&hw, 0); wr_u8(&hw, 1);
        wr_u16(&hw, 0xFF93);
    }
    wr_u16(&hw, 0xFFD9);
    ps = j2k_parser_new();
    if (hw.oom || !ps) {
        ret = HTJ2K_ERR_ENOMEM;
        goto done;
    }
    j2k_parser_set_log(ps, parser_log, NULL);
    memset(&dopts, 0, sizeof dopts);
    dopts.req_pix_fmt = pix_fmt;
    /* the decoder's own entry, headers only (what htj2k_probe runs), then its geometry builder */
    if ((ret = j2k_parse(ps, hw.p, (int)hw.n, &dopts, 1, NULL)) != 0 || !ps->tile) {
        elog(log, opaque, "encoder: the decoder does not accept the header written for this frame\n");
        ret = ret < 0 ? ret : HTJ2K_ERR_BUG;
        goto done;
    }
    if (ps->pix_fmt != pix_fmt) {
        elog(log, opaque, "encoder: %s at %d bits would not decode to the same layout\n", pd->name, bits);
        ret = HTJ2K_ERR_PATCHWELCOME;
        goto done;
    }
    if ((ret = t2_build_geometry(ps)) < 0 || (ret = ps->geo.static_err) < 0)
        goto done;
    if (ps->geo.ntiles != f->ntiles) {
        ret = HTJ2K_ERR_BUG;
        goto done;
    }
    for (t = 0; t < f->ntiles; t++)
        if ((ret = ps->geo.tile_err[t]) < 0) {
            elog(log, opaque, "encoder: the decoder does not accept tile %d of this frame\n", t);
            goto done;
        }

    /* blocks tile by tile, in a tile in packet order: LRCP over one precinct per resolution (none where the tile-component
     * has no samples at that resolution: then there is no packet) */
    {
        const GeomCache *g = &ps->geo;
        int nblk = 0, npb = 0, bi = 0, pi = 0, ki = 0;
        for (t = 0; t < f->ntiles; t++)
            for (r = 0; r <= f->nl; r++)
                for (c = 0; c < f->ncomp; c++) {
                    const ResGeom *rg = &g->tc[t * f->ncomp + c].res[r];
                    if (rg->npx * rg->npy > 1) {
                        ret = HTJ2K_ERR_BUG;
                        goto done;
                    }
                    for (b = 0; b < rg->nbands; b++) {
                        const BandGeom *bg = &rg->band[b];
                        const int gb = r ? 3 * (r - 1) + b + 1 : 0;
                        /* the quantiser divides by the decoder's own step (0 where the decoder refuses the step) */
                        f->fstep[c][gb] = f->irrev ? bg->fstep : 1.0f;
                        if (!(f->fstep[c][gb] > 0) || !isfinite(f->fstep[c][gb])) {
                            elog(log, opaque, "encoder: band %d of component %d gets a step the decoder does not accept\n", gb, c);
                            ret = HTJ2K_ERR_EINVAL;
                            goto done;
                        }
                        if (rg->npx * rg->npy == 0 || bg->x0 == bg->x1 || bg->y0 == bg->y1)
                            continue;
                        nblk += g->pb[rg->pb0 + (uint32_t)b].ncw * g->pb[rg->pb0 + (uint32_t)b].nch;
                        npb++;
                    }
                }
        f->blk = (EncBlock *)calloc((size_t)max32(nblk, 1), sizeof(EncBlock));
        f->pb = (EncPB *)calloc((size_t)max32(npb, 1), sizeof(EncPB));
        f->pkt = (EncPacket *)calloc((size_t)(f->nl + 1) * f->ncomp * f->ntiles, sizeof(EncPacket));
        f->tile = (EncTile *)calloc((size_t)f->ntiles, sizeof(EncTile));
        if (!f->blk || !f->pb || !f->pkt || !f->tile) {
            ret = HTJ2K_ERR_ENOMEM;
            goto done;
        }
        for (t = 0; t < f->ntiles; t++)
            tile_blocks(f, g, t, &bi, &pi, &ki);
        f->nblk = nblk;
        f->npb = npb;
        f->npkt = ki;
    }
    if (f->target > 0 || f->quality > 0 || f->group > 0)
        ret = rc_weights(f);
done:
    free(hw.p);
    j2k_parser_free(ps);
    if (ret < 0)
        enc_frame_free(f);
    return ret < 0 ? ret : 0;
}

void enc_frame_free(EncFrame *f)
{
    free(f->blk); free(f->pb); free(f->pkt); free(f->tile);
    f->blk = NULL; f->pb = NULL; f->pkt = NULL; f->tile = NULL;
}

int enc_guard_bits(const EncFrame *f, const int *max_u, const int *planes, enc_log_fn log, void *opaque)
{
    int i, need = f->qgiven ? 1 : 2;
    if (max_u)
        for (i = 0; i < f->nblk; i++)
            if (max_u[i] > 0)                                        /* M_b = expn + G - 1 >= U + the planes dropped */
                need = max32(need, max_u[i] + (planes ? max32(planes[i], 0) : 0) - f->blk[i].expn + 1);
    if (f->guard_opt && f->guard_opt < need) {
        elog(log, opaque, "encoder: %d guard bits are too few, the coefficients need %d\n", f->guard_opt, need);
        return HTJ2K_ERR_EINVAL;
    }
    if (f->guard_opt)
        need = f->guard_opt;
    if (need > 7) {
        elog(log, opaque, "encoder: %d guard bits do not fit the QCD segment\n", need);
        return HTJ2K_ERR_PATCHWELCOME;
    }
    for (i = 0; i < f->ncomp * (3 * f->nl + 1); i++)
        if (f->expn[i / (3 * f->nl + 1)][i % (3 * f->nl + 1)] + need - 1 > 30) {
            elog(log, opaque, "encoder: a band needs more than 30 magnitude bits\n");
            return HTJ2K_ERR_PATCHWELCOME;
        }
    return need;
}

/* ------------------------------------------------------------------ packet headers (T.800 B.10) */
typedef struct BitOut { Wr *w; uint32_t tmp; int nbits, maxbits; } BitOut;
static void bo_bit(BitOut *b, int bit)
{
    b->tmp = (b->tmp << 1) | (uint32_t)(bit & 1);
    if (++b->nbits == b->maxbits) {
        wr_u8(b->w, b->tmp);
        b->maxbits = b->tmp == 0xFF ? 7 : 8;     /* a byte after 0xFF carries seven bits */
        b->tmp = 0;
        b->nbits = 0;
    }
}
static void bo_bits(BitOut *b, uint32_t v, int n) { while (n-- > 0) bo_bit(b, (int)(v >> n) & 1); }
static void bo_flush(BitOut *b)
{
    if (b->nbits) {
        b->tmp <<= b->maxbits - b->nbits;
        wr_u8(b->w, b->tmp);
        if (b->tmp == 0xFF)
            wr_u8(b->w, 0);
    } else if (b->maxbits == 7) {
        wr_u8(b->w, 0);
    }
}

/* tag tree (T.800 B.10.2) over a ncw x nch grid: leaves first, then each coarser level */
typedef struct TNode { int value, low, known, parent; } TNode;
static TNode *tt_make(int w, int h, int *count)
{
    int lw[40], lh[40], lv = 0, total = 0, k, i, j, base = 0;
    TNode *n;
    lw[0] = w; lh[0] = h;
    for (;;) {
        total += lw[lv] * lh[lv];
        if (lw[lv] <= 1 && lh[lv] <= 1)
            break;
        lw[lv + 1] = (lw[lv] + 1) >> 1; lh[lv + 1] = (lh[lv] + 1) >> 1;
        lv++;
    }
    n = (TNode *)calloc((size_t)total, sizeof(TNode));
    if (!n)
        return NULL;
    for (k = 0; k <= lv; k++) {
        const int next = base + lw[k] * lh[k];
        for (i = 0; i < lh[k]; i++)
            for (j = 0; j < lw[k]; j++)
                n[base + i * lw[k] + j].parent = k == lv ? -1 : next + (i >> 1) * lw[k + 1] + (j >> 1);
        base = next;
    }
    for (i = 0; i < total; i++)
        n[i].value = INT_MAX;
    *count = total;
    return n;
}
static void tt_set(TNode *t, int leaf, int value)
{
    for (int n = leaf; n >= 0 && t[n].value > value; n = t[n].parent)
        t[n].value = value;
}
static void tt_code(TNode *t, BitOut *b, int leaf, int threshold)
{
    int stk[40], sp = 0, n, low = 0;
    for (n = leaf; n >= 0; n = t[n].parent)
        stk[sp++] = n;
    while (sp-- > 0) {
        TNode *nd = &t[stk[sp]];
        if (low > nd->low)
            nd->low = low;
        else
            low = nd->low;
        while (low < threshold) {
            if (low >= nd->value) {
                if (!nd->known) {
                    bo_bit(b, 1);
                    nd->known = 1;
                }
                break;
            }
            bo_bit(b, 0);
            low++;
        }
        nd->low = low;
    }
}

static int bitlen(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

static void out_piece(EncOut *o, uint32_t src, uint32_t len, int block)
{
    if (!len)
        return;
    if (o->npc == o->pc_cap) {
        size_t nc = o->pc_cap ? 2 * o->pc_cap : 256;
        EncPiece *np = (EncPiece *)realloc(o->pc, nc * sizeof(EncPiece));
        if (!np) {
            o->oom = 1;
            return;
        }
        o->pc = np;
        o->pc_cap = nc;
    }
    o->pc[o->npc].dst = o->size;
    o->pc[o->npc].src = src;
    o->pc[o->npc].len = len;
    o->pc[o->npc].block = block;
    o->pc[o->npc].pad = 0;
    o->npc++;
    o->size += len;
}
/* literal bytes: kept in o->lit, one piece */
static void out_lit(EncOut *o, const Wr *w)
{
    if (!w->n)
        return;
    if (o->nlit + w->n > o->lit_cap) {
        size_t nc = o->lit_cap ? 2 * o->lit_cap : 4096;
        uint8_t *np;
        while (nc < o->nlit + w->n)
            nc *= 2;
        np = (uint8_t *)realloc(o->lit, nc);
        if (!np) {
            o->oom = 1;
            return;
        }
        o->lit = np;
        o->lit_cap = nc;
    }
    memcpy(o->lit + o->nlit, w->p, w->n);
    out_piece(o, (uint32_t)o->nlit, (uint32_t)w->n, -1);
    o->nlit += w->n;
}

/* tile t as one tile-part: SOT, SOD and the tile's packets, appended to `o` (hdr, ph: scratch writers) */
static int write_tile(const EncFrame *f, int guard, const int *lcup, const int *lref, const int *npasses, const int *planes,
                      int t, Wr *hdr, Wr *ph, EncOut *o)
{
    /* tile-part length: the packet headers are written first, into the pieces, and Psot patched after */
    const EncTile *et = &f->tile[t];
    const size_t sot_piece = o->nlit;
    uint64_t body = 0;
    int k, p, ret = 0;
    hdr->n = 0;
    wr_u16(hdr, 0xFF90); wr_u16(hdr, 10); wr_u16(hdr, (unsigned)t); wr_u32(hdr, 0); wr_u8(hdr, 0); wr_u8(hdr, 1);
    wr_u16(hdr, 0xFF93);
    out_lit(o, hdr);
    for (p = et->pkt0; p < et->pkt0 + et->npkt && !ret; p++) {
        const EncPacket *pk = &f->pkt[p];
        BitOut bo = { ph, 0, 0, 8 };
        int any = 0, q;
        ph->n = 0;
        for (q = pk->pb0; q < pk->pb0 + pk->npb; q++)
            for (k = 0; k < f->pb[q].ncw * f->pb[q].nch; k++)
                any |= lcup[f->pb[q].blk0 + k] > 0;
        if (!any) {
            bo_bit(&bo, 0);                          /* empty packet */
            bo_flush(&bo);
            out_lit(o, ph);
            body += ph->n;
            continue;
        }
        bo_bit(&bo, 1);
        for (q = pk->pb0; q < pk->pb0 + pk->npb && !ret; q++) {
            const EncPB *pb = &f->pb[q];
            const int nb = pb->ncw * pb->nch;
            int nincl = 0, nzbp = 0;
            TNode *incl = tt_make(pb->ncw, pb->nch, &nincl), *zbp = tt_make(pb->ncw, pb->nch, &nzbp);
            if (!incl || !zbp) {
                free(incl); free(zbp);
                ret = HTJ2K_ERR_ENOMEM;
                break;
            }
            for (k = 0; k < nb; k++) {
                const int in = lcup[pb->blk0 + k] > 0;
                tt_set(incl, k, in ? 0 : 1);
                if (in)      /* zbp = M_b - 1 - p: one cleanup pass that starts at bit-plane p */
                    tt_set(zbp, k, f->blk[pb->blk0 + k].expn + guard - 2 - (planes ? planes[pb->blk0 + k] : 0));
            }
            for (k = 0; k < nb; k++) {
                const int L = lcup[pb->blk0 + k];
                const int np = npasses ? npasses[pb->blk0 + k] : 1, Lr = np > 1 ? lref[pb->blk0 + k] : 0, b2 = np == 3;
                int lblock = 3, extra;
                tt_code(incl, &bo, k, 1);
                if (L <= 0)
                    continue;
                tt_code(zbp, &bo, k, f->blk[pb->blk0 + k].expn + guard - 1 - (planes ? planes[pb->blk0 + k] : 0));
                if (np == 1)                         /* the number of coding passes (T.800 Table B.4) */
                    bo_bit(&bo, 0);
                else if (np == 2)
                    bo_bits(&bo, 2, 2);
                else
                    bo_bits(&bo, 0xC, 4);
                /* Lblock holds both fields: the refinement segment's has Lblock bits, one more for two passes in it */
                for (extra = max32(0, max32(bitlen((uint32_t)L), bitlen((uint32_t)Lr) - b2) - lblock); extra > 0; extra--) {
                    bo_bit(&bo, 1);                  /* Lblock increments (B.10.7.1) */
                    lblock++;
                }
                bo_bit(&bo, 0);
                bo_bits(&bo, (uint32_t)L, lblock);
                if (np > 1)
                    bo_bits(&bo, (uint32_t)Lr, lblock + b2);
            }
            free(incl); free(zbp);
        }
        bo_flush(&bo);
        out_lit(o, ph);
        body += ph->n;
        for (q = pk->pb0; q < pk->pb0 + pk->npb; q++)
            for (k = 0; k < f->pb[q].ncw * f->pb[q].nch; k++) {
                const int i = f->pb[q].blk0 + k;
                if (lcup[i] > 0) {                   /* Dref lies behind Dcup */
                    const uint32_t n = (uint32_t)lcup[i] + (uint32_t)(npasses && npasses[i] > 1 ? lref[i] : 0);
                    out_piece(o, 0, n, i);
                    body += n;
                }
            }
    }
    if (ret < 0 || hdr->oom || ph->oom || o->oom)
        return ret;
    if (body + 14 > 0xFFFFFFFFu)
        return HTJ2K_ERR_PATCHWELCOME;
    {
        uint8_t *psot = o->lit + sot_piece + 6;      /* Psot: SOT .. end of the tile-part's data */
        const uint32_t v = (uint32_t)(body + 14);
        psot[0] = (uint8_t)(v >> 24); psot[1] = (uint8_t)(v >> 16); psot[2] = (uint8_t)(v >> 8); psot[3] = (uint8_t)v;
    }
    return 0;
}

int enc_write(const EncFrame *f, int guard, const int *lcup, const int *lref, const int *npasses, const int *planes, EncOut *o)
{
    Wr hdr = { 0 }, ph = { 0 };
    int t, ret = 0;

    write_main_header(f, guard, &hdr);
    out_lit(o, &hdr);
    for (t = 0; t < f->ntiles && !ret; t++)
        ret = write_tile(f, guard, lcup, lref, npasses, planes, t, &hdr, &ph, o);
    hdr.n = 0;
    wr_u16(&hdr, 0xFFD9);
    out_lit(o, &hdr);
    free(hdr.p); free(ph.p);
    if (hdr.oom || ph.oom || o->oom)
        return HTJ2K_ERR_ENOMEM;
    return ret;
}

int64_t enc_min_size(const EncFrame *f)
{
    EncOut o;
    int64_t n;
    int *lcup = (int *)calloc((size_t)max32(f->nblk, 1), sizeof(int));
    int r;
    memset(&o, 0, sizeof o);
    if (!lcup)
        return HTJ2K_ERR_ENOMEM;
    r = enc_write(f, 2, lcup, NULL, NULL, NULL, &o);          /* the guard bits are a field of QCD: they do not change the size */
    n = r < 0 ? r : (int64_t)o.size;
    enc_out_free(&o);
    free(lcup);
    return n;
}

void enc_out_free(EncOut *o)
{
    free(o->lit); free(o->pc);
    memset(o, 0, sizeof *o);
}

/* MagSgn: at most 32 bits per sample, seven in a byte after 0xFF; MEL + VLC: Scup <= 4079.  The 32 bits hold for
 * any index the quantiser writes (|v| <= 2147483000 < 2^31: 2 (|v| - 1) + sign < 2^32), i.e. for M_b up to 31, and
 * so for lossless and lossy blocks alike. */
size_t enc_block_bound(int w, int h)
{
    return ((size_t)w * h * 32 + 6) / 7 + 4080;
}

/* Dref: SigProp writes at most 2 bits (the bit and a sign) for a sample the cleanup pass left insignificant, MagRef 1
 * for a significant one; each pass packs at least 7 bits to a byte and ends in a partial one */
size_t enc_refine_bound(int w, int h)
{
    return ((size_t)w * h * 2 + 6) / 7 + 2;
}

/* ------------------------------------------------------------------ rate control: the last resort's choice */
static int drop_cmp(const void *pa, const void *pb)
{
    const EncDrop *a = (const EncDrop *)pa, *b = (const EncDrop *)pb;
    if (a->gain != b->gain)
        return a->gain < b->gain ? -1 : 1;
    return (a->block > b->block) - (a->block < b->block);
}

size_t enc_drop_take(EncDrop *e, size_t n, size_t next, int64_t excess, int64_t *saved)
{
    if (next == 0 && n > 1)
        qsort(e, n, sizeof *e, drop_cmp);
    *saved = 0;
    while (next < n && *saved < excess)
        *saved += e[next++].bytes;
    return next;
}

/* ------------------------------------------------------------------ context-free entry points */
size_t htj2k_encode_bound(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts)
{
    EncFrame f;
    size_t n;
    if (enc_frame_init(&f, width, height, pix_fmt, bits, opts, NULL, NULL) < 0)
        return 0;
    n = enc_frame_bound(&f);
    enc_frame_free(&f);
    return n;
}

size_t enc_frame_bound(const EncFrame *f)
{
    size_t n;
    int i;
    /* headers: SOC SIZ CAP COD QCD + QCCs (two bytes a band for 9/7), per tile SOT SOD, EOC; per packet one byte of
     * header (+ a stuffed one), per block at most 2 * 2 * log2 of the grid tag-tree bits, 1 pass bit, up to 32 Lblock
     * bits and the length; with refinement passes Dref, 3 more pass bits and the second length (3 bytes cover both) */
    n = 2 + 2 + 38 + 3 * 4 + 12 + 14 + 4 * (2 + 4 + 2 * (3 * 32 + 1)) + (size_t)f->ntiles * 14 + 2 + (size_t)f->npkt * 2;
    for (i = 0; i < f->nblk; i++)
        n += enc_block_bound(f->blk[i].w, f->blk[i].h) + (f->passes > 1 ? enc_refine_bound(f->blk[i].w, f->blk[i].h) + 3 : 0) + 16;
    return n;
}

int htj2k_enc_layout(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts,
                     htj2k_enc_block *blocks, int cap)
{
    EncFrame f;
    int r = enc_frame_init(&f, width, height, pix_fmt, bits, opts, NULL, NULL);
    if (r < 0)
        return r;
    if (blocks && cap > 0)
        memcpy(blocks, f.blk, (size_t)min32(cap, f.nblk) * sizeof(EncBlock));
    r = f.nblk;
    enc_frame_free(&f);
    return r;
}

int htj2k_enc_band_weights(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts, double *w, int cap)
{
    EncFrame f;
    int i, r = enc_frame_init(&f, width, height, pix_fmt, bits, opts, NULL, NULL);
    if (r < 0)
        return r;
    if ((r = rc_weights(&f)) == 0) {
        for (i = 0; w && i < cap && i < f.nblk; i++)
            w[i] = enc_block_weight(&f, &f.blk[i]);
        r = f.nblk;
    }
    enc_frame_free(&f);
    return r;
}

double enc_block_weight(const EncFrame *f, const EncBlock *b)
{
    return f->wgt[b->comp][b->res ? 3 * (b->res - 1) + b->band : 0];
}

float enc_block_step(const EncFrame *f, const EncBlock *b)
{
    return f->fstep[b->comp][b->res ? 3 * (b->res - 1) + b->band : 0];
}

int htj2k_enc_tiles(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts, htj2k_enc_tile *tiles, int cap)
{
    EncFrame f;
    int i, r = enc_frame_init(&f, width, height, pix_fmt, bits, opts, NULL, NULL);
    if (r < 0)
        return r;
    for (i = 0; tiles && i < cap && i < f.ntiles; i++)
        tiles[i] = f.tile[i].t;
    r = f.ntiles;
    enc_frame_free(&f);
    return r;
}

static int assemble(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts, const htj2k_enc_quant *quant,
                    const uint8_t *const *block_bytes, const int *lcup, const int *lref, const int *npasses,
                    const int *max_u, const int *planes, int nblocks, uint8_t *out, size_t cap, size_t *out_len);

int htj2k_enc_assemble(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts,
                       const uint8_t *const *block_bytes, const int *lcup, const int *max_u, int nblocks,
                       uint8_t *out, size_t cap, size_t *out_len)
{
    return htj2k_enc_assemble_planes(width, height, pix_fmt, bits, opts, block_bytes, lcup, max_u, NULL, nblocks, out, cap, out_len);
}

int htj2k_enc_assemble_planes(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts,
                              const uint8_t *const *block_bytes, const int *lcup, const int *max_u, const int *planes,
                              int nblocks, uint8_t *out, size_t cap, size_t *out_len)
{
    return htj2k_enc_assemble_passes(width, height, pix_fmt, bits, opts, block_bytes, lcup, NULL, NULL, max_u, planes, nblocks,
                                     out, cap, out_len);
}

int htj2k_enc_assemble_passes(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts,
                              const uint8_t *const *block_bytes, const int *lcup, const int *lref, const int *npasses,
                              const int *max_u, const int *planes, int nblocks, uint8_t *out, size_t cap, size_t *out_len)
{
    return assemble(width, height, pix_fmt, bits, opts, NULL, block_bytes, lcup, lref, npasses, max_u, planes, nblocks, out, cap,
                    out_len);
}

int htj2k_enc_assemble_quant(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts,
                             const htj2k_enc_quant *quant, const uint8_t *const *block_bytes, const int *lcup,
                             const int *lref, const int *npasses, const int *planes, int nblocks,
                             uint8_t *out, size_t cap, size_t *out_len)
{
    if (!quant) {
        if (out_len)
            *out_len = 0;
        return HTJ2K_ERR_EINVAL;
    }
    return assemble(width, height, pix_fmt, bits, opts, quant, block_bytes, lcup, lref, npasses, NULL, planes, nblocks, out, cap,
                    out_len);
}

static int assemble(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts, const htj2k_enc_quant *quant,
                    const uint8_t *const *block_bytes, const int *lcup, const int *lref, const int *npasses,
                    const int *max_u, const int *planes, int nblocks, uint8_t *out, size_t cap, size_t *out_len)
{
    EncFrame f;
    EncOut o;
    size_t i;
    int r, guard, *cp = NULL;                           /* cp: the plane of every block's cleanup pass */
    memset(&o, 0, sizeof o);
    if (out_len)
        *out_len = 0;
    if ((r = enc_frame_init_q(&f, width, height, pix_fmt, bits, opts, quant, NULL, NULL)) < 0)
        return r;
    r = HTJ2K_ERR_EINVAL;
    if (nblocks != f.nblk || (f.nblk && (!lcup || !block_bytes)) || !out || (npasses && !lref))
        goto done;
    for (i = 0; i < (size_t)f.nblk; i++)
        if (lcup[i] < 0 || (lcup[i] > 0 && !block_bytes[i]))
            goto done;
    /* a refinement segment comes with more than one pass and with a cleanup segment, and only so */
    for (i = 0; npasses && i < (size_t)f.nblk; i++)
        if (npasses[i] < 1 || npasses[i] > 3 || lref[i] < 0 || (lref[i] > 0) != (npasses[i] > 1) || (lref[i] > 0 && lcup[i] == 0))
            goto done;
    if (planes || npasses) {
        if (!(cp = (int *)malloc((size_t)max32(f.nblk, 1) * sizeof(int)))) {
            r = HTJ2K_ERR_ENOMEM;
            goto done;
        }
        for (i = 0; i < (size_t)f.nblk; i++) {
            const int p = planes ? planes[i] : 0, up = npasses && npasses[i] > 1;
            if (p < -1 || p + up > 31 || (p < 0 && lcup[i] > 0))
                goto done;
            cp[i] = p < 0 ? p : p + up;
        }
    }
    if ((guard = enc_guard_bits(&f, max_u, cp, NULL, NULL)) < 0) {
        r = guard;
        goto done;
    }
    for (i = 0; cp && i < (size_t)f.nblk; i++)
        if (lcup[i] > 0 && f.blk[i].expn + guard - 2 - cp[i] < 0)
            goto done;
    r = enc_write(&f, guard, lcup, lref, npasses, cp, &o);
    if (!r && o.size > cap)
        r = HTJ2K_ERR_ENOSPC;
    if (!r) {
        for (i = 0; i < o.npc; i++) {
            const EncPiece *p = &o.pc[i];
            memcpy(out + p->dst, p->block < 0 ? o.lit + p->src : block_bytes[p->block], p->len);
        }
        if (out_len)
            *out_len = (size_t)o.size;
    }
done:
    free(cp);
    enc_out_free(&o);
    enc_frame_free(&f);
    return r;
}
