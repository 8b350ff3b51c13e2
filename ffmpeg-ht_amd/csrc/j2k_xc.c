/*
 * j2k_xc.c -- host side of the transcoder (Part-1, and on request HT and MIXED, in, HTJ2K out; DESIGN.md 3.5, "Transcoding"): what a parsed
 * source must look like, the encoder's frame with the source's parameters, the 1:1 matching of the source's
 * code-blocks with the encoder's layout, the block rule, and the context-free htj2k_transcode_check.
 *
 * The source is read by the decoder's parser (j2k_syntax.c, j2k_tier2.c, j2k_plan.c); the layout is the encoder's
 * (j2k_enc.c), which is itself laid out by the decoder's geometry code.  Both number the samples of a component in
 * the same plane (every tile-component's Mallat layout in its rectangle), so two blocks are the same block when
 * they have the same component and the same rectangle there.
 */
#include <stdio.h>
#include <stdlib.h>
#include "j2k_host.h"
#include "j2k_enc.h"

static int refuse(enc_log_fn log, void *opaque, int err, const char *fmt, ...) __attribute__((format(printf, 4, 5)));
static int refuse(enc_log_fn log, void *opaque, int err, const char *fmt, ...)
{
    char msg[256];
    va_list ap;
    if (log) {
        int n = snprintf(msg, sizeof msg, "transcode: ");
        va_start(ap, fmt);
        vsnprintf(msg + n, sizeof msg - (size_t)n, fmt, ap);
        va_end(ap);
        log(opaque, LOGL_ERROR, msg);
    }
    return err;
}

/* what the headers say: < 0 refuses; else the encoder's options and the quantisation to copy.  ht_sources: streams
 * with HT code-blocks (HT or MIXED) are in scope (htj2k_transcode_opts.ht_sources) */
static int source_params(const J2kParser *ps, int ht_sources, htj2k_enc_opts *o, htj2k_enc_quant *q, int *bits, enc_log_fn log, void *opaque)
{
    const CompCoding *k0 = &ps->cod[0];
    const J2kPixDesc *pd = j2k_pix_desc(ps->pix_fmt);
    int c, b, t, nb;

    for (c = 0; c < ps->ncomp; c++)
        if (!ht_sources && (ps->is_ht || (ps->cod[c].cb_style & (CBS_HT | CBS_HT_MIXED))))
            return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "the source has HT code-blocks already\n");
    if (ps->reduce)
        return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "a reduction factor drops resolutions the output must keep\n");
    if (ps->ncomp < 1 || ps->ncomp > J2K_MAX_COMPS || !pd || pd->pal || ps->palettised || ps->pix_fmt == HTJ2K_PIX_XYZ12)
        return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "pixel format %d is not one the encoder writes\n", ps->pix_fmt);
    if (ps->xosiz || ps->yosiz || ps->xtosiz || ps->ytosiz)
        return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "image or tile-grid origin (%d, %d) / (%d, %d) is not 0\n",
                      ps->xosiz, ps->yosiz, ps->xtosiz, ps->ytosiz);
    for (c = 0; c < ps->ncomp; c++) {
        const CompCoding *k = &ps->cod[c];
        if (ps->is_signed[c])
            return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "component %d is signed\n", c);
        if (ps->roi[c])
            return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "component %d has a region of interest (RGN shift %d)\n", c, ps->roi[c]);
        if (ps->depth[c] != ps->depth[0] || ps->q[c].guard != ps->q[0].guard)
            return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "component %d differs in depth or guard bits\n", c);
        if (k->nres != k0->nres || k->cbw != k0->cbw || k->cbh != k0->cbh || k->wavelet != k0->wavelet ||
            k->cb_style != k0->cb_style || k->mct != k0->mct)
            return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME,
                          "component %d differs in levels, block size, transform or style: more than one COD can say\n", c);
    }
    for (t = 0; t < (int)(ps->tiles_x * ps->tiles_y); t++) {
        if (ps->tile[t].own_params & TILE_OWN_PARAMS)
            return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "tile %d has coding parameters of its own\n", t);
        for (c = 0; c < ps->ncomp; c++)
            if (ps->tile[t].roi[c])
                return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "tile %d has a region of interest\n", t);
    }
    htj2k_enc_opts_default(o);
    o->levels = k0->nres - 1;
    o->cb_w_log2 = k0->cbw;
    o->cb_h_log2 = k0->cbh;
    o->mct = k0->mct ? 1 : 0;
    o->irreversible = k0->wavelet != J2K_DWT53;
    o->tile_w = ps->xtsiz;
    o->tile_h = ps->ytsiz;
    o->ht_passes = 3;                                   /* room for what the rule may ask of a block */
    memset(q, 0, sizeof *q);
    q->guard_bits = ps->q[0].guard;
    nb = 3 * o->levels + 1;
    for (c = 0; c < ps->ncomp; c++) {
        const CompQuant *s = &ps->q[c];
        /* the output signals "no quantisation" with 5/3 and expounded steps with 9/7, as the encoder does */
        if (o->irreversible ? (s->style != 1 && s->style != 2) : s->style != 0)
            return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "quantisation style %d of component %d does not go with its transform\n",
                          s->style, c);
        for (b = 0; b < nb; b++) {
            if (s->expn[b] + s->guard - 1 > 30 || s->guard < 1)
                return refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "band %d of component %d has more than 30 magnitude bits or no guard bit\n", b, c);
            q->expn[c][b] = s->expn[b];
            q->mant[c][b] = o->irreversible ? s->mant[b] : 0;      /* a derived QCD is expanded by the parser already */
        }
    }
    *bits = ps->depth[0];
    return 0;
}

typedef struct Key { int32_t comp, y, x, idx; } Key;
static int key_cmp(const void *a, const void *b)
{
    const Key *p = (const Key *)a, *q = (const Key *)b;
    if (p->comp != q->comp) return p->comp < q->comp ? -1 : 1;
    if (p->y != q->y) return p->y < q->y ? -1 : 1;
    if (p->x != q->x) return p->x < q->x ? -1 : 1;
    return 0;
}

void xc_frame_free(XcFrame *x)
{
    enc_frame_free(&x->f);
    free(x->src); free(x->plane); free(x->passes);
    x->src = x->plane = x->passes = NULL;
}

/* 0 / 1, else HTJ2K_ERR_EINVAL with a log line */
int xc_ht_sources_ok(int ht_sources, enc_log_fn log, void *opaque)
{
    if (ht_sources == 0 || ht_sources == 1)
        return 0;
    return refuse(log, opaque, HTJ2K_ERR_EINVAL, "ht_sources is 0 or 1, not %d\n", ht_sources);
}

int xc_frame_init(XcFrame *x, const J2kParser *ps, const J2kPlan *plan, int ht_sources, enc_log_fn log, void *opaque)
{
    htj2k_enc_opts o;
    htj2k_enc_quant q;
    EncFrame *f = &x->f;
    Key *keys = NULL;
    int bits = 0, r, i, c, t;

    memset(x, 0, sizeof *x);
    if ((r = source_params(ps, ht_sources, &o, &q, &bits, log, opaque)) < 0)
        return r;
    if ((r = enc_frame_init_q(f, ps->xsiz, ps->ysiz, ps->pix_fmt, bits, &o, &q, log, opaque)) < 0) {
        /* what the encoder cannot lay out is out of scope here, whatever it calls it */
        return refuse(log, opaque, r == HTJ2K_ERR_ENOMEM ? r : HTJ2K_ERR_PATCHWELCOME, "the encoder does not take the source's layout\n");
    }
    for (c = 0; c < f->ncomp; c++)
        if (f->dx[c] != ps->sub_x[c] || f->dy[c] != ps->sub_y[c]) {
            r = refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "component %d is sub-sampled otherwise than its pixel format says\n", c);
            goto fail;
        }
    x->src = (int32_t *)malloc((size_t)max32(f->nblk, 1) * sizeof(int32_t));
    x->plane = (int32_t *)malloc((size_t)max32(f->nblk, 1) * sizeof(int32_t));
    x->passes = (int32_t *)malloc((size_t)max32(f->nblk, 1) * sizeof(int32_t));
    keys = (Key *)malloc((size_t)max32(f->nblk, 1) * sizeof(Key));
    if (!x->src || !x->plane || !x->passes || !keys) {
        r = HTJ2K_ERR_ENOMEM;
        goto fail;
    }
    if (plan->nblocks != f->nblk || plan->ntilecomps != f->ntiles * f->ncomp) {
        r = refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME, "the source has %d code-blocks where the encoder's layout has %d: precincts cut its blocks\n",
                   plan->nblocks, f->nblk);
        goto fail;
    }
    for (i = 0; i < f->nblk; i++) {
        keys[i].comp = f->blk[i].comp; keys[i].y = f->blk[i].y; keys[i].x = f->blk[i].x; keys[i].idx = i;
        x->src[i] = -1;
    }
    qsort(keys, (size_t)f->nblk, sizeof(Key), key_cmp);
    for (i = 0; i < plan->nblocks; i++) {
        const J2kBlock *b = &plan->blocks[i];
        const J2kTileComp *tc;
        Key want, *hit;
        uint32_t off;
        int n, K, k, rr, pc;
        /* the block's tile-component, and where the block lies in that plane */
        t = (int)ps->geo.row_tc[i];
        if (t < 0 || t >= plan->ntilecomps || !b->stride || b->plane_off < plan->tilecomps[t].plane_off) {
            r = HTJ2K_ERR_BUG;
            goto fail;
        }
        tc = &plan->tilecomps[t];
        off = b->plane_off - tc->plane_off;
        want.comp = tc->comp;
        want.y = tc->y0 + (int32_t)(off / b->stride);
        want.x = tc->x0 + (int32_t)(off % b->stride);
        hit = (Key *)bsearch(&want, keys, (size_t)f->nblk, sizeof(Key), key_cmp);
        if (!hit || f->blk[hit->idx].w != b->w || f->blk[hit->idx].h != b->h || x->src[hit->idx] >= 0) {
            r = refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME,
                       "the %dx%d code-block at (%d, %d) of component %d is not in the encoder's layout: precincts cut the source's blocks\n",
                       b->w, b->h, want.x, want.y, want.comp);
            goto fail;
        }
        x->src[hit->idx] = i;
        /* the block rule, by the block's own coder */
        n = b->npasses;
        x->plane[hit->idx] = -1;
        x->passes[hit->idx] = 1;
        if (!n)
            continue;
        if (!(b->flags & J2K_BLK_PART1)) {
            /* an HT block: n counts the placeholder passes, zbp is the true count of zero bit-planes; the cleanup pass
             * lies S_blk planes below the top of the band's M_b (what the kernels compute as num_plhd / 3 + zbp) */
            const int P0 = (n - 1) / 3, S_blk = b->zbp + P0;
            if (!ht_sources) {                          /* (source_params has refused such a stream) */
                r = HTJ2K_ERR_BUG;
                goto fail;
            }
            k = n - 3 * P0;
            pc = b->M_b - 1 - S_blk;
            if (pc - (k > 1) < 0) {
                r = refuse(log, opaque, HTJ2K_ERR_INVALIDDATA, "a code-block has %d passes over %d bit-planes\n", n, b->M_b - b->zbp);
                goto fail;
            }
            x->plane[hit->idx] = pc - (k > 1);
            x->passes[hit->idx] = k;
            continue;
        }
        K = b->zbp;
        k = (n - 1) / 3; rr = (n - 1) % 3;
        pc = K - 1 - k;
        if (pc - (rr > 0) < 0) {
            r = refuse(log, opaque, HTJ2K_ERR_INVALIDDATA, "a code-block has %d passes over %d bit-planes\n", n, K);
            goto fail;
        }
        if (K >= b->M_b) {
            r = refuse(log, opaque, HTJ2K_ERR_PATCHWELCOME,
                       "a code-block fills all %d magnitude bits of its band: an HT block needs one more guard bit\n", b->M_b);
            goto fail;
        }
        x->plane[hit->idx] = rr ? pc - 1 : pc;
        x->passes[hit->idx] = 1 + rr;
    }
    free(keys);
    return 0;
fail:
    free(keys);
    xc_frame_free(x);
    return r;
}

typedef struct CheckLog { htj2k_log_fn fn; void *opaque; } CheckLog;
static void check_log(void *opaque, int level, const char *msg)
{
    const CheckLog *l = (const CheckLog *)opaque;
    if (l->fn)
        l->fn(l->opaque, level, msg);
}

int htj2k_transcode_check(const uint8_t *pkt, int pkt_size, size_t *bound, htj2k_log_fn log, void *opaque)
{
    return htj2k_transcode_check_opts(pkt, pkt_size, NULL, bound, NULL, log, opaque);
}

int htj2k_transcode_min_size(const uint8_t *pkt, int pkt_size, int64_t *min_bytes, htj2k_log_fn log, void *opaque)
{
    if (!min_bytes)
        return HTJ2K_ERR_EINVAL;
    return htj2k_transcode_check_opts(pkt, pkt_size, NULL, NULL, min_bytes, log, opaque);
}

int htj2k_transcode_check_opts(const uint8_t *pkt, int pkt_size, const htj2k_transcode_opts *opts, size_t *bound, int64_t *min_bytes,
                               htj2k_log_fn log, void *opaque)
{
    CheckLog l = { log, opaque };
    const int ht_sources = opts ? opts->ht_sources : 0;
    const J2kPlan *plan = NULL;
    J2kParser *ps;
    XcFrame x;
    int r;
    if (bound)
        *bound = 0;
    if (min_bytes)
        *min_bytes = 0;
    if (!pkt || pkt_size < 1)
        return HTJ2K_ERR_EINVAL;
    if ((r = xc_ht_sources_ok(ht_sources, check_log, &l)) < 0)
        return r;
    if (!(ps = j2k_parser_new()))
        return HTJ2K_ERR_ENOMEM;
    j2k_parser_set_log(ps, check_log, &l);
    j2k_parser_set_gather(ps, 0);                       /* the packet headers are read, the code-block bytes are not */
    /* the headers first: what is out of scope is said to be so even where the decoder would not take the packets */
    if ((r = j2k_parse(ps, pkt, pkt_size, NULL, 1, &plan)) == 0) {
        htj2k_enc_opts o;
        htj2k_enc_quant q;
        int bits;
        r = source_params(ps, ht_sources, &o, &q, &bits, check_log, &l);
    }
    if (r == 0 && (r = j2k_parse(ps, pkt, pkt_size, NULL, 0, &plan)) == 0 && (r = xc_frame_init(&x, ps, plan, ht_sources, check_log, &l)) == 0) {
        if (bound)
            *bound = enc_frame_bound(&x.f);
        if (min_bytes && (*min_bytes = enc_min_size(&x.f)) < 0) {
            r = (int)*min_bytes;
            *min_bytes = 0;
        }
        xc_frame_free(&x);
    }
    j2k_parser_free(ps);
    return r;
}
