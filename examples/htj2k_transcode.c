/*
 * htj2k_transcode.c -- plain-C use of the transcoder: a Part-1 (EBCOT / MQ) codestream or JP2 file is re-coded block by
 * block into an HTJ2K codestream on the GPU (htj2k_transcode_frame), and both are decoded (htj2k_decode) and compared:
 * the output must give the very same frame, 5/3 and 9/7 alike, for no coefficient changes on the way.
 * With a budget in bytes as third argument (htj2k_transcode_frame_opts) the output is at most that large: blocks keep
 * their source's form or a coarser one, so the frames may differ, and the check is that the output decodes without a
 * block error.
 * With --ht-sources in front (htj2k_transcode_opts.ht_sources) the source may itself hold HT code-blocks, an HTJ2K or a
 * MIXED stream: with a budget that makes a smaller HTJ2K stream of an HTJ2K master, with no transform and no second
 * quantiser.
 *
 *   make examples && ./examples/htj2k_transcode [--ht-sources] in.j2c out.jph [bytes]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "htj2k_amd.h"

static void log_line(void *opaque, int level, const char *msg)
{
    (void)opaque; (void)level;
    fputs(msg, stderr);
}

static uint8_t *read_file(const char *path, size_t *size)
{
    FILE *f = fopen(path, "rb");
    uint8_t *p = NULL;
    long n;
    if (!f)
        return NULL;
    if (fseek(f, 0, SEEK_END) == 0 && (n = ftell(f)) > 0 && fseek(f, 0, SEEK_SET) == 0 && (p = calloc(1, (size_t)n + 64)) != NULL) {
        if (fread(p, 1, (size_t)n, f) != (size_t)n) {
            free(p);
            p = NULL;
        }
        *size = (size_t)n;                             /* 64 bytes of zero padding follow, as after an AVPacket */
    }
    fclose(f);
    return p;
}

static int decode(htj2k_ctx *dec, const uint8_t *cs, size_t len, htj2k_info *info, uint8_t *planes[4], size_t bytes[4],
                  htj2k_stats *st)
{
    htj2k_frame fr;
    int p, r;
    if ((r = htj2k_probe(dec, cs, (int)len, info)) < 0)
        return r;
    memset(&fr, 0, sizeof fr);
    for (p = 0; p < info->nplanes; p++) {
        fr.linesize[p] = info->plane_width[p] * info->plane_bytes_per_sample[p];
        bytes[p] = (size_t)fr.linesize[p] * info->plane_height[p];
        fr.data[p] = planes[p] = calloc(1, bytes[p] ? bytes[p] : 1);
    }
    return htj2k_decode(dec, cs, (int)len, &fr, st);
}

int main(int argc, char **argv)
{
    htj2k_ctx *dec = NULL;
    htj2k_enc_ctx *enc = NULL;
    htj2k_opts o;
    htj2k_transcode_opts xo;
    htj2k_stats sa, sb;
    htj2k_info ia, ib;
    uint8_t *src, *out, *pa[4] = { 0 }, *pb[4] = { 0 };
    size_t n = 0, bound = 0, len = 0, na[4] = { 0 }, nb[4] = { 0 };
    int r, p, same = 1, ok;
    const char *from;
    FILE *f;

    htj2k_transcode_opts_default(&xo);
    if (argc > 1 && strcmp(argv[1], "--ht-sources") == 0) {
        xo.ht_sources = 1;
        argv[1] = argv[0];
        argv++;
        argc--;
    }
    if (argc != 3 && argc != 4) {
        fprintf(stderr, "usage: %s [--ht-sources] in.j2c|in.jp2 out.jph [bytes]\n", argv[0]);
        return 2;
    }
    if (argc == 4 && (xo.target_bytes = atoll(argv[3])) <= 0) {
        fprintf(stderr, "the budget is a number of bytes above 0\n");
        return 2;
    }
    if (!(src = read_file(argv[1], &n))) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    /* no device needed yet: is the stream in scope, and how large can the output get? */
    if ((r = htj2k_transcode_check_opts(src, (int)n, &xo, &bound, NULL, log_line, NULL)) < 0) {
        fprintf(stderr, "%s cannot be transcoded: %d\n", argv[1], r);
        return 1;
    }
    out = malloc(bound);
    memset(&o, 0, sizeof o);
    o.req_pix_fmt = HTJ2K_PIX_NONE;
    if ((r = htj2k_open(&o, &dec)) < 0 || (r = htj2k_enc_open(0, &enc)) < 0) {
        fprintf(stderr, "no device: %d\n", r);
        return 1;
    }
    htj2k_set_log(dec, log_line, NULL);
    htj2k_enc_set_log(enc, log_line, NULL);
    if ((r = htj2k_transcode_frame_opts(dec, enc, src, (int)n, &xo, out, bound, &len)) < 0) {
        fprintf(stderr, "transcode failed: %d\n", r);
        return 1;
    }
    if (!(f = fopen(argv[2], "wb")) || fwrite(out, 1, len, f) != len || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    if ((r = decode(dec, src, n, &ia, pa, na, &sa)) < 0 || (r = decode(dec, out, len, &ib, pb, nb, &sb)) < 0) {
        fprintf(stderr, "decode failed: %d\n", r);
        return 1;
    }
    from = ia.is_ht ? "HTJ2K" : "Part-1";                  /* (a source with HT code-blocks: only with --ht-sources) */
    same = ia.width == ib.width && ia.height == ib.height && ia.pix_fmt == ib.pix_fmt && ia.nplanes == ib.nplanes && ib.is_ht == 1;
    for (p = 0; same && p < ia.nplanes; p++)
        same = na[p] == nb[p] && memcmp(pa[p], pb[p], na[p]) == 0;
    if (xo.target_bytes > 0) {
        ok = sb.n_block_errors == 0 && (long long)len <= (long long)xo.target_bytes && ia.width == ib.width &&
             ia.height == ib.height && ia.pix_fmt == ib.pix_fmt && ib.is_ht == 1;
        printf("%dx%d: %zu bytes of %s -> %zu bytes of HTJ2K (budget %lld, bound %zu), %d block errors, %s\n", ia.width,
               ia.height, n, from, len, (long long)xo.target_bytes, bound, sb.n_block_errors,
               same ? "frames identical" : "frames differ");
    } else {
        ok = same;
        printf("%dx%d: %zu bytes of %s -> %zu bytes of HTJ2K (bound %zu), %s\n", ia.width, ia.height, n, from, len, bound,
               same ? "frames identical" : "frames DIFFER");
    }
    for (p = 0; p < 4; p++) {
        free(pa[p]);
        free(pb[p]);
    }
    htj2k_enc_close(enc);
    htj2k_close(dec);
    free(src); free(out);
    return ok ? 0 : 1;
}
