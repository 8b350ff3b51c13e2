/*
 * htj2k_encode.c -- plain-C round trip through the library: a synthetic RGB frame is encoded
 * losslessly on the GPU (htj2k_encode_frame), decoded again (htj2k_decode) and compared; then once
 * more as a grid of 1000 x 1000 tiles (htj2k_enc_opts.tile_w / tile_h).  With a byte budget the frame is coded again under it (rate control: lossless where that fits, 5/3 with
 * dropped bit-planes where not), its size checked against the budget, and decoded.
 *
 *   make examples && ./examples/htj2k_encode [width height [budget_bytes]]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "htj2k_amd.h"

int main(int argc, char **argv)
{
    const int w = argc > 2 ? atoi(argv[1]) : 1920, h = argc > 2 ? atoi(argv[2]) : 1080;
    htj2k_enc_ctx *enc = NULL;
    htj2k_ctx *dec = NULL;
    htj2k_opts o;
    htj2k_enc_opts eo;
    htj2k_frame in, back;
    htj2k_info info;
    const long long budget = argc > 3 ? atoll(argv[3]) : 0;
    size_t cap, len = 0;
    uint8_t *src, *cs, *dst;
    int x, y, r;

    if (w < 1 || h < 1 || w > 32768 || h > 32768)
        return 2;
    src = malloc((size_t)w * h * 3);
    dst = malloc((size_t)w * h * 3);
    for (y = 0; y < h; y++)
        for (x = 0; x < w; x++) {
            uint8_t *p = src + ((size_t)y * w + x) * 3;
            p[0] = (uint8_t)(x + y); p[1] = (uint8_t)(x * 3 ^ y); p[2] = (uint8_t)((x * y) >> 4);
        }
    htj2k_enc_opts_default(&eo);
    cap = htj2k_encode_bound(w, h, HTJ2K_PIX_RGB24, 8, &eo);
    cs = malloc(cap);
    memset(&in, 0, sizeof in);
    in.data[0] = src; in.linesize[0] = w * 3; in.width = w; in.height = h; in.pix_fmt = HTJ2K_PIX_RGB24;
    if ((r = htj2k_enc_open(0, &enc)) < 0 || (r = htj2k_encode_frame(enc, &in, 8, &eo, cs, cap, &len)) < 0) {
        fprintf(stderr, "encode failed: %d\n", r);
        return 1;
    }
    memset(&o, 0, sizeof o);
    o.req_pix_fmt = HTJ2K_PIX_RGB24;
    memset(&back, 0, sizeof back);
    back.data[0] = dst; back.linesize[0] = w * 3;
    if ((r = htj2k_open(&o, &dec)) < 0 || (r = htj2k_probe(dec, cs, (int)len, &info)) < 0 ||
        (r = htj2k_decode(dec, cs, (int)len, &back, NULL)) < 0) {
        fprintf(stderr, "decode failed: %d\n", r);
        return 1;
    }
    r = memcmp(src, dst, (size_t)w * h * 3) != 0;
    printf("%dx%d rgb24: %zu bytes (%.3f bits per pixel), %s\n", w, h, len, 8.0 * len / ((double)w * h),
           r ? "round trip FAILED" : "round trip ok");
    if (!r) {
        /* the same frame as a tile grid: tiles whose size is no multiple of 2^levels start at odd positions */
        size_t tcap, tlen = 0;
        uint8_t *tcs;
        int ntiles;
        eo.tile_w = eo.tile_h = 1000;
        ntiles = htj2k_enc_tiles(w, h, HTJ2K_PIX_RGB24, 8, &eo, NULL, 0);
        tcap = htj2k_encode_bound(w, h, HTJ2K_PIX_RGB24, 8, &eo);
        tcs = malloc(tcap ? tcap : 1);
        memset(dst, 0, (size_t)w * h * 3);
        if (ntiles < 0 || (r = htj2k_encode_frame(enc, &in, 8, &eo, tcs, tcap, &tlen)) < 0 ||
            (r = htj2k_decode(dec, tcs, (int)tlen, &back, NULL)) < 0) {
            fprintf(stderr, "tiled encode or decode failed: %d\n", ntiles < 0 ? ntiles : r);
            return 1;
        }
        r = memcmp(src, dst, (size_t)w * h * 3) != 0;
        printf("%d tiles of %dx%d: %zu bytes, %s\n", ntiles, eo.tile_w, eo.tile_h, tlen,
               r ? "tiled round trip FAILED" : "tiled round trip ok");
        free(tcs);
        eo.tile_w = eo.tile_h = 0;
    }
    if (!r && budget > 0) {
        htj2k_enc_rc rc;
        double se = 0;
        size_t i;
        eo.target_bytes = budget;
        if ((r = htj2k_encode_frame(enc, &in, 8, &eo, cs, cap, &len)) < 0) {
            fprintf(stderr, "encode under a budget of %lld bytes failed: %d\n", budget, r);
            return 1;
        }
        if ((r = htj2k_decode(dec, cs, (int)len, &back, NULL)) < 0) {
            fprintf(stderr, "decode failed: %d\n", r);
            return 1;
        }
        htj2k_enc_rc_info(enc, 0, &rc);
        for (i = 0; i < (size_t)w * h * 3; i++)
            se += ((double)src[i] - dst[i]) * ((double)src[i] - dst[i]);
        r = len > (size_t)budget;
        printf("budget %lld: %zu bytes (fill %.3f), %d HT launch(es), %d of %d blocks left out, mean squared error %.3f, %s\n",
               budget, len, (double)len / (double)budget, rc.ht_launches, rc.blocks_left_out, rc.nblocks,
               se / ((double)w * h * 3), r ? "budget EXCEEDED" : "budget kept");
    }
    htj2k_close(dec);
    htj2k_enc_close(enc);
    free(src); free(dst); free(cs);
    return r;
}
