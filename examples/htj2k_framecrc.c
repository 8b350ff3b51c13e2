/*
 * htj2k_framecrc.c -- `ffmpeg -i in.j2k -f framecrc -` for a sequence of codestreams, without a frame ever leaving the
 * device: the file is cut into packets by htj2k_splitter_*, the packets go through the asynchronous pipeline
 * (htj2k_pipe_send) and every frame comes back as its checksum (htj2k_pipe_receive_hash, 4 bytes where
 * htj2k_pipe_receive copies the planes).
 *
 *   htj2k_framecrc in.j2k        back-to-back codestreams / JP2 files -> the text of the framecrc muxer on stdout:
 *                                the `#` header lines of a raw video stream, then per frame
 *                                stream, dts, pts, duration, size, 0x<Adler-32 of the packed planes>
 *                                with pts counting from 0 in a time base of 1/25
 * A packet that does not decode is reported on stderr and has no line; the exit status is then 1.
 *
 * build: make examples   (cc examples/htj2k_framecrc.c -Iinclude -Lffmpeg-ht_amd -lhtj2k_amd)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "htj2k_amd.h"

static void log_cb(void *opaque, int level, const char *msg)
{
    (void)opaque;
    if (level <= 24)                                     /* AV_LOG_WARNING and worse */
        fprintf(stderr, "[htj2k %d] %s", level, msg);
}

static long long pts;
static int failed;

/* the next frame of the pipe as one line; HTJ2K_ERR_EAGAIN: nothing in flight */
static int print_next(htj2k_pipe *pipe)
{
    htj2k_info info;
    htj2k_frame_hash h;
    const int r = htj2k_pipe_receive_hash(pipe, &info, &h);
    if (r == HTJ2K_ERR_EAGAIN) return r;
    if (r < 0) {
        fprintf(stderr, "packet %lld: error %d\n", pts + failed, r);
        failed++;
        return 0;
    }
    if (pts == 0) {                                      /* libavformat/framecrcenc.c, ff_framehash_write_header */
        printf("#software: %s\n#tb 0: 1/25\n#media_type 0: video\n#codec_id 0: rawvideo\n", htj2k_version());
        printf("#dimensions 0: %dx%d\n#sar 0: %d/%d\n", info.width, info.height, info.sar_num, info.sar_den ? info.sar_den : 1);
    }
    printf("0, %10lld, %10lld, %8d, %8llu, 0x%08x\n", pts, pts, 1, (unsigned long long)h.nbytes, (unsigned)h.adler32);
    pts++;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s in.j2k\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    htj2k_opts opts;
    memset(&opts, 0, sizeof(opts));
    opts.req_pix_fmt = HTJ2K_PIX_NONE;
    htj2k_ctx *ctx = NULL;
    htj2k_splitter *sp = NULL;
    htj2k_pipe *pipe = NULL;
    int r = htj2k_open(&opts, &ctx);
    if (r < 0) { fprintf(stderr, "htj2k_open: %d (no gfx950 device? there is no CPU fallback)\n", r); return 1; }
    htj2k_set_log(ctx, log_cb, NULL);
    if ((r = htj2k_splitter_open(&sp)) < 0 || (r = htj2k_pipe_open(ctx, 8, 3, &pipe)) < 0) { fprintf(stderr, "open: %d\n", r); return 1; }
    static uint8_t chunk[65536 + 64];
    int eof = 0;
    while (!eof) {
        int n = (int)fread(chunk, 1, 65536, f), pos = 0;
        eof = n == 0;                                        /* a final call with size 0 flushes the last frame */
        memset(chunk + n, 0, 64);
        do {
            const uint8_t *frame = NULL;
            int fsize = 0;
            int used = htj2k_splitter_parse(sp, chunk + pos, n - pos, &frame, &fsize);
            if (used < 0) { fprintf(stderr, "htj2k_splitter_parse: %d\n", used); return 1; }
            pos += used;
            if (frame && fsize > 0) {
                /* the pipe copies the packet; when `depth` batches wait, take a frame out and try again */
                while ((r = htj2k_pipe_send(pipe, frame, fsize)) == HTJ2K_ERR_EAGAIN)
                    if ((r = print_next(pipe)) < 0) break;
                if (r < 0) { fprintf(stderr, "htj2k_pipe_send: %d\n", r); return 1; }
            } else if (used == 0) {
                break;
            }
        } while (pos < n);
    }
    fclose(f);
    htj2k_pipe_flush(pipe);
    while ((r = print_next(pipe)) == 0)
        ;
    htj2k_pipe_close(pipe);
    htj2k_splitter_close(sp);
    htj2k_close(ctx);
    return failed ? 1 : 0;
}
