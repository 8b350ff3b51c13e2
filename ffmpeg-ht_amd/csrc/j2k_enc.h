/*
 * j2k_enc.h -- internals of the HTJ2K encoder (not installed): what the host writer
 * (j2k_enc.c) and the device layer (htj2k_encode.hip) share.
 *
 * A frame is described once on the host (EncFrame): component sizes, band exponents, the tiles
 * and the code-blocks tile by tile in packet order, with their rectangles in the component's
 * coefficient plane (every tile-component's Mallat layout, DESIGN.md section 2, in its own
 * rectangle of the plane).  The geometry is the decoder's own
 * (j2k_tier2.c), read off a main header written for the frame.  After the blocks are coded,
 * enc_write() lays out the codestream as a list of pieces: literal header bytes, or the bytes
 * of one block.
 */
#ifndef J2K_ENC_H
#define J2K_ENC_H

#include <stddef.h>
#include <stdint.h>
#include "../../include/htj2k_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ENC_MAX_BANDS (3 * 32 + 1)

typedef htj2k_enc_block EncBlock;

typedef struct EncPB {              /* the blocks of one band of one (maximal) precinct */
    int32_t blk0, ncw, nch;
} EncPB;

typedef struct EncPacket {          /* LRCP: resolution-major, then component */
    int32_t pb0, npb;
} EncPacket;

typedef struct EncTile {            /* one tile: its blocks and packets in the frame's tables, its tile-components */
    htj2k_enc_tile t;
    int32_t pkt0, npkt;
} EncTile;

typedef struct EncFrame {
    int w, h, pix_fmt, bits, ncomp, nl, cbw, cbh, mct, guard_opt;
    int shift;                      /* precision - cbps of the layout: low bits the encoder ignores */
    int planar, step, bytes;        /* layout: planar, samples per pixel (packed), bytes per sample */
    int cw[4], ch[4], dx[4], dy[4];
    int irrev;                      /* 9/7 + ICT + scalar-expounded quantisation (htj2k_enc_opts.irreversible) */
    uint8_t expn[4][ENC_MAX_BANDS];
    uint16_t mant[4][ENC_MAX_BANDS];   /* 9/7: mantissa of each band's step (0 for 5/3) */
    float fstep[4][ENC_MAX_BANDS];  /* 9/7: the decoder's step of each band (BandGeom.fstep), what the quantiser divides by */
    double wgt[4][ENC_MAX_BANDS];   /* rate control: squared error of the output pixels per unit of squared error of the
                                     * band's quantisation index (step x synthesis gain x inverse MCT column norm, squared) */
    int64_t target;                 /* htj2k_enc_opts.target_bytes */
    double quality;                 /* htj2k_enc_opts.target_psnr */
    int64_t group;                  /* htj2k_enc_opts.group_bytes */
    int passes;                     /* htj2k_enc_opts.ht_passes, 0 resolved: the most passes a block gets, 1 .. 3 */
    int qgiven;                     /* expn, mant and guard_opt were given (enc_frame_init_q), not derived from bits / qstep */
    int tw, th, ntx, nty, ntiles;   /* XTsiz, YTsiz (htj2k_enc_opts.tile_w / tile_h, 0 resolved) and the tile grid */
    int nblk, npb, npkt;            /* over all tiles, tile-major */
    EncTile *tile;
    EncBlock *blk;
    EncPB *pb;
    EncPacket *pkt;
} EncFrame;

/* one part of an output codestream: `len` literal bytes at `src` of the literal buffer, or (block >= 0) the first
 * `len` bytes of that block's code */
typedef struct EncPiece {
    uint64_t dst;
    uint32_t src, len;
    int32_t  block;
    int32_t  pad;
} EncPiece;

typedef struct EncOut {
    uint8_t *lit; size_t nlit, lit_cap;
    EncPiece *pc; size_t npc, pc_cap;
    uint64_t size;
    int oom;
} EncOut;

typedef void (*enc_log_fn)(void *opaque, int level, const char *msg);

void enc_opts_resolve(const htj2k_enc_opts *in, htj2k_enc_opts *out);
/* validates the scope and lays out the frame; < 0: HTJ2K_ERR_* */
int  enc_frame_init(EncFrame *f, int w, int h, int pix_fmt, int bits, const htj2k_enc_opts *opts, enc_log_fn log, void *opaque);
/* the same with the quantisation given (q != NULL): its exponents, mantissas (9/7) and guard bits instead of
 * depth + gain (+ 1) and the qstep ladder */
int  enc_frame_init_q(EncFrame *f, int w, int h, int pix_fmt, int bits, const htj2k_enc_opts *opts, const htj2k_enc_quant *q,
                      enc_log_fn log, void *opaque);
void enc_frame_free(EncFrame *f);
/* rate control and constant quality: the weight of block b's band (f->wgt; frames with a budget or a PSNR target),
 * and the step of its band (1 for 5/3) */
double enc_block_weight(const EncFrame *f, const EncBlock *b);
/* the weights of a frame laid out without a budget (the transcoder's, when its call names one); < 0: HTJ2K_ERR_* */
int    enc_rc_weights(EncFrame *f);
float  enc_block_step(const EncFrame *f, const EncBlock *b);
/* worst-case bytes of the frame's codestream (htj2k_encode_bound) */
size_t enc_frame_bound(const EncFrame *f);
/* the guard bits of the frame from its blocks' largest U (max_u[i] of block i; <= 0 for a block left out) and the
 * planes they were coded from (NULL: all 0): M_b must hold max_u[i] + planes[i] */
int  enc_guard_bits(const EncFrame *f, const int *max_u, const int *planes, enc_log_fn log, void *opaque);
/* codestream of the frame: lcup[i] = 0 leaves block i out; planes[i] (NULL: all 0) is the bit-plane block i's cleanup
 * pass starts at (zbp = M_b - 1 - planes[i]); npasses[i] (NULL: all 1) its passes, of which those after the first are
 * the lref[i] bytes behind the cleanup segment.  Appends pieces to `o`, at o->size onwards */
int  enc_write(const EncFrame *f, int guard, const int *lcup, const int *lref, const int *npasses, const int *planes, EncOut *o);
/* bytes of the frame's smallest stream: headers and empty packets, every block left out; < 0: HTJ2K_ERR_* */
int64_t enc_min_size(const EncFrame *f);
void enc_out_free(EncOut *o);
/* worst-case bytes of block i's cleanup segment (any int32 index of magnitude below 2^31, i.e. M_b up to 31) */
size_t enc_block_bound(int w, int h);
/* and of its refinement segment (SigProp + MagRef) */
size_t enc_refine_bound(int w, int h);
/* CxtVLC encode table: entry [table][ctx][rho][eps] = valid << 15 | ek << 11 | len << 8 | cwd */
void enc_cxtvlc_table(uint16_t tab[2 * 8 * 16 * 16]);

/* rate control's last resort (htj2k_encode.hip): which coded blocks are left out when a stream is still `excess` bytes
 * beyond its limit.  A candidate is a coded block, the bytes leaving it out saves, and its gain: the weighted
 * distortion that adds per byte saved.  The least gain goes first; among equals the smaller block index */
typedef struct EncDrop {
    double  gain;
    int32_t block, bytes;
} EncDrop;
/* the call with next = 0 puts e[0 .. n) into that order.  Every call takes entries from e[next] on while the bytes
 * they save are below `excess`; -> the new next, *saved the bytes.  The caller measures again and comes back with the
 * returned next while it is over */
size_t enc_drop_take(EncDrop *e, size_t n, size_t next, int64_t excess, int64_t *saved);


/* ------------------------------------------------------------------ transcoding (j2k_xc.c, htj2k_device.hip)
 * A parsed source (the decoder's parser and its plan; Part-1, and with ht_sources HT and MIXED) -> the encoder's frame with the source's parameters, and
 * for every block of the encoder's layout what the block rule (htj2k_amd.h, "transcoding") gives it. */
struct J2kParser;
struct J2kPlan;
typedef struct XcFrame {
    EncFrame f;
    int32_t *src;                   /* [f.nblk] the source's block (plan order) at this place of the layout */
    int32_t *plane, *passes;        /* [f.nblk] the plane of the last pass (-1: no passes in the source) and the passes */
} XcFrame;
/* scope checks, layout, block matching and the rule; < 0: HTJ2K_ERR_* with a log line, and *x is empty.  ht_sources
 * (htj2k_transcode_opts, 0 / 1): streams with HT code-blocks are in scope */
int  xc_frame_init(XcFrame *x, const struct J2kParser *ps, const struct J2kPlan *plan, int ht_sources, enc_log_fn log, void *opaque);
int  xc_ht_sources_ok(int ht_sources, enc_log_fn log, void *opaque);
void xc_frame_free(XcFrame *x);

/* the decoder's side (htj2k_device.hip; not installed): one job of the decoder context holds the call's sources */
struct htj2k_ctx;
int  htj2k_xc_device_(const struct htj2k_ctx *dec);
/* parses the packets into the context's transcode job, without a pixel-format request (as htj2k_transcode_check does);
 * the parsers' log lines go to `log` as well as to the context's own; reduction_factor != 0: HTJ2K_ERR_PATCHWELCOME */
int  htj2k_xc_parse_(struct htj2k_ctx *dec, const uint8_t *const *pkts, const int *sizes, int n, htj2k_log_fn log, void *opaque);
const struct J2kParser *htj2k_xc_parser_(struct htj2k_ctx *dec, int frame);
const struct J2kPlan   *htj2k_xc_plan_(struct htj2k_ctx *dec, int frame);
/* runs the block stage with raw stores; returns the blocks that failed to decode (waits for the job's stream); *event:
 * a hipEvent_t recorded behind the stage; *ms: its device time */
int  htj2k_xc_run_(struct htj2k_ctx *dec, void **event, float *ms);
/* device address of tile-component t of frame `frame` after htj2k_xc_run_: w x h int32 indices, row stride w */
const int32_t *htj2k_xc_plane_(struct htj2k_ctx *dec, int frame, int t);
/* htj2k_encode_batch_measured: the encoder's own streams parsed with `pix_fmt` as the pixel-format request and decoded as
 * one job of the decoder context (waited for; a rejected block: HTJ2K_ERR_BUG); *job goes to htj2k_job_compare */
struct htj2k_job;
int  htj2k_meas_decode_(struct htj2k_ctx *dec, const uint8_t *const *pkts, const int *sizes, int n, int pix_fmt, struct htj2k_job **job);
int  htj2k_meas_reduction_(const struct htj2k_ctx *dec);

/* htj2k_device.hip, for htj2k_encode_tensor_curves (htj2k_encode.hip): htj2k_tensor_image_size_mix_in with the curves of
 * "tensors as frames, with curves" checked behind the mix.  Internal to the library: not exported */
__attribute__((visibility("hidden")))
int htj2k_tensor_image_size_curves_in_(int pix_fmt, int width, int height, int bits, const htj2k_tensor_spec *spec,
                                       const htj2k_tensor_mix_in *mix, const htj2k_tensor_curves_in *curves, size_t *elems, size_t *bytes);

#ifdef __cplusplus
}
#endif
#endif
