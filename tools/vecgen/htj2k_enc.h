/* htj2k_enc.h -- test-vector factory (see htj2k_enc.c).  Test tooling only. */
#ifndef HTJ2K_ENC_H
#define HTJ2K_ENC_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct htj2k_enc_params {
    int width, height;          /* image area (Xsiz - XOsiz, Ysiz - YOsiz) */
    int x_off, y_off;           /* XOsiz, YOsiz */
    int tile_w, tile_h;         /* 0 = one tile */
    int tx_off, ty_off;         /* XTOsiz, YTOsiz */
    int ncomp;
    int depth[4], sgnd[4], dx[4], dy[4];
    int nlevels;                /* decomposition levels NL */
    int cb_w_log2, cb_h_log2;   /* 2..10, sum <= 12 */
    int transform;              /* 1 = reversible 5/3, 0 = irreversible 9/7 (COD value) */
    int mct;
    int guard_bits;             /* 0 = 2 */
    int prog_order;             /* 0 LRCP 1 RLCP 2 RPCL 3 PCRL 4 CPRL */
    int nprec;                  /* 0 = maximal precincts, else entries in prec_*_log2 (last one repeats) */
    int prec_w_log2[34], prec_h_log2[34];
    double qstep;               /* 9/7: base step size relative to the sample range */
    int expn_bias;              /* 5/3: added to every exponent (more headroom) */
    int passes;                 /* 1 cleanup; 2 +SigProp; 3 +SigProp+MagRef */
    int placeholder_sets;       /* p0: 3*p0 placeholder passes signalled before the cleanup pass */
    int cblk_style;             /* only 0x08 (vertically causal) is honoured */
    int sop, eph;
    int force_include;          /* code all-zero blocks too */
    int never_empty_packets;
    int psot_zero;              /* last tile-part: Psot = 0 */
    int rsiz;
    int cap_extra_bits;         /* OR'ed into Ccap15 bits 11..15 (test error paths) */
    const char *comment;
    int part1;                  /* 1: Part-1 (MQ-coded) blocks, no CAP marker; cblk_style then honours BYPASS 0x01,
                                 * RESET 0x02, TERMALL 0x04, VSC 0x08, SEGSYM 0x20 */
    int p1_drop_passes;         /* Part-1: leave out the last N coding passes of every block (lossy truncation) */
    int mixed;                  /* 1: MIXED stream (SPcod bits 6-7 = 3, Ccap15 bits 14-15 = 3): HT and Part-1 blocks in a
                                 * checkerboard; of cblk_style only VSC is honoured */
    int roi_shift[4];           /* per component: Maxshift region of interest (T.800 Annex H), up-shift s > 0: the magnitudes
                                 * inside a fixed pattern of blobs are coded times 2^s, every band in M_b + s planes, one RGN
                                 * segment per such component, Ccap15 bit 12 set */
    int roi_seed;               /* moves the pattern */
    int rgn_value_bias;         /* added to the SPrgn written: a stream whose signalled shift is not the coded one */
    /* per-component coding parameters (COC / QCC).  c_set[c] != 0: component c is coded with the c_*[c] values below, all
     * of them, instead of the common ones above.  COD / QCD carry component 0's parameters; every other component that
     * differs from them gets a COC and / or a QCC, whichever differs.  The component transform is applied only when the
     * first three components share one wavelet (it stays signalled otherwise); mct with unequal sizes is refused (-22).
     * HT against Part-1 is not a per-component choice here: part1 / mixed hold for the stream */
    int c_set[4];
    int c_nlevels[4], c_cb_w_log2[4], c_cb_h_log2[4], c_transform[4];
    int c_guard_bits[4];
    double c_qstep[4];
    int c_expn_bias[4];
    int c_passes[4], c_cblk_style[4];
    int c_nprec[4], c_prec_w_log2[4][34], c_prec_h_log2[4][34];
    int coc_in_tile_hdr;        /* the COC / QCC go into the first tile-part header of every tile, not the main header; an HT
                                 * stream with such segments sets Ccap15 bit 11 (heterogeneous codestream) */
    int layers;                 /* quality layers (0 = 1).  The coding passes of every block are dealt out over the layers by a
                                 * fixed function of (layer_seed, component, resolution, band, precinct, block): blocks first
                                 * included in a later layer, layers a block skips, empty packets.  Cuts fall between passes; inside
                                 * a Part-1 codeword segment the bytes are cut at a position from the seed */
    int layer_seed;
} htj2k_enc_params;

/* comps[c]: int32 samples of component c, row-major, ceil(X1/dx)-ceil(X0/dx) wide.
 * params_size: sizeof the caller's htj2k_enc_params; fields behind it count as zero.
 * Returns 0 and a malloc'ed codestream (free with htj2k_enc_free), or <0:
 * -4 = a band needs more magnitude bits than M_b (raise guard_bits / expn_bias);
 * -6 = roi_shift: a magnitude is 2^s or more (not a Maxshift stream); -7 = roi_shift: M_b + s > 30 in some band. */
int  htj2k_encode_sized(const htj2k_enc_params *P, size_t params_size, const int32_t *const comps[4], uint8_t **out, size_t *out_len);
/* as htj2k_encode_sized() with the block that ended with `mixed`: callers built before roi_shift was appended */
int  htj2k_encode(const htj2k_enc_params *P, const int32_t *const comps[4], uint8_t **out, size_t *out_len);
void htj2k_enc_free(uint8_t *p);
/* what the last htj2k_encode_sized() of this thread did with its layers: counters, indexed by HTJ2K_LS_* */
enum { HTJ2K_LS_BLOCKS, HTJ2K_LS_FIRST_LATER, HTJ2K_LS_MULTI_PACKET, HTJ2K_LS_PACKETS, HTJ2K_LS_EMPTY_PACKETS, HTJ2K_LS_SKIP_RESUME,
       HTJ2K_LS_NOT_INCLUDED_BIT, HTJ2K_LS_HT_PLACEHOLDERS_ALONE, HTJ2K_LS_HT_CLEANUP_ALONE, HTJ2K_LS_HT_CUP_SP_THEN_MR,
       HTJ2K_LS_HT_CUP_THEN_SP_MR, HTJ2K_LS_HT_THREE_LAYERS, HTJ2K_LS_BYPASS_IN_TEN, HTJ2K_LS_BYPASS_IN_RAW_PAIR,
       HTJ2K_LS_CUT_IN_SEGMENT, HTJ2K_LS_COUNT };
void htj2k_enc_layer_stats(int out[HTJ2K_LS_COUNT]);
int  htj2k_encode_block(const int32_t *vals, int w, int h, int passes, int causal,
                        uint8_t **out, int *lcup, int *lref, int *max_U);
int  htj2k_encode_block_p1(const int32_t *vals, int w, int h, int band, int style, int drop_passes,
                           uint8_t **out, int *kbits, int *npasses, int *nseg, int *seglen, int *segpasses);
#ifdef __cplusplus
}
#endif
#endif
