/*
 * htj2k_amd.h -- C ABI of the MI355X-native HTJ2K decode path.
 *
 * This is the drop-in boundary for FFmpeg's JPEG 2000 decoder plugin
 * (`const FFCodec ff_jpeg2000_decoder`, libavcodec/jpeg2000dec.c:2926-2939):
 *
 *   FFCodec.init   (jpeg2000_decode_init,  jpeg2000dec.c:2807)  -> htj2k_open()
 *   FFCodec.cb.decode (jpeg2000_decode_frame, jpeg2000dec.c:2825) -> htj2k_probe() + htj2k_decode()
 *   FFCodec.close  (none in the reference; device state persists here)  -> htj2k_close()
 *
 * Everything from `tile_codeblocks()` down (jpeg2000dec.c:2212-2299: HT block
 * decode, dequantisation, inverse DWT) plus `mct_decode()` (:2183) and
 * `write_frame_8/16()` (:2301-2364) runs as HIP kernels on gfx950.  Marker and
 * Tier-2 packet parsing (jpeg2000dec.c:197-1869) stays on the host in C.
 *
 * Plain C types only: no FFmpeg, no torch, no HIP types cross this boundary.
 * The FFmpeg-side binding a maintainer adds is shown in INTEGRATION.md.
 */
#ifndef HTJ2K_AMD_H
#define HTJ2K_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes: numerically identical to FFmpeg's AVERROR values
 *      (libavutil/error.h:41,61,64) so the glue can return them unchanged ---- */
#define HTJ2K_ERR_INVALIDDATA   (-0x41444E49) /* AVERROR_INVALIDDATA  = -MKTAG('I','N','D','A') */
#define HTJ2K_ERR_PATCHWELCOME  (-0x45574150) /* AVERROR_PATCHWELCOME = -MKTAG('P','A','W','E') */
#define HTJ2K_ERR_BUG           (-0x21475542) /* AVERROR_BUG          = -MKTAG('B','U','G','!') */
#define HTJ2K_ERR_EXTERNAL      (-0x20545845) /* AVERROR_EXTERNAL     = -MKTAG('E','X','T',' ') : HIP runtime failure */
#define HTJ2K_ERR_EAGAIN        (-11)         /* AVERROR(EAGAIN): pipeline: send more / receive first */
#define HTJ2K_ERR_ENOMEM        (-12)         /* AVERROR(ENOMEM) */
#define HTJ2K_ERR_EINVAL        (-22)         /* AVERROR(EINVAL) */
#define HTJ2K_ERR_ENOSYS        (-38)         /* AVERROR(ENOSYS): no usable gfx950 device */

/* ---- output sample layouts the reference can pick in get_siz()
 *      (jpeg2000dec.c:170-193,330-420).  The glue maps them 1:1 to AV_PIX_FMT_*. ---- */
enum htj2k_pix_fmt {
    HTJ2K_PIX_NONE = -1,
    HTJ2K_PIX_PAL8 = 0, HTJ2K_PIX_RGB24, HTJ2K_PIX_RGBA, HTJ2K_PIX_RGB48, HTJ2K_PIX_RGBA64,
    HTJ2K_PIX_GRAY8, HTJ2K_PIX_YA8, HTJ2K_PIX_GRAY16, HTJ2K_PIX_YA16,
    HTJ2K_PIX_YUV410P, HTJ2K_PIX_YUV411P, HTJ2K_PIX_YUVA420P,
    HTJ2K_PIX_YUV420P, HTJ2K_PIX_YUV422P, HTJ2K_PIX_YUVA422P,
    HTJ2K_PIX_YUV440P, HTJ2K_PIX_YUV444P, HTJ2K_PIX_YUVA444P,
    HTJ2K_PIX_YUV420P9, HTJ2K_PIX_YUV422P9, HTJ2K_PIX_YUV444P9,
    HTJ2K_PIX_YUVA420P9, HTJ2K_PIX_YUVA422P9, HTJ2K_PIX_YUVA444P9,
    HTJ2K_PIX_YUV420P10, HTJ2K_PIX_YUV422P10, HTJ2K_PIX_YUV444P10,
    HTJ2K_PIX_YUVA420P10, HTJ2K_PIX_YUVA422P10, HTJ2K_PIX_YUVA444P10,
    HTJ2K_PIX_YUV420P12, HTJ2K_PIX_YUV422P12, HTJ2K_PIX_YUV444P12,
    HTJ2K_PIX_YUV420P14, HTJ2K_PIX_YUV422P14, HTJ2K_PIX_YUV444P14,
    HTJ2K_PIX_YUV420P16, HTJ2K_PIX_YUV422P16, HTJ2K_PIX_YUV444P16,
    HTJ2K_PIX_YUVA420P16, HTJ2K_PIX_YUVA422P16, HTJ2K_PIX_YUVA444P16,
    HTJ2K_PIX_XYZ12,
    HTJ2K_PIX_NB
};

/* options: mirror of what jpeg2000dec.c reads from AVCodecContext / its AVOption
 * (jpeg2000dec.c:224,543,2488,2811-2817,2913-2917) plus device selection */
typedef struct htj2k_opts {
    int bitexact;          /* AV_CODEC_FLAG_BITEXACT: 9/7 float -> 9/7 fixed point (jpeg2000dec.c:543) */
    int reduction_factor;  /* private option "lowres" (jpeg2000dec.c:2913-2917) */
    int64_t max_pixels;    /* avctx->max_pixels (jpeg2000dec.c:224); 0 = INT_MAX */
    int strict;            /* strict_std_compliance >= FF_COMPLIANCE_STRICT (jpeg2000dec.c:2488) */
    int device_id;         /* HIP device ordinal */
    int frames_in_flight;  /* device-side pipeline depth: the `depth` of htj2k_pipe_open when that is called with depth 0
                            * (batches in flight, each on a HIP stream of its own); 0 = default (3) */
    int req_pix_fmt;       /* avctx->pix_fmt preset by the caller, or HTJ2K_PIX_NONE (jpeg2000dec.c:354) */
} htj2k_opts;

/* what jpeg2000_read_main_headers()/get_siz() write back into AVCodecContext
 * (jpeg2000dec.c:213,326,330-420,546,2867) */
typedef struct htj2k_info {
    int width, height;         /* ff_set_dimensions() arguments (jpeg2000dec.c:326) */
    int pix_fmt;               /* enum htj2k_pix_fmt */
    int bits_per_raw_sample;   /* s->precision (jpeg2000dec.c:420) */
    int profile;               /* Rsiz (jpeg2000dec.c:213) */
    int lossless;              /* FF_CODEC_PROPERTY_LOSSLESS (jpeg2000dec.c:546) */
    int sar_num, sar_den;      /* JP2 'res ' box (jpeg2000dec.c:2762-2795,2867) */
    int ncomponents;
    int is_ht;                 /* CAP marker announced Part 15 (jpeg2000dec.c:437) */
    int nplanes;               /* planes of pix_fmt */
    int plane_width[4];        /* in samples */
    int plane_height[4];
    int plane_bytes_per_sample[4]; /* bytes per sample * samples per pixel in that plane (row = this * plane_width) */
    int has_palette;           /* pal8 (JP2 pclr box): plane 1 is the palette, 256 native-endian 0xAARRGGBB entries (jpeg2000dec.c:2900-2901) */
} htj2k_info;

/* mirror of AVFrame.data/linesize (libavutil/frame.h:410,434): caller-owned system memory */
typedef struct htj2k_frame {
    uint8_t *data[4];
    int      linesize[4];
    int      width, height;    /* filled by htj2k_decode */
    int      pix_fmt;
} htj2k_frame;

/* per-call statistics (all optional) */
typedef struct htj2k_stats {
    int   n_codeblocks;        /* codeblocks dispatched to the device */
    int   n_block_errors;      /* blocks the HT decoder rejected (left zero, frame still returned;
                                  jpeg2000dec.c:2275-2278, jpeg2000htdec.c:1305-1306) */
    float ms_parse;            /* host marker + Tier-2 parse */
    float ms_h2d, ms_kernels, ms_d2h;
    float ms_ht, ms_idwt, ms_pack; /* device time per stage (hipEvent) */
} htj2k_stats;

typedef struct htj2k_ctx htj2k_ctx;

typedef void (*htj2k_log_fn)(void *opaque, int level, const char *msg);

/* FFCodec.init equivalent.  Fails with HTJ2K_ERR_ENOSYS when no gfx950 device /
 * HIP runtime is usable: there is NO CPU fallback in this library. */
int  htj2k_open(const htj2k_opts *opts, htj2k_ctx **out);
/* FFCodec.close equivalent */
void htj2k_close(htj2k_ctx *ctx);
void htj2k_set_log(htj2k_ctx *ctx, htj2k_log_fn fn, void *opaque);

/* Parse the main header only and report what get_siz()/get_cod() would set on the
 * AVCodecContext, so the glue can call ff_thread_get_buffer() before decoding
 * (jpeg2000dec.c:2864-2878).  Returns 0 or a negative HTJ2K_ERR_*. */
int  htj2k_probe(htj2k_ctx *ctx, const uint8_t *pkt, int pkt_size, htj2k_info *info);

/* One packet (= one codestream or JP2 file) -> one frame in caller memory.
 * Returns bytes consumed (>= 0) like FFCodec.cb.decode (codec_internal.h:188-192),
 * or a negative HTJ2K_ERR_*.  The packet is only read; nothing is retained. */
int  htj2k_decode(htj2k_ctx *ctx, const uint8_t *pkt, int pkt_size,
                  htj2k_frame *frame, htj2k_stats *stats);

/* ---- staged interface (what htj2k_decode does internally), used by the frame
 *      pipeline and by bench.py to time the device-resident hot path ---- */
typedef struct htj2k_job htj2k_job;  /* one parsed frame: descriptors + device buffers */

/* host: markers + Tier-2 -> per-codeblock descriptor table (no device work) */
int  htj2k_job_parse(htj2k_ctx *ctx, const uint8_t *pkt, int pkt_size, htj2k_job **job);
/* same for a batch of independent frames (the reference's frame-thread axis,
 * libavcodec/pthread_frame.c:856-889): the descriptor tables are concatenated so that each
 * device stage of the whole batch is ONE launch */
int  htj2k_job_parse_batch(htj2k_ctx *ctx, const uint8_t *const *pkts, const int *pkt_sizes, int nframes,
                           htj2k_job **job);
/* as htj2k_job_parse_batch; pinned[i] != 0 says that packet i lies in page-locked memory (htj2k_host_alloc) and stays
 * valid and unchanged until htj2k_job_upload's transfers are done (htj2k_job_wait): the H2D copy then starts from the
 * packet itself and the staging copy is left out.  pinned == NULL: none is. */
int  htj2k_job_parse_batch_ex(htj2k_ctx *ctx, const uint8_t *const *pkts, const int *pkt_sizes, int nframes,
                              const uint8_t *pinned, htj2k_job **job);
int  htj2k_job_num_frames(const htj2k_job *job);
/* host cost of the last htj2k_job_parse(_batch), averaged over its frames (each frame is timed on the thread that worked
 * on it): `ms_parse` the marker + Tier-2 parse (no code-block byte is read with "device_gather", the default), `ms_stage`
 * the copy of the packet into pinned memory that the H2D transfer starts from (for a single large packet, whose copy runs
 * on helper threads under the parse: the part of it the parse did not cover) */
int  htj2k_job_host_ms(const htj2k_job *job, float *ms_parse, float *ms_stage);
int  htj2k_job_frame_info(const htj2k_job *job, int frame, htj2k_info *info);
/* What a parse answers by itself (htj2k_job_frame_info, _info, _num_frames, _num_blocks, _num_tilecomps, _tilecomp_dims,
 * _bytes_consumed, _host_ms) is there after the parse alone.  What reads device state needs htj2k_job_upload since the
 * last parse, because until then the device holds the content before: htj2k_job_download_frame, _download, _read_plane,
 * _block_errors and _device_frame return HTJ2K_ERR_EINVAL without touching the device, htj2k_job_device_plane NULL. */
/* D2H of frame `frame` into caller planes, then waits for the job's stream; HTJ2K_ERR_EINVAL before the upload */
int  htj2k_job_download_frame(htj2k_ctx *ctx, htj2k_job *job, int frame, htj2k_frame *out);
/* per-launch device time (ms) and algorithmic bytes (2 * 4 * lh * lv per plane and level, one
 * read + one write of every sample) of the IDWT kernels of the last run; returns the number of
 * launches.  htj2k_job_idwt_hbm_bytes() gives, for the same launches, the bytes the kernel has
 * to move through HBM at least: the same figure for a plain level, 4 * lh * lv + the frame bytes
 * written for a final level that is fused with the MCT / pack stage. */
int  htj2k_job_idwt_launches(htj2k_ctx *ctx, htj2k_job *job, float *ms, double *bytes, int cap);
/* 1 when the last htj2k_job_run kept the sub-bands as 16-bit samples between the block decoder and the inverse DWT
 * (exact: reversible 5/3 jobs whose every band has M_b <= 15, rgb24 output, all levels of even geometry; knob
 * "coef16", default on).  The reference holds them as int32 (comp->i_data, jpeg2000.c:499-511). */
int  htj2k_job_coef16(const htj2k_job *job);
/* codeblocks per wavefront in the MagSgn kernel of the last HT stage run: 1 (k_ht_decode: a lane per sample column), 2
 * (k_ht_decode_pair, or k_ht_decode_multi with blocks of up to 64 columns), 4 (k_ht_decode_multi, blocks of up to 32
 * columns); 0 before the first run.  Which kernel applies is decided per job: DESIGN.md section 3.1. */
int  htj2k_job_ht_blocks_per_wave(const htj2k_job *job);
/* 0: the last run held the LL bands between the IDWT levels as int32 (as the reference, jpeg2000dwt.c:539-581);
 * 1: as 16-bit samples (knob "ll16", jobs with 16-bit sub-bands only); 2: it did, a sample of an LL band did not fit
 * -- only crafted or corrupt coefficients do that -- and htj2k_job_wait / _download ran the transform again with
 * int32 LL bands before handing out the frames.  Like the accessors above it speaks of the last run that had that stage;
 * a parse or an upload puts them all back to 0 */
int  htj2k_job_ll16(const htj2k_job *job);
/* 0: no launch of the last run's final IDWT level ran on pairs of 16-bit samples; otherwise the number of bits the LL
 * bands of the job had to fit for that (10..16; knob "idwt_pk").  The final 5/3 level of 8-bit pictures (rgb24 or 8-bit
 * planes out, 16-bit sub-bands and LL band in) is computed with packed 16-bit instructions -- lifting, inverse RCT
 * (jpeg2000dsp.c:78-91) and clip -- where the bands' M_b and the checked range of the LL band prove that no intermediate
 * leaves 16 bits; the result is the reference's int32 arithmetic exactly. */
int  htj2k_job_idwt_packed(const htj2k_job *job);
int  htj2k_job_idwt_hbm_bytes(htj2k_ctx *ctx, htj2k_job *job, double *bytes, int cap);
/* H2D: compressed codeblock bytes + descriptors (async on the job's stream) */
int  htj2k_job_upload(htj2k_ctx *ctx, htj2k_job *job);
/* device: HT block decode + dequant -> IDWT -> MCT/level shift/clip/pack (async) */
int  htj2k_job_run(htj2k_ctx *ctx, htj2k_job *job);
/* D2H into caller planes, then waits for the job's stream; HTJ2K_ERR_EINVAL before the upload */
int  htj2k_job_download(htj2k_ctx *ctx, htj2k_job *job, htj2k_frame *frame);
int  htj2k_job_wait(htj2k_ctx *ctx, htj2k_job *job);
int  htj2k_job_info(const htj2k_job *job, htj2k_info *info);
int  htj2k_job_bytes_consumed(const htj2k_job *job);
void htj2k_job_free(htj2k_ctx *ctx, htj2k_job *job);
/* debugging / parity hooks: copy a tile-component's coefficient plane (int32 or
 * float, after the last stage that ran) back to the host; htj2k_job_read_plane returns HTJ2K_ERR_EINVAL before the
 * upload (the dimensions are the parse's and answer at once) */
int  htj2k_job_num_tilecomps(const htj2k_job *job);
int  htj2k_job_tilecomp_dims(const htj2k_job *job, int tc, int *w, int *h, int *is_float);
int  htj2k_job_read_plane(htj2k_ctx *ctx, htj2k_job *job, int tc, void *dst, size_t dst_bytes);
/* run only some stages (bit 0 = HT+dequant, bit 1 = IDWT, bit 2 = MCT+pack).  Any mask may follow any run of the job's
 * content: the call gives what a run of all stages gives for the stages it names -- the IDWT runs the block stage again
 * first when the sub-bands are no longer there in the form the current knobs read -- or it returns HTJ2K_ERR_EINVAL and
 * launches nothing: masks 4 and 5 unless the last IDWT run wrote every final plane (a run of 7 or 6 with the pack stage
 * fused into the final level does not) and no block stage has run since or would write over one (DESIGN.md section 2,
 * "A job used again") */
int  htj2k_job_run_stages(htj2k_ctx *ctx, htj2k_job *job, int stage_mask);
/* device-side event timing of the last run of each stage, ms */
int  htj2k_job_stage_ms(htj2k_ctx *ctx, htj2k_job *job, float *ms_ht, float *ms_idwt, float *ms_pack);

/* ---- kernel-level entry points (unit parity tests call these through the C ABI) ---- */
/* ff_dwt_decode() (jpeg2000dwt.c:601) on a host plane: uploads, runs the IDWT
 * kernels, downloads.  border = {{x0,x1},{y0,y1}} as ff_jpeg2000_dwt_init
 * (jpeg2000dwt.c:539); type: 0 = 9/7 float, 1 = 5/3, 2 = 9/7 fixed. */
int  htj2k_idwt_plane(htj2k_ctx *ctx, void *plane, const int border[2][2],
                      int decomp_levels, int type);
/* same, device-resident and timed: runs `iters` back-to-back transforms of
 * `nplanes` identical-geometry planes and returns mean ms per iteration */
int  htj2k_idwt_bench(htj2k_ctx *ctx, int w, int h, int decomp_levels, int type,
                      int nplanes, int iters, float *ms_per_iter);
/* calibration for the roofline figures (no counterpart in the reference): GB/s, read + written, of a kernel that only
 * copies `mbytes` MB of device memory per launch (16-byte elements, grid-stride; best of three launch shapes) on the
 * context's device -- the ceiling a bandwidth-bound kernel can be held against on this particular box */
int  htj2k_copy_bench(htj2k_ctx *ctx, int mbytes, int iters, float *gbps);
/* The host-side proof behind knob "idwt_pk" (no GPU needed; tests/test_pk16_bounds.py checks it against a simulation
 * of the kernel's wrapping 16-bit arithmetic): with |LL| <= ll, |HL| <= hl, |LH| <= lh, |HH| <= hh on one level of the
 * inverse 5/3 transform (jpeg2000dwt.c:309-385), the largest magnitude any output sample can have, or -1 when some
 * intermediate sum of the horizontal or vertical lifting could leave 16 bits. */
long htj2k_pk16_lift_bound(long ll, long hl, long lh, long hh);
/* ... and for a group of `nc` components, b[c] = { ll, hl, lh, hh }, followed by the inverse RCT when `rct` != 0
 * (jpeg2000dsp.c:78-91; the two final sums of the RCT saturate and are not bounded): 1 = exact in 16 bits, 0 = not */
int  htj2k_pk16_bounds(const long (*b)[4], int nc, int rct);
/* Jpeg2000DSPContext.mct_decode[type] (jpeg2000dsp.c:43-91) on host planes */
int  htj2k_mct_planes(htj2k_ctx *ctx, void *p0, void *p1, void *p2, int csize, int type);

/* ff_jpeg2000_decode_htj2k() + dequantisation (jpeg2000htdec.c:1188, jpeg2000dec.c:2098-2181)
 * on a caller-built table of `nblocks` 32-byte codeblock descriptors (layout: struct J2kBlock
 * in ffmpeg-ht_amd/csrc/j2k_plan.h) over a byte pool, into `coef` (nsamples 32-bit samples).
 * status[i] != 0: block i was rejected and left zero.
 * Which kernels run is knob "unit_ht" (htj2k_set_int).  On its routes 3 and 4 the samples are int16_t, at index
 * plane_off (and with the stride) of `coef` read as int16_t; `coef` still has nsamples 32-bit words, every window still
 * lies inside the first nsamples elements, and the whole buffer is uploaded before the kernels run: what no block
 * writes comes back as it went in, on every route.  A table that the route's conditions exclude: HTJ2K_ERR_EINVAL,
 * `coef` and `status` untouched. */
int  htj2k_ht_blocks(htj2k_ctx *ctx, const void *blocks, int nblocks, const uint8_t *bytes, size_t nbytes,
                     void *coef, size_t nsamples, int *status);
/* decode_cblk() + dequantisation (jpeg2000dec.c:1993-2089, 2098-2181) on a table of Part-1 (MQ-coded) blocks:
 * descriptors with J2K_BLK_PART1 set, bytes laid out as in j2k_plan.h (segments back to back, 0xFF 0xFF behind
 * terminated ones and behind the last byte, J2kPart1Trailer behind that).  status[i] != 0: decode_cblk() failed
 * part-way ("bpno became invalid", "Missing needed termination"); `coef` then holds the passes decoded up to there,
 * which is what the reference dequantises (jpeg2000dec.c:2275-2290). */
int  htj2k_mq_blocks(htj2k_ctx *ctx, const void *blocks, int nblocks, const uint8_t *bytes, size_t nbytes,
                     void *coef, size_t nsamples, int *status);
/* htj2k_mq_blocks without the dequantiser (what the transcoder runs, "transcoding" below): `coef` receives the signed
 * quantiser index of every sample, +-(magnitude >> (31 - M_b)) as int32, with the half bit the reference keeps below
 * the last coded bit-plane cleared; the transform bits, the steps and the ROI shift of the descriptors are not read.
 * HTJ2K_ERR_EINVAL as htj2k_mq_blocks, and for M_b > 31 or a ROI shift. */
int  htj2k_mq_blocks_raw(htj2k_ctx *ctx, const void *blocks, int nblocks, const uint8_t *bytes, size_t nbytes,
                         void *coef, size_t nsamples, int *status);
/* htj2k_ht_blocks without the dequantiser (what the transcoder runs on HT blocks with ht_sources): `coef` receives the
 * signed quantiser index of every sample, +-(mu >> (31 - M_b)) as int32, where mu is the decoded sign-magnitude word
 * with every reconstruction half bit left out: the cleanup pass's below its plane, SigProp's and MagRef's below theirs.
 * HTJ2K_ERR_EINVAL as htj2k_ht_blocks, and for M_b > 31 or a ROI shift.  Routes 0, 1 and 2 of knob "unit_ht" (on 2 the
 * RAW instantiation of k_ht_decode_multi); 3 and 4 are refused: no job combines raw stores with 16-bit samples. */
int  htj2k_ht_blocks_raw(htj2k_ctx *ctx, const void *blocks, int nblocks, const uint8_t *bytes, size_t nbytes,
                         void *coef, size_t nsamples, int *status);
/* codeblocks the HT decoder rejected in the job's last run (they are left zero); HTJ2K_ERR_EINVAL before the upload */
int  htj2k_job_block_errors(htj2k_ctx *ctx, htj2k_job *job);
int  htj2k_job_num_blocks(const htj2k_job *job);
/* device addresses of the decoded planes of frame `frame` of the job (data[] = device pointers), for callers that
 * keep frames on the GPU; valid until the job is parsed again, and HTJ2K_ERR_EINVAL from that parse
 * until the job is uploaded */
int  htj2k_job_device_frame(htj2k_ctx *ctx, htj2k_job *job, int frame, htj2k_frame *out);
/* device address of an output plane, for callers that keep decoded frames on the GPU.  Call htj2k_job_wait first: the
 * planes of a run are final only after it (htj2k_job_device_frame waits by itself).  NULL before the upload */
void *htj2k_job_device_plane(htj2k_job *job, int plane, int *linesize);
/* tuning / test knobs:
 *   "idwt_mode"   0 generic closed-form kernels, 1 LDS tile kernel, 3 register-streaming kernel (default)
 *   "fuse_pack"   1 (default): with idwt_mode 3, a run that covers both the IDWT and the pack stage
 *                 lets the final IDWT level do the inverse MCT and write the frame
 *   "ht_mode"     1 (default) k_ht_unstuff + k_ht_vlc + k_ht_decode<true>, 0 single kernel
 *   "packet_threads" 1 (default) .. 16: a frame that is parsed on its own (htj2k_decode, jobs of one frame) has the packets
 *                 of every tile with a complete PLT packet-length list, one quality layer and no PPM / PPT read by this many
 *                 threads; the plan is the same, and any disagreement between the list and the packets sends the frame through
 *                 the sequential reader (csrc/j2k_tier2.c: read_tile_parallel)
 *   "ht_multi"    1 (default): jobs with 32-bit sub-bands whose HT blocks all are cleanup-only, at most 64 columns wide,
 *                 without ROI shift and of one transform decode 2 or 4 blocks per wavefront (k_ht_decode_multi); 0: one
 *                 block per wavefront, a lane per sample column
 *   "unit_ht"     the HT kernels of the unit entry points htj2k_ht_blocks and htj2k_ht_blocks_raw (jobs do not read it):
 *                 0 (default) a fixed plain choice: k_ht_vlc, one block per wave in the un-stuffing kernel, k_ht_decode<true>
 *                   with 32-bit stores (the single kernel with "ht_mode" 0)
 *                 1 what a job that holds exactly these blocks launches with 32-bit sub-bands and "ht_multi" 0: k_ht_vlc2
 *                   when no block is wider than 64 columns, 4 or 2 blocks per wave in the un-stuffing kernel by the widest
 *                   block (HTJ2K_UNSTUFF_G still overrides), k_ht_decode<true>; the single kernel with "ht_mode" 0
 *                 2 the same in front of k_ht_decode_multi, 4 blocks per wave when none is wider than 32 columns, else 2
 *                 3 k_ht_decode_pair with 16-bit stores        4 k_ht_decode<true> with 16-bit stores
 *                 Routes 2 to 4 take the tables a job may put on them and refuse every other with HTJ2K_ERR_EINVAL, as
 *                 they do with "ht_mode" 0.  2: all blocks at most 64 columns wide, without ROI shift, of one transform,
 *                 the wave's MagSgn bits within HTJ2K_MULTI_LDS, blocks with SigProp / MagRef passes at most 64 rows high
 *                 (their LDS at most 24 KiB).  4: all blocks at most 64 columns wide, M_b <= 15, no ROI shift, reversible
 *                 5/3 with i_step 32768, the cleanup pass only behind the placeholder passes.  3: as 4, and even widths,
 *                 strides and plane offsets.  Other values: HTJ2K_ERR_EINVAL from htj2k_set_int
 *   "coef16"      1 (default): jobs that qualify keep the sub-bands as 16-bit samples (htj2k_job_coef16)
 *   "ht_pair"     1 (default): such jobs decode MagSgn with k_ht_decode_pair (two blocks per wave, a lane per quad)
 *   "idwt_x3"     1 (default): jobs with 16-bit LL bands run the first three 5/3 levels of every plane as one launch, the LL
 *                 bands in between in LDS (k_idwt_stream_ll16_x3); 0: one launch per level
 *   "idwt_x2"     the last plain 5/3 level of an 8-bit RGB job runs inside the final-level launch, its output (the largest LL
 *                 band) in LDS windows instead of memory (k_idwt_stream_pack_x2; jobs with 16-bit LL bands on the packed
 *                 16-bit path, planes at the origin, rgb24 out): 0 never, 1 whenever the job qualifies, 2 (default) when that
 *                 LL band of the job takes at least "idwt_x2_min_bytes" bytes (default 20 MiB: smaller ones make their round
 *                 trip in the last-level cache); "idwt_x2_th": final-level rows per workgroup (even, default 20, lowered
 *                 until the windows fit the LDS of a workgroup)
 *   "idwt_pk"     1 (default): final 5/3 levels of 8-bit pictures on pairs of 16-bit samples where that is exact
 *                 (htj2k_job_idwt_packed); 0: 32-bit arithmetic throughout
 *   "ll16"        1 (default): such jobs also hold the LL bands between the IDWT levels as 16-bit samples, with a check
 *                 on the device and a second run with int32 LL bands should one not fit (htj2k_job_ll16)
 *   "device_gather"  1 (default): packets are uploaded as they are and the byte pool of the job is put together by
 *                 k_gather on the device from the parser's gather table; 0: the parser copies the code-block bytes
 *                 into the pool on the host
 *   "parse_threads"  host threads that parse the frames of a batch (0 = min(cores, 16))
 *   "bitexact", "reduction_factor"   as the AVCodecContext flag / the decoder's `lowres` option
 * Environment variables (experiments and tests; read by htj2k_open unless noted):
 *   HTJ2K_HT=fused|split             "ht_mode" 0 | 1
 *   HTJ2K_IDWT=generic|tile|stream   "idwt_mode" 0 | 1 | 3
 *   HTJ2K_LL16=0|1, HTJ2K_FUSE=0|1, HTJ2K_PK=0|1   "ll16", "fuse_pack", "idwt_pk"
 *   HTJ2K_MULTI_LDS=bytes            (per upload) most LDS a wave of k_ht_decode_multi may take for its blocks' MagSgn bits
 *                                    (default 12288): above it the job decodes one block per wave
 *   HTJ2K_UNSTUFF_G=1|2|4            (per launch) codeblocks per wavefront in the un-stuffing kernel (default 4 for jobs without blocks wider
 *                                    than 32 columns, else 2)
 *   HTJ2K_STRIP=rows                 (per launch) rows per wave of the streaming IDWT kernels (default 8 or 16 by launch size)
 *   HTJ2K_TW16 / HTJ2K_TW32 / HTJ2K_TWF=columns   (per launch) output columns per wave of the streaming IDWT for 16-bit LL
 *                                    bands / 32-bit LL bands / the fused final level (64 .. 244; default 224 or 244 by row length)
 *   HTJ2K_WPB=waves                  (per launch) waves per workgroup of the 16-bit streaming IDWT kernels, 1 .. 8 (default: the
 *                                    strips of a row, at most 8)
 *   HTJ2K_PK_LDS=bytes               (first launch) dynamic LDS the packed final-level kernel is launched with -- an occupancy limit,
 *                                    the kernel uses none (default: two workgroups of eight waves per CU)
 *   HTJ2K_X3_TH=rows                 (per launch) rows of the third level one workgroup of k_idwt_stream_ll16_x3 reconstructs (default 24)
 *   HTJ2K_POISON=1                   (read once per process) fresh device buffers start as 0xA5 bytes: a kernel that leaves part of
 *                                    its output unwritten cannot pass on what an earlier run left there (tests/test_idwt_strips_gpu.py
 *                                    runs its sweeps once in a child process with it; tools/gpu_random_configs.py takes it as well) */
int  htj2k_set_int(htj2k_ctx *ctx, const char *name, int value);

/* ---- measured quality: two frames compared on the device ------------------------------------------------
 * What AV_CODEC_FLAG_PSNR asks of an encoder (AVCodecContext.error[] per coded frame, handed on by
 * ff_side_data_set_encoder_stats) and what `ffmpeg -lavfi psnr` computes on the host, as exact integers from one kernel
 * (k_frame_diff, csrc/cmp_kernels.hpp): nothing is downloaded but 96 bytes of sums per pair of frames.
 * A sample is read as htj2k_encode_frame reads it, (word >> (precision - bits)) & (2^bits - 1): bits below the shift and
 * bits of the word above `bits` never change a result.  Components are the layout's components, not its planes (rgb24:
 * three entries, ya8: two); sub-sampled components have their own cw x ch, with the decoder's ceilings. */
typedef struct htj2k_frame_diff {
    uint64_t sse[4];       /* per component: sum of (a - b)^2, in units of the `bits`-bit sample */
    uint64_t ndiff[4];     /* samples with a != b */
    uint64_t nsamples[4];  /* cw * ch of the component (0 for components the layout does not have) */
    uint32_t max_abs[4];   /* largest |a - b| */
    double   psnr;         /* pooled over the components' own samples: 10 log10(peak^2 N / SSE), peak = 2^bits - 1;
                            * +infinity when SSE = 0 (the definition of "constant quality" above) */
} htj2k_frame_diff;
/* a[i] against b[i] for i in 0 .. n - 1, all pairs in one launch.  The n frames share one pix_fmt (any but PAL8, whose
 * samples are indices: HTJ2K_ERR_PATCHWELCOME; XYZ12 is in scope); sizes may differ from pair to pair, the two frames
 * of a pair have one size.  a_on_device / b_on_device: the planes of that operand are device addresses and are read in
 * place; a host operand is uploaded by the call.  `linesize` may exceed the row and need not be a multiple of anything,
 * pointers need no alignment, padding is never read.  Planes whose bases and linesizes are multiples of 16 are read with
 * 16-byte loads; any other plane gives the same sums on a narrower path.
 * HTJ2K_ERR_EINVAL, nothing launched: a missing argument, n < 1, bits < 1 or above the layout's depth, frames of a pair
 * that differ in size or layout, a missing plane, a negative or too short linesize.  The arguments are checked before
 * the context; a NULL context with valid arguments answers HTJ2K_ERR_ENOSYS. */
int  htj2k_compare_frames(htj2k_ctx *ctx, const htj2k_frame *a, int a_on_device,
                          const htj2k_frame *b, int b_on_device, int n, int bits, htj2k_frame_diff *out);
/* device ms of the last comparison launch(es) on this context, of either kind: k_frame_diff (htj2k_compare_frames,
 * htj2k_job_compare) or k_frame_ssim (htj2k_compare_frames_ssim, htj2k_job_compare_ssim); 0 after a call that had
 * nothing to launch */
int  htj2k_compare_ms(htj2k_ctx *ctx, float *ms);
/* every frame of the job's last run against ref[0 .. nframes - 1], on the device, nothing downloaded; bits 0: the job's
 * bits_per_raw_sample.  Waits for the job first (as htj2k_job_device_frame does).  HTJ2K_ERR_EINVAL as above, and for a
 * job whose last run did not write its frames (a run without the pack stage: htj2k_job_run_stages with a mask that
 * lacks bit 2).  A frame of the job without a plan gets nsamples all 0 and psnr NaN; the call still answers for the
 * others. */
int  htj2k_job_compare(htj2k_ctx *ctx, htj2k_job *job, const htj2k_frame *ref, int ref_on_device, int bits,
                       htj2k_frame_diff *out);

/* ---- measured quality: structural similarity ------------------------------------------------------------
 * What `ffmpeg -lavfi ssim` computes on the host (libavfilter/vf_ssim.c: ssim_4x4xn, ssim_end1 / ssim_end1x,
 * ssim_plane), per component of the layout and from one kernel (k_frame_ssim, csrc/cmp_kernels.hpp), restated so that
 * the result is an integer: samples, components and operands are those of htj2k_compare_frames.
 *   blocks     bw = cw >> 2, bh = ch >> 2; samples beyond 4 bw columns or 4 bh rows are not read.  Every 4x4 block has
 *              s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b
 *   windows    the 2x2 blocks at block (i, j), 0 <= i < bw - 1, 0 <= j < bh - 1: 8x8 samples at stride 4, their sums
 *              the sums of the four blocks; nwin = (bw - 1)(bh - 1), 0 where cw < 8 or ch < 8
 *   constants  peak = 2^bits - 1, c1 = (64 peak^2 + 5000) / 10000, c2 = (36288 peak^2 + 5000) / 10000, floor
 *              divisions: 416 and 235963 at 8 bits, vf_ssim.c's values
 *   a window   vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2, A = 2 s1 s2 + c1, B = 2 covar + c2,
 *              C = s1^2 + s2^2 + c1, D = vars + c2: int64, below 2^46, exact as doubles; v = (A * B) / (C * D) in
 *              IEEE doubles, three operations, no contraction
 *   result     q32 = sum over the windows of rint(v * 2^32) (ties to even) as int64: an integer sum, so it does not
 *              depend on the order of the windows and repeats; ssim = q32 / 2^32 / nwin
 *   all        sum_c ssim_c cw_c ch_c / sum_c cw_c ch_c over the components that have windows: vf_ssim's "All"
 * Below 4 bits c1 is 0 and an all-zero window would be 0 / 0: such calls are refused. */
typedef struct htj2k_frame_ssim {
    int64_t  q32[4];    /* per component: sum over its windows of rint(v * 2^32) */
    uint64_t nwin[4];   /* windows of the component; 0: none (cw < 8 or ch < 8, or the layout lacks it) */
    double   ssim[4];   /* q32 / 2^32 / nwin; NaN where nwin = 0 */
    double   all;       /* weighted by cw * ch over the components that have windows; NaN when none has */
} htj2k_frame_ssim;
/* htj2k_compare_frames with that figure: the same arguments, operands, refusals and their order, and bits < 4 is
 * HTJ2K_ERR_EINVAL as well (PAL8 is still HTJ2K_ERR_PATCHWELCOME first).  A pair none of whose components has a window
 * is valid and launches nothing.  Knob "ssim_rows" (htj2k_set_int): block rows of windows a wave walks before the next
 * strip begins, 1 .. 256, 0 (default) the measured choice, anything else HTJ2K_ERR_EINVAL; results never depend on
 * it (tests put strip seams inside small frames with it). */
int  htj2k_compare_frames_ssim(htj2k_ctx *ctx, const htj2k_frame *a, int a_on_device,
                               const htj2k_frame *b, int b_on_device, int n, int bits, htj2k_frame_ssim *out);
/* htj2k_job_compare with that figure: a frame of the job without a plan gets nwin all 0 and NaNs */
int  htj2k_job_compare_ssim(htj2k_ctx *ctx, htj2k_job *job, const htj2k_frame *ref, int ref_on_device, int bits,
                            htj2k_frame_ssim *out);

/* ---- frame checksums: framecrc without a download ---------------------------------------------------------
 * What one line of `ffmpeg -f framecrc` prints for a raw video frame, what FATE states a decoder's output in and what
 * tests/golden/kats.json holds: Adler-32 with both halves seeded 0 (av_adler32_update(0, ...), zlib.adler32(bytes, 0))
 * over the bytes av_image_copy_to_buffer(..., align 1) would write, from one kernel (k_frame_adler,
 * csrc/cmp_kernels.hpp): nothing is downloaded but 64 bytes of sums per frame.
 *   bytes      the planes in order, each plane_height rows of exactly plane_width * plane_bytes_per_sample bytes
 *              (htj2k_info); `linesize` padding is never read.  PAL8 is plane 0 followed by the 1024 palette bytes of
 *              plane 1 as they are stored
 *   sums       with seed 0 the value is linear in the N bytes d_0 .. d_{N-1}: A = sum d_i mod 65521,
 *              B = sum (N - i) d_i mod 65521, adler32 = B << 16 | A.  Integer sums: the result does not depend on the
 *              order of arrival, is exact and repeats
 *   planes     every plane is summed on its own, with weights relative to its own end: A_p, B_p.  The frame's A is
 *              sum A_p, its B is sum (B_p + A_p * (bytes after plane p)), mod 65521; plane_adler32 falls out
 * It is a checksum of bytes, not of samples: bits of a 16-bit word above the sample's depth are part of it.  That
 * differs from htj2k_compare_frames, which masks them.  Every layout is in scope, PAL8 and XYZ12 included. */
typedef struct htj2k_frame_hash {
    uint32_t adler32;          /* the frame: what one framecrc line prints */
    uint32_t plane_adler32[4]; /* each plane's bytes alone, seed 0; 0 for planes the layout lacks */
    uint64_t nbytes;           /* bytes hashed (the framecrc line's size field) */
} htj2k_frame_hash;
/* n frames of any layouts and sizes, which may differ from frame to frame, all in one launch (chunks of 65535 planes).
 * on_device: the planes are device addresses and are read in place; host planes are uploaded by the call.  Linesizes
 * and pointers as for htj2k_compare_frames: any linesize of at least the row, no alignment needed (planes whose base
 * and linesize are multiples of 16 are read with 16-byte loads, others byte by byte, with the same result).
 * HTJ2K_ERR_EINVAL, nothing launched: a missing argument, n < 1, a pix_fmt outside the enum, a size below 1, a plane
 * of 2^38 bytes or more, a missing plane, a negative or too short linesize.  The arguments are checked before the
 * context; a NULL context with valid arguments answers HTJ2K_ERR_ENOSYS.  htj2k_compare_ms reports the device time.
 * Comparisons and checksums of one context take turns (a lock): a pipe's consumer may hash while another thread
 * compares. */
int  htj2k_hash_frames(htj2k_ctx *ctx, const htj2k_frame *f, int on_device, int n, htj2k_frame_hash *out);
/* every frame of the job's last run, on the device, nothing of a frame downloaded.  Waits for the job first.
 * HTJ2K_ERR_EINVAL before the upload and the first run, and after a run that did not write the frames
 * (htj2k_job_run_stages with a mask that lacks bit 2).  A frame of the job without a plan gets nbytes 0 and zeros; the
 * call still answers for the others. */
int  htj2k_job_hash(htj2k_ctx *ctx, htj2k_job *job, htj2k_frame_hash *out);

/* ---- frames as tensors: decoded frames as float images on the device ----------------------------------------
 * What a framework wants of a decoded frame: a batch of fixed-size, normalised float images, channels first or last,
 * written by one kernel launch (k_frame_tensor / k_frame_tensor_any, csrc/tensor_kernels.hpp) from frames where they
 * are.  For frame i, channel c and output pixel (x, y) of an out_w x out_h image whose top-left corner is the source
 * pixel (ox_i, oy_i):
 *   sample     s = component c of the layout at ((ox_i + x) >> sw_c, (oy_i + y) >> sh_c); sw_c, sh_c are the layout's
 *              chroma shifts for components 1 and 2 and 0 for every other component: nearest replication of sub-sampled
 *              chroma on the decoder's ceilinged component sizes (no interpolation: that would be a filter).  The
 *              sample is read as htj2k_compare_frames reads it, (word >> (precision - bits)) & (2^bits - 1);
 *              components are the layout's in their order (rgb24: R, G, B; ya8: Y, A; yuva420p: Y, U, V, A; xyz12: X, Y, Z)
 *   value      t = (float)s * scale[c] + bias[c]: one IEEE binary32 multiplication, then one binary32 addition, each
 *              rounded to nearest even, never contracted into a fused multiply-add
 *   stored as  float32: t itself.  float16: t rounded to nearest even; it overflows to +-inf and subnormals are kept.
 *              bfloat16: t rounded to nearest even, in bits (u + 0x7FFF + ((u >> 16) & 1)) >> 16 of t's bits u
 *   layout     NCHW: element ((i * C + c) * out_h + y) * out_w + x.  NHWC: element ((i * out_h + y) * out_w + x) * C + c.
 *              The output is contiguous; C is the layout's component count
 * PAL8 is refused with HTJ2K_ERR_PATCHWELCOME (its samples are indices); XYZ12 is in scope. */
enum { HTJ2K_TENSOR_F32 = 0, HTJ2K_TENSOR_F16 = 1, HTJ2K_TENSOR_BF16 = 2 };
enum { HTJ2K_TENSOR_NCHW = 0, HTJ2K_TENSOR_NHWC = 1 };
typedef struct htj2k_tensor_spec {
    int   dtype, layout;
    int   out_w, out_h;        /* 0, 0: the frames' own size (all frames of the call then share one size) */
    float scale[4], bias[4];   /* per component; finite */
} htj2k_tensor_spec;
void   htj2k_tensor_spec_default(htj2k_tensor_spec *s);   /* F32, NCHW, 0 x 0, scale 1, bias 0 */

/* context-free: elements and bytes of ONE image of the call (either may be NULL), or the refusal the calls below would
 * give for this layout, size, bits and spec with an origin of 0, 0 */
int    htj2k_tensor_image_size(int pix_fmt, int width, int height, int bits, const htj2k_tensor_spec *spec,
                               size_t *elems, size_t *bytes);

/* n frames of one layout (sizes may differ when out_w/out_h are given) -> n images back to back at dst.
 * dst is device memory of at least n x bytes; bytes of dst beyond n x bytes and everything in front of dst are not
 * touched; dst needs its element's own alignment only (4, 2 or 2 bytes).  on_device: the planes are device addresses
 * and are read in place; host planes are uploaded by the call, as htj2k_compare_frames does.  Linesizes and base
 * pointers follow the rules of htj2k_compare_frames: any linesize of at least the row, no alignment needed, padding
 * never read.  The call returns after the images are written -- its stream is synchronised, so a consumer on any stream
 * may read dst at once; the caller must have no work queued on other streams that touches dst.  Tensor calls take turns
 * with comparisons and checksums under the context's lock; htj2k_compare_ms reports the device time.
 * HTJ2K_ERR_EINVAL, nothing launched and dst untouched, checked in this order and before the context (a NULL context
 * with valid arguments answers HTJ2K_ERR_ENOSYS): a missing argument; n < 1; a pix_fmt outside the enum (PAL8 at this
 * point: HTJ2K_ERR_PATCHWELCOME); bits < 1 or above the layout's depth; dtype or layout outside its enum; a scale or bias
 * that is not finite (only the first C entries are read); out_w and out_h not both 0 and not both >= 1; frames of
 * different layout; out_w/out_h 0 with frames of different size; a missing plane; a negative or too short linesize; a
 * negative origin; a window that leaves the frame (ox + out_w > width or oy + out_h > height); dst_bytes too small; dst
 * misaligned for its element. */
int    htj2k_frames_to_tensor(htj2k_ctx *ctx, const htj2k_frame *f, int on_device, int n, int bits,
                              const htj2k_tensor_spec *spec, const int32_t *origins /* 2 n: ox, oy; NULL: all 0 */,
                              void *dst, size_t dst_bytes);
/* every frame of the job's last run; status[i] (may be NULL): 0 written, 1 the frame has no plan and its image is
 * all-zero bits.  bits 0: the job's bits_per_raw_sample.  Waits for the job first.  HTJ2K_ERR_EINVAL as above, before
 * the upload and the first run, after a run that did not write the frames (the rules of htj2k_job_hash), and for a job
 * whose frames have different layouts. */
int    htj2k_job_to_tensor(htj2k_ctx *ctx, htj2k_job *job, int bits /* 0: the job's */, const htj2k_tensor_spec *spec,
                           const int32_t *origins, void *dst, size_t dst_bytes, int *status);
/* which kernel route the last tensor call on this context took: 0 nothing launched, 1 fast, 2 general, 3 both.  Knob
 * "tensor_path" (htj2k_set_int): 0 (default) the route is chosen per plane -- the fast one for planes without chroma
 * shift whose base and linesize are multiples of 16 and whose window starts on a 16-byte (three interleaved
 * components: 48-byte) boundary of the source row, NHWC only for interleaved layouts; 1 the general route for
 * everything; anything else HTJ2K_ERR_EINVAL.  Results never depend on it: it exists so that tests can compare the two.
 * After a resized call (below) the answer is 4: k_frame_resize, whatever the window.  Calls with a mix (further below)
 * answer 5, 6, 7 (the mix kernels' fast route, general route, both) and 8 (resized with a mix). */
int    htj2k_tensor_last_route(htj2k_ctx *ctx);

/* ---- frames as tensors, resized: windows of any size resampled to the image's size on the device ---------------
 * The plain call crops at the source's own scale; these calls resample.  Every frame i of a call has a window
 * (ox_i, oy_i, ww_i, wh_i) of its own, and every image is out_w x out_h: frames of one layout and of different sizes
 * go into one batch, and decode, random-resized-crop and normalise is one launch (k_frame_resize,
 * csrc/resize_kernels.hpp) that reads each window's rows once.  The resampling is defined in integers, so the result
 * depends neither on the order of summation nor on the kernel's shape.  Output pixel (x, y) of channel c:
 *   source     pixel (X, Y) of the window, 0 <= X < ww, 0 <= Y < wh, has the sample the plain call defines: component c at
 *              ((ox + X) >> sw_c, (oy + Y) >> sh_c), read as (word >> (precision - bits)) & (2^bits - 1).  Sub-sampled
 *              chroma is thus resampled from its nearest-replicated full-resolution image: no siting choice is made, and
 *              the identity below is exact
 *   weights    one axis at a time (the axes are separable); for x with ww and out_w, for y the same with wh and out_h.
 *              D = 2 out_w.  Source pixel X has its centre at (2X + 1) out_w, output pixel x at cx = (2x + 1) ww, both
 *              in units of 1 / D of a source pixel.
 *              HTJ2K_RESIZE_NEAREST takes the single source pixel X = cx / D (floor; torch's "nearest-exact") with the
 *              weight 2^14.
 *              HTJ2K_RESIZE_BILINEAR uses S = D: a triangle one source pixel wide, as interpolate(antialias=False).
 *              HTJ2K_RESIZE_TRIANGLE uses S = 2 max(out_w, ww): the triangle widened by the reduction factor, as
 *              interpolate(antialias=True) or PIL's bilinear.
 *              For both, a_X = S - |(2X + 1) out_w - cx| for the X in 0 .. ww - 1 where that is > 0: one contiguous run;
 *              taps outside the window are dropped.  A = sum a_X; q_X = (a_X << 14) / A (floor); the remainder
 *              2^14 - sum q_X is added to the first tap of largest a_X.  So sum q_X = 2^14 exactly and a constant picture
 *              stays constant.
 *              Scope: ww, wh, out_w, out_h <= 32768, and for HTJ2K_RESIZE_TRIANGLE ww <= 64 out_w and wh <= 64 out_h.
 *              Then a pixel has at most 129 taps per axis, a_X << 14 < 2^31 and A < 2^23 (32768 -> 512: 128 taps, A = 2^22),
 *              and 32-bit arithmetic suffices: (2X + 1) out_w and cx stay below 2^31 and are subtracted as they are;
 *              cx + S may pass 2^31 and is never formed
 *   value      acc = sum_Y qy_Y sum_X qx_X s(X, Y), an integer below 2^44; f = (float)((double)acc * 2^-28): the product
 *              is exact and the conversion is one rounding to nearest even.  Then t = f * scale[c] + bias[c] in two rounded
 *              binary32 operations, never contracted, stored and laid out exactly as htj2k_frames_to_tensor does
 *   identity   with ww = out_w and wh = out_h every filter has the single tap 2^14 and f is the sample itself: the call
 *              equals htj2k_frames_to_tensor on the same window, bit for bit
 * Out of scope: cubic and Lanczos kernels, chroma-siting-aware interpolation, rotation and flips.  A scaler that writes
 * frames is htj2k_resize_frames ("resized frames" below). */
enum { HTJ2K_RESIZE_NEAREST = 0, HTJ2K_RESIZE_BILINEAR = 1, HTJ2K_RESIZE_TRIANGLE = 2 };
/* context-free, no device: the taps of output index x of one axis -> their number; *first = the first source index;
 * q[0 .. taps) the weights (cap >= 129 always suffices).  HTJ2K_ERR_EINVAL: a missing argument, a filter outside its
 * enum, win or out < 1, x outside 0 .. out - 1, cap too small; HTJ2K_ERR_PATCHWELCOME: a size or a reduction out of
 * scope, as the calls below refuse it. */
int    htj2k_resize_weights(int win, int out, int filter, int x, int32_t *first, uint16_t *q, int cap);
/* htj2k_frames_to_tensor with a window per frame resampled to spec->out_w x out_h, which must both be >= 1.  Frames of
 * one layout may differ in size and in window.  Operands, dst, the lock, htj2k_compare_ms: as the plain call.  Refusals,
 * nothing launched and dst untouched, in the plain call's order and before the context (a NULL context with valid
 * arguments answers HTJ2K_ERR_ENOSYS), with these in their places: after dtype and layout, a filter outside its enum
 * (HTJ2K_ERR_EINVAL); out_w or out_h < 1; where the plain call checks its origins and windows: first ww or wh < 1, then a
 * negative origin, then a window that leaves its frame (ox + ww > width or oy + wh > height), each HTJ2K_ERR_EINVAL over
 * all frames before the next; then, each HTJ2K_ERR_PATCHWELCOME with a log line, out_w or out_h above 32768, and per
 * frame ww or wh above 32768 or, under HTJ2K_RESIZE_TRIANGLE, ww > 64 out_w or wh > 64 out_h; then dst_bytes and dst's
 * alignment.  Knob "resize_rows" (htj2k_set_int): the source rows a workgroup takes per step, 1 .. 16, 0 (default) the
 * library's choice (8), anything else HTJ2K_ERR_EINVAL; results never depend on it (tests put the seams of the row
 * streaming inside small frames with it).  Knob "resize_share": 1 .. 6 make 1, 2, 4, 8, 16, 32 neighbouring lanes share
 * the taps of one horizontal sum, 0 (default) lets the library choose per window from the taps and the interleaved
 * components (about 48 sample loads a lane), anything else HTJ2K_ERR_EINVAL; results never depend on it either: it is
 * there for tests and measurements. */
int    htj2k_frames_to_tensor_resized(htj2k_ctx *ctx, const htj2k_frame *f, int on_device, int n, int bits,
                                      const htj2k_tensor_spec *spec, const int32_t *windows /* 4 n: ox, oy, ww, wh; NULL: each frame whole */,
                                      int filter, void *dst, size_t dst_bytes);
/* htj2k_job_to_tensor the same way: every frame of the job's last run; a frame without a plan gets an image of zero bits
 * and status 1, and its window is checked for its sign and size only */
int    htj2k_job_to_tensor_resized(htj2k_ctx *ctx, htj2k_job *job, int bits, const htj2k_tensor_spec *spec,
                                   const int32_t *windows, int filter, void *dst, size_t dst_bytes, int *status);

/* ---- resized frames: windows of frames resampled to frames of another size, plane by plane (proxies) ------------
 * The calls above hand a resampled window to a network as floats.  These write it as a frame of the same layout, for
 * everything that takes htj2k_frames: a 4K master decoded as a job, resized and given to htj2k_encode_batch
 * (in_on_device) is a 1080p or 720p proxy, a size reduction_factor cannot reach; htj2k_compare_frames, htj2k_hash_frames
 * and the measured encodes read the result as they read any frame.  A window (ox, oy, ww, wh) of each of n source
 * frames, which share one layout and may differ in size, becomes a frame of out_w x out_h; every destination frame has
 * the sources' layout and that one size.  Every plane is resampled on its own grid, in integers (k_frame_rescale,
 * csrc/resize_kernels.hpp):
 *   geometry   plane p has the layout's chroma shifts (sw, sh): those of the layout for planes 1 and 2 of a planar
 *              layout, 0 for luma, alpha and interleaved planes.  Its source window has the origin (ox >> sw, oy >> sh) and
 *              the size pw = (ww + 2^sw - 1) >> sw, ph = (wh + 2^sh - 1) >> sh, in samples of the plane; its destination is
 *              dw = (out_w + 2^sw - 1) >> sw by dh = (out_h + 2^sh - 1) >> sh, the decoder's ceilinged sizes.  ox must be
 *              a multiple of the layout's largest 2^sw and oy of its largest 2^sh: then every plane's window lies inside
 *              the plane.  ww and wh need not be multiples of anything
 *   weights    htj2k_resize_weights(pw, dw, filter, x) for the horizontal axis and (ph, dh, filter, y) for the vertical,
 *              unchanged, under HTJ2K_RESIZE_NEAREST, HTJ2K_RESIZE_BILINEAR or HTJ2K_RESIZE_TRIANGLE.  The scope is the
 *              resized tensor call's, stated for the frame: ww, wh, out_w, out_h <= 32768, and under
 *              HTJ2K_RESIZE_TRIANGLE ww <= 64 out_w and wh <= 64 out_h.  No plane needs a refusal of its own: ww <= 64 out_w
 *              implies pw <= 64 dw, because ceil(ww / 2) <= 32 out_w <= 64 ceil(out_w / 2), and likewise
 *              ceil(ww / 4) <= 16 out_w <= 64 ceil(out_w / 4) for a shift of 2
 *   value      the source sample s(X, Y) = (word >> (precision - bits)) & (2^bits - 1), as every other call reads it;
 *              acc = sum_Y qy_Y sum_X qx_X s(X, Y), below 2^44; the output sample r = (acc + 2^27) >> 28.  The weights are
 *              non-negative and those of a sample sum to 2^28, so r <= 2^bits - 1 without a clamp, a constant picture
 *              stays constant and the peak stays the peak
 *   stored as  the word r << (precision - bits) with every other bit zero, as htj2k_tensor_to_frames stores.  Bytes of a
 *              row beyond its samples and between rows (linesize padding) are not written
 *   identity   with ww = out_w and wh = out_h every tap is 2^14 in either axis and the call is a crop of every plane,
 *              bit for bit (of the samples: bits of a word outside the sample come out zero)
 *   chroma     sub-sampled chroma is resampled at its own resolution and centre-aligned like luma: the plane is an image of
 *              its own.  This is deliberately not the resized tensor call's definition, which resamples chroma from its
 *              nearest-replicated full-size image: a frame stays sub-sampled, and each chroma sample is read once
 * PAL8 answers HTJ2K_ERR_PATCHWELCOME (indices do not interpolate); every other layout is in scope, XYZ12 included.
 * Out of scope: chroma-siting-aware interpolation, cubic and Lanczos kernels, a change of layout or depth, rotation and
 * flips.
 *
 * htj2k_resize_frames: src[0 .. n) are host frames (src_on_device 0, uploaded by the call as the other frame calls stage
 * them) or frames of device addresses; dst[0 .. n) gives device planes, linesizes, pix_fmt and out_w x out_h in width and
 * height.  Base pointers and linesizes of either side need no alignment (a two-byte sample is read or written as one word
 * where its plane's base and linesize are even, byte by byte elsewhere, with the same result).  The call returns after the
 * frames are written; it takes its turn under the context's lock with comparisons, checksums and the tensor calls, and
 * htj2k_compare_ms reports its device time.  A destination that overlaps a source is undefined and not checked.  Knobs
 * "resize_rows" and "resize_share" act as in the resized tensor calls (the share is chosen per plane from its own taps);
 * results never depend on them.  Refusals, nothing launched and nothing written, before the context (a NULL context with
 * valid arguments answers HTJ2K_ERR_ENOSYS), HTJ2K_ERR_EINVAL unless stated, in this order: a missing argument (src, dst);
 * n < 1; a pix_fmt (src[0]'s) outside the enum (PAL8 at this point: HTJ2K_ERR_PATCHWELCOME); bits < 1 or above the
 * layout's depth; a filter outside its enum; sources of unlike layout or of a size below 1, then a missing source plane,
 * then a negative or too short source linesize; destinations of a layout other than the sources', of unlike size, or of a
 * size below 1; then over all frames before the next: ww or wh < 1; a negative origin; a window that leaves its frame; an
 * origin off the chroma grid; then, each HTJ2K_ERR_PATCHWELCOME with a log line, out_w or out_h above 32768, and per frame
 * ww or wh above 32768 or, under HTJ2K_RESIZE_TRIANGLE, ww > 64 out_w or wh > 64 out_h; then a missing destination plane,
 * then a negative or too short destination linesize. */
int    htj2k_resize_frames(htj2k_ctx *ctx, const htj2k_frame *src, int src_on_device, int n, int bits,
                           const int32_t *windows /* 4 n: ox, oy, ww, wh; NULL: whole frames */, int filter,
                           const htj2k_frame *dst /* n, device planes, out_w x out_h in dst[i].width/height */);
/* the same over every frame of the job's last run, read where the job keeps them; bits 0: the job's.  A frame without a
 * plan gets zero samples and status 1 (status may be NULL), and its window is checked for its sign and size only */
int    htj2k_job_resize_frames(htj2k_ctx *ctx, htj2k_job *job, int bits, const int32_t *windows, int filter,
                               const htj2k_frame *dst, int *status);
/* context-free, no device: the planes of a width x height frame of a layout -> their number; plane_w[p] and plane_h[p]
 * the plane in pixels of the plane (chroma at its ceilinged size, an interleaved plane at the frame's), row_bytes[p] the
 * bytes of a row that hold samples -- what htj2k_info states for a decoded frame, and what a destination of
 * htj2k_resize_frames needs of every plane; PAL8's second plane is its palette, 256 x 1 of 4 bytes.  Any of the three
 * arrays may be NULL.  HTJ2K_ERR_EINVAL: a pix_fmt outside the enum, a size below 1 or beyond what a frame call takes. */
int    htj2k_frame_plane_sizes(int pix_fmt, int width, int height, int plane_w[4], int plane_h[4], int row_bytes[4]);

/* ---- frames as tensors, mixed: a colour matrix (Y'CbCr to RGB, BGR, luma, alpha dropped) inside the same launch ----
 * The calls above give a channel for every component of the layout, in the layout's order.  With a mix every output pixel
 * is one linear map of the layout's C components to K channels, applied where the samples are read: yuv422p10le or
 * yuv420p to normalised R, G, B, rgb24 to BGR or to one luma channel, rgba without its alpha.  For frame i, output pixel
 * (x, y) and channel k < K:
 *   source     f_c, c = 0 .. C - 1.  In the plain calls f_c = (float)s_c, s_c the sample htj2k_frames_to_tensor defines for
 *              component c at that pixel: the same shift and mask, the same nearest replication of sub-sampled chroma.  In
 *              the resized calls f_c is the resampled value htj2k_frames_to_tensor_resized defines,
 *              (float)((double)acc * 2^-28): resampling comes first, the mix second
 *   mix        a = f_0 * m[k][0]; then for c = 1 .. C - 1 in this order a = a + (f_c * m[k][c]); then t = a + b[k].  Every
 *              operation is one IEEE binary32 operation rounded to nearest even, never contracted.  All C terms are part
 *              of the definition, those with a zero weight included: x + (+0) turns a -0 into +0, and a weight of -0.0
 *              gives -0 products; signed zeros of the result are defined by this order
 *   no scale   with a mix spec->scale and spec->bias are not read: a per-channel normalisation is folded into m and b by
 *              whoever builds them (htj2k_tensor_mix_ycbcr does it).  There is no clamp: out-of-gamut values are stored
 *              as they come
 *   stored as  htj2k_frames_to_tensor stores t, with K in the place of C: float32 t itself, float16 rounded to nearest
 *              even with infinities and subnormals kept, bfloat16 by the integer formula; NCHW element
 *              ((i * K + k) * out_h + y) * out_w + x, NHWC element ((i * out_h + y) * out_w + x) * K + k, contiguous
 *   identity   nout = C, m the identity and b = 0 gives the bits of the same call without a mix at scale 1 and bias 0:
 *              samples are non-negative, so every sum is exact
 * Out of scope here: transfer functions (they are the calls of "frames as tensors, with curves" below: for xyz12le the
 * matrix alone is linear in the coded values); 3-D LUTs; chroma interpolation or siting (chroma stays replicated); clamping; more than four
 * channels.  The encode direction has a mix of its own: "tensors as frames, mixed" below. */
typedef struct htj2k_tensor_mix {
    int   nout;        /* K: channels of an image, 1 .. 4 */
    float m[4][4];     /* m[k][c]: weight of the layout's component c in channel k; rows < K, columns < C are read */
    float b[4];        /* added last */
} htj2k_tensor_mix;    /* 84 bytes */
/* context-free: Y'CbCr of `bits` bits -> R', G', B' (nominal 0 .. 1) times gain[k] plus offset[k]; nout 3, or 4 with `alpha`
 * (row 3 = component 3 / (2^bits - 1)).  standard: 601, 709, 2020 (Kr, Kb = 0.299, 0.114 / 0.2126, 0.0722 / 0.2627, 0.0593);
 * Kg = 1 - Kr - Kb.  Limited range: Y' = (s_Y - 16 q) / (219 q), Pb = (s_Cb - 2^(bits-1)) / (224 q) and Pr likewise, with
 * q = 2^(bits-8).  Full range: Y' = s_Y / (2^bits - 1), Pb = (s_Cb - 2^(bits-1)) / (2^bits - 1) and Pr likewise.
 * R' = Y' + 2 (1 - Kr) Pr;  B' = Y' + 2 (1 - Kb) Pb;  G' = Y' - (2 Kb (1 - Kb) / Kg) Pb - (2 Kr (1 - Kr) / Kg) Pr.
 * Every m[k][c] and b[k] is evaluated in double, with gain and offset folded in, and rounded to float once; entries the
 * map does not use are 0.  HTJ2K_ERR_EINVAL: a missing mix, an unknown standard, bits outside 8 .. 16, a gain or offset
 * that is not finite. */
int    htj2k_tensor_mix_ycbcr(htj2k_tensor_mix *mix, int standard, int full_range, int bits, int alpha,
                              const float gain[3] /* NULL: 1 */, const float offset[3] /* NULL: 0 */);
/* htj2k_tensor_image_size for a call with a mix: K x out_w x out_h elements.  mix NULL: htj2k_tensor_image_size itself */
int    htj2k_tensor_image_size_mix(int pix_fmt, int width, int height, int bits, const htj2k_tensor_spec *spec,
                                   const htj2k_tensor_mix *mix, size_t *elems, size_t *bytes);
/* The calls above with `mix` behind `spec`; mix NULL is the call above exactly (which is a one-line call of these).
 * Refusals come in the order of the call without a mix, before the context (a NULL context with valid arguments answers
 * HTJ2K_ERR_ENOSYS), with these differences: where scale and bias are checked, a mix is checked in their place -- nout
 * outside 1 .. 4, then an m[k][c] with k < K and c < C or a b[k] with k < K that is not finite, each HTJ2K_ERR_EINVAL
 * (entries that are not read may hold anything); dst_bytes and the image size count K channels.  A job frame without a
 * plan gets an image of zero bits, K channels, and status 1.
 * Kernels (csrc/mix_kernels.hpp): the plain calls are one launch of k_frame_mix / k_frame_mix_any, cut per frame so that a
 * lane holds all components of its pixels.  A frame takes the fast route when the layout is interleaved or planar with a
 * horizontal chroma shift of 0 or 1, every plane's base and linesize are multiples of 16 and ox is a multiple of the
 * kernel's pixel group (16 bytes of an interleaved plane, 48 for three components; 16 / bytes-per-sample pixels of a
 * planar layout, twice that with a horizontal shift of 1); any oy, any vertical shift, both layouts.  Everything else
 * (4:1:1, 4:1:0, other origins and alignments) takes the general route.  htj2k_tensor_last_route answers 5 (fast), 6
 * (general), 7 (both in one call); knob "tensor_path" = 1 forces the general route, and results never depend on it.
 * The resized calls run k_frame_resize as it is into a float32 NCHW scratch of the context at scale 1 and bias 0, which
 * stores f_c exactly, then k_tensor_mix from the scratch to dst, both on the call's stream under the context's lock;
 * htj2k_compare_ms reports the sum; htj2k_tensor_last_route answers 8.  The call walks its frames in chunks so that the
 * scratch stays under knob "mix_scratch" (htj2k_set_int) bytes, one frame at the least; 0 (default) is 64 MiB, the
 * implementer's choice and not a measured number; negative HTJ2K_ERR_EINVAL.  Results never depend on it: it exists so
 * that tests can put chunk seams into small calls. */
int    htj2k_frames_to_tensor_mix(htj2k_ctx *ctx, const htj2k_frame *f, int on_device, int n, int bits,
                                  const htj2k_tensor_spec *spec, const htj2k_tensor_mix *mix, const int32_t *origins,
                                  void *dst, size_t dst_bytes);
int    htj2k_job_to_tensor_mix(htj2k_ctx *ctx, htj2k_job *job, int bits, const htj2k_tensor_spec *spec,
                               const htj2k_tensor_mix *mix, const int32_t *origins, void *dst, size_t dst_bytes, int *status);
int    htj2k_frames_to_tensor_resized_mix(htj2k_ctx *ctx, const htj2k_frame *f, int on_device, int n, int bits,
                                          const htj2k_tensor_spec *spec, const htj2k_tensor_mix *mix, const int32_t *windows,
                                          int filter, void *dst, size_t dst_bytes);
int    htj2k_job_to_tensor_resized_mix(htj2k_ctx *ctx, htj2k_job *job, int bits, const htj2k_tensor_spec *spec,
                                       const htj2k_tensor_mix *mix, const int32_t *windows, int filter, void *dst,
                                       size_t dst_bytes, int *status);

/* ---- frames as tensors, with curves: a transfer curve before the mix and one after it (X'Y'Z' to RGB) ----------------
 * A digital cinema package codes X'Y'Z' at 12 bits with a 2.6 power law; RGB from it is a curve (2.6 decode to linear
 * XYZ), a matrix (XYZ to linear RGB) and a second curve (the display's or the model's encoding: sRGB, BT.709, PQ).  The
 * same two curves serve the other layouts: Y'CbCr or R'G'B' frames as linear-light tensors, PQ masters as display-referred
 * ones.  With curves a mix is required.  For frame i, output pixel (x, y) and channel k < K:
 *   source     f_c, c = 0 .. C - 1, exactly what the mix calls define: (float)s_c in the plain calls, the resampled value
 *              (float)((double)acc * 2^-28) in the resized ones.  Resampling therefore works on the coded values, before
 *              any curve; resampling in linear light is out of scope
 *   in-curve   g_c = E(f_c; in) when bit c of in_mask is set and an in-curve is given (in.n > 0), else g_c = f_c
 *   mix        a = g_0 * m[k][0]; a = a + (g_c * m[k][c]) for c = 1 .. C - 1 in this order; t = a + b[k]: the mix's own
 *              arithmetic, all C terms
 *   out-curve  v = E(t; out) when bit k of out_mask is set and an out-curve is given, else v = t
 *   normalise  e = v * gain[k] + offset[k], two rounded binary32 operations; e is stored as htj2k_frames_to_tensor_mix
 *              stores t: float32, float16 or bfloat16, NCHW or NHWC, K channels
 * A curve is n knots t[0 .. n-1], knot j at x0 + j / inv_dx.  E(x; curve) is made of binary32 operations only, each
 * rounded to nearest even and none contracted:
 *     u = (x - x0) * inv_dx                       one subtraction, one multiplication
 *     u = fminf(fmaxf(u, 0.0f), (float)(n - 1))   maxNum / minNum: a NaN becomes 0, and a -0 becomes +0
 *     i = (int)u                                  truncation; 0 <= i <= n - 1
 *     r = u - (float)i                            exact
 *     d = t[i+1] - t[i]                           with t[n] taken as t[n-1]
 *     E = t[i] + (r * d)                          one multiplication, one addition
 * What follows from that: a curve with n = 2^bits, x0 = 0 and inv_dx = 1 on a plain call is an exact table lookup of the
 * sample (r = 0, so E = t[s] + (+-0): only the sign of a zero entry can change, a -0.0 entry with d >= 0 reads +0);
 * values beyond either end of the table take the end knot; a NaN (inf - inf in the mix) takes knot 0; signed zeros follow
 * from the operations above and nothing else.  There is no other clamp.
 * Frames instead of tensors: htj2k_frames_to_tensor_curves followed by htj2k_tensor_to_frames.
 * The encode direction (RGB tensors to X'Y'Z' frames) is "tensors as frames, with curves" below.
 * Out of scope: a root of the argument before the lookup (the encode direction has one); non-uniform knots; 3-D LUTs; resampling in linear
 * light; more than 4097 knots; tables kept on the device between calls. */
#define HTJ2K_CURVE_MAX_KNOTS 4097
typedef struct htj2k_tensor_curve {
    int          n;         /* knots: 0 (no curve) or 2 .. HTJ2K_CURVE_MAX_KNOTS */
    float        x0;        /* the argument of knot 0 */
    float        inv_dx;    /* 1 / the knots' spacing, > 0 */
    const float *t;         /* n floats in host memory, read during the call; nothing is retained */
} htj2k_tensor_curve;
typedef struct htj2k_tensor_curves {
    htj2k_tensor_curve in, out;
    uint32_t in_mask;       /* bit c: component c goes through the in-curve; bits at or above C must be 0 */
    uint32_t out_mask;      /* bit k: channel k goes through the out-curve; bits at or above K must be 0 */
    float    gain[4], offset[4];    /* e = v * gain[k] + offset[k]; entries k < K are read */
} htj2k_tensor_curves;
/* context-free: t[j] = F(lo + j (hi - lo) / (n - 1)), j = 0 .. n - 1, F evaluated in double and rounded to float once.
 *   HTJ2K_CURVE_POWER         max(x, 0) ^ param (2.6: the DCI decode)
 *   HTJ2K_CURVE_SRGB_ENCODE   IEC 61966-2-1: 12.92 x up to 0.0031308, else 1.055 x^(1/2.4) - 0.055;  _DECODE its inverse,
 *                             x / 12.92 up to 0.04045
 *   HTJ2K_CURVE_BT709_ENCODE  4.5 x below 0.018, else 1.099 x^0.45 - 0.099;  _DECODE its inverse, x / 4.5 below 0.081
 *   HTJ2K_CURVE_PQ_ENCODE     SMPTE ST 2084 from x = luminance / 10000;  _DECODE its inverse
 * The argument is clamped to 0 .. 1 for all but POWER; param is read by POWER only.  HTJ2K_ERR_EINVAL: a missing table,
 * n < 2, an unknown kind, hi <= lo, a parameter or end that is not finite. */
enum { HTJ2K_CURVE_POWER = 0, HTJ2K_CURVE_SRGB_ENCODE = 1, HTJ2K_CURVE_SRGB_DECODE = 2, HTJ2K_CURVE_BT709_ENCODE = 3,
       HTJ2K_CURVE_BT709_DECODE = 4, HTJ2K_CURVE_PQ_ENCODE = 5, HTJ2K_CURVE_PQ_DECODE = 6 };
int    htj2k_tensor_curve_fill(float *t, int n, int kind, double param, double lo, double hi);
/* context-free: linear XYZ -> linear RGB of the primaries 709 (also sRGB), 2020 or HTJ2K_PRIMARIES_P3D65, white point D65
 * (0.3127, 0.3290): the inverse of the normalised primary matrix derived in double from the chromaticities, times
 * `scale`, rounded to float once; nout = 3, b = 0.  A DCI master's decoded values are XYZ * 48 / 52.37 (48 cd/m2 of a
 * peak luminance of 52.37), so the DCI normalisation is scale = 52.37 / 48.  HTJ2K_ERR_EINVAL: a missing mix, unknown
 * primaries, a scale that is not finite. */
enum { HTJ2K_PRIMARIES_P3D65 = 3 };
int    htj2k_tensor_mix_xyz(htj2k_tensor_mix *mix, int primaries, double scale);
/* The mix calls with `curves` behind `mix`; curves NULL is the mix call exactly (which is a one-line call of these), and
 * the image size is htj2k_tensor_image_size_mix's.  Refusals come in the mix call's order; where the mix has been checked
 * the curves are checked next, each HTJ2K_ERR_EINVAL, before the context (a NULL context with valid arguments answers
 * HTJ2K_ERR_ENOSYS), with nothing launched and dst untouched: (1) curves without a mix; (2) both n equal to 0; (3) an n
 * outside 0, 2 .. 4097; (4) a table pointer missing; (5) an x0 that is not finite; (6) an inv_dx that is not finite or not
 * > 0; (7) a table entry that is not finite or exceeds 2^100 in magnitude (so that d cannot overflow); (8) a bit of
 * in_mask at or above C or of out_mask at or above K; (9) a gain[k] or offset[k], k < K, that is not finite.  Entries that
 * are not read (x0, inv_dx and t of a curve with n = 0, gain and offset at or above K) may hold anything.
 * Kernels (csrc/curve_kernels.hpp): k_frame_curves and k_frame_curves_any on the mix calls' two routes (the same frames
 * qualify), k_tensor_curves behind k_frame_resize in the resized calls.  The call uploads both tables (n + 1 floats each,
 * padded to 16 bytes) on its own stream before the launch, and every workgroup stages them into LDS.
 * htj2k_tensor_last_route answers 9 (fast), 10 (general), 11 (both) and 12 (resized with curves); knobs "tensor_path" and
 * "mix_scratch" act as on the mix calls, and results depend on neither.  A launch's grid leaves every workgroup knob
 * "curves_grid" times its tables' bytes of source to read (0, the default: 4; 1 .. 4096; results do not depend on it: it
 * exists so that the factor can be measured). */
int    htj2k_frames_to_tensor_curves(htj2k_ctx *ctx, const htj2k_frame *f, int on_device, int n, int bits,
                                     const htj2k_tensor_spec *spec, const htj2k_tensor_mix *mix,
                                     const htj2k_tensor_curves *curves, const int32_t *origins, void *dst, size_t dst_bytes);
int    htj2k_job_to_tensor_curves(htj2k_ctx *ctx, htj2k_job *job, int bits, const htj2k_tensor_spec *spec,
                                  const htj2k_tensor_mix *mix, const htj2k_tensor_curves *curves, const int32_t *origins,
                                  void *dst, size_t dst_bytes, int *status);
int    htj2k_frames_to_tensor_resized_curves(htj2k_ctx *ctx, const htj2k_frame *f, int on_device, int n, int bits,
                                             const htj2k_tensor_spec *spec, const htj2k_tensor_mix *mix,
                                             const htj2k_tensor_curves *curves, const int32_t *windows, int filter, void *dst,
                                             size_t dst_bytes);
int    htj2k_job_to_tensor_resized_curves(htj2k_ctx *ctx, htj2k_job *job, int bits, const htj2k_tensor_spec *spec,
                                          const htj2k_tensor_mix *mix, const htj2k_tensor_curves *curves,
                                          const int32_t *windows, int filter, void *dst, size_t dst_bytes, int *status);

/* ---- tensors as frames: float images on the device as frames, and straight into the encoder -------------------
 * The way back in: a batch of images held as a float tensor (a model's output, a filtered or rendered frame) becomes
 * frames (htj2k_tensor_to_frames, below) or HTJ2K codestreams (htj2k_encode_tensor, with the encoder) without a packed
 * buffer built by hand.  A tensor is n images of C channels, H x W, contiguous, in device memory; C is the layout's
 * component count:
 *   NCHW       the element at ((i * C + c) * H + Y) * W + X.    NHWC: the element at ((i * H + Y) * W + X) * C + c.
 * Every image of a call has the same frame size W x H.  For frame i, component c and sample (x, y) of the component's
 * own cw_c x ch_c (the decoder's ceilinged sizes):
 *   element    e = the tensor element at (X, Y) = (x << sw_c, y << sh_c); sw_c, sh_c are the layout's chroma shifts for
 *              components 1 and 2 and 0 for every other component.  The co-sited top-left element of a chroma sample's
 *              footprint is taken, not an average (an average is a filter and belongs to a scaler): the exact right
 *              inverse of the replication of htj2k_frames_to_tensor, so frames -> tensor -> frames is the identity
 *              wherever the numbers are representable
 *   value      f = (float)e, exact for all three element types; u = f * scale[c], one binary32 multiplication, then
 *              u + bias[c], one binary32 addition, each rounded to nearest even and never contracted; r = rintf(u),
 *              ties to even
 *   sample     with peak = 2^bits - 1: s = 0 unless r > 0 (NaN, -inf, negatives, -0); s = peak where r >= peak (+inf);
 *              otherwise s = (uint)r
 *   stored as  (where a frame is written) the word s << (precision - bits), which htj2k_encode_frame reads back as s;
 *              every other bit of the word is zero.  Bytes of a row beyond the samples and between rows (linesize
 *              padding) are not written
 * scale and bias are the caller's forward constants in this direction, e.g. 255 and 0 for images in [0, 1]; they are not
 * the inverse of a to-tensor spec (a division would not invert exactly and is not offered).  htj2k_tensor_spec gives
 * dtype, layout, scale and bias; out_w and out_h must both be 0 (HTJ2K_ERR_EINVAL otherwise); htj2k_tensor_image_size
 * with a 0 x 0 spec answers the elements and bytes of one image.
 * Out of scope: any resize or window (the other direction has them: htj2k_frames_to_tensor_resized); a measured encode
 * from a tensor (htj2k_tensor_to_frames + htj2k_encode_batch_measured(in_on_device = 1) does it); tensors in host memory.
 * Channel orders other than the layout's own, a colour matrix and a chroma average are htj2k_tensor_to_frames_mix and
 * htj2k_encode_tensor_mix ("tensors as frames, mixed" below); these two calls are one-line calls of those with a NULL mix.
 *
 * htj2k_tensor_to_frames: the n images at src as the sample words of every component of dst[0 .. n) (k_tensor_frame,
 * csrc/tensor_kernels.hpp).  dst[i] gives data (device planes), linesize, width, height and pix_fmt; all n frames share
 * one layout and one size; any layout but PAL8, XYZ12 included; base pointers and linesizes need no alignment.  Nothing
 * but the bytes of samples is written.  src is only read.  The call returns after the frames are written; it takes its
 * turn under the context's lock with comparisons, checksums and the other tensor calls, and htj2k_compare_ms reports
 * its device time.  HTJ2K_ERR_EINVAL, nothing launched and nothing written, checked in this order and before the context
 * (a NULL context with valid arguments answers HTJ2K_ERR_ENOSYS): a missing argument; n < 1; a pix_fmt outside the enum
 * (PAL8 at this point: HTJ2K_ERR_PATCHWELCOME); bits < 1 or above the layout's depth; dtype or layout outside its enum;
 * a scale or bias that is not finite (only the first C entries are read); out_w / out_h not both 0; frames of different
 * layout or size, or a size below 1; a missing plane; a negative or too short linesize; src_bytes below n images; src
 * misaligned for its element (4, 2, 2 bytes). */
int    htj2k_tensor_to_frames(htj2k_ctx *ctx, const void *src, size_t src_bytes, int n, int bits,
                              const htj2k_tensor_spec *spec, const htj2k_frame *dst /* n, device planes */);

/* ---- tensors as frames, mixed: a colour matrix (RGB to Y'CbCr, BGR, alpha dropped) and a chroma filter on the way in ----
 * The calls above take a tensor whose channels are the layout's components, and a chroma sample from one element.  With a
 * mix the tensor has K channels of its own, every component is a linear map of them, and a chroma sample may be the mean of
 * its footprint, all in the same launch.  A tensor is n images of K channels, H x W, contiguous, in device memory:
 *   NCHW       the element at ((i * K + k) * H + Y) * W + X.    NHWC: the element at ((i * H + Y) * W + X) * K + k.
 * For frame i, component c and sample (x, y) of the component's own cw_c x ch_c:
 *   footprint  the elements (X, Y) with x << sw_c <= X < min((x + 1) << sw_c, W) and y << sh_c <= Y < min((y + 1) << sh_c, H):
 *              N of them, 1 .. 16; the last column and row of an odd picture are clipped.  sw_c, sh_c are the layout's
 *              chroma shifts for components 1 and 2 and 0 for every other component
 *   gather     per channel k < K, with f_k(X, Y) the element widened to binary32 (exact for all three element types):
 *              HTJ2K_CHROMA_COSITED, or N = 1: g_k = f_k(x << sw_c, y << sh_c).  HTJ2K_CHROMA_BOX and N > 1: start from the
 *              first element of the footprint in raster order (rows outer), add the others in that order, each one
 *              binary32 addition, then one binary32 multiplication by rcp_N, the binary32 nearest to 1 / N.  There is no
 *              division; powers of two give the exact mean
 *   mix        a = g_0 * m[c][0]; then for k = 1 .. K - 1 in this order a = a + (g_k * m[c][k]); then u = a + b[c].  Every
 *              operation is one IEEE binary32 operation rounded to nearest even and never contracted; all K terms belong to
 *              the definition, zero weights included (inf * 0 is NaN and ends as sample 0)
 *   sample     as the plain call: r = rintf(u); s = 0 unless r > 0; s = 2^bits - 1 where r reaches it; otherwise (uint)r.
 *              Where a frame is written the word is s << (precision - bits), every other bit zero, padding not written
 *   no scale   with a mix spec->scale and spec->bias are not read; dtype and layout are, and out_w / out_h must be 0
 *   identity   for a tensor of finite elements, nin = C, m the identity, b = 0 and HTJ2K_CHROMA_COSITED give the bytes of
 *              the plain call at scale 1 and bias 0
 * The channels are averaged first and mixed once: K sums per chroma sample, not N mixes, and the box call equals the
 * co-sited call on a float32 tensor averaged beforehand by the same rule.
 * Out of scope: siting other than these two (MPEG-2's left-centred 4:2:0, longer filters); transfer functions here (they
 * are the calls of "tensors as frames, with curves" below); more than four channels; windows or resizes in this direction; tensors in host memory. */
enum { HTJ2K_CHROMA_COSITED = 0, HTJ2K_CHROMA_BOX = 1 };
typedef struct htj2k_tensor_mix_in {
    int   nin;         /* K: channels of an image of the tensor, 1 .. 4 */
    int   chroma;      /* HTJ2K_CHROMA_* */
    float m[4][4];     /* m[c][k]: weight of tensor channel k in component c; rows < C, columns < K are read */
    float b[4];        /* added last */
} htj2k_tensor_mix_in; /* 88 bytes */
/* context-free, the inverse of htj2k_tensor_mix_ycbcr with the same arguments: tensor channel k holds
 * t_k = R'_k * gain[k] + offset[k] (R', G', B' nominally 0 .. 1) and the components are Y', Cb, Cr of `bits` bits.
 * Y' = Kr R' + Kg G' + Kb B', Pb = (B' - Y') / (2 (1 - Kb)), Pr = (R' - Y') / (2 (1 - Kr)); limited range:
 * s_Y = 16 q + 219 q Y', s_Cb = 2^(bits-1) + 224 q Pb and Cr likewise, q = 2^(bits-8); full range: s_Y = (2^bits - 1) Y',
 * s_Cb = 2^(bits-1) + (2^bits - 1) Pb.  With A the 3 x 3 map of (R', G', B') and o its constants, m[c][k] = A[c][k] / gain[k]
 * and b[c] = o_c - sum_k A[c][k] offset[k] / gain[k], evaluated in double and rounded to float once; unused entries are 0.
 * nin is 3; with `alpha` 4, and row 3 is channel 3 times 2^bits - 1.  HTJ2K_ERR_EINVAL: a missing mix, an unknown standard,
 * bits outside 8 .. 16, a gain that is zero or not finite, an offset that is not finite, a chroma outside the enum. */
int    htj2k_tensor_mix_in_rgb(htj2k_tensor_mix_in *mix, int standard, int full_range, int bits, int alpha,
                               const float gain[3] /* NULL: 1 */, const float offset[3] /* NULL: 0 */, int chroma);
/* htj2k_tensor_image_size for a call with such a mix: K x W x H elements.  mix NULL: htj2k_tensor_image_size itself */
int    htj2k_tensor_image_size_mix_in(int pix_fmt, int width, int height, int bits, const htj2k_tensor_spec *spec,
                                      const htj2k_tensor_mix_in *mix, size_t *elems, size_t *bytes);
/* htj2k_tensor_to_frames and htj2k_encode_tensor with `mix` behind `spec`; mix NULL is the plain call exactly.  Refusals
 * come in the order of the plain call, before the context (a NULL context with valid arguments answers HTJ2K_ERR_ENOSYS),
 * with two differences: where scale and bias are checked, the mix is checked in their place -- nin outside 1 .. 4, then
 * chroma outside the enum, then an m[c][k] with c < C and k < K or a b[c] with c < C that is not finite, each
 * HTJ2K_ERR_EINVAL (entries that are not read may hold anything); src_bytes and the image size count K channels.
 * htj2k_encode_tensor_mix gives, byte for byte, htj2k_encode_batch of the frames htj2k_tensor_to_frames_mix writes, for
 * every `opts`.
 * Kernels: k_tensor_frame_mix (csrc/mix_in_kernels.hpp) is output-driven as k_tensor_frame, takes any base and linesize and
 * runs under the context's lock (htj2k_compare_ms reports its device time); k_enc_unpack_tensor_mix (csrc/enc_kernels.hpp)
 * is cut by chroma footprint: a lane loads the K x N elements of one footprint once, stores the N samples of every
 * full-resolution component and one sample of each chroma component.  Both call the same two device functions for the
 * gather and the mix.  Every load is one element. */
int    htj2k_tensor_to_frames_mix(htj2k_ctx *ctx, const void *src, size_t src_bytes, int n, int bits,
                                  const htj2k_tensor_spec *spec, const htj2k_tensor_mix_in *mix,
                                  const htj2k_frame *dst /* n, device planes */);

/* ---- tensors as frames, with curves: a transfer curve before the mix and one after it (RGB to X'Y'Z') -----------------
 * The way back into a digital cinema package: an RGB tensor (sRGB, BT.709, PQ or linear light) becomes X'Y'Z' of 12 bits
 * through a curve (the source's decode to linear light), a matrix (linear RGB to XYZ) and a second curve (the 1 / 2.6
 * power law), inside the launch that reads the tensor.  The same steps serve linear-light RGB that is to become BT.709
 * Y'CbCr 4:2:2 or PQ BT.2020 Y'CbCr 4:2:0: the transfer function has to come before the matrix and the chroma rule.
 * With curves a mix is required.  The definition is "tensors as frames, mixed" with three steps added; for frame i,
 * component c and sample (x, y) of the component's own cw_c x ch_c:
 *   footprint  exactly as in the mix
 *   in-curve   on every element of the footprint, f_k(X, Y) the element widened to binary32: h_k = R(f_k; in) when bit k
 *              of in_mask is set and in.n > 0, else h_k = f_k.  Per element, before any average: a chroma sample is the
 *              mean of encoded values, as video practice has it
 *   gather     the mix's rule applied to h: co-sited, or the box sum in raster order times rcp_N
 *   mix        a = g_0 * m[c][0]; a = a + (g_k * m[c][k]) for k = 1 .. K - 1; u = a + b[c]: the mix's own arithmetic, all
 *              K terms
 *   out-curve  v = R(u; out) when bit c of out_mask is set and out.n > 0, else v = u
 *   normalise  w = v * gain[c] + offset[c], two rounded binary32 operations, never contracted
 *   sample     the existing end: r = rintf(w); s = 0 unless r > 0; s = 2^bits - 1 where r reaches it; otherwise (uint)r;
 *              the word is s << (precision - bits)
 * R(x; curve) with the curve's root r in 0 .. 3:
 *     p = x                          when r = 0
 *     p = fmaxf(x, 0.0f)             otherwise (a NaN becomes 0), then r times p = sqrtf(p), correctly rounded
 *     R = E(p; n, x0, inv_dx, t)     exactly the six-operation E of "frames as tensors, with curves"
 * so the table is indexed by the 2^r-th root of the argument: knot j stands at the argument (x0 + j / inv_dx) ^ (2^r).
 * Why a root: uniform knots with linear interpolation are the wrong tool for x^(1/2.6) and for PQ's x^0.159, whose
 * slope at 0 is infinite.  With 4097 knots uniform in x, 255 of the 4096 twelve-bit codes do not come back from their
 * linear values through the DCI encode; uniform in the fourth root (r = 2) all of them do, at 1025 knots already
 * ("Transfer curves on the way in", has the table).  sqrtf is correctly rounded in IEEE 754, so the
 * definition stays bit-exact and the kernels stay table lookups.  r = 0 is exactly the E of the other direction.
 * What follows from that: values beyond either end of the table take the end knot; a NaN takes knot 0 (through E's own
 * clamp when r = 0, through fmaxf otherwise); negatives under a root take the knot of 0.  There is no other clamp.
 * identity: an in-curve that is the two-knot table { 0, 1 } with x0 = 0 and inv_dx = 1, no out-curve, gain 1 and offset 0
 * on finite elements in 0 .. 1 give the bytes of the mix call.
 * An X'Y'Z' codestream: the encoder does not take the XYZ12 layout (htj2k_encode_bound answers 0 for it); three 4:4:4
 * components of 12 bits are what it writes for HTJ2K_PIX_RGB48LE at bits = 12 with mct = 0, whose sample words s << 4 are
 * exactly xyz12le's, and the decoder returns such a stream as xyz12le under req_pix_fmt.  htj2k_tensor_to_frames_curves
 * takes xyz12le frames as it takes any layout.
 * Out of scope: a `root` for the decode direction's curves; resizes or windows in this direction; 3-D LUTs; tables kept
 * on the device between calls; the encoder accepting the XYZ12 layout; non-uniform knots; more than 4097 knots. */
#define HTJ2K_CURVE_MAX_ROOT 3
typedef struct htj2k_tensor_curve_in {
    int          n;         /* knots: 0 (no curve) or 2 .. HTJ2K_CURVE_MAX_KNOTS */
    int          root;      /* square roots taken of the argument before the lookup, 0 .. HTJ2K_CURVE_MAX_ROOT */
    float        x0;        /* the rooted argument of knot 0 */
    float        inv_dx;    /* 1 / the knots' spacing in the rooted argument, > 0 */
    const float *t;         /* n floats in host memory, read during the call; nothing is retained */
} htj2k_tensor_curve_in;
typedef struct htj2k_tensor_curves_in {
    htj2k_tensor_curve_in in, out;
    uint32_t in_mask;       /* bit k: tensor channel k goes through the in-curve; bits at or above K must be 0 */
    uint32_t out_mask;      /* bit c: component c goes through the out-curve; bits at or above C must be 0 */
    float    gain[4], offset[4];    /* w = v * gain[c] + offset[c]; entries c < C are read */
} htj2k_tensor_curves_in;
/* context-free: htj2k_tensor_curve_fill for a curve with a root: t[j] = F(y_j ^ (2^root)), y_j = lo + j (hi - lo) / (n - 1),
 * the power by `root` squarings in double, F evaluated in double and rounded to float once.  root 0 is
 * htj2k_tensor_curve_fill itself.  The same refusals, and HTJ2K_ERR_EINVAL for a root outside 0 .. 3. */
int    htj2k_tensor_curve_fill_root(float *t, int n, int kind, double param, double lo, double hi, int root);
/* context-free: linear RGB of the primaries 709 (also sRGB), 2020 or HTJ2K_PRIMARIES_P3D65, white point D65, to linear XYZ
 * as a mix on the way in: the normalised primary matrix derived in double from the chromaticities, times `scale`, rounded
 * to float once; nin = 3, chroma co-sited, b = 0.  It is the inverse of htj2k_tensor_mix_xyz with the reciprocal scale;
 * a DCI master codes XYZ * 48 / 52.37, so the DCI scale is 48 / 52.37.  HTJ2K_ERR_EINVAL: a missing mix, unknown
 * primaries, a scale that is not finite. */
int    htj2k_tensor_mix_in_xyz(htj2k_tensor_mix_in *mix, int primaries, double scale);
/* htj2k_tensor_to_frames_mix and htj2k_encode_tensor_mix with `curves` behind `mix`; curves NULL is the mix call exactly
 * (which is a one-line call of these: the same bytes, kernels and refusals), and the image size is
 * htj2k_tensor_image_size_mix_in's.  Refusals come in the mix call's order; where the mix has been checked the curves are
 * checked next, each HTJ2K_ERR_EINVAL, before the context (a NULL context with valid arguments answers HTJ2K_ERR_ENOSYS),
 * with nothing launched and nothing written: (1) curves without a mix; (2) both n equal to 0; (3) an n outside 0,
 * 2 .. 4097; (4) a root outside 0 .. 3 on a curve with n > 0; (5) a table pointer missing; (6) an x0 that is not finite;
 * (7) an inv_dx that is not finite or not > 0; (8) a table entry that is not finite or exceeds 2^100 in magnitude; (9) a
 * bit of in_mask at or above K or of out_mask at or above C; (10) a gain[c] or offset[c], c < C, that is not finite.
 * Entries that are not read (root, x0, inv_dx and t of a curve with n = 0, gain and offset at or above C) may hold anything.
 * htj2k_encode_tensor_curves gives, byte for byte, htj2k_encode_batch of the frames htj2k_tensor_to_frames_curves
 * writes, for every `opts`.
 * Kernels (csrc/curve_in_kernels.hpp, csrc/enc_kernels.hpp): k_tensor_frame_curves is output-driven as k_tensor_frame_mix;
 * k_enc_unpack_tensor_curves keeps k_enc_unpack_tensor_mix's cut by chroma footprint and walks a frame's footprints in a
 * grid-stride loop.  Both call the same two device functions (the curve with its root; mix, out-curve, gain and offset,
 * sample).  The call uploads both tables (n + 1 floats each, padded to 16 bytes) before the launch and every workgroup
 * stages them into LDS; a grid leaves every workgroup several times its tables' bytes of tensor to read: knob
 * "curves_grid" for htj2k_tensor_to_frames_curves (default 4), HTJ2K_ENC_CURVES_GRID in the environment of htj2k_enc_open
 * for the encoder (1 .. 4096, default 2, the measured best); results depend on neither. */
int    htj2k_tensor_to_frames_curves(htj2k_ctx *ctx, const void *src, size_t src_bytes, int n, int bits,
                                     const htj2k_tensor_spec *spec, const htj2k_tensor_mix_in *mix,
                                     const htj2k_tensor_curves_in *curves, const htj2k_frame *dst /* n, device planes */);

/* Pinned (page-locked) host memory for frame planes: a D2H copy into it runs at PCIe rate (about 5x a
 * copy into pageable memory).  An integration wraps it in its buffer pool, e.g. av_buffer_create()
 * with htj2k_host_free as the free callback.  Plain pageable planes work everywhere, only slower. */
void *htj2k_host_alloc(htj2k_ctx *ctx, size_t size);
void  htj2k_host_free(htj2k_ctx *ctx, void *ptr);
/* copies `size` bytes of a device plane handed out by htj2k_pipe_receive_device / htj2k_job_device_frame to host memory
 * (a consumer that keeps frames on the GPU and wants one on the host after all); synchronous */
int   htj2k_device_to_host(htj2k_ctx *ctx, void *dst, const void *device_src, size_t size);

/* ---- asynchronous pipeline: packets in, frames out, in order (csrc/htj2k_pipe.cpp) ----
 * The throughput path for a stream of frames.  It takes the place of FFmpeg's frame threads
 * (libavcodec/pthread_frame.c:856-889: N decoder contexts, one packet each) and maps onto
 * FFCodec.cb.receive_frame: `depth` device jobs of `batch` frames are kept in flight, so that host
 * parsing (on several threads, see "parse_threads"), PCIe transfers and kernels overlap.
 *   htj2k_pipe_send     queues a copy of the packet; HTJ2K_ERR_EAGAIN when `depth` batches are
 *                       waiting to be received
 *   htj2k_pipe_flush    starts the partly filled batch (end of stream, or latency matters)
 *   htj2k_pipe_info     what the next frame will be (blocks until its batch is decoded);
 *                       HTJ2K_ERR_EAGAIN when nothing is in flight
 *   htj2k_pipe_receive  copies the next frame into the caller's planes; a packet that failed
 *                       returns its own error, the other frames of its batch are still delivered
 *   htj2k_pipe_receive_hash  the next frame's checksum instead of its planes (framecrc without a download)
 *   htj2k_pipe_receive_tensor  the next frame as a float image in the caller's device memory
 *   htj2k_pipe_receive_tensor_resized  a window of the next frame resampled to such an image
 *   htj2k_pipe_receive_tensor_mix, htj2k_pipe_receive_tensor_resized_mix  the same two through a colour matrix
 *   htj2k_pipe_receive_resized  a window of the next frame resampled to a frame in the caller's device memory
 *   htj2k_pipe_skip     drops the next frame
 * One producer/consumer thread at a time may use a pipe (like an AVCodecContext). */
typedef struct htj2k_pipe htj2k_pipe;
/* batch: 1 .. 256 frames per device job; depth: 1 .. 16 jobs in flight, 0 = htj2k_opts.frames_in_flight */
int  htj2k_pipe_open(htj2k_ctx *ctx, int batch, int depth, htj2k_pipe **pipe);
int  htj2k_pipe_send(htj2k_pipe *pipe, const uint8_t *pkt, int size);
/* as htj2k_pipe_send without the copy: `pkt` (with its 64 bytes of input padding) stays valid until
 * release(opaque) is called -- when the packet's frame has been received or skipped, or on close */
int  htj2k_pipe_send_ref(htj2k_pipe *pipe, const uint8_t *pkt, int size, void (*release)(void *opaque), void *opaque);
int  htj2k_pipe_flush(htj2k_pipe *pipe);
int  htj2k_pipe_info(htj2k_pipe *pipe, htj2k_info *info);
int  htj2k_pipe_receive(htj2k_pipe *pipe, htj2k_frame *out);
/* as htj2k_pipe_receive without the copy: `out->data[]` are the device pointers of the decoded planes; they stay
 * valid until the pipe has handed out all frames of `depth - 1` further batches.  The pipe keeps 2 depth - 1 jobs for
 * this: `depth` batches in flight and the depth - 1 most recent ones whose frames are out */
int  htj2k_pipe_receive_device(htj2k_pipe *pipe, htj2k_frame *out);
/* the same for consumers that keep frames for as long as they like (reference-counted frames: the AV_PIX_FMT_HIP
 * hand-out of glue/jpeg2000_hip_hw.c): the planes stay valid until htj2k_pipe_release_device(token) -- callable from
 * any thread, e.g. an AVBuffer free callback; a token releases its own frame, once.  Until all frames of a batch are
 * released its job is not reused; the other jobs go on (a new batch takes any free job, frames still come out in the
 * order their packets went in).  A consumer that sits on frames of 2 depth - 1 batches starves the pipe (htj2k_pipe_send
 * answers HTJ2K_ERR_EAGAIN and nothing is in flight): size `depth` for the frames the consumer holds, as
 * extra_hw_frames does for hardware decoders. */
int  htj2k_pipe_receive_device_ref(htj2k_pipe *pipe, htj2k_frame *out, uint64_t *token);
int  htj2k_pipe_release_device(htj2k_pipe *pipe, uint64_t token);
/* the next frame of the pipe as its checksum (htj2k_frame_hash above): what htj2k_pipe_receive would hand out, hashed on
 * the device; nothing of the frame is downloaded.  `info` (may be NULL) is the frame's htj2k_pipe_info.  A packet that
 * failed returns its own error and the pipe moves on, as in htj2k_pipe_receive, with the same per-packet retry of a
 * failed batch.  The slot is not a device hand-out: it becomes free as after htj2k_pipe_receive.  The frames of a
 * batch are hashed in one launch when the first of them is asked for. */
int  htj2k_pipe_receive_hash(htj2k_pipe *pipe, htj2k_info *info, htj2k_frame_hash *out);
/* the next frame of the pipe as one image at dst (htj2k_frames_to_tensor above with n = 1; bits 0: the frame's own;
 * origin NULL: 0, 0).  The job's planes are read in place: the slot is not handed out and becomes free as after
 * htj2k_pipe_receive.  `info` (may be NULL), a packet that failed and the per-packet retry of a failed batch: as
 * htj2k_pipe_receive_hash.  A refusal of the arguments consumes the frame, as every receive call's error does. */
int  htj2k_pipe_receive_tensor(htj2k_pipe *pipe, htj2k_info *info, int bits, const htj2k_tensor_spec *spec,
                               const int32_t origin[2], void *dst, size_t dst_bytes);
/* the same through htj2k_frames_to_tensor_resized with n = 1: the frame's window (ox, oy, ww, wh; NULL: the frame whole)
 * resampled to spec->out_w x out_h.  Everything else as htj2k_pipe_receive_tensor, the consumption of the frame on a
 * refusal included; the call mixes with the other receive calls. */
int  htj2k_pipe_receive_tensor_resized(htj2k_pipe *pipe, htj2k_info *info, int bits, const htj2k_tensor_spec *spec,
                                       const int32_t window[4], int filter, void *dst, size_t dst_bytes);
/* both with a colour matrix ("frames as tensors, mixed" above): the image has mix->nout channels; mix NULL: the calls above */
int  htj2k_pipe_receive_tensor_mix(htj2k_pipe *pipe, htj2k_info *info, int bits, const htj2k_tensor_spec *spec,
                                   const htj2k_tensor_mix *mix, const int32_t origin[2], void *dst, size_t dst_bytes);
int  htj2k_pipe_receive_tensor_curves(htj2k_pipe *pipe, htj2k_info *info, int bits, const htj2k_tensor_spec *spec,
                                      const htj2k_tensor_mix *mix, const htj2k_tensor_curves *curves, const int32_t origin[2],
                                      void *dst, size_t dst_bytes);     /* "frames as tensors, with curves"; curves NULL: _mix */
int  htj2k_pipe_receive_tensor_resized_curves(htj2k_pipe *pipe, htj2k_info *info, int bits, const htj2k_tensor_spec *spec,
                                              const htj2k_tensor_mix *mix, const htj2k_tensor_curves *curves,
                                              const int32_t window[4], int filter, void *dst, size_t dst_bytes);
int  htj2k_pipe_receive_tensor_resized_mix(htj2k_pipe *pipe, htj2k_info *info, int bits, const htj2k_tensor_spec *spec,
                                           const htj2k_tensor_mix *mix, const int32_t window[4], int filter, void *dst,
                                           size_t dst_bytes);
/* the next frame through htj2k_resize_frames with n = 1 ("resized frames" above): its window (NULL: the frame whole)
 * resampled plane by plane to the caller's frame dst (device planes, out_w x out_h in width and height, the frame's own
 * layout); bits 0: the frame's own.  Everything else as htj2k_pipe_receive_tensor_resized: a refusal consumes the frame, a
 * packet of a failed batch is decoded alone and returns its own error, and the call mixes with the other receive calls. */
int  htj2k_pipe_receive_resized(htj2k_pipe *pipe, htj2k_info *info, int bits, const int32_t window[4], int filter,
                                const htj2k_frame *dst);
int  htj2k_pipe_skip(htj2k_pipe *pipe);
/* Stops the workers, drops what is queued and frees the pipe -- unless frames handed out by
 * htj2k_pipe_receive_device_ref are still out: then the jobs they live in, the pipe and the context (the pipe holds a
 * reference: an htj2k_close by the caller does not free it yet) stay until the last htj2k_pipe_release_device, the only
 * call the handle is still good for.  Frames may so outlive the decoder that made them. */
void htj2k_pipe_close(htj2k_pipe *pipe);

/* ---- framing: cutting a byte stream of back-to-back frames into packets ----------------------------
 * The reference's AVCodecParser for this codec, `ff_jpeg2000_parser` (libavcodec/jpeg2000_parser.c:213-218,
 * used by av_parser_parse2() for raw .j2k / .jp2 sequences and image pipes).  No device involved.
 *   htj2k_splitter_find_end  = find_frame_end() (jpeg2000_parser.c:92-184): scans `size` more bytes and returns
 *                              the offset, relative to `buf`, of the first byte of the NEXT frame -- negative
 *                              (down to -11) when that byte arrived with an earlier call -- or
 *                              HTJ2K_SPLIT_END_NOT_FOUND.
 *   htj2k_splitter_parse     = jpeg2000_parse() + ff_combine_frame() (jpeg2000_parser.c:186-211,
 *                              parser.c:203-288): returns the number of bytes of `buf` consumed; when a frame is
 *                              complete *frame / *frame_size describe it (valid until the next call, followed by
 *                              zeroed input padding unless it points into `buf`), else they are NULL / 0.
 *                              Call with size 0 at the end of the input to flush the last frame. */
#define HTJ2K_SPLIT_END_NOT_FOUND (-100)      /* END_NOT_FOUND, libavcodec/parser.h:40 */
typedef struct htj2k_splitter htj2k_splitter;
int  htj2k_splitter_open(htj2k_splitter **sp);
int  htj2k_splitter_find_end(htj2k_splitter *sp, const uint8_t *buf, int size);
int  htj2k_splitter_parse(htj2k_splitter *sp, const uint8_t *buf, int size, const uint8_t **frame, int *frame_size);
void htj2k_splitter_close(htj2k_splitter *sp);

/* ---- MXF: JPEG 2000 picture essence out of a file held in memory ------------------------------------
 * The KLV layer of the reference's demuxer (klv_read_packet, libavformat/mxfdec.c:432-504, and the essence
 * branch of mxf_read_packet, :4034-4160); no header metadata is read.  Starting at *pos, finds the next
 * generic-container picture element that carries JPEG 2000 (SMPTE 422M: key ...0d.01.03.01.15.nn.08.nn
 * frame-wrapped, ...15.nn.09.nn clip-wrapped; libavformat/mxfenc.c:216-217) and advances *pos behind it.
 * Returns 1 with *out filled in (pointing into `buf`), 0 at the end of the buffer, < 0 on a malformed length.
 * A frame-wrapped element is one packet for htj2k_decode / htj2k_pipe_send; a clip-wrapped one holds all
 * codestreams back to back and is cut apart by htj2k_splitter_*. */
#define HTJ2K_MXF_FRAME_WRAPPED 1
#define HTJ2K_MXF_CLIP_WRAPPED  2
typedef struct htj2k_mxf_essence {
    const uint8_t *data;
    size_t   size;                /* shorter than the KLV length when the file is truncated */
    size_t   klv_offset;          /* of the element's key (AVPacket.pos) */
    uint32_t track_number;        /* key bytes 12..15: matches the track's TrackNumber (SMPTE 379M 7.3) */
    int      wrapping;
} htj2k_mxf_essence;
int  htj2k_mxf_next_essence(const uint8_t *buf, size_t size, size_t *pos, htj2k_mxf_essence *out);

/* ---- lossless HTJ2K encoding: frames in, HT codestreams out --------------------------------------------
 * The other direction of this library.  The reference's encoder (libavcodec/j2kenc.c) is Part-1 only and runs
 * on the CPU; this one writes T.814 codestreams whose every code-block is one HT cleanup pass (T.814 clause 7
 * read backwards; with htj2k_enc_opts.ht_passes also the SigProp and MagRef passes, see "refinement passes") over reversible 5/3 coefficients (T.800 F.4.8.2) and, for the RGB family, the forward RCT
 * (T.800 G.2); or, with htj2k_enc_opts.irreversible, over quantised 9/7 coefficients and the forward ICT.  Scope: one
 * tile equal to the image or a regular tile grid (htj2k_enc_opts.tile_w / tile_h; one tile-part per tile), image and
 * tile-grid origin 0, one quality layer, LRCP, maximal precincts, no SOP / EPH, unsigned components in any
 * htj2k_pix_fmt but PAL8 and XYZ12.  A tile-component is at most 32768 samples wide and high (the decoder's limit);
 * the picture may be larger when its tiles are not.  Anything else answers HTJ2K_ERR_PATCHWELCOME with a log line.
 * What the encoder writes, marker by marker, is in DESIGN.md 3.5. */
#define HTJ2K_ERR_ENOSPC        (-28)         /* AVERROR(ENOSPC): the output buffer is smaller than the codestreams;
                                               * nothing is written past `cap` (and nothing at all by a call of one
                                               * round) */

/* replaces j2kenc.c's AVOptions and the fields of AVCodecContext it reads (prediction, levels).
 *
 * Lossy coding (irreversible = 1, what j2kenc.c's prediction = dwt97 selects): the forward ICT (T.800 G.3) where mct
 * is on, the irreversible 9/7 transform (T.800 F.4.8.2, un-normalised lifting) and scalar-expounded dead-zone
 * quantisation (QCD style 2, one exponent / mantissa pair per band).  The band at level l (the LL band: l = NL) gets
 * the step d = qstep * 2^-((l - 1) / 2) in sample units of the normalised transform, signalled as
 * e = floor(log2 d), mantissa = floor((d / 2^e - 1) * 2048 + 0.5) (a mantissa of 2048 carries into e), exponent
 * bits - e.  There is no gain term and no MCT bit.  Every exponent must fall in 0 .. 31 (HTJ2K_ERR_EINVAL otherwise).
 * The quantiser divides by the step the decoder derives from that header (f_stepsize, jpeg2000.c:214-272), so the
 * two never disagree about it.  A zero tail (irreversible 0, qstep 0) means lossless 5/3, as before the fields. */
typedef struct htj2k_enc_opts {
    int levels;            /* decomposition levels NL, 0 .. 32 (default 5) */
    int cb_w_log2;         /* code-block size, 2 .. 10 each, sum <= 12 (default 6 x 6: 64 x 64) */
    int cb_h_log2;
    int mct;               /* forward RCT (ICT when irreversible) of components 0..2: -1 auto (on for the RGB family),
                            * 0 off, 1 on (RGB family only) */
    int guard_bits;        /* 0 auto: 2, or more where a block's largest exponent bound U needs it; 1 .. 7 fixed */
    int irreversible;      /* 0: reversible 5/3, lossless (default); 1: irreversible 9/7 with quantisation */
    double qstep;          /* base step of the 9/7 quantiser, finite and > 0 (default 1.0); read only when irreversible */
    int64_t target_bytes;  /* rate control: upper limit of one frame's whole codestream, SOC to EOC, in bytes; 0: off
                            * (default).  In a batch it applies to each frame on its own.  See "rate control" below */
    int tile_w, tile_h;    /* nominal tile size on the reference grid (XTsiz, YTsiz); 0 in a direction: one tile spans
                            * the image in that direction (tile_w 0, tile_h 128: strips).  Both 0 (default): one tile,
                            * the stream written before these fields.  HTJ2K_ERR_EINVAL: a negative size, more than
                            * 65535 tiles, or a grid that leaves a tile-component without samples (4:2:0 with 1 x 1
                            * tiles).  See "tiles" below */
    int ht_passes;         /* the most coding passes a code-block gets: 0 or 1 (default): the cleanup pass alone, the
                            * stream written before this field; 2: SigProp as well; 3: SigProp and MagRef.  Lossy, also
                            * over 5/3, and deterministic.  Anything else: HTJ2K_ERR_EINVAL and a log line.  Together with
                            * target_bytes it widens what the allocation chooses from.  See "refinement passes" below */
    double target_psnr;    /* constant quality: the PSNR in dB every frame is to reach, in the model's terms, with as few
                            * bytes as it takes; 0: off (default), the stream written before this field.  Valid with
                            * irreversible 0 or 1, tiles and ht_passes; in a batch it applies to each frame on its own.
                            * Negative, NaN or infinite: HTJ2K_ERR_EINVAL and a log line (the context-free calls too).
                            * See "constant quality" below */
    int64_t group_bytes;   /* a byte budget over the frames of one call: upper limit of the codestreams of all n frames of
                            * an htj2k_encode_batch together, each SOC to EOC (htj2k_encode_frame: a group of one); 0: off
                            * (default), the stream written before this field.  Valid with irreversible 0 or 1, tiles,
                            * ht_passes, frames of different sizes, device input and output, and with target_bytes (both
                            * hold).  Negative: HTJ2K_ERR_EINVAL and a log line (the context-free calls too).  See "a budget
                            * over a group of frames" below */
} htj2k_enc_opts;
void   htj2k_enc_opts_default(htj2k_enc_opts *opts);

/* one code-block in the encoder's order (tile by tile; in a tile packet order: resolution, component, band, raster) */
typedef struct htj2k_enc_block {
    int32_t comp, res, band;   /* band: 0 LL, 1 HL, 2 LH, 3 HH */
    int32_t x, y, w, h;        /* rectangle in the component's coefficient plane: every tile-component's Mallat layout
                                * (LL top-left) sits in that tile-component's rectangle of the plane */
    int32_t expn;              /* exponent of its band in QCD / QCC (T.800 A.6.4) */
} htj2k_enc_block;

/* Context-free (no device needed).
 *   htj2k_encode_bound  worst-case codestream bytes of one frame; 0 when the frame is out of scope
 *   htj2k_enc_layout    the code-blocks of a frame (derived with the decoder's geometry code, j2k_tier2.c); returns
 *                       their number, fills at most `cap` entries
 *   htj2k_enc_assemble  the codestream of a frame from caller-coded blocks: block_bytes[i] / lcup[i] (0: an all-zero
 *                       block, left out), max_u[i] its largest U (for the automatic guard bits; NULL: 2 or opts');
 *                       nblocks must be the layout's block count (HTJ2K_ERR_EINVAL otherwise).
 *                       Writes SOC, SIZ (put_siz), CAP, COD (put_cod), QCD / QCC (put_qcd), per tile SOT, SOD and the
 *                       packets (encode_packet, tag_tree_code; T.800 B.9-B.10), and EOC.  HTJ2K_ERR_ENOSPC past `cap`. */
/* ---- tiles (htj2k_enc_opts.tile_w / tile_h) ----
 * SIZ carries the tile size (a 0 resolved to the image's), the main header is the one of the untiled stream -- QCD, QCC,
 * MAGB and the guard bits are decided over the blocks of all tiles --, and every tile follows in raster order of its
 * index as one tile-part: SOT (Isot, Psot, TPsot 0, TNsot 1), SOD, the tile's packets.  No TLM, no PLT.  Blocks are
 * numbered tile by tile everywhere (htj2k_enc_layout, htj2k_enc_assemble, htj2k_enc_last_planes).  target_bytes stays
 * the budget of the frame's whole codestream; its smallest stream holds every tile's SOT, SOD and empty packets.
 *   htj2k_enc_tiles     the tiles of a frame: returns their number, fills at most `cap` entries */
typedef struct htj2k_enc_tile {
    int32_t blk0, nblk;        /* the tile's blocks in htj2k_enc_layout's order */
    int32_t x0[4], y0[4], x1[4], y1[4];   /* per component: the tile-component's rectangle in the component plane */
} htj2k_enc_tile;
int    htj2k_enc_tiles(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts,
                       htj2k_enc_tile *tiles, int cap);
size_t htj2k_encode_bound(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts);
int    htj2k_enc_layout(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts,
                        htj2k_enc_block *blocks, int cap);
int    htj2k_enc_assemble(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts,
                          const uint8_t *const *block_bytes, const int *lcup, const int *max_u, int nblocks,
                          uint8_t *out, size_t cap, size_t *out_len);
/* htj2k_enc_assemble with the bit-plane each block was coded from: block i holds sign(v) * (|v| >> planes[i]) and is
 * signalled with zbp = expn + G - 2 - planes[i] zero bit-planes (planes = NULL: all 0, which is htj2k_enc_assemble).
 * The automatic guard bits G cover max_u[i] + planes[i].  HTJ2K_ERR_EINVAL, nothing written: a negative plane of an
 * included block (-1 is accepted for a block that is left out, lcup[i] = 0: what htj2k_enc_last_planes reports;
 * anything below -1 never), a plane that makes zbp negative, or, under fixed guard bits, max_u[i] + planes[i] beyond
 * M_b = expn + G - 1. */
int    htj2k_enc_assemble_planes(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts,
                                 const uint8_t *const *block_bytes, const int *lcup, const int *max_u, const int *planes,
                                 int nblocks, uint8_t *out, size_t cap, size_t *out_len);

/* ---- refinement passes (htj2k_enc_opts.ht_passes 2 or 3) ----
 * Without a budget every block is coded as the cleanup pass at bit-plane 1 (of sign * (|v| >> 1)) and, at plane 0, the SigProp pass
 * (ht_passes 2) or SigProp and MagRef (3), both in one refinement segment Dref behind the cleanup segment (T.814 7.4,
 * 7.5; code-block style 0x40, no vertically causal mode).  The packet header signals the pass count (T.800 Table B.4)
 * and two lengths.  This is lossy even with three passes: a sample of magnitude 1 that no significant neighbour leads
 * SigProp to is decoded as 0.  Fallback: a block with no |v| >= 2, or whose Dref would be empty (two passes and every
 * sample significant at plane 1, a 1 x 1 block for one), is coded as one cleanup pass at plane 0, as without the
 * option.  htj2k_encode_bound grows by the worst case of Dref only when ht_passes > 1.
 * With a budget (target_bytes > 0) a block's candidates are, for every plane p, one pass at p, "cleanup at p + 1 and
 * SigProp at p" and (ht_passes 3) "... and MagRef at p", besides "left out": steps between the quantisers 2^p and
 * 2^(p + 1).  Their distortions and the bits of the two passes are exact (htj2k_enc_rc_stats_passes), their lengths the
 * cleanup estimate of plane p + 1 plus those bits in bytes; the trial rule, the correction rounds and the last resort
 * are as described under "rate control", on the bytes of both segments.  htj2k_enc_last_planes / htj2k_enc_last_passes
 * report what every block got.
 *   htj2k_enc_assemble_passes  htj2k_enc_assemble_planes for blocks of up to three passes: block_bytes[i] holds
 *                       lcup[i] + lref[i] bytes, Dcup then Dref; npasses[i] in 1 .. 3; planes[i] is the plane p of the
 *                       refinement passes, the cleanup pass of a block of more than one pass having coded plane p + 1
 *                       (zbp = expn + G - 2 - (p + 1); the automatic guard bits cover max_u[i] + p + 1).  npasses =
 *                       NULL: all 1 (lref is not read).  HTJ2K_ERR_EINVAL, nothing written: a pass count outside
 *                       1 .. 3, lref[i] > 0 with one pass, lref[i] = 0 with more than one, and what
 *                       htj2k_enc_assemble_planes refuses, with p + 1 for the plane of such a block. */
int    htj2k_enc_assemble_passes(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts,
                                 const uint8_t *const *block_bytes, const int *lcup, const int *lref, const int *npasses,
                                 const int *max_u, const int *planes, int nblocks, uint8_t *out, size_t cap, size_t *out_len);

/* ---- rate control (htj2k_enc_opts.target_bytes > 0) ----
 * HT code-blocks are not embedded, but a cleanup pass may start at any bit-plane p of a block, signalled by the
 * block's zero-bit-plane count alone; dropping p planes is quantising the block with step 2^p * step.  A budgeted call
 * codes every block from the caller's quality (qstep; lossless for 5/3) and picks p per block, or leaves the block
 * out, so that the frame fits target_bytes with the least distortion (the PCRD-opt idea of T.800 J.14 over the points
 * plane 0, 1, .. 15 and "left out").  The choice is made on the device from estimated lengths; the exact lengths are
 * known after coding, and frames that came out too large are corrected.
 *   a call that returns 0 has written at most target_bytes bytes for every frame;
 *   a budget below the frame's smallest stream (headers and empty packets) or a negative one: HTJ2K_ERR_EINVAL and a
 *   log line, nothing written;  a budget at or above the unconstrained size: the unconstrained bytes exactly.
 * htj2k_encode_bound, `cap` and HTJ2K_ERR_ENOSPC do not depend on the budget. */

/* ---- a budget over a group of frames (htj2k_enc_opts.group_bytes > 0) ----
 * The minimum-distortion answer to a constraint on a sum is one slope for all blocks of all frames: an easy frame gives
 * its bytes to a hard one.  With est_f(lambda) the estimate rate control sums for frame f at slope lambda (scaled
 * lengths of the candidates of least w d + lambda * bytes, plus the header bits rounded to bytes per frame; an all-zero
 * block counts at its plane-0 length) and room = group_bytes - the sum of the frames' smallest streams:
 *   1. only with target_bytes > 0: rate control's selection per frame, unchanged -> lambda_f (0 for a frame on trial; 0
 *      for every frame without caps);
 *   2. trial: every block takes plane 0 when the sum of the frames' lower bounds fits the room and no frame has lambda_f > 0;
 *   3. else rate control's bisection (slope 0 first, then 64 halvings of (0, 1 + the largest w * dskip of the group),
 *      ending on the feasible side) on E(lambda) = sum over f of est_f(max(lambda, lambda_f)) -> lambda_g;
 *   4. the blocks of frame f take their candidate at max(lambda_g, lambda_f).
 * A group of one frame without a cap is therefore the call with target_bytes = group_bytes, byte for byte, and with caps
 * a group_bytes that the capped selection's estimate fits (n * target_bytes for one) is the capped call.
 *   a call that returns 0 has written at most group_bytes bytes in all, and at most target_bytes per frame where set;
 *   a group_bytes at or above the unconstrained total: the unconstrained bytes exactly;
 *   deterministic and independent of the order of the frames: every frame's stream is the same wherever it stands.
 * HTJ2K_ERR_EINVAL and a log line, nothing written: a negative group_bytes; one below the sum of the frames' smallest
 * streams; target_psnr > 0 as well; a call that would take more than one round (2^30 samples, or HTJ2K_ENC_ROUND): a
 * group is selected with all its statistics on the device at once.
 * Correction: frames over their own cap are selected again as in rate control (new lambda_f); when the sum is over,
 * every coded block's estimates are scaled by actual / estimated, the room shrinks by the overshoot and steps 2 - 4 run
 * again; both feed the same HT launch, at most 3 launches.  Then the last resort of rate control for frames over their
 * cap and, while the sum is over, blocks are left out across the group, least weighted distortion per byte saved first
 * (last_resort = 1).  A group under budget is left alone.
 * htj2k_encode_bound, `cap` and HTJ2K_ERR_ENOSPC do not depend on group_bytes. */

/* ---- constant quality (htj2k_enc_opts.target_psnr > 0) ----
 * The dual of rate control over the same candidates: every frame reaches target_psnr, in the terms of the model below,
 * with the least estimated bytes.  For a frame of N samples (every component's own samples) and peak = 2^bits - 1,
 *   D(selection) = sum over the blocks of  w_b * (base_b + d_b / 4)
 *   model_psnr   = 10 log10(peak^2 N / D),      D_target = peak^2 N / 10^(target_psnr / 10)
 * w_b is the weight of the block's band (htj2k_enc_band_weights: step, synthesis norm, column norm of the inverse ICT /
 * RCT, squared); d_b the statistic of the candidate the block got (htj2k_enc_rc_stats' dist, htj2k_enc_rc_stats_passes'
 * dist2 / dist3, or the distortion of leaving it out; d is twice the error, hence the 4); base_b the error of the
 * caller's quantiser itself, in index units: the sum over the block's samples of e^2 with c = |v| / step, m = floor(c),
 * e = c - (m + 1/2) where m > 0 and e = c where m = 0 (htj2k_enc_rc_base); 0 for 5/3.  The model leaves out the cross
 * term between the two errors, and it is stated in coefficients: the rounding of the output pixels to integers is not
 * in it (DESIGN.md 3.5 has what both cost, measured).  The guarantee is stated in the model:
 *   a call that returns 0 has D <= D_target for every frame, or the frame has short_of_target = 1: base_psnr, the best
 *   the caller's qstep allows, is below the target, and every block is one cleanup pass at plane 0.  Not an error.
 * The selection is the largest slope lambda, by the bisection of rate control, at which D <= D_target; every block
 * takes the candidate of least w d + lambda * estimated bytes.  The sizes are estimates, the constraint is a sum of
 * exact numbers: a quality-only call takes one HT launch and no correction rounds.  When leaving every block out meets
 * the target, every block is left out; an all-zero block keeps plane 0.
 * With target_bytes > 0 as well the budget is a cap: the quality selection runs first, and a frame whose estimate or
 * whose coded size exceeds target_bytes is coded again exactly as the call with the budget alone codes it (capped = 1;
 * htj2k_enc_rc_info as for that call); rate control's guarantee and its HTJ2K_ERR_EINVAL rules hold.
 * Deterministic: double sums run in a fixed order (strided per thread, the wave, then the waves in order).
 *   htj2k_enc_band_weights  context-free: the weight w of every block in htj2k_enc_layout's order; returns the number
 *                           of blocks, fills at most `cap` entries */
int    htj2k_enc_band_weights(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts, double *w, int cap);

/* The device encoder (FFCodec.init / .close of an encoder: j2kenc.c's j2kenc_init / j2kenc_destroy).  Fails with
 * HTJ2K_ERR_ENOSYS without a usable gfx950 device: there is no CPU fallback. */
typedef struct htj2k_enc_ctx htj2k_enc_ctx;
int    htj2k_enc_open(int device_id, htj2k_enc_ctx **out);
void   htj2k_enc_close(htj2k_enc_ctx *ctx);
void   htj2k_enc_set_log(htj2k_enc_ctx *ctx, htj2k_log_fn fn, void *opaque);
/* encode_frame (j2kenc.c): one frame in host memory (`in` as the decoder hands frames out: data / linesize /
 * width / height / pix_fmt) -> one codestream in `out`.  `bits` = bits_per_raw_sample (the layout's depth or less:
 * samples are read as value >> (precision - bits), the inverse of the decoder's pack stage).  Only those `bits` bits
 * of a sample are read: the bits below the shift are dropped, and the bits of the word above `bits` (layouts stored
 * without a shift, e.g. bits 10 .. 15 of a yuv420p10le word) are masked off, so neither changes the codestream.
 * `linesize` may exceed the row (padding is never read) and need not be a multiple of the sample size. */
int    htj2k_encode_frame(htj2k_enc_ctx *ctx, const htj2k_frame *in, int bits, const htj2k_enc_opts *opts,
                          uint8_t *out, size_t cap, size_t *out_len);
/* n frames of one layout and depth (sizes may differ) -> n codestreams back to back in `out`, frame i at
 * offsets[i] .. offsets[i + 1].  in_on_device: the planes of `in` are device addresses (htj2k_job_device_frame,
 * htj2k_pipe_receive_device); out_on_device: `out` is device memory.  Every stage runs as one launch over the
 * frames (large batches go through in a few such rounds). */
int    htj2k_encode_batch(htj2k_enc_ctx *ctx, const htj2k_frame *in, int n, int bits, const htj2k_enc_opts *opts,
                          int in_on_device, uint8_t *out, size_t cap, int out_on_device, size_t *offsets);
/* n images of width x height in a float tensor in device memory -> n codestreams, as htj2k_encode_batch writes them
 * ("tensors as frames" above has the definition of a sample).  The unpack stage reads the tensor itself
 * (k_enc_unpack_tensor, csrc/enc_kernels.hpp): no frame is materialised, and everything behind that stage is the
 * encoder's own.  The result is, byte for byte, htj2k_encode_batch of the frames htj2k_tensor_to_frames writes for this
 * tensor, for every `opts`; htj2k_enc_stage_ms' first figure is the reading kernel's time, and the other info calls
 * speak of the call as they do for htj2k_encode_batch.  src is only read; the call returns after the codestreams are
 * written.  HTJ2K_ERR_EINVAL, nothing launched and nothing written, checked in this order and before the context (a NULL
 * context with valid arguments answers HTJ2K_ERR_ENOSYS): a missing argument (opts may be NULL: the defaults); n < 1;
 * width or height < 1; a pix_fmt outside the enum (PAL8 at this point: HTJ2K_ERR_PATCHWELCOME); bits < 1 or above the
 * layout's depth; dtype or layout outside its enum; a scale or bias that is not finite (only the first C entries are
 * read); out_w / out_h not both 0; src_bytes below n images; src misaligned for its element (4, 2, 2 bytes).  Then
 * whatever htj2k_encode_batch refuses for n frames of that size, layout, bits and opts, with its codes and log lines
 * (XYZ12: HTJ2K_ERR_PATCHWELCOME, as there). */
int    htj2k_encode_tensor(htj2k_enc_ctx *enc, const void *src, size_t src_bytes, int n, int width, int height,
                           int pix_fmt, int bits, const htj2k_tensor_spec *spec, const htj2k_enc_opts *opts,
                           uint8_t *out, size_t cap, int out_on_device, size_t *offsets);
/* the same from a tensor of K channels through a colour matrix and a chroma filter ("tensors as frames, mixed" above has
 * the definition and the refusals); mix NULL: htj2k_encode_tensor exactly, which is a one-line call of this */
int    htj2k_encode_tensor_mix(htj2k_enc_ctx *enc, const void *src, size_t src_bytes, int n, int width, int height,
                               int pix_fmt, int bits, const htj2k_tensor_spec *spec, const htj2k_tensor_mix_in *mix,
                               const htj2k_enc_opts *opts, uint8_t *out, size_t cap, int out_on_device, size_t *offsets);
/* the same with a transfer curve before the matrix and one after it ("tensors as frames, with curves" above has the
 * definition and the refusals; k_enc_unpack_tensor_curves); curves NULL: htj2k_encode_tensor_mix exactly, which is a
 * one-line call of this */
int    htj2k_encode_tensor_curves(htj2k_enc_ctx *enc, const void *src, size_t src_bytes, int n, int width, int height,
                                  int pix_fmt, int bits, const htj2k_tensor_spec *spec, const htj2k_tensor_mix_in *mix,
                                  const htj2k_tensor_curves_in *curves, const htj2k_enc_opts *opts, uint8_t *out, size_t cap,
                                  int out_on_device, size_t *offsets);
/* ---- measured quality (what AV_CODEC_FLAG_PSNR asks of an encoder: AVCodecContext.error[] per coded frame,
 *      ff_side_data_set_encoder_stats) ----
 * target_psnr holds in the terms of the model, in coefficients; the decoded pixels may fall short of it (5/3 with the
 * RCT at 44 dB: by about 1 dB).  htj2k_encode_batch_measured answers with pixels: it encodes as
 * htj2k_encode_batch does, decodes its own streams with the product decoder `dec` as jobs on the device and compares
 * them with the input where it lies (htj2k_job_compare: a device input is read in place, no frame crosses PCIe for the
 * measurement; the codestream bytes do when out_on_device is set, because the parser reads host memory).
 *
 * Report only (mopts NULL, close_loop 0, or no target_psnr): the streams are byte for byte those of htj2k_encode_batch
 * with the same arguments, any opts; rounds = 1, first_psnr = diff.psnr, and short_measured says whether the stream
 * measures below a target_psnr that was given.  The streams are parsed with the input's layout as the pixel-format
 * request, whatever `dec` was opened with; its bitexact is honoured; they decode in chunks of frames bounded by the
 * encoder's round size.  reduction_factor != 0 on `dec`: HTJ2K_ERR_PATCHWELCOME; contexts on different devices:
 * HTJ2K_ERR_EINVAL (the rules of htj2k_transcode_batch); a block error in the decode of the encoder's own stream:
 * HTJ2K_ERR_BUG.  Missing arguments, close_loop outside 0 .. 1 and max_rounds outside 0 .. 16 are HTJ2K_ERR_EINVAL,
 * checked before the contexts; a NULL context then answers HTJ2K_ERR_ENOSYS.
 *
 * Closing the loop (close_loop 1, opts->target_psnr = T > 0).  Round 1 is the plain call.  A frame is final when its
 * measured PSNR m is at least T, when quality_info.capped is set (the budget decided) or when .short_of_target is set
 * (it is the plane-0 stream already).  The others are encoded again as one batch, each with a target of its own,
 *     T_next = T_prev + max(T - m, 0.05 dB)        (the floor makes every correction move)
 * for up to max_rounds quality rounds (0: the default, 8: the worst case measured over the 24 cases of
 * tests/test_encode_measured_gpu.py, 7, plus one).  Frames still short are coded once more with target_psnr
 * off -- the finest the caller's quantiser allows, lossless for 5/3 --, get fell_back = 1 and are measured.
 *   a call that returns 0 has diff.psnr >= target_psnr for every frame, or the frame has short_measured = 1 and is the
 *   finest stream the options allow (fell_back, short_of_target or capped is then set);
 *   the loop adds no coding path: a frame's final stream is byte for byte the output of htj2k_encode_batch of that frame
 *   alone with target_psnr = target_used (with target_psnr = 0 when fell_back is set): constant quality treats every
 *   frame on its own and is deterministic.
 * htj2k_enc_quality_info, htj2k_enc_rc_info, htj2k_enc_last_planes and htj2k_enc_last_passes speak of each frame's final
 * round.  The streams are packed back to back in `out` after the last round; HTJ2K_ERR_ENOSPC is judged on the final
 * sizes, and nothing is written past `cap` (nothing at all then). */
typedef struct htj2k_enc_measure_opts {
    int close_loop;     /* 0: report only.  1: with opts->target_psnr > 0, hold the target in decoded pixels */
    int max_rounds;     /* quality rounds of the loop, 1 .. 16; 0: the default */
} htj2k_enc_measure_opts;
typedef struct htj2k_enc_measured {
    htj2k_frame_diff diff;   /* the final stream, decoded by `dec`, against the input */
    double  first_psnr;      /* measured PSNR of round 1 (= diff.psnr when rounds = 1) */
    double  target_used;     /* the target_psnr the final stream was selected with (0: none / fell back) */
    int32_t rounds;          /* quality rounds this frame took part in, >= 1 */
    int32_t fell_back;       /* 1: still short after max_rounds; the frame is the stream without target_psnr */
    int32_t short_measured;  /* 1: the final stream measures below target_psnr (in a closed loop only ever with fell_back,
                              * quality_info.short_of_target or .capped: nothing finer was allowed) */
} htj2k_enc_measured;
int    htj2k_encode_batch_measured(htj2k_ctx *dec, htj2k_enc_ctx *enc, const htj2k_frame *in, int n, int bits,
                                   const htj2k_enc_opts *opts, const htj2k_enc_measure_opts *mopts, int in_on_device,
                                   uint8_t *out, size_t cap, int out_on_device, size_t *offsets, htj2k_enc_measured *res);
/* on = 1: htj2k_encode_batch_measured also calls htj2k_job_compare_ssim on every job it has just compared (no second
 * decode) and keeps, per frame, the figures of that frame's final stream: in a closed loop those of the last round the
 * frame took part in, the fall-back round included.  0 (default): nothing changes -- streams, htj2k_enc_measured,
 * timings and launches are what they were.  Other values: HTJ2K_ERR_EINVAL.  The loop still closes on PSNR. */
int    htj2k_enc_measure_ssim(htj2k_enc_ctx *enc, int on);
/* the structural similarity of frame `frame` of the last call; HTJ2K_ERR_EINVAL when that call was not a
 * htj2k_encode_batch_measured that returned 0 with the switch on, or when `frame` is not one of its frames */
int    htj2k_enc_last_ssim(htj2k_enc_ctx *enc, int frame, htj2k_frame_ssim *out);
/* ---- kernel-level entry points of the encoder (unit tests) ---- */
/* the forward 5/3 transform (T.800 F.4.8.2, origin 0) of a host int32 plane of w x h samples, in place, into the
 * Mallat layout the decoder's HT stage writes (the inverse of htj2k_idwt_plane with type 1) */
int    htj2k_fdwt_plane(htj2k_enc_ctx *ctx, int32_t *plane, int w, int h, int levels);
/* the forward 9/7 counterpart: un-normalised float lifting (origin 0, whole-sample symmetric extension; a line of one
 * sample is scaled by 1 / X, at every level) of a host float plane, in place, into the Mallat layout (the inverse of
 * htj2k_idwt_plane with type 0) */
int    htj2k_fdwt97_plane(htj2k_enc_ctx *ctx, float *plane, int w, int h, int levels);
/* the same transforms of tile-components that do not start at 0: region i is the w x h samples at (px, py) of a host
 * plane of plane_w x plane_h 4-byte samples (int32 for 5/3; float with irreversible), and stands for the samples
 * x0 .. x0 + w - 1, y0 .. y0 + h - 1 of a tile-component (T.800 F.4.8: the samples at even positions are low-pass and
 * come first, the extension reflects about the first and the last sample; a line of one sample at an odd position is
 * doubled by 5/3 and scaled by 2 / K by 9/7).  Regions must not overlap; every region is transformed in place over
 * its own `levels`, all of them in one launch per level and direction, and the rest of the plane is not touched. */
typedef struct htj2k_enc_region {
    int32_t px, py, w, h;      /* where the region lies in the plane */
    int32_t x0, y0;            /* the tile-component coordinates of its first sample, >= 0 */
    int32_t levels;            /* 0 .. 32 */
} htj2k_enc_region;
int    htj2k_fdwt_regions(htj2k_enc_ctx *ctx, void *plane, int plane_w, int plane_h, const htj2k_enc_region *regions,
                          int nregions, int irreversible);
/* HT cleanup encoding of the blocks (x, y, w, h of each) of a host int32 plane of signed coefficients: block i's
 * bytes land at out + offsets[i] (the call sets offsets[0 .. nblocks]), lcup[i] of them (0: all zero), max_u[i] its
 * largest exponent bound U.  A block must fit T.800's limits (w, h <= 1024, w * h <= 4096) and have at most 1024
 * quads (ceil(w / 2) * ceil(h / 2)), else HTJ2K_ERR_EINVAL; the arguments are checked before the context, and a
 * NULL context with valid arguments answers HTJ2K_ERR_ENOSYS. */
int    htj2k_ht_encode_blocks(htj2k_enc_ctx *ctx, const int32_t *coef, int plane_w, int plane_h,
                              const htj2k_enc_block *blocks, int nblocks, uint8_t *out, size_t cap,
                              size_t *offsets, int *lcup, int *max_u);
/* the same with block i coded from sign(v) * (|v| >> planes[i]), planes[i] in 0 .. 31 (HTJ2K_ERR_EINVAL otherwise);
 * planes = NULL is htj2k_ht_encode_blocks */
int    htj2k_ht_encode_blocks_planes(htj2k_enc_ctx *ctx, const int32_t *coef, int plane_w, int plane_h,
                                     const htj2k_enc_block *blocks, int nblocks, const int *planes, uint8_t *out, size_t cap,
                                     size_t *offsets, int *lcup, int *max_u);
/* the same with up to three passes: passes[i] in 1 .. 3 (NULL: all 1), planes[i] (NULL: all 0) the plane p of the last
 * pass; for more than one pass p <= 30, the cleanup pass codes sign(v) * (|v| >> (p + 1)) and the refinement segment
 * follows it at out + offsets[i] + lcup[i], lref[i] bytes.  A block that falls back ("refinement passes" above) comes
 * back as one pass at p: lref[i] = 0.  The regions between offsets are larger for blocks that ask for passes; the
 * bytes are those of the vector factory's encode_block(sign(v) * (|v| >> p), passes). */
int    htj2k_ht_encode_blocks_passes(htj2k_enc_ctx *ctx, const int32_t *coef, int plane_w, int plane_h,
                                     const htj2k_enc_block *blocks, int nblocks, const int *planes, const int *passes,
                                     uint8_t *out, size_t cap, size_t *offsets, int *lcup, int *lref, int *max_u);
/* what the rate allocation reads, for blocks (as above) of a host int32 plane: for block i and p in 0 .. nplanes - 1
 * (1 <= nplanes <= 16), row-major [block][p],
 *   dist     sum over the samples of d^2, d twice the error of the decoder's mid-point reconstruction of
 *            sign * (m >> p) against m + 1/2: 0 where m = 0; 2 m + 1 where m >> p = 0;
 *            else 2 m + 1 - 2 ((m >> p) << p) - 2^p.  Exact.
 *   len_est  estimated bytes of the cleanup segment of sign * (m >> p): 0 exactly where every m >> p is 0 */
int    htj2k_enc_rc_stats(htj2k_enc_ctx *ctx, const int32_t *coef, int plane_w, int plane_h,
                          const htj2k_enc_block *blocks, int nblocks, int nplanes, uint64_t *dist, uint32_t *len_est);
/* the same for the candidates of more than one pass (htj2k_enc_opts.ht_passes), row-major [block][p]: of "cleanup at
 * plane p + 1, SigProp at p" the distortion dist2 and the bits SigProp writes (a bit per sample it visits, a sign per
 * newly significant one), of "... and MagRef at p" the distortion dist3 and MagRef's bits (one per sample significant at
 * p + 1); d as above with the decoder's reconstruction of such a block: the mid-point of the planes a significant
 * sample has, 3/2 * 2^p for a newly significant one, 0 for every other.  All exact.  Where nothing is significant at
 * plane p + 1 there is no such candidate and all four are 0; sp_bits 0 alone: none of two passes. */
int    htj2k_enc_rc_stats_passes(htj2k_enc_ctx *ctx, const int32_t *coef, int plane_w, int plane_h,
                                 const htj2k_enc_block *blocks, int nblocks, int nplanes, uint64_t *dist2, uint64_t *dist3,
                                 uint32_t *sp_bits, uint32_t *mr_bits);
/* base_b of "constant quality" for blocks (as above) of a host float plane of 9/7 coefficients before the quantiser:
 * step[i] (finite, > 0) is the step of block i's band, base[i] the sum over the block's samples of e^2.  The division
 * is the quantiser's, (double)|v| / (double)step, so m is the index it writes.  Argument checks as htj2k_enc_rc_stats. */
int    htj2k_enc_rc_base(htj2k_enc_ctx *ctx, const float *coef, int plane_w, int plane_h,
                         const htj2k_enc_block *blocks, int nblocks, const float *step, double *base);
/* the last htj2k_encode_batch, frame by frame (0 .. n - 1): the plane chosen for every block in htj2k_enc_layout's
 * order (-1: left out by the allocation; a block that is all zero at its plane keeps the plane); returns the number of
 * blocks, fills at most `cap` entries.  Without a budget every plane is 0. */
int    htj2k_enc_last_planes(htj2k_enc_ctx *ctx, int frame, int *planes, int cap);
/* beside it, the passes every block got (1 .. 3; 1 for a block that is left out).  For a block of more than one pass
 * htj2k_enc_last_planes reports the plane of the refinement passes */
int    htj2k_enc_last_passes(htj2k_enc_ctx *ctx, int frame, int *passes, int cap);
typedef struct htj2k_enc_rc {
    int64_t target_bytes;      /* the budget (0: none) */
    int64_t est_bytes;         /* size the first selection expected */
    int64_t final_bytes;       /* size written */
    int32_t nblocks;
    int32_t blocks_left_out;   /* blocks the allocation left out */
    int32_t ht_launches;       /* HT cleanup launches this frame took part in (1 .. 3) */
    int32_t blocks_recoded;    /* blocks coded more than once */
    int32_t trial;             /* 1: the first launch coded every block at plane 0 because the frame might fit as it is */
    int32_t last_resort;       /* 1: still over budget after the third launch; the host left blocks out until it fitted */
} htj2k_enc_rc;
int    htj2k_enc_rc_info(htj2k_enc_ctx *ctx, int frame, htj2k_enc_rc *info);
/* the same for the group of the last htj2k_encode_batch; all 0 after a call without group_bytes.  htj2k_enc_rc_info,
 * htj2k_enc_last_planes and htj2k_enc_last_passes keep their per-frame meaning (target_bytes: the frame's own cap, or 0) */
typedef struct htj2k_enc_group {
    int64_t group_bytes, est_bytes, final_bytes;   /* sums over the frames, whole codestreams */
    double  lambda;            /* the common slope the first selection ended on (0: trial, or the caps alone decided) */
    int32_t nframes, nblocks;
    int32_t frames_capped;     /* frames whose own target_bytes gave them a steeper slope than the group's */
    int32_t ht_launches;       /* 1 .. 3 */
    int32_t trial, last_resort;
} htj2k_enc_group;
int    htj2k_enc_group_info(htj2k_enc_ctx *ctx, htj2k_enc_group *info);
/* device ms of the group kernels (k_rc_group_sweep, k_rc_group_step, k_rc_group_apply), all their runs in the last
 * htj2k_encode_batch; not in htj2k_enc_rc_stage_ms' second figure */
int    htj2k_enc_group_stage_ms(htj2k_enc_ctx *ctx, float *ms);
/* the group selection on caller-made tables, single-pass candidates: nblk[f] blocks per frame, concatenated; per block
 * kmax (0 .. 16), dist[16], len[16] (row-major [block][p]), dskip, low0, weight, scale (NULL: 1); per frame floor
 * (NULL: 0) the slope lambda_f; room in bytes.  -> planes (-1: left out), *lambda, *est (the sum of est_f), *trial.
 * HTJ2K_ERR_EINVAL: a missing argument, nframes < 1, a frame without blocks, more than 2^24 blocks, kmax outside
 * 0 .. 16, a negative room, or a dskip, weight, scale or floor that is negative or not finite.  The arguments are
 * checked before the context; a NULL context with valid arguments answers HTJ2K_ERR_ENOSYS */
int    htj2k_enc_rc_group_select(htj2k_enc_ctx *ctx, int nframes, const int *nblk, const int *kmax, const uint64_t *dist,
                                 const uint32_t *len, const double *dskip, const uint32_t *low0, const double *weight,
                                 const double *scale, const double *floor, int64_t room, int allow_trial,
                                 int32_t *planes, double *lambda, uint64_t *est, int *trial);
/* the same for "constant quality"; all 0 for a call without target_psnr */
typedef struct htj2k_enc_quality {
    double  target_psnr;       /* as asked (0: none) */
    double  base_psnr;         /* model PSNR with every block at plane 0: the best qstep allows (infinity for 5/3) */
    double  model_psnr;        /* model PSNR of what was written */
    double  lambda;            /* the slope the selection ended on */
    int32_t short_of_target;   /* 1: base_psnr < target_psnr; the frame is the plane-0 stream */
    int32_t capped;            /* 1: target_bytes decided the frame, not target_psnr */
} htj2k_enc_quality;
int    htj2k_enc_quality_info(htj2k_enc_ctx *ctx, int frame, htj2k_enc_quality *info);
/* device ms of what constant quality adds to the last htj2k_encode_batch: k_rc_base97; the quality runs of the select
 * kernel (k_rc_select_q; not in htj2k_enc_rc_stage_ms' second figure) */
int    htj2k_enc_quality_stage_ms(htj2k_enc_ctx *ctx, float ms[2]);
/* device ms of the rate-control stages of the last htj2k_encode_batch: k_rc_stats, k_rc_select (all its runs), the HT
 * cleanup launches of the correction rounds (the first launch is htj2k_enc_stage_ms' third figure) */
int    htj2k_enc_rc_stage_ms(htj2k_enc_ctx *ctx, float ms[3]);
/* device ms of what a call that asks for passes adds to the last htj2k_encode_batch (both 0 when it asked for one):
 * k_ht_refine_plan + k_ht_refine_encode of the first HT launch (htj2k_enc_stage_ms' third figure stays the cleanup
 * kernel's), and k_rc_stats_passes (htj2k_enc_rc_stage_ms' first figure stays k_rc_stats').  The launches of the
 * correction rounds, refinement kernels included, are htj2k_enc_rc_stage_ms' third figure. */
int    htj2k_enc_ref_stage_ms(htj2k_enc_ctx *ctx, float ms[2]);
/* device time (ms) of the stages of the last htj2k_encode_batch: unpack + RCT / ICT, forward DWT (+ the quantiser when
 * irreversible), HT cleanup, gather */
int    htj2k_enc_stage_ms(htj2k_enc_ctx *ctx, float ms[4]);
/* rounds the last htj2k_encode_batch / htj2k_transcode_batch went through (HTJ2K_ENC_ROUND) */
int    htj2k_enc_last_rounds(htj2k_enc_ctx *ctx);
/* with HTJ2K_ENC_STAMPS=1 in the environment of htj2k_enc_open (measurements only): clock64() cycles of the HT cleanup
 * kernel's phases in the last htj2k_encode_batch / htj2k_ht_encode_blocks, summed over its coded blocks -- exponents +
 * contexts + codewords, MagSgn bit packing, the byte-after-0xFF pass, MEL + VLC, copy-out.  Returns the blocks counted. */
int    htj2k_enc_ht_cycles(htj2k_enc_ctx *ctx, uint64_t cycles[5]);
/* the same of k_ht_refine_encode, summed over the blocks that got a refinement segment -- the map, membership, SigProp
 * bits, the byte-after-0xFF pass, MagRef bits, MagRef bytes + copy-out.  Returns the blocks counted. */
int    htj2k_enc_ref_cycles(htj2k_enc_ctx *ctx, uint64_t cycles[6]);

/* ---- transcoding: Part-1 codestreams (with ht_sources = 1: HT and MIXED ones too) in, HTJ2K codestreams out,
 * coefficient-exact ----
 * Every code-block of a Part-1 (EBCOT / MQ) stream is decoded to its quantiser indices and coded again as an HT block
 * that decodes to the same sign-magnitude words, 5/3 and 9/7 alike: no inverse transform runs and nothing is lost
 * (T.814's headline use).  The output is the stream the encoder writes (above) with size, components,
 * sub-sampling, depth, tile grid, levels, code-block size, transform, the MCT bit, guard bits and every band's exponent
 * and mantissa copied from the source (a derived QCD is written expounded).  Code-blocks map 1:1.
 *
 * The block rule.  A source block has K coded bit-planes and n passes; n = 0: left out.  Otherwise n = 1 + 3 k + r and
 * its last cleanup pass coded plane pc = K - 1 - k:  r = 0 -> one HT cleanup pass at pc;  r = 1 -> cleanup at pc and
 * SigProp at pc - 1;  r = 2 -> cleanup at pc, SigProp and MagRef at pc - 1.  Where nothing is significant at pc, or the
 * refinement segment would be empty, the block is one cleanup pass at pc; a block that decodes to all zeros is left out.
 * htj2k_enc_last_planes / htj2k_enc_last_passes report, per block of the last call in htj2k_enc_layout's order, the plane
 * of the last pass and the passes it got (-1 and 1 for a source block without passes).
 *
 * An HT source block (htj2k_transcode_opts.ht_sources = 1; in a MIXED stream every block follows the rule of its own
 * coder) has n passes, placeholder passes included, and Z zero bit-planes of its band's M_b; n = 0: left out.  Otherwise
 * it has P0 = (n - 1) / 3 placeholder sets and k = n - 3 P0 passes (1 .. 3), and its cleanup pass coded plane
 * pc = M_b - 1 - (Z + P0):  the block is written with the same k passes, the last at pc - (k > 1), so a plain transcode
 * of an HT stream is a re-packing (and a budgeted one the way to a smaller HTJ2K stream without a second quantiser).
 * The two fall-backs apply as above; pc - (k > 1) < 0 is HTJ2K_ERR_INVALIDDATA.  A vertically causal source (Part-1
 * or HT) gives the non-causal output: the flag changes how the passes were coded, not the words they decode to.
 *
 * Accepted: Part-1 streams (or JP2 files) in any progression order, with any number of layers, precincts, tile-parts,
 * SOP / EPH, PPM / PPT and any code-block style; unsigned components in a layout the encoder accepts; image and
 * tile-grid origin 0.  Refused with a log line, nothing written:
 *   HTJ2K_ERR_PATCHWELCOME  HT or MIXED sources unless ht_sources = 1; RGN / ROI shift; components (or tiles) coded with different levels,
 *                           block size, transform, style, depth or guard bits; reduction_factor != 0 on `dec`; PAL8,
 *                           XYZ12, signed components; an origin other than 0; a quantisation style that does not go
 *                           with the transform (5/3 with steps, 9/7 without); precincts that cut code-blocks, i.e. a
 *                           block partition other than the encoder's layout; a Part-1 block that fills all M_b magnitude
 *                           bits (an HT block needs one of headroom: K < M_b)
 *   HTJ2K_ERR_INVALIDDATA   a frame in which any block fails to decode, or has more passes than bit-planes: damage is
 *                           not laundered into a clean-looking stream
 *   HTJ2K_ERR_EINVAL        contexts on different devices, missing arguments
 * The sources are parsed without a pixel-format request, whatever `dec` was opened with (htj2k_transcode_check does the
 * same, so its answer and its bound hold for every `dec`).  Log lines: the reason of every refusal, the decoder's
 * parser's included, goes to the log of `enc` (the parser's lines also to the log of `dec`).
 * out / cap / out_on_device / HTJ2K_ERR_ENOSPC / offsets: as htj2k_encode_batch.  The frames of a call may differ in
 * everything; they go through the encoder in rounds as its own frames do (HTJ2K_ENC_ROUND). */
int    htj2k_transcode_batch(htj2k_ctx *dec, htj2k_enc_ctx *enc, const uint8_t *const *pkts, const int *pkt_sizes, int n,
                             uint8_t *out, size_t cap, int out_on_device, size_t *offsets);
int    htj2k_transcode_frame(htj2k_ctx *dec, htj2k_enc_ctx *enc, const uint8_t *pkt, int pkt_size,
                             uint8_t *out, size_t cap, size_t *out_len);
/* context-free, no device: 0 if the stream is in scope, else the error htj2k_transcode_* would give for it (with the
 * log line; what only decoding the blocks shows is not found here); *bound = worst-case output bytes */
int    htj2k_transcode_check(const uint8_t *pkt, int pkt_size, size_t *bound, htj2k_log_fn log, void *opaque);
/* A byte budget per frame over the source's indices.  target_bytes > 0 is the upper limit of every
 * frame's codestream; 0, or opts == NULL, is htj2k_transcode_batch.
 *
 * For a source block the block rule gives (pr, k): pr the plane of its last pass, k its HT passes 1 .. 3, pc = pr + (k > 1)
 * its cleanup plane.  Under a budget an output block is that form or a coarser one, never a finer one: bits below the
 * source's last pass do not exist.  In planes relative to pr (p' = p - pr, m' = |index| >> pr) its candidates are what
 * an encoder call with ht_passes = 3 offers on m' -- one cleanup pass at p' >= 0, "cleanup at p' + 1, SigProp at p'",
 * "... and MagRef at p'", and "left out" -- and at p' = 0 only what the source can back:
 *     k = 1   all three
 *     k = 2   the two-pass candidate only (one pass at pr, or a MagRef at pr, would state bits the source never coded)
 *     k = 3   the two-pass and the three-pass candidate (one pass at pr would state bit pr of samples SigProp did not reach)
 * Where the block has no such candidate (nothing significant at pc, or SigProp would write nothing) its finest form is
 * one pass at pc, the rule's own fall-back.  The block's weight is its band's times 4^pr, so the model's reference
 * m' + 1/2 is the source decoder's mid-point and the source's own form has distortion 0.  One known offset: a block whose
 * source ended on SigProp (k = 2) shows d = 1 per sample significant at pc for its own form (the true reference there
 * is m' + 1); it shifts all of that block's candidates nearly alike and is not corrected.
 *
 * The first HT launch is the plain transcode, and each frame is measured.  A frame at or under target_bytes is final:
 * byte for byte the unbudgeted stream (htj2k_enc_rc_info: trial = 1, ht_launches = 1, est_bytes = 0).  Only when a frame
 * of a round is over do the statistics run; the frames that are over then go through the encoder's correction rounds
 * (at most 3 HT launches counting the first, then blocks are left out).  Guarantees: a call that returns 0 has written
 * at most target_bytes per frame; a budget at or above the unbudgeted size gives the unbudgeted bytes; every block is its
 * source's form or a coarser one; the result is deterministic, and each frame stands on its own in a batch and across
 * rounds.  A budget below a frame's smallest stream (htj2k_transcode_min_size), or a negative one: HTJ2K_ERR_EINVAL with a
 * log line, for the whole call, before anything runs and with nothing written.  cap, HTJ2K_ERR_ENOSPC and the bound of
 * htj2k_transcode_check do not depend on the budget.  htj2k_enc_last_planes / htj2k_enc_last_passes report absolute
 * planes and the passes written; htj2k_enc_rc_info is filled per frame as for a budgeted encode.
 * HT and MIXED sources (ht_sources = 1) take a budget as Part-1 sources do: the table above is stated in (pr, k), which
 * the block rule gives for either coder, and a batch may mix Part-1, HT and MIXED frames.
 * Not offered: group_bytes and target_psnr for transcodes, filling a frame that came in under its budget.
 *
 * ht_sources: 0 (the default) refuses a source with HT code-blocks (HT or MIXED) with HTJ2K_ERR_PATCHWELCOME; 1 accepts
 * it; any other value is HTJ2K_ERR_EINVAL with a log line.  Everything else on the list of refusals stays refused.
 * htj2k_transcode_opts_default writes the whole struct; the field is the struct's tail, so a caller that declares the
 * struct without it must hand over zeroed room for it. */
typedef struct htj2k_transcode_opts {
    int64_t target_bytes;
    int     ht_sources;
} htj2k_transcode_opts;
void   htj2k_transcode_opts_default(htj2k_transcode_opts *opts);
int    htj2k_transcode_batch_opts(htj2k_ctx *dec, htj2k_enc_ctx *enc, const uint8_t *const *pkts, const int *pkt_sizes, int n,
                                  const htj2k_transcode_opts *opts, uint8_t *out, size_t cap, int out_on_device, size_t *offsets);
int    htj2k_transcode_frame_opts(htj2k_ctx *dec, htj2k_enc_ctx *enc, const uint8_t *pkt, int pkt_size,
                                  const htj2k_transcode_opts *opts, uint8_t *out, size_t cap, size_t *out_len);
/* context-free, as htj2k_transcode_check and with its refusals: *min_bytes = the smallest stream a budget may name
 * (headers and empty packets, every block left out) */
int    htj2k_transcode_min_size(const uint8_t *pkt, int pkt_size, int64_t *min_bytes, htj2k_log_fn log, void *opaque);
/* htj2k_transcode_check and htj2k_transcode_min_size in one call, for the scope `opts` names (ht_sources; the budget is
 * not read): *bound and *min_bytes as there, either may be NULL.  opts == NULL: the two entries above. */
int    htj2k_transcode_check_opts(const uint8_t *pkt, int pkt_size, const htj2k_transcode_opts *opts, size_t *bound,
                                  int64_t *min_bytes, htj2k_log_fn log, void *opaque);
/* unit entry: the tables a budgeted transcode selects from, for caller-given blocks of one plane of indices (as
 * htj2k_enc_rc_stats; nplanes 2 .. 16).  src_plane[i] (0 .. 30) and src_passes[i] (1 .. 3) are the source's (pr, k) of
 * block i.  dist, len_est (htj2k_enc_rc_stats) and dist2, dist3, sp_bits, mr_bits (htj2k_enc_rc_stats_passes) are taken
 * on |v| >> pr and carry UINT64_MAX where the table above disables a candidate; own_len[i] is the estimate of the block's
 * own form.  Arguments are checked before the context; a NULL context: HTJ2K_ERR_ENOSYS. */
int    htj2k_xc_rc_tables(htj2k_enc_ctx *ctx, const int32_t *coef, int plane_w, int plane_h, const htj2k_enc_block *blocks,
                          int nblocks, const int *src_plane, const int *src_passes, int nplanes, uint64_t *dist,
                          uint32_t *len_est, uint64_t *dist2, uint64_t *dist3, uint32_t *sp_bits, uint32_t *mr_bits,
                          uint32_t *own_len);
/* device ms of the last htj2k_transcode_batch: the source's block stage (on the decoder's stream), the scatter of the
 * tile-component planes into the encoder's planes, the HT stage (cleanup + refinement kernels), gather */
int    htj2k_transcode_stage_ms(htj2k_enc_ctx *enc, float ms[4]);
/* the quantisation of a stream given explicitly instead of derived from bits / qstep: guard bits 1 .. 7 and, per
 * component and band (0 LL, then HL LH HH from the lowest resolution up), the exponent (0 .. 31) and, for 9/7, the
 * mantissa (0 .. 2047) of QCD / QCC */
typedef struct htj2k_enc_quant {
    int      guard_bits;
    uint8_t  expn[4][97];
    uint16_t mant[4][97];
} htj2k_enc_quant;
/* htj2k_enc_assemble_passes with that quantisation (opts->qstep and opts->guard_bits are not read; there is no max_u:
 * the guard bits are the caller's).  HTJ2K_ERR_EINVAL as there, and for values outside the ranges above. */
int    htj2k_enc_assemble_quant(int width, int height, int pix_fmt, int bits, const htj2k_enc_opts *opts,
                                const htj2k_enc_quant *quant, const uint8_t *const *block_bytes, const int *lcup,
                                const int *lref, const int *npasses, const int *planes, int nblocks,
                                uint8_t *out, size_t cap, size_t *out_len);

const char *htj2k_version(void);
/* name of the device the context is bound to, e.g. "gfx950" */
const char *htj2k_device_name(htj2k_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* HTJ2K_AMD_H */
