/*
 * htj2k_device.hip -- the C ABI of include/htj2k_amd.h: device management, the frame
 * pipeline (parse -> H2D -> HT decode -> IDWT -> MCT/pack -> D2H) and the kernel launches.
 *
 * Mirrors the plugin surface of `ff_jpeg2000_decoder` (libavcodec/jpeg2000dec.c:2926-2939):
 * htj2k_open = FFCodec.init, htj2k_decode = FFCodec.cb.decode (jpeg2000_decode_frame,
 * :2825-2908), htj2k_close = FFCodec.close.  There is no CPU fallback anywhere in this
 * library: without a usable HIP device htj2k_open fails with HTJ2K_ERR_ENOSYS.
 */
#include <hip/hip_runtime.h>
#include <assert.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/htj2k_amd.h"
#include "j2k_plan.h"
#include "ht_cxtvlc_rows.h"
#include "ht_kernels.hpp"
#include "dwt_kernels.hpp"
#include "pack_kernels.hpp"
#include "dwt_stream.hpp"
#include "mq_kernels.hpp"
#include "cmp_kernels.hpp"
#include "tensor_kernels.hpp"
#include "resize_kernels.hpp"
#include "mix_kernels.hpp"
#include "curve_kernels.hpp"
#include "mix_in_kernels.hpp"
#include "curve_in_kernels.hpp"
#include "j2k_enc.h"

using namespace htj2k;

/* ------------------------------------------------------------------ k_gather
 * Puts the byte pool together on the device from the uploaded packets: the host parser only emits the gather table
 * (J2kSeg, j2k_plan.h) and never touches a code-block byte.  One wavefront per code-block walks the block's pieces in
 * order; a piece goes from an arbitrary byte offset of the packet to its place in the 16-byte aligned region of the
 * block -- single bytes up to the first aligned destination dword, then a dword per lane from two aligned source
 * dwords (v_alignbyte), single bytes at the end -- and a terminated Part-1 segment gets its 0xFF 0xFF.  The pool was
 * cleared before, so the pads stay zero.  (jpeg2000dec.c:1508-1516 is the host loop this replaces in the reference:
 * bytestream2_get_bufferu into cblk->data, packet by packet.) */
__global__ void __launch_bounds__(256) k_gather(const J2kSeg *__restrict__ segs, const uint32_t *__restrict__ first_seg, int ngroups,
                                                 const uint8_t *__restrict__ pkt, const uint8_t *__restrict__ lit,
                                                 uint8_t *__restrict__ pool)
{
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= ngroups) return;
    const uint32_t s1 = first_seg[g + 1];
    for (uint32_t s = first_seg[g]; s < s1; s++) {
        const J2kSeg sg = segs[s];
        const uint8_t *src = ((sg.flags & J2K_SEG_LIT) ? lit : pkt) + sg.src;
        uint8_t *dst = pool + sg.dst;
        const uint32_t head = min(sg.len, (uint32_t)(-(intptr_t)dst & 3));
        if ((uint32_t)lane < head) dst[lane] = src[lane];
        const uint32_t body = (sg.len - head) >> 2, tail0 = head + 4 * body;
        const uint8_t *bs = src + head;
        const uint32_t sh = (uint32_t)((uintptr_t)bs & 3);
        const uint32_t *al = (const uint32_t *)(bs - sh);
        uint32_t *out = (uint32_t *)(dst + head);
        for (uint32_t k = lane; k < body; k += 64) {
            const uint32_t lo = al[k], hi = sh ? al[k + 1] : 0u;
            out[k] = __builtin_amdgcn_alignbyte(hi, lo, sh);
        }
        if ((uint32_t)lane < sg.len - tail0) dst[tail0 + lane] = src[tail0 + lane];
        if ((sg.flags & J2K_SEG_TERM) && lane < 2) dst[sg.len + lane] = 0xFF;
    }
}

#define LOG_ERROR 16
#define LOG_WARNING 24
#define LOG_INFO 32

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t n)
    {
        if (n <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = n + n / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return HTJ2K_ERR_ENOMEM; }
        cap = want;
        /* test aid: fresh device memory is not zero in a long-lived process; HTJ2K_POISON=1 makes every new buffer
         * start as 0xA5 bytes so that a read of memory no kernel wrote shows up at once (tools/gpu_random_configs.py) */
        static const bool poison = getenv("HTJ2K_POISON") && atoi(getenv("HTJ2K_POISON"));
        if (poison) {                                     /* (the fill runs on the null stream and need not have happened when
                                                            * hipMemset returns; the jobs' streams do not wait for that stream) */
            (void)hipMemset(p, 0xA5, want);
            (void)hipDeviceSynchronize();
        }
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct HostBuf {                       /* pinned host memory (async H2D at PCIe rate), grow-only */
    void *p = nullptr;
    size_t cap = 0;
    int device = 0;
    void *ensure(size_t n)
    {
        if (n <= cap) return p;
        /* called from the parse threads: bind the thread to the device only when something has to be
         * allocated (the first HIP call of a fresh thread costs milliseconds) */
        if (hipSetDevice(device) != hipSuccess) return nullptr;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        const size_t want = n + n / 4 + 4096;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; return nullptr; }
        cap = want;
        return p;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

/* idwt_x2 = 2: smaller LL bands make their round trip through the 256 MiB last-level cache, not through HBM, and the job
 * keeps its two launches */
#define X2_MIN_BYTES_DEFAULT (20 << 20)

struct htj2k_ctx {
    htj2k_opts opts;
    int device = 0;
    char devname[256];
    htj2k_log_fn log = nullptr;
    void *log_opaque = nullptr;
    uint16_t *d_tables = nullptr;      /* 2 x 1024 CxtVLC decode entries */
    J2kParser *probe_parser = nullptr;
    htj2k_job *own_job = nullptr;      /* used by htj2k_decode */
    htj2k_job *xc_job = nullptr;       /* the sources of htj2k_transcode_batch (htj2k_xc_*_) */
    htj2k_log_fn xc_log = nullptr;     /* ... and, while they are parsed, where the parsers' lines go as well: the encoder
                                        * context's log, so that the caller of the transcoder finds the reason in one place */
    void *xc_log_opaque = nullptr;
    htj2k_job *meas_job = nullptr;     /* the encoder's own streams of htj2k_encode_batch_measured (htj2k_meas_*_) */
    /* measuring frames (MeasCall): its stream and events, the results, table and uploaded operands, their pinned staging, the last launches' ms */
    hipStream_t cmp_stream = nullptr;
    hipEvent_t cmp_ev[2] = { nullptr, nullptr };
    DevBuf cmp_d;
    HostBuf cmp_h;
    float cmp_ms = 0;
    std::mutex cmp_mutex;              /* one comparison or hash at a time: a pipe's consumer hashes while other threads may compare */
    int ssim_rows = 0;                 /* block rows per strip of k_frame_ssim; 0: SSIM_ROWS_DEFAULT */
    int tensor_path = 0;               /* frames as tensors: 0 the fast route where a plane allows it, 1 the general route for everything */
    std::atomic<int> tensor_route{0};  /* the last tensor call's route, as htj2k_tensor_last_route answers it */
    int resize_rows = 0;               /* source rows per step of k_frame_resize; 0: RS_ROWS_DEFAULT */
    int curves_grid = 0;               /* source bytes a workgroup of a launch with curves reads, in table bytes; 0: CURVES_SRC_PER_TABLE */
    int resize_share = 0;              /* 1 .. 6: 1, 2, .. 32 lanes share a horizontal sum's taps; 0: resize_share() chooses */
    DevBuf mix_d;                      /* a resized call with a mix: k_frame_resize's float32 images, read by k_tensor_mix */
    int mix_scratch = 0;               /* the most bytes of mix_d a chunk of frames may take; 0: MIX_SCRATCH_DEFAULT */
    int idwt_mode = 3;                /* 0 = generic two-pass kernels, 1 = LDS tile kernel, 3 = register-streaming kernel (dwt_stream.hpp) */
    int fuse_pack = 1;                 /* idwt_mode 3, IDWT and pack stages run in one call: the final level writes the frame */
    int idwt_x3 = 1;                   /* 1: jobs with 16-bit LL bands run the first three 5/3 levels as one launch (k_idwt_stream_ll16_x3) */
    int idwt_x2 = 2;                   /* the last plain 5/3 level inside the final-level launch (k_idwt_stream_pack_x2): 0 never, 1 whenever
                                        * the job is eligible, 2 when the LL band that then stays on the CU is at least idwt_x2_min_bytes */
    int idwt_x2_th = 20;               /* ... final-level rows per workgroup */
    int idwt_x2_min_bytes = X2_MIN_BYTES_DEFAULT;
    int ht_pair = 1;                   /* 1: jobs with 16-bit sub-bands use k_ht_decode_pair (two blocks per wave, a lane per quad) */
    int ht_multi = 1;                  /* 1: jobs with 32-bit sub-bands whose HT blocks qualify use k_ht_decode_multi (2 or 4 blocks per wave) */
    int idwt_pk = 1;                   /* 1: fused final 5/3 levels of 8-bit pictures on pairs of 16-bit samples where the bounds allow (pk16_bounds) */
    int ll16_test_bits = 16;           /* tests: an LL sample "overflows" when it does not fit this many bits */
    int ll16 = 1;                      /* 1: such jobs also keep the LL bands between the IDWT levels as int16_t (overflow is detected
                                        * on the device and the transform run again with 32-bit LL bands, job_settle) */
    int coef16 = 1;                    /* 1: reversible jobs whose coefficients fit 16 bits keep them as int16_t between the
                                        * block decoder and the IDWT (see coef16_ok) */
    int ht_mode = 1;                   /* 0 = one kernel (serial stage on lane 0), 1 = k_ht_vlc (lane per block) + k_ht_decode<true> */
    int unit_ht = 0;                   /* the kernels htj2k_ht_blocks / _raw launch: 0 a fixed plain choice, 1 .. 4 a job's routes (ht_blocks) */
    int max_dyn_lds = 64 * 1024;
    bool x2_lds_ok = false;            /* k_idwt_stream_pack_x2 may take more than 48 KiB of dynamic LDS (lds_opt_in_all) */
    int parse_threads = 0;             /* host threads that parse the frames of a batch; 0 = min(cores, 16) */
    int packet_threads = 1;            /* > 1: a frame parsed on its own (htj2k_decode, batches of one) has the packets of tiles with a
                                        * PLT list read by this many threads (j2k_parser_set_packet_threads); off by default:
                                        * at 0.4 ms per 4K frame waking the threads costs what they save */
    int device_gather = 1;             /* 1: the packets are uploaded as they are and k_gather puts the byte pool together on the
                                        * device (the parser does not touch code-block bytes); 0: the parser gathers on the host */
    std::mutex log_mutex;
    std::atomic<int> refs{1};          /* the caller's, + one per pipe that is still open or has device frames out (htj2k_pipe.cpp) */
};

struct LevelLaunch {                   /* one IDWT launch: all planes (of all frames) of one type that have this level */
    int type, level;
    int count = 0;                     /* entries of its table: planes, or groups of a fused final level */
    size_t table_off = 0;              /* byte offset of its DwtLevel / DwtTileArgs table in d_desc */
    int max_lh = 0, max_lv = 0, min_l = 1 << 30;   /* min_l: smallest line length of any plane (1-sample lines need k_idwt_tile) */
    double alg_bytes = 0;              /* sum over its planes of 2 * 4 * lh * lv */
    double hbm_bytes = 0;              /* least HBM traffic: alg_bytes, or for a fused final level 4 * lh * lv read +
                                        * the frame bytes written */
    int nc = 0;                        /* 0: table of DwtTileArgs; 1/3/4: table of DwtFusedArgs (fused final level) */
    int outk = -1;                     /* fused level: the fast store all its entries qualify for (stream_fast_outk), -1: general path */
    bool all_fast = true;              /* every entry qualifies for the streaming kernels' fast path */
    int pk_bits = 0;                   /* fused 5/3 level with an 8-bit fast store: the packed 16-bit kernel is exact when its LL input fits
                                        * this many bits (pk16_bounds); 0: not at all */
    LevelLaunch(int type_, int level_) : type(type_), level(level_) {}
    void add(const DwtLevel &g)        /* one more plane */
    {
        max_lh = std::max(max_lh, g.lh); max_lv = std::max(max_lv, g.lv);
        min_l = std::min(min_l, std::min(g.lh, g.lv));
        alg_bytes += 8.0 * g.lh * g.lv;
        all_fast = all_fast && stream_fast_geom(g);
    }
};

/* What the content of a job and its descriptor tables determine about the IDWT and pack launches: written by
 * build_descriptors and pk16_eligibility, read by the stage code.  The rule is JobRun's, from the other side: a field that
 * follows from the content belongs here, one that describes a run belongs in JobRun, and what the stage code patches per
 * run (final_eff, h_desc, h_desc_dev, d_desc) stays on the job. */
struct IdwtPlan {
    std::vector<LevelLaunch> launches_generic, launches_tile;
    std::vector<LevelLaunch> launches_fused;   /* idwt_mode 3 with the pack stage fused into the final level */
    std::vector<uint8_t> tile_fusable;         /* per PackTile */
    std::vector<uint8_t> plane_fused;          /* per tilecomp: a fused IDWT run never writes its final plane */
    bool any_fusable = false;
    std::vector<int> final_buf;        /* per tilecomp, tile mode: 0 = coef, 1 = t0, 2 = t1 */
    bool tile_ok = true;               /* no empty levels: all planes of a launch ping-pong in step */
    size_t pack_off = 0; int npack = 0; int pack_maxw = 0, pack_maxh = 0;
    int pk_bits = 0;                   /* the LL bands of this job must fit this many bits for its packed 16-bit final levels (0: none) */
    /* k_idwt_stream_ll16_x3: the first three 5/3 levels of every plane in one launch (jobs with 16-bit LL bands) */
    struct X3 {
        bool ok = false;               /* the rest means something only with it */
        size_t tab[3] = { 0, 0, 0 };   /* the three levels' DwtTileArgs tables in d_desc (same planes, same order) */
        int count = 0, lh[3] = { 0, 0, 0 }, lv2 = 0;
        double alg = 0, hbm = 0;
    } x3;
    /* k_idwt_stream_pack_x2: the last plain 5/3 level and the fused rgb24 level as one launch */
    struct X2 {
        bool ok = false;               /* the rest means something only with it */
        int plain = -1, fused = -1;    /* the two entries of launches_fused */
        double alg = 0, hbm = 0, ll_bytes = 0;   /* ll_bytes: what the plain level would write */
    } x2;
};

struct FrameSlot {                     /* one frame of a batch */
    J2kParser *parser = nullptr;
    const J2kPlan *plan = nullptr;
    HostBuf h_pkt;                     /* device gather: the packet staged in pinned memory (the caller's is only borrowed for the call) */
    const uint8_t *h2d_src = nullptr;  /* ... or the caller's packet itself when that is page-locked (htj2k_job_parse_batch_ex) */
    bool h2d_own = false;              /* h2d_src is h_pkt (64 bytes of zero padding behind the packet) */
    size_t pkt_base = 0;               /* ... and where it goes in d_pkt */
    HostBuf h_bytes;                   /* host gather: the parser gathers the codeblock bytes straight into pinned memory */
    float ms_stage = 0, ms_parse = 0;  /* host time of the last parse_batch: staging copy, parser */
    uint32_t block_base = 0, tc_base = 0, sample_base = 0;
    size_t bytes_base = 0;
    DevBuf d_out[4];
    OutPlanes out;
};

/* ---- the block stage (un-stuff, k_ht_vlc / k_ht_vlc2, k_ht_refine, the k_ht_decode family, k_mq_decode) is set up in three
 * pieces that the jobs and the unit entry points (htj2k_ht_blocks, htj2k_mq_blocks) share: a host layout of the block table
 * (BlockLayout, block_layout), the device buffers with their sizes (BlockBufs, block_bufs_ensure, block_tables_upload) and
 * the kernel choice (HtChoice), which the launchers (launch_ht_blocks, launch_mq_blocks) take ---- */

/* Offsets in the tables that go to the device are 32-bit: samples, bytes of the pool and of the packets, gather segments,
 * quads, refinement masks, scratch rows.  A job or block table with more of any is refused (HTJ2K_ERR_PATCHWELCOME) */
static const size_t JOB_OFFSET_LIMIT = 0xFFFFFF00ull;

/* Host layout of a block table with HT blocks in [0, nht) and Part-1 (MQ-coded) blocks in [nht, n) */
struct BlockLayout {
    int nht = 0, n = 0;
    size_t nbytes = 0, nsamples = 0;   /* the byte pool and the coefficient buffer the descriptors point into */
    HtLds lds = {}, lds_ext = {};      /* the caller's: LDS layout of k_ht_decode<false>, and of k_ht_decode<true> (no VLC windows, no
                                        * tables), from the plans' figures (ht_lds_layout) or the table itself (build_ht_lds) */
    std::vector<uint32_t> qoff;        /* first quad of every block in d_qsym */
    size_t nquads = 0;
    std::vector<uint32_t> reflist, roff;   /* blocks with refinement passes that k_ht_refine handles; first mask of each in d_refbits */
    size_t nrefmasks = 0;
    uint32_t ref_max_w = 0;            /* widest block of reflist: k_ht_refine keeps 32-bit row masks when it is at most 32 */
    uint32_t ref_max_h = 0;            /* tallest: k_ht_decode_multi stages the SigProp masks of its blocks in LDS (at most 64 rows) */
    uint32_t max_lref = 0;             /* longest refinement segment of a coded HT block */
    std::vector<MqWave> mqwaves;       /* one per 64 Part-1 blocks */
    size_t mq_scratch_units = 0;       /* 512-byte row slots of k_mq_decode's scratch */
    uint32_t mq_planes = 1;            /* most bit-planes of a Part-1 block: sizes the LDS of k_mq_decode */
};

/* Device buffers of the block stage (sizes: block_bufs_ensure) */
struct BlockBufs {
    DevBuf d_bytes, d_blocks, d_status, d_coef, d_qsym, d_qoff, d_vlcu, d_melu, d_reflist, d_roff, d_refbits, d_mqwaves, d_mqscratch;
    void release()
    {
        for (DevBuf *b : { &d_bytes, &d_blocks, &d_status, &d_coef, &d_qsym, &d_qoff, &d_vlcu, &d_melu, &d_reflist, &d_roff, &d_refbits,
                           &d_mqwaves, &d_mqscratch })
            b->release();
    }
};

/* What the HT part of the block stage launches */
struct HtChoice {
    bool extended = false;             /* un-stuff, VLC, refine and MagSgn kernels; else the single k_ht_decode<false> (serial stage on lane 0) */
    bool vlc2 = false;                 /* k_ht_vlc2 (no block wider than 64 columns), else k_ht_vlc */
    int unstuff_g = 1;                 /* blocks per wave of the un-stuffing kernel (launch_unstuff) */
    enum { COLUMN, PAIR, MULTI } magsgn = COLUMN;   /* k_ht_decode<true>, k_ht_decode_pair, k_ht_decode_multi */
    int bpw = 1;                       /* ... and its blocks per wave: 1, 2 (pair), 2 or 4 (multi) */
    int multi_t = 0;                   /* k_ht_decode_multi: the transform all blocks share */
    bool coef16 = false;               /* the sub-bands are written as int16_t */
    bool raw = false;                  /* the RAW instantiations (every block carries J2K_DWT_RAW) */
};

/* What the runs of a job leave behind.  A parse, and an upload (which lays the buffers out anew), put a fresh JobRun in
 * its place (job_forget), so that what the accessors report (htj2k_job_coef16, _ll16, _idwt_packed, _ht_blocks_per_wave,
 * _idwt_launches, _stage_ms) and what a stage call may build on (coef_ok, planes_ok, fused_last) speak of runs of the
 * content the job holds now.  A field that describes a run belongs here, one that describes the content or follows from
 * the knobs does not: that is the whole rule. */
struct JobRun {
    int ran = 0;                       /* the stage masks of the runs so far: which of ev[2..5] htj2k_job_stage_ms may read */
    bool coef_is16 = false;            /* what the last HT stage run actually wrote */
    int ht_bpw = 0;                    /* ... and with how many blocks per wave in the MagSgn kernel */
    bool ll16_run = false;             /* the last IDWT run wrote its LL bands as int16_t ... */
    bool ll16_checked = true;          /* ... and the overflow flag behind d_status has been looked at since */
    int ll16_fallbacks = 0;            /* the last IDWT run overflowed and was run again (job_settle) */
    bool fused_last = false;           /* the last run used launches_fused */
    bool pk_run = false;               /* the last IDWT run took the packed kernels where a launch qualified (the knob idwt_pk) */
    int pk_used = 0;                   /* ... and launched a packed final level: the LL bands were checked against this many bits */
    /* what a stage call without the stages before it may build on (htj2k_job_run_stages) */
    bool coef_ok = false;              /* d_coef holds the sub-bands the block stage wrote (the generic IDWT works in place) */
    bool planes_ok = false;            /* every plane is where final_eff says: an IDWT run that was not fused, no block stage since */
    bool frames_ok = false;            /* the last run wrote the frames (its mask had the pack stage): what htj2k_job_compare reads */
    int lev_ev_used = 0;               /* the events of lev_ev that bracket the last run's IDWT launches */
    std::vector<double> lev_bytes, lev_hbm;   /* algorithmic / least-HBM bytes of each recorded launch */
};

struct htj2k_job : BlockBufs {         /* (the block stage's buffers as a base: the IDWT and pack code reads d_coef and d_status too) */
    std::vector<FrameSlot> frames;
    int nframes = 0;
    /* merged (re-based) tables of the whole batch */
    std::vector<J2kBlock> blocks;
    std::vector<J2kTileComp> tilecomps;
    std::vector<int> tc_frame;         /* frame index of each merged tile-component */
    size_t nbytes = 0, nsamples = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    std::vector<hipEvent_t> lev_ev;    /* per-IDWT-launch brackets (roofline measurement); a pool: the events are used again */
    JobRun run;
    DevBuf d_t0, d_t1, d_desc;
    BlockLayout lay;                   /* of `blocks`, which job_order_blocks has put in order: HT blocks first */
    /* every sample the block decoder writes fits int16_t and only the FASTONLY streaming IDWT kernels read them: all
     * planes coded, reversible 5/3 with at least one level, all blocks HT cleanup-only, <= 64 columns, M_b <= 15,
     * step size 1, no ROI shift, all levels of fast geometry.  The sub-bands then travel as 2 bytes per sample. */
    bool pair_ok = false;              /* ... and k_ht_decode_pair's dword stores are aligned: even widths, strides, offsets */
    int multi_nb = 0;                  /* k_ht_decode_multi: blocks per wave (2: blocks up to 64 columns, 4: up to 32), 0: not eligible */
    int multi_t = 0;                   /* ... and the transform all HT blocks of the job share */
    bool raw = false;                  /* the transcoder's job: every block carries J2K_DWT_RAW, the HT kernels are the RAW instantiations */
    bool coef16_ok = false;
    /* device gather: all packets of the batch, the parsers' literal bytes, the merged gather table, first piece of every block */
    bool dev_gather = false;
    DevBuf d_pkt, d_lit, d_gsegs, d_ggroups;
    std::vector<J2kSeg> gsegs;
    std::vector<uint32_t> ggroups;
    std::vector<uint8_t> lit;
    size_t pkt_bytes = 0;
    bool pkt_h2d_issued = false;       /* htj2k_job_parse_batch has sent the packets on their way already: the next upload does not */
    std::vector<uint8_t> h_desc;      /* host image of d_desc: level tables + pack tiles */
    std::vector<uint8_t> h_desc_dev;   /* ... and what d_desc holds (empty after a parse: the tables are rebuilt and d_desc may move) */
    IdwtPlan idwt;                     /* the launches those tables serve (build_descriptors) */
    int uploaded = 0;                  /* the content the job holds is on the device (htj2k_job_upload; a parse clears it) */
    std::vector<int> final_eff;        /* where each plane actually is after the last IDWT run */
};

static void clog(htj2k_ctx *c, int level, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    if (!c || !c->log) return;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->log(c->log_opaque, level, buf);
}

static void parser_log_tramp(void *opaque, int level, const char *msg)
{
    htj2k_ctx *c = (htj2k_ctx *)opaque;
    if (c && (c->log || c->xc_log)) {
        std::lock_guard<std::mutex> lk(c->log_mutex);      /* frames of a batch are parsed by several threads */
        if (c->log) c->log(c->log_opaque, level, msg);
        if (c->xc_log) c->xc_log(c->xc_log_opaque, level, msg);
    }
}

#define HIP_TRY(c, expr)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            clog(c, LOG_ERROR, "HIP error %s at %s:%d (%s)\n", hipGetErrorString(e_), __FILE__, __LINE__, #expr); \
            return e_ == hipErrorOutOfMemory ? HTJ2K_ERR_ENOMEM : HTJ2K_ERR_EXTERNAL;         \
        }                                                                                     \
    } while (0)

/* ------------------------------------------------------------------ CxtVLC decode tables
 * expanded on the host from the Annex C rows (the reference's dec_cxt_vlc_table0/1,
 * libavcodec/jpeg2000htdec.c:1342-1502, hold the same constants pre-expanded);
 * entry: bit0 u_off, bits1-3 len, 4-7 rho, 8-11 e_k, 12-15 e_1 (:320-327) */
static uint16_t h_tables[2][1024];
static void tbl_row(int t, int ctx, int rho, int uoff, int ek, int e1, int cwd, int len)
{
    uint16_t v = (uint16_t)(uoff | (len << 1) | (rho << 4) | (ek << 8) | (e1 << 12));
    for (int hi = 0; hi < (1 << (7 - len)); hi++)
        h_tables[t][(ctx << 7) | (hi << len) | cwd] = v;
}
#define DROW0(c, r, u, k, o, w, l) tbl_row(0, c, r, u, k, o, w, l);
#define DROW1(c, r, u, k, o, w, l) tbl_row(1, c, r, u, k, o, w, l);
static void build_tables()
{
    HT_CXTVLC_ROWS0(DROW0)
    HT_CXTVLC_ROWS1(DROW1)
}

/* ------------------------------------------------------------------ open / close */
extern "C" const char *htj2k_version(void) { return "htj2k-amd 0.1 (gfx950)"; }

/* Kernels that may be launched with more than 48 KiB of dynamic LDS are opted in once, here, to the most the device gives
 * a workgroup.  The attribute belongs to the function, not to a stream or a job: set per launch to what that launch needs,
 * two jobs of different geometry running on two threads of one context (the pipe's slots) could lower each other's value
 * between the call and the launch.  What a launch then asks for is checked where it is sized (ht_lds_layout,
 * launch_unstuff, run_idwt) and by the launch itself.  Returns whether k_idwt_stream_pack_x2 was opted in (run_idwt
 * falls back to two launches otherwise). */
static bool lds_opt_in_all(int cap)
{
    auto opt = [cap](const void *kern) {
        const bool ok = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, cap) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        return ok;
    };
    opt((const void *)k_ht_unstuff_g<16>); opt((const void *)k_ht_unstuff_g<32>); opt((const void *)k_ht_unstuff);
    opt((const void *)k_ht_decode<false>); opt((const void *)k_ht_decode_raw<false>);
    opt((const void *)k_ht_decode<true>); opt((const void *)k_ht_decode_raw<true>);
    opt((const void *)k_ht_vlc);
#define OPT_MULTI_T(NB_, T_) opt((const void *)k_ht_decode_multi<NB_, T_, true>); opt((const void *)k_ht_decode_multi<NB_, T_, false>)
#define OPT_MULTI(NB_) OPT_MULTI_T(NB_, J2K_DWT53); OPT_MULTI_T(NB_, J2K_DWT97); OPT_MULTI_T(NB_, J2K_DWT_RAW); OPT_MULTI_T(NB_, J2K_DWT97_INT)
    OPT_MULTI(2); OPT_MULTI(4);
#undef OPT_MULTI
#undef OPT_MULTI_T
    opt((const void *)k_idwt_stream_pack<J2K_DWT53, 3, true, true, true, 0, true>);
    opt((const void *)k_idwt_stream_pack<J2K_DWT53, 1, true, true, true, 2, true>);
    opt((const void *)k_idwt_stream_ll16_x3<true>); opt((const void *)k_idwt_stream_ll16_x3<false>);
    return opt((const void *)k_idwt_stream_pack_x2<3, 0, true>);
}

extern "C" int htj2k_open(const htj2k_opts *opts, htj2k_ctx **out)
{
    int ndev = 0;
    if (!out) return HTJ2K_ERR_EINVAL;
    *out = nullptr;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return HTJ2K_ERR_ENOSYS;                 /* no GPU: fail loudly, there is no CPU path */
    htj2k_ctx *c = new (std::nothrow) htj2k_ctx();
    if (!c) return HTJ2K_ERR_ENOMEM;
    memset(&c->opts, 0, sizeof(c->opts));
    c->opts.req_pix_fmt = HTJ2K_PIX_NONE;
    if (opts) c->opts = *opts;
    c->device = c->opts.device_id;
    if (c->device < 0 || c->device >= ndev) { delete c; return HTJ2K_ERR_EINVAL; }
    if (hipSetDevice(c->device) != hipSuccess) { delete c; return HTJ2K_ERR_ENOSYS; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) { delete c; return HTJ2K_ERR_ENOSYS; }
    snprintf(c->devname, sizeof(c->devname), "%s", prop.gcnArchName);
    c->max_dyn_lds = (int)prop.sharedMemPerBlock;
    c->x2_lds_ok = lds_opt_in_all(c->max_dyn_lds);
    build_tables();
    if (hipMalloc((void **)&c->d_tables, sizeof(h_tables)) != hipSuccess ||
        hipMemcpy(c->d_tables, h_tables, sizeof(h_tables), hipMemcpyHostToDevice) != hipSuccess) {
        delete c;
        return HTJ2K_ERR_ENOSYS;
    }
    c->probe_parser = j2k_parser_new();
    if (!c->probe_parser) { (void)hipFree(c->d_tables); delete c; return HTJ2K_ERR_ENOMEM; }
    const char *hm = getenv("HTJ2K_HT");
    if (hm && !strcmp(hm, "fused")) c->ht_mode = 0;
    if (hm && !strcmp(hm, "split")) c->ht_mode = 1;
    const char *m = getenv("HTJ2K_IDWT");
    if (m && !strcmp(m, "generic")) c->idwt_mode = 0;
    if (m && !strcmp(m, "tile")) c->idwt_mode = 1;
    if (m && !strcmp(m, "stream")) c->idwt_mode = 3;
    const char *l16 = getenv("HTJ2K_LL16");
    if (l16) c->ll16 = atoi(l16) ? 1 : 0;
    const char *pk = getenv("HTJ2K_PK");
    if (pk) c->idwt_pk = atoi(pk) ? 1 : 0;
    const char *fz = getenv("HTJ2K_FUSE");
    if (fz) c->fuse_pack = atoi(fz) != 0;
    *out = c;
    return 0;
}

extern "C" void htj2k_set_log(htj2k_ctx *c, htj2k_log_fn fn, void *opaque)
{
    if (!c) return;
    c->log = fn;
    c->log_opaque = opaque;
    j2k_parser_set_log(c->probe_parser, fn ? parser_log_tramp : nullptr, c);
}

extern "C" int htj2k_set_int(htj2k_ctx *c, const char *name, int value)
{
    if (!c || !name) return HTJ2K_ERR_EINVAL;
    if (!strcmp(name, "idwt_mode")) { c->idwt_mode = value <= 0 ? 0 : (value >= 3 ? 3 : 1); return 0; }
    if (!strcmp(name, "fuse_pack")) { c->fuse_pack = value ? 1 : 0; return 0; }
    if (!strcmp(name, "parse_threads")) { c->parse_threads = value < 0 ? 0 : (value > 64 ? 64 : value); return 0; }
    if (!strcmp(name, "ht_mode")) { c->ht_mode = value ? 1 : 0; return 0; }
    if (!strcmp(name, "device_gather")) { c->device_gather = value ? 1 : 0; return 0; }
    if (!strcmp(name, "packet_threads")) { c->packet_threads = value < 1 ? 1 : (value > 16 ? 16 : value); return 0; }
    if (!strcmp(name, "coef16")) { c->coef16 = value ? 1 : 0; return 0; }
    if (!strcmp(name, "ht_pair")) { c->ht_pair = value ? 1 : 0; return 0; }
    if (!strcmp(name, "idwt_x3")) { c->idwt_x3 = value ? 1 : 0; return 0; }
    if (!strcmp(name, "idwt_x2")) { c->idwt_x2 = value <= 0 ? 0 : (value >= 2 ? 2 : 1); return 0; }
    if (!strcmp(name, "idwt_x2_th")) { c->idwt_x2_th = std::max(4, std::min(4096, value)) & ~1; return 0; }
    if (!strcmp(name, "idwt_x2_min_bytes")) { c->idwt_x2_min_bytes = std::max(0, value); return 0; }
    if (!strcmp(name, "idwt_pk")) { c->idwt_pk = value ? 1 : 0; return 0; }
    if (!strcmp(name, "ht_multi")) { c->ht_multi = value ? 1 : 0; return 0; }
    if (!strcmp(name, "unit_ht")) { if (value < 0 || value > 4) return HTJ2K_ERR_EINVAL; c->unit_ht = value; return 0; }
    if (!strcmp(name, "ll16")) { c->ll16 = value ? 1 : 0; return 0; }
    if (!strcmp(name, "ll16_test_bits")) { if (value < 2 || value > 16) return HTJ2K_ERR_EINVAL; c->ll16_test_bits = value; return 0; }
    if (!strcmp(name, "ssim_rows")) { if (value < 0 || value > 256) return HTJ2K_ERR_EINVAL; c->ssim_rows = value; return 0; }
    if (!strcmp(name, "resize_rows")) { if (value < 0 || value > 16) return HTJ2K_ERR_EINVAL; c->resize_rows = value; return 0; }
    if (!strcmp(name, "curves_grid")) { if (value < 0 || value > 4096) return HTJ2K_ERR_EINVAL; c->curves_grid = value; return 0; }
    if (!strcmp(name, "resize_share")) { if (value < 0 || value > 6) return HTJ2K_ERR_EINVAL; c->resize_share = value; return 0; }
    if (!strcmp(name, "mix_scratch")) { if (value < 0) return HTJ2K_ERR_EINVAL; c->mix_scratch = value; return 0; }
    if (!strcmp(name, "tensor_path")) { if (value < 0 || value > 1) return HTJ2K_ERR_EINVAL; c->tensor_path = value; return 0; }
    if (!strcmp(name, "bitexact")) { c->opts.bitexact = value; return 0; }
    if (!strcmp(name, "reduction_factor")) { c->opts.reduction_factor = value; return 0; }
    return HTJ2K_ERR_EINVAL;
}

extern "C" const char *htj2k_device_name(htj2k_ctx *c) { return c ? c->devname : ""; }

extern "C" void *htj2k_host_alloc(htj2k_ctx *c, size_t size)
{
    void *p = nullptr;
    if (!c || !size || hipSetDevice(c->device) != hipSuccess) return nullptr;
    if (hipHostMalloc(&p, size, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

extern "C" void htj2k_host_free(htj2k_ctx *c, void *ptr)
{
    (void)c;
    if (ptr) (void)hipHostFree(ptr);
}

extern "C" int htj2k_device_to_host(htj2k_ctx *c, void *dst, const void *src, size_t size)
{
    if (!c || !dst || !src) return HTJ2K_ERR_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy(dst, src, size, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" void htj2k_job_free(htj2k_ctx *c, htj2k_job *j)
{
    (void)c;
    if (!j) return;
    if (j->stream) (void)hipStreamSynchronize(j->stream);
    j->BlockBufs::release();
    j->d_t0.release(); j->d_t1.release(); j->d_desc.release();
    j->d_pkt.release(); j->d_lit.release(); j->d_gsegs.release(); j->d_ggroups.release();
    for (FrameSlot &f : j->frames) {
        for (int i = 0; i < 4; i++) f.d_out[i].release();
        j2k_parser_free(f.parser);
        f.h_bytes.release();
        f.h_pkt.release();
    }
    for (int i = 0; i < 6; i++) if (j->ev[i]) (void)hipEventDestroy(j->ev[i]);
    for (hipEvent_t e : j->lev_ev) if (e) (void)hipEventDestroy(e);
    if (j->stream) (void)hipStreamDestroy(j->stream);
    delete j;
}

/* a pipe keeps its context alive: htj2k_close by the caller while a closed pipe still has device frames out (reference-
 * counted frames may outlive the decoder) must not free what those frames' release path needs */
extern "C" void htj2k_ctx_ref_(htj2k_ctx *c) { if (c) c->refs.fetch_add(1); }
/* htj2k_opts.frames_in_flight: the pipeline depth of a pipe opened with depth 0 */
extern "C" int htj2k_ctx_default_depth_(const htj2k_ctx *c)
{
    const int d = c ? c->opts.frames_in_flight : 0;
    return d <= 0 ? 3 : (d > 16 ? 16 : d);
}

extern "C" void htj2k_close(htj2k_ctx *c)
{
    if (c && c->refs.fetch_sub(1) != 1) return;            /* the last reference frees */
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->own_job) htj2k_job_free(c, c->own_job);
    if (c->xc_job) htj2k_job_free(c, c->xc_job);
    if (c->meas_job) htj2k_job_free(c, c->meas_job);
    if (c->cmp_stream) { (void)hipStreamSynchronize(c->cmp_stream); (void)hipStreamDestroy(c->cmp_stream); }
    for (hipEvent_t e : c->cmp_ev) if (e) (void)hipEventDestroy(e);
    c->cmp_d.release(); c->cmp_h.release(); c->mix_d.release();
    if (c->d_tables) (void)hipFree(c->d_tables);
    j2k_parser_free(c->probe_parser);
    delete c;
}

extern "C" int htj2k_probe(htj2k_ctx *c, const uint8_t *pkt, int size, htj2k_info *info)
{
    const J2kPlan *pl = nullptr;
    if (!c || !pkt || !info) return HTJ2K_ERR_EINVAL;
    int ret = j2k_parse(c->probe_parser, pkt, size, &c->opts, 1, &pl);
    if (ret < 0) return ret;
    *info = pl->info;
    return 0;
}

/* ------------------------------------------------------------------ job: parse
 * A job holds a batch of frames.  Every frame is parsed by its own parser; the descriptor tables are then concatenated
 * (offsets re-based into one device arena) so that each stage of the whole batch is a single launch: frames are
 * independent, so a batch is simply a longer codeblock table, more planes per IDWT level, more tiles to pack.
 * htj2k_job_parse_batch_ex at the end of this section is the list of steps; each step is a function above it. */
static int job_new(htj2k_ctx *c, htj2k_job **out)
{
    htj2k_job *j = new (std::nothrow) htj2k_job();
    if (!j) return HTJ2K_ERR_ENOMEM;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&j->stream, hipStreamNonBlocking) != hipSuccess) {
        delete j; return HTJ2K_ERR_EXTERNAL;
    }
    for (int i = 0; i < 6; i++)
        if (hipEventCreate(&j->ev[i]) != hipSuccess) { htj2k_job_free(c, j); return HTJ2K_ERR_EXTERNAL; }
    *out = j;
    return 0;
}

/* one packet -> its place in d_pkt, asynchronously on the job's stream.  A staging copy of ours carries its 64 bytes of zero
 * padding; a caller's page-locked packet is read up to its last byte only and the padding is set on the device (k_gather reads
 * whole dwords, up to 3 bytes past a segment) */
static hipError_t job_packet_h2d(htj2k_job *j, const FrameSlot &F, size_t size)
{
    uint8_t *dst = (uint8_t *)j->d_pkt.p + F.pkt_base;
    hipError_t e = hipMemcpyAsync(dst, F.h2d_src, size + (F.h2d_own ? 64 : 0), hipMemcpyHostToDevice, j->stream);
    if (e == hipSuccess && !F.h2d_own) e = hipMemsetAsync(dst + size, 0, 64, j->stream);
    return e;
}

/* the slot of a packet in d_pkt: the packet and its 64 bytes of padding, rounded up to 16 */
static size_t pkt_slot(size_t size) { return (size + 64 + 15) & ~(size_t)15; }
/* the bytes of a packet the caller gives this size: what the parser reads of it (pl->pkt_size, j2k_plan.c: j2k_parse) */
static size_t pkt_len(int size) { return size > 0 ? (size_t)size : 0; }

/* Where every packet goes in d_pkt follows from the sizes alone, so it is settled before anything is parsed: the early
 * H2D, the solo path, the merge and the upload all take pkt_base and pkt_bytes from here.  False: the packets do not fit
 * the 32-bit offsets of the gather table (the merge refuses such a job) */
static bool job_place_packets(htj2k_job *j, const int *sizes, int n)
{
    size_t total = 0;
    bool fits = true;
    for (int f = 0; f < n; f++) {
        j->frames[f].pkt_base = total;
        total += pkt_slot(pkt_len(sizes[f]));
        if (total > JOB_OFFSET_LIMIT) fits = false;
    }
    j->pkt_bytes = total;
    return fits;
}

/* A parse, and an upload (which lays the buffers out anew), leave nothing of earlier runs behind (JobRun) */
static void job_forget(htj2k_job *j) { j->run = JobRun(); }

struct ParseCall {                     /* one call of htj2k_job_parse_batch_ex, as its steps see it */
    htj2k_ctx *c; htj2k_job *j;
    const uint8_t *const *pkts; const int *sizes; const uint8_t *pinned;
    int n, nthreads;
    bool places_fit;                   /* job_place_packets */
    std::vector<const uint8_t *> src;  /* what the parsers read: the caller's packets, or the staged copies of them */
    std::vector<int> rc;               /* per frame: the refusal of a step */
};

/* the first failing frame in submission order decides, whatever thread found it and when */
static int first_error(const std::vector<int> &rc) { for (int r : rc) if (r < 0) return r; return 0; }

/* fn(f) for every frame f of [0, n) on nthreads host threads, the caller's own among them; a thread that comes free takes
 * the next frame (frames are independent: SURVEY 8f rank 1) */
template <class Fn>
static void parallel_frames(int nthreads, int n, Fn &&fn)
{
    std::atomic<int> next(0);
    auto work = [&]() {
        for (;;) {
            const int f = next.fetch_add(1);
            if (f >= n) break;
            fn(f);
        }
    };
    if (nthreads <= 1) {
        work();
    } else {
        std::vector<std::thread> pool;
        for (int t = 1; t < nthreads; t++) pool.emplace_back(work);
        work();
        for (std::thread &t : pool) t.join();
    }
}

/* Step: the frames' slots, a parser each and the parsers' hooks.  Host gather: the parser gathers the codeblock bytes
 * straight into pinned memory (h_bytes); device gather: the packet is staged in pinned memory as it is (h_pkt).  Either
 * way the H2D copy of the upload then runs at PCIe rate and truly asynchronously.  The allocation hook is registered again
 * on every call: the FrameSlot may have moved when the vector grew.  packet_threads is for a frame on its own only:
 * batches have one frame per thread instead */
static int prepare_frames(htj2k_ctx *c, htj2k_job *j, int n)
{
    if ((int)j->frames.size() < n) j->frames.resize(n);
    for (int f = 0; f < n; f++) {
        FrameSlot &F = j->frames[f];
        if (!F.parser) {
            F.parser = j2k_parser_new();
            if (!F.parser) return HTJ2K_ERR_ENOMEM;
            j2k_parser_set_log(F.parser, parser_log_tramp, c);
        }
        F.h_bytes.device = c->device;
        F.h_pkt.device = c->device;
        j2k_parser_set_gather(F.parser, !j->dev_gather);
        j2k_parser_set_packet_threads(F.parser, n == 1 ? c->packet_threads : 1);
        j2k_parser_set_bytes_alloc(F.parser, [](void *opaque, size_t nb) -> void * { return ((HostBuf *)opaque)->ensure(nb); },
                                   &F.h_bytes);
        F.plan = nullptr;
    }
    return 0;
}

/* Step, the solo path: one frame on its own (htj2k_decode) whose packet is pageable, at least SOLO_MIN_BYTES long and
 * gathered on the device.  The staging copy of a 4K packet (15.7 MB, 0.55 ms on one core) was the longest item of the
 * call.  Helper threads copy it in pieces of SOLO_PIECE_BYTES, each piece goes to the device as soon as it is in page-
 * locked memory, and this thread meanwhile parses the caller's packet itself -- the parser reads headers only and, with
 * the device gathering, nothing looks at the packet again after the parse.  The stage time is the wall time of the step
 * less the parse.  1: done; 0: not taken (also when d_pkt cannot be had: the general path then tries again); < 0: refused */
static const int SOLO_MIN_BYTES = 4 << 20;
static const size_t SOLO_PIECE_BYTES = 2 << 20;

static int parse_solo(ParseCall &P)
{
    htj2k_ctx *c = P.c;
    htj2k_job *j = P.j;
    if (!j->dev_gather || P.n != 1 || (P.pinned && P.pinned[0]) || P.sizes[0] < SOLO_MIN_BYTES ||
        hipSetDevice(c->device) != hipSuccess) return 0;
    FrameSlot &F = j->frames[0];
    const uint8_t *pkt = P.pkts[0];
    const size_t sz = (size_t)P.sizes[0];
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t *h = (uint8_t *)F.h_pkt.ensure(sz + 64);
    if (!h) return HTJ2K_ERR_ENOMEM;
    if (j->d_pkt.ensure(j->pkt_bytes + 256) != 0) return 0;
    uint8_t *d = (uint8_t *)j->d_pkt.p + F.pkt_base;
    F.h2d_src = h; F.h2d_own = true;
    const size_t piece = SOLO_PIECE_BYTES, npieces = (sz + piece - 1) / piece;
    const int nhelp = std::thread::hardware_concurrency() > 1 ? 3 : 1;
    std::atomic<size_t> nextp(0);
    std::atomic<int> bad(0);
    auto copy_pieces = [&]() {
        if (hipSetDevice(c->device) != hipSuccess) { bad = 1; return; }
        for (;;) {
            const size_t k = nextp.fetch_add(1);
            if (k >= npieces) break;
            const size_t off = k * piece, len = std::min(piece, sz - off), pad = k + 1 == npieces ? 64 : 0;
            memcpy(h + off, pkt + off, len);
            if (pad) memset(h + sz, 0, 64);
            if (hipMemcpyAsync(d + off, h + off, len + pad, hipMemcpyHostToDevice, j->stream) != hipSuccess) bad = 1;
        }
    };
    std::vector<std::thread> helpers;
    for (int t = 0; t < nhelp; t++) helpers.emplace_back(copy_pieces);
    const auto t1 = std::chrono::steady_clock::now();
    const int rc = j2k_parse(F.parser, pkt, P.sizes[0], &c->opts, 0, &F.plan);
    F.ms_parse = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
    for (std::thread &t : helpers) t.join();
    F.ms_stage = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count() - F.ms_parse;
    if (bad) return HTJ2K_ERR_EXTERNAL;
    if (rc < 0) return rc;
    j->pkt_h2d_issued = true;
    return 1;
}

/* Step, device gather: every packet into page-locked memory with its 64 bytes of zero padding, unless the caller's
 * already is page-locked and stable -- the upload then reads the packet itself.  F.ms_stage is this copy */
static int stage_packets(ParseCall &P)
{
    parallel_frames(P.nthreads, P.n, [&](int f) {
        FrameSlot &F = P.j->frames[f];
        const auto t0 = std::chrono::steady_clock::now();
        F.h2d_src = nullptr;
        F.h2d_own = !(P.pinned && P.pinned[f]);
        if (F.h2d_own) {
            const size_t sz = pkt_len(P.sizes[f]);
            uint8_t *h = (uint8_t *)F.h_pkt.ensure(sz + 64);
            if (!h) { P.rc[f] = HTJ2K_ERR_ENOMEM; return; }
            memcpy(h, P.src[f], sz);
            memset(h + sz, 0, 64);
            P.src[f] = h;
        }
        F.h2d_src = P.src[f];
        F.ms_stage = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    });
    return first_error(P.rc);
}

/* Step, device gather: the staged packets on their way to the device BEFORE they are parsed.  Their places are known and
 * the parser needs nothing from the device, so the transfer of a frame (0.35 ms for a 4K frame) runs under its parse
 * (0.36 ms) instead of behind it.  Where this cannot be done (d_pkt not to be had, a copy refused) the upload sends them */
static void send_packets_early(ParseCall &P)
{
    htj2k_job *j = P.j;
    if (!P.places_fit || hipSetDevice(P.c->device) != hipSuccess || j->d_pkt.ensure(j->pkt_bytes + 256) != 0) return;
    bool ok = true;
    for (int f = 0; f < P.n && ok; f++) ok = job_packet_h2d(j, j->frames[f], pkt_len(P.sizes[f])) == hipSuccess;
    j->pkt_h2d_issued = ok;
}

/* Step: the parsers, a frame per thread; F.ms_parse is the parser's time */
static int parse_frames(ParseCall &P)
{
    parallel_frames(P.nthreads, P.n, [&](int f) {
        FrameSlot &F = P.j->frames[f];
        const auto t1 = std::chrono::steady_clock::now();
        P.rc[f] = j2k_parse(F.parser, P.src[f], P.sizes[f], &P.c->opts, 0, &F.plan);
        F.ms_parse = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
        if (!P.j->dev_gather) F.ms_stage = 0;
    });
    return first_error(P.rc);
}

/* Step, the merge: the frames' tables become the job's.  Blocks and tile-components move to the frame's part of the
 * coefficient buffer and of the byte pool; with device gather the frame's gather table joins the job's, sources re-based to
 * where the packet (pkt_base) or the literal bytes will sit on the device, destinations to the frame's part of the pool.
 * What does not fit 32-bit offsets is refused (JOB_OFFSET_LIMIT) */
static int merge_plans(htj2k_job *j, int n)
{
    size_t nbytes = 0, nsamples = 0;
    j->blocks.clear(); j->tilecomps.clear(); j->tc_frame.clear();
    j->gsegs.clear(); j->ggroups.clear(); j->lit.clear();
    for (int f = 0; f < n; f++) {
        FrameSlot &F = j->frames[f];
        const J2kPlan *pl = F.plan;
        if (nsamples + pl->nsamples > JOB_OFFSET_LIMIT || nbytes + pl->nbytes > JOB_OFFSET_LIMIT) return HTJ2K_ERR_PATCHWELCOME;
        F.block_base = (uint32_t)j->blocks.size();
        F.tc_base = (uint32_t)j->tilecomps.size();
        F.sample_base = (uint32_t)nsamples;
        nbytes += 16;                                  /* k_ht_unstuff's backward dword loads may start up to 3 bytes
                                                        * in front of a block: never in front of the buffer */
        F.bytes_base = nbytes;
        for (int i = 0; i < pl->nblocks; i++) {
            J2kBlock b = pl->blocks[i];
            b.data_off += (uint32_t)nbytes;
            b.plane_off += (uint32_t)nsamples;
            b.tcomp = (uint8_t)(b.tcomp + F.tc_base);          /* informational only (wraps beyond 255 tile-components) */
            j->blocks.push_back(b);
        }
        for (int t = 0; t < pl->ntilecomps; t++) {
            J2kTileComp tc = pl->tilecomps[t];
            tc.plane_off += (uint32_t)nsamples;
            j->tilecomps.push_back(tc);
            j->tc_frame.push_back(f);
        }
        if (j->dev_gather) {
            if (F.pkt_base + (size_t)pl->pkt_size > JOB_OFFSET_LIMIT || j->lit.size() + pl->nlit > JOB_OFFSET_LIMIT ||
                j->gsegs.size() + pl->nsegs > JOB_OFFSET_LIMIT)
                return HTJ2K_ERR_PATCHWELCOME;
            const uint32_t lit_base = (uint32_t)j->lit.size(), seg_base = (uint32_t)j->gsegs.size();
            for (uint32_t k = 0; k < pl->nsegs; k++) {
                J2kSeg g = pl->segs[k];
                g.src += (g.flags & J2K_SEG_LIT) ? lit_base : (uint32_t)F.pkt_base;
                g.dst += (uint32_t)nbytes;
                j->gsegs.push_back(g);
            }
            for (int i = 0; i < pl->nblocks; i++) j->ggroups.push_back(seg_base + pl->blk_seg0[i]);
            j->lit.insert(j->lit.end(), pl->lit, pl->lit + pl->nlit);
        }
        nbytes += (pl->nbytes + 63) & ~(size_t)63;
        nsamples += pl->nsamples;
    }
    if (j->dev_gather) j->ggroups.push_back((uint32_t)j->gsegs.size());
    j->nbytes = nbytes;
    j->nsamples = nsamples;
    return 0;
}

/* The steps above, in order; a refused call leaves a job without frames (nframes 0) that the next parse may use */
extern "C" int htj2k_job_parse_batch_ex(htj2k_ctx *c, const uint8_t *const *pkts, const int *sizes, int n, const uint8_t *pinned,
                                        htj2k_job **job)
{
    int r;
    if (!c || !pkts || !sizes || n <= 0 || !job) return HTJ2K_ERR_EINVAL;
    if (!*job && (r = job_new(c, job)) < 0) return r;
    htj2k_job *j = *job;
    /* the previous batch of this job may still be in flight and reads the parsers' arenas */
    if (hipStreamSynchronize(j->stream) != hipSuccess) return HTJ2K_ERR_EXTERNAL;
    j->uploaded = 0;
    job_forget(j);
    j->raw = false;
    j->nframes = 0;
    j->dev_gather = c->device_gather != 0;
    if ((r = prepare_frames(c, j, n)) < 0) return r;
    ParseCall P = { c, j, pkts, sizes, pinned, n, 0, false, std::vector<const uint8_t *>(pkts, pkts + n), std::vector<int>(n, 0) };
    P.nthreads = c->parse_threads > 0 ? c->parse_threads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (P.nthreads > n) P.nthreads = n;
    P.places_fit = j->dev_gather && job_place_packets(j, sizes, n);
    if ((r = parse_solo(P)) < 0) return r;
    if (!r) {                                              /* the general path */
        j->pkt_h2d_issued = false;
        if (j->dev_gather) {
            if ((r = stage_packets(P)) < 0) return r;
            send_packets_early(P);
        }
        if ((r = parse_frames(P)) < 0) return r;
    }
    if ((r = merge_plans(j, n)) < 0) return r;
    j->nframes = n;
    return 0;
}

extern "C" int htj2k_job_parse_batch(htj2k_ctx *c, const uint8_t *const *pkts, const int *sizes, int n, htj2k_job **job)
{
    return htj2k_job_parse_batch_ex(c, pkts, sizes, n, nullptr, job);
}

extern "C" int htj2k_job_parse(htj2k_ctx *c, const uint8_t *pkt, int size, htj2k_job **job)
{
    const uint8_t *pk[1] = { pkt };
    int sz[1] = { size };
    if (!pkt) return HTJ2K_ERR_EINVAL;
    return htj2k_job_parse_batch(c, pk, sz, 1, job);
}

extern "C" int htj2k_job_num_frames(const htj2k_job *j) { return j ? j->nframes : HTJ2K_ERR_EINVAL; }

extern "C" int htj2k_job_host_ms(const htj2k_job *j, float *ms_parse, float *ms_stage)
{
    if (!j || j->nframes <= 0) return HTJ2K_ERR_EINVAL;
    float p = 0, s = 0;
    for (int f = 0; f < j->nframes; f++) { p += j->frames[f].ms_parse; s += j->frames[f].ms_stage; }
    if (ms_parse) *ms_parse = p / j->nframes;
    if (ms_stage) *ms_stage = s / j->nframes;
    return 0;
}

extern "C" int htj2k_job_frame_info(const htj2k_job *j, int frame, htj2k_info *info)
{
    if (!j || frame < 0 || frame >= j->nframes || !j->frames[frame].plan || !info) return HTJ2K_ERR_EINVAL;
    *info = j->frames[frame].plan->info;
    return 0;
}
extern "C" int htj2k_job_info(const htj2k_job *j, htj2k_info *info) { return htj2k_job_frame_info(j, 0, info); }
extern "C" int htj2k_job_bytes_consumed(const htj2k_job *j)
{
    return j && j->nframes > 0 && j->frames[0].plan ? j->frames[0].plan->bytes_consumed : HTJ2K_ERR_EINVAL;
}
extern "C" int htj2k_job_num_tilecomps(const htj2k_job *j) { return j && j->nframes ? (int)j->tilecomps.size() : HTJ2K_ERR_EINVAL; }
extern "C" int htj2k_job_num_blocks(const htj2k_job *j) { return j && j->nframes ? (int)j->blocks.size() : HTJ2K_ERR_EINVAL; }
extern "C" int htj2k_job_tilecomp_dims(const htj2k_job *j, int tc, int *w, int *h, int *is_float)
{
    if (!j || !j->nframes || tc < 0 || tc >= (int)j->tilecomps.size()) return HTJ2K_ERR_EINVAL;
    if (w) *w = j->tilecomps[tc].w;
    if (h) *h = j->tilecomps[tc].h;
    if (is_float) *is_float = j->tilecomps[tc].transform == J2K_DWT97;
    return 0;
}

/* ------------------------------------------------------------------ job: upload */
static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/* LDS windows of the HT kernel are sized from the largest cleanup prefix / suffix, quad row
 * and (for blocks with refinement passes) state bitmap in the table */
static int ht_lds_layout(htj2k_ctx *c, uint32_t max_p, uint32_t max_s, uint32_t max_qw, uint32_t bm_words, HtLds *out, HtLds *out_ext)
{
    HtLds &L = *out;
    size_t off = 4096;                                   /* the two CxtVLC tables */
    L.ms_words = ((max_p * 8 + 31) / 32 + 3 + 3) & ~3u;  /* a multiple of 4: the kernels clear the array 16 bytes per lane */
    L.off_ms = (uint32_t)off;  off += (size_t)L.ms_words * 4;
    L.vlc_words = (max_s * 8 + 31) / 32 + 2;
    L.off_vlc = (uint32_t)off; off += (size_t)L.vlc_words * 4;
    L.suf_bytes = (uint32_t)align_up(max_s, 4);
    L.off_suf = (uint32_t)off; off += L.suf_bytes;
    L.max_qw = max_qw;
    L.off_qinfo = (uint32_t)off; off += (size_t)2 * max_qw * 4;
    L.off_E = (uint32_t)off;   off += align_up((size_t)2 * (2 * max_qw + 8), 4);
    L.bm_words = bm_words;
    L.off_bm = (uint32_t)off;  off += (size_t)4 * bm_words * 4;
    L.total = (uint32_t)align_up(off, 16);
    if (out_ext) {                                       /* MagSgn-only kernel: bit array, exponents, bitmaps */
        HtLds &X = *out_ext;
        size_t o = 0;
        X = L;
        X.off_ms = 0; o += (size_t)X.ms_words * 4;
        X.off_vlc = (uint32_t)o; X.vlc_words = 0;
        X.off_suf = (uint32_t)o; X.suf_bytes = 0;
        X.off_qinfo = (uint32_t)o; o += (size_t)2 * max_qw * 4;
        X.off_E = (uint32_t)o; o += align_up((size_t)2 * (2 * max_qw + 8), 4);
        X.off_bm = (uint32_t)o; o += (size_t)4 * bm_words * 4;
        X.total = (uint32_t)align_up(o, 16);
    }
    if ((int)L.total > 160 * 1024) {
        clog(c, LOG_ERROR, "a codeblock needs %u bytes of LDS\n", L.total);
        return HTJ2K_ERR_PATCHWELCOME;
    }
    return 0;
}

/* LDS sizing from a block table + byte pool (unit entry point; jobs take the figures from the plans) */
static int build_ht_lds(htj2k_ctx *c, const J2kBlock *blocks, int nblocks, const uint8_t *pool, HtLds *out, HtLds *out_ext)
{
    uint32_t max_p = 0, max_s = 2, max_qw = 1, bm_words = 0;
    for (int i = 0; i < nblocks; i++) {
        const J2kBlock &b = blocks[i];
        if (!b.npasses) continue;
        uint32_t qw = (b.w + 1u) >> 1;
        if (qw > max_qw) max_qw = qw;
        if (b.lcup >= 2) {
            const uint8_t *D = pool + b.data_off;
            uint32_t scup = ((uint32_t)D[b.lcup - 1] << 4) + (D[b.lcup - 2] & 0x0F);
            if (scup >= 2 && scup <= b.lcup && scup <= 4079) {
                if (scup > max_s) max_s = scup;
                if (b.lcup - scup > max_p) max_p = b.lcup - scup;
            }
        }
        int rem = b.npasses % 3, plhd = rem ? b.npasses - rem : b.npasses - 3;
        if (b.npasses - plhd > 1) {
            uint32_t wds = ((uint32_t)(b.w + 2) * (b.h + 2) + 31) / 32 + 1;
            if (wds > bm_words) bm_words = wds;
        }
    }
    return ht_lds_layout(c, max_p, max_s, max_qw, bm_words, out, out_ext);
}

/* Which blocks k_ht_refine handles (SigProp / MagRef passes, at most 64 columns, no ROI shift) and where their masks
 * go: the block on lane l of the kernel's wave g (reflist[64 g + l]) has mask k of row y at
 * roff[block] + (3 y + k) * HT_REF_STRIDE, roff[block] = base of wave g + l; a wave takes 64 * 3 * (its tallest block)
 * words.  Returns the total in 64-bit words; *max_w = the widest such block. */
static size_t ref_layout(const J2kBlock *blocks, size_t nblocks, std::vector<uint32_t> &reflist, std::vector<uint32_t> &roff, uint32_t *max_w,
                         uint32_t *max_h = nullptr)
{
    reflist.clear();
    roff.assign(nblocks + 1, 0);
    *max_w = 0;
    if (max_h) *max_h = 0;
    for (size_t i = 0; i < nblocks; i++) {
        const J2kBlock &b = blocks[i];
        const int rem = b.npasses % 3, plhd = rem ? b.npasses - rem : b.npasses - 3;
        if (b.npasses && !(b.flags & J2K_BLK_PART1) && b.npasses - plhd > 1 && b.w <= 64 && b.roi_shift == 0) {
            reflist.push_back((uint32_t)i);
            if (b.w > *max_w) *max_w = b.w;
            if (max_h && b.h > *max_h) *max_h = b.h;
        }
    }
    size_t nm = 0;
    for (size_t g = 0; g < reflist.size(); g += 64) {
        uint32_t hmax = 0;
        for (size_t l = g; l < std::min(g + 64, reflist.size()); l++) hmax = std::max<uint32_t>(hmax, blocks[reflist[l]].h);
        for (size_t l = g; l < std::min(g + 64, reflist.size()); l++) roff[reflist[l]] = (uint32_t)(nm + (l - g));
        nm += (size_t)HT_REF_STRIDE * 3 * hmax;
    }
    return nm;
}

/* Where every block's quad symbols and refinement masks go, and the Part-1 blocks in waves of 64 (the offsets are 32-bit
 * on the device).  L.lds and L.lds_ext are the caller's to fill. */
static int block_layout(const J2kBlock *blocks, int nht, int n, size_t nbytes, size_t nsamples, BlockLayout &L)
{
    L.nht = nht; L.n = n; L.nbytes = nbytes; L.nsamples = nsamples;
    L.qoff.resize((size_t)n + 1);
    L.max_lref = 0;
    size_t q = 0;
    for (int i = 0; i < n; i++) {
        const J2kBlock &b = blocks[i];
        L.qoff[i] = (uint32_t)q;
        if (i < nht && b.npasses) {
            q += ht_qsym_words(b.w, b.h);
            L.max_lref = std::max<uint32_t>(L.max_lref, b.lref);
        }
    }
    if (q > JOB_OFFSET_LIMIT) return HTJ2K_ERR_PATCHWELCOME;
    L.nquads = q;
    /* blocks with SigProp / MagRef passes go through k_ht_refine (one lane per block) when
     * k_ht_decode's row-mask path can take them: up to 64 columns, no ROI shift */
    const size_t nm = ref_layout(blocks, (size_t)n, L.reflist, L.roff, &L.ref_max_w, &L.ref_max_h);
    if (nm > JOB_OFFSET_LIMIT) return HTJ2K_ERR_PATCHWELCOME;
    L.nrefmasks = nm;
    L.mqwaves.clear();
    L.mq_planes = 1;
    size_t units = 0;
    for (int i = nht; i < n; i += 64) {
        MqWave W;
        int hmax = 0, wmax = 0, pmax = 0;
        for (int k = i; k < std::min(i + 64, n); k++) {
            const J2kBlock &b = blocks[k];
            hmax = std::max<int>(hmax, b.h); wmax = std::max<int>(wmax, b.w); pmax = std::max<int>(pmax, b.npasses);
        }
        const int planes = std::min((pmax + 1) / 3 + 1, 32);
        W.hmax = (uint16_t)hmax; W.wmax = (uint16_t)wmax; W.pmax = (uint16_t)pmax;
        W.rows = (uint16_t)(((hmax + 3) & ~3) + 2);
        W.chunks = (uint16_t)((wmax + 63) / 64);
        W.pad = 0;
        if (units > JOB_OFFSET_LIMIT) return HTJ2K_ERR_PATCHWELCOME;
        W.soff = (uint32_t)units;
        units += (size_t)(4 + planes) * W.rows * W.chunks;
        L.mq_planes = std::max<uint32_t>(L.mq_planes, (uint32_t)planes);
        L.mqwaves.push_back(W);
    }
    L.mq_scratch_units = units;
    return 0;
}

/* The coefficient buffer (and the IDWT's two of its size) ends in 64 spare words: the MagSgn kernels send the stores of
 * rows and columns a block does not have to a sink 32 words behind the samples */
static size_t coef_buf_bytes(size_t nsamples) { return (nsamples + 64) * sizeof(uint32_t); }

static int block_bufs_ensure(BlockBufs &B, const BlockLayout &L)
{
    int r;
    if ((r = B.d_bytes.ensure(L.nbytes + 256)) < 0) return r;          /* k_mq_decode's 128-byte windows start inside a block */
    if (!L.mqwaves.empty() &&
        ((r = B.d_mqwaves.ensure(L.mqwaves.size() * sizeof(MqWave))) < 0 ||
         (r = B.d_mqscratch.ensure(L.mq_scratch_units * 512 + 512)) < 0)) return r;
    if ((r = B.d_blocks.ensure((size_t)(L.n + 1) * sizeof(J2kBlock))) < 0) return r;
    if ((r = B.d_status.ensure((size_t)(L.n + 1) * sizeof(int))) < 0) return r;   /* + 1: the LL overflow flag of the IDWT */
    if ((r = B.d_coef.ensure(coef_buf_bytes(L.nsamples))) < 0) return r;
    /* + the scratch line of k_ht_vlc's flush, + what k_ht_decode_pair's symbol preload reads past the last block (32 rows of 34) */
    if ((r = B.d_qsym.ensure(L.nquads * sizeof(ht_sym_t) + 256 + 8192)) < 0) return r;
    if ((r = B.d_qoff.ensure((L.qoff.size() + 1) * sizeof(uint32_t))) < 0) return r;
    /* a corrupt block can run k_ht_vlc's bit positions past its own arrays (38 VLC / 18 MEL bits per quad pair at
     * most, 4096 samples per block: < 3 KB): the last block of the pool must still read inside the allocation */
    if ((r = B.d_vlcu.ensure(L.nbytes + 16384)) < 0 || (r = B.d_melu.ensure(L.nbytes + 16384)) < 0) return r;
    if ((r = B.d_reflist.ensure((L.reflist.size() + 1) * sizeof(uint32_t))) < 0 ||
        (r = B.d_roff.ensure(L.roff.size() * sizeof(uint32_t))) < 0 ||
        (r = B.d_refbits.ensure((L.nrefmasks + 8) * sizeof(uint64_t))) < 0) return r;
    return 0;
}

static hipError_t block_tables_upload(const BlockBufs &B, const J2kBlock *blocks, const BlockLayout &L, hipStream_t st)
{
    if (!L.n) return hipSuccess;
    hipError_t e = hipMemcpyAsync(B.d_blocks.p, blocks, (size_t)L.n * sizeof(J2kBlock), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(B.d_qoff.p, L.qoff.data(), L.qoff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(B.d_roff.p, L.roff.data(), L.roff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !L.reflist.empty())
        e = hipMemcpyAsync(B.d_reflist.p, L.reflist.data(), L.reflist.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !L.mqwaves.empty())
        e = hipMemcpyAsync(B.d_mqwaves.p, L.mqwaves.data(), L.mqwaves.size() * sizeof(MqWave), hipMemcpyHostToDevice, st);
    return e;
}

/* blocks per wave of the un-stuffing kernel: the caller's figure unless a test asks otherwise */
static int unstuff_group(int g)
{
    const char *s = getenv("HTJ2K_UNSTUFF_G");
    return s ? atoi(s) : g;
}

/* the un-stuffing kernel with `g` codeblocks per wavefront (4, 2 or 1; fewer if the LDS of g blocks would not fit; more than
 * 48 KiB: lds_opt_in_all) */
static hipError_t launch_unstuff(hipStream_t st, const J2kBlock *blocks, int nblocks, const uint8_t *bytes, uint32_t *vlcu, uint32_t *melu,
                                 uint32_t us_words, int g)
{
    const size_t us_lds = (size_t)us_words * 4;
    if (g >= 4 && 4 * us_lds <= 64 * 1024)
        hipLaunchKernelGGL(k_ht_unstuff_g<16>, dim3((nblocks + 3) / 4), dim3(64), 4 * us_lds, st, blocks, nblocks, bytes, vlcu, melu, us_words);
    else if (g >= 2 && 2 * us_lds <= 64 * 1024)
        hipLaunchKernelGGL(k_ht_unstuff_g<32>, dim3((nblocks + 1) / 2), dim3(64), 2 * us_lds, st, blocks, nblocks, bytes, vlcu, melu, us_words);
    else
        hipLaunchKernelGGL(k_ht_unstuff, dim3(nblocks), dim3(64), us_lds, st, blocks, nblocks, bytes, vlcu, melu, us_words);
    return hipGetLastError();
}

/* The HT blocks [0, L.nht) on `st`, with the kernels `k` names */
static hipError_t launch_ht_blocks(hipStream_t st, const uint16_t *d_tables, const BlockBufs &B, const BlockLayout &L, const HtChoice &k)
{
    const int nblocks = L.nht;
    const J2kBlock *blocks = (const J2kBlock *)B.d_blocks.p;
    const uint8_t *bytes = (const uint8_t *)B.d_bytes.p;
    uint32_t *coef = (uint32_t *)B.d_coef.p, *sink = coef + L.nsamples + 32;
    int *status = (int *)B.d_status.p;
    ht_sym_t *qsym = (ht_sym_t *)B.d_qsym.p;
    const uint32_t *qoff = (const uint32_t *)B.d_qoff.p, *roff = (const uint32_t *)B.d_roff.p;
    uint32_t *vlcu = (uint32_t *)B.d_vlcu.p, *melu = (uint32_t *)B.d_melu.p;
    uint64_t *refbits = (uint64_t *)B.d_refbits.p;
    const bool refine = !L.reflist.empty();
    hipError_t e = hipSuccess;
    if (!k.extended) {
        auto kern = k.raw ? k_ht_decode_raw<false> : k_ht_decode<false>;
        hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64), L.lds.total, st, blocks, nblocks, bytes, coef, d_tables, status, L.lds,
                           (const ht_sym_t *)nullptr, (const uint32_t *)nullptr, sink, (const uint64_t *)nullptr, (const uint32_t *)nullptr, 0);
        return hipGetLastError();
    }
    const uint32_t mr_words = refine ? ht_nsp(L.max_lref) : 0u;
    if ((e = launch_unstuff(st, blocks, nblocks, bytes, vlcu, melu, 2 * std::max(L.lds.vlc_words, mr_words), k.unstuff_g)) != hipSuccess) return e;
    uint32_t *vlc_sink = (uint32_t *)qsym + L.nquads / 2 + 32;
    if (k.vlc2) {
        const int wg = 64 * HT_VLC_NARROW_WAVES;
        hipLaunchKernelGGL(k_ht_vlc2, dim3((nblocks + wg - 1) / wg), dim3(wg), HT_VLC2_LDS, st, blocks, nblocks, bytes, d_tables, qsym, qoff,
                           (const uint32_t *)vlcu, vlc_sink);
    } else {
        const size_t vlc_lds = ht_vlc_lds_bytes(L.lds.max_qw);
        hipLaunchKernelGGL(k_ht_vlc, dim3((nblocks + 63) / 64), dim3(64), vlc_lds, st, blocks, nblocks, bytes, d_tables, qsym, qoff, L.lds.max_qw,
                           (const uint32_t *)vlcu, (const uint32_t *)melu, vlc_sink);
    }
    if (refine) {
        /* k_ht_decode_multi deals out the MagRef bits itself; the column-per-lane kernel takes them from k_ht_refine */
        const bool magref = k.magsgn != HtChoice::MULTI;
        auto kref = L.ref_max_w <= 32 ? (magref ? k_ht_refine<uint32_t, true> : k_ht_refine<uint32_t, false>)
                                      : (magref ? k_ht_refine<uint64_t, true> : k_ht_refine<uint64_t, false>);
        hipLaunchKernelGGL(kref, dim3(((unsigned)L.reflist.size() + 63) / 64), dim3(64), 0, st, blocks, (const uint32_t *)B.d_reflist.p,
                           (int)L.reflist.size(), bytes, (const ht_sym_t *)qsym, qoff, (const uint32_t *)vlcu, (const uint32_t *)melu, refbits, roff);
    }
    if (k.magsgn == HtChoice::PAIR) {
        hipLaunchKernelGGL(k_ht_decode_pair, dim3((nblocks + 1) / 2), dim3(64), 2 * (L.lds_ext.ms_words + 4) * 4, st, blocks, nblocks, bytes,
                           coef, status, L.lds_ext.ms_words, (const ht_sym_t *)qsym, qoff, sink);
    } else if (k.magsgn == HtChoice::MULTI) {
        const uint32_t rg_rows = refine ? L.ref_max_h : 0u;
        const size_t lds = (size_t)k.bpw * (L.lds_ext.ms_words + 4) * 4 + (refine ? ht_multi_refine_lds(k.bpw, mr_words, rg_rows) : 0);
#define HT_MULTI_R(NB_, T_, R_) do { \
            hipLaunchKernelGGL((k_ht_decode_multi<NB_, T_, R_>), dim3((nblocks + NB_ - 1) / NB_), dim3(64), lds, st, blocks, nblocks, bytes, \
                               coef, status, L.lds_ext.ms_words, (const ht_sym_t *)qsym, qoff, sink, (const uint64_t *)refbits, roff, \
                               (const uint32_t *)melu, mr_words, rg_rows); } while (0)
#define HT_MULTI_T(NB_, T_) do { if (refine) HT_MULTI_R(NB_, T_, true); else HT_MULTI_R(NB_, T_, false); } while (0)
#define HT_MULTI(NB_) do { \
            if (k.multi_t == J2K_DWT53) HT_MULTI_T(NB_, J2K_DWT53); else if (k.multi_t == J2K_DWT97) HT_MULTI_T(NB_, J2K_DWT97); \
            else if (k.multi_t == J2K_DWT_RAW) HT_MULTI_T(NB_, J2K_DWT_RAW); else HT_MULTI_T(NB_, J2K_DWT97_INT); } while (0)
        if (k.bpw == 4) HT_MULTI(4); else HT_MULTI(2);
#undef HT_MULTI
#undef HT_MULTI_T
#undef HT_MULTI_R
    } else {
        auto kern = k.raw ? k_ht_decode_raw<true> : k_ht_decode<true>;
        hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64), L.lds_ext.total, st, blocks, nblocks, bytes, coef, d_tables, status, L.lds_ext,
                           (const ht_sym_t *)qsym, qoff, sink, (const uint64_t *)refbits, roff, k.coef16 ? 1 : 0);
    }
    return hipGetLastError();
}

/* The Part-1 blocks [L.nht, L.n) on `st`: the first `nwide` waves hold a block wider than 64 columns and run k_mq_decode<true> */
static hipError_t launch_mq_blocks(hipStream_t st, const BlockBufs &B, const BlockLayout &L, unsigned nwide)
{
    const uint32_t area = mq_lds_area(L.mq_planes);
    const unsigned nnarrow = (unsigned)L.mqwaves.size() - nwide;
    const J2kBlock *blocks = (const J2kBlock *)B.d_blocks.p + L.nht;
    int *status = (int *)B.d_status.p + L.nht;
    const int n = L.n - L.nht;
    if (nwide)
        hipLaunchKernelGGL(k_mq_decode<true>, dim3(nwide), dim3(64), area + MQ_LDS_TABLES, st, blocks, n, (const uint8_t *)B.d_bytes.p,
                           (uint32_t *)B.d_coef.p, status, (const MqWave *)B.d_mqwaves.p, (uint64_t *)B.d_mqscratch.p, area);
    if (nnarrow)
        hipLaunchKernelGGL(k_mq_decode<false>, dim3(nnarrow), dim3(64), area + MQ_LDS_TABLES, st, blocks + 64 * (size_t)nwide, n - 64 * (int)nwide,
                           (const uint8_t *)B.d_bytes.p, (uint32_t *)B.d_coef.p, status + 64 * (size_t)nwide,
                           (const MqWave *)B.d_mqwaves.p + nwide, (uint64_t *)B.d_mqscratch.p, area);
    return hipGetLastError();
}

static void push_bytes(std::vector<uint8_t> &v, const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    v.insert(v.end(), b, b + n);
}

/* descriptor tables for the IDWT launches and the pack stage */
/* Every table of a descriptor buffer starts on 16 bytes: pads, appends, returns where the table starts */
static size_t desc_append(std::vector<uint8_t> &v, const void *p, size_t n)
{
    v.resize(align_up(v.size(), 16), 0);
    const size_t off = v.size();
    push_bytes(v, p, n);
    return off;
}

/* One level of one plane as the kernels take it: the only place that fills a DwtLevel (its .g) or a DwtTileArgs */
static DwtTileArgs level_args(const J2kTileComp &tc, int lev)
{
    DwtTileArgs a;
    a.g.plane_off = tc.plane_off; a.g.stride = tc.w;
    a.g.lh = tc.linelen[lev][0]; a.g.lv = tc.linelen[lev][1];
    a.g.mh = tc.mod[lev][0]; a.g.mv = tc.mod[lev][1];
    a.g.last = (tc.transform == J2K_DWT97_INT && lev == tc.ndeclevels - 1) ? 1 : 0;
    a.ll_off = tc.plane_off; a.ll_stride = tc.w;
    a.out_off = tc.plane_off; a.out_stride = tc.w;
    return a;
}

/* ---- packed 16-bit final level (dwt_stream.hpp, PK): when is it exact? ----
 * The kernel computes the horizontal and vertical 5/3 lifting of the final level, the inverse RCT and the clip on pairs of
 * 16-bit samples with wrapping sums.  It equals the 32-bit arithmetic of the reference exactly when no intermediate leaves
 * 16 bits.  What bounds the inputs: a reversible HT coefficient is a 31-bit magnitude shifted down by 31 - M_b
 * (jpeg2000dec.c:2135-2144), so |coefficient| <= 2^M_b - 1 whatever the block's bytes hold; and the LL band is the output
 * of the level below, which the kernels that write it check against `bits` bits (their `ovf` flag: a job that fails runs
 * again with int32 LL bands and the 32-bit kernels).  Interval arithmetic through the step -- every sum, every shifted sum --
 * says whether a given `bits` is enough.  bound() returns the largest magnitude of a component's output samples, or -1. */
static long pk16_lift_bound(long ll, long hl, long lh, long hh)
{
    const long LIM = 32767;
    bool ok = true;
    auto s1 = [&](long c0, long a) { if (2 * a + 2 > LIM) ok = false; return c0 + (2 * a + 2) / 4; };   /* c - ((a + b + 2) >> 2) */
    auto s2 = [&](long c0, long a) { if (2 * a > LIM) ok = false; return c0 + a; };                     /* c + ((a + b) >> 1) */
    const long e = s1(ll, hl), o = s2(hl, e);              /* horizontal, vertical-low rows */
    const long eh = s1(lh, hh), oh = s2(hh, eh);           /* horizontal, vertical-high rows */
    const long re0 = s1(e, eh), ro0 = s2(eh, re0);         /* vertical, even columns */
    const long re1 = s1(o, oh), ro1 = s2(oh, re1);         /* vertical, odd columns */
    const long m = std::max(std::max(re0, ro0), std::max(re1, ro1));
    return ok && m <= LIM && e <= LIM && o <= LIM && eh <= LIM && oh <= LIM ? m : -1;
}
static bool pk16_bounds(const long (*B)[4], int nc, bool rct)     /* B[c] = { LL, HL, LH, HH } magnitude bounds of component c */
{
    long bc[3] = { 0, 0, 0 };
    for (int c = 0; c < nc; c++)
        if ((bc[c] = pk16_lift_bound(B[c][0], B[c][1], B[c][2], B[c][3])) < 0) return false;
    if (rct) {                                              /* g = y - ((cr + cb) >> 2); g + cr and g + cb saturate */
        if (bc[1] + bc[2] > 32767) return false;
        if (bc[0] + (bc[1] + bc[2]) / 4 + 1 > 32767) return false;
    }
    return true;
}

extern "C" long htj2k_pk16_lift_bound(long ll, long hl, long lh, long hh) { return pk16_lift_bound(ll, hl, lh, hh); }
extern "C" int htj2k_pk16_bounds(const long (*b)[4], int nc, int rct) { return b && nc >= 1 && nc <= 3 && pk16_bounds(b, nc, rct != 0) ? 1 : 0; }

/* The largest k, from `k` down to kmin, for which holds(k); 0: none.  A launch of level 0 reads the block decoder's LL
 * band, which no k bounds: there the first answer is the only one. */
template <class F> static int pk16_most_bits(int k, int kmin, bool level0, F holds)
{
    for (; k >= kmin; k--) {
        if (holds(k)) return k;
        if (level0) break;
    }
    return 0;
}

static void pk16_eligibility(htj2k_job *j)
{
    IdwtPlan &P = j->idwt;
    P.pk_bits = 0;
    for (LevelLaunch &L : P.launches_fused) L.pk_bits = 0;
    if (!j->coef16_ok) return;
    const int ntc = (int)j->tilecomps.size();
    /* the largest M_b among the blocks of every band: [plane][level][0 LL (level 0 only), 1 HL, 2 LH, 3 HH] */
    std::vector<std::pair<uint32_t, int>> start(ntc);
    for (int t = 0; t < ntc; t++) start[t] = { j->tilecomps[t].plane_off, t };
    std::sort(start.begin(), start.end());
    auto plane_of = [&](uint32_t off) {
        auto it = std::upper_bound(start.begin(), start.end(), std::make_pair(off, 1 << 30));
        return it == start.begin() ? -1 : (it - 1)->second;
    };
    std::vector<uint8_t> mb((size_t)ntc * J2K_MAX_DWTLEV * 4, 0);
    for (const J2kBlock &b : j->blocks) {
        const int t = plane_of(b.plane_off);
        if (t < 0) return;
        const J2kTileComp &tc = j->tilecomps[t];
        if (tc.ndeclevels < 1 || tc.ndeclevels > J2K_MAX_DWTLEV || tc.w <= 0) return;
        const uint32_t off = b.plane_off - tc.plane_off;
        const int x = (int)(off % (uint32_t)tc.w), y = (int)(off / (uint32_t)tc.w);
        int lev = tc.ndeclevels - 1, band = 0;
        for (; lev >= 0; lev--) {                           /* the outermost level whose low-pass quadrant does not hold the block */
            const int mh = tc.mod[lev][0], mv = tc.mod[lev][1];
            const int nlx = ((mh + tc.linelen[lev][0] + 1) >> 1) - ((mh + 1) >> 1), nly = ((mv + tc.linelen[lev][1] + 1) >> 1) - ((mv + 1) >> 1);
            band = (x >= nlx ? 1 : 0) + (y >= nly ? 2 : 0);
            if (band || lev == 0) break;
        }
        uint8_t &m = mb[((size_t)t * J2K_MAX_DWTLEV + lev) * 4 + band];
        if (b.M_b > m) m = b.M_b;
    }
    /* the most bits (16 .. 10 for 8-bit components) of LL input with which plane t's
     * level lev stays inside 16 bits: 0 = none; level 0 reads the block decoder's LL band, bounded by its own M_b and unchecked */
    auto bounds_of = [&](int t, int lev, int k, long (&B)[4]) {
        const uint8_t *m = &mb[((size_t)t * J2K_MAX_DWTLEV + lev) * 4];
        B[0] = lev == 0 ? (1L << m[0]) - 1 : 1L << (k - 1);
        for (int q = 1; q < 4; q++) B[q] = (1L << m[q]) - 1;
    };
    int job_bits = 16;
    for (LevelLaunch &L : P.launches_fused) {
        if (L.type != J2K_DWT53) continue;
        int bits = 16;
        if (L.nc == 0) {                                    /* plain level: its output is checked, its input has to be bounded */
            const DwtTileArgs *ta = (const DwtTileArgs *)(j->h_desc.data() + L.table_off);
            for (int i = 0; i < L.count && bits; i++) {
                const int t = plane_of(ta[i].g.plane_off);
                if (t < 0 || j->tilecomps[t].plane_off != ta[i].g.plane_off) { bits = 0; break; }
                /* (a component of n bits has LL bands of n + 1 bits with the RCT, and the check must leave an ordinary picture
                 * alone: twice that range at least) */
                bits = pk16_most_bits(bits, j->tilecomps[t].cbps + 2, L.level == 0, [&](int k) {
                    long B[4];
                    bounds_of(t, L.level, k, B);
                    return pk16_lift_bound(B[0], B[1], B[2], B[3]) >= 0;
                });
            }
        } else {
            if (!(L.outk == 0 || L.outk == 2)) continue;
            const DwtFusedArgs *fa = (const DwtFusedArgs *)(j->h_desc.data() + L.table_off);
            for (int i = 0; i < L.count && bits; i++) {
                const PackTile *PT = (const PackTile *)(j->h_desc.data() + P.pack_off) + fa[i].pack_tile;
                const bool rct = L.outk == 0 && PT->mct != 0;
                int tcs[3];
                bool ok = PT->precision == 8;
                for (int cc = 0; cc < L.nc && ok; cc++) {
                    tcs[cc] = plane_of(fa[i].a[cc].g.plane_off);
                    ok = tcs[cc] >= 0 && j->tilecomps[tcs[cc]].plane_off == fa[i].a[cc].g.plane_off && PT->c[L.outk == 2 ? fa[i].comp0 : cc].cbps == 8;
                }
                if (!ok) { bits = 0; break; }
                bits = pk16_most_bits(bits, 10, L.level == 0, [&](int k) {
                    long B[3][4];
                    for (int cc = 0; cc < L.nc; cc++) bounds_of(tcs[cc], L.level, k, B[cc]);
                    return pk16_bounds(B, L.nc, rct);
                });
            }
        }
        L.pk_bits = bits;
        if (bits && L.level > 0) job_bits = std::min(job_bits, bits);
    }
    P.pk_bits = job_bits;
}

/* ---- the IDWT launch plan (IdwtPlan), built by build_descriptors in the steps below; they run in this order, which is
 * the order of the tables in h_desc ---- */

/* The plain launch of (level, type): every coded plane of that transform that has the level, in tile-component order, as
 * DwtTileArgs in `ta`; of the planes that `skip_final` marks, not the final level (a fused launch runs that one).
 * An empty level is no launch entry: the generic kernels have nothing to do there, and the tile and fused plans are only
 * run when no plane has one (tile_ok; groups exist only then), so for them the test never fires. */
static LevelLaunch plain_launch(const htj2k_job *j, int lev, int type, const std::vector<uint8_t> &skip_final, std::vector<DwtTileArgs> &ta)
{
    LevelLaunch g(type, lev);
    for (size_t t = 0; t < j->tilecomps.size(); t++) {
        const J2kTileComp &tc = j->tilecomps[t];
        if (!tc.coded || tc.transform != type || lev >= tc.ndeclevels) continue;
        if (tc.linelen[lev][0] <= 0 || tc.linelen[lev][1] <= 0) continue;   /* empty level: no-op */
        if (skip_final[t] && lev == tc.ndeclevels - 1) continue;
        ta.push_back(level_args(tc, lev));
        g.add(ta.back().g);
    }
    g.count = (int)ta.size();
    return g;
}

/* the plain level tables of the generic (DwtLevel) and tile (DwtTileArgs) modes, where at least one plane has the level */
static void plan_plain_levels(htj2k_job *j, int maxlev)
{
    const std::vector<uint8_t> none(j->tilecomps.size(), 0);
    for (int lev = 0; lev < maxlev; lev++)
        for (int type = 0; type < 3; type++) {
            std::vector<DwtTileArgs> ta;
            LevelLaunch tl = plain_launch(j, lev, type, none, ta), g = tl;
            if (ta.empty()) continue;
            std::vector<DwtLevel> lv;
            for (const DwtTileArgs &a : ta) lv.push_back(a.g);
            g.table_off = desc_append(j->h_desc, lv.data(), lv.size() * sizeof(DwtLevel));
            tl.table_off = desc_append(j->h_desc, ta.data(), ta.size() * sizeof(DwtTileArgs));
            j->idwt.launches_generic.push_back(g);
            j->idwt.launches_tile.push_back(tl);
        }
}

/* tile mode ping-pongs between the two scratch buffers: the level that runs k-th for a
 * plane reads LL from buffer (k-1) and writes buffer k (1 = t0, 2 = t1) */
static void plan_final_bufs(htj2k_job *j)
{
    IdwtPlan &P = j->idwt;
    P.tile_ok = true;
    for (const J2kTileComp &tc : j->tilecomps) {
        int k = 0;
        if (tc.coded)
            for (int lev = 0; lev < tc.ndeclevels; lev++) {
                if (tc.linelen[lev][0] > 0 && tc.linelen[lev][1] > 0) k++;
                else P.tile_ok = false;        /* a level deeper than the size allows: planes would fall out of step */
            }
        P.final_buf.push_back(k == 0 ? 0 : 1 + ((k - 1) & 1));
    }
}

/* pack tiles; their source pointers are patched at launch time */
static void plan_pack_tiles(htj2k_job *j)
{
    IdwtPlan &P = j->idwt;
    std::vector<PackTile> tiles;
    for (int f = 0; f < j->nframes; f++) {
        const FrameSlot &F = j->frames[f];
        const J2kPlan *pl = F.plan;
        for (int ti = 0; ti < pl->ntiles; ti++) {
            PackTile T;
            memset(&T, 0, sizeof(T));
            T.out = F.out;
            T.ncomp = pl->info.ncomponents;
            T.out_bytes = pl->out_bytes;
            T.precision = pl->out_shift_precision;
            for (int cc = 0; cc < T.ncomp; cc++) {
                const J2kTileComp &tc = j->tilecomps[F.tc_base + ti * T.ncomp + cc];
                PackComp &C = T.c[cc];
                C.src = nullptr;
                C.w = tc.w; C.h = tc.h; C.transform = tc.transform; C.cbps = tc.cbps;
                C.out_plane = tc.out_plane; C.out_x = tc.out_x; C.out_y = tc.out_y;
                C.pix_step = tc.pix_step; C.pix_off = tc.pix_off;
                if (tc.w > T.maxw) T.maxw = tc.w;
                if (tc.h > T.maxh) T.maxh = tc.h;
                if (cc == 0) T.mct = tc.mct;
            }
            if (T.maxw > P.pack_maxw) P.pack_maxw = T.maxw;
            if (T.maxh > P.pack_maxh) P.pack_maxh = T.maxh;
            tiles.push_back(T);
        }
    }
    P.npack = (int)tiles.size();
    P.pack_off = desc_append(j->h_desc, tiles.data(), tiles.size() * sizeof(PackTile));
}

/* The components of a fusable tile whose final level runs as one entry of a fused launch: nc tile-components from tc0,
 * the components from comp0 of pack tile pack_tile */
struct FusedGroup { int tc0, nc, comp0, pack_tile; };

/* Which tiles can have their final level fused with the pack stage, and in which groups: sets tile_fusable, plane_fused
 * and any_fusable */
static std::vector<FusedGroup> plan_fused_groups(htj2k_job *j)
{
    IdwtPlan &P = j->idwt;
    std::vector<FusedGroup> groups;
    P.tile_fusable.assign(P.npack, 0);
    P.plane_fused.assign(j->tilecomps.size(), 0);
    if (P.tile_ok) {
        int ti = 0;
        for (int f = 0; f < j->nframes; f++) {
            const FrameSlot &F = j->frames[f];
            const J2kPlan *pl = F.plan;
            const int nc = pl->info.ncomponents;
            for (int k = 0; k < pl->ntiles; k++, ti++) {
                const int base = F.tc_base + k * nc;
                auto final_ok = [&](const J2kTileComp &tc) {
                    if (!tc.coded || tc.ndeclevels < 1) return false;
                    const int lev = tc.ndeclevels - 1;
                    return tc.linelen[lev][0] >= 2 && tc.linelen[lev][1] >= 2 && tc.linelen[lev][0] == tc.w && tc.linelen[lev][1] == tc.h;
                };
                auto same = [&](const J2kTileComp &a, const J2kTileComp &b) {
                    const int lev = a.ndeclevels - 1;
                    return a.w == b.w && a.h == b.h && a.ndeclevels == b.ndeclevels && a.transform == b.transform &&
                           a.mod[lev][0] == b.mod[lev][0] && a.mod[lev][1] == b.mod[lev][1];
                };
                bool ok = nc >= 1 && nc <= 4;
                for (int cc = 0; cc < nc && ok; cc++) ok = final_ok(j->tilecomps[base + cc]);
                if (!ok) continue;
                const J2kTileComp &t0 = j->tilecomps[base];
                std::vector<FusedGroup> mine;
                if (t0.pix_step > 1) {
                    ok = nc == 3 || nc == 4;
                    for (int cc = 1; cc < nc && ok; cc++)
                        ok = same(t0, j->tilecomps[base + cc]) && j->tilecomps[base + cc].pix_step == t0.pix_step &&
                             j->tilecomps[base + cc].out_plane == t0.out_plane;
                    mine.push_back({ base, nc, 0, ti });
                } else {
                    int first = 0;
                    if (t0.mct) {
                        ok = nc >= 3 && same(t0, j->tilecomps[base + 1]) && same(t0, j->tilecomps[base + 2]);
                        mine.push_back({ base, 3, 0, ti });
                        first = 3;
                    }
                    for (int cc = first; cc < nc; cc++) mine.push_back({ base + cc, 1, cc, ti });
                }
                if (!ok) continue;
                P.tile_fusable[ti] = 1;
                P.any_fusable = true;
                for (const FusedGroup &g : mine) {
                    groups.push_back(g);
                    for (int cc = 0; cc < g.nc; cc++) P.plane_fused[g.tc0 + cc] = 1;
                }
            }
        }
    }
    return groups;
}

/* ---- fused plan (idwt_mode 3): the final level of every fusable tile goes through
 * k_idwt_stream_pack, which writes the frame; everything else as in launches_tile ---- */
static void plan_fused_levels(htj2k_job *j, int maxlev, const std::vector<FusedGroup> &groups)
{
    IdwtPlan &P = j->idwt;
    if (!P.any_fusable) return;
    for (int lev = 0; lev < maxlev; lev++)
        for (int type = 0; type < 3; type++) {
            std::vector<DwtTileArgs> ta;
            LevelLaunch g = plain_launch(j, lev, type, P.plane_fused, ta);
            if (!ta.empty()) {
                g.table_off = desc_append(j->h_desc, ta.data(), ta.size() * sizeof(DwtTileArgs));
                P.launches_fused.push_back(g);
            }
            /* one launch per (components in the group, fast store kind): groups whose geometry and frame qualify for
             * a fast store go to the FASTONLY kernel of that kind, the rest to the general kernel (outk -1) */
            for (int nc = 1; nc <= 4; nc++)
            for (int outk = -1; outk <= 3; outk++) {
                LevelLaunch fz(type, lev);
                fz.nc = nc;
                fz.all_fast = outk >= 0;
                fz.outk = outk;
                std::vector<DwtFusedArgs> fa;
                for (const FusedGroup &gr : groups) {
                    const J2kTileComp &tc = j->tilecomps[gr.tc0];
                    if (gr.nc != nc || tc.transform != type || tc.ndeclevels - 1 != lev) continue;
                    const PackTile *PT = (const PackTile *)(j->h_desc.data() + P.pack_off) + gr.pack_tile;
                    const DwtLevel g0 = level_args(tc, lev).g;
                    int kind = stream_fast_geom(g0) ? stream_fast_outk(*PT, g0, nc, gr.comp0) : -1;
                    if (kind > 0 && type == J2K_DWT97_INT) kind = -1;      /* rgb48 / plane stores: 5/3 and 9/7 float only */
                    if (kind != outk) continue;
                    DwtFusedArgs A;
                    memset(&A, 0, sizeof(A));
                    for (int cc = 0; cc < nc; cc++) {      /* (the planes of a group have the final level's geometry in common) */
                        A.a[cc] = level_args(j->tilecomps[gr.tc0 + cc], lev);
                        fz.add(A.a[cc].g);
                    }
                    A.ncomp = nc; A.pack_tile = gr.pack_tile; A.comp0 = gr.comp0;
                    fa.push_back(A);
                    fz.hbm_bytes += (double)nc * g0.lh * g0.lv * (4.0 + PT->out_bytes);
                }
                if (fa.empty()) continue;
                fz.count = (int)fa.size();
                fz.table_off = desc_append(j->h_desc, fa.data(), fa.size() * sizeof(DwtFusedArgs));
                P.launches_fused.push_back(fz);
            }
        }
}

/* levels 0-2 of the reversible planes as one launch: the three plain launches must list the same planes (none of them has
 * its final level there), every level of fast geometry, every plane at the origin of its level */
static void plan_x3(htj2k_job *j)
{
    IdwtPlan::X3 &X = j->idwt.x3;
    const LevelLaunch *L3[3] = { nullptr, nullptr, nullptr };
    for (const LevelLaunch &L : j->idwt.launches_fused)
        if (L.type == J2K_DWT53 && L.nc == 0 && L.level < 3) L3[L.level] = &L;
    if (!(L3[0] && L3[1] && L3[2] && L3[0]->count == L3[1]->count && L3[1]->count == L3[2]->count)) return;
    X.ok = true;
    for (int k = 0; k < 3 && X.ok; k++) {
        const DwtTileArgs *A = (const DwtTileArgs *)(j->h_desc.data() + L3[k]->table_off);
        for (int i = 0; i < L3[k]->count && X.ok; i++) {
            X.ok = stream_fast_geom(A[i].g) && A[i].g.mh == 0 && A[i].g.mv == 0;
            const double n = (double)A[i].g.lh * A[i].g.lv;
            X.alg += 8.0 * n;
            X.hbm += 2.0 * n * (k == 0 ? 1.0 : 0.75) + (k == 2 ? 2.0 * n : 0.0);   /* 16-bit: the sub-bands in, the third level out */
        }
        X.tab[k] = L3[k]->table_off;
        X.lh[k] = L3[k]->max_lh;
    }
    /* (the planes of a launch are listed in tile-component order by every level: same index, same plane) */
    X.count = L3[0]->count;
    X.lv2 = L3[2]->max_lv;
}

/* the last plain 5/3 level inside the final-level launch: the job's only fused 5/3 launch is an rgb24 fast-store one, the
 * plain launch of the level below lists exactly its planes, component by component in the same order, and both levels
 * are of fast geometry at the origin */
static void plan_x2(htj2k_job *j)
{
    const std::vector<LevelLaunch> &LL = j->idwt.launches_fused;
    IdwtPlan::X2 &X = j->idwt.x2;
    int nfz = 0, iq = -1, ip = -1;
    for (size_t i = 0; i < LL.size(); i++)
        if (LL[i].type == J2K_DWT53 && LL[i].nc) { nfz++; iq = (int)i; }
    if (nfz == 1 && LL[iq].nc == 3 && LL[iq].outk == 0 && LL[iq].level >= 1)
        for (size_t i = 0; i < LL.size(); i++)
            if (LL[i].type == J2K_DWT53 && !LL[i].nc && LL[i].level == LL[iq].level - 1) ip = (int)i;
    if (ip < 0 || LL[ip].count != 3 * LL[iq].count) return;
    const DwtTileArgs *ta = (const DwtTileArgs *)(j->h_desc.data() + LL[ip].table_off);
    const DwtFusedArgs *fa = (const DwtFusedArgs *)(j->h_desc.data() + LL[iq].table_off);
    const PackTile *PT = (const PackTile *)(j->h_desc.data() + j->idwt.pack_off);
    X.ok = true;
    X.plain = ip; X.fused = iq;
    for (int i = 0; i < LL[iq].count && X.ok; i++)
        for (int cc = 0; cc < 3 && X.ok; cc++) {
            const DwtTileArgs &f = fa[i].a[cc], &a = ta[3 * i + cc];
            X.ok = stream_fast_geom(f.g) && !f.g.mh && !f.g.mv && stream_fast_geom(a.g) && !a.g.mh && !a.g.mv &&
                   a.g.plane_off == f.g.plane_off && a.out_off == f.ll_off && a.out_stride == f.ll_stride &&
                   a.g.lh == (f.g.lh + 1) / 2 && a.g.lv == (f.g.lv + 1) / 2 && f.g.lh == fa[i].a[0].g.lh && f.g.lv == fa[i].a[0].g.lv;
            const double nf = (double)f.g.lh * f.g.lv, na = (double)a.g.lh * a.g.lv;
            X.alg += 8.0 * (nf + na);
            /* 16-bit: everything the level below reads, the final level's three sub-band quarters, the frame bytes */
            X.hbm += 2.0 * na + 1.5 * nf + nf * PT[fa[i].pack_tile].out_bytes;
            X.ll_bytes += 2.0 * na;
        }
}

static void build_descriptors(htj2k_job *j)
{
    j->h_desc.clear();
    j->h_desc_dev.clear();                              /* d_desc is written again by the next run */
    j->final_eff.assign(j->tilecomps.size(), 0);
    j->idwt = IdwtPlan();
    int maxlev = 0;
    for (const J2kTileComp &tc : j->tilecomps)
        if (tc.coded && tc.ndeclevels > maxlev) maxlev = tc.ndeclevels;
    plan_plain_levels(j, maxlev);
    plan_final_bufs(j);
    plan_pack_tiles(j);
    const std::vector<FusedGroup> groups = plan_fused_groups(j);
    plan_fused_levels(j, maxlev, groups);
    plan_x3(j);
    plan_x2(j);
}

/* LDS windows of the HT kernels from the plans' figures */
static int job_ht_lds(htj2k_ctx *c, htj2k_job *j)
{
    uint32_t max_p = 0, max_s = 2, max_qw = 1, bm_words = 0;
    for (int f = 0; f < j->nframes; f++) {
        const J2kPlan *pl = j->frames[f].plan;
        max_p = std::max(max_p, pl->max_pcup); max_s = std::max(max_s, pl->max_scup);
        max_qw = std::max(max_qw, pl->max_qw); bm_words = std::max(bm_words, pl->max_bm_words);
    }
    return ht_lds_layout(c, max_p, max_s, max_qw, bm_words, &j->lay.lds, &j->lay.lds_ext);
}

/* Blocks are independent: order the table by quad count (then width), largest first, so that the 64 lanes of a k_ht_vlc
 * wave (one lane per block) run similar trip counts, and put the Part-1 blocks behind the HT blocks.  Returns the number
 * of HT blocks. */
static int job_order_blocks(std::vector<J2kBlock> &blocks)
{
    /* two stable counting passes (least significant key first) */
    auto quads = [](const J2kBlock &b) { return b.npasses ? (uint32_t)((b.w + 1) >> 1) * ((b.h + 1) >> 1) : 0u; };
    std::vector<J2kBlock> tmp(blocks.size());
    {
        std::vector<uint32_t> cnt(1026, 0);
        for (const J2kBlock &b : blocks) cnt[1024 - std::min<uint32_t>(b.w, 1024) + 1]++;
        for (size_t i = 1; i < cnt.size(); i++) cnt[i] += cnt[i - 1];
        for (const J2kBlock &b : blocks) tmp[cnt[1024 - std::min<uint32_t>(b.w, 1024)]++] = b;
    }
    {
        uint32_t maxq = 0;
        for (const J2kBlock &b : tmp) maxq = std::max(maxq, quads(b));
        std::vector<uint32_t> cnt((size_t)maxq + 2, 0);
        for (const J2kBlock &b : tmp) cnt[maxq - quads(b) + 1]++;
        for (size_t i = 1; i < cnt.size(); i++) cnt[i] += cnt[i - 1];
        for (const J2kBlock &b : tmp) blocks[cnt[maxq - quads(b)]++] = b;
    }
    /* Part-1 blocks behind the HT blocks, ordered so that the 64 lanes of a k_mq_decode wave walk blocks of
     * one size with similar pass counts (the sort above already grouped sizes) */
    auto mid = std::stable_partition(blocks.begin(), blocks.end(), [](const J2kBlock &b) { return !(b.flags & J2K_BLK_PART1); });
    std::stable_sort(mid, blocks.end(), [](const J2kBlock &a, const J2kBlock &b) {
        if ((a.w > 64) != (b.w > 64)) return a.w > 64;     /* the waves that need k_mq_decode<true> come first */
        if (a.h != b.h) return a.h > b.h;
        if (a.w != b.w) return a.w > b.w;
        return a.npasses > b.npasses;
    });
    return (int)(mid - blocks.begin());
}

/* Which of the faster MagSgn kernels the blocks of a table, laid out as L, allow.  This is all the kernels themselves
 * rely on: a job adds what its planes and IDWT launches ask (job_ht_eligibility), the unit entry points refuse a table
 * that the route asked of them excludes (ht_blocks) */
struct HtRoutes {
    bool coef16 = false;               /* 16-bit stores: k_ht_decode<true> with coef16, and ... */
    bool pair = false;                 /* ... k_ht_decode_pair, whose dword stores want even widths, strides, offsets */
    int multi_nb = 0;                  /* k_ht_decode_multi: blocks per wave (2: blocks up to 64 columns, 4: up to 32), 0: not eligible */
    int multi_t = 0;                   /* ... and the transform all blocks share */
};
static HtRoutes ht_block_routes(const J2kBlock *blocks, size_t n, const BlockLayout &L)
{
    HtRoutes R;
    /* 16-bit stores: all blocks HT blocks of a reversible 5/3 band with step 1, at most 64 columns, M_b <= 15, no ROI
     * shift, the cleanup pass only behind the placeholder passes */
    bool ok = L.nht == (int)n && L.reflist.empty() && n;
    for (size_t i = 0; ok && i < n; i++) {
        const J2kBlock &b = blocks[i];
        ok = b.w <= 64 && b.M_b <= 15 && b.roi_shift == 0 && b.i_step == 32768 && (b.flags & 3) == J2K_DWT53;
        if (ok && b.npasses) { const int rem = b.npasses % 3; ok = b.npasses - (rem ? b.npasses - rem : b.npasses - 3) == 1; }
    }
    R.coef16 = ok;
    for (size_t i = 0; ok && i < n; i++) {
        const J2kBlock &b = blocks[i];
        ok = !(b.w & 1) && !(b.stride & 1) && !(b.plane_off & 1);
    }
    R.pair = ok;
    /* k_ht_decode_multi: every block an HT block, at most 64 columns, no ROI shift, one transform for all of them;
     * four blocks per wave when none is wider than 32 columns */
    /* (blocks with SigProp / MagRef passes of such tables are all on k_ht_refine's list: same conditions) */
    bool mok = L.nht == (int)n && n;
    int maxw = 0;
    const int t0 = mok ? (blocks[0].flags & 3) : 0;
    for (size_t i = 0; mok && i < n; i++) {
        const J2kBlock &b = blocks[i];
        mok = b.w <= 64 && b.roi_shift == 0 && (b.flags & 3) == t0;
        if (b.w > maxw) maxw = b.w;
    }
    R.multi_nb = mok ? (maxw <= 32 ? 4 : 2) : 0;
    R.multi_t = t0;
    /* the kernel holds the un-stuffed MagSgn bits of all its blocks in LDS: with long segments (16-bit material: 10 KB
     * per 64 x 64 block) two blocks per wave leave 2 waves per SIMD and the column-per-lane kernel is quicker
     * (C4 gray16 1.50 -> 1.64 ms per 16 frames), with short ones it is not (int32 C2 2.93 -> 2.74, C3 2.15 -> 1.65) */
    const size_t multi_lds_max = getenv("HTJ2K_MULTI_LDS") ? (size_t)atoi(getenv("HTJ2K_MULTI_LDS")) : 12 * 1024;
    if (mok && (size_t)R.multi_nb * (L.lds_ext.ms_words + 4) * 4 > multi_lds_max) R.multi_nb = 0;
    /* blocks with refinement passes: their SigProp masks and MagRef bits are staged in LDS, up to 64 sample rows */
    if (R.multi_nb && !L.reflist.empty() &&
        (L.ref_max_h > 64 || ht_multi_refine_lds(R.multi_nb, ht_nsp(L.max_lref), L.ref_max_h) > 24 * 1024)) R.multi_nb = 0;
    return R;
}

/* Which of the faster HT kernels the job's blocks and planes allow: coef16_ok (and with it the packed final levels,
 * pk16_eligibility), pair_ok, multi_nb / multi_t.  Needs the layout and the descriptors (build_descriptors). */
static void job_ht_eligibility(htj2k_job *j)
{
    const HtRoutes R = ht_block_routes(j->blocks.data(), j->blocks.size(), j->lay);
    /* 16-bit sub-bands: what the blocks allow, and only the FASTONLY streaming IDWT kernels read them */
    bool ok = R.coef16 && j->idwt.tile_ok && j->idwt.any_fusable;
    for (size_t t = 0; ok && t < j->tilecomps.size(); t++) {
        const J2kTileComp &tc = j->tilecomps[t];
        ok = tc.coded && tc.transform == J2K_DWT53 && tc.ndeclevels >= 1;
    }
    for (size_t i = 0; ok && i < j->idwt.launches_fused.size(); i++) {
        const LevelLaunch &LL = j->idwt.launches_fused[i];
        ok = LL.all_fast && LL.type == J2K_DWT53 && LL.min_l >= 2;
    }
    for (size_t i = 0; ok && i < j->idwt.tile_fusable.size(); i++) ok = j->idwt.tile_fusable[i] != 0;
    j->coef16_ok = ok;
    pk16_eligibility(j);
    j->pair_ok = ok && R.pair;
    j->multi_nb = R.multi_nb;
    j->multi_t = R.multi_t;
}

/* What every extended run launches in front of the MagSgn kernel, by the widest block in quads: the VLC kernel and the
 * blocks per wave of the un-stuffing kernel */
static HtChoice ht_choice_front(const htj2k_ctx *c, uint32_t max_qw, bool raw)
{
    HtChoice k;
    k.raw = raw;
    k.vlc2 = max_qw <= 32;
    k.extended = c->ht_mode == 1 && (k.vlc2 ? (size_t)HT_VLC2_LDS : ht_vlc_lds_bytes(max_qw)) <= 160 * 1024;
    if (!k.extended) {
        k.vlc2 = false;
        return k;
    }
    /* blocks per wave of the un-stuffing kernel: four (16 lanes each) where no block is wider than 32 columns, else
     * two -- per 128 frames of C2 (64 x 64 blocks) 404 us with one, 378 with two, 456 with four (more passes, each
     * with its fixed cost); per 96 frames of C3 (32 x 32) 820 / 529 / 451 */
    k.unstuff_g = unstuff_group(max_qw <= 16 ? 4 : 2);
    return k;
}

/* What a run of the job with stage mask `mask` launches for its HT blocks: the context's knobs over what the job allows */
static HtChoice job_ht_choice(const htj2k_ctx *c, const htj2k_job *j, int mask)
{
    HtChoice k = ht_choice_front(c, j->lay.lds.max_qw, j->raw);
    if (!k.extended) return k;
    /* 16-bit sub-bands only when this very call also runs the (fused, streaming) IDWT that reads them */
    k.coef16 = c->coef16 && j->coef16_ok && mask == 7 && c->idwt_mode == 3 && c->fuse_pack && !j->raw;
    if (k.coef16 && j->pair_ok && c->ht_pair) {
        k.magsgn = HtChoice::PAIR;
        k.bpw = 2;
    } else if (!k.coef16 && j->multi_nb && c->ht_multi) {
        k.magsgn = HtChoice::MULTI;
        k.bpw = j->multi_nb;
        k.multi_t = j->multi_t;
    }
    return k;
}

/* Upload step: the output planes of every frame, sized from the plan, and what the pack stage needs to know of them
 * (OutPlanes).  Samples of the picture that no tile-component covers (image offsets with subsampling can leave a chroma
 * row or column out, write_frame_8/16 jpeg2000dec.c:2312-2358) are never written, in the reference either; such planes
 * are cleared so that what the caller gets there does not depend on what the buffer held before */
static int upload_out_planes(htj2k_ctx *c, htj2k_job *j)
{
    int r;
    for (int f = 0; f < j->nframes; f++) {
        FrameSlot &F = j->frames[f];
        const J2kPlan *pl = F.plan;
        memset(&F.out, 0, sizeof(F.out));
        for (int p = 0; p < pl->info.nplanes; p++) {
            const int ls = pl->info.plane_width[p] * pl->info.plane_bytes_per_sample[p];
            if ((r = F.d_out[p].ensure((size_t)ls * pl->info.plane_height[p] + 64)) < 0) return r;
            F.out.ptr[p] = (uint8_t *)F.d_out[p].p;
            F.out.linesize[p] = ls;
            F.out.width[p] = pl->info.plane_width[p];
            F.out.height[p] = pl->info.plane_height[p];
        }
        for (int p = 0; p < pl->info.nplanes && p < 4; p++) {
            if (pl->info.has_palette && p == 1) continue;
            long long covered = 0;
            int first = -1;                                      /* packed formats: the components share the pixels */
            for (int t = 0; t < pl->ntilecomps; t++)
                if (pl->tilecomps[t].out_plane == p && (first < 0 || pl->tilecomps[t].comp < first)) first = pl->tilecomps[t].comp;
            for (int t = 0; t < pl->ntilecomps; t++) {
                const J2kTileComp &tc = pl->tilecomps[t];
                if (tc.out_plane == p && tc.comp == first && tc.out_w > 0 && tc.out_h > 0) covered += (long long)tc.out_w * tc.out_h;
            }
            const long long need = (long long)pl->info.plane_width[p] * pl->info.plane_height[p];
            if (covered < need)
                HIP_TRY(c, hipMemsetAsync(F.d_out[p].p, 0, (size_t)F.out.linesize[p] * F.out.height[p], j->stream));
        }
    }
    return 0;
}

/* Upload step: the code-block bytes into the pool d_bytes.  Device gather: the packets as they are (unless the parse has
 * sent them on their way already), the parsers' literal bytes and the merged gather table; the pool is cleared and
 * k_gather puts it together.  Host gather: the pool part each parser gathered, a copy per frame */
static int upload_block_bytes(htj2k_ctx *c, htj2k_job *j)
{
    int r;
    if (!j->dev_gather) {
        for (int f = 0; f < j->nframes; f++) {
            const FrameSlot &F = j->frames[f];
            if (F.plan->nbytes)
                HIP_TRY(c, hipMemcpyAsync((uint8_t *)j->d_bytes.p + F.bytes_base, F.plan->bytes, F.plan->nbytes,
                                          hipMemcpyHostToDevice, j->stream));
        }
        return 0;
    }
    if ((r = j->d_pkt.ensure(j->pkt_bytes + 256)) < 0 || (r = j->d_lit.ensure(j->lit.size() + 64)) < 0 ||
        (r = j->d_gsegs.ensure((j->gsegs.size() + 1) * sizeof(J2kSeg))) < 0 ||
        (r = j->d_ggroups.ensure((j->ggroups.size() + 1) * sizeof(uint32_t))) < 0) return r;
    if (!j->pkt_h2d_issued)
        for (int f = 0; f < j->nframes; f++)
            HIP_TRY(c, job_packet_h2d(j, j->frames[f], (size_t)j->frames[f].plan->pkt_size));
    j->pkt_h2d_issued = false;
    if (!j->lit.empty())
        HIP_TRY(c, hipMemcpyAsync(j->d_lit.p, j->lit.data(), j->lit.size(), hipMemcpyHostToDevice, j->stream));
    if (!j->gsegs.empty())
        HIP_TRY(c, hipMemcpyAsync(j->d_gsegs.p, j->gsegs.data(), j->gsegs.size() * sizeof(J2kSeg), hipMemcpyHostToDevice, j->stream));
    HIP_TRY(c, hipMemcpyAsync(j->d_ggroups.p, j->ggroups.data(), j->ggroups.size() * sizeof(uint32_t), hipMemcpyHostToDevice, j->stream));
    HIP_TRY(c, hipMemsetAsync(j->d_bytes.p, 0, j->nbytes + 256, j->stream));
    const int ngroups = (int)j->ggroups.size() - 1;
    if (ngroups > 0 && !j->gsegs.empty()) {
        hipLaunchKernelGGL(k_gather, dim3((ngroups + 3) / 4), dim3(256), 0, j->stream, (const J2kSeg *)j->d_gsegs.p,
                           (const uint32_t *)j->d_ggroups.p, ngroups, (const uint8_t *)j->d_pkt.p, (const uint8_t *)j->d_lit.p,
                           (uint8_t *)j->d_bytes.p);
        HIP_TRY(c, hipGetLastError());
    }
    return 0;
}

/* Everything of the job's content that the stages read, queued on the job's stream: ev[0] .. ev[1] bracket the transfers */
extern "C" int htj2k_job_upload(htj2k_ctx *c, htj2k_job *j)
{
    if (!c || !j || j->nframes <= 0) return HTJ2K_ERR_EINVAL;
    int r;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((r = job_ht_lds(c, j)) < 0) return r;
    const int nht = job_order_blocks(j->blocks);
    const int nblocks = (int)j->blocks.size();
    if ((r = block_layout(j->blocks.data(), nht, nblocks, j->nbytes, j->nsamples, j->lay)) < 0) return r;
    if ((r = block_bufs_ensure(*j, j->lay)) < 0) return r;
    if ((r = j->d_t0.ensure(coef_buf_bytes(j->nsamples))) < 0 || (r = j->d_t1.ensure(coef_buf_bytes(j->nsamples))) < 0) return r;
    if ((r = upload_out_planes(c, j)) < 0) return r;
    build_descriptors(j);
    job_forget(j);                                         /* (final_eff is back at the coefficient buffer) */
    job_ht_eligibility(j);
    if ((r = j->d_desc.ensure(j->h_desc.size() + 64)) < 0) return r;
    HIP_TRY(c, hipEventRecord(j->ev[0], j->stream));
    if ((r = upload_block_bytes(c, j)) < 0) return r;
    for (int f = 0; f < j->nframes; f++) {                 /* PAL8: the palette is the second plane (jpeg2000dec.c:2900-2901) */
        const FrameSlot &F = j->frames[f];
        if (F.plan->info.has_palette && F.plan->info.nplanes > 1)
            HIP_TRY(c, hipMemcpyAsync(F.out.ptr[1], F.plan->palette, 256 * sizeof(uint32_t), hipMemcpyHostToDevice, j->stream));
    }
    HIP_TRY(c, block_tables_upload(*j, j->blocks.data(), j->lay, j->stream));
    HIP_TRY(c, hipEventRecord(j->ev[1], j->stream));
    j->uploaded = 1;
    return 0;
}

/* ------------------------------------------------------------------ job: run */
static uint32_t *buf_ptr(htj2k_job *j, int which)
{
    return (uint32_t *)(which == 0 ? j->d_coef.p : which == 1 ? j->d_t0.p : j->d_t1.p);
}

/* tile mode: the buffer that holds the LL band a level reads (the level below wrote it; level 0 reads the block decoder's) */
static uint32_t *ll_buf(htj2k_job *j, int level) { return buf_ptr(j, level == 0 ? 0 : 1 + ((level - 1) & 1)); }

/* the table at byte offset `off` of d_desc */
template <class T> static const T *desc_at(const htj2k_job *j, size_t off) { return (const T *)((const uint8_t *)j->d_desc.p + off); }

/* f(transform type as an integral constant): the kernels' <TYPE> */
template <class F> static void with_dwt_type(int type, F f)
{
    using std::integral_constant;
    if (type == J2K_DWT53) f(integral_constant<int, J2K_DWT53>());
    else if (type == J2K_DWT97) f(integral_constant<int, J2K_DWT97>());
    else f(integral_constant<int, J2K_DWT97_INT>());
}

template <int TYPE>
static void launch_generic_level(htj2k_job *j, const LevelLaunch &L)
{
    const DwtLevel *tab = desc_at<DwtLevel>(j, L.table_off);
    dim3 gh((L.max_lh + 255) / 256, L.max_lv, L.count), gv((L.max_lh + 255) / 256, L.max_lv, L.count);
    hipLaunchKernelGGL((k_idwt_h<TYPE>), gh, dim3(256), 0, j->stream, tab, (const uint32_t *)j->d_coef.p, (uint32_t *)j->d_t0.p);
    hipLaunchKernelGGL((k_idwt_v<TYPE>), gv, dim3(256), 0, j->stream, tab, (const uint32_t *)j->d_t0.p, (uint32_t *)j->d_coef.p);
}

#define TILE_W 64
#define TILE_H 32

/* rows per wave of the streaming kernels.  Measured on the 4K batch (tools/gpu_strip.py): the
 * launches are bound by the memory pipeline, not by the HALO rows a strip re-reads (those hit in
 * the XCD's L2, see stream_strip()), and 12..18 rows per strip is the flat optimum -- many short
 * waves keep more loads in flight and leave a shorter tail than few long ones. */
static int stream_strip_rows(int max_lh, int max_lv, int count)
{
    const char *e = getenv("HTJ2K_STRIP");
    if (e && atoi(e) >= 8) return atoi(e) & ~1;
    const long cols = (max_lh + STREAM_TW - 1) / STREAM_TW;
    return cols * ((max_lv + 15) / 16) * count >= 2048 ? 16 : 8;
}

/* Output columns per wave.  out_bytes = bytes one output column takes in the row a strip stores (2 / 4: a 16- / 32-bit
 * LL band; 3 / 6 / 1 / 2: rgb24 / rgb48 / 8- / 16-bit plane of the fused final level; 0: general path). */
static int stream_strip_cols(int max_lh, int out_bytes)
{
    const char *e = getenv(out_bytes == 2 ? "HTJ2K_TW16" : out_bytes == 4 ? "HTJ2K_TW32" : "HTJ2K_TWF");
    if (e && atoi(e) >= 64 && atoi(e) <= STREAM_TW) return atoi(e) & ~3;
    /* 224 columns are 448 / 896 / 1344 bytes of 16-bit / 32-bit / rgb48 output: whole 64-byte pieces, so that two
     * neighbouring strips never write into the same piece of a line (244 columns end mid-line, and half of a 16-bit
     * strip's lines are shared with a neighbour).  It idles 5 more lanes of 64 and adds a strip per 11, which only pays
     * once a row has several strips: measured per level on C2 / C3 / C4, 16-bit rows from 1920
     * columns (288 -> 265 us at 1920, 67 -> 73 at 960), 32-bit rows from 960 (237 -> 221 us at 1920, 76 -> 66 at 960).
     * rgb24 rows (732 bytes per strip, never a multiple of 64 below 256 columns) keep the full width. */
    if (out_bytes == 2) return max_lh >= 1920 ? 224 : STREAM_TW;
    if (out_bytes == 4 || out_bytes == 6) return max_lh >= 960 ? 224 : STREAM_TW;
    return STREAM_TW;
}

static StreamGrid stream_grid(int max_lh, int max_lv, int th, int count, int tw = STREAM_TW, int wpb = 1)
{
    StreamGrid G;
    G.tw = tw;
    G.gx = (max_lh + tw - 1) / tw;
    G.gy = (max_lv + th - 1) / th;
    G.nstrips = G.gx * G.gy * count;
    G.per_xcd = ((G.nstrips + 7) / 8 + wpb - 1) / wpb * wpb;      /* launches of 8 * per_xcd / wpb workgroups of wpb waves */
    return G;
}
/* Waves per workgroup of the streaming kernels that take more than one (the 16-bit FASTONLY ones).  Eight neighbouring
 * strips -- half a row of a 4K plane -- as one workgroup walk down the same rows of neighbouring column ranges together on one
 * CU, so what they ask of a DRAM page comes close together in time: final level of C2 740 -> 711 us with the 32-bit arithmetic
 * (4 waves per SIMD), 774 -> 660 with the packed one at two such workgroups per CU (below); 6 or 10 waves, which do not divide
 * the 16 strips of a row, 718 / 724; 16 waves 700-707; level 4 250 -> 238-243 us. */
static int stream_wpb(int max_lh, int tw)
{
    const int e = getenv("HTJ2K_WPB") ? atoi(getenv("HTJ2K_WPB")) : 0;      /* (per launch: tools/gpu_idwt_ab.py flips it between runs) */
    if (e >= 1 && e <= 8) return e;
    return std::max(1, std::min(8, (max_lh + tw - 1) / tw));
}
/* Dynamic LDS the packed final-level kernel is launched with -- it uses none: it is there to keep the CU at 16 waves.  The
 * kernel needs 61 VGPRs and would run 8 waves per SIMD, and with that many strips in flight the memory system does worse:
 * C2 final level, one wave per workgroup, 792 us at 32 waves per CU, 754 at 20, 732 at 16, 718 at 12, 757 at 8; workgroups
 * of eight waves 713 us at three per CU, 660-683 at two, 739 at one. */
/* experiments: dynamic LDS (bytes per wave) for the other multi-wave streaming launches, as an occupancy limit */
static int stream_occ_lds(int wpb)
{
    const int e = getenv("HTJ2K_OCC_LDS") ? atoi(getenv("HTJ2K_OCC_LDS")) : 0;
    return std::min(e * wpb, 48 * 1024);
}
static int stream_pk_lds(int wpb)
{
    const int e = getenv("HTJ2K_PK_LDS") ? atoi(getenv("HTJ2K_PK_LDS")) : -1;
    if (e >= 0) return e;
    const int per_cu = wpb >= 8 ? 2 : wpb >= 4 ? 3 : 12 / wpb;          /* workgroups */
    return (160 * 1024 / per_cu) & ~1023;
}

template <int TYPE>
static void launch_tile_generic(const void *tab, int max_lh, int max_lv, int min_l, int count, int mode, hipStream_t s,
                                const uint32_t *ll, const uint32_t *band, uint32_t *out, bool all_fast, int coef16 = 0)
{
    if (mode >= 3 && min_l >= 2) {
        const int th = stream_strip_rows(max_lh, max_lv, count);
        const int tw = stream_strip_cols(max_lh, all_fast ? 4 : 0);
        const int wpb = all_fast || (TYPE == J2K_DWT53 && coef16) ? stream_wpb(max_lh, tw) : 1;
        const StreamGrid G = stream_grid(max_lh, max_lv, th, count, tw, wpb);
        const dim3 g(8 * G.per_xcd / wpb), blk(64 * wpb);
        const int lds = stream_occ_lds(wpb);
        if (TYPE == J2K_DWT53 && coef16 == 2) hipLaunchKernelGGL((k_idwt_stream<J2K_DWT53, true, true, true>), g, blk, lds, s, (const DwtTileArgs *)tab, ll, band, out, th, G);
        else if (TYPE == J2K_DWT53 && coef16 == 1) hipLaunchKernelGGL((k_idwt_stream<J2K_DWT53, true, true, false>), g, blk, lds, s, (const DwtTileArgs *)tab, ll, band, out, th, G);
        else if (all_fast) hipLaunchKernelGGL((k_idwt_stream<TYPE, true>), g, blk, lds, s, (const DwtTileArgs *)tab, ll, band, out, th, G);
        else hipLaunchKernelGGL((k_idwt_stream<TYPE, false>), g, dim3(64), 0, s, (const DwtTileArgs *)tab, ll, band, out, th, G);
    } else {
        dim3 g((max_lh + TILE_W - 1) / TILE_W, (max_lv + TILE_H - 1) / TILE_H, count);
        hipLaunchKernelGGL((k_idwt_tile<TYPE, TILE_W, TILE_H>), g, dim3(256), 0, s, (const DwtTileArgs *)tab, ll, band, out);
    }
}

/* how many bits the 16-bit LL bands of a job must fit: 16, fewer where a packed final level needs it (pk16_eligibility) or a test says so */
static int ll16_check_bits(const htj2k_ctx *c, const htj2k_job *j)
{
    return std::min(c->ll16_test_bits, c->idwt_pk && j->idwt.pk_bits ? j->idwt.pk_bits : 16);
}

template <int TYPE>
static void launch_tile_level(htj2k_ctx *c, htj2k_job *j, const LevelLaunch &L, const uint32_t *ll, uint32_t *out)
{
    if (TYPE == J2K_DWT53 && j->run.ll16_run && c->idwt_mode >= 3 && L.min_l >= 2) {    /* 16-bit sub-bands and LL bands, in and out */
        const int th = stream_strip_rows(L.max_lh, L.max_lv, L.count);
        const int tw = stream_strip_cols(L.max_lh, 2), wpb = stream_wpb(L.max_lh, tw);
        const StreamGrid G = stream_grid(L.max_lh, L.max_lv, th, L.count, tw, wpb);
        if (L.pk_bits && j->run.pk_run)
            hipLaunchKernelGGL(k_idwt_stream_ll16<true>, dim3(8 * G.per_xcd / wpb), dim3(64 * wpb), 0, j->stream,
                               desc_at<DwtTileArgs>(j, L.table_off), ll, (const uint32_t *)j->d_coef.p, out, th, G,
                               (int *)j->d_status.p + j->blocks.size(), ll16_check_bits(c, j));
        else
            hipLaunchKernelGGL(k_idwt_stream_ll16<false>, dim3(8 * G.per_xcd / wpb), dim3(64 * wpb), 0, j->stream,
                               desc_at<DwtTileArgs>(j, L.table_off), ll, (const uint32_t *)j->d_coef.p, out, th, G,
                               (int *)j->d_status.p + j->blocks.size(), ll16_check_bits(c, j));
        return;
    }
    launch_tile_generic<TYPE>(desc_at<DwtTileArgs>(j, L.table_off), L.max_lh, L.max_lv, L.min_l, L.count, c->idwt_mode,
                              j->stream, ll, (const uint32_t *)j->d_coef.p, out, L.all_fast,
                              j->run.coef_is16 ? (L.level == 0 ? 2 : 1) : 0);   /* 16-bit sub-bands; at level 0 the LL band too */
}

template <int TYPE>
static void launch_fused_level(htj2k_job *j, const LevelLaunch &L, const uint32_t *ll)
{
    const int th = stream_strip_rows(L.max_lh, L.max_lv, L.count);
    const int tw = stream_strip_cols(L.max_lh, L.outk == 0 ? 3 : L.outk == 1 ? 6 : L.outk == 2 ? 1 : L.outk == 3 ? 2 : 0);
    const bool multi = (TYPE == J2K_DWT53 && j->run.coef_is16) || (TYPE != J2K_DWT97_INT && (L.outk >= 1 || (L.nc == 3 && L.all_fast)));   /* FASTONLY kernels */
    const int wpb = multi ? stream_wpb(L.max_lh, tw) : 1;
    const int occ_lds = stream_occ_lds(wpb);
    const StreamGrid G = stream_grid(L.max_lh, L.max_lv, th, L.count, tw, wpb);
    dim3 g(8 * G.per_xcd / wpb);
    const dim3 blk(64 * wpb);
    const DwtFusedArgs *tab = desc_at<DwtFusedArgs>(j, L.table_off);
    const PackTile *tiles = desc_at<PackTile>(j, j->idwt.pack_off);
    const uint32_t *band = (const uint32_t *)j->d_coef.p;
#define FUSED_FAST(NC_, C16_, LL16_, K_) hipLaunchKernelGGL((k_idwt_stream_pack<TYPE == J2K_DWT97_INT && (K_) ? J2K_DWT53 : TYPE, NC_, true, C16_, LL16_, K_>), g, blk, occ_lds, j->stream, tab, ll, band, tiles, th, G)
    if (TYPE == J2K_DWT53 && j->run.coef_is16) {             /* coef16_ok: every fused launch is a fast-store one */
        const bool l0 = L.level == 0 || j->run.ll16_run;      /* the LL band is 16-bit: the block decoder's, or the level below wrote it so */
        const bool pk = l0 && L.pk_bits && j->run.pk_run;   /* pairs of 16-bit samples all the way (pk16_eligibility) */
        const int pk_lds = pk ? stream_pk_lds(wpb) : 0;
        if (pk && (L.outk == 0 || L.outk == 2)) j->run.pk_used = L.level == 0 ? 16 : std::min(16, j->idwt.pk_bits);
        if (pk && L.outk == 0) {                         /* (more than 48 KiB of dynamic LDS: lds_opt_in_all) */
            hipLaunchKernelGGL((k_idwt_stream_pack<J2K_DWT53, 3, true, true, true, 0, true>), g, blk, pk_lds, j->stream, tab, ll, band, tiles, th, G);
        } else if (pk && L.outk == 2) {
            hipLaunchKernelGGL((k_idwt_stream_pack<J2K_DWT53, 1, true, true, true, 2, true>), g, blk, pk_lds, j->stream, tab, ll, band, tiles, th, G);
        }
        else if (L.outk == 0) { if (l0) FUSED_FAST(3, true, true, 0); else FUSED_FAST(3, true, false, 0); }
        else if (L.outk == 1) { if (l0) FUSED_FAST(3, true, true, 1); else FUSED_FAST(3, true, false, 1); }
        else if (L.outk == 2) { if (l0) FUSED_FAST(1, true, true, 2); else FUSED_FAST(1, true, false, 2); }
        else { if (l0) FUSED_FAST(1, true, true, 3); else FUSED_FAST(1, true, false, 3); }
    } else if (L.outk == 1) FUSED_FAST(3, false, false, 1);
    else if (L.outk == 2) FUSED_FAST(1, false, false, 2);
    else if (L.outk == 3) FUSED_FAST(1, false, false, 3);
    else if (L.nc == 1) hipLaunchKernelGGL((k_idwt_stream_pack<TYPE, 1, false>), g, dim3(64), 0, j->stream, tab, ll, band, tiles, th, G);
    else if (L.nc == 3 && L.all_fast) hipLaunchKernelGGL((k_idwt_stream_pack<TYPE, 3, true>), g, blk, occ_lds, j->stream, tab, ll, band, tiles, th, G);
    else if (L.nc == 3) hipLaunchKernelGGL((k_idwt_stream_pack<TYPE, 3, false>), g, dim3(64), 0, j->stream, tab, ll, band, tiles, th, G);
    else hipLaunchKernelGGL((k_idwt_stream_pack<TYPE, 4, false>), g, dim3(64), 0, j->stream, tab, ll, band, tiles, th, G);
}

static hipEvent_t lev_event(htj2k_job *j)
{
    if (j->run.lev_ev_used >= (int)j->lev_ev.size()) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        j->lev_ev.push_back(e);
    }
    return j->lev_ev[j->run.lev_ev_used++];
}

/* Levels 0-2 of every reversible plane as one launch (k_idwt_stream_ll16_x3), where the plan allows it (x3.ok) and the
 * windows fit the LDS of a workgroup.  Returns whether it ran: the loop of run_idwt then leaves those three launches out. */
static bool launch_x3(htj2k_ctx *c, htj2k_job *j, const std::vector<LevelLaunch> &LL)
{
    const IdwtPlan::X3 &X = j->idwt.x3;
    const int th = getenv("HTJ2K_X3_TH") ? std::max(8, atoi(getenv("HTJ2K_X3_TH")) & ~3) : 24;   /* C2: 91 us at 24 rows, 93 at 36, 97 at 16 or 48, 104 at 68 (three launches: 123) */
    const size_t lds = ((size_t)x3_win0_rows(th) * X.lh[0] + (size_t)x3_win1_rows(th) * X.lh[1]) * sizeof(uint16_t);
    if (lds > 64 * 1024) return false;
    const int nbands = (X.lv2 + th - 1) / th, total = nbands * X.count;
    hipEvent_t e0 = lev_event(j);
    if (e0) (void)hipEventRecord(e0, j->stream);
    bool x3pk = j->run.pk_run;                            /* all three levels on pairs of 16-bit samples, or none */
    for (const LevelLaunch &L : LL)
        if (L.type == J2K_DWT53 && L.nc == 0 && L.level < 3 && !L.pk_bits) x3pk = false;
    auto kern = x3pk ? k_idwt_stream_ll16_x3<true> : k_idwt_stream_ll16_x3<false>;
    hipLaunchKernelGGL(kern, dim3(8 * ((total + 7) / 8)), dim3(256), lds, j->stream,
                       desc_at<DwtTileArgs>(j, X.tab[0]), desc_at<DwtTileArgs>(j, X.tab[1]), desc_at<DwtTileArgs>(j, X.tab[2]),
                       (const uint32_t *)j->d_coef.p, buf_ptr(j, 1),
                       th, nbands, X.count, X.lh[0], X.lh[1], (int *)j->d_status.p + j->blocks.size(), ll16_check_bits(c, j));
    hipEvent_t e1 = lev_event(j);
    if (e1) (void)hipEventRecord(e1, j->stream);
    j->run.lev_bytes.push_back(X.alg);
    j->run.lev_hbm.push_back(X.hbm);
    return true;
}

/* The last plain level inside the final-level launch (k_idwt_stream_pack_x2): the two launches it replaces (null: it does
 * not run) and its shape */
struct X2Run {
    const LevelLaunch *plain = nullptr, *fused = nullptr;
    int th = 0, tw = 0, wpb = 0, lds = 0;      /* final-level rows per workgroup, strip width, waves per workgroup, dynamic LDS */
};

/* ... runs where the job qualifies (x2.ok), both levels run on pairs of 16-bit samples, x3 does not take the plain level,
 * and the windows fit the LDS of a workgroup */
static X2Run choose_x2(const htj2k_ctx *c, const htj2k_job *j, const std::vector<LevelLaunch> &LL, bool fuse, bool x3)
{
    const IdwtPlan::X2 &X = j->idwt.x2;
    X2Run R;
    if (!(fuse && j->run.ll16_run && j->run.coef_is16 && j->run.pk_run && X.ok && c->idwt_x2 &&
          (c->idwt_x2 == 1 || X.ll_bytes >= (double)c->idwt_x2_min_bytes))) return R;
    const LevelLaunch &P = LL[X.plain], &Q = LL[X.fused];
    if (!(P.pk_bits && Q.pk_bits && !(x3 && P.level < 3))) return R;
    R.tw = stream_strip_cols(Q.max_lh, 3);
    R.wpb = stream_wpb(Q.max_lh, R.tw);
    R.th = c->idwt_x2_th;
    auto win = [&](int th) { return (size_t)3 * x2_win_rows(th) * x2_win_cols(R.wpb, R.tw) * sizeof(uint16_t); };
    while (R.th > 4 && win(R.th) > (size_t)c->max_dyn_lds) R.th -= 2;
    /* at least what the packed final level reserves to hold the CU at 16 waves (stream_pk_lds) */
    R.lds = (int)std::max(win(R.th), (size_t)stream_pk_lds(R.wpb));
    /* (not opted in to that much LDS: the two launches, as without the knob) */
    const bool fits = win(R.th) <= (size_t)c->max_dyn_lds && (R.lds <= 48 * 1024 || c->x2_lds_ok);
    if (fits) { R.plain = &P; R.fused = &Q; }
    return R;
}

static void launch_x2(htj2k_ctx *c, htj2k_job *j, const X2Run &R)
{
    const LevelLaunch &P = *R.plain, &L = *R.fused;
    X2Grid G;
    G.tw = R.tw;
    G.gx = (L.max_lh + R.wpb * R.tw - 1) / (R.wpb * R.tw);
    G.gy = (L.max_lv + R.th - 1) / R.th;
    G.total = G.gx * G.gy * L.count;
    G.per_xcd = (G.total + 7) / 8;
    j->run.pk_used = std::min(16, j->idwt.pk_bits);
    hipLaunchKernelGGL((k_idwt_stream_pack_x2<3, 0, true>), dim3(8 * G.per_xcd), dim3(64 * R.wpb), R.lds, j->stream,
                       desc_at<DwtTileArgs>(j, P.table_off), desc_at<DwtFusedArgs>(j, L.table_off),
                       (const uint32_t *)ll_buf(j, P.level), (const uint32_t *)j->d_coef.p,
                       desc_at<PackTile>(j, j->idwt.pack_off), R.th, G,
                       (int *)j->d_status.p + j->blocks.size(), ll16_check_bits(c, j));
}

static int run_idwt(htj2k_ctx *c, htj2k_job *j, bool use_tile, bool fuse)
{
    j->run.lev_ev_used = 0;
    j->run.lev_bytes.clear();
    j->run.lev_hbm.clear();
    j->run.pk_run = c->idwt_pk != 0;
    j->run.pk_used = 0;
    const std::vector<LevelLaunch> &LL = fuse ? j->idwt.launches_fused : use_tile ? j->idwt.launches_tile : j->idwt.launches_generic;
    const bool x3 = fuse && j->run.ll16_run && j->idwt.x3.ok && c->idwt_x3 && launch_x3(c, j, LL);
    const X2Run x2 = choose_x2(c, j, LL, fuse, x3);
    for (const LevelLaunch &L : LL) {
        if (x3 && L.type == J2K_DWT53 && L.nc == 0 && L.level < 3) continue;     /* done by k_idwt_stream_ll16_x3 */
        if (&L == x2.plain) continue;                                            /* done with the final level below */
        hipEvent_t e0 = lev_event(j);
        if (e0) (void)hipEventRecord(e0, j->stream);
        if (&L == x2.fused) {
            launch_x2(c, j, x2);
            hipEvent_t e1 = lev_event(j);
            if (e1) (void)hipEventRecord(e1, j->stream);
            j->run.lev_bytes.push_back(j->idwt.x2.alg);
            j->run.lev_hbm.push_back(j->idwt.x2.hbm);
            continue;
        }
        with_dwt_type(L.type, [&](auto T) {
            constexpr int TYPE = decltype(T)::value;
            if (L.nc) launch_fused_level<TYPE>(j, L, ll_buf(j, L.level));
            else if (!use_tile) launch_generic_level<TYPE>(j, L);
            else launch_tile_level<TYPE>(c, j, L, ll_buf(j, L.level), buf_ptr(j, 1 + (L.level & 1)));
        });
        hipEvent_t e1 = lev_event(j);
        if (e1) (void)hipEventRecord(e1, j->stream);
        j->run.lev_bytes.push_back(L.alg_bytes);
        /* bytes that have to move: a level reads its LL quarter and three sub-band quarters and writes every sample
         * (alg_bytes = 8 per sample); the fused level writes the packed pixels instead (hbm_bytes = 4 + out per
         * sample).  With 16-bit sub-bands three quarters of the reads are 2 bytes (all of them at level 0). */
        double hb = L.nc ? L.hbm_bytes : L.alg_bytes;
        if (j->run.coef_is16) hb -= L.alg_bytes / 8.0 * ((L.level == 0 || j->run.ll16_run) ? 2.0 : 1.5);
        if (j->run.ll16_run && !L.nc) hb -= L.alg_bytes / 8.0 * 2.0;            /* ... and writes 2 instead of 4 bytes per sample */
        j->run.lev_hbm.push_back(hb);
    }
    return 0;
}

static int run_stages(htj2k_ctx *c, htj2k_job *j, int mask, bool force_ll32)
{
    if (!c || !j || j->nframes <= 0 || !j->uploaded) return HTJ2K_ERR_EINVAL;
    const int nall = (int)j->blocks.size(), ntc = (int)j->tilecomps.size();
    /* A call gives the right result or is refused before anything is launched ("A job used again").
     * The pack stage without the IDWT needs the planes: an IDWT run that was not fused (a fused run never writes the final
     * planes, plane_fused) and no block stage since -- nor one in this call that writes over a plane in the coefficient
     * buffer */
    if ((mask & 6) == 4) {
        bool ok = j->run.planes_ok;
        for (int t = 0; ok && (mask & 1) && t < ntc; t++) ok = j->final_eff[t] != 0;
        if (!ok) return HTJ2K_ERR_EINVAL;
    }
    /* The IDWT without the block stage needs the sub-bands as the path the knobs select NOW reads them: the generic
     * kernels transform in place, and only the streaming kernels read 16-bit sub-bands.  Otherwise the block stage runs
     * again first (a mask other than 7 gives 32-bit sub-bands) */
    if ((mask & 2) && !(mask & 1) && (!j->run.coef_ok || (j->run.coef_is16 && c->idwt_mode != 3))) mask |= 1;
    HIP_TRY(c, hipSetDevice(c->device));
    if (mask & 1) {
        const BlockLayout &L = j->lay;
        HIP_TRY(c, hipEventRecord(j->ev[2], j->stream));
        if (nall) HIP_TRY(c, hipMemsetAsync(j->d_status.p, 0, ((size_t)nall + 1) * sizeof(int), j->stream));   /* + the LL overflow flag */
        if (nall > L.nht) {
            unsigned nwide = 0;                                      /* waves holding a block wider than 64 columns (sorted to the front) */
            while (nwide < L.mqwaves.size() && L.mqwaves[nwide].chunks > 1) nwide++;
            HIP_TRY(c, launch_mq_blocks(j->stream, *j, L, nwide));
        }
        j->run.coef_is16 = false;
        if (L.nht) {
            const HtChoice k = job_ht_choice(c, j, mask);
            j->run.coef_is16 = k.coef16;
            j->run.ht_bpw = k.bpw;
            HIP_TRY(c, launch_ht_blocks(j->stream, c->d_tables, *j, L, k));
        }
        HIP_TRY(c, hipEventRecord(j->ev[3], j->stream));
        j->run.coef_ok = true;
        if ((mask & 7) == 1) {                                   /* the planes are the sub-bands again (htj2k_job_read_plane) */
            j->final_eff.assign(ntc, 0);
            j->run.fused_last = false;
            j->run.planes_ok = false;
        }
    }
    if (mask & 6) {
        const bool use_tile = c->idwt_mode != 0 && j->idwt.tile_ok;
        const bool fuse = use_tile && c->idwt_mode == 3 && c->fuse_pack && (mask & 6) == 6 && j->idwt.any_fusable;
        if (mask & 2)
            for (int t = 0; t < ntc; t++) j->final_eff[t] = use_tile ? j->idwt.final_buf[t] : 0;
        j->run.fused_last = fuse;
        /* one upload of all descriptor tables, pack source pointers patched for where the
         * planes are (or will be) after the IDWT */
        PackTile *T = (PackTile *)(j->h_desc.data() + j->idwt.pack_off);
        int ti = 0;
        for (int f = 0; f < j->nframes; f++) {
            const FrameSlot &F = j->frames[f];
            for (int k = 0; k < F.plan->ntiles; k++, ti++) {
                T[ti].fused = fuse && j->idwt.tile_fusable[ti];
                for (int cc = 0; cc < T[ti].ncomp; cc++) {
                    const int t = F.tc_base + k * T[ti].ncomp + cc;
                    T[ti].c[cc].src = buf_ptr(j, j->final_eff[t]) + j->tilecomps[t].plane_off;
                }
            }
        }
        if (!(mask & 1)) HIP_TRY(c, hipEventRecord(j->ev[3], j->stream));
        /* the tables only change with the knobs (which buffer a plane ends in, fused or not): a run whose tables are what the
         * device already holds uploads nothing -- a pageable copy in the middle of the stream, once per step, otherwise */
        if (j->h_desc != j->h_desc_dev) {
            HIP_TRY(c, hipMemcpyAsync(j->d_desc.p, j->h_desc.data(), j->h_desc.size(), hipMemcpyHostToDevice, j->stream));
            j->h_desc_dev = j->h_desc;
        }
        if (mask & 2) {
            /* coef16_ok has checked that every level of every plane is a FASTONLY streaming launch and every plane ends fused */
            j->run.ll16_run = c->ll16 && j->run.coef_is16 && fuse && use_tile && !force_ll32;
            j->run.ll16_checked = !j->run.ll16_run;
            if (!force_ll32) j->run.ll16_fallbacks = 0;
            /* (the block stage clears the overflow flag with the blocks' status; without it an earlier run's may stand) */
            if (j->run.ll16_run && !(mask & 1)) HIP_TRY(c, hipMemsetAsync((int *)j->d_status.p + nall, 0, sizeof(int), j->stream));
            int r = run_idwt(c, j, use_tile, fuse);
            if (r < 0) return r;
            HIP_TRY(c, hipGetLastError());
            j->run.coef_ok = use_tile;                               /* k_idwt_h / k_idwt_v leave the planes in the coefficient buffer */
            j->run.planes_ok = !fuse;
        }
        HIP_TRY(c, hipEventRecord(j->ev[4], j->stream));
    }
    if (mask & 4) {
        bool all_fused = j->run.fused_last;
        for (size_t i = 0; all_fused && i < j->idwt.tile_fusable.size(); i++) all_fused = j->idwt.tile_fusable[i] != 0;
        if (j->idwt.npack && j->idwt.pack_maxw > 0 && j->idwt.pack_maxh > 0 && !all_fused) {
            dim3 g((j->idwt.pack_maxw + 1023) / 1024, j->idwt.pack_maxh, j->idwt.npack);
            hipLaunchKernelGGL(k_mct_pack, g, dim3(256), 0, j->stream, desc_at<PackTile>(j, j->idwt.pack_off));
            HIP_TRY(c, hipGetLastError());
        }
        HIP_TRY(c, hipEventRecord(j->ev[5], j->stream));
    }
    j->run.ran |= mask;
    j->run.frames_ok = (mask & 4) != 0;
    return 0;
}

extern "C" int htj2k_job_run_stages(htj2k_ctx *c, htj2k_job *j, int mask) { return run_stages(c, j, mask, false); }
extern "C" int htj2k_job_run(htj2k_ctx *c, htj2k_job *j) { return run_stages(c, j, 7, false); }

/* Wait for the job's stream; if its last IDWT run kept the LL bands as 16-bit samples, look at the overflow flag once and,
 * if a sample did not fit, run the transform again with 32-bit LL bands (the sub-bands are still there) */
static int job_settle(htj2k_ctx *c, htj2k_job *j)
{
    HIP_TRY(c, hipStreamSynchronize(j->stream));
    if (j->run.ll16_checked) return 0;
    j->run.ll16_checked = true;
    int flag = 0;
    HIP_TRY(c, hipMemcpy(&flag, (const int *)j->d_status.p + j->blocks.size(), sizeof(int), hipMemcpyDeviceToHost));
    if (!flag) return 0;
    clog(c, LOG_INFO, "an LL band left the 16-bit range: inverse DWT run again with 32-bit LL bands\n");
    j->run.ll16_fallbacks++;
    const int r = run_stages(c, j, 6, true);
    if (r < 0) return r;
    HIP_TRY(c, hipStreamSynchronize(j->stream));
    return 0;
}

extern "C" int htj2k_job_wait(htj2k_ctx *c, htj2k_job *j)
{
    if (!c || !j) return HTJ2K_ERR_EINVAL;
    return job_settle(c, j);
}

/* 0: the last run's LL bands were 32-bit, 1: 16-bit, 2: 16-bit, overflowed and run again with 32 (after htj2k_job_wait) */
extern "C" int htj2k_job_idwt_packed(const htj2k_job *j) { return j ? j->run.pk_used : HTJ2K_ERR_EINVAL; }
extern "C" int htj2k_job_ll16(const htj2k_job *j) { return j ? (j->run.ll16_run ? 1 : (j->run.ll16_fallbacks ? 2 : 0)) : HTJ2K_ERR_EINVAL; }

extern "C" int htj2k_job_stage_ms(htj2k_ctx *c, htj2k_job *j, float *ms_ht, float *ms_idwt, float *ms_pack)
{
    if (!c || !j) return HTJ2K_ERR_EINVAL;
    HIP_TRY(c, hipStreamSynchronize(j->stream));
    float a = 0, b = 0, d = 0;
    if (j->run.ran & 1) (void)hipEventElapsedTime(&a, j->ev[2], j->ev[3]);
    if (j->run.ran & 2) (void)hipEventElapsedTime(&b, j->ev[3], j->ev[4]);
    if (j->run.ran & 4) (void)hipEventElapsedTime(&d, j->ev[4], j->ev[5]);
    if (ms_ht) *ms_ht = a;
    if (ms_idwt) *ms_idwt = b;
    if (ms_pack) *ms_pack = d;
    return 0;
}

/* per-launch device time and algorithmic bytes (2 * 4 * lh * lv summed over the planes of
 * the launch) of the IDWT kernels of the job's last run: the roofline inputs of bench.py */
extern "C" int htj2k_job_idwt_launches(htj2k_ctx *c, htj2k_job *j, float *ms, double *bytes, int cap)
{
    if (!c || !j) return HTJ2K_ERR_EINVAL;
    HIP_TRY(c, hipStreamSynchronize(j->stream));
    const int n = (int)j->run.lev_bytes.size();
    for (int i = 0; i < n && i < cap; i++) {
        float t = 0;
        (void)hipEventElapsedTime(&t, j->lev_ev[2 * i], j->lev_ev[2 * i + 1]);
        if (ms) ms[i] = t;
        if (bytes) bytes[i] = j->run.lev_bytes[i];
    }
    return n;
}

/* 1 when the last htj2k_job_run kept the sub-bands as 16-bit samples between the block decoder and the IDWT */
extern "C" int htj2k_job_coef16(const htj2k_job *j) { return j ? (j->run.coef_is16 ? 1 : 0) : HTJ2K_ERR_EINVAL; }
extern "C" int htj2k_job_ht_blocks_per_wave(const htj2k_job *j) { return j ? j->run.ht_bpw : HTJ2K_ERR_EINVAL; }

extern "C" int htj2k_job_idwt_hbm_bytes(htj2k_ctx *c, htj2k_job *j, double *bytes, int cap)
{
    if (!c || !j) return HTJ2K_ERR_EINVAL;
    const int n = (int)j->run.lev_hbm.size();
    for (int i = 0; i < n && i < cap; i++)
        if (bytes) bytes[i] = j->run.lev_hbm[i];
    return n;
}

/* From here on: reads of device state.  Between a parse and the upload the buffers still hold (and are sized for) the
 * content before, so these calls are refused until the job is uploaded, before the stream or a buffer is touched */
extern "C" int htj2k_job_block_errors(htj2k_ctx *c, htj2k_job *j)
{
    if (!c || !j || j->nframes <= 0 || !j->uploaded) return HTJ2K_ERR_EINVAL;
    const int n = (int)j->blocks.size();
    if (!n) return 0;
    std::vector<int> st(n);
    HIP_TRY(c, hipStreamSynchronize(j->stream));
    HIP_TRY(c, hipMemcpy(st.data(), j->d_status.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    int e = 0;
    for (int i = 0; i < n; i++) e += st[i] != 0;
    return e;
}

extern "C" int htj2k_job_read_plane(htj2k_ctx *c, htj2k_job *j, int tc, void *dst, size_t dst_bytes)
{
    if (!c || !j || j->nframes <= 0 || !j->uploaded || tc < 0 || tc >= (int)j->tilecomps.size()) return HTJ2K_ERR_EINVAL;
    const J2kTileComp &t = j->tilecomps[tc];
    const size_t n = (size_t)t.w * t.h * 4;
    if (dst_bytes < n) return HTJ2K_ERR_EINVAL;
    const int fb = j->final_eff.empty() ? 0 : j->final_eff[tc];
    if (j->run.fused_last && !j->idwt.plane_fused.empty() && j->idwt.plane_fused[tc]) return HTJ2K_ERR_EINVAL;   /* never materialised */
    if (!j->run.ll16_checked) { const int r = job_settle(c, j); if (r < 0) return r; }
    HIP_TRY(c, hipStreamSynchronize(j->stream));
    HIP_TRY(c, hipMemcpy(dst, buf_ptr(j, fb) + t.plane_off, n, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int htj2k_job_download_frame(htj2k_ctx *c, htj2k_job *j, int f, htj2k_frame *frame)
{
    if (!c || !j || f < 0 || f >= j->nframes || !j->uploaded || !frame) return HTJ2K_ERR_EINVAL;
    const FrameSlot &F = j->frames[f];
    const J2kPlan *pl = F.plan;
    if (!j->run.ll16_checked) { const int r = job_settle(c, j); if (r < 0) return r; }
    for (int p = 0; p < pl->info.nplanes; p++) {
        const int rowbytes = pl->info.plane_width[p] * pl->info.plane_bytes_per_sample[p];
        if (!frame->data[p] || frame->linesize[p] < rowbytes) return HTJ2K_ERR_EINVAL;
        HIP_TRY(c, hipMemcpy2DAsync(frame->data[p], frame->linesize[p], F.d_out[p].p, F.out.linesize[p],
                                    rowbytes, pl->info.plane_height[p], hipMemcpyDeviceToHost, j->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(j->stream));
    frame->width = pl->info.width;
    frame->height = pl->info.height;
    frame->pix_fmt = pl->info.pix_fmt;
    return 0;
}

extern "C" int htj2k_job_download(htj2k_ctx *c, htj2k_job *j, htj2k_frame *frame)
{
    return htj2k_job_download_frame(c, j, 0, frame);
}

/* a parsed frame's output planes where the job keeps them on the device, as a frame */
static void job_frame_view(const FrameSlot &F, htj2k_frame *frame)
{
    const htj2k_info &I = F.plan->info;
    memset(frame, 0, sizeof(*frame));
    for (int p = 0; p < I.nplanes && p < 4; p++) {
        frame->data[p] = F.out.ptr[p];
        frame->linesize[p] = F.out.linesize[p];
    }
    frame->width = I.width;
    frame->height = I.height;
    frame->pix_fmt = I.pix_fmt;
}

/* device addresses / pitches of the output planes of frame f (for callers that keep frames on the GPU); valid
 * until the job is parsed again */
extern "C" int htj2k_job_device_frame(htj2k_ctx *c, htj2k_job *j, int f, htj2k_frame *frame)
{
    if (!c || !j || f < 0 || f >= j->nframes || !j->uploaded || !frame) return HTJ2K_ERR_EINVAL;
    /* the planes are final only once the 16-bit LL check of the last run has been looked at (and the transform run
     * again if it tripped): that also waits for the job's stream */
    if (!j->run.ll16_checked) { const int r = job_settle(c, j); if (r < 0) return r; }
    job_frame_view(j->frames[f], frame);
    return 0;
}

/* device address of an output plane of frame 0 (for callers that keep frames on the GPU); htj2k_job_wait must have
 * returned since the last run: only then are the planes final (this call has no context to wait with) */
extern "C" void *htj2k_job_device_plane(htj2k_job *j, int plane, int *linesize)
{
    if (!j || j->nframes <= 0 || !j->uploaded || plane < 0 || plane > 3) return nullptr;
    if (linesize) *linesize = j->frames[0].out.linesize[plane];
    return j->frames[0].out.ptr[plane];
}

/* ------------------------------------------------------------------ measuring frames (cmp_kernels.hpp)
 * Differences (k_frame_diff), SSIM (k_frame_ssim) and checksums (k_frame_adler) of frames where they are.  All three are
 * one staged call (MeasCall) over a table of planes; a metric says which planes take part, fills its entries and turns
 * the sums into its result. */
using namespace htj2k_cmp;

/* width and height of component k of a w x h picture: components 1 and 2 are shifted by the chroma shifts, rounded up */
static int pix_comp_w(const J2kPixDesc *pd, int w, int k) { const int s = (k == 1 || k == 2) ? pd->log2_chroma_w : 0; return (int)(((int64_t)w + (1 << s) - 1) >> s); }
static int pix_comp_h(const J2kPixDesc *pd, int h, int k) { const int s = (k == 1 || k == 2) ? pd->log2_chroma_h : 0; return (int)(((int64_t)h + (1 << s) - 1) >> s); }

/* the bytes of a row of plane p that hold samples, and its rows: a planar layout's plane is its component, any other
 * layout has all components in plane 0 */
struct PlaneGeo { size_t rowbytes; int rows; };
static PlaneGeo pix_plane(const J2kPixDesc *pd, int w, int h, int p)
{
    if (!pd->planar) return { (size_t)w * pd->nb_components * pd->bytes, h };
    return { (size_t)pix_comp_w(pd, w, p) * pd->bytes, pix_comp_h(pd, h, p) };
}

static size_t meas_pitch(size_t rowbytes) { return (rowbytes + 15) & ~(size_t)15; }

/* a table entry's `aligned`, from the pointers and linesizes it ends up with */
static uint32_t meas_aligned(const void *a, int64_t lsa, const void *b = nullptr, int64_t lsb = 0)
{
    return (((uintptr_t)a | (uintptr_t)b | (uint64_t)lsa | (uint64_t)lsb) & 15) == 0;
}

/* The call every metric makes, under cmp_mutex for as long as it lives.  The staging image is the plane table, then the
 * host operands' planes, rows at a pitch of a multiple of 16 so that uploaded operands take the aligned path; its device
 * copy has the results in front.  What the kernels rely on is stated here once: all slots' results are zeroed, only the
 * rowbytes of a source row are read, and cmp_ms is 0 when nothing was launched. */
struct MeasCall {
    htj2k_ctx *const c;
    std::lock_guard<std::mutex> lk;
    uint8_t *h = nullptr, *d = nullptr;    /* the image and its place on the device */
    size_t at = 0;                         /* bytes of it in use */
    std::vector<uint8_t> sums;             /* every slot's results, after run() */

    explicit MeasCall(htj2k_ctx *ctx) : c(ctx), lk(ctx->cmp_mutex) {}

    /* room for `slots` results, `entries` table entries and staged_bytes of planes (meas_pitch x rows each) */
    int reserve(size_t slots, size_t slot_bytes, size_t entries, size_t entry_bytes, size_t staged_bytes)
    {
        HIP_TRY(c, hipSetDevice(c->device));
        if (!c->cmp_stream) {
            HIP_TRY(c, hipStreamCreateWithFlags(&c->cmp_stream, hipStreamNonBlocking));
            for (hipEvent_t &e : c->cmp_ev) HIP_TRY(c, hipEventCreate(&e));
        }
        auto r256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
        const size_t sums_bytes = r256(slots * slot_bytes), tab_bytes = r256(entries * entry_bytes);
        h = (uint8_t *)c->cmp_h.ensure(tab_bytes + staged_bytes);
        if (!h) return HTJ2K_ERR_ENOMEM;
        const int r = c->cmp_d.ensure(sums_bytes + tab_bytes + staged_bytes);
        if (r < 0) return r;
        d = (uint8_t *)c->cmp_d.p + sums_bytes;
        at = tab_bytes;
        sums.assign(slots * slot_bytes, 0);
        return 0;
    }

    /* a host operand's plane into the image: where the kernel will find it, and its linesize there */
    void stage(const htj2k_frame &f, int p, PlaneGeo g, const uint8_t **base, int64_t *ls)
    {
        const size_t pitch = meas_pitch(g.rowbytes);
        for (int y = 0; y < g.rows; y++)
            memcpy(h + at + (size_t)y * pitch, f.data[p] + (size_t)y * f.linesize[p], g.rowbytes);
        *base = d + at;
        *ls = (int64_t)pitch;
        at += pitch * g.rows;
    }

    /* bytes (a multiple of 16, counted in reserve's staged_bytes) into the image behind what is there: their place on the device */
    const void *put(const void *src, size_t bytes)
    {
        memcpy(h + at, src, bytes);
        const void *p = d + at;
        at += bytes;
        return p;
    }

    /* launch(stream, d_table, d_sums) -> 0 or an error, over the nt entries at h; not called when nt is 0 */
    template <class Launch> int run(size_t nt, Launch launch)
    {
        hipStream_t st = c->cmp_stream;
        void *d_sums = c->cmp_d.p;
        if (!sums.empty()) HIP_TRY(c, hipMemsetAsync(d_sums, 0, sums.size(), st));     /* a call without results: frames as tensors */
        HIP_TRY(c, hipMemcpyAsync(d, h, at, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipEventRecord(c->cmp_ev[0], st));
        if (nt) {
            const int r = launch(st, (const void *)d, d_sums);
            if (r < 0) return r;
            HIP_TRY(c, hipGetLastError());
        }
        HIP_TRY(c, hipEventRecord(c->cmp_ev[1], st));
        if (!sums.empty()) HIP_TRY(c, hipMemcpyAsync(sums.data(), d_sums, sums.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        c->cmp_ms = 0;
        if (nt) (void)hipEventElapsedTime(&c->cmp_ms, c->cmp_ev[0], c->cmp_ev[1]);
        return 0;
    }
};

/* a kernel over a table of nt planes, in chunks of the 65535 entries grid.z takes (as the encoder's plane launches).
 * grid.x: the most work of any plane, `per` units of it a workgroup; fewer workgroups a plane where there are many planes */
template <class Kernel, class Plane, class Sums, class... Args>
static void meas_launch(Kernel kernel, hipStream_t st, const Plane *d_planes, size_t nt, size_t work, size_t per, Sums *d_sums, Args... args)
{
    const unsigned gx = (unsigned)std::min<size_t>((work + per - 1) / per, nt >= 64 ? 256 : 2048);
    for (size_t z0 = 0; z0 < nt; z0 += 65535)
        hipLaunchKernelGGL(kernel, dim3(gx, 1, (unsigned)std::min<size_t>(65535, nt - z0)), dim3(CMP_THREADS), 0, st,
                           d_planes + z0, d_sums, args...);
}


/* ---- pairs of frames: what AV_CODEC_FLAG_PSNR makes an encoder report (AVCodecContext.error[],
 * ff_side_data_set_encoder_stats), and SSIM beside it, for any two frames of one layout: exact integer sums per component
 * from one launch over all frames of the call. */
struct CmpLayout {                     /* what a call's frames share */
    const J2kPixDesc *pd;
    int nplanes, bytes, step;
    uint32_t shift, mask;
};

/* the shift k_enc_unpack reads a sample with (j2k_enc.c: enc_frame_init; the inverse of j2k_plan.c's out_shift_precision) */
static int cmp_shift(int pix_fmt, int bits)
{
    return bits <= 8 ? 8 - bits
         : (pix_fmt == HTJ2K_PIX_RGB48 || pix_fmt == HTJ2K_PIX_RGBA64 || pix_fmt == HTJ2K_PIX_GRAY16 || pix_fmt == HTJ2K_PIX_XYZ12) ? 16 - bits : 0;
}

static int cmp_layout(int pix_fmt, int bits, CmpLayout *L)
{
    const J2kPixDesc *pd = j2k_pix_desc(pix_fmt);
    if (!pd) return HTJ2K_ERR_EINVAL;
    if (pd->pal) return HTJ2K_ERR_PATCHWELCOME;           /* indices are not samples */
    if (bits < 1 || bits > pd->depth[0]) return HTJ2K_ERR_EINVAL;
    L->pd = pd;
    L->nplanes = pd->planar ? pd->nb_components : 1;
    L->bytes = pd->bytes;
    L->step = pd->planar ? 1 : pd->nb_components;
    L->shift = (uint32_t)cmp_shift(pix_fmt, bits);
    L->mask = (1u << bits) - 1;
    return 0;
}

/* one operand of a pair: present, of the call's layout, every plane there with a linesize that holds the row */
static bool cmp_frame_ok(const CmpLayout &L, const htj2k_frame &f, int pix_fmt)
{
    if (f.pix_fmt != pix_fmt || f.width < 1 || f.height < 1 || (int64_t)f.width * L.step * L.bytes > INT32_MAX) return false;
    for (int p = 0; p < L.nplanes; p++)
        if (!f.data[p] || f.linesize[p] < 0 || (size_t)f.linesize[p] < pix_plane(L.pd, f.width, f.height, p).rowbytes) return false;
    return true;
}

/* f(bytes per sample, interleaved components per plane), both as integral constants: the kernels' <BYTES, STEP> */
template <class F> static int cmp_dispatch(const CmpLayout &L, F f)
{
    using std::integral_constant;
    switch (L.bytes * 8 + L.step) {
    case 8 + 1:  f(integral_constant<int, 1>(), integral_constant<int, 1>()); break;
    case 8 + 2:  f(integral_constant<int, 1>(), integral_constant<int, 2>()); break;
    case 8 + 3:  f(integral_constant<int, 1>(), integral_constant<int, 3>()); break;
    case 8 + 4:  f(integral_constant<int, 1>(), integral_constant<int, 4>()); break;
    case 16 + 1: f(integral_constant<int, 2>(), integral_constant<int, 1>()); break;
    case 16 + 2: f(integral_constant<int, 2>(), integral_constant<int, 2>()); break;
    case 16 + 3: f(integral_constant<int, 2>(), integral_constant<int, 3>()); break;
    case 16 + 4: f(integral_constant<int, 2>(), integral_constant<int, 4>()); break;
    default: return HTJ2K_ERR_BUG;
    }
    return 0;
}

#define SSIM_ROWS_DEFAULT 16           /* block rows per strip (DESIGN.md 3.5 has the sweep) */

/* block columns and rows of component k, and its windows: (bw - 1)(bh - 1), 0 where cw < 8 or ch < 8 */
static uint64_t ssim_nwin(const CmpLayout &L, int w, int h, int k)
{
    const uint64_t bw = (uint64_t)pix_comp_w(L.pd, w, k) >> 2, bh = (uint64_t)pix_comp_h(L.pd, h, k) >> 2;
    return bw < 2 || bh < 2 ? 0 : (bw - 1) * (bh - 1);
}

/* wave items of a plane under k_frame_ssim: strips x runs of 63 groups */
static size_t ssim_items(const CmpLayout &L, size_t rowbytes, int rows, int strip)
{
    const size_t unit = (size_t)4 * L.step * L.bytes, group = L.step == 3 ? (L.bytes == 1 ? 24 : 48) : std::max<size_t>(unit, 16);   /* SsimShape */
    const size_t bw = rowbytes / unit, bh = (size_t)rows >> 2;
    if (bw < 2 || bh < 2) return 0;
    const size_t nb = group / unit, gw = (bw - 1 + nb - 1) / nb;
    return ((gw + SSIM_LANES - 1) / SSIM_LANES) * ((bh - 1 + strip - 1) / strip);
}

static void ssim_result(const CmpLayout &L, int w, int h, const SsimSums *S, htj2k_frame_ssim *o)
{
    memset(o, 0, sizeof *o);
    double num = 0, den = 0;
    for (int k = 0; k < 4; k++) {
        o->nwin[k] = k < L.pd->nb_components ? ssim_nwin(L, w, h, k) : 0;
        o->q32[k] = S && o->nwin[k] ? (int64_t)S->q[k] : 0;
        o->ssim[k] = o->nwin[k] ? (double)o->q32[k] / 4294967296.0 / (double)o->nwin[k] : (double)NAN;
        if (o->nwin[k]) {
            const double wt = (double)pix_comp_w(L.pd, w, k) * (double)pix_comp_h(L.pd, h, k);
            num += o->ssim[k] * wt;
            den += wt;
        }
    }
    o->all = den > 0 ? num / den : (double)NAN;
}

static void cmp_result(const CmpLayout &L, int bits, int w, int h, const CmpSums &S, htj2k_frame_diff *o)
{
    memset(o, 0, sizeof *o);
    unsigned long long se = 0, ns = 0;
    for (int k = 0; k < L.pd->nb_components; k++) {
        o->sse[k] = S.sse[k];
        o->ndiff[k] = S.ndiff[k];
        o->max_abs[k] = (uint32_t)S.max_abs[k];
        o->nsamples[k] = (uint64_t)pix_comp_w(L.pd, w, k) * (uint64_t)pix_comp_h(L.pd, h, k);
        se += S.sse[k];
        ns += o->nsamples[k];
    }
    const double peak = (double)((1u << bits) - 1);
    o->psnr = se == 0 ? (double)INFINITY : 10.0 * log10(peak * peak * (double)ns / (double)se);
}

/* The two metrics of a pair: its sums, a plane's work in the units of the kernel's grid (0: the plane takes no part),
 * the launch, and sums to result. */
struct DiffMetric {
    typedef CmpSums Sums;
    const CmpLayout &L;
    int bits;
    htj2k_frame_diff *out;
    /* a lane per group and step; enough workgroups to fill the device twice over when one frame is all there is */
    size_t work(PlaneGeo g) const { const size_t group = L.step == 3 ? 48 : 16; return ((g.rowbytes + group - 1) / group) * (size_t)g.rows; }
    int launch(hipStream_t st, const CmpPlane *dp, size_t nt, size_t most, CmpSums *ds) const
    {
        const CmpFmt F = { L.shift, L.mask };
        return cmp_dispatch(L, [&](auto B, auto S) {
            meas_launch(k_frame_diff<decltype(B)::value, decltype(S)::value>, st, dp, nt, most, CMP_THREADS, ds, F);
        });
    }
    void result(int i, int w, int h, const CmpSums &S) const { cmp_result(L, bits, w, h, S, &out[i]); }
};

struct SsimMetric {
    typedef SsimSums Sums;
    const CmpLayout &L;
    int strip;
    htj2k_frame_ssim *out;
    /* a wave per item and step; k_frame_ssim must not meet a plane without a window: such planes have no work */
    size_t work(PlaneGeo g) const { return ssim_items(L, g.rowbytes, g.rows, strip) * 64; }
    int launch(hipStream_t st, const CmpPlane *dp, size_t nt, size_t most, SsimSums *ds) const
    {
        const long long peak2 = (long long)L.mask * L.mask;
        const SsimFmt F = { L.shift, L.mask, (uint32_t)strip, 0, (64 * peak2 + 5000) / 10000, (36288 * peak2 + 5000) / 10000 };
        return cmp_dispatch(L, [&](auto B, auto S) {
            meas_launch(k_frame_ssim<decltype(B)::value, decltype(S)::value>, st, dp, nt, most, CMP_THREADS, ds, F);
        });
    }
    void result(int i, int w, int h, const SsimSums &S) const { ssim_result(L, w, h, &S, &out[i]); }
};

/* the checked call: pairs i with skip[i] set (skip may be NULL) take no part and keep what the metric's `out` holds for them */
template <class Metric>
static int pair_run(htj2k_ctx *c, const CmpLayout &L, const htj2k_frame *a, int a_dev, const htj2k_frame *b, int b_dev, int n,
                    const uint8_t *skip, const Metric &m)
{
    typedef typename Metric::Sums Sums;
    MeasCall call(c);
    auto geo = [&](int i, int p) { return pix_plane(L.pd, a[i].width, a[i].height, p); };
    auto work = [&](int i, int p) { return skip && skip[i] ? 0 : m.work(geo(i, p)); };
    size_t staged = 0, nt = 0, most = 1;
    for (int i = 0; i < n; i++)
        for (int p = 0; p < L.nplanes; p++)
            if (work(i, p)) staged += (size_t)(!a_dev + !b_dev) * meas_pitch(geo(i, p).rowbytes) * geo(i, p).rows;
    int r = call.reserve((size_t)n, sizeof(Sums), (size_t)n * L.nplanes, sizeof(CmpPlane), staged);
    if (r < 0) return r;
    CmpPlane *tab = (CmpPlane *)call.h;
    for (int i = 0; i < n; i++) {
        for (int p = 0; p < L.nplanes; p++) {
            if (!work(i, p)) continue;
            const PlaneGeo g = geo(i, p);
            CmpPlane &P = tab[nt++];
            memset(&P, 0, sizeof P);
            if (a_dev) { P.a = a[i].data[p]; P.lsa = a[i].linesize[p]; } else call.stage(a[i], p, g, &P.a, &P.lsa);
            if (b_dev) { P.b = b[i].data[p]; P.lsb = b[i].linesize[p]; } else call.stage(b[i], p, g, &P.b, &P.lsb);
            P.rowbytes = (uint32_t)g.rowbytes;
            P.rows = (uint32_t)g.rows;
            P.slot = (uint32_t)i;
            P.comp0 = L.pd->planar ? (uint32_t)p : 0;
            P.aligned = meas_aligned(P.a, P.lsa, P.b, P.lsb);
            most = std::max(most, work(i, p));
        }
    }
    r = call.run(nt, [&](hipStream_t st, const void *d_tab, void *d_sums) { return m.launch(st, (const CmpPlane *)d_tab, nt, most, (Sums *)d_sums); });
    if (r < 0) return r;
    for (int i = 0; i < n; i++)
        if (!(skip && skip[i])) m.result(i, a[i].width, a[i].height, ((const Sums *)call.sums.data())[i]);
    return 0;
}


/* c1 is 0 below 4 bits, and an all-zero window would then be 0 / 0 */
#define SSIM_MIN_BITS 4

/* what both pair calls refuse, in the order they refuse it: arguments, the layout and bits, then the frames */
static int pair_check(const htj2k_frame *a, const htj2k_frame *b, const void *out, int n, int bits, int min_bits, CmpLayout *L)
{
    if (!a || !b || !out || n < 1) return HTJ2K_ERR_EINVAL;
    const int r = cmp_layout(a[0].pix_fmt, bits, L);
    if (r < 0) return r;
    if (bits < min_bits) return HTJ2K_ERR_EINVAL;
    for (int i = 0; i < n; i++)
        if (!cmp_frame_ok(*L, a[i], a[0].pix_fmt) || !cmp_frame_ok(*L, b[i], a[0].pix_fmt) || a[i].width != b[i].width ||
            a[i].height != b[i].height)
            return HTJ2K_ERR_EINVAL;
    return 0;
}

static int ssim_strip(const htj2k_ctx *c) { return c->ssim_rows ? c->ssim_rows : SSIM_ROWS_DEFAULT; }

extern "C" int htj2k_compare_frames(htj2k_ctx *c, const htj2k_frame *a, int a_on_device, const htj2k_frame *b, int b_on_device,
                                    int n, int bits, htj2k_frame_diff *out)
{
    CmpLayout L;
    const int r = pair_check(a, b, out, n, bits, 1, &L);
    if (r < 0) return r;
    if (!c) return HTJ2K_ERR_ENOSYS;
    return pair_run(c, L, a, a_on_device, b, b_on_device, n, nullptr, DiffMetric{ L, bits, out });
}

extern "C" int htj2k_compare_frames_ssim(htj2k_ctx *c, const htj2k_frame *a, int a_on_device, const htj2k_frame *b, int b_on_device,
                                         int n, int bits, htj2k_frame_ssim *out)
{
    CmpLayout L;
    const int r = pair_check(a, b, out, n, bits, SSIM_MIN_BITS, &L);
    if (r < 0) return r;
    if (!c) return HTJ2K_ERR_ENOSYS;
    return pair_run(c, L, a, a_on_device, b, b_on_device, n, nullptr, SsimMetric{ L, ssim_strip(c), out });
}

extern "C" int htj2k_compare_ms(htj2k_ctx *c, float *ms)
{
    if (!c || !ms) return HTJ2K_ERR_EINVAL;
    *ms = c->cmp_ms;
    return 0;
}

/* htj2k_job_compare (out) or htj2k_job_compare_ssim (sout) */
static int job_compare(htj2k_ctx *c, htj2k_job *j, const htj2k_frame *ref, int ref_on_device, int bits, htj2k_frame_diff *out,
                       htj2k_frame_ssim *sout)
{
    if (!j || !ref || (!out && !sout) || j->nframes < 1) return HTJ2K_ERR_EINVAL;
    const int n = j->nframes;
    int first = -1;
    for (int f = 0; f < n && first < 0; f++)
        if (j->frames[f].plan) first = f;
    if (first < 0) return HTJ2K_ERR_EINVAL;
    const htj2k_info &I0 = j->frames[first].plan->info;
    if (bits == 0) bits = I0.bits_per_raw_sample;
    CmpLayout L;
    int r = cmp_layout(I0.pix_fmt, bits, &L);
    if (r < 0) return r;
    if (sout && bits < SSIM_MIN_BITS) return HTJ2K_ERR_EINVAL;
    std::vector<htj2k_frame> dev((size_t)n);
    std::vector<uint8_t> skip((size_t)n, 0);
    for (int f = 0; f < n; f++) {
        const FrameSlot &F = j->frames[f];
        if (!F.plan) { skip[f] = 1; continue; }           /* no frame there to compare */
        const htj2k_info &I = F.plan->info;
        if (I.pix_fmt != I0.pix_fmt || !cmp_frame_ok(L, ref[f], I0.pix_fmt) || ref[f].width != I.width || ref[f].height != I.height)
            return HTJ2K_ERR_EINVAL;
        job_frame_view(F, &dev[f]);
    }
    if (!j->run.frames_ok) return HTJ2K_ERR_EINVAL;            /* the last run did not write the frames (htj2k_job_run_stages) */
    if (!c) return HTJ2K_ERR_ENOSYS;
    if ((r = job_settle(c, j)) < 0) return r;              /* waits for the job's stream; the planes are final behind it */
    for (int f = 0; f < n; f++)
        if (skip[f]) {
            if (sout) {
                ssim_result(L, 0, 0, nullptr, &sout[f]);      /* no windows: nwin 0 and NaNs */
            } else {
                memset(&out[f], 0, sizeof out[f]);
                out[f].psnr = (double)NAN;
            }
        } else if (!cmp_frame_ok(L, dev[f], I0.pix_fmt)) {
            return HTJ2K_ERR_BUG;
        }
    if (sout) return pair_run(c, L, dev.data(), 1, ref, ref_on_device, n, skip.data(), SsimMetric{ L, ssim_strip(c), sout });
    return pair_run(c, L, dev.data(), 1, ref, ref_on_device, n, skip.data(), DiffMetric{ L, bits, out });
}

extern "C" int htj2k_job_compare(htj2k_ctx *c, htj2k_job *j, const htj2k_frame *ref, int ref_on_device, int bits, htj2k_frame_diff *out)
{
    if (!out) return HTJ2K_ERR_EINVAL;
    return job_compare(c, j, ref, ref_on_device, bits, out, nullptr);
}

extern "C" int htj2k_job_compare_ssim(htj2k_ctx *c, htj2k_job *j, const htj2k_frame *ref, int ref_on_device, int bits,
                                      htj2k_frame_ssim *out)
{
    if (!out) return HTJ2K_ERR_EINVAL;
    return job_compare(c, j, ref, ref_on_device, bits, nullptr, out);
}

/* ------------------------------------------------------------------ frame checksums (k_frame_adler, cmp_kernels.hpp)
 * What one line of `-f framecrc` prints: Adler-32 seeded with 0 over the frame's bytes as av_image_copy_to_buffer(align 1)
 * packs them.  The kernel sums every plane on its own; the planes are combined here. */
struct HashLayout {                    /* the planes of one frame as they are hashed */
    int nplanes;
    PlaneGeo plane[4];
};

#define HASH_MAX_PLANE (1ull << 38)     /* bytes; the decoder's largest plane, 32768^2 samples of 8 bytes, has 2^33 */

/* false: a pix_fmt outside the enum, a size below 1, a row beyond 2^31 bytes or a plane of HASH_MAX_PLANE */
static bool hash_layout(int pix_fmt, int w, int h, HashLayout *H)
{
    const J2kPixDesc *pd = j2k_pix_desc(pix_fmt);
    if (!pd || w < 1 || h < 1 || (int64_t)w * pd->nb_components * pd->bytes > INT32_MAX) return false;
    memset(H, 0, sizeof *H);
    H->nplanes = pd->nplanes;
    for (int p = 0; p < pd->nplanes; p++) {
        if (pd->pal && p == 1) { H->plane[p] = { 1024, 1 }; continue; }    /* the palette as it is stored */
        H->plane[p] = pix_plane(pd, w, h, p);
        if ((uint64_t)H->plane[p].rowbytes * (uint64_t)H->plane[p].rows >= HASH_MAX_PLANE) return false;
    }
    return true;
}

static bool hash_frame_ok(const htj2k_frame &f, HashLayout *H)
{
    if (!hash_layout(f.pix_fmt, f.width, f.height, H)) return false;
    for (int p = 0; p < H->nplanes; p++)
        if (!f.data[p] || f.linesize[p] < 0 || (size_t)f.linesize[p] < H->plane[p].rowbytes) return false;
    return true;
}

/* the planes' sums into the frame's figures: A = sum A_p, B = sum (B_p + A_p * bytes after plane p), mod 65521 */
static void hash_result(const HashLayout &H, const HashSums &S, htj2k_frame_hash *o)
{
    memset(o, 0, sizeof *o);
    uint64_t after = 0, A = 0, B = 0;
    for (int p = H.nplanes - 1; p >= 0; p--) {
        const uint64_t ap = S.a[p] % ADLER_MOD, bp = S.b[p] % ADLER_MOD;
        o->plane_adler32[p] = (uint32_t)(bp << 16 | ap);
        A += ap;
        B += bp + ap * (after % ADLER_MOD);
        after += (uint64_t)H.plane[p].rowbytes * (uint64_t)H.plane[p].rows;
    }
    o->adler32 = (uint32_t)((B % ADLER_MOD) << 16 | (A % ADLER_MOD));
    o->nbytes = after;
}

/* the checked call: frames i with skip[i] set (skip may be NULL) take no part and keep what `out` holds for them */
static int hash_run(htj2k_ctx *c, const htj2k_frame *f, const HashLayout *H, int on_dev, int n, const uint8_t *skip, htj2k_frame_hash *out)
{
    MeasCall call(c);
    size_t np = 0, staged = 0, nt = 0, most = 1;
    for (int i = 0; i < n; i++) {
        if (skip && skip[i]) continue;
        np += (size_t)H[i].nplanes;
        for (int p = 0; p < H[i].nplanes && !on_dev; p++)
            staged += meas_pitch(H[i].plane[p].rowbytes) * (size_t)H[i].plane[p].rows;
    }
    int r = call.reserve((size_t)n, sizeof(HashSums), np, sizeof(HashPlane), staged);
    if (r < 0) return r;
    HashPlane *tab = (HashPlane *)call.h;
    for (int i = 0; i < n; i++) {
        if (skip && skip[i]) continue;
        for (int p = 0; p < H[i].nplanes; p++) {
            const PlaneGeo g = H[i].plane[p];
            /* a group adds less than 2^29 to the kernel's 64-bit B accumulator: exact below 2^38 bytes a plane */
            assert((uint64_t)g.rowbytes * (uint64_t)g.rows < HASH_MAX_PLANE);
            HashPlane &P = tab[nt++];
            memset(&P, 0, sizeof P);
            if (on_dev) { P.p = f[i].data[p]; P.ls = f[i].linesize[p]; } else call.stage(f[i], p, g, &P.p, &P.ls);
            P.rowbytes = (uint32_t)g.rowbytes;
            P.rows = (uint32_t)g.rows;
            P.slot = (uint32_t)i;
            P.plane = (uint32_t)p;
            P.aligned = meas_aligned(P.p, P.ls);
            most = std::max(most, ((g.rowbytes + 15) / 16) * (size_t)g.rows);
        }
    }
    /* 16-byte groups whatever the layout, two a lane and step */
    r = call.run(nt, [&](hipStream_t st, const void *d_tab, void *d_sums) {
        meas_launch(k_frame_adler, st, (const HashPlane *)d_tab, nt, most, 2 * CMP_THREADS, (HashSums *)d_sums);
        return 0;
    });
    if (r < 0) return r;
    for (int i = 0; i < n; i++)
        if (!(skip && skip[i])) hash_result(H[i], ((const HashSums *)call.sums.data())[i], &out[i]);
    return 0;
}

extern "C" int htj2k_hash_frames(htj2k_ctx *c, const htj2k_frame *f, int on_device, int n, htj2k_frame_hash *out)
{
    if (!f || !out || n < 1) return HTJ2K_ERR_EINVAL;
    std::vector<HashLayout> H((size_t)n);
    for (int i = 0; i < n; i++)
        if (!hash_frame_ok(f[i], &H[(size_t)i])) return HTJ2K_ERR_EINVAL;
    if (!c) return HTJ2K_ERR_ENOSYS;
    return hash_run(c, f, H.data(), on_device, n, nullptr, out);
}

extern "C" int htj2k_job_hash(htj2k_ctx *c, htj2k_job *j, htj2k_frame_hash *out)
{
    if (!j || !out || j->nframes < 1) return HTJ2K_ERR_EINVAL;
    if (!j->uploaded || !j->run.frames_ok) return HTJ2K_ERR_EINVAL;     /* no run yet, or one that did not write the frames */
    if (!c) return HTJ2K_ERR_ENOSYS;
    const int n = j->nframes;
    int r = job_settle(c, j);                              /* waits for the job's stream; the planes are final behind it */
    if (r < 0) return r;
    std::vector<htj2k_frame> dev((size_t)n);
    std::vector<HashLayout> H((size_t)n);
    std::vector<uint8_t> skip((size_t)n, 0);
    for (int f = 0; f < n; f++) {
        const FrameSlot &F = j->frames[f];
        memset(&out[f], 0, sizeof out[f]);
        if (!F.plan) { skip[f] = 1; continue; }           /* no frame there: nbytes 0 and zeros */
        job_frame_view(F, &dev[f]);
        if (!hash_frame_ok(dev[f], &H[f])) return HTJ2K_ERR_BUG;
    }
    return hash_run(c, dev.data(), H.data(), 1, n, skip.data(), out);
}

/* ------------------------------------------------------------------ frames as tensors (tensor_kernels.hpp)
 * Frames of one layout as normalised float images, NCHW or NHWC, written to the caller's device memory.  The call is a
 * MeasCall without results: its table holds the planes of the fast route (k_frame_tensor), then those of the general one
 * (k_frame_tensor_any); the route is chosen per plane (tensor_fast). */
struct TensorCall {                    /* a checked call: what its frames share */
    CmpLayout L;
    int dtype, nhwc, ow, oh, ncomp;
    size_t esize, elems;               /* bytes of an element, elements of an image */
    float scale[4], bias[4];
    int nout;                          /* K: channels of an image; ncomp without a mix */
    const htj2k_tensor_mix *mix;       /* checked (tensor_spec_check), or NULL; scale and bias are then not read */
    const htj2k_tensor_mix_in *mix_in; /* tensors as frames: the same for the way in; nout is then its K */
    const htj2k_tensor_curves *curves; /* checked (curves_check), or NULL; only beside a mix */
    const htj2k_tensor_curves_in *curves_in;   /* the way in: checked (curves_in_check), or NULL; only beside a mix_in */
};

/* what a resized call has beside a plain one: its windows (4 n: ox, oy, ww, wh; NULL: each frame whole) and its filter */
struct ResizeArgs { const int32_t *windows; int filter; htj2k_ctx *log; /* may be NULL */ };

/* frame i's window of a resized call: ox, oy, ww, wh */
static void resize_window(const ResizeArgs &rs, const htj2k_frame *f, int i, int32_t w[4])
{
    if (rs.windows) memcpy(w, rs.windows + 4 * (size_t)i, 4 * sizeof(int32_t));
    else { w[0] = w[1] = 0; w[2] = f[i].width; w[3] = f[i].height; }
}

/* refusals 3 to 7 of the header's list, in its order; 0 x 0 leaves ow and oh 0 for the frames to fill.  A resized call
 * (rs) has its filter checked behind dtype and layout, and has no 0 x 0 */
static int curves_check(const htj2k_tensor_curves *q, bool mix, int C, int K);
static int curves_in_check(const htj2k_tensor_curves_in *q, bool mix, int C, int K);

static int tensor_spec_check(int pix_fmt, int bits, const htj2k_tensor_spec *s, TensorCall *T, const ResizeArgs *rs = nullptr,
                             const htj2k_tensor_mix *mix = nullptr, const htj2k_tensor_mix_in *mix_in = nullptr,
                             const htj2k_tensor_curves *curves = nullptr, const htj2k_tensor_curves_in *curves_in = nullptr)
{
    memset(T, 0, sizeof *T);
    const int r = cmp_layout(pix_fmt, bits, &T->L);      /* a pix_fmt outside the enum, PAL8, then bits */
    if (r < 0) return r;
    if (s->dtype < HTJ2K_TENSOR_F32 || s->dtype > HTJ2K_TENSOR_BF16 || s->layout < HTJ2K_TENSOR_NCHW || s->layout > HTJ2K_TENSOR_NHWC)
        return HTJ2K_ERR_EINVAL;
    if (rs && (rs->filter < HTJ2K_RESIZE_NEAREST || rs->filter > HTJ2K_RESIZE_TRIANGLE)) return HTJ2K_ERR_EINVAL;
    T->ncomp = T->nout = T->L.pd->nb_components;
    if (mix) {                                             /* in the place of scale and bias: K, then the entries that are read */
        if (mix->nout < 1 || mix->nout > 4) return HTJ2K_ERR_EINVAL;
        for (int k = 0; k < mix->nout; k++) {
            for (int c = 0; c < T->ncomp; c++)
                if (!std::isfinite(mix->m[k][c])) return HTJ2K_ERR_EINVAL;
            if (!std::isfinite(mix->b[k])) return HTJ2K_ERR_EINVAL;
        }
        T->nout = mix->nout;
        T->mix = mix;
    }
    if (curves) {                                          /* where the mix has been checked: the curves, against C and K */
        const int rc = curves_check(curves, mix != nullptr, T->ncomp, T->nout);
        if (rc < 0) return rc;
        T->curves = curves;
    }
    if (mix_in) {                                          /* the way in: K, the chroma rule, then the entries that are read */
        if (mix_in->nin < 1 || mix_in->nin > 4) return HTJ2K_ERR_EINVAL;
        if (mix_in->chroma < HTJ2K_CHROMA_COSITED || mix_in->chroma > HTJ2K_CHROMA_BOX) return HTJ2K_ERR_EINVAL;
        for (int c = 0; c < T->ncomp; c++) {
            for (int k = 0; k < mix_in->nin; k++)
                if (!std::isfinite(mix_in->m[c][k])) return HTJ2K_ERR_EINVAL;
            if (!std::isfinite(mix_in->b[c])) return HTJ2K_ERR_EINVAL;
        }
        T->nout = mix_in->nin;
        T->mix_in = mix_in;
    }
    if (curves_in) {                                       /* where the mix has been checked: the curves, against C and K */
        const int rc = curves_in_check(curves_in, mix_in != nullptr, T->ncomp, T->nout);
        if (rc < 0) return rc;
        T->curves_in = curves_in;
    }
    for (int k = 0; k < T->ncomp && !mix && !mix_in; k++) {
        if (!std::isfinite(s->scale[k]) || !std::isfinite(s->bias[k])) return HTJ2K_ERR_EINVAL;
        T->scale[k] = s->scale[k];
        T->bias[k] = s->bias[k];
    }
    if (!((s->out_w == 0 && s->out_h == 0 && !rs) || (s->out_w >= 1 && s->out_h >= 1))) return HTJ2K_ERR_EINVAL;
    T->dtype = s->dtype;
    T->nhwc = s->layout == HTJ2K_TENSOR_NHWC;
    T->ow = s->out_w;
    T->oh = s->out_h;
    T->esize = s->dtype == HTJ2K_TENSOR_F32 ? 4 : 2;
    return 0;
}

/* the window checks of a resized call, in the header's order: the three refusals of a window, over all frames each, then
 * what is out of scope.  htj2k_resize_frames has one more between them: an origin with a bit of grid_x or grid_y set is off
 * the layout's chroma grid */
static int resize_windows_check(const TensorCall &T, const htj2k_frame *f, int n, const uint8_t *skip, const ResizeArgs &rs,
                                int grid_x = 0, int grid_y = 0)
{
    auto there = [&](int i) { return !(skip && skip[i]); };
    int32_t w[4];
    for (int i = 0; i < n; i++) {
        if (!there(i) && !rs.windows) continue;            /* a frame that is not there has no size to be whole in */
        resize_window(rs, f, i, w);
        if (w[2] < 1 || w[3] < 1) return HTJ2K_ERR_EINVAL;
    }
    for (int i = 0; i < n && rs.windows; i++)
        if (rs.windows[4 * i] < 0 || rs.windows[4 * i + 1] < 0) return HTJ2K_ERR_EINVAL;
    for (int i = 0; i < n; i++) {
        if (!there(i)) continue;
        resize_window(rs, f, i, w);
        if ((int64_t)w[0] + w[2] > f[i].width || (int64_t)w[1] + w[3] > f[i].height) return HTJ2K_ERR_EINVAL;
    }
    for (int i = 0; i < n && (grid_x || grid_y); i++) {
        if (!there(i)) continue;
        resize_window(rs, f, i, w);
        if ((w[0] & grid_x) || (w[1] & grid_y)) return HTJ2K_ERR_EINVAL;
    }
    if (T.ow > RS_MAX_SIZE || T.oh > RS_MAX_SIZE) {
        clog(rs.log, LOG_ERROR, "resize: an output of %d x %d; the limit is %d either way\n", T.ow, T.oh, (int)RS_MAX_SIZE);
        return HTJ2K_ERR_PATCHWELCOME;
    }
    for (int i = 0; i < n; i++) {
        if (!there(i)) continue;
        resize_window(rs, f, i, w);
        if (w[2] > RS_MAX_SIZE || w[3] > RS_MAX_SIZE) {
            clog(rs.log, LOG_ERROR, "resize: a window of %d x %d; the limit is %d either way\n", w[2], w[3], (int)RS_MAX_SIZE);
            return HTJ2K_ERR_PATCHWELCOME;
        }
        if (rs.filter == HTJ2K_RESIZE_TRIANGLE && (w[2] > (int64_t)RS_MAX_REDUCTION * T.ow || w[3] > (int64_t)RS_MAX_REDUCTION * T.oh)) {
            clog(rs.log, LOG_ERROR, "resize: %d x %d to %d x %d; the triangle filter reduces by %d at the most\n", w[2], w[3], T.ow, T.oh,
                 (int)RS_MAX_REDUCTION);
            return HTJ2K_ERR_PATCHWELCOME;
        }
    }
    return 0;
}

/* refusals 8 to 15: the frames (skip[i] set: frame i is not there), the windows, the destination.  A resized call (rs)
 * has its own windows in place of the origins */
static int tensor_frames_check(TensorCall *T, const htj2k_frame *f, int n, const uint8_t *skip, int pix_fmt, const int32_t *origins,
                               const void *dst, size_t dst_bytes, const ResizeArgs *rs = nullptr)
{
    const CmpLayout &L = T->L;
    auto there = [&](int i) { return !(skip && skip[i]); };
    for (int i = 0; i < n; i++)
        if (there(i) && f[i].pix_fmt != pix_fmt) return HTJ2K_ERR_EINVAL;
    int first = -1;
    for (int i = 0; i < n; i++) {
        if (!there(i)) continue;
        if (f[i].width < 1 || f[i].height < 1 || (int64_t)f[i].width * L.step * L.bytes > INT32_MAX) return HTJ2K_ERR_EINVAL;
        if (first < 0) first = i;
        if (!T->ow && (f[i].width != f[first].width || f[i].height != f[first].height)) return HTJ2K_ERR_EINVAL;
    }
    if (first < 0) return HTJ2K_ERR_EINVAL;
    if (!T->ow) { T->ow = f[first].width; T->oh = f[first].height; }
    for (int i = 0; i < n; i++)
        for (int p = 0; p < L.nplanes && there(i); p++)
            if (!f[i].data[p]) return HTJ2K_ERR_EINVAL;
    for (int i = 0; i < n; i++)
        for (int p = 0; p < L.nplanes && there(i); p++)
            if (f[i].linesize[p] < 0 || (size_t)f[i].linesize[p] < pix_plane(L.pd, f[i].width, f[i].height, p).rowbytes) return HTJ2K_ERR_EINVAL;
    if (rs) {
        const int r = resize_windows_check(*T, f, n, skip, *rs);
        if (r < 0) return r;
    }
    for (int i = 0; i < n && origins && !rs; i++)
        if (origins[2 * i] < 0 || origins[2 * i + 1] < 0) return HTJ2K_ERR_EINVAL;
    for (int i = 0; i < n && !rs; i++) {
        const int64_t ox = origins ? origins[2 * i] : 0, oy = origins ? origins[2 * i + 1] : 0;
        if (there(i) && (ox + T->ow > f[i].width || oy + T->oh > f[i].height)) return HTJ2K_ERR_EINVAL;
    }
    T->elems = (size_t)T->nout * (size_t)T->ow * (size_t)T->oh;
    if (dst_bytes / T->esize / T->elems < (size_t)n) return HTJ2K_ERR_EINVAL;
    if ((uintptr_t)dst % T->esize) return HTJ2K_ERR_EINVAL;
    return 0;
}

/* Is plane p's window on the fast route?  No chroma shift; the window's first byte on a group boundary of its row; base
 * and linesize multiples of 16, so that every full group is read with 16-byte loads; and, for NHWC, all channels of the
 * image interleaved in this plane (or one channel: then NHWC is NCHW). */
static bool tensor_fast(const TensorCall &T, int p, const uint8_t *base, int64_t ls, int ox)
{
    const J2kPixDesc *pd = T.L.pd;
    const int k = pd->planar ? p : 0;
    if (((k == 1 || k == 2) && (pd->log2_chroma_w || pd->log2_chroma_h)) || (T.nhwc && pd->planar && T.ncomp > 1)) return false;
    const size_t group = T.L.step == 3 ? 48 : 16;
    return ((size_t)ox * T.L.step * T.L.bytes) % group == 0 && meas_aligned(base, ls);
}

/* The store-alignment rule, beside meas_aligned: a plane's runs go out in 16-byte stores when every full run of the
 * plane starts on a multiple of 16 -- the image's first byte, the bytes of a destination row and the bytes of a run are
 * multiples of 16, and for NCHW the bytes of a channel as well.  A run is a group's pixels of one component (NCHW) or all
 * of a group's samples (NHWC).  The source's origin has no part in it: runs are counted from the window's corner. */
static uint32_t tensor_wide(const TensorCall &T, const void *dst, uint64_t dst_img)
{
    const size_t group = T.L.step == 3 ? 48 : 16, ns = group / T.L.bytes, np = ns / T.L.step;
    const bool nhwc = T.nhwc && T.ncomp > 1;
    const uint64_t row = (uint64_t)T.ow * T.esize * (nhwc ? T.ncomp : 1), run = (nhwc ? ns : np) * T.esize;
    const uint64_t chan = nhwc ? 0 : (uint64_t)T.ow * T.oh * T.esize;
    return (((uintptr_t)dst + dst_img * T.esize) % 16 == 0 && row % 16 == 0 && run % 16 == 0 && chan % 16 == 0) ? 1u : 0u;
}

template <int DT, class B, class S>
static void tensor_launch_fast(B, S, bool nhwc, hipStream_t st, const TensorPlane *tab, size_t nt, size_t most, uint8_t *dst, const TensorFmt &F)
{
    if (nhwc) meas_launch(k_frame_tensor<B::value, S::value, DT, 1>, st, tab, nt, most, CMP_THREADS, dst, F);
    else      meas_launch(k_frame_tensor<B::value, S::value, DT, 0>, st, tab, nt, most, CMP_THREADS, dst, F);
}

/* what the kernels of a checked call share */
static TensorFmt tensor_fmt(const TensorCall &T)
{
    TensorFmt F;
    memset(&F, 0, sizeof F);
    F.shift = T.L.shift; F.mask = T.L.mask;
    F.out_w = (uint32_t)T.ow; F.out_h = (uint32_t)T.oh;
    F.ncomp = (uint32_t)T.ncomp; F.bytes = (uint32_t)T.L.bytes;
    F.nhwc = T.nhwc && T.ncomp > 1;
    for (int k = 0; k < 4; k++) { F.scale[k] = T.scale[k]; F.bias[k] = T.bias[k]; }
    return F;
}

/* the bytes a call's host operands take in the staging image, and the planes of the frames that are there */
static size_t tensor_staged_bytes(const CmpLayout &L, const htj2k_frame *f, int on_dev, int n, const uint8_t *skip, size_t *nplanes)
{
    size_t staged = 0;
    *nplanes = 0;
    for (int i = 0; i < n; i++) {
        if (skip && skip[i]) continue;
        *nplanes += (size_t)L.nplanes;
        for (int p = 0; p < L.nplanes && !on_dev; p++) {
            const PlaneGeo g = pix_plane(L.pd, f[i].width, f[i].height, p);
            staged += meas_pitch(g.rowbytes) * (size_t)g.rows;
        }
    }
    return staged;
}

/* the checked call: n images at dst; frames i with skip[i] set (skip may be NULL) get an image of zero bits */
static int tensor_run(htj2k_ctx *c, const TensorCall &T, const htj2k_frame *f, int on_dev, int n, const uint8_t *skip,
                      const int32_t *origins, void *dst)
{
    const CmpLayout &L = T.L;
    MeasCall call(c);
    c->tensor_route = 0;
    auto there = [&](int i) { return !(skip && skip[i]); };
    size_t np = 0;
    const size_t staged = tensor_staged_bytes(L, f, on_dev, n, skip, &np);
    int r = call.reserve(0, 0, np, sizeof(TensorPlane), staged);
    if (r < 0) return r;
    /* both routes' entries, then the table: the fast route's in front */
    std::vector<TensorPlane> fast, any;
    size_t most_fast = 1, most_any = 1;
    const size_t group = L.step == 3 ? 48 : 16;
    /* lanes that share a group: TensorShape::SHARE */
    const size_t run = (T.nhwc && T.ncomp > 1) ? group / L.bytes : group / L.bytes / L.step, per16 = 16 / T.esize;
    const size_t share = (run % per16 == 0 && run / per16 >= 2) ? run / per16 : 1;
    for (int i = 0; i < n; i++) {
        if (!there(i)) continue;
        const int ox = origins ? origins[2 * i] : 0, oy = origins ? origins[2 * i + 1] : 0;
        for (int p = 0; p < L.nplanes; p++) {
            TensorPlane P;
            memset(&P, 0, sizeof P);
            if (on_dev) { P.src = f[i].data[p]; P.ls = f[i].linesize[p]; }
            else call.stage(f[i], p, pix_plane(L.pd, f[i].width, f[i].height, p), &P.src, &P.ls);
            const int k = L.pd->planar ? p : 0;
            P.dst_img = (uint64_t)i * T.elems;
            P.comp0 = (uint32_t)k;
            P.step = (uint32_t)L.step;
            P.sw = (k == 1 || k == 2) ? L.pd->log2_chroma_w : 0;
            P.sh = (k == 1 || k == 2) ? L.pd->log2_chroma_h : 0;
            if (!c->tensor_path && tensor_fast(T, p, P.src, P.ls, ox)) {
                P.src += (int64_t)oy * P.ls + (int64_t)ox * L.step * L.bytes;
                P.wide = tensor_wide(T, dst, P.dst_img);
                fast.push_back(P);
                most_fast = std::max(most_fast, (((size_t)T.ow * L.step * L.bytes + group - 1) / group) * (size_t)T.oh * share);
            } else {
                P.ox = (uint32_t)ox;
                P.oy = (uint32_t)oy;
                any.push_back(P);
                most_any = std::max(most_any, (size_t)L.step * T.ow * T.oh);
            }
        }
    }
    TensorPlane *tab = (TensorPlane *)call.h;
    if (!fast.empty()) memcpy(tab, fast.data(), fast.size() * sizeof(TensorPlane));
    if (!any.empty()) memcpy(tab + fast.size(), any.data(), any.size() * sizeof(TensorPlane));
    const TensorFmt F = tensor_fmt(T);
    int route = 0;
    const size_t nt = fast.size() + any.size();
    r = call.run(nt, [&](hipStream_t st, const void *d_tab, void *) {
        uint8_t *out = (uint8_t *)dst;
        for (int i = 0; i < n; i++)
            if (!there(i)) HIP_TRY(c, hipMemsetAsync(out + (size_t)i * T.elems * T.esize, 0, T.elems * T.esize, st));
        const TensorPlane *dt = (const TensorPlane *)d_tab;
        if (!fast.empty()) {
            const int rr = cmp_dispatch(L, [&](auto B, auto S) {
                switch (T.dtype) {
                case HTJ2K_TENSOR_F32:  tensor_launch_fast<TENSOR_F32>(B, S, F.nhwc != 0, st, dt, fast.size(), most_fast, out, F); break;
                case HTJ2K_TENSOR_F16:  tensor_launch_fast<TENSOR_F16>(B, S, F.nhwc != 0, st, dt, fast.size(), most_fast, out, F); break;
                default:                tensor_launch_fast<TENSOR_BF16>(B, S, F.nhwc != 0, st, dt, fast.size(), most_fast, out, F); break;
                }
            });
            if (rr < 0) return rr;
            route |= 1;
        }
        if (!any.empty()) {
            const TensorPlane *da = dt + fast.size();
            switch (T.dtype) {
            case HTJ2K_TENSOR_F32:  meas_launch(k_frame_tensor_any<TENSOR_F32>, st, da, any.size(), most_any, CMP_THREADS, out, F); break;
            case HTJ2K_TENSOR_F16:  meas_launch(k_frame_tensor_any<TENSOR_F16>, st, da, any.size(), most_any, CMP_THREADS, out, F); break;
            default:                meas_launch(k_frame_tensor_any<TENSOR_BF16>, st, da, any.size(), most_any, CMP_THREADS, out, F); break;
            }
            route |= 2;
        }
        return 0;
    });
    if (r < 0) return r;
    c->tensor_route = route;
    return 0;
}

/* ---- a colour matrix in the tensor calls (mix_kernels.hpp): K channels from the layout's C components, one linear map
 * per pixel inside the launch that reads the samples.  The table holds a frame per entry, the fast route's in front. */
struct MixCut {                        /* how the mix kernels see a layout */
    int planar;                        /* component c is plane c; else all components interleaved in plane 0 */
    int sw, sh;                        /* chroma shifts of planes 1 and 2 */
    int np;                            /* pixels of a fast-route group (MixShape::NP); 0: the layout has no fast route */
};

static MixCut mix_cut(const TensorCall &T)
{
    const J2kPixDesc *pd = T.L.pd;
    MixCut M;
    M.planar = pd->planar && T.ncomp > 1;
    M.sw = M.planar && T.ncomp >= 3 ? pd->log2_chroma_w : 0;
    M.sh = M.planar && T.ncomp >= 3 ? pd->log2_chroma_h : 0;
    M.np = M.planar ? (M.sw <= 1 ? (16 << M.sw) / T.L.bytes : 0) : (T.L.step == 3 ? 48 : 16) / (T.L.step * T.L.bytes);
    return M;
}

/* Is the frame on the fast route?  A horizontal chroma shift of 0 or 1; the window's first pixel on a group boundary;
 * every plane's base and linesize a multiple of 16.  Any vertical shift, any oy, both layouts, every K. */
static bool mix_fast(const TensorCall &T, const MixCut &M, const MixFrame &P, int ox)
{
    if (!M.np || ox % M.np) return false;
    for (int p = 0; p < T.L.nplanes; p++)
        if (!meas_aligned(P.src[p], P.ls[p])) return false;
    return true;
}

/* tensor_wide for a frame of the mix kernel: a lane's run is PART pixels (NCHW) or PART pixels times K (NHWC) */
static uint32_t mix_wide(const TensorCall &T, const MixCut &M, const void *dst, uint64_t dst_img)
{
    const size_t per16 = 16 / T.esize, np = (size_t)M.np;
    const size_t share = (np % per16 == 0 && np / per16 >= 2) ? np / per16 : 1, part = np / share;
    const bool nhwc = T.nhwc && T.nout > 1;
    const uint64_t row = (uint64_t)T.ow * T.esize * (nhwc ? T.nout : 1), run = part * (nhwc ? T.nout : 1) * T.esize;
    const uint64_t chan = nhwc ? 0 : (uint64_t)T.ow * T.oh * T.esize;
    return (((uintptr_t)dst + dst_img * T.esize) % 16 == 0 && row % 16 == 0 && run % 16 == 0 && chan % 16 == 0) ? 1u : 0u;
}

static MixFmt mix_fmt(const TensorCall &T, const MixCut &M)
{
    MixFmt F;
    memset(&F, 0, sizeof F);
    F.shift = T.L.shift; F.mask = T.L.mask;
    F.out_w = (uint32_t)T.ow; F.out_h = (uint32_t)T.oh;
    F.ncomp = (uint32_t)T.ncomp; F.nout = (uint32_t)T.nout;
    F.bytes = (uint32_t)T.L.bytes; F.step = (uint32_t)T.L.step;
    F.planar = (uint32_t)M.planar; F.sw = (uint32_t)M.sw; F.sh = (uint32_t)M.sh;
    F.nhwc = T.nhwc && T.nout > 1;
    for (int k = 0; k < T.nout; k++) {                       /* what is not read stays zero */
        for (int c = 0; c < T.ncomp; c++) F.m[k][c] = T.mix->m[k][c];
        F.b[k] = T.mix->b[k];
    }
    return F;
}

/* f(bytes per sample, interleaved components per plane, planes, horizontal chroma shift): k_frame_mix's cut */
template <class F> static int mix_dispatch(const TensorCall &T, const MixCut &M, F f)
{
    using std::integral_constant;
    typedef integral_constant<int, 0> I0; typedef integral_constant<int, 1> I1; typedef integral_constant<int, 2> I2;
    typedef integral_constant<int, 3> I3; typedef integral_constant<int, 4> I4;
    if (!M.planar) return cmp_dispatch(T.L, [&](auto B, auto S) { f(B, S, I1(), I0()); });
    switch (T.L.bytes * 100 + T.ncomp * 10 + M.sw) {
    case 130: f(I1(), I1(), I3(), I0()); break;
    case 131: f(I1(), I1(), I3(), I1()); break;
    case 140: f(I1(), I1(), I4(), I0()); break;
    case 141: f(I1(), I1(), I4(), I1()); break;
    case 230: f(I2(), I1(), I3(), I0()); break;
    case 231: f(I2(), I1(), I3(), I1()); break;
    case 240: f(I2(), I1(), I4(), I0()); break;
    case 241: f(I2(), I1(), I4(), I1()); break;
    default: return HTJ2K_ERR_BUG;
    }
    return 0;
}

template <int DT, class B, class S, class N, class W>
static void mix_launch_fast(B, S, N, W, bool nhwc, hipStream_t st, const MixFrame *tab, size_t nt, size_t most, uint8_t *dst, const MixFmt &F)
{
    if (nhwc) meas_launch(k_frame_mix<B::value, S::value, N::value, W::value, DT, 1>, st, tab, nt, most, CMP_THREADS, dst, F);
    else      meas_launch(k_frame_mix<B::value, S::value, N::value, W::value, DT, 0>, st, tab, nt, most, CMP_THREADS, dst, F);
}

/* ---- transfer curves around the mix (curve_kernels.hpp): the same calls, tables and routes, with both curves' tables
 * uploaded behind the call's planes and staged into LDS by every workgroup. */
/* refusals 1 to 9 of the header's list, in its order; C and K are the checked mix's */
static int curves_check(const htj2k_tensor_curves *q, bool mix, int C, int K)
{
    const htj2k_tensor_curve *cv[2] = { &q->in, &q->out };
    if (!mix) return HTJ2K_ERR_EINVAL;
    if (q->in.n == 0 && q->out.n == 0) return HTJ2K_ERR_EINVAL;
    for (const htj2k_tensor_curve *v : cv)
        if (v->n != 0 && (v->n < 2 || v->n > HTJ2K_CURVE_MAX_KNOTS)) return HTJ2K_ERR_EINVAL;
    for (const htj2k_tensor_curve *v : cv)
        if (v->n && !v->t) return HTJ2K_ERR_EINVAL;
    for (const htj2k_tensor_curve *v : cv)
        if (v->n && !std::isfinite(v->x0)) return HTJ2K_ERR_EINVAL;
    for (const htj2k_tensor_curve *v : cv)
        if (v->n && !(std::isfinite(v->inv_dx) && v->inv_dx > 0.0f)) return HTJ2K_ERR_EINVAL;
    for (const htj2k_tensor_curve *v : cv)
        for (int j = 0; j < v->n; j++)
            if (!(fabsf(v->t[j]) <= 0x1p100f)) return HTJ2K_ERR_EINVAL;     /* a NaN fails the comparison as well */
    if ((q->in_mask >> C) || (q->out_mask >> K)) return HTJ2K_ERR_EINVAL;
    for (int k = 0; k < K; k++)
        if (!std::isfinite(q->gain[k]) || !std::isfinite(q->offset[k])) return HTJ2K_ERR_EINVAL;
    return 0;
}

/* the ten refusals of "tensors as frames, with curves", in the header's order; C and K are the checked mix's */
static int curves_in_check(const htj2k_tensor_curves_in *q, bool mix, int C, int K)
{
    const htj2k_tensor_curve_in *cv[2] = { &q->in, &q->out };
    if (!mix) return HTJ2K_ERR_EINVAL;
    if (q->in.n == 0 && q->out.n == 0) return HTJ2K_ERR_EINVAL;
    for (const htj2k_tensor_curve_in *v : cv)
        if (v->n != 0 && (v->n < 2 || v->n > HTJ2K_CURVE_MAX_KNOTS)) return HTJ2K_ERR_EINVAL;
    for (const htj2k_tensor_curve_in *v : cv)
        if (v->n && (v->root < 0 || v->root > HTJ2K_CURVE_MAX_ROOT)) return HTJ2K_ERR_EINVAL;
    for (const htj2k_tensor_curve_in *v : cv)
        if (v->n && !v->t) return HTJ2K_ERR_EINVAL;
    for (const htj2k_tensor_curve_in *v : cv)
        if (v->n && !std::isfinite(v->x0)) return HTJ2K_ERR_EINVAL;
    for (const htj2k_tensor_curve_in *v : cv)
        if (v->n && !(std::isfinite(v->inv_dx) && v->inv_dx > 0.0f)) return HTJ2K_ERR_EINVAL;
    for (const htj2k_tensor_curve_in *v : cv)
        for (int j = 0; j < v->n; j++)
            if (!(fabsf(v->t[j]) <= 0x1p100f)) return HTJ2K_ERR_EINVAL;     /* a NaN fails the comparison as well */
    if ((q->in_mask >> K) || (q->out_mask >> C)) return HTJ2K_ERR_EINVAL;
    for (int c = 0; c < C; c++)
        if (!std::isfinite(q->gain[c]) || !std::isfinite(q->offset[c])) return HTJ2K_ERR_EINVAL;
    return 0;
}

/* floats of a table in the upload and in LDS: its n knots and t[n] = t[n-1], padded to 16 bytes; 0 without a curve */
static size_t curve_floats(const htj2k_tensor_curve &v) { return v.n ? ((size_t)v.n + 1 + 3) & ~(size_t)3 : 0; }
static size_t curves_bytes(const htj2k_tensor_curves *q) { return q ? (curve_floats(q->in) + curve_floats(q->out)) * sizeof(float) : 0; }

/* the tables into the call's staging image (behind its planes), and what the kernels get */
static CurveFmt curves_fmt(const TensorCall &T, MeasCall *call)
{
    const htj2k_tensor_curves &q = *T.curves;
    CurveFmt Q;
    memset(&Q, 0, sizeof Q);
    std::vector<float> tab(curves_bytes(&q) / sizeof(float));
    const htj2k_tensor_curve *cv[2] = { &q.in, &q.out };
    size_t at = 0;
    for (const htj2k_tensor_curve *v : cv) {
        const size_t nf = curve_floats(*v);
        for (size_t j = 0; j < nf; j++) tab[at + j] = v->t[std::min<size_t>(j, (size_t)v->n - 1)];
        at += nf;
    }
    Q.tab = (const float *)call->put(tab.data(), tab.size() * sizeof(float));
    Q.n_in = (uint32_t)q.in.n; Q.n_out = (uint32_t)q.out.n;
    Q.out_at = (uint32_t)curve_floats(q.in); Q.nfloat = (uint32_t)tab.size();
    Q.x0_in = q.in.x0; Q.inv_in = q.in.inv_dx; Q.x0_out = q.out.x0; Q.inv_out = q.out.inv_dx;
    Q.in_mask = q.in.n ? q.in_mask : 0; Q.out_mask = q.out.n ? q.out_mask : 0;
    for (int k = 0; k < T.nout; k++) { Q.gain[k] = q.gain[k]; Q.offset[k] = q.offset[k]; }
    return Q;
}

/* The grid of a launch with curves.  meas_launch gives a workgroup one unit of work a thread on small calls; here every
 * workgroup first stages the tables, so grid.x is also kept to what leaves a workgroup CURVES_SRC_PER_TABLE times its
 * tables' bytes of source to read (one workgroup where the frame is smaller).  Knob "curves_grid" sets another factor
 * (results do not depend on it); what was measured under it: DESIGN.md 3.5, "Transfer curves" */
#define CURVES_SRC_PER_TABLE 4
static unsigned curves_grid(const htj2k_ctx *c, size_t gx, size_t src_bytes, size_t table_bytes)
{
    return curve_grid(gx, src_bytes, table_bytes, c->curves_grid ? (size_t)c->curves_grid : (size_t)CURVES_SRC_PER_TABLE);
}

/* as meas_launch, with the curves' grid rule and their dynamic LDS; src_bytes: what a frame's window reads */
template <class Kernel>
static void curves_launch(const htj2k_ctx *c, Kernel kernel, hipStream_t st, const MixFrame *d_frames, size_t nt, size_t work, size_t src_bytes, uint8_t *dst,
                          const MixFmt &F, const CurveFmt &Q)
{
    const size_t lds = (size_t)Q.nfloat * sizeof(float);
    const unsigned gx = curves_grid(c, std::min<size_t>((work + CMP_THREADS - 1) / CMP_THREADS, nt >= 64 ? 256 : 2048), src_bytes, lds);
    for (size_t z0 = 0; z0 < nt; z0 += 65535)
        hipLaunchKernelGGL(kernel, dim3(gx, 1, (unsigned)std::min<size_t>(65535, nt - z0)), dim3(CMP_THREADS), lds, st, d_frames + z0, dst, F, Q);
}

template <int DT, class B, class S, class N, class W>
static void curves_launch_fast(const htj2k_ctx *c, B, S, N, W, bool nhwc, hipStream_t st, const MixFrame *tab, size_t nt, size_t most, size_t src_bytes, uint8_t *dst,
                               const MixFmt &F, const CurveFmt &Q)
{
    if (nhwc) curves_launch(c, k_frame_curves<B::value, S::value, N::value, W::value, DT, 1>, st, tab, nt, most, src_bytes, dst, F, Q);
    else      curves_launch(c, k_frame_curves<B::value, S::value, N::value, W::value, DT, 0>, st, tab, nt, most, src_bytes, dst, F, Q);
}

/* bytes of source a frame's window holds: every component's samples, sub-sampled chroma counted once */
static size_t mix_window_bytes(const TensorCall &T, const MixCut &M)
{
    size_t b = 0;
    for (int c = 0; c < T.ncomp; c++) {
        const bool chroma = M.planar && (c == 1 || c == 2);
        b += (((size_t)T.ow + (chroma ? (1u << M.sw) - 1 : 0)) >> (chroma ? M.sw : 0)) *
             (((size_t)T.oh + (chroma ? (1u << M.sh) - 1 : 0)) >> (chroma ? M.sh : 0)) * (size_t)T.L.bytes;
    }
    return b;
}

/* the checked plain call with a mix: as tensor_run, a frame per table entry.  Routes 5 (fast), 6 (general), 7 (both);
 * with curves 9, 10, 11 */
static int mix_run(htj2k_ctx *c, const TensorCall &T, const htj2k_frame *f, int on_dev, int n, const uint8_t *skip,
                   const int32_t *origins, void *dst)
{
    const CmpLayout &L = T.L;
    const MixCut M = mix_cut(T);
    MeasCall call(c);
    c->tensor_route = 0;
    auto there = [&](int i) { return !(skip && skip[i]); };
    size_t np = 0;
    const size_t staged = tensor_staged_bytes(L, f, on_dev, n, skip, &np);
    int r = call.reserve(0, 0, np / (size_t)L.nplanes, sizeof(MixFrame), staged + curves_bytes(T.curves));
    if (r < 0) return r;
    std::vector<MixFrame> fast, any;
    const size_t per16 = 16 / T.esize;
    const size_t share = M.np ? (((size_t)M.np % per16 == 0 && (size_t)M.np / per16 >= 2) ? (size_t)M.np / per16 : 1) : 1;   /* MixShape::SHARE */
    for (int i = 0; i < n; i++) {
        if (!there(i)) continue;
        const int ox = origins ? origins[2 * i] : 0, oy = origins ? origins[2 * i + 1] : 0;
        MixFrame P;
        memset(&P, 0, sizeof P);
        for (int p = 0; p < L.nplanes; p++) {
            if (on_dev) { P.src[p] = f[i].data[p]; P.ls[p] = f[i].linesize[p]; }
            else call.stage(f[i], p, pix_plane(L.pd, f[i].width, f[i].height, p), &P.src[p], &P.ls[p]);
        }
        P.dst_img = (uint64_t)i * T.elems;
        P.oy = (uint32_t)oy;
        if (!c->tensor_path && mix_fast(T, M, P, ox)) {
            for (int p = 0; p < L.nplanes; p++)
                P.src[p] += (int64_t)(ox >> ((M.planar && (p == 1 || p == 2)) ? M.sw : 0)) * L.step * L.bytes;
            P.wide = mix_wide(T, M, dst, P.dst_img);
            fast.push_back(P);
        } else {
            P.ox = (uint32_t)ox;
            any.push_back(P);
        }
    }
    MixFrame *tab = (MixFrame *)call.h;
    if (!fast.empty()) memcpy(tab, fast.data(), fast.size() * sizeof(MixFrame));
    if (!any.empty()) memcpy(tab + fast.size(), any.data(), any.size() * sizeof(MixFrame));
    const MixFmt F = mix_fmt(T, M);
    CurveFmt Q;
    if (T.curves) Q = curves_fmt(T, &call);
    const size_t src_bytes = mix_window_bytes(T, M);
    const size_t most_fast = M.np ? (((size_t)T.ow + M.np - 1) / M.np) * (size_t)T.oh * share : 1, most_any = (size_t)T.ow * T.oh;
    int route = 0;
    r = call.run(fast.size() + any.size(), [&](hipStream_t st, const void *d_tab, void *) {
        uint8_t *out = (uint8_t *)dst;
        for (int i = 0; i < n; i++)
            if (!there(i)) HIP_TRY(c, hipMemsetAsync(out + (size_t)i * T.elems * T.esize, 0, T.elems * T.esize, st));
        const MixFrame *dt = (const MixFrame *)d_tab;
        if (!fast.empty()) {
            const int rr = mix_dispatch(T, M, [&](auto B, auto S, auto N, auto W) {
                if (T.curves) {
                    switch (T.dtype) {
                    case HTJ2K_TENSOR_F32:  curves_launch_fast<TENSOR_F32>(c, B, S, N, W, F.nhwc != 0, st, dt, fast.size(), most_fast, src_bytes, out, F, Q); break;
                    case HTJ2K_TENSOR_F16:  curves_launch_fast<TENSOR_F16>(c, B, S, N, W, F.nhwc != 0, st, dt, fast.size(), most_fast, src_bytes, out, F, Q); break;
                    default:                curves_launch_fast<TENSOR_BF16>(c, B, S, N, W, F.nhwc != 0, st, dt, fast.size(), most_fast, src_bytes, out, F, Q); break;
                    }
                    return;
                }
                switch (T.dtype) {
                case HTJ2K_TENSOR_F32:  mix_launch_fast<TENSOR_F32>(B, S, N, W, F.nhwc != 0, st, dt, fast.size(), most_fast, out, F); break;
                case HTJ2K_TENSOR_F16:  mix_launch_fast<TENSOR_F16>(B, S, N, W, F.nhwc != 0, st, dt, fast.size(), most_fast, out, F); break;
                default:                mix_launch_fast<TENSOR_BF16>(B, S, N, W, F.nhwc != 0, st, dt, fast.size(), most_fast, out, F); break;
                }
            });
            if (rr < 0) return rr;
            route |= 1;
        }
        if (!any.empty()) {
            const MixFrame *da = dt + fast.size();
            if (T.curves) switch (T.dtype) {
            case HTJ2K_TENSOR_F32:  curves_launch(c, k_frame_curves_any<TENSOR_F32>, st, da, any.size(), most_any, src_bytes, out, F, Q); break;
            case HTJ2K_TENSOR_F16:  curves_launch(c, k_frame_curves_any<TENSOR_F16>, st, da, any.size(), most_any, src_bytes, out, F, Q); break;
            default:                curves_launch(c, k_frame_curves_any<TENSOR_BF16>, st, da, any.size(), most_any, src_bytes, out, F, Q); break;
            }
            else switch (T.dtype) {
            case HTJ2K_TENSOR_F32:  meas_launch(k_frame_mix_any<TENSOR_F32>, st, da, any.size(), most_any, CMP_THREADS, out, F); break;
            case HTJ2K_TENSOR_F16:  meas_launch(k_frame_mix_any<TENSOR_F16>, st, da, any.size(), most_any, CMP_THREADS, out, F); break;
            default:                meas_launch(k_frame_mix_any<TENSOR_BF16>, st, da, any.size(), most_any, CMP_THREADS, out, F); break;
            }
            route |= 2;
        }
        return 0;
    });
    if (r < 0) return r;
    c->tensor_route = route ? (T.curves ? 8 : 4) + route : 0;
    return 0;
}

/* k_tensor_mix over nimg images of the scratch, for a checked resized call with a mix */
template <int DT>
static void mix_launch_scratch(bool nhwc, hipStream_t st, const float *src, uint8_t *dst, uint64_t dst_img, uint32_t nimg, const MixFmt &F)
{
    const uint64_t total = (uint64_t)F.out_w * F.out_h * nimg;
    const unsigned gx = (unsigned)std::min<uint64_t>((total + CMP_THREADS - 1) / CMP_THREADS, 65536);
    if (nhwc) hipLaunchKernelGGL((k_tensor_mix<DT, 1>), dim3(gx), dim3(CMP_THREADS), 0, st, src, dst, dst_img, nimg, F);
    else      hipLaunchKernelGGL((k_tensor_mix<DT, 0>), dim3(gx), dim3(CMP_THREADS), 0, st, src, dst, dst_img, nimg, F);
}

/* the same with curves: k_tensor_curves, its grid under the curves' rule */
template <int DT>
static void curves_launch_scratch(const htj2k_ctx *c, bool nhwc, hipStream_t st, const float *src, uint8_t *dst, uint64_t dst_img, uint32_t nimg, const MixFmt &F,
                                  const CurveFmt &Q)
{
    const uint64_t total = (uint64_t)F.out_w * F.out_h * nimg;
    const size_t lds = (size_t)Q.nfloat * sizeof(float);
    const unsigned gx = curves_grid(c, (size_t)std::min<uint64_t>((total + CMP_THREADS - 1) / CMP_THREADS, 65536), (size_t)total * F.ncomp * 4, lds);
    if (nhwc) hipLaunchKernelGGL((k_tensor_curves<DT, 1>), dim3(gx), dim3(CMP_THREADS), lds, st, src, dst, dst_img, nimg, F, Q);
    else      hipLaunchKernelGGL((k_tensor_curves<DT, 0>), dim3(gx), dim3(CMP_THREADS), lds, st, src, dst, dst_img, nimg, F, Q);
}

/* bytes of the scratch a chunk of frames of a resized call with a mix may take when knob "mix_scratch" is 0: a choice,
 * not a measured number (a quarter of the last-level cache, so that the round trip has a chance to stay in it) */
#define MIX_SCRATCH_DEFAULT (64 << 20)

/* log2 of the lanes of k_frame_resize that share the taps of one horizontal sum: as many as leave a lane about 48 sample
 * loads, taps times interleaved components (measured under knob "resize_share": one lane for all 36 x 3 loads of rgb24
 * 3840 -> 224 took 2.3 times as long as four, and more lanes than this cost 1.2 to 5 times on every row; DESIGN.md 3.5,
 * "Resized windows").  Results do not depend on it */
static uint32_t resize_share(int ww, int ow, int step, int filter)
{
    const int taps = filter == HTJ2K_RESIZE_TRIANGLE && ww > ow ? (int)((2 * (int64_t)ww + ow - 1) / ow) + 1 : 2;
    uint32_t share = 0;
    while (share < 5 && (48 << share) <= taps * step) share++;
    return share;
}

/* the checked resized call (resize_kernels.hpp): as tensor_run, with one kernel for every plane; the table holds every
 * plane's window, and the weights are made on the device */
static int resize_run(htj2k_ctx *c, const TensorCall &T, const htj2k_frame *f, int on_dev, int n, const uint8_t *skip,
                      const ResizeArgs &rs, void *dst)
{
    const CmpLayout &L = T.L;
    MeasCall call(c);
    c->tensor_route = 0;
    auto there = [&](int i) { return !(skip && skip[i]); };
    size_t nt = 0;
    const size_t staged = tensor_staged_bytes(L, f, on_dev, n, skip, &nt);
    int r = call.reserve(0, 0, nt, sizeof(ResizePlane), staged + curves_bytes(T.curves));
    if (r < 0) return r;
    ResizePlane *tab = (ResizePlane *)call.h;
    /* with a mix the kernel writes f_c itself, float32 NCHW at scale 1 and bias 0 (f * 1 + 0 is f for the non-negative
     * finite values it makes), into the context's scratch, `chunk` frames at a time; k_tensor_mix takes them from there */
    TensorCall Tr = T;
    int chunk = n;
    if (T.mix) {
        Tr.dtype = HTJ2K_TENSOR_F32; Tr.nhwc = 0; Tr.esize = 4;
        Tr.elems = (size_t)T.ncomp * (size_t)T.ow * (size_t)T.oh;
        for (int k = 0; k < 4; k++) { Tr.scale[k] = 1.0f; Tr.bias[k] = 0.0f; }
        const size_t room = c->mix_scratch ? (size_t)c->mix_scratch : (size_t)MIX_SCRATCH_DEFAULT;
        chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, room / (Tr.elems * 4)));
        if ((r = c->mix_d.ensure((size_t)chunk * Tr.elems * 4)) < 0) return r;
    }
    std::vector<size_t> ent((size_t)n + 1, 0);             /* frame i's first entry of the table */
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        ent[i] = at;
        ent[i + 1] = at;
        if (!there(i)) continue;
        ent[i + 1] = at + (size_t)L.nplanes;
        int32_t w[4];
        resize_window(rs, f, i, w);
        for (int p = 0; p < L.nplanes; p++) {
            ResizePlane &P = tab[at++];
            memset(&P, 0, sizeof P);
            if (on_dev) { P.src = f[i].data[p]; P.ls = f[i].linesize[p]; }
            else call.stage(f[i], p, pix_plane(L.pd, f[i].width, f[i].height, p), &P.src, &P.ls);
            const int k = L.pd->planar ? p : 0;
            P.dst_img = T.mix ? (uint64_t)(i % chunk) * Tr.elems : (uint64_t)i * T.elems;
            P.ox = (uint32_t)w[0]; P.oy = (uint32_t)w[1]; P.ww = (uint32_t)w[2]; P.wh = (uint32_t)w[3];
            P.comp0 = (uint32_t)k;
            P.step = (uint32_t)L.step;
            P.sw = (k == 1 || k == 2) ? L.pd->log2_chroma_w : 0;
            P.sh = (k == 1 || k == 2) ? L.pd->log2_chroma_h : 0;
            P.pair = (((uintptr_t)P.src | (uint64_t)P.ls) & 1) == 0;
            P.share = c->resize_share ? (uint32_t)c->resize_share - 1 : resize_share(w[2], T.ow, L.step, rs.filter);
        }
    }
    CurveFmt Q;
    if (T.curves) Q = curves_fmt(T, &call);
    ResizeFmt R;
    R.T = tensor_fmt(Tr);
    R.filter = (uint32_t)rs.filter;
    R.rows = (uint32_t)(c->resize_rows ? c->resize_rows : RS_ROWS_DEFAULT);
    const size_t tiles = (((size_t)T.ow + RS_TW - 1) / RS_TW) * (((size_t)T.oh + RS_TH - 1) / RS_TH);
    r = call.run(nt, [&](hipStream_t st, const void *d_tab, void *) {
        uint8_t *out = (uint8_t *)dst;
        for (int i = 0; i < n; i++)
            if (!there(i)) HIP_TRY(c, hipMemsetAsync(out + (size_t)i * T.elems * T.esize, 0, T.elems * T.esize, st));
        const ResizePlane *dt = (const ResizePlane *)d_tab;
        if (T.mix) {
            const MixFmt MF = mix_fmt(T, mix_cut(T));
            for (int i0 = 0; i0 < n; i0 += chunk) {
                const int i1 = std::min(n, i0 + chunk);
                if (ent[i1] > ent[i0])
                    meas_launch(k_frame_resize<TENSOR_F32>, st, dt + ent[i0], ent[i1] - ent[i0], tiles, 1, (uint8_t *)c->mix_d.p, R);
                for (int i = i0; i < i1;) {                  /* runs of frames that are there */
                    int j = i;
                    while (j < i1 && there(j)) j++;
                    if (j > i) {
                        const float *src = (const float *)c->mix_d.p + (size_t)(i - i0) * Tr.elems;
                        if (T.curves) switch (T.dtype) {
                        case HTJ2K_TENSOR_F32:  curves_launch_scratch<TENSOR_F32>(c, MF.nhwc != 0, st, src, out, (uint64_t)i * T.elems, (uint32_t)(j - i), MF, Q); break;
                        case HTJ2K_TENSOR_F16:  curves_launch_scratch<TENSOR_F16>(c, MF.nhwc != 0, st, src, out, (uint64_t)i * T.elems, (uint32_t)(j - i), MF, Q); break;
                        default:                curves_launch_scratch<TENSOR_BF16>(c, MF.nhwc != 0, st, src, out, (uint64_t)i * T.elems, (uint32_t)(j - i), MF, Q); break;
                        }
                        else switch (T.dtype) {
                        case HTJ2K_TENSOR_F32:  mix_launch_scratch<TENSOR_F32>(MF.nhwc != 0, st, src, out, (uint64_t)i * T.elems, (uint32_t)(j - i), MF); break;
                        case HTJ2K_TENSOR_F16:  mix_launch_scratch<TENSOR_F16>(MF.nhwc != 0, st, src, out, (uint64_t)i * T.elems, (uint32_t)(j - i), MF); break;
                        default:                mix_launch_scratch<TENSOR_BF16>(MF.nhwc != 0, st, src, out, (uint64_t)i * T.elems, (uint32_t)(j - i), MF); break;
                        }
                    }
                    i = j + 1;
                }
            }
            return 0;
        }
        switch (T.dtype) {
        case HTJ2K_TENSOR_F32:  meas_launch(k_frame_resize<TENSOR_F32>, st, dt, nt, tiles, 1, out, R); break;
        case HTJ2K_TENSOR_F16:  meas_launch(k_frame_resize<TENSOR_F16>, st, dt, nt, tiles, 1, out, R); break;
        default:                meas_launch(k_frame_resize<TENSOR_BF16>, st, dt, nt, tiles, 1, out, R); break;
        }
        return 0;
    });
    if (r < 0) return r;
    c->tensor_route = T.curves ? 12 : T.mix ? 8 : 4;
    return 0;
}

extern "C" int htj2k_resize_weights(int win, int out, int filter, int x, int32_t *first, uint16_t *q, int cap)
{
    if (!first || !q || filter < HTJ2K_RESIZE_NEAREST || filter > HTJ2K_RESIZE_TRIANGLE) return HTJ2K_ERR_EINVAL;
    if (win < 1 || out < 1 || x < 0 || x >= out) return HTJ2K_ERR_EINVAL;
    if (win > RS_MAX_SIZE || out > RS_MAX_SIZE || (filter == HTJ2K_RESIZE_TRIANGLE && win > (int64_t)RS_MAX_REDUCTION * out))
        return HTJ2K_ERR_PATCHWELCOME;
    uint16_t w[RS_MAX_TAPS];
    const int n = resize_weights(win, out, filter, x, first, w);
    if (n > cap) return HTJ2K_ERR_EINVAL;
    memcpy(q, w, (size_t)n * sizeof(uint16_t));
    return n;
}

extern "C" int htj2k_frames_to_tensor_resized_curves(htj2k_ctx *c, const htj2k_frame *f, int on_device, int n, int bits,
                                                     const htj2k_tensor_spec *spec, const htj2k_tensor_mix *mix,
                                                     const htj2k_tensor_curves *curves, const int32_t *windows, int filter, void *dst,
                                                     size_t dst_bytes)
{
    if (c) c->tensor_route = 0;
    if (!f || !spec || !dst || n < 1) return HTJ2K_ERR_EINVAL;
    const ResizeArgs rs = { windows, filter, c };
    TensorCall T;
    int r = tensor_spec_check(f[0].pix_fmt, bits, spec, &T, &rs, mix, nullptr, curves);
    if (r < 0) return r;
    if ((r = tensor_frames_check(&T, f, n, nullptr, f[0].pix_fmt, nullptr, dst, dst_bytes, &rs)) < 0) return r;
    if (!c) return HTJ2K_ERR_ENOSYS;
    return resize_run(c, T, f, on_device, n, nullptr, rs, dst);
}

extern "C" int htj2k_frames_to_tensor_resized_mix(htj2k_ctx *c, const htj2k_frame *f, int on_device, int n, int bits,
                                                  const htj2k_tensor_spec *spec, const htj2k_tensor_mix *mix, const int32_t *windows,
                                                  int filter, void *dst, size_t dst_bytes)
{
    return htj2k_frames_to_tensor_resized_curves(c, f, on_device, n, bits, spec, mix, nullptr, windows, filter, dst, dst_bytes);
}

extern "C" int htj2k_frames_to_tensor_resized(htj2k_ctx *c, const htj2k_frame *f, int on_device, int n, int bits, const htj2k_tensor_spec *spec,
                                              const int32_t *windows, int filter, void *dst, size_t dst_bytes)
{
    return htj2k_frames_to_tensor_resized_mix(c, f, on_device, n, bits, spec, nullptr, windows, filter, dst, dst_bytes);
}

extern "C" void htj2k_tensor_spec_default(htj2k_tensor_spec *s)
{
    if (!s) return;
    memset(s, 0, sizeof *s);
    s->dtype = HTJ2K_TENSOR_F32;
    s->layout = HTJ2K_TENSOR_NCHW;
    for (int k = 0; k < 4; k++) s->scale[k] = 1.0f;
}

/* Y'CbCr -> R'G'B' as a mix: every entry in double, gain and offset folded in, rounded to float once */
extern "C" int htj2k_tensor_mix_ycbcr(htj2k_tensor_mix *mix, int standard, int full_range, int bits, int alpha, const float gain[3],
                                      const float offset[3])
{
    if (!mix) return HTJ2K_ERR_EINVAL;
    double kr, kb;
    switch (standard) {
    case 601:  kr = 0.299;  kb = 0.114;  break;
    case 709:  kr = 0.2126; kb = 0.0722; break;
    case 2020: kr = 0.2627; kb = 0.0593; break;
    default: return HTJ2K_ERR_EINVAL;
    }
    if (bits < 8 || bits > 16) return HTJ2K_ERR_EINVAL;
    for (int k = 0; k < 3; k++)
        if ((gain && !std::isfinite(gain[k])) || (offset && !std::isfinite(offset[k]))) return HTJ2K_ERR_EINVAL;
    const double kg = 1.0 - kr - kb, q = (double)(1 << (bits - 8)), peak = (double)((1 << bits) - 1), mid = (double)(1 << (bits - 1));
    const double ys = full_range ? 1.0 / peak : 1.0 / (219.0 * q), y0 = full_range ? 0.0 : 16.0 * q;   /* Y' = (s_Y - y0) ys */
    const double cs = full_range ? 1.0 / peak : 1.0 / (224.0 * q);                                     /* Pb = (s_Cb - mid) cs */
    const double w[3][3] = { { 1.0, 0.0, 2.0 * (1.0 - kr) },                                           /* of Y', Pb, Pr */
                             { 1.0, -(2.0 * kb * (1.0 - kb) / kg), -(2.0 * kr * (1.0 - kr) / kg) },
                             { 1.0, 2.0 * (1.0 - kb), 0.0 } };
    memset(mix, 0, sizeof *mix);
    mix->nout = alpha ? 4 : 3;
    for (int k = 0; k < 3; k++) {
        const double g = gain ? (double)gain[k] : 1.0, o = offset ? (double)offset[k] : 0.0;
        mix->m[k][0] = (float)(g * (w[k][0] * ys));
        mix->m[k][1] = (float)(g * (w[k][1] * cs));
        mix->m[k][2] = (float)(g * (w[k][2] * cs));
        mix->b[k] = (float)(g * (-(y0 * ys) * w[k][0] - (mid * cs) * (w[k][1] + w[k][2])) + o);
    }
    if (alpha) mix->m[3][3] = (float)(1.0 / peak);
    return 0;
}

/* the transfer functions of htj2k_tensor_curve_fill, in double; x is clamped to 0 .. 1 for all but the power law */
static double curve_function(int kind, double param, double x)
{
    if (kind == HTJ2K_CURVE_POWER) return pow(std::max(x, 0.0), param);
    x = std::min(std::max(x, 0.0), 1.0);
    const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0;                  /* SMPTE ST 2084 */
    const double c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
    switch (kind) {
    case HTJ2K_CURVE_SRGB_ENCODE:  return x <= 0.0031308 ? 12.92 * x : 1.055 * pow(x, 1.0 / 2.4) - 0.055;
    case HTJ2K_CURVE_SRGB_DECODE:  return x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4);
    case HTJ2K_CURVE_BT709_ENCODE: return x < 0.018 ? 4.5 * x : 1.099 * pow(x, 0.45) - 0.099;
    case HTJ2K_CURVE_BT709_DECODE: return x < 0.081 ? x / 4.5 : pow((x + 0.099) / 1.099, 1.0 / 0.45);
    case HTJ2K_CURVE_PQ_ENCODE:  { const double y = pow(x, m1); return pow((c1 + c2 * y) / (1.0 + c3 * y), m2); }
    default:                     { const double p = pow(x, 1.0 / m2); return pow(std::max(p - c1, 0.0) / (c2 - c3 * p), 1.0 / m1); }
    }
}

extern "C" int htj2k_tensor_curve_fill(float *t, int n, int kind, double param, double lo, double hi)
{
    if (!t || n < 2 || kind < HTJ2K_CURVE_POWER || kind > HTJ2K_CURVE_PQ_DECODE) return HTJ2K_ERR_EINVAL;
    if (!std::isfinite(param) || !std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo)) return HTJ2K_ERR_EINVAL;
    for (int j = 0; j < n; j++) t[j] = (float)curve_function(kind, param, lo + (double)j * (hi - lo) / (double)(n - 1));
    return 0;
}

/* the table of a curve with a root: knot j stands at y_j in the rooted argument, so it holds F(y_j ^ (2 ^ root)), the
 * power by `root` squarings in double */
extern "C" int htj2k_tensor_curve_fill_root(float *t, int n, int kind, double param, double lo, double hi, int root)
{
    if (root == 0) return htj2k_tensor_curve_fill(t, n, kind, param, lo, hi);
    if (!t || n < 2 || kind < HTJ2K_CURVE_POWER || kind > HTJ2K_CURVE_PQ_DECODE) return HTJ2K_ERR_EINVAL;
    if (!std::isfinite(param) || !std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo)) return HTJ2K_ERR_EINVAL;
    if (root < 0 || root > HTJ2K_CURVE_MAX_ROOT) return HTJ2K_ERR_EINVAL;
    for (int j = 0; j < n; j++) {
        double y = lo + (double)j * (hi - lo) / (double)(n - 1);
        for (int r = 0; r < root; r++) y = y * y;
        t[j] = (float)curve_function(kind, param, y);
    }
    return 0;
}

static void inv3(const double a[3][3], double o[3][3])
{
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])
                     + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;   /* the cofactor of a[c][r] */
            o[r][c] = (a[r1][c1] * a[r2][c2] - a[r1][c2] * a[r2][c1]) / det;
        }
}

/* the normalised primary matrix (SMPTE RP 177) of the primaries and D65: linear RGB -> linear XYZ */
static int primary_matrix(int primaries, double N[3][3])
{
    static const double P709[3][2] = { { 0.640, 0.330 }, { 0.300, 0.600 }, { 0.150, 0.060 } };
    static const double P2020[3][2] = { { 0.708, 0.292 }, { 0.170, 0.797 }, { 0.131, 0.046 } };
    static const double PP3[3][2] = { { 0.680, 0.320 }, { 0.265, 0.690 }, { 0.150, 0.060 } };
    const double (*p)[2];
    switch (primaries) {
    case 709:  p = P709;  break;
    case 2020: p = P2020; break;
    case HTJ2K_PRIMARIES_P3D65: p = PP3; break;
    default: return HTJ2K_ERR_EINVAL;
    }
    const double xw = 0.3127, yw = 0.3290;
    double A[3][3], Ai[3][3];
    for (int j = 0; j < 3; j++) { A[0][j] = p[j][0] / p[j][1]; A[1][j] = 1.0; A[2][j] = (1.0 - p[j][0] - p[j][1]) / p[j][1]; }
    const double W[3] = { xw / yw, 1.0, (1.0 - xw - yw) / yw };
    inv3(A, Ai);
    for (int j = 0; j < 3; j++) {
        const double s = Ai[j][0] * W[0] + Ai[j][1] * W[1] + Ai[j][2] * W[2];
        for (int r = 0; r < 3; r++) N[r][j] = A[r][j] * s;
    }
    return 0;
}

/* linear XYZ -> linear RGB: the inverse of the normalised primary matrix, times `scale`; a DCI master's X'Y'Z' decoded by
 * the 2.6 law is XYZ * 48 / 52.37, so its scale is 52.37 / 48 */
extern "C" int htj2k_tensor_mix_xyz(htj2k_tensor_mix *mix, int primaries, double scale)
{
    if (!mix || !std::isfinite(scale)) return HTJ2K_ERR_EINVAL;
    double N[3][3], Ni[3][3];
    if (primary_matrix(primaries, N) < 0) return HTJ2K_ERR_EINVAL;
    inv3(N, Ni);
    memset(mix, 0, sizeof *mix);
    mix->nout = 3;
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 3; c++) mix->m[k][c] = (float)(Ni[k][c] * scale);
    return 0;
}

/* linear RGB -> linear XYZ on the way in: the normalised primary matrix itself, times `scale`; the inverse of
 * htj2k_tensor_mix_xyz with the reciprocal scale.  A DCI master codes XYZ * 48 / 52.37, so its scale is 48 / 52.37 */
extern "C" int htj2k_tensor_mix_in_xyz(htj2k_tensor_mix_in *mix, int primaries, double scale)
{
    if (!mix || !std::isfinite(scale)) return HTJ2K_ERR_EINVAL;
    double N[3][3];
    if (primary_matrix(primaries, N) < 0) return HTJ2K_ERR_EINVAL;
    memset(mix, 0, sizeof *mix);
    mix->nin = 3;
    mix->chroma = HTJ2K_CHROMA_COSITED;
    for (int c = 0; c < 3; c++)
        for (int k = 0; k < 3; k++) mix->m[c][k] = (float)(N[c][k] * scale);
    return 0;
}

/* the image of a call with a mix of either direction (at most one of them) */
static int tensor_image_size(int pix_fmt, int width, int height, int bits, const htj2k_tensor_spec *spec, const htj2k_tensor_mix *mix,
                             const htj2k_tensor_mix_in *mix_in, size_t *elems, size_t *bytes, const htj2k_tensor_curves_in *curves_in = nullptr)
{
    if (!spec) return HTJ2K_ERR_EINVAL;
    TensorCall T;
    const int r = tensor_spec_check(pix_fmt, bits, spec, &T, nullptr, mix, mix_in, nullptr, curves_in);
    if (r < 0) return r;
    if (width < 1 || height < 1 || (int64_t)width * T.L.step * T.L.bytes > INT32_MAX) return HTJ2K_ERR_EINVAL;
    if (!T.ow) { T.ow = width; T.oh = height; }
    if (T.ow > width || T.oh > height) return HTJ2K_ERR_EINVAL;
    const size_t e = (size_t)T.nout * (size_t)T.ow * (size_t)T.oh;
    if (elems) *elems = e;
    if (bytes) *bytes = e * T.esize;
    return 0;
}

extern "C" int htj2k_tensor_image_size_mix(int pix_fmt, int width, int height, int bits, const htj2k_tensor_spec *spec,
                                           const htj2k_tensor_mix *mix, size_t *elems, size_t *bytes)
{
    return tensor_image_size(pix_fmt, width, height, bits, spec, mix, nullptr, elems, bytes);
}

extern "C" int htj2k_tensor_image_size_mix_in(int pix_fmt, int width, int height, int bits, const htj2k_tensor_spec *spec,
                                              const htj2k_tensor_mix_in *mix, size_t *elems, size_t *bytes)
{
    return tensor_image_size(pix_fmt, width, height, bits, spec, nullptr, mix, elems, bytes);
}

/* for htj2k_encode_tensor_curves (htj2k_encode.hip): the same with the curves checked behind the mix; declared in j2k_enc.h,
 * not exported */
extern "C" int htj2k_tensor_image_size_curves_in_(int pix_fmt, int width, int height, int bits, const htj2k_tensor_spec *spec,
                                                  const htj2k_tensor_mix_in *mix, const htj2k_tensor_curves_in *curves, size_t *elems, size_t *bytes)
{
    return tensor_image_size(pix_fmt, width, height, bits, spec, nullptr, mix, elems, bytes, curves);
}

/* R'G'B' (times gain plus offset) -> Y'CbCr as a mix on the way in: the inverse of htj2k_tensor_mix_ycbcr, every entry in
 * double, rounded to float once */
extern "C" int htj2k_tensor_mix_in_rgb(htj2k_tensor_mix_in *mix, int standard, int full_range, int bits, int alpha, const float gain[3],
                                       const float offset[3], int chroma)
{
    if (!mix) return HTJ2K_ERR_EINVAL;
    double kr, kb;
    switch (standard) {
    case 601:  kr = 0.299;  kb = 0.114;  break;
    case 709:  kr = 0.2126; kb = 0.0722; break;
    case 2020: kr = 0.2627; kb = 0.0593; break;
    default: return HTJ2K_ERR_EINVAL;
    }
    if (bits < 8 || bits > 16) return HTJ2K_ERR_EINVAL;
    for (int k = 0; k < 3; k++)
        if ((gain && (!std::isfinite(gain[k]) || gain[k] == 0.0f)) || (offset && !std::isfinite(offset[k]))) return HTJ2K_ERR_EINVAL;
    if (chroma < HTJ2K_CHROMA_COSITED || chroma > HTJ2K_CHROMA_BOX) return HTJ2K_ERR_EINVAL;
    const double kg = 1.0 - kr - kb, q = (double)(1 << (bits - 8)), peak = (double)((1 << bits) - 1), mid = (double)(1 << (bits - 1));
    const double ys = full_range ? peak : 219.0 * q, y0 = full_range ? 0.0 : 16.0 * q;     /* s_Y = y0 + ys Y' */
    const double cs = full_range ? peak : 224.0 * q;                                       /* s_Cb = mid + cs Pb */
    const double pb = cs / (2.0 * (1.0 - kb)), pr = cs / (2.0 * (1.0 - kr));
    const double A[3][3] = { { ys * kr, ys * kg, ys * kb },                                /* of R', G', B' */
                             { -pb * kr, -pb * kg, pb * (1.0 - kb) },
                             { pr * (1.0 - kr), -pr * kg, -pr * kb } };
    const double o[3] = { y0, mid, mid };
    memset(mix, 0, sizeof *mix);
    mix->nin = alpha ? 4 : 3;
    mix->chroma = chroma;
    for (int c = 0; c < 3; c++) {
        double b = o[c];
        for (int k = 0; k < 3; k++) {
            const double g = gain ? (double)gain[k] : 1.0, off = offset ? (double)offset[k] : 0.0;
            mix->m[c][k] = (float)(A[c][k] / g);
            b -= A[c][k] * off / g;
        }
        mix->b[c] = (float)b;
    }
    if (alpha) mix->m[3][3] = (float)peak;
    return 0;
}

extern "C" int htj2k_tensor_image_size(int pix_fmt, int width, int height, int bits, const htj2k_tensor_spec *spec, size_t *elems, size_t *bytes)
{
    return htj2k_tensor_image_size_mix(pix_fmt, width, height, bits, spec, nullptr, elems, bytes);
}

extern "C" int htj2k_frames_to_tensor_curves(htj2k_ctx *c, const htj2k_frame *f, int on_device, int n, int bits, const htj2k_tensor_spec *spec,
                                             const htj2k_tensor_mix *mix, const htj2k_tensor_curves *curves, const int32_t *origins,
                                             void *dst, size_t dst_bytes)
{
    if (c) c->tensor_route = 0;
    if (!f || !spec || !dst || n < 1) return HTJ2K_ERR_EINVAL;
    TensorCall T;
    int r = tensor_spec_check(f[0].pix_fmt, bits, spec, &T, nullptr, mix, nullptr, curves);
    if (r < 0) return r;
    if ((r = tensor_frames_check(&T, f, n, nullptr, f[0].pix_fmt, origins, dst, dst_bytes)) < 0) return r;
    if (!c) return HTJ2K_ERR_ENOSYS;
    return mix ? mix_run(c, T, f, on_device, n, nullptr, origins, dst) : tensor_run(c, T, f, on_device, n, nullptr, origins, dst);
}

extern "C" int htj2k_frames_to_tensor_mix(htj2k_ctx *c, const htj2k_frame *f, int on_device, int n, int bits, const htj2k_tensor_spec *spec,
                                          const htj2k_tensor_mix *mix, const int32_t *origins, void *dst, size_t dst_bytes)
{
    return htj2k_frames_to_tensor_curves(c, f, on_device, n, bits, spec, mix, nullptr, origins, dst, dst_bytes);
}

extern "C" int htj2k_frames_to_tensor(htj2k_ctx *c, const htj2k_frame *f, int on_device, int n, int bits, const htj2k_tensor_spec *spec,
                                      const int32_t *origins, void *dst, size_t dst_bytes)
{
    return htj2k_frames_to_tensor_mix(c, f, on_device, n, bits, spec, nullptr, origins, dst, dst_bytes);
}

/* frames f0 .. f0 + nf - 1 of the job (htj2k_job_to_tensor: all of them; the pipe: one); rs: resized, its windows in
 * place of the origins */
static int job_to_tensor(htj2k_ctx *c, htj2k_job *j, int f0, int nf, int bits, const htj2k_tensor_spec *spec, const htj2k_tensor_mix *mix,
                         const htj2k_tensor_curves *curves, const int32_t *origins, void *dst, size_t dst_bytes, int *status,
                         const ResizeArgs *rs = nullptr)
{
    if (c) c->tensor_route = 0;
    if (!j || !spec || !dst || j->nframes < 1 || f0 < 0 || nf < 1 || f0 + nf > j->nframes) return HTJ2K_ERR_EINVAL;
    if (!j->uploaded || !j->run.frames_ok) return HTJ2K_ERR_EINVAL;     /* no run yet, or one that did not write the frames */
    int first = -1;
    for (int f = 0; f < nf && first < 0; f++)
        if (j->frames[f0 + f].plan) first = f0 + f;
    if (first < 0) return HTJ2K_ERR_EINVAL;
    const htj2k_info &I0 = j->frames[first].plan->info;
    if (bits == 0) bits = I0.bits_per_raw_sample;
    TensorCall T;
    int r = tensor_spec_check(I0.pix_fmt, bits, spec, &T, rs, mix, nullptr, curves);
    if (r < 0) return r;
    std::vector<htj2k_frame> dev((size_t)nf);
    std::vector<uint8_t> skip((size_t)nf, 0);
    for (int f = 0; f < nf; f++) {
        const FrameSlot &F = j->frames[f0 + f];
        if (!F.plan) { skip[f] = 1; continue; }           /* no frame there: an image of zeros */
        job_frame_view(F, &dev[f]);
    }
    if ((r = tensor_frames_check(&T, dev.data(), nf, skip.data(), I0.pix_fmt, origins, dst, dst_bytes, rs)) < 0) return r;
    if (!c) return HTJ2K_ERR_ENOSYS;
    if ((r = job_settle(c, j)) < 0) return r;              /* waits for the job's stream; the planes are final behind it */
    r = rs ? resize_run(c, T, dev.data(), 1, nf, skip.data(), *rs, dst)
      : mix ? mix_run(c, T, dev.data(), 1, nf, skip.data(), origins, dst) : tensor_run(c, T, dev.data(), 1, nf, skip.data(), origins, dst);
    if (r < 0) return r;
    for (int f = 0; f < nf && status; f++) status[f] = skip[f];
    return 0;
}

extern "C" int htj2k_job_to_tensor_curves(htj2k_ctx *c, htj2k_job *j, int bits, const htj2k_tensor_spec *spec, const htj2k_tensor_mix *mix,
                                          const htj2k_tensor_curves *curves, const int32_t *origins, void *dst, size_t dst_bytes, int *status)
{
    return job_to_tensor(c, j, 0, j ? j->nframes : 0, bits, spec, mix, curves, origins, dst, dst_bytes, status);
}

extern "C" int htj2k_job_to_tensor_mix(htj2k_ctx *c, htj2k_job *j, int bits, const htj2k_tensor_spec *spec, const htj2k_tensor_mix *mix,
                                       const int32_t *origins, void *dst, size_t dst_bytes, int *status)
{
    return htj2k_job_to_tensor_curves(c, j, bits, spec, mix, nullptr, origins, dst, dst_bytes, status);
}

extern "C" int htj2k_job_to_tensor(htj2k_ctx *c, htj2k_job *j, int bits, const htj2k_tensor_spec *spec, const int32_t *origins,
                                   void *dst, size_t dst_bytes, int *status)
{
    return htj2k_job_to_tensor_mix(c, j, bits, spec, nullptr, origins, dst, dst_bytes, status);
}

extern "C" int htj2k_job_to_tensor_resized_curves(htj2k_ctx *c, htj2k_job *j, int bits, const htj2k_tensor_spec *spec,
                                                  const htj2k_tensor_mix *mix, const htj2k_tensor_curves *curves, const int32_t *windows,
                                                  int filter, void *dst, size_t dst_bytes, int *status)
{
    const ResizeArgs rs = { windows, filter, c };
    return job_to_tensor(c, j, 0, j ? j->nframes : 0, bits, spec, mix, curves, nullptr, dst, dst_bytes, status, &rs);
}

extern "C" int htj2k_job_to_tensor_resized_mix(htj2k_ctx *c, htj2k_job *j, int bits, const htj2k_tensor_spec *spec, const htj2k_tensor_mix *mix,
                                               const int32_t *windows, int filter, void *dst, size_t dst_bytes, int *status)
{
    return htj2k_job_to_tensor_resized_curves(c, j, bits, spec, mix, nullptr, windows, filter, dst, dst_bytes, status);
}

extern "C" int htj2k_job_to_tensor_resized(htj2k_ctx *c, htj2k_job *j, int bits, const htj2k_tensor_spec *spec, const int32_t *windows,
                                           int filter, void *dst, size_t dst_bytes, int *status)
{
    return htj2k_job_to_tensor_resized_mix(c, j, bits, spec, nullptr, windows, filter, dst, dst_bytes, status);
}

/* htj2k_pipe_receive_tensor and htj2k_pipe_receive_tensor_resized (htj2k_pipe.cpp): frame `frame` of a slot's job as one
 * image; a frame without a plan has nothing to give.  resized: `window` is ox, oy, ww, wh (NULL: the frame whole) and
 * `filter` counts; otherwise `window` is the origin */
extern "C" int htj2k_job_frame_to_tensor_(htj2k_ctx *c, htj2k_job *j, int frame, int bits, const htj2k_tensor_spec *spec,
                                          const htj2k_tensor_mix *mix, const htj2k_tensor_curves *curves, const int32_t *window,
                                          int resized, int filter, void *dst, size_t dst_bytes)
{
    const ResizeArgs rs = { window, filter, c };
    return job_to_tensor(c, j, frame, 1, bits, spec, mix, curves, resized ? nullptr : window, dst, dst_bytes, nullptr, resized ? &rs : nullptr);
}

extern "C" int htj2k_tensor_last_route(htj2k_ctx *c)
{
    return c ? c->tensor_route.load() : HTJ2K_ERR_EINVAL;
}

/* ---- resized frames (k_frame_rescale, resize_kernels.hpp): windows of frames resampled to frames of one size, every
 * plane on its own grid and in integers.  A MeasCall without results: its table holds every plane of every frame that is
 * there, source and destination side by side; host sources are staged as the other frame calls stage them. */

/* the planes of a width x height frame of a layout, from the table the checksums are laid out by (hash_layout) */
extern "C" int htj2k_frame_plane_sizes(int pix_fmt, int width, int height, int plane_w[4], int plane_h[4], int row_bytes[4])
{
    HashLayout H;
    if (!hash_layout(pix_fmt, width, height, &H)) return HTJ2K_ERR_EINVAL;
    const J2kPixDesc *pd = j2k_pix_desc(pix_fmt);
    for (int p = 0; p < H.nplanes; p++) {
        const size_t per = pd->pal && p == 1 ? 4 : (size_t)pd->bytes * (pd->planar ? 1 : pd->nb_components);   /* bytes of a pixel of the plane */
        if (plane_w) plane_w[p] = (int)(H.plane[p].rowbytes / per);
        if (plane_h) plane_h[p] = H.plane[p].rows;
        if (row_bytes) row_bytes[p] = (int)H.plane[p].rowbytes;
    }
    return H.nplanes;
}

/* refusals 3 to 13 of the header's list, in its order; skip[i] set (skip may be NULL): source frame i is not there, and
 * its window is checked for its sign and size only */
static int rescale_check(int pix_fmt, int bits, const htj2k_frame *src, int n, const uint8_t *skip, const ResizeArgs &rs,
                         const htj2k_frame *dst, CmpLayout *Lout)
{
    const int r = cmp_layout(pix_fmt, bits, Lout);       /* a pix_fmt outside the enum, PAL8, then bits */
    if (r < 0) return r;
    const CmpLayout &L = *Lout;
    if (rs.filter < HTJ2K_RESIZE_NEAREST || rs.filter > HTJ2K_RESIZE_TRIANGLE) return HTJ2K_ERR_EINVAL;
    auto there = [&](int i) { return !(skip && skip[i]); };
    int first = -1;
    for (int i = 0; i < n; i++)
        if (there(i) && src[i].pix_fmt != pix_fmt) return HTJ2K_ERR_EINVAL;
    for (int i = 0; i < n; i++) {
        if (!there(i)) continue;
        if (src[i].width < 1 || src[i].height < 1 || (int64_t)src[i].width * L.step * L.bytes > INT32_MAX) return HTJ2K_ERR_EINVAL;
        if (first < 0) first = i;
    }
    if (first < 0) return HTJ2K_ERR_EINVAL;
    for (int i = 0; i < n; i++)
        for (int p = 0; p < L.nplanes && there(i); p++)
            if (!src[i].data[p]) return HTJ2K_ERR_EINVAL;
    for (int i = 0; i < n; i++)
        for (int p = 0; p < L.nplanes && there(i); p++)
            if (src[i].linesize[p] < 0 || (size_t)src[i].linesize[p] < pix_plane(L.pd, src[i].width, src[i].height, p).rowbytes) return HTJ2K_ERR_EINVAL;
    const int ow = dst[0].width, oh = dst[0].height;
    for (int i = 0; i < n; i++)
        if (dst[i].pix_fmt != pix_fmt || dst[i].width != ow || dst[i].height != oh) return HTJ2K_ERR_EINVAL;
    if (ow < 1 || oh < 1 || (int64_t)ow * L.step * L.bytes > INT32_MAX) return HTJ2K_ERR_EINVAL;
    TensorCall T;                                          /* the windows' checks read the output's size from it */
    memset(&T, 0, sizeof T);
    T.ow = ow; T.oh = oh;
    const int rw = resize_windows_check(T, src, n, skip, rs, (1 << L.pd->log2_chroma_w) - 1, (1 << L.pd->log2_chroma_h) - 1);
    if (rw < 0) return rw;
    for (int i = 0; i < n; i++)
        for (int p = 0; p < L.nplanes; p++)
            if (!dst[i].data[p]) return HTJ2K_ERR_EINVAL;
    for (int i = 0; i < n; i++)
        for (int p = 0; p < L.nplanes; p++)
            if (dst[i].linesize[p] < 0 || (size_t)dst[i].linesize[p] < pix_plane(L.pd, ow, oh, p).rowbytes) return HTJ2K_ERR_EINVAL;
    return 0;
}

/* the checked call: one kernel for every plane of the frames that are there; a frame that is not gets zero samples */
static int rescale_run(htj2k_ctx *c, const CmpLayout &L, const htj2k_frame *f, int on_dev, int n, const uint8_t *skip, const ResizeArgs &rs,
                       const htj2k_frame *dst)
{
    MeasCall call(c);
    auto there = [&](int i) { return !(skip && skip[i]); };
    size_t nt = 0;
    const size_t staged = tensor_staged_bytes(L, f, on_dev, n, skip, &nt);
    int r = call.reserve(0, 0, nt, sizeof(RescalePlane), staged);
    if (r < 0) return r;
    RescalePlane *tab = (RescalePlane *)call.h;
    const int ow = dst[0].width, oh = dst[0].height;
    size_t at = 0, most = 1;
    for (int i = 0; i < n; i++) {
        if (!there(i)) continue;
        int32_t w[4];
        resize_window(rs, f, i, w);
        for (int p = 0; p < L.nplanes; p++) {
            RescalePlane &P = tab[at++];
            memset(&P, 0, sizeof P);
            if (on_dev) { P.src = f[i].data[p]; P.ls = f[i].linesize[p]; }
            else call.stage(f[i], p, pix_plane(L.pd, f[i].width, f[i].height, p), &P.src, &P.ls);
            const int k = L.pd->planar ? p : 0;
            const int sw = (k == 1 || k == 2) ? L.pd->log2_chroma_w : 0, sh = (k == 1 || k == 2) ? L.pd->log2_chroma_h : 0;
            P.dst = dst[i].data[p];
            P.dls = dst[i].linesize[p];
            P.ox = (uint32_t)(w[0] >> sw); P.oy = (uint32_t)(w[1] >> sh);
            P.pw = (uint32_t)((w[2] + (1 << sw) - 1) >> sw); P.ph = (uint32_t)((w[3] + (1 << sh) - 1) >> sh);
            P.dw = (uint32_t)pix_comp_w(L.pd, ow, k); P.dh = (uint32_t)pix_comp_h(L.pd, oh, k);
            P.step = (uint32_t)L.step;
            P.pair = (((uintptr_t)P.src | (uint64_t)P.ls) & 1) == 0;
            P.dpair = (((uintptr_t)P.dst | (uint64_t)P.dls) & 1) == 0;
            P.share = c->resize_share ? (uint32_t)c->resize_share - 1 : resize_share((int)P.pw, (int)P.dw, L.step, rs.filter);
            most = std::max(most, (((size_t)P.dw + RS_TW - 1) / RS_TW) * (((size_t)P.dh + RS_TH - 1) / RS_TH));
        }
    }
    RescaleFmt R;
    R.bytes = (uint32_t)L.bytes; R.shift = L.shift; R.mask = L.mask;
    R.filter = (uint32_t)rs.filter;
    R.rows = (uint32_t)(c->resize_rows ? c->resize_rows : RS_ROWS_DEFAULT);
    return call.run(nt, [&](hipStream_t st, const void *d_tab, void *) {
        for (int i = 0; i < n; i++)
            for (int p = 0; p < L.nplanes && !there(i); p++) {
                const PlaneGeo g = pix_plane(L.pd, ow, oh, p);
                HIP_TRY(c, hipMemset2DAsync(dst[i].data[p], (size_t)dst[i].linesize[p], 0, g.rowbytes, (size_t)g.rows, st));
            }
        const RescalePlane *dt = (const RescalePlane *)d_tab;
        const unsigned gx = (unsigned)std::min<size_t>(most, nt >= 64 ? 256 : 2048);      /* as meas_launch, a tile a workgroup */
        for (size_t z0 = 0; z0 < nt; z0 += 65535)
            hipLaunchKernelGGL(k_frame_rescale, dim3(gx, 1, (unsigned)std::min<size_t>(65535, nt - z0)), dim3(CMP_THREADS), 0, st, dt + z0, R);
        return 0;
    });
}

extern "C" int htj2k_resize_frames(htj2k_ctx *c, const htj2k_frame *src, int src_on_device, int n, int bits, const int32_t *windows,
                                   int filter, const htj2k_frame *dst)
{
    if (!src || !dst || n < 1) return HTJ2K_ERR_EINVAL;
    const ResizeArgs rs = { windows, filter, c };
    CmpLayout L;
    const int r = rescale_check(src[0].pix_fmt, bits, src, n, nullptr, rs, dst, &L);
    if (r < 0) return r;
    if (!c) return HTJ2K_ERR_ENOSYS;
    return rescale_run(c, L, src, src_on_device, n, nullptr, rs, dst);
}

/* frames f0 .. f0 + nf - 1 of the job (htj2k_job_resize_frames: all of them; the pipe: one) */
static int job_resize_frames(htj2k_ctx *c, htj2k_job *j, int f0, int nf, int bits, const int32_t *windows, int filter,
                             const htj2k_frame *dst, int *status)
{
    if (!j || !dst || j->nframes < 1 || f0 < 0 || nf < 1 || f0 + nf > j->nframes) return HTJ2K_ERR_EINVAL;
    if (!j->uploaded || !j->run.frames_ok) return HTJ2K_ERR_EINVAL;     /* no run yet, or one that did not write the frames */
    int first = -1;
    for (int f = 0; f < nf && first < 0; f++)
        if (j->frames[f0 + f].plan) first = f0 + f;
    if (first < 0) return HTJ2K_ERR_EINVAL;
    const htj2k_info &I0 = j->frames[first].plan->info;
    if (bits == 0) bits = I0.bits_per_raw_sample;
    std::vector<htj2k_frame> dev((size_t)nf);
    std::vector<uint8_t> skip((size_t)nf, 0);
    for (int f = 0; f < nf; f++) {
        const FrameSlot &F = j->frames[f0 + f];
        if (!F.plan) { skip[f] = 1; continue; }           /* no frame there: zero samples */
        job_frame_view(F, &dev[f]);
    }
    const ResizeArgs rs = { windows, filter, c };
    CmpLayout L;
    int r = rescale_check(I0.pix_fmt, bits, dev.data(), nf, skip.data(), rs, dst, &L);
    if (r < 0) return r;
    if (!c) return HTJ2K_ERR_ENOSYS;
    if ((r = job_settle(c, j)) < 0) return r;              /* waits for the job's stream; the planes are final behind it */
    if ((r = rescale_run(c, L, dev.data(), 1, nf, skip.data(), rs, dst)) < 0) return r;
    for (int f = 0; f < nf && status; f++) status[f] = skip[f];
    return 0;
}

extern "C" int htj2k_job_resize_frames(htj2k_ctx *c, htj2k_job *j, int bits, const int32_t *windows, int filter, const htj2k_frame *dst,
                                       int *status)
{
    return job_resize_frames(c, j, 0, j ? j->nframes : 0, bits, windows, filter, dst, status);
}

/* htj2k_pipe_receive_resized (htj2k_pipe.cpp): frame `frame` of a slot's job as one resized frame */
extern "C" int htj2k_job_frame_resize_(htj2k_ctx *c, htj2k_job *j, int frame, int bits, const int32_t *window, int filter, const htj2k_frame *dst)
{
    return job_resize_frames(c, j, frame, 1, bits, window, filter, dst, nullptr);
}

/* ---- tensors as frames: the definition of htj2k_encode_tensor written out as frames (k_tensor_frame; with a mix, that
 * of htj2k_encode_tensor_mix by k_tensor_frame_mix; with curves, that of htj2k_encode_tensor_curves by
 * k_tensor_frame_curves).  A MeasCall without results and without staged planes: its table holds every plane of every
 * destination frame, and with curves both tables stand behind it */
extern "C" int htj2k_tensor_to_frames_curves(htj2k_ctx *c, const void *src, size_t src_bytes, int n, int bits, const htj2k_tensor_spec *spec,
                                             const htj2k_tensor_mix_in *mix, const htj2k_tensor_curves_in *curves, const htj2k_frame *dst)
{
    if (!src || !spec || !dst || n < 1) return HTJ2K_ERR_EINVAL;
    TensorCall T;
    int r = tensor_spec_check(dst[0].pix_fmt, bits, spec, &T, nullptr, nullptr, mix, nullptr, curves);   /* the layout, bits, dtype and layout, scale and bias or the mix, the curves */
    if (r < 0) return r;
    if (spec->out_w || spec->out_h) return HTJ2K_ERR_EINVAL;       /* no window in this direction */
    const CmpLayout &L = T.L;
    const int w = dst[0].width, h = dst[0].height;
    for (int i = 0; i < n; i++)
        if (dst[i].pix_fmt != dst[0].pix_fmt || dst[i].width != w || dst[i].height != h) return HTJ2K_ERR_EINVAL;
    if (w < 1 || h < 1 || (int64_t)w * L.step * L.bytes > INT32_MAX) return HTJ2K_ERR_EINVAL;
    for (int i = 0; i < n; i++)
        for (int p = 0; p < L.nplanes; p++)
            if (!dst[i].data[p]) return HTJ2K_ERR_EINVAL;
    for (int i = 0; i < n; i++)
        for (int p = 0; p < L.nplanes; p++)
            if (dst[i].linesize[p] < 0 || (size_t)dst[i].linesize[p] < pix_plane(L.pd, w, h, p).rowbytes) return HTJ2K_ERR_EINVAL;
    T.elems = (size_t)T.nout * (size_t)w * (size_t)h;      /* C channels, or the mix's K */
    if (src_bytes / T.esize / T.elems < (size_t)n) return HTJ2K_ERR_EINVAL;
    if ((uintptr_t)src % T.esize) return HTJ2K_ERR_EINVAL;
    if (!c) return HTJ2K_ERR_ENOSYS;

    MeasCall call(c);
    const size_t nt = (size_t)n * L.nplanes;
    std::vector<float> ctab;                               /* with curves: what the kernel gets, and the tables as they are uploaded */
    CurveInFmt Q;
    memset(&Q, 0, sizeof Q);
    if (curves) Q = curve_in_fmt(*curves, T.ncomp, &ctab);
    if ((r = call.reserve(0, 0, nt, mix ? sizeof(MixInPlane) : sizeof(TensorInPlane), ctab.size() * sizeof(float))) < 0) return r;
    if (curves) Q.tab = (const float *)call.put(ctab.data(), ctab.size() * sizeof(float));
    TensorInPlane *tab = (TensorInPlane *)call.h;
    MixInPlane *mtab = (MixInPlane *)call.h;              /* with a mix: the same entries, each with its footprints' rcp_N */
    size_t most = 1;
    for (int i = 0; i < n; i++)
        for (int p = 0; p < L.nplanes; p++) {
            TensorInPlane &P = mix ? mtab[(size_t)i * L.nplanes + p].P : tab[(size_t)i * L.nplanes + p];
            const int k = L.pd->planar ? p : 0;
            memset(&P, 0, sizeof P);
            P.dst = dst[i].data[p];
            P.ls = dst[i].linesize[p];
            P.src_img = (uint64_t)i * T.elems;
            P.comp0 = (uint32_t)k;
            P.step = (uint32_t)L.step;
            P.sw = (k == 1 || k == 2) ? L.pd->log2_chroma_w : 0;
            P.sh = (k == 1 || k == 2) ? L.pd->log2_chroma_h : 0;
            P.pw = (uint32_t)(L.pd->planar ? pix_comp_w(L.pd, w, k) : w);
            P.ph = (uint32_t)(L.pd->planar ? pix_comp_h(L.pd, h, k) : h);
            most = std::max(most, (size_t)P.step * P.pw * P.ph);
            if (mix) {                                     /* 1 / N of a full footprint and of those the last column and row clip */
                const int lastw = w - (int)((P.pw - 1) << P.sw), lasth = h - (int)((P.ph - 1) << P.sh);
                MixInRcp &R = mtab[(size_t)i * L.nplanes + p].rcp;
                for (int cy = 0; cy < 2; cy++)
                    for (int cx = 0; cx < 2; cx++)
                        R.r[cy][cx] = 1.0f / (float)((cx ? lastw : 1 << P.sw) * (cy ? lasth : 1 << P.sh));
            }
        }
    TensorInFmt F;
    memset(&F, 0, sizeof F);
    F.shift = L.shift; F.peak = L.mask;
    F.w = (uint32_t)w; F.h = (uint32_t)h;
    F.ncomp = (uint32_t)T.ncomp; F.bytes = (uint32_t)L.bytes;
    F.nhwc = T.nhwc;
    for (int k = 0; k < 4; k++) { F.scale[k] = T.scale[k]; F.bias[k] = T.bias[k]; }
    MixIn M;
    memset(&M, 0, sizeof M);
    if (mix) {
        M.nin = (uint32_t)mix->nin;
        M.box = mix->chroma == HTJ2K_CHROMA_BOX;
        memcpy(M.m, mix->m, sizeof M.m);
        memcpy(M.b, mix->b, sizeof M.b);
    }
    return call.run(nt, [&](hipStream_t st, const void *d_tab, void *) {
        const TensorInPlane *dt = (const TensorInPlane *)d_tab;
        const uint8_t *in = (const uint8_t *)src;
        if (curves) {                                      /* a workgroup stages the tables first: the grid of the other direction's launches */
            const MixInPlane *mt = (const MixInPlane *)d_tab;
            const size_t lds = ctab.size() * sizeof(float);
            const unsigned gx = curves_grid(c, std::min<size_t>((most + CURVE_IN_THREADS - 1) / CURVE_IN_THREADS, nt >= 64 ? 256 : 2048),
                                            T.elems * T.esize, lds);
            for (size_t z0 = 0; z0 < nt; z0 += 65535) {
                const dim3 grid(gx, 1, (unsigned)std::min<size_t>(65535, nt - z0));
                switch (T.dtype) {
                case HTJ2K_TENSOR_F32:  hipLaunchKernelGGL(k_tensor_frame_curves<TENSOR_F32>, grid, dim3(CURVE_IN_THREADS), lds, st, mt + z0, in, F, M, Q); break;
                case HTJ2K_TENSOR_F16:  hipLaunchKernelGGL(k_tensor_frame_curves<TENSOR_F16>, grid, dim3(CURVE_IN_THREADS), lds, st, mt + z0, in, F, M, Q); break;
                default:                hipLaunchKernelGGL(k_tensor_frame_curves<TENSOR_BF16>, grid, dim3(CURVE_IN_THREADS), lds, st, mt + z0, in, F, M, Q); break;
                }
            }
            return 0;
        }
        if (mix) {
            const MixInPlane *mt = (const MixInPlane *)d_tab;
            switch (T.dtype) {
            case HTJ2K_TENSOR_F32:  meas_launch(k_tensor_frame_mix<TENSOR_F32>, st, mt, nt, most, CMP_THREADS, in, F, M); break;
            case HTJ2K_TENSOR_F16:  meas_launch(k_tensor_frame_mix<TENSOR_F16>, st, mt, nt, most, CMP_THREADS, in, F, M); break;
            default:                meas_launch(k_tensor_frame_mix<TENSOR_BF16>, st, mt, nt, most, CMP_THREADS, in, F, M); break;
            }
            return 0;
        }
        switch (T.dtype) {
        case HTJ2K_TENSOR_F32:  meas_launch(k_tensor_frame<TENSOR_F32>, st, dt, nt, most, CMP_THREADS, in, F); break;
        case HTJ2K_TENSOR_F16:  meas_launch(k_tensor_frame<TENSOR_F16>, st, dt, nt, most, CMP_THREADS, in, F); break;
        default:                meas_launch(k_tensor_frame<TENSOR_BF16>, st, dt, nt, most, CMP_THREADS, in, F); break;
        }
        return 0;
    });
}

extern "C" int htj2k_tensor_to_frames_mix(htj2k_ctx *c, const void *src, size_t src_bytes, int n, int bits, const htj2k_tensor_spec *spec,
                                          const htj2k_tensor_mix_in *mix, const htj2k_frame *dst)
{
    return htj2k_tensor_to_frames_curves(c, src, src_bytes, n, bits, spec, mix, nullptr, dst);
}

extern "C" int htj2k_tensor_to_frames(htj2k_ctx *c, const void *src, size_t src_bytes, int n, int bits, const htj2k_tensor_spec *spec,
                                      const htj2k_frame *dst)
{
    return htj2k_tensor_to_frames_mix(c, src, src_bytes, n, bits, spec, nullptr, dst);
}

/* htj2k_encode_batch_measured (htj2k_encode.hip) decodes the encoder's own streams with the product decoder: they are parsed
 * with the input's layout as the pixel-format request, whatever the context was opened with (its bitexact holds), and run as
 * one job that stays on the device, for htj2k_job_compare.  A block the decoder rejects in such a stream is a bug. */
extern "C" int htj2k_meas_decode_(htj2k_ctx *c, const uint8_t *const *pkts, const int *sizes, int n, int pix_fmt, htj2k_job **job)
{
    if (!c || !job) return HTJ2K_ERR_EINVAL;
    const int req = c->opts.req_pix_fmt;
    c->opts.req_pix_fmt = pix_fmt;
    int r = htj2k_job_parse_batch(c, pkts, sizes, n, &c->meas_job);
    c->opts.req_pix_fmt = req;
    if (r < 0) return r;
    htj2k_job *j = c->meas_job;
    if ((r = htj2k_job_upload(c, j)) < 0 || (r = htj2k_job_run(c, j)) < 0 || (r = htj2k_job_wait(c, j)) < 0) return r;
    if ((r = htj2k_job_block_errors(c, j)) != 0) {
        if (r > 0) clog(c, LOG_ERROR, "measured encode: the decoder rejected %d code-block(s) of the encoder's own stream\n", r);
        return r < 0 ? r : HTJ2K_ERR_BUG;
    }
    *job = j;
    return 0;
}

extern "C" int htj2k_meas_reduction_(const htj2k_ctx *c) { return c ? c->opts.reduction_factor : 0; }

/* ------------------------------------------------------------------ one-call decode */
extern "C" int htj2k_decode(htj2k_ctx *c, const uint8_t *pkt, int size, htj2k_frame *frame, htj2k_stats *stats)
{
    if (!c || !pkt || !frame) return HTJ2K_ERR_EINVAL;
    auto t0 = std::chrono::steady_clock::now();
    int r = htj2k_job_parse(c, pkt, size, &c->own_job);
    if (r < 0) return r;
    auto t1 = std::chrono::steady_clock::now();
    htj2k_job *j = c->own_job;
    if ((r = htj2k_job_upload(c, j)) < 0) return r;
    if ((r = htj2k_job_run(c, j)) < 0) return r;
    auto t2 = std::chrono::steady_clock::now();
    if ((r = htj2k_job_download(c, j, frame)) < 0) return r;
    auto t3 = std::chrono::steady_clock::now();
    int nerr = htj2k_job_block_errors(c, j);
    if (nerr > 0)
        clog(c, LOG_ERROR, "Bad HT cleanup segment in %d codeblock(s)\n", nerr);   /* jpeg2000htdec.c:1305 */
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->n_codeblocks = (int)j->blocks.size();
        stats->n_block_errors = nerr > 0 ? nerr : 0;
        stats->ms_parse = std::chrono::duration<float, std::milli>(t1 - t0).count();
        (void)hipEventElapsedTime(&stats->ms_h2d, j->ev[0], j->ev[1]);
        (void)hipEventElapsedTime(&stats->ms_kernels, j->ev[2], j->ev[5]);
        stats->ms_d2h = std::chrono::duration<float, std::milli>(t3 - t2).count();
        htj2k_job_stage_ms(c, j, &stats->ms_ht, &stats->ms_idwt, &stats->ms_pack);
    }
    return j->frames[0].plan->bytes_consumed;
}

/* ------------------------------------------------------------------ kernel-level entry points */
static void fill_levels(const int border[2][2], int levels, int32_t linelen[][2], uint8_t mod[][2])
{
    int b[2][2], lev = levels;
    for (int i = 0; i < 2; i++) for (int k = 0; k < 2; k++) b[i][k] = border[i][k];
    while (--lev >= 0)
        for (int i = 0; i < 2; i++) {
            linelen[lev][i] = b[i][1] - b[i][0];
            mod[lev][i] = b[i][0] & 1;
            for (int k = 0; k < 2; k++) b[i][k] = (b[i][k] + 1) >> 1;
        }
}

struct PlaneSet {                 /* nplanes identical-geometry planes laid out back to back */
    int w, h, levels, type, nplanes;
    size_t plane_samples;
    std::vector<std::vector<uint8_t>> tables_generic, tables_tile;   /* per level */
    std::vector<int> lh, lv;
    std::vector<uint8_t> fast;        /* per level: stream_fast_geom */
};

static void planeset_build(PlaneSet &P, const int border[2][2], int levels, int type, int nplanes)
{
    P.w = border[0][1] - border[0][0]; P.h = border[1][1] - border[1][0];
    P.levels = levels; P.type = type; P.nplanes = nplanes;
    P.plane_samples = align_up((size_t)P.w * P.h, 64);
    J2kTileComp tc;                    /* what level_args reads of a tile-component */
    memset(&tc, 0, sizeof(tc));
    tc.w = P.w; tc.transform = type; tc.ndeclevels = levels;
    fill_levels(border, levels, tc.linelen, tc.mod);
    for (int lev = 0; lev < levels; lev++) {
        std::vector<uint8_t> tg, tt;
        for (int p = 0; p < nplanes; p++) {
            tc.plane_off = (uint32_t)(p * P.plane_samples);
            const DwtTileArgs a = level_args(tc, lev);
            push_bytes(tg, &a.g, sizeof(a.g));
            push_bytes(tt, &a, sizeof(a));
        }
        P.tables_generic.push_back(tg); P.tables_tile.push_back(tt);
        P.lh.push_back(tc.linelen[lev][0]); P.lv.push_back(tc.linelen[lev][1]);
        P.fast.push_back(stream_fast_geom(level_args(tc, lev).g));
    }
}

template <int TYPE>
static void planeset_launch_level(const PlaneSet &P, int lev, int mode, int kth, const void *d_tab,
                                  uint32_t *coef, uint32_t *t0, uint32_t *t1, hipStream_t s)
{
    if (mode == 0) {
        dim3 g((P.lh[lev] + 255) / 256, P.lv[lev], P.nplanes);
        hipLaunchKernelGGL((k_idwt_h<TYPE>), g, dim3(256), 0, s, (const DwtLevel *)d_tab, (const uint32_t *)coef, t0);
        hipLaunchKernelGGL((k_idwt_v<TYPE>), g, dim3(256), 0, s, (const DwtLevel *)d_tab, (const uint32_t *)t0, coef);
    } else {
        const uint32_t *ll = kth == 0 ? coef : ((kth - 1) & 1) ? t1 : t0;
        uint32_t *out = (kth & 1) ? t1 : t0;
        launch_tile_generic<TYPE>(d_tab, P.lh[lev], P.lv[lev], P.lh[lev] < P.lv[lev] ? P.lh[lev] : P.lv[lev], P.nplanes, mode, s,
                                  ll, (const uint32_t *)coef, out, P.fast[lev] != 0);
    }
}

/* returns which buffer (0 coef, 1 t0, 2 t1) holds the result */
static int planeset_run(const PlaneSet &P, int mode, uint8_t *d_tabs, const std::vector<size_t> &tab_off,
                        uint32_t *coef, uint32_t *t0, uint32_t *t1, hipStream_t s)
{
    int kth = 0;
    for (int lev = 0; lev < P.levels; lev++) {
        if (P.lh[lev] <= 0 || P.lv[lev] <= 0) continue;
        with_dwt_type(P.type, [&](auto T) { planeset_launch_level<decltype(T)::value>(P, lev, mode, kth, d_tabs + tab_off[lev], coef, t0, t1, s); });
        kth++;
    }
    if (mode == 0 || kth == 0) return 0;
    return 1 + ((kth - 1) & 1);
}

static int planeset_upload_tables(htj2k_ctx *c, const PlaneSet &P, int mode, DevBuf &d_tabs, std::vector<size_t> &off)
{
    std::vector<uint8_t> all;
    off.clear();
    for (int lev = 0; lev < P.levels; lev++) {
        const std::vector<uint8_t> &t = mode == 0 ? P.tables_generic[lev] : P.tables_tile[lev];
        off.push_back(desc_append(all, t.data(), t.size()));
    }
    int r = d_tabs.ensure(all.size() + 64);
    if (r < 0) return r;
    if (!all.empty()) HIP_TRY(c, hipMemcpy(d_tabs.p, all.data(), all.size(), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int htj2k_idwt_plane(htj2k_ctx *c, void *plane, const int border[2][2], int levels, int type)
{
    if (!c || !plane || levels < 0 || levels > J2K_MAX_DWTLEV || type < 0 || type > 2) return HTJ2K_ERR_EINVAL;
    if (border[0][1] <= border[0][0] || border[1][1] <= border[1][0]) return HTJ2K_ERR_EINVAL;
    if (levels == 0) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    PlaneSet P;
    planeset_build(P, border, levels, type, 1);
    DevBuf coef, t0, t1, tabs;
    std::vector<size_t> off;
    const size_t bytes = P.plane_samples * 4 + 256;
    int r;
    if ((r = coef.ensure(bytes)) < 0 || (r = t0.ensure(bytes)) < 0 || (r = t1.ensure(bytes)) < 0 ||
        (r = planeset_upload_tables(c, P, c->idwt_mode, tabs, off)) < 0) {
        coef.release(); t0.release(); t1.release(); tabs.release();
        return r;
    }
    hipError_t e = hipMemcpy(coef.p, plane, (size_t)P.w * P.h * 4, hipMemcpyHostToDevice);
    int fb = 0;
    if (e == hipSuccess) {
        fb = planeset_run(P, c->idwt_mode, (uint8_t *)tabs.p, off, (uint32_t *)coef.p, (uint32_t *)t0.p, (uint32_t *)t1.p, 0);
        e = hipDeviceSynchronize();
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpy(plane, fb == 0 ? coef.p : fb == 1 ? t0.p : t1.p, (size_t)P.w * P.h * 4, hipMemcpyDeviceToHost);
    coef.release(); t0.release(); t1.release(); tabs.release();
    if (e != hipSuccess) { clog(c, LOG_ERROR, "HIP error %s in htj2k_idwt_plane\n", hipGetErrorString(e)); return HTJ2K_ERR_EXTERNAL; }
    return 0;
}

__global__ void k_fill_pattern(uint32_t *p, size_t n, int is_float)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t h = (uint32_t)i * 2654435761u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    int v = (int)(h % 511u) - 255;
    p[i] = is_float ? __float_as_uint((float)v * 0.25f) : (uint32_t)v;
}

extern "C" int htj2k_idwt_bench(htj2k_ctx *c, int w, int h, int levels, int type, int nplanes, int iters, float *ms_per_iter)
{
    if (!c || w <= 0 || h <= 0 || levels <= 0 || levels > J2K_MAX_DWTLEV || type < 0 || type > 2 || nplanes <= 0 || iters <= 0 || !ms_per_iter)
        return HTJ2K_ERR_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    const int border[2][2] = { { 0, w }, { 0, h } };
    PlaneSet P;
    planeset_build(P, border, levels, type, nplanes);
    DevBuf coef, t0, t1, tabs;
    std::vector<size_t> off;
    const size_t n = P.plane_samples * nplanes, bytes = n * 4 + 256;
    int r;
    if ((r = coef.ensure(bytes)) < 0 || (r = t0.ensure(bytes)) < 0 || (r = t1.ensure(bytes)) < 0 ||
        (r = planeset_upload_tables(c, P, c->idwt_mode, tabs, off)) < 0) {
        coef.release(); t0.release(); t1.release(); tabs.release();
        return r;
    }
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_fill_pattern, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (uint32_t *)coef.p, n, type == J2K_DWT97);
        planeset_run(P, c->idwt_mode, (uint8_t *)tabs.p, off, (uint32_t *)coef.p, (uint32_t *)t0.p, (uint32_t *)t1.p, s);   /* warm-up */
        e = hipStreamSynchronize(s);
    }
    if (e == hipSuccess) {
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < iters; i++)
            planeset_run(P, c->idwt_mode, (uint8_t *)tabs.p, off, (uint32_t *)coef.p, (uint32_t *)t0.p, (uint32_t *)t1.p, s);
        (void)hipEventRecord(e1, s);
        e = hipStreamSynchronize(s);
    }
    float ms = 0;
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s) (void)hipStreamDestroy(s);
    coef.release(); t0.release(); t1.release(); tabs.release();
    if (e != hipSuccess) { clog(c, LOG_ERROR, "HIP error %s in htj2k_idwt_bench\n", hipGetErrorString(e)); return HTJ2K_ERR_EXTERNAL; }
    *ms_per_iter = ms / iters;
    return 0;
}

/* Calibration for the roofline figures: what a kernel that does nothing but move bytes reaches on THIS device, so
 * that a box whose memory system copies at 5.1 TB/s is not read as a kernel at 0.55 of 8 TB/s.  A grid-stride copy of
 * 16-byte elements, `mbytes` MB read and as many written per launch; the launch shapes of tools/ubench/membw.hip,
 * the best of them is returned (GB/s, read + written). */
__global__ void __launch_bounds__(256) k_copy_linear(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

extern "C" int htj2k_copy_bench(htj2k_ctx *c, int mbytes, int iters, float *gbps)
{
    if (!c || mbytes <= 0 || mbytes > 8192 || iters <= 0 || !gbps) return HTJ2K_ERR_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)mbytes * 1000000 / 16;
    DevBuf src, dst;
    int r;
    if ((r = src.ensure(n * 16)) < 0 || (r = dst.ensure(n * 16)) < 0) { src.release(); dst.release(); return r; }
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipMemsetAsync(src.p, 1, n * 16, s);
    float best = 0;
    const int grids[3] = { 8192, 65536, 262144 };
    for (int g = 0; g < 3 && e == hipSuccess; g++) {
        for (int i = 0; i < 2; i++)
            hipLaunchKernelGGL(k_copy_linear, dim3(grids[g]), dim3(256), 0, s, (const uint4 *)src.p, (uint4 *)dst.p, n);
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < iters; i++)
            hipLaunchKernelGGL(k_copy_linear, dim3(grids[g]), dim3(256), 0, s, (const uint4 *)src.p, (uint4 *)dst.p, n);
        (void)hipEventRecord(e1, s);
        e = hipStreamSynchronize(s);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && ms > 0) best = std::max(best, (float)(2.0 * n * 16 * iters / (ms * 1e-3) / 1e9));
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s) (void)hipStreamDestroy(s);
    src.release(); dst.release();
    if (e != hipSuccess) { clog(c, LOG_ERROR, "HIP error %s in htj2k_copy_bench\n", hipGetErrorString(e)); return HTJ2K_ERR_EXTERNAL; }
    *gbps = best;
    return 0;
}

extern "C" int htj2k_mct_planes(htj2k_ctx *c, void *p0, void *p1, void *p2, int csize, int type)
{
    if (!c || !p0 || !p1 || !p2 || csize <= 0 || type < 0 || type > 2) return HTJ2K_ERR_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf d[3];
    void *h[3] = { p0, p1, p2 };
    int r = 0;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 3 && r >= 0; i++) r = d[i].ensure((size_t)csize * 4);
    for (int i = 0; i < 3 && r >= 0 && e == hipSuccess; i++) e = hipMemcpy(d[i].p, h[i], (size_t)csize * 4, hipMemcpyHostToDevice);
    if (r >= 0 && e == hipSuccess) {
        hipLaunchKernelGGL(k_mct_only, dim3((csize + 255) / 256), dim3(256), 0, 0, (uint32_t *)d[0].p, (uint32_t *)d[1].p, (uint32_t *)d[2].p, csize, type);
        e = hipDeviceSynchronize();
    }
    for (int i = 0; i < 3 && r >= 0 && e == hipSuccess; i++) e = hipMemcpy(h[i], d[i].p, (size_t)csize * 4, hipMemcpyDeviceToHost);
    for (int i = 0; i < 3; i++) d[i].release();
    if (r < 0) return r;
    return e == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

/* HT block decoder alone: decode `n` codeblocks given as a descriptor table + byte pool into
 * a sample buffer (unit parity against ff_jpeg2000_decode_htj2k + dequantisation) */
/* decode_cblk() + dequantisation on a caller-built table of Part-1 blocks: every descriptor carries J2K_BLK_PART1 and
 * its bytes are laid out as j2k_plan.c does it (j2k_plan.h: segments, 0xFF 0xFF terminators, J2kPart1Trailer) */
/* A caller-built descriptor (the unit entry points below) gets the guarantees the job path has from the host parser:
 * the block is at most 4096 samples and 1024 in either direction (jpeg2000htdec.c:1230-1232, what the kernels' LDS and
 * quad-symbol sizing assume), its window lies inside the coefficient buffer, the numbers the kernels shift by are in
 * range. */
static bool block_desc_ok(const J2kBlock &b, size_t nsamples)
{
    if (!b.w || !b.h || b.w > 1024 || b.h > 1024 || (uint32_t)b.w * b.h > 4096 || b.stride < b.w) return false;
    if ((size_t)b.plane_off + (size_t)(b.h - 1) * b.stride + b.w > nsamples) return false;
    if (b.roi_shift > 30 || b.npasses >= 100) return false;
    return true;
}

/* The unit entry points run the block stage as a job does, with the jobs' launchers, on the null stream and between
 * synchronous copies: the tables, the re-packed pool and the caller's samples in; the samples and the blocks' status out */
static int unit_run(htj2k_ctx *c, const char *who, const J2kBlock *blocks, const uint8_t *pool, const BlockLayout &L, const HtChoice &k,
                    unsigned nwide, void *coef, int *status)
{
    BlockBufs B;
    const int r = block_bufs_ensure(B, L);
    hipError_t e = hipSuccess;
    if (r == 0) {
        e = block_tables_upload(B, blocks, L, 0);
        if (e == hipSuccess) e = hipMemcpy(B.d_bytes.p, pool, L.nbytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(B.d_coef.p, coef, L.nsamples * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(B.d_status.p, 0, (size_t)L.n * sizeof(int));
        if (e == hipSuccess && L.n > L.nht) e = launch_mq_blocks(0, B, L, nwide);
        if (e == hipSuccess && L.nht) e = launch_ht_blocks(0, c->d_tables, B, L, k);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(coef, B.d_coef.p, L.nsamples * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && status) e = hipMemcpy(status, B.d_status.p, (size_t)L.n * sizeof(int), hipMemcpyDeviceToHost);
    }
    B.release();
    if (r < 0) return r;
    if (e != hipSuccess) { clog(c, LOG_ERROR, "HIP error %s in %s\n", hipGetErrorString(e), who); return HTJ2K_ERR_EXTERNAL; }
    return 0;
}

/* raw: the descriptors go to the kernel with J2K_DWT_RAW for a transform (the transcoder's stores) */
static int mq_blocks(htj2k_ctx *c, const void *blocks_in, int nblocks, const uint8_t *bytes_in, size_t nbytes_in,
                     void *coef, size_t nsamples, int *status, bool raw)
{
    if (!c || !blocks_in || nblocks <= 0 || !bytes_in || !coef) return HTJ2K_ERR_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<J2kBlock> blk((const J2kBlock *)blocks_in, (const J2kBlock *)blocks_in + nblocks);
    std::vector<uint8_t> pool(16, 0);
    for (int i = 0; i < nblocks; i++) {
        J2kBlock &b = blk[i];
        if (!(b.flags & J2K_BLK_PART1) || !block_desc_ok(b, nsamples) || b.M_b > 37) return HTJ2K_ERR_EINVAL;
        if (raw) {
            if (b.M_b > 31 || b.roi_shift) return HTJ2K_ERR_EINVAL;
            b.flags |= J2K_DWT_RAW;
        }
        const size_t len = J2K_P1_TRAILER_OFF(b.lcup) + 4 + 2 * (size_t)b.lref;
        if ((size_t)b.data_off + len > nbytes_in) return HTJ2K_ERR_EINVAL;
        {   /* the trailer is trusted by the kernel: segment count and starts must lie inside the block's bytes */
            const J2kPart1Trailer *tr = (const J2kPart1Trailer *)(bytes_in + b.data_off + J2K_P1_TRAILER_OFF(b.lcup));
            if (tr->nterm != b.lref || tr->bandpos > 3) return HTJ2K_ERR_EINVAL;
            for (uint32_t k = 0; k < tr->nterm; k++)
                if (tr->start[k] > b.lcup) return HTJ2K_ERR_EINVAL;
        }
        const size_t o = pool.size();
        pool.resize(o + J2K_P1_REGION(b.lcup, b.lref), 0);
        memcpy(pool.data() + o, bytes_in + b.data_off, len);
        b.data_off = (uint32_t)o;
    }
    pool.resize(pool.size() + 256, 0);
    BlockLayout L;
    int r = block_layout(blk.data(), 0, nblocks, pool.size(), nsamples, L);
    if (r < 0) return r;
    /* the blocks stay in the caller's order, so one kernel takes all waves: the wide one if any block is wider than 64 columns */
    unsigned nwide = 0;
    for (const MqWave &W : L.mqwaves)
        if (W.chunks > 1) nwide = (unsigned)L.mqwaves.size();
    return unit_run(c, "htj2k_mq_blocks", blk.data(), pool.data(), L, HtChoice(), nwide, coef, status);
}

extern "C" int htj2k_mq_blocks(htj2k_ctx *c, const void *blocks_in, int nblocks, const uint8_t *bytes_in, size_t nbytes_in,
                               void *coef, size_t nsamples, int *status)
{
    return mq_blocks(c, blocks_in, nblocks, bytes_in, nbytes_in, coef, nsamples, status, false);
}

extern "C" int htj2k_mq_blocks_raw(htj2k_ctx *c, const void *blocks_in, int nblocks, const uint8_t *bytes_in, size_t nbytes_in,
                                   void *coef, size_t nsamples, int *status)
{
    return mq_blocks(c, blocks_in, nblocks, bytes_in, nbytes_in, coef, nsamples, status, true);
}

/* ------------------------------------------------------------------ the transcoder's sources (j2k_enc.h)
 * htj2k_transcode_batch (htj2k_encode.hip) parses its sources into a job of this context, looks at the parsers and
 * plans (j2k_xc.c), and then runs the block stage with raw stores: every descriptor, Part-1 or HT, gets J2K_DWT_RAW
 * before the upload, and the job runs the RAW instantiations of the HT kernels.  The planes stay in the job's coefficient buffer, from where the encoder's stream fetches them. */
extern "C" int htj2k_xc_device_(const htj2k_ctx *c) { return c ? c->device : -1; }

extern "C" int htj2k_xc_parse_(htj2k_ctx *c, const uint8_t *const *pkts, const int *sizes, int n, htj2k_log_fn log, void *opaque)
{
    if (!c) return HTJ2K_ERR_EINVAL;
    if (c->opts.reduction_factor) {
        if (log) log(opaque, LOG_ERROR, "transcode: a reduction factor on the decoder drops resolutions the output must keep\n");
        return HTJ2K_ERR_PATCHWELCOME;
    }
    /* the sources are parsed as htj2k_transcode_check parses them: no pixel format asked for, whatever the context was
     * opened with (the output keeps the source's components as they are) */
    const int req = c->opts.req_pix_fmt;
    c->opts.req_pix_fmt = HTJ2K_PIX_NONE;
    c->xc_log = log;
    c->xc_log_opaque = opaque;
    const int r = htj2k_job_parse_batch(c, pkts, sizes, n, &c->xc_job);
    c->xc_log = nullptr;
    c->opts.req_pix_fmt = req;
    return r;
}

extern "C" const J2kParser *htj2k_xc_parser_(htj2k_ctx *c, int f)
{
    return c && c->xc_job && f >= 0 && f < c->xc_job->nframes ? c->xc_job->frames[f].parser : nullptr;
}

extern "C" const J2kPlan *htj2k_xc_plan_(htj2k_ctx *c, int f)
{
    return c && c->xc_job && f >= 0 && f < c->xc_job->nframes ? c->xc_job->frames[f].plan : nullptr;
}

extern "C" int htj2k_xc_run_(htj2k_ctx *c, void **event, float *ms)
{
    htj2k_job *j = c ? c->xc_job : nullptr;
    if (!j || j->nframes <= 0 || j->uploaded) return HTJ2K_ERR_EINVAL;
    for (J2kBlock &b : j->blocks)
        b.flags |= J2K_DWT_RAW;
    j->raw = true;
    int r = htj2k_job_upload(c, j);
    if (r < 0) return r;
    if ((r = htj2k_job_run_stages(c, j, 1)) < 0) return r;
    if (event) *event = (void *)j->ev[3];
    const int bad = htj2k_job_block_errors(c, j);          /* waits for the job's stream */
    if (bad >= 0 && ms) (void)htj2k_job_stage_ms(c, j, ms, nullptr, nullptr);
    return bad;
}

extern "C" const int32_t *htj2k_xc_plane_(htj2k_ctx *c, int f, int t)
{
    htj2k_job *j = c ? c->xc_job : nullptr;
    if (!j || f < 0 || f >= j->nframes || t < 0 || t >= j->frames[f].plan->ntilecomps || !(j->run.ran & 1)) return nullptr;
    return (const int32_t *)j->d_coef.p + j->tilecomps[j->frames[f].tc_base + (size_t)t].plane_off;
}

/* raw: the descriptors go to the RAW instantiations of the kernels with J2K_DWT_RAW for a transform (the transcoder's stores) */
static int ht_blocks(htj2k_ctx *c, const void *blocks_in, int nblocks, const uint8_t *bytes_in, size_t nbytes_in,
                     void *coef, size_t nsamples, int *status, bool raw)
{
    if (!c || !blocks_in || nblocks <= 0 || !bytes_in || !coef) return HTJ2K_ERR_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    /* the kernels want the layout j2k_plan.c produces: every block's bytes at a 16-byte aligned
     * offset, J2K_BLOCK_PAD bytes behind them and 16 in front of the first: re-pack the caller's pool */
    std::vector<J2kBlock> blk((const J2kBlock *)blocks_in, (const J2kBlock *)blocks_in + nblocks);
    std::vector<uint8_t> pool(16, 0);
    for (int i = 0; i < nblocks; i++) {
        J2kBlock &b = blk[i];
        const size_t len = (size_t)b.lcup + b.lref;
        if ((b.flags & J2K_BLK_PART1) || !block_desc_ok(b, nsamples) || b.M_b > 30) return HTJ2K_ERR_EINVAL;
        if (raw) {
            if (b.M_b > 31 || b.roi_shift) return HTJ2K_ERR_EINVAL;
            b.flags |= J2K_DWT_RAW;
        }
        if ((size_t)b.data_off + len > nbytes_in) return HTJ2K_ERR_EINVAL;
        const size_t o = pool.size();
        pool.resize(o + J2K_BLOCK_REGION(len), 0);
        memcpy(pool.data() + o, bytes_in + b.data_off, len);
        b.data_off = (uint32_t)o;
    }
    BlockLayout L;
    int r = build_ht_lds(c, blk.data(), nblocks, pool.data(), &L.lds, &L.lds_ext);
    if (r < 0 || (r = block_layout(blk.data(), nblocks, nblocks, pool.size(), nsamples, L)) < 0) return r;
    HtChoice k;
    if (c->unit_ht == 0) {
        /* a fixed choice that keeps the plain kernels exercised: k_ht_vlc, one block per wave in the un-stuffing kernel,
         * k_ht_decode<true> with 32-bit stores */
        k.extended = c->ht_mode == 1 && ht_vlc_lds_bytes(L.lds.max_qw) <= 160 * 1024;
        k.unstuff_g = unstuff_group(1);
        k.raw = raw;
    } else {
        /* the knob unit_ht: what a job that holds exactly these blocks launches on one of its routes, and no kernel on a
         * block that a job could not hand it -- a table that the route's conditions exclude is refused here, before
         * anything is uploaded (the transcoder's jobs never have 16-bit sub-bands: no raw table on routes 3 and 4) */
        const HtRoutes R = ht_block_routes(blk.data(), (size_t)nblocks, L);
        k = ht_choice_front(c, L.lds.max_qw, raw);
        if (c->unit_ht == 2) {
            if (!k.extended || !R.multi_nb) return HTJ2K_ERR_EINVAL;
            k.magsgn = HtChoice::MULTI;
            k.bpw = R.multi_nb;
            k.multi_t = R.multi_t;
        } else if (c->unit_ht == 3 || c->unit_ht == 4) {
            if (!k.extended || raw || !R.coef16 || (c->unit_ht == 3 && !R.pair)) return HTJ2K_ERR_EINVAL;
            k.coef16 = true;
            if (c->unit_ht == 3) {
                k.magsgn = HtChoice::PAIR;
                k.bpw = 2;
            }
        }
    }
    return unit_run(c, "htj2k_ht_blocks", blk.data(), pool.data(), L, k, 0, coef, status);
}

extern "C" int htj2k_ht_blocks(htj2k_ctx *c, const void *blocks_in, int nblocks, const uint8_t *bytes_in, size_t nbytes_in,
                               void *coef, size_t nsamples, int *status)
{
    return ht_blocks(c, blocks_in, nblocks, bytes_in, nbytes_in, coef, nsamples, status, false);
}

extern "C" int htj2k_ht_blocks_raw(htj2k_ctx *c, const void *blocks_in, int nblocks, const uint8_t *bytes_in, size_t nbytes_in,
                                   void *coef, size_t nsamples, int *status)
{
    return ht_blocks(c, blocks_in, nblocks, bytes_in, nbytes_in, coef, nsamples, status, true);
}
