/*
 * htj2k_encode.hip -- device layer of the HTJ2K encoder: the htj2k_enc_* entry points of
 * include/htj2k_amd.h that need a GPU.
 *
 * htj2k_encode_batch checks every frame of the call before anything runs, then encodes the frames in
 * rounds of at most ENC_ROUND_SAMPLES samples (HTJ2K_ENC_ROUND in the environment of htj2k_enc_open:
 * fewer, for tests; a round takes at least one frame).  A round is a `Round` and encode_round the list
 * of its stages; every device stage is one launch over the round's frames (descriptor tables, as the
 * decoder's jobs):
 *
 *   layout -> unpack (upload, k_enc_unpack; htj2k_encode_tensor: k_enc_unpack_tensor reads the float tensor) -> block table -> transform (k_fdwt*; 9/7: then, in calls with a PSNR target,
 *   k_rc_base97 over the float planes, and k_quant97, int32 indices in the float planes) -> select (budgeted calls:
 *   k_rc_stats, k_rc_select; calls with a PSNR target: k_rc_stats, k_rc_select_q) -> code
 *   (k_ht_encode, read-back; calls with ht_passes > 1: k_ht_refine_plan before it, k_ht_refine_encode behind it)
 *   -> cap (calls with a PSNR target and a budget: the frames beyond the budget start again as budgeted frames)
 *   -> enforce (budgeted calls: exact sizes, correction launches, last resort; a budget over the group: the same on the
 *   sum, round_enforce_group)
 *   -> headers (j2k_enc.c) -> gather (k_enc_gather, D2H)
 *
 * htj2k_transcode_batch feeds the same rounds from Part-1 codestreams: the decoder context parses the sources and runs its
 * block stage with raw stores (htj2k_xc_*_, htj2k_device.hip), j2k_xc.c checks the scope and applies the block rule, and
 * a round is
 *
 *   layout -> fetch (k_xc_scatter: the decoder's tile-component planes into the component planes; the block table with
 *   the rule's plane and passes) -> code (k_ht_refine_plan, k_ht_encode, k_ht_refine_encode) -> enforce (calls with a
 *   budget, htj2k_transcode_opts: frames beyond it get the statistics at every block's base plane, k_rc_stats<true>,
 *   k_rc_stats_passes<true>, k_xc_limit, round_xc_stats; then the budgeted frames' correction launches) -> headers -> gather
 *
 * htj2k_encode_batch_measured is encode_batch, then the decoder context decodes the streams as a job of its own
 * (htj2k_meas_decode_, htj2k_device.hip) and htj2k_job_compare measures them against the input; with close_loop the
 * frames that measure short are encoded again, each with a target of its own (encode_batch's `quality`).
 *
 * Rate control on the host, behind the first launch: rc_select_again and group_select_again select again (rc_rescale,
 * rc_fetch_selection), rc_collect and rc_code_again code the blocks that changed, and rc_last_resort leaves blocks out,
 * for one frame against its target or for all frames against the group's (the choice itself: enc_drop_take, j2k_enc.c;
 * the candidates' distortion: BlockDist, which frame_model_d reads too).  The unit entry points over caller-given blocks
 * begin with UnitCall.
 *
 * Every way out of a round, and of the unit entry points, waits for the stream first (StreamWait).
 * Built with -ffp-contract=off: the float stages must round as the vector factory does.  The kernels
 * are in enc_kernels.hpp.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include <utility>
#include <vector>
#include "j2k_plan.h"
#include "j2k_enc.h"
#include "enc_kernels.hpp"

using namespace htj2k_enc;

#define ENC_ROUND_SAMPLES ((size_t)1 << 30)    /* samples of all components of the frames of one round */
#define ENC_MAX_LEVELS    32
#define UNPACK_ROWS       65535                /* rows one entry of k_enc_unpack's table covers: what grid.y takes */
#define ENC_CURVES_SRC_PER_TABLE 2             /* the unpack stage with curves; measured at 1, 2, 4, 8, 16: DESIGN.md 3.5, "Transfer curves on the way in" */
#define RC_MAX_LAUNCHES   3                    /* HT cleanup launches a budgeted round of frames may take */

/* the events of a round, by what has been enqueued when they are recorded; EV_T0 and EV_T1 bracket one span at a
 * time: those of rate control, then the gather's (EV_T0 to EV_GATHERED) */
enum { EV_START, EV_UNPACKED, EV_TRANSFORMED, EV_CODED, EV_GATHERED, EV_SELECTED, EV_T0, EV_T1, EV_PLANNED, EV_REFINED, EV_STATS2,
       EV_BASE0, EV_BASE1, EV_G0, EV_G1, ENC_EVENTS };

struct DevBuf {                                /* device memory that only grows; freed with its owner */
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    ~DevBuf() { (void)hipFree(p); }
    int ensure(size_t n)
    {
        if (n <= cap)
            return 0;
        (void)hipFree(p);
        n = (n + 0xFFFF) & ~(size_t)0xFFFF;
        cap = hipMalloc(&p, n) == hipSuccess ? n : 0;
        if (!cap)
            p = nullptr;
        return cap ? 0 : HTJ2K_ERR_ENOMEM;
    }
};

struct RcBufs {                                /* rate control on the device */
    DevBuf dist, len, dskip, low, kmax;        /* k_rc_stats' outputs: S points into them */
    DevBuf w, scale, frames;                   /* k_rc_select's inputs */
    DevBuf planes, sel_len, sel;               /* and outputs */
    DevBuf blk2, res2;                         /* launch table and results of a correction launch (sized by the round) */
    DevBuf dist2, dist3, spbits, mrbits, passes;   /* calls that ask for passes: k_rc_stats_passes' outputs, k_rc_select's passes */
    DevBuf step, base, qframes, qual;              /* calls with a PSNR target: k_rc_base97's input and output, k_rc_select_q's frames and results */
    DevBuf chunks, gframes, floors, partial, aux, fsum, group, which;   /* a budget over a group: the k_rc_group_* kernels' */
    DevBuf xbase, xpass;                           /* transcoding with a budget: per block the base plane and the source's passes */
    int ensure_xc(int nblk)
    {
        return xbase.ensure(((size_t)nblk + 1) * 4) < 0 || xpass.ensure(((size_t)nblk + 1) * 4) < 0 ? HTJ2K_ERR_ENOMEM : 0;
    }
    RcStats S = {};
    RcPassStats P = {};
    int ensure_group(size_t nchunks, size_t nf)
    {
        if (chunks.ensure((nchunks + 1) * sizeof(RcChunk)) < 0 || gframes.ensure((nf + 1) * sizeof(RcGFrame)) < 0 ||
            floors.ensure((nf + 1) * 8) < 0 || partial.ensure((nchunks + 1) * RC_GROUP_SLOTS * 8) < 0 ||
            aux.ensure((nchunks + 1) * sizeof(RcGroupAux)) < 0 || fsum.ensure((nf + 1) * RC_GROUP_SLOTS * 8) < 0 ||
            group.ensure(sizeof(RcGroup)) < 0 || which.ensure((nf + 1) * 4) < 0)
            return HTJ2K_ERR_ENOMEM;
        return 0;
    }
    int ensure(int nblk, int nf, bool multi, bool quality = false)
    {
        const size_t n = (size_t)nblk + 1;
        if (quality && (step.ensure(n * 4) < 0 || base.ensure(n * 8) < 0 || qframes.ensure((size_t)(nf + 1) * sizeof(RcQFrame)) < 0 ||
                        qual.ensure((size_t)(nf + 1) * sizeof(RcQual)) < 0))
            return HTJ2K_ERR_ENOMEM;
        if (multi) {
            if (dist2.ensure(n * RC_PLANES * 8) < 0 || dist3.ensure(n * RC_PLANES * 8) < 0 || spbits.ensure(n * RC_PLANES * 4) < 0 ||
                mrbits.ensure(n * RC_PLANES * 4) < 0 || passes.ensure(n * 4) < 0)
                return HTJ2K_ERR_ENOMEM;
            P = { (uint64_t *)dist2.p, (uint64_t *)dist3.p, (uint32_t *)spbits.p, (uint32_t *)mrbits.p };
        }
        if (dist.ensure(n * RC_PLANES * 8) < 0 || len.ensure(n * RC_PLANES * 4) < 0 || dskip.ensure(n * 8) < 0 ||
            low.ensure(n * 4) < 0 || kmax.ensure(n * 4) < 0 || w.ensure(n * 8) < 0 || scale.ensure(n * 8) < 0 ||
            planes.ensure(n * 4) < 0 || sel_len.ensure(n * 4) < 0 ||
            frames.ensure((size_t)(nf + 1) * sizeof(RcFrame)) < 0 || sel.ensure((size_t)(nf + 1) * sizeof(RcSel)) < 0)
            return HTJ2K_ERR_ENOMEM;
        S = { (uint64_t *)dist.p, (uint32_t *)len.p, (double *)dskip.p, (uint32_t *)low.p, (int32_t *)kmax.p };
        return 0;
    }
};

struct htj2k_enc_ctx {
    int device = 0;
    int max_dyn_lds = 64 * 1024;
    htj2k_log_fn log = nullptr;
    void *log_opaque = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[ENC_EVENTS] = {};
    float ms[4] = { 0, 0, 0, 0 };
    float rc_ms[3] = { 0, 0, 0 };      /* k_rc_stats, k_rc_select, the HT launches of the correction rounds */
    float q_ms[2] = { 0, 0 };          /* k_rc_base97; the runs of k_rc_select_q */
    float ref_ms[2] = { 0, 0 };        /* k_ht_refine_plan + k_ht_refine_encode of the first launch; k_rc_stats_passes */
    std::vector<std::vector<int>> last_planes, last_passes;   /* of the last batch, per frame */
    std::vector<htj2k_enc_rc> last_rc;
    std::vector<htj2k_enc_quality> last_q;
    int measure_ssim = 0;              /* htj2k_enc_measure_ssim */
    std::vector<htj2k_frame_ssim> last_ssim;   /* of the last call when it was a measured one with the switch on, else empty */
    htj2k_enc_group last_group = {};
    float group_ms = 0;                /* the k_rc_group_* kernels, all their runs */
    RcGroup group_init = {};           /* what a queued copy reads: the state a group selection starts from */
    int stamps = 0;                    /* HTJ2K_ENC_STAMPS=1: k_ht_encode records the clock at its phase boundaries */
    size_t round_samples = ENC_ROUND_SAMPLES;   /* HTJ2K_ENC_ROUND=n: samples per round (tests: several rounds of small frames) */
    size_t curves_grid = ENC_CURVES_SRC_PER_TABLE;   /* HTJ2K_ENC_CURVES_GRID=n: tensor bytes a workgroup of the unpack stage with curves reads, in table bytes */
    uint64_t cycles[ENC_STAMPS - 1] = { 0, 0, 0, 0, 0 };
    uint64_t stamped = 0;
    uint64_t ref_cycles[REF_STAMPS - 1] = { 0, 0, 0, 0, 0, 0 };   /* the same of k_ht_refine_encode, behind them in c->st */
    uint64_t ref_stamped = 0;
    uint16_t *d_tab = nullptr;
    DevBuf in, coef, tmp, pool, args, blk, res, lit, pieces, out, st;
    DevBuf curve_tab;                  /* a call with curves: both tables, as every workgroup stages them */
    DevBuf xc;                         /* transcoding: k_xc_scatter's table */
    float xc_ms = 0;                   /* ... and the device time of the decoder's block stage in the last call */
    int rounds = 0;                    /* rounds the last batch call took */
    RcBufs rc;
};

static void enc_log(void *opaque, int level, const char *msg)
{
    htj2k_enc_ctx *c = (htj2k_enc_ctx *)opaque;
    if (c && c->log)
        c->log(c->log_opaque, level, msg);
}

#define HIP_OK(x) do { if ((x) != hipSuccess) return HTJ2K_ERR_EXTERNAL; } while (0)
#define ENC_OK(x) do { const int r_ = (x); if (r_ < 0) return r_; } while (0)

/* Declared behind the host memory that queued copies read or write, so that it goes first: whichever way the scope is
 * left, the stream is idle before that memory goes and the caller has its buffers back.  Success ends in sync(). */
struct StreamWait {
    hipStream_t stream;
    bool pending = true;
    ~StreamWait() { if (pending) (void)hipStreamSynchronize(stream); }
    int sync() { pending = false; return hipStreamSynchronize(stream) == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL; }
};

extern "C" int htj2k_enc_open(int device_id, htj2k_enc_ctx **out)
{
    int n = 0;
    hipDeviceProp_t prop;
    *out = nullptr;
    if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n)
        return HTJ2K_ERR_ENOSYS;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return HTJ2K_ERR_ENOSYS;
    htj2k_enc_ctx *c = new htj2k_enc_ctx;
    c->device = device_id;
    c->max_dyn_lds = (int)prop.sharedMemPerBlock;
    const char *e = getenv("HTJ2K_ENC_STAMPS");
    c->stamps = e && atoi(e) > 0;
    e = getenv("HTJ2K_ENC_ROUND");
    if (e && atoll(e) > 0 && (unsigned long long)atoll(e) < ENC_ROUND_SAMPLES)
        c->round_samples = (size_t)atoll(e);
    e = getenv("HTJ2K_ENC_CURVES_GRID");
    if (e && atoll(e) > 0 && atoll(e) <= 4096)
        c->curves_grid = (size_t)atoll(e);
    uint16_t tab[2 * 8 * 16 * 16];
    enc_cxtvlc_table(tab);
    bool ok = hipSetDevice(device_id) == hipSuccess &&
              hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc(&c->d_tab, sizeof tab) == hipSuccess &&
              hipMemcpy(c->d_tab, tab, sizeof tab, hipMemcpyHostToDevice) == hipSuccess;
    for (int i = 0; ok && i < ENC_EVENTS; i++)
        ok = hipEventCreate(&c->ev[i]) == hipSuccess;
    if (!ok) {
        htj2k_enc_close(c);
        return HTJ2K_ERR_ENOSYS;
    }
    *out = c;
    return 0;
}

extern "C" void htj2k_enc_close(htj2k_enc_ctx *c)
{
    if (!c)
        return;
    (void)hipSetDevice(c->device);
    if (c->stream)
        (void)hipStreamSynchronize(c->stream);
    for (int i = 0; i < ENC_EVENTS; i++)
        if (c->ev[i])
            (void)hipEventDestroy(c->ev[i]);
    (void)hipFree(c->d_tab);
    if (c->stream)
        (void)hipStreamDestroy(c->stream);
    delete c;                                          /* every DevBuf frees its memory */
}

extern "C" void htj2k_enc_set_log(htj2k_enc_ctx *c, htj2k_log_fn fn, void *opaque)
{
    c->log = fn;
    c->log_opaque = opaque;
}

extern "C" int htj2k_enc_stage_ms(htj2k_enc_ctx *c, float ms[4])
{
    memcpy(ms, c->ms, sizeof c->ms);
    return 0;
}

extern "C" int htj2k_enc_rc_stage_ms(htj2k_enc_ctx *c, float ms[3])
{
    memcpy(ms, c->rc_ms, sizeof c->rc_ms);
    return 0;
}

extern "C" int htj2k_enc_ref_stage_ms(htj2k_enc_ctx *c, float ms[2])
{
    memcpy(ms, c->ref_ms, sizeof c->ref_ms);
    return 0;
}

static int last_ints(const std::vector<std::vector<int>> &all, int frame, int *dst, int cap)
{
    if (frame < 0 || (size_t)frame >= all.size())
        return HTJ2K_ERR_EINVAL;
    const std::vector<int> &v = all[(size_t)frame];
    for (int i = 0; dst && i < cap && (size_t)i < v.size(); i++)
        dst[i] = v[(size_t)i];
    return (int)v.size();
}

extern "C" int htj2k_enc_last_passes(htj2k_enc_ctx *c, int frame, int *passes, int cap)
{
    return c ? last_ints(c->last_passes, frame, passes, cap) : HTJ2K_ERR_EINVAL;
}

extern "C" int htj2k_enc_last_planes(htj2k_enc_ctx *c, int frame, int *planes, int cap)
{
    return c ? last_ints(c->last_planes, frame, planes, cap) : HTJ2K_ERR_EINVAL;
}

extern "C" int htj2k_enc_rc_info(htj2k_enc_ctx *c, int frame, htj2k_enc_rc *info)
{
    if (!c || !info || frame < 0 || (size_t)frame >= c->last_rc.size())
        return HTJ2K_ERR_EINVAL;
    *info = c->last_rc[(size_t)frame];
    return 0;
}

extern "C" int htj2k_enc_group_info(htj2k_enc_ctx *c, htj2k_enc_group *info)
{
    if (!c || !info)
        return HTJ2K_ERR_EINVAL;
    *info = c->last_group;
    return 0;
}

extern "C" int htj2k_enc_group_stage_ms(htj2k_enc_ctx *c, float *ms)
{
    if (!c || !ms)
        return HTJ2K_ERR_EINVAL;
    *ms = c->group_ms;
    return 0;
}

extern "C" int htj2k_enc_quality_info(htj2k_enc_ctx *c, int frame, htj2k_enc_quality *info)
{
    if (!c || !info || frame < 0 || (size_t)frame >= c->last_q.size())
        return HTJ2K_ERR_EINVAL;
    *info = c->last_q[(size_t)frame];
    return 0;
}

extern "C" int htj2k_enc_measure_ssim(htj2k_enc_ctx *c, int on)
{
    if (!c || on < 0 || on > 1)
        return HTJ2K_ERR_EINVAL;
    c->measure_ssim = on;
    return 0;
}

extern "C" int htj2k_enc_last_ssim(htj2k_enc_ctx *c, int frame, htj2k_frame_ssim *out)
{
    if (!c || !out || frame < 0 || (size_t)frame >= c->last_ssim.size())
        return HTJ2K_ERR_EINVAL;
    *out = c->last_ssim[(size_t)frame];
    return 0;
}

extern "C" int htj2k_enc_quality_stage_ms(htj2k_enc_ctx *c, float ms[2])
{
    if (!c || !ms)
        return HTJ2K_ERR_EINVAL;
    memcpy(ms, c->q_ms, sizeof c->q_ms);
    return 0;
}

extern "C" int htj2k_enc_ht_cycles(htj2k_enc_ctx *c, uint64_t cycles[5])
{
    memcpy(cycles, c->cycles, sizeof c->cycles);
    return (int)(c->stamped > INT32_MAX ? INT32_MAX : c->stamped);
}

extern "C" int htj2k_enc_ref_cycles(htj2k_enc_ctx *c, uint64_t cycles[6])
{
    memcpy(cycles, c->ref_cycles, sizeof c->ref_cycles);
    return (int)(c->ref_stamped > INT32_MAX ? INT32_MAX : c->ref_stamped);
}

/* calls launch(z0, nz) for the n entries of a table in chunks of what grid.z takes */
template <typename Launch>
static void for_z_chunks(size_t n, Launch launch)
{
    for (size_t z0 = 0; z0 < n; z0 += 65535)
        launch(z0, (unsigned)std::min(n - z0, (size_t)65535));
}

/* one tile-component to transform: its first sample in the plane and in the scratch plane (row stride `stride`), its
 * rectangle x0 .. x1 - 1, y0 .. y1 - 1 in tile-component coordinates, its levels */
struct DwtRegion {
    int32_t *p, *t;
    int32_t stride, x0, y0, x1, y1, levels;
};

static int32_t ceil_shift(int32_t v, int l) { return (int32_t)(((int64_t)v + ((int64_t)1 << l) - 1) >> l); }

/* the forward DWT of `regions` (in place, scratch alongside), one launch per level and direction over all of them, the
 * grid as large as the level's largest entry needs; the launch tables go to c->args from byte `args_off` on (the
 * caller has sized it for the sum of the regions' levels) through `tab`, which the caller keeps until the stream is
 * synchronised */
static int run_fdwt(htj2k_enc_ctx *c, const std::vector<DwtRegion> &regions, size_t args_off, std::vector<DwtPlane> &tab,
                    bool irrev)
{
    int maxl = 0;
    for (const DwtRegion &r : regions)
        maxl = std::max(maxl, r.levels);
    tab.clear();
    std::vector<size_t> off, cnt;
    std::vector<int> gx, gy;
    for (int l = 0; l < maxl; l++) {
        int mw = 0, mh = 0;
        off.push_back(tab.size());
        for (const DwtRegion &r : regions) {
            if (l >= r.levels)
                continue;
            const int32_t x0 = ceil_shift(r.x0, l), y0 = ceil_shift(r.y0, l);
            const DwtPlane d = { r.p, r.t, r.stride, ceil_shift(r.x1, l) - x0, ceil_shift(r.y1, l) - y0, x0 & 1, y0 & 1 };
            if (d.lw < 1 || d.lh < 1)
                continue;                             /* no samples left at this level */
            if (d.lw == 1 && d.lh == 1 && !d.px && !d.py && !irrev)
                continue;                             /* one sample at an even position: 5/3 leaves it as it is (at an odd
                                                       * one it doubles it; 9/7 scales it either way, every level) */
            tab.push_back(d);
            mw = d.lw > mw ? d.lw : mw;
            mh = d.lh > mh ? d.lh : mh;
        }
        cnt.push_back(tab.size() - off.back());
        gx.push_back((mw + 255) / 256);
        gy.push_back(mh);
    }
    if (tab.empty())
        return 0;
    if (args_off + tab.size() * sizeof(DwtPlane) > c->args.cap)
        return HTJ2K_ERR_BUG;
    DwtPlane *d_tab = (DwtPlane *)((uint8_t *)c->args.p + args_off);
    HIP_OK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(DwtPlane), hipMemcpyHostToDevice, c->stream));
    for (int l = 0; l < maxl; l++)
        for_z_chunks(cnt[l], [&](size_t z0, unsigned nz) {
            const dim3 grid((unsigned)gx[l], (unsigned)gy[l], nz);
            hipLaunchKernelGGL(irrev ? k_fdwt97_v : k_fdwt_v, grid, dim3(256), 0, c->stream, d_tab + off[l] + z0);
            hipLaunchKernelGGL(irrev ? k_fdwt97_h : k_fdwt_h, grid, dim3(256), 0, c->stream, d_tab + off[l] + z0);
        });
    return hipGetLastError() == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

/* c->st must hold nblk * ENC_STAMPS words when c->stamps is set (sized with the other buffers, before any launch) */
static int run_ht(htj2k_enc_ctx *c, const EncBlk *d_blk, int nblk, EncRes *d_res)
{
    if (ENC_LDS_BYTES > c->max_dyn_lds) {
        enc_log(c, 16, "encoder: the HT kernel needs more LDS than a workgroup may have\n");
        return HTJ2K_ERR_PATCHWELCOME;
    }
    uint64_t *st = c->stamps ? (uint64_t *)c->st.p : nullptr;
    if (st)
        HIP_OK(hipMemsetAsync(st, 0, (size_t)nblk * ENC_STAMPS * sizeof(uint64_t), c->stream));
    if (nblk > 0)
        hipLaunchKernelGGL(k_ht_encode, dim3((unsigned)nblk), dim3(64), ENC_LDS_BYTES, c->stream, d_blk,
                           (const int32_t *)c->coef.p, (uint8_t *)c->pool.p, d_res, (const uint16_t *)c->d_tab, st);
    return hipGetLastError() == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

/* blocks that ask for passes: before run_ht, which of them fall back to one (the table gets the cleanup planes) */
static int run_refine_plan(htj2k_enc_ctx *c, EncBlk *d_blk, int nblk, EncRes *d_res)
{
    if (nblk > 0)
        hipLaunchKernelGGL(k_ht_refine_plan, dim3((unsigned)nblk), dim3(64), 0, c->stream, d_blk, (const int32_t *)c->coef.p, d_res);
    return hipGetLastError() == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

/* and behind run_ht: the refinement segments (their stamps behind run_ht's in c->st) */
static int run_refine(htj2k_enc_ctx *c, const EncBlk *d_blk, int nblk, EncRes *d_res)
{
    uint64_t *st = c->stamps ? (uint64_t *)c->st.p + (size_t)nblk * ENC_STAMPS : nullptr;
    if (st)
        HIP_OK(hipMemsetAsync(st, 0, (size_t)nblk * REF_STAMPS * sizeof(uint64_t), c->stream));
    if (nblk > 0)
        hipLaunchKernelGGL(k_ht_refine_encode, dim3((unsigned)nblk), dim3(64), 0, c->stream, d_blk, (const int32_t *)c->coef.p,
                           (uint8_t *)c->pool.p, d_res, st);
    return hipGetLastError() == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

/* `base` (transcoding with a budget): per block the plane the statistics start at; null: plane 0, the encoder's tables */
static int run_rc_stats(htj2k_enc_ctx *c, int nblk, int nplanes, const int32_t *base = nullptr)
{
    if (nblk > 0)
        hipLaunchKernelGGL(base ? k_rc_stats<true> : k_rc_stats<false>, dim3((unsigned)nblk), dim3(64), 0, c->stream,
                           (const EncBlk *)c->blk.p, (const int32_t *)c->coef.p, (const uint16_t *)c->d_tab, nplanes, c->rc.S, base);
    return hipGetLastError() == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

static int run_rc_stats_passes(htj2k_enc_ctx *c, int nblk, int nplanes, const int32_t *base = nullptr)
{
    if (nblk > 0)
        hipLaunchKernelGGL(base ? k_rc_stats_passes<true> : k_rc_stats_passes<false>, dim3((unsigned)nblk), dim3(64), 0, c->stream,
                           (const EncBlk *)c->blk.p, (const int32_t *)c->coef.p, nplanes, c->rc.P, base);
    return hipGetLastError() == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

/* behind both, with the bases: what the source's passes (c->rc.xpass) allow at the base plane, and every block's own form
 * into c->rc.planes, c->rc.passes, c->rc.sel_len */
static int run_xc_limit(htj2k_enc_ctx *c, int nblk)
{
    if (nblk > 0)
        hipLaunchKernelGGL(k_xc_limit, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, c->stream, nblk,
                           (const int32_t *)c->rc.xpass.p, c->rc.S, c->rc.P, (int32_t *)c->rc.planes.p, (int32_t *)c->rc.passes.p,
                           (uint32_t *)c->rc.sel_len.p);
    return hipGetLastError() == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

/* the first `nframes` entries of c->rc.frames: planes (and, maxpass > 1, passes) into c->blk, c->rc.planes,
 * c->rc.passes, c->rc.sel_len, c->rc.sel */
static int run_rc_select(htj2k_enc_ctx *c, size_t nframes, int maxpass)
{
    hipLaunchKernelGGL(k_rc_select, dim3((unsigned)nframes), dim3(RC_THREADS), 0, c->stream, (const RcFrame *)c->rc.frames.p,
                       c->rc.S, maxpass > 1 ? c->rc.P : RcPassStats(), maxpass, (const double *)c->rc.w.p,
                       (const double *)c->rc.scale.p, (EncBlk *)c->blk.p, (int32_t *)c->rc.planes.p,
                       (int32_t *)c->rc.passes.p, (uint32_t *)c->rc.sel_len.p, (RcSel *)c->rc.sel.p);
    return hipGetLastError() == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

/* the chunk table of a group: frame f has nblk[f] blocks from blk0[f] on; every chunk lies inside one frame */
static void group_chunks(const int *blk0, const int *nblk, int nf, std::vector<RcChunk> &chunks, std::vector<RcGFrame> &gf)
{
    chunks.clear();
    gf.clear();
    for (int f = 0; f < nf; f++) {
        gf.push_back(RcGFrame{ (int32_t)chunks.size(), (nblk[f] + RC_GROUP_CHUNK - 1) / RC_GROUP_CHUNK });
        for (int i = 0; i < nblk[f]; i += RC_GROUP_CHUNK)
            chunks.push_back(RcChunk{ blk0[f] + i, std::min(RC_GROUP_CHUNK, nblk[f] - i), f, 0 });
    }
}

/* the group selection over the tables in c->rc (chunks, gframes, floors; S, P, w, scale): planes and passes as
 * run_rc_select leaves them, per frame c->rc.sel, the result in c->rc.group.  Every launch is enqueued here; the bracket
 * moves on the device.  EV_G0 and EV_G1 bracket the kernels */
static int run_rc_group(htj2k_enc_ctx *c, size_t nchunks, int nframes, int maxpass, int64_t room, int allow_trial)
{
    c->group_init = RcGroup{};
    c->group_init.room = room;
    c->group_init.allow_trial = allow_trial;
    RcGroup *G = (RcGroup *)c->rc.group.p;
    const RcChunk *ch = (const RcChunk *)c->rc.chunks.p;
    const RcGFrame *gf = (const RcGFrame *)c->rc.gframes.p;
    const double *fl = (const double *)c->rc.floors.p, *w = (const double *)c->rc.w.p, *sc = (const double *)c->rc.scale.p;
    uint64_t *partial = (uint64_t *)c->rc.partial.p, *fsum = (uint64_t *)c->rc.fsum.p;
    RcGroupAux *aux = (RcGroupAux *)c->rc.aux.p;
    const RcPassStats P = maxpass > 1 ? c->rc.P : RcPassStats();
    HIP_OK(hipMemcpyAsync(G, &c->group_init, sizeof(RcGroup), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->ev[EV_G0], c->stream));
    for (int sweep = 0; sweep <= (RC_STEPS + RC_GROUP_LEVELS - 1) / RC_GROUP_LEVELS; sweep++) {
        hipLaunchKernelGGL(k_rc_group_sweep, dim3((unsigned)nchunks), dim3(RC_GROUP_CHUNK), 0, c->stream, (const RcGroup *)G, ch, fl,
                           c->rc.S, P, maxpass, w, sc, sweep == 0, partial, aux);
        hipLaunchKernelGGL(k_rc_group_step, dim3(1), dim3(RC_THREADS), 0, c->stream, G, gf, nframes, (int)nchunks, fl,
                           (const uint64_t *)partial, (const RcGroupAux *)aux, fsum, sweep == 0 ? RC_GROUP_INIT : RC_GROUP_STEP,
                           (RcSel *)c->rc.sel.p);
    }
    hipLaunchKernelGGL(k_rc_group_apply, dim3((unsigned)nchunks), dim3(RC_GROUP_CHUNK), 0, c->stream, (const RcGroup *)G, ch, fl,
                       c->rc.S, P, maxpass, w, sc, (EncBlk *)c->blk.p, (int32_t *)c->rc.planes.p, (int32_t *)c->rc.passes.p,
                       (uint32_t *)c->rc.sel_len.p, partial);
    hipLaunchKernelGGL(k_rc_group_step, dim3(1), dim3(RC_THREADS), 0, c->stream, G, gf, nframes, (int)nchunks, fl,
                       (const uint64_t *)partial, (const RcGroupAux *)aux, fsum, RC_GROUP_FINISH, (RcSel *)c->rc.sel.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(c->ev[EV_G1], c->stream));
    return 0;
}

/* the floors of the `n` frames run_rc_select has just selected (entry j: frame which[j]; null: frame j) */
static int run_rc_group_floors(htj2k_enc_ctx *c, const int32_t *d_which, int n)
{
    if (n > 0)
        hipLaunchKernelGGL(k_rc_group_floors, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const RcSel *)c->rc.sel.p,
                           d_which, n, (double *)c->rc.floors.p);
    return hipGetLastError() == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

/* blocks of the table `d_blk` over the float coefficients, before the quantiser: base_b into c->rc.base */
static int run_rc_base(htj2k_enc_ctx *c, const EncBlk *d_blk, int nblk)
{
    if (nblk > 0)
        hipLaunchKernelGGL(k_rc_base97, dim3((unsigned)nblk), dim3(64), 0, c->stream, d_blk, (const float *)c->coef.p,
                           (const float *)c->rc.step.p, (double *)c->rc.base.p);
    return hipGetLastError() == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

/* the first `nframes` entries of c->rc.qframes: as run_rc_select, on the distortion; per frame also c->rc.qual */
static int run_rc_select_q(htj2k_enc_ctx *c, size_t nframes, int maxpass, bool irrev)
{
    hipLaunchKernelGGL(k_rc_select_q, dim3((unsigned)nframes), dim3(RC_THREADS), 0, c->stream, (const RcQFrame *)c->rc.qframes.p,
                       c->rc.S, maxpass > 1 ? c->rc.P : RcPassStats(), maxpass, (const double *)c->rc.w.p,
                       (const double *)c->rc.scale.p, irrev ? (const double *)c->rc.base.p : nullptr, (EncBlk *)c->blk.p,
                       (int32_t *)c->rc.planes.p, (int32_t *)c->rc.passes.p, (uint32_t *)c->rc.sel_len.p, (RcSel *)c->rc.sel.p,
                       (RcQual *)c->rc.qual.p);
    return hipGetLastError() == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
}

/* after the stream is synchronised: the phase cycles of the last k_ht_encode, summed over the coded blocks, and with
 * `refined` those of the k_ht_refine_encode behind it, summed over the blocks that got a Dref */
static int collect_stamps(htj2k_enc_ctx *c, int nblk, bool refined)
{
    if (!c->stamps || nblk <= 0)
        return 0;
    std::vector<uint64_t> v((size_t)nblk * (ENC_STAMPS + (refined ? REF_STAMPS : 0)));
    HIP_OK(hipMemcpy(v.data(), c->st.p, v.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < nblk; i++) {
        const uint64_t *t = &v[(size_t)i * ENC_STAMPS];
        if (!t[ENC_STAMPS - 1])
            continue;                                  /* all-zero block: left before the phases */
        for (int k = 0; k < ENC_STAMPS - 1; k++)
            c->cycles[k] += t[k + 1] - t[k];
        c->stamped++;
    }
    for (int i = 0; refined && i < nblk; i++) {
        const uint64_t *t = &v[(size_t)nblk * ENC_STAMPS + (size_t)i * REF_STAMPS];
        if (!t[REF_STAMPS - 1])
            continue;                                  /* a block of one pass */
        for (int k = 0; k < REF_STAMPS - 1; k++)
            c->ref_cycles[k] += t[k + 1] - t[k];
        c->ref_stamped++;
    }
    return 0;
}

static int ensure_stamps(htj2k_enc_ctx *c, int nblk)
{
    return c->stamps ? c->st.ensure((size_t)(nblk + 1) * (ENC_STAMPS + REF_STAMPS) * sizeof(uint64_t)) : 0;
}

static int check_coded(htj2k_enc_ctx *c, const EncRes *res, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (res[i].lcup < 0) {
            enc_log(c, 16, "encoder: a code-block could not be coded (MEL + VLC beyond 4079 bytes)\n");
            return HTJ2K_ERR_BUG;
        }
    return 0;
}

static float ev_ms(hipEvent_t a, hipEvent_t b)
{
    float t = 0;
    return hipEventElapsedTime(&t, a, b) == hipSuccess ? t : 0.0f;
}

/* regions of one plane of 4-byte samples through the forward DWT and back */
extern "C" int htj2k_fdwt_regions(htj2k_enc_ctx *c, void *plane, int plane_w, int plane_h, const htj2k_enc_region *regions,
                                  int nregions, int irreversible)
{
    if (!c || !plane || plane_w < 1 || plane_h < 1 || nregions < 1 || !regions)
        return HTJ2K_ERR_EINVAL;
    size_t nlev = 0;
    for (int i = 0; i < nregions; i++) {
        const htj2k_enc_region &r = regions[i];
        if (r.w < 1 || r.h < 1 || r.w > 32768 || r.h > 32768 || r.px < 0 || r.py < 0 || r.px > plane_w - r.w ||
            r.py > plane_h - r.h || r.x0 < 0 || r.y0 < 0 || r.x0 > INT32_MAX - r.w || r.y0 > INT32_MAX - r.h ||
            r.levels < 0 || r.levels > ENC_MAX_LEVELS)
            return HTJ2K_ERR_EINVAL;
        nlev += (size_t)r.levels;
    }
    HIP_OK(hipSetDevice(c->device));
    const size_t n = (size_t)plane_w * plane_h;
    if (c->coef.ensure(n * 4) < 0 || c->tmp.ensure(n * 4) < 0 || c->args.ensure((nlev + 1) * sizeof(DwtPlane)) < 0)
        return HTJ2K_ERR_ENOMEM;
    std::vector<DwtRegion> rg;
    for (int i = 0; i < nregions; i++) {
        const htj2k_enc_region &r = regions[i];
        const size_t at = (size_t)r.py * plane_w + r.px;
        rg.push_back(DwtRegion{ (int32_t *)c->coef.p + at, (int32_t *)c->tmp.p + at, plane_w, r.x0, r.y0, r.x0 + r.w,
                                r.y0 + r.h, r.levels });
    }
    std::vector<DwtPlane> tab;
    StreamWait wait{ c->stream };
    HIP_OK(hipMemcpyAsync(c->coef.p, plane, n * 4, hipMemcpyHostToDevice, c->stream));
    ENC_OK(run_fdwt(c, rg, 0, tab, irreversible != 0));
    HIP_OK(hipMemcpyAsync(plane, c->coef.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    return wait.sync();
}

/* one whole plane: a region at origin 0 */
static int fdwt_plane(htj2k_enc_ctx *c, void *plane, int w, int h, int levels, bool irrev)
{
    const htj2k_enc_region all = { 0, 0, w, h, 0, 0, levels };
    return htj2k_fdwt_regions(c, plane, w, h, &all, 1, irrev);
}

extern "C" int htj2k_fdwt_plane(htj2k_enc_ctx *c, int32_t *plane, int w, int h, int levels)
{
    return fdwt_plane(c, plane, w, h, levels, false);
}

extern "C" int htj2k_fdwt97_plane(htj2k_enc_ctx *c, float *plane, int w, int h, int levels)
{
    return fdwt_plane(c, plane, w, h, levels, true);
}

/* a block's region of the pool; one that asks for passes has room for its refinement segment too */
static size_t region(int w, int h, int passes)
{
    return (enc_block_bound(w, h) + (passes > 1 ? enc_refine_bound(w, h) : 0) + 15) & ~(size_t)15;
}

/* the launch-table entry of a w x h block at sample `coef` of its plane; its region of the pool starts at *at, which moves on */
static EncBlk enc_blk(uint64_t coef, int stride, int w, int h, int plane, int passes, size_t *at)
{
    const EncBlk e = { coef, *at, stride, (uint16_t)w, (uint16_t)h, plane, passes };
    *at += region(w, h, passes);
    return e;
}

/* the launch table of caller-given blocks of one plane; what k_ht_encode's and k_rc_stats' LDS hold: ENC_MAX_QUADS
 * quads, 4096 samples (every T.800 block size, clipped or not) */
static int block_table(const htj2k_enc_block *blocks, int nblocks, int plane_w, int plane_h, const int *planes, const int *passes,
                       std::vector<EncBlk> &tab, size_t *offsets, size_t *total)
{
    size_t at = 0;
    tab.assign((size_t)nblocks + 1, EncBlk());
    for (int i = 0; i < nblocks; i++) {
        const htj2k_enc_block &b = blocks[i];
        if (b.w < 1 || b.h < 1 || b.w > 1024 || b.h > 1024 || b.w * b.h > 4096 ||
            ((b.w + 1) >> 1) * ((b.h + 1) >> 1) > ENC_MAX_QUADS || b.x < 0 || b.y < 0 ||
            b.x + b.w > plane_w || b.y + b.h > plane_h || (planes && (planes[i] < 0 || planes[i] > 31)) ||
            (passes && (passes[i] < 1 || passes[i] > 3 || (passes[i] > 1 && planes && planes[i] > 30))))
            return HTJ2K_ERR_EINVAL;
        if (offsets)
            offsets[i] = at;
        tab[i] = enc_blk((uint64_t)b.y * plane_w + b.x, plane_w, b.w, b.h, planes ? planes[i] : 0, passes ? passes[i] : 1, &at);
    }
    if (offsets)
        offsets[nblocks] = at;
    *total = at;
    return 0;
}

/* What the unit entry points over caller-given blocks of one plane begin with.  begin() refuses in this order: EINVAL
 * (the plane, `args_ok`: the caller's own arguments, the blocks), ENOSPC (`cap`, where the call returns the blocks'
 * bytes), ENOSYS (no context); then -> 0: an empty call with nothing to do (`empty_ok`), or 1: the device is set and
 * c->coef and c->blk hold the plane and the table.  upload() queues both, so it goes behind the caller's StreamWait */
struct UnitCall {
    std::vector<EncBlk> tab;
    size_t samples = 0, pool = 0;                      /* of the plane; bytes of the blocks' regions */
    int nblocks = 0;
    int begin(htj2k_enc_ctx *c, bool args_ok, const void *coef, int plane_w, int plane_h, const htj2k_enc_block *blocks, int n,
              const int *planes, const int *passes, size_t *offsets, const size_t *cap, bool empty_ok)
    {
        if (!coef || plane_w < 1 || plane_h < 1 || n < 0 || (n && !blocks) || !args_ok ||
            block_table(blocks, n, plane_w, plane_h, planes, passes, tab, offsets, &pool) < 0)
            return HTJ2K_ERR_EINVAL;
        if (cap && pool > *cap)
            return HTJ2K_ERR_ENOSPC;
        if (!c)
            return HTJ2K_ERR_ENOSYS;                   /* the arguments are fine; there is no device to run on */
        if (!n && empty_ok)
            return 0;
        HIP_OK(hipSetDevice(c->device));
        nblocks = n;
        samples = (size_t)plane_w * plane_h;
        if (c->coef.ensure(samples * 4) < 0 || c->blk.ensure(tab.size() * sizeof(EncBlk)) < 0)
            return HTJ2K_ERR_ENOMEM;
        return 1;
    }
    int upload(htj2k_enc_ctx *c, const void *coef) const
    {
        HIP_OK(hipMemcpyAsync(c->coef.p, coef, samples * 4, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(c->blk.p, tab.data(), (size_t)nblocks * sizeof(EncBlk), hipMemcpyHostToDevice, c->stream));
        return 0;
    }
};

extern "C" int htj2k_ht_encode_blocks(htj2k_enc_ctx *c, const int32_t *coef, int plane_w, int plane_h,
                                      const htj2k_enc_block *blocks, int nblocks, uint8_t *out, size_t cap,
                                      size_t *offsets, int *lcup, int *max_u)
{
    return htj2k_ht_encode_blocks_planes(c, coef, plane_w, plane_h, blocks, nblocks, nullptr, out, cap, offsets, lcup, max_u);
}

extern "C" int htj2k_ht_encode_blocks_planes(htj2k_enc_ctx *c, const int32_t *coef, int plane_w, int plane_h,
                                             const htj2k_enc_block *blocks, int nblocks, const int *planes, uint8_t *out,
                                             size_t cap, size_t *offsets, int *lcup, int *max_u)
{
    return htj2k_ht_encode_blocks_passes(c, coef, plane_w, plane_h, blocks, nblocks, planes, nullptr, out, cap, offsets, lcup,
                                         nullptr, max_u);
}

extern "C" int htj2k_ht_encode_blocks_passes(htj2k_enc_ctx *c, const int32_t *coef, int plane_w, int plane_h,
                                             const htj2k_enc_block *blocks, int nblocks, const int *planes, const int *passes,
                                             uint8_t *out, size_t cap, size_t *offsets, int *lcup, int *lref, int *max_u)
{
    UnitCall u;
    const int go = u.begin(c, !nblocks || (offsets && lcup && max_u && (!passes || lref)), coef, plane_w, plane_h, blocks, nblocks,
                           planes, passes, offsets, &cap, false);
    if (go < 0)
        return go;
    const size_t at = u.pool;
    if (c->res.ensure(u.tab.size() * sizeof(EncRes)) < 0 || c->pool.ensure(at + 16) < 0 || ensure_stamps(c, nblocks) < 0)
        return HTJ2K_ERR_ENOMEM;
    std::vector<EncRes> res((size_t)nblocks + 1);
    StreamWait wait{ c->stream };
    ENC_OK(u.upload(c, coef));
    if (passes)
        ENC_OK(run_refine_plan(c, (EncBlk *)c->blk.p, nblocks, (EncRes *)c->res.p));
    ENC_OK(run_ht(c, (const EncBlk *)c->blk.p, nblocks, (EncRes *)c->res.p));
    if (passes)
        ENC_OK(run_refine(c, (const EncBlk *)c->blk.p, nblocks, (EncRes *)c->res.p));
    HIP_OK(hipMemcpyAsync(res.data(), c->res.p, (size_t)nblocks * sizeof(EncRes), hipMemcpyDeviceToHost, c->stream));
    if (at)
        HIP_OK(hipMemcpyAsync(out, c->pool.p, at, hipMemcpyDeviceToHost, c->stream));
    ENC_OK(wait.sync());
    memset(c->cycles, 0, sizeof c->cycles);
    c->stamped = 0;
    memset(c->ref_cycles, 0, sizeof c->ref_cycles);
    c->ref_stamped = 0;
    ENC_OK(collect_stamps(c, nblocks, passes != nullptr));
    int r = 0;
    for (int i = 0; i < nblocks; i++) {
        lcup[i] = res[i].lcup;
        max_u[i] = res[i].max_u;
        if (lref)
            lref[i] = passes ? res[i].lref : 0;
        if (res[i].lcup < 0)
            r = HTJ2K_ERR_BUG;
    }
    return r;
}

extern "C" int htj2k_enc_rc_stats(htj2k_enc_ctx *c, const int32_t *coef, int plane_w, int plane_h,
                                  const htj2k_enc_block *blocks, int nblocks, int nplanes, uint64_t *dist, uint32_t *len_est)
{
    UnitCall u;
    const int go = u.begin(c, nplanes >= 1 && nplanes <= RC_PLANES && (!nblocks || (dist && len_est)), coef, plane_w, plane_h,
                           blocks, nblocks, nullptr, nullptr, nullptr, nullptr, true);
    if (go <= 0)
        return go;
    if (c->rc.ensure(nblocks, 1, false) < 0)
        return HTJ2K_ERR_ENOMEM;
    std::vector<uint64_t> d((size_t)nblocks * RC_PLANES);
    std::vector<uint32_t> l((size_t)nblocks * RC_PLANES);
    StreamWait wait{ c->stream };
    ENC_OK(u.upload(c, coef));
    ENC_OK(run_rc_stats(c, nblocks, nplanes));
    HIP_OK(hipMemcpyAsync(d.data(), c->rc.S.dist, d.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(l.data(), c->rc.S.len, l.size() * 4, hipMemcpyDeviceToHost, c->stream));
    ENC_OK(wait.sync());
    for (int i = 0; i < nblocks; i++)
        for (int p = 0; p < nplanes; p++) {
            dist[(size_t)i * nplanes + p] = d[(size_t)i * RC_PLANES + p];
            len_est[(size_t)i * nplanes + p] = l[(size_t)i * RC_PLANES + p];
        }
    return 0;
}

extern "C" int htj2k_enc_rc_stats_passes(htj2k_enc_ctx *c, const int32_t *coef, int plane_w, int plane_h,
                                         const htj2k_enc_block *blocks, int nblocks, int nplanes, uint64_t *dist2, uint64_t *dist3,
                                         uint32_t *sp_bits, uint32_t *mr_bits)
{
    UnitCall u;
    const int go = u.begin(c, nplanes >= 1 && nplanes <= RC_PLANES && (!nblocks || (dist2 && dist3 && sp_bits && mr_bits)), coef,
                           plane_w, plane_h, blocks, nblocks, nullptr, nullptr, nullptr, nullptr, true);
    if (go <= 0)
        return go;
    const size_t rows = (size_t)nblocks * RC_PLANES;
    if (c->rc.ensure(nblocks, 1, true) < 0)
        return HTJ2K_ERR_ENOMEM;
    std::vector<uint64_t> d2(rows), d3(rows);
    std::vector<uint32_t> sp(rows), mr(rows);
    StreamWait wait{ c->stream };
    ENC_OK(u.upload(c, coef));
    ENC_OK(run_rc_stats_passes(c, nblocks, nplanes));
    HIP_OK(hipMemcpyAsync(d2.data(), c->rc.P.dist2, rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(d3.data(), c->rc.P.dist3, rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(sp.data(), c->rc.P.spbits, rows * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(mr.data(), c->rc.P.mrbits, rows * 4, hipMemcpyDeviceToHost, c->stream));
    ENC_OK(wait.sync());
    for (int i = 0; i < nblocks; i++)
        for (int p = 0; p < nplanes; p++) {
            const size_t to = (size_t)i * nplanes + p, from = (size_t)i * RC_PLANES + p;
            dist2[to] = d2[from];
            dist3[to] = d3[from];
            sp_bits[to] = sp[from];
            mr_bits[to] = mr[from];
        }
    return 0;
}

/* the tables of a budgeted transcode over caller-given blocks: both statistics at the blocks' bases, then k_xc_limit */
extern "C" int htj2k_xc_rc_tables(htj2k_enc_ctx *c, const int32_t *coef, int plane_w, int plane_h, const htj2k_enc_block *blocks,
                                  int nblocks, const int *src_plane, const int *src_passes, int nplanes, uint64_t *dist,
                                  uint32_t *len_est, uint64_t *dist2, uint64_t *dist3, uint32_t *sp_bits, uint32_t *mr_bits,
                                  uint32_t *own_len)
{
    bool ok = nplanes >= 2 && nplanes <= RC_PLANES && nblocks >= 0 &&
              (!nblocks || (src_plane && src_passes && dist && len_est && dist2 && dist3 && sp_bits && mr_bits && own_len));
    for (int i = 0; ok && i < nblocks; i++)
        ok = src_plane[i] >= 0 && src_plane[i] <= 30 && src_passes[i] >= 1 && src_passes[i] <= 3;
    UnitCall u;
    const int go = u.begin(c, ok, coef, plane_w, plane_h, blocks, nblocks, nullptr, nullptr, nullptr, nullptr, true);
    if (go <= 0)
        return go;
    const size_t rows = (size_t)nblocks * RC_PLANES;
    if (c->rc.ensure(nblocks, 1, true) < 0 || c->rc.ensure_xc(nblocks) < 0)
        return HTJ2K_ERR_ENOMEM;
    std::vector<uint64_t> d(rows), d2(rows), d3(rows);
    std::vector<uint32_t> l(rows), sp(rows), mr(rows);
    const std::vector<int32_t> base(src_plane, src_plane + nblocks), pass(src_passes, src_passes + nblocks);
    StreamWait wait{ c->stream };
    ENC_OK(u.upload(c, coef));
    HIP_OK(hipMemcpyAsync(c->rc.xbase.p, base.data(), (size_t)nblocks * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.xpass.p, pass.data(), (size_t)nblocks * 4, hipMemcpyHostToDevice, c->stream));
    ENC_OK(run_rc_stats(c, nblocks, RC_PLANES, (const int32_t *)c->rc.xbase.p));
    ENC_OK(run_rc_stats_passes(c, nblocks, RC_PLANES, (const int32_t *)c->rc.xbase.p));
    ENC_OK(run_xc_limit(c, nblocks));
    HIP_OK(hipMemcpyAsync(d.data(), c->rc.S.dist, rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(l.data(), c->rc.S.len, rows * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(d2.data(), c->rc.P.dist2, rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(d3.data(), c->rc.P.dist3, rows * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(sp.data(), c->rc.P.spbits, rows * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(mr.data(), c->rc.P.mrbits, rows * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(own_len, c->rc.sel_len.p, (size_t)nblocks * 4, hipMemcpyDeviceToHost, c->stream));
    ENC_OK(wait.sync());
    for (int i = 0; i < nblocks; i++)
        for (int p = 0; p < nplanes; p++) {
            const size_t to = (size_t)i * nplanes + p, from = (size_t)i * RC_PLANES + p;
            dist[to] = d[from];
            len_est[to] = l[from];
            dist2[to] = d2[from];
            dist3[to] = d3[from];
            sp_bits[to] = sp[from];
            mr_bits[to] = mr[from];
        }
    return 0;
}

extern "C" int htj2k_enc_rc_base(htj2k_enc_ctx *c, const float *coef, int plane_w, int plane_h, const htj2k_enc_block *blocks,
                                 int nblocks, const float *step, double *base)
{
    bool steps_ok = nblocks <= 0 || (step && base);
    for (int i = 0; steps_ok && i < nblocks; i++)
        steps_ok = step[i] > 0 && !(step[i] > 3.0e38f);
    UnitCall u;
    const int go = u.begin(c, steps_ok, coef, plane_w, plane_h, blocks, nblocks, nullptr, nullptr, nullptr, nullptr, true);
    if (go <= 0)
        return go;
    if (c->rc.ensure(nblocks, 1, false, true) < 0)
        return HTJ2K_ERR_ENOMEM;
    StreamWait wait{ c->stream };
    ENC_OK(u.upload(c, coef));
    HIP_OK(hipMemcpyAsync(c->rc.step.p, step, (size_t)nblocks * 4, hipMemcpyHostToDevice, c->stream));
    ENC_OK(run_rc_base(c, (const EncBlk *)c->blk.p, nblocks));
    HIP_OK(hipMemcpyAsync(base, c->rc.base.p, (size_t)nblocks * 8, hipMemcpyDeviceToHost, c->stream));
    return wait.sync();
}

extern "C" int htj2k_enc_rc_group_select(htj2k_enc_ctx *c, int nframes, const int *nblk, const int *kmax, const uint64_t *dist,
                                         const uint32_t *len, const double *dskip, const uint32_t *low0, const double *weight,
                                         const double *scale, const double *floor, int64_t room, int allow_trial,
                                         int32_t *planes, double *lambda, uint64_t *est, int *trial)
{
    if (nframes < 1 || !nblk || !kmax || !dist || !len || !dskip || !low0 || !weight || !planes || !lambda || !est || !trial || room < 0)
        return HTJ2K_ERR_EINVAL;
    size_t n = 0;
    std::vector<int> blk0((size_t)nframes);
    for (int f = 0; f < nframes; f++) {
        if (nblk[f] < 1 || n + (size_t)nblk[f] > ((size_t)1 << 24) || (floor && !(floor[f] >= 0 && std::isfinite(floor[f]))))
            return HTJ2K_ERR_EINVAL;
        blk0[(size_t)f] = (int)n;
        n += (size_t)nblk[f];
    }
    for (size_t b = 0; b < n; b++)
        if (kmax[b] < 0 || kmax[b] > RC_PLANES || !(dskip[b] >= 0 && std::isfinite(dskip[b])) ||
            !(weight[b] >= 0 && std::isfinite(weight[b])) || (scale && !(scale[b] >= 0 && std::isfinite(scale[b]))))
            return HTJ2K_ERR_EINVAL;
    if (!c)
        return HTJ2K_ERR_ENOSYS;
    HIP_OK(hipSetDevice(c->device));
    std::vector<RcChunk> chunks;
    std::vector<RcGFrame> gf;
    group_chunks(blk0.data(), nblk, nframes, chunks, gf);
    if (c->rc.ensure((int)n, nframes, false) < 0 || c->rc.ensure_group(chunks.size(), (size_t)nframes) < 0 ||
        c->blk.ensure((n + 1) * sizeof(EncBlk)) < 0)
        return HTJ2K_ERR_ENOMEM;
    const std::vector<double> ones(scale ? 0 : n, 1.0), zeros(floor ? 0 : (size_t)nframes, 0.0);
    RcGroup G = {};
    StreamWait wait{ c->stream };
    HIP_OK(hipMemcpyAsync(c->rc.S.kmax, kmax, n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.S.dist, dist, n * RC_PLANES * 8, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.S.len, len, n * RC_PLANES * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.S.dskip, dskip, n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.S.low0, low0, n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.w.p, weight, n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.scale.p, scale ? scale : ones.data(), n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.floors.p, floor ? floor : zeros.data(), (size_t)nframes * 8, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.chunks.p, chunks.data(), chunks.size() * sizeof(RcChunk), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.gframes.p, gf.data(), gf.size() * sizeof(RcGFrame), hipMemcpyHostToDevice, c->stream));
    ENC_OK(run_rc_group(c, chunks.size(), nframes, 1, room, allow_trial != 0));
    HIP_OK(hipMemcpyAsync(planes, c->rc.planes.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(&G, c->rc.group.p, sizeof G, hipMemcpyDeviceToHost, c->stream));
    ENC_OK(wait.sync());
    *lambda = G.lambda;
    *est = G.est;
    *trial = G.trial;
    return 0;
}

struct TensorIn {                   /* the input of htj2k_encode_tensor: n images back to back in device memory */
    const uint8_t *src;
    size_t image_bytes;             /* of one image */
    int dtype, nhwc;                /* HTJ2K_TENSOR_F32 .. ; the layout is NHWC */
    float scale[4], bias[4];
    const htj2k_tensor_mix_in *mix; /* htj2k_encode_tensor_mix: checked, or NULL; scale and bias are then not read */
    const htj2k_tensor_curves_in *curves;   /* htj2k_encode_tensor_curves: checked, or NULL; only beside a mix */
};

struct Call {                       /* what htj2k_encode_batch hands every round */
    const htj2k_frame *in;          /* the frames; a call with a tensor: their sizes and layout only, no planes */
    const EncFrame *fr;
    const int64_t *minsz;           /* calls with a budget or a PSNR target: the smallest stream of every frame */
    int in_on_device, out_on_device;
    uint8_t *out;
    size_t cap, *offsets;
    /* htj2k_transcode_batch: the sources (fr[i] is xc[i].f), the decoder that holds their planes, the event behind its block stage */
    const XcFrame *xc = nullptr;
    htj2k_ctx *dec = nullptr;
    hipEvent_t dec_done = nullptr;
    const TensorIn *tensor = nullptr;   /* htj2k_encode_tensor: the samples come from here (in_on_device is 1) */
};

/* the planes of the input layout and their rows */
static int in_planes(const EncFrame &F) { return F.planar ? F.ncomp : 1; }
static size_t in_row(const EncFrame &F, int p) { return (size_t)(F.planar ? F.cw[p] : F.w * F.step) * F.bytes; }
static int in_rows(const EncFrame &F, int p) { return F.planar ? F.ch[p] : F.h; }

struct Over { int f; int64_t size; };                  /* a frame beyond its target, and its exact bytes */

/* Frames [f0, f0 + nf) of a call: what crosses stages, and the host memory that queued copies read or write (a Round
 * outlives every wait for the stream: encode_round) */
struct Round {
    const Call &call;
    const int f0, nf, nc;
    const bool budget, quality;     /* the call has a byte budget; a PSNR target (with both the budget is a cap) */
    const int64_t group;            /* the call's budget over all its frames (0: none); `budget` is then the frames' own caps */
    const bool xc;                  /* a round of htj2k_transcode_batch: the budget comes in behind the first launch (round_xc_stats) */
    const bool rc, irrev, multi;    /* budget, quality or group: the device selects; 9/7; blocks may get refinement passes */
    const uint64_t out_base;        /* where the round's codestreams start in the call's output */
    int nblk = 0, maxw = 0, maxh = 0;
    size_t ns = 0, nin = 0, npool = 0;                 /* samples, input bytes, pool bytes */
    size_t nua = 0, ntc = 0, ndwt = 0;                 /* entries: unpack table, tile-components, DWT tables at most */
    size_t dwt_args = 0, q_args = 0, q_steps = 0;      /* the args buffer: unpack table at 0, then these */
    std::vector<size_t> plane_off, in_off;             /* [f * nc + k] samples, [f * 4 + p] bytes */
    std::vector<int> blk0;                             /* first block of frame f, [nf] = nblk */
    std::vector<UnpackArgs> ua;                        /* launch tables */
    std::vector<UnpackTensorArgs> uta;                 /* ... of the unpack stage of a call with a tensor */
    std::vector<float> curve_tab;                      /* ... and its curves' tables */
    std::vector<DwtPlane> dwt_tab;
    std::vector<QuantPlane> qp;
    std::vector<float> qs;
    std::vector<GatherPiece> gp;
    std::vector<XcPlane> xp;                           /* transcoding */
    /* ... with a budget, per block: the base plane of its tables (the source's last pass), the source's passes (0: it
     * left the block out), and whether the block came out empty at its source's form (every coarser form is empty too) */
    std::vector<int32_t> xbase, xpass;
    std::vector<uint8_t> xzero;
    std::vector<EncBlk> bt, bt2;                       /* every block; those of a correction launch */
    std::vector<EncRes> res, res2;                     /* the blocks as they stand; of a correction launch */
    std::vector<int32_t> cur_plane, new_plane;         /* the plane every block is coded from; what k_rc_select gave again */
    std::vector<int32_t> new_pass;                     /* and, in calls that ask for passes, the passes (those a block has: res) */
    int maxpass() const { return call.fr[f0].passes; }
    std::vector<uint32_t> sel_len;                     /* k_rc_stats' estimate at the selected plane */
    std::vector<uint8_t> recoded;
    std::vector<double> rc_w, rc_scale;                /* rate control, per block */
    std::vector<RcFrame> rc_fr, again;                 /* per frame, as last selected; the frames selected again */
    std::vector<RcSel> sel, sel2;                      /* of the first selection; of the capped frames' */
    std::vector<float> rc_step;                        /* a PSNR target: per block the step of its band (k_rc_base97) */
    std::vector<RcQFrame> q_fr;                        /* ... per frame k_rc_select_q's table, its results, the record */
    std::vector<RcQual> qual;
    std::vector<htj2k_enc_quality> qinfo;
    std::vector<htj2k_enc_rc> info;
    std::vector<RcChunk> chunks;                       /* a budget over the group: the chunk table, its frames, the frames */
    std::vector<RcGFrame> gframes;                     /* selected again, the first selection's result, the room left */
    std::vector<int32_t> which;
    RcGroup g = {};
    int64_t room = 0;
    htj2k_enc_group ginfo = {};
    EncOut o;                                          /* the codestreams' pieces */

    Round(const Call &k, int first, int end, uint64_t base)
        : call(k), f0(first), nf(end - first), nc(k.fr[first].ncomp), budget(k.fr[first].target > 0),
          quality(k.fr[first].quality > 0), group(k.fr[first].group), xc(k.xc != nullptr),
          rc(!xc && (budget || quality || group > 0)),
          irrev(k.fr[first].irrev != 0), multi(k.fr[first].passes > 1), out_base(base), o() {}
    ~Round() { enc_out_free(&o); }
    const EncFrame &frame(int f) const { return call.fr[f0 + f]; }
    size_t plane_at(int f, int k) const { return plane_off[(size_t)f * nc + k]; }
};

static int round_layout(htj2k_enc_ctx *c, Round &R)
{
    R.in_off.resize((size_t)R.nf * 4);
    for (int f = 0; f < R.nf; f++) {
        const EncFrame &F = R.frame(f);
        for (int k = 0; k < R.nc; k++) {
            R.plane_off.push_back(R.ns);
            R.ns += ((size_t)F.cw[k] * F.ch[k] + 63) & ~(size_t)63;
        }
        for (int p = 0; p < in_planes(F); p++) {
            R.in_off[(size_t)f * 4 + p] = R.nin;
            R.nin += (in_row(F, p) * in_rows(F, p) + 255) & ~(size_t)255;
        }
        for (int i = 0; i < F.nblk; i++) {             /* the launch table of k_ht_encode, every block at plane 0 */
            const EncBlock &b = F.blk[i];
            R.bt.push_back(enc_blk(R.plane_at(f, b.comp) + (uint64_t)b.y * F.cw[b.comp] + (uint64_t)b.x, F.cw[b.comp],
                                   b.w, b.h, 0, F.passes, &R.npool));
            if (R.rc)
                R.bt.back().npasses = 1;                /* k_rc_select decides; the region has room for any choice */
        }
        R.blk0.push_back(R.nblk);
        R.nblk += F.nblk;
        R.maxw = std::max(R.maxw, F.w);
        R.maxh = std::max(R.maxh, std::min(F.h, UNPACK_ROWS));
        R.nua += ((size_t)F.h + UNPACK_ROWS - 1) / UNPACK_ROWS;
        R.ntc += (size_t)F.ntiles * R.nc;
        R.ndwt += (size_t)F.ntiles * R.nc * F.nl;
    }
    R.blk0.push_back(R.nblk);
    R.bt.push_back(EncBlk());
    /* the args buffer: unpack table, DWT tables (an entry per tile-component and level), then (9/7) the quantiser's
     * tile-component table and the step tables, one per component of a frame */
    R.dwt_args = (R.nua * sizeof(UnpackArgs) + 255) & ~(size_t)255;
    R.q_args = R.dwt_args + ((R.ndwt * sizeof(DwtPlane) + 255) & ~(size_t)255);
    R.q_steps = R.q_args + ((R.ntc * sizeof(QuantPlane) + 255) & ~(size_t)255);
    const size_t args_end = R.irrev ? R.q_steps + (size_t)R.nf * R.nc * ENC_MAX_BANDS * sizeof(float) : R.q_args;
    const size_t nb = (size_t)R.nblk + 1;
    if (c->coef.ensure(R.ns * 4) < 0 || c->tmp.ensure(R.ns * 4) < 0 || c->pool.ensure(R.npool + 16) < 0 ||
        c->blk.ensure(nb * sizeof(EncBlk)) < 0 || c->res.ensure(nb * sizeof(EncRes)) < 0 || c->args.ensure(args_end) < 0 ||
        (!R.call.in_on_device && c->in.ensure(R.nin + 256) < 0) || ensure_stamps(c, R.nblk) < 0 ||
        (R.rc && (c->rc.ensure(R.nblk, R.nf, R.multi, R.quality) < 0 || c->rc.blk2.ensure(nb * sizeof(EncBlk)) < 0 ||
                  c->rc.res2.ensure(nb * sizeof(EncRes)) < 0)))
        return HTJ2K_ERR_ENOMEM;
    if (R.group) {
        std::vector<int> nblk;
        for (int f = 0; f < R.nf; f++)
            nblk.push_back(R.frame(f).nblk);
        group_chunks(R.blk0.data(), nblk.data(), R.nf, R.chunks, R.gframes);
        ENC_OK(c->rc.ensure_group(R.chunks.size(), (size_t)R.nf));
    }
    return 0;
}

/* k_enc_unpack_tensor<IRREV, DT, NHWC> over the table, in chunks of what grid.z takes */
template <bool IRREV, int DT>
static void unpack_tensor_launch(htj2k_enc_ctx *c, const Round &R, size_t n, const UnpackTensorFmt &U)
{
    void (*const kernel)(const UnpackTensorArgs *, UnpackTensorFmt) =
        R.call.tensor->nhwc ? k_enc_unpack_tensor<IRREV, DT, 1> : k_enc_unpack_tensor<IRREV, DT, 0>;
    for_z_chunks(n, [&](size_t z0, unsigned nz) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((R.maxw + 255) / 256), (unsigned)R.maxh, nz), dim3(256), 0, c->stream,
                           (const UnpackTensorArgs *)c->args.p + z0, U);
    });
}

/* the unpack stage of a call whose input is a tensor: the table of round_unpack with the frame's image in place of its
 * planes.  A band keeps the image's first element and carries its first row, since a chroma row y reads the tensor's
 * row y << sh */
/* k_enc_unpack_tensor_mix<IRREV, DT, NHWC> over the table of footprint bands: fw x fh footprints at the most in a band */
template <bool IRREV, int DT>
static void unpack_tensor_mix_launch(htj2k_enc_ctx *c, const Round &R, size_t n, int fw, int fh, const UnpackTensorMixFmt &U)
{
    void (*const kernel)(const UnpackTensorArgs *, UnpackTensorMixFmt) =
        R.call.tensor->nhwc ? k_enc_unpack_tensor_mix<IRREV, DT, 1> : k_enc_unpack_tensor_mix<IRREV, DT, 0>;
    for_z_chunks(n, [&](size_t z0, unsigned nz) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((fw + 255) / 256), (unsigned)fh, nz), dim3(256), 0, c->stream,
                           (const UnpackTensorArgs *)c->args.p + z0, U);
    });
}

/* the unpack stage of a call with a tensor and a mix: the table is cut in bands of UNPACK_ROWS footprint rows (never more
 * entries than round_layout counted: a footprint row is one row or more).  The frames of such a call share one size */
static UnpackTensorMixFmt unpack_tensor_mix_fmt(const Round &R)
{
    const TensorIn &T = *R.call.tensor;
    const EncFrame &F0 = R.frame(0);
    UnpackTensorMixFmt U = {};
    U.ncomp = R.nc; U.bits = F0.bits; U.mct = F0.mct;
    for (int k = 1; k < R.nc && k < 3; k++) {              /* the layout's chroma shifts: components 1 and 2 */
        while ((1 << U.sw) < F0.dx[k]) U.sw++;
        while ((1 << U.sh) < F0.dy[k]) U.sh++;
    }
    U.mix.nin = (uint32_t)T.mix->nin;
    U.mix.box = T.mix->chroma == HTJ2K_CHROMA_BOX;
    memcpy(U.mix.m, T.mix->m, sizeof U.mix.m);
    memcpy(U.mix.b, T.mix->b, sizeof U.mix.b);
    const int fcols = ceil_shift(F0.w, U.sw), frows = ceil_shift(F0.h, U.sh);
    const int lastw = F0.w - ((fcols - 1) << U.sw), lasth = F0.h - ((frows - 1) << U.sh);   /* of the clipped footprints */
    for (int cy = 0; cy < 2; cy++)
        for (int cx = 0; cx < 2; cx++)
            U.rcp.r[cy][cx] = 1.0f / (float)((cx ? lastw : 1 << U.sw) * (cy ? lasth : 1 << U.sh));
    return U;
}

static int round_unpack_tensor_curves(htj2k_enc_ctx *c, Round &R);

static int round_unpack_tensor_mix(htj2k_enc_ctx *c, Round &R)
{
    const TensorIn &T = *R.call.tensor;
    if (T.curves)
        return round_unpack_tensor_curves(c, R);
    const EncFrame &F0 = R.frame(0);
    const UnpackTensorMixFmt U = unpack_tensor_mix_fmt(R);
    const int fcols = ceil_shift(F0.w, U.sw), frows = ceil_shift(F0.h, U.sh);
    std::vector<UnpackTensorArgs> &ua = R.uta;
    for (int f = 0; f < R.nf; f++) {
        const EncFrame &F = R.frame(f);
        UnpackTensorArgs A = {};
        A.src = T.src + (size_t)(R.f0 + f) * T.image_bytes;
        A.w = F.w;
        A.ih = F.h;
        for (int y0 = 0; y0 < frows; y0 += UNPACK_ROWS) {
            A.y0 = y0;
            A.h = frows - y0;
            for (int k = 0; k < R.nc; k++) {
                const int row = F.dy[k] > 1 ? y0 : y0 << U.sh;     /* the band's first row in the component's own rows */
                A.dst[k] = (int32_t *)c->coef.p + R.plane_at(f, k) + (size_t)row * F.cw[k];
                A.cw[k] = F.cw[k];
                A.ch[k] = F.ch[k] - row;
            }
            ua.push_back(A);
        }
    }
    HIP_OK(hipMemcpyAsync(c->args.p, ua.data(), ua.size() * sizeof(UnpackTensorArgs), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->ev[EV_START], c->stream));
    const int gh = std::min(frows, UNPACK_ROWS);
    switch (T.dtype) {
    case HTJ2K_TENSOR_F32:
        if (R.irrev) unpack_tensor_mix_launch<true, htj2k_cmp::TENSOR_F32>(c, R, ua.size(), fcols, gh, U);
        else         unpack_tensor_mix_launch<false, htj2k_cmp::TENSOR_F32>(c, R, ua.size(), fcols, gh, U);
        break;
    case HTJ2K_TENSOR_F16:
        if (R.irrev) unpack_tensor_mix_launch<true, htj2k_cmp::TENSOR_F16>(c, R, ua.size(), fcols, gh, U);
        else         unpack_tensor_mix_launch<false, htj2k_cmp::TENSOR_F16>(c, R, ua.size(), fcols, gh, U);
        break;
    default:
        if (R.irrev) unpack_tensor_mix_launch<true, htj2k_cmp::TENSOR_BF16>(c, R, ua.size(), fcols, gh, U);
        else         unpack_tensor_mix_launch<false, htj2k_cmp::TENSOR_BF16>(c, R, ua.size(), fcols, gh, U);
        break;
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(c->ev[EV_UNPACKED], c->stream));
    return 0;
}

/* k_enc_unpack_tensor_curves<IRREV, DT, NHWC> over a table of whole frames, gx workgroups each */
template <bool IRREV, int DT>
static void unpack_tensor_curves_launch(htj2k_enc_ctx *c, const Round &R, size_t n, unsigned gx, const UnpackTensorMixFmt &U,
                                        const htj2k_cmp::CurveInFmt &Q)
{
    void (*const kernel)(const UnpackTensorArgs *, UnpackTensorMixFmt, htj2k_cmp::CurveInFmt) =
        R.call.tensor->nhwc ? k_enc_unpack_tensor_curves<IRREV, DT, 1> : k_enc_unpack_tensor_curves<IRREV, DT, 0>;
    for_z_chunks(n, [&](size_t z0, unsigned nz) {
        hipLaunchKernelGGL(kernel, dim3(gx, 1, nz), dim3(CURVE_IN_THREADS), (size_t)Q.nfloat * sizeof(float), c->stream,
                           (const UnpackTensorArgs *)c->args.p + z0, U, Q);
    });
}

/* the unpack stage of a call with a tensor, a mix and curves: one table entry a frame, both tables uploaded in front of
 * the launch.  Every workgroup stages the tables before it reads a tensor element, so a frame gets no more workgroups
 * than leave each ENC_CURVES_SRC_PER_TABLE times the tables' bytes of tensor to read (HTJ2K_ENC_CURVES_GRID: another
 * factor; results do not depend on it), and never more than a footprint a thread asks for */
static int round_unpack_tensor_curves(htj2k_enc_ctx *c, Round &R)
{
    const TensorIn &T = *R.call.tensor;
    const EncFrame &F0 = R.frame(0);
    const UnpackTensorMixFmt U = unpack_tensor_mix_fmt(R);
    const int fcols = ceil_shift(F0.w, U.sw), frows = ceil_shift(F0.h, U.sh);
    htj2k_cmp::CurveInFmt Q = htj2k_cmp::curve_in_fmt(*T.curves, R.nc, &R.curve_tab);
    const size_t table_bytes = R.curve_tab.size() * sizeof(float);
    ENC_OK(c->curve_tab.ensure(table_bytes));
    Q.tab = (const float *)c->curve_tab.p;
    std::vector<UnpackTensorArgs> &ua = R.uta;
    for (int f = 0; f < R.nf; f++) {
        const EncFrame &F = R.frame(f);
        UnpackTensorArgs A = {};
        A.src = T.src + (size_t)(R.f0 + f) * T.image_bytes;
        A.w = F.w;
        A.ih = F.h;
        A.h = frows;
        for (int k = 0; k < R.nc; k++) {
            A.dst[k] = (int32_t *)c->coef.p + R.plane_at(f, k);
            A.cw[k] = F.cw[k];
            A.ch[k] = F.ch[k];
        }
        ua.push_back(A);
    }
    HIP_OK(hipMemcpyAsync(c->args.p, ua.data(), ua.size() * sizeof(UnpackTensorArgs), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->curve_tab.p, R.curve_tab.data(), table_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->ev[EV_START], c->stream));
    const size_t foot = (size_t)fcols * (size_t)frows;
    const unsigned gx = htj2k_cmp::curve_grid(std::min<size_t>((foot + CURVE_IN_THREADS - 1) / CURVE_IN_THREADS, ua.size() >= 64 ? 256 : 2048),
                                                 T.image_bytes, table_bytes, c->curves_grid);
    switch (T.dtype) {
    case HTJ2K_TENSOR_F32:
        if (R.irrev) unpack_tensor_curves_launch<true, htj2k_cmp::TENSOR_F32>(c, R, ua.size(), gx, U, Q);
        else         unpack_tensor_curves_launch<false, htj2k_cmp::TENSOR_F32>(c, R, ua.size(), gx, U, Q);
        break;
    case HTJ2K_TENSOR_F16:
        if (R.irrev) unpack_tensor_curves_launch<true, htj2k_cmp::TENSOR_F16>(c, R, ua.size(), gx, U, Q);
        else         unpack_tensor_curves_launch<false, htj2k_cmp::TENSOR_F16>(c, R, ua.size(), gx, U, Q);
        break;
    default:
        if (R.irrev) unpack_tensor_curves_launch<true, htj2k_cmp::TENSOR_BF16>(c, R, ua.size(), gx, U, Q);
        else         unpack_tensor_curves_launch<false, htj2k_cmp::TENSOR_BF16>(c, R, ua.size(), gx, U, Q);
        break;
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(c->ev[EV_UNPACKED], c->stream));
    return 0;
}

static int round_unpack_tensor(htj2k_enc_ctx *c, Round &R)
{
    static_assert(sizeof(UnpackTensorArgs) <= sizeof(UnpackArgs), "the args buffer is laid out for UnpackArgs entries");
    const TensorIn &T = *R.call.tensor;
    if (T.mix)
        return round_unpack_tensor_mix(c, R);
    const EncFrame &F0 = R.frame(0);
    std::vector<UnpackTensorArgs> &ua = R.uta;
    for (int f = 0; f < R.nf; f++) {
        const EncFrame &F = R.frame(f);
        UnpackTensorArgs A = {};
        A.src = T.src + (size_t)(R.f0 + f) * T.image_bytes;
        A.w = F.w;
        A.ih = F.h;
        for (int y0 = 0; y0 < F.h; y0 += UNPACK_ROWS) {
            A.y0 = y0;
            A.h = F.h - y0;
            for (int k = 0; k < R.nc; k++) {
                A.dst[k] = (int32_t *)c->coef.p + R.plane_at(f, k) + (size_t)y0 * F.cw[k];
                A.cw[k] = F.cw[k];
                A.ch[k] = std::max(F.ch[k] - y0, 0);
            }
            ua.push_back(A);
        }
    }
    UnpackTensorFmt U = {};
    U.ncomp = R.nc; U.bits = F0.bits; U.mct = F0.mct;
    for (int k = 0; k < R.nc; k++) {
        while ((1 << U.sw[k]) < F0.dx[k]) U.sw[k]++;
        while ((1 << U.sh[k]) < F0.dy[k]) U.sh[k]++;
        U.scale[k] = T.scale[k];
        U.bias[k] = T.bias[k];
    }
    HIP_OK(hipMemcpyAsync(c->args.p, ua.data(), ua.size() * sizeof(UnpackTensorArgs), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->ev[EV_START], c->stream));
    switch (T.dtype) {
    case HTJ2K_TENSOR_F32:
        if (R.irrev) unpack_tensor_launch<true, htj2k_cmp::TENSOR_F32>(c, R, ua.size(), U);
        else         unpack_tensor_launch<false, htj2k_cmp::TENSOR_F32>(c, R, ua.size(), U);
        break;
    case HTJ2K_TENSOR_F16:
        if (R.irrev) unpack_tensor_launch<true, htj2k_cmp::TENSOR_F16>(c, R, ua.size(), U);
        else         unpack_tensor_launch<false, htj2k_cmp::TENSOR_F16>(c, R, ua.size(), U);
        break;
    default:
        if (R.irrev) unpack_tensor_launch<true, htj2k_cmp::TENSOR_BF16>(c, R, ua.size(), U);
        else         unpack_tensor_launch<false, htj2k_cmp::TENSOR_BF16>(c, R, ua.size(), U);
        break;
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(c->ev[EV_UNPACKED], c->stream));
    return 0;
}

static int round_unpack(htj2k_enc_ctx *c, Round &R)
{
    if (R.call.tensor)
        return round_unpack_tensor(c, R);
    const EncFrame &F0 = R.frame(0);
    for (int f = 0; f < R.nf; f++) {
        const EncFrame &F = R.frame(f);
        const htj2k_frame &I = R.call.in[R.f0 + f];
        UnpackArgs A = {};
        A.w = F.w;
        A.h = F.h;
        for (int p = 0; p < in_planes(F); p++) {
            const size_t row = in_row(F, p);
            uint8_t *d = R.call.in_on_device ? nullptr : (uint8_t *)c->in.p + R.in_off[(size_t)f * 4 + p];
            if (d)                                     /* host input: packed rows in c->in */
                HIP_OK(hipMemcpy2DAsync(d, row, I.data[p], (size_t)I.linesize[p], row, (size_t)in_rows(F, p),
                                        hipMemcpyHostToDevice, c->stream));
            A.src[p] = d ? d : I.data[p];
            A.linesize[p] = d ? (int64_t)row : I.linesize[p];
        }
        for (int k = 0; k < R.nc; k++) {
            A.dst[k] = (int32_t *)c->coef.p + R.plane_at(f, k);
            A.cw[k] = F.cw[k];
            A.ch[k] = F.ch[k];
        }
        /* a frame taller than grid.y goes in as bands of UNPACK_ROWS rows: the same table entry, moved down */
        for (int y0 = 0; y0 < F.h; y0 += UNPACK_ROWS) {
            UnpackArgs B = A;
            B.h = F.h - y0;
            for (int p = 0; p < in_planes(F); p++)
                B.src[p] += (int64_t)y0 * A.linesize[p];
            for (int k = 0; k < R.nc; k++) {
                B.dst[k] += (size_t)y0 * F.cw[k];
                B.ch[k] = std::max(F.ch[k] - y0, 0);
            }
            R.ua.push_back(B);
        }
    }
    const UnpackFmt U = { R.nc, F0.planar, F0.step, F0.bytes, F0.shift, F0.bits, F0.mct };
    HIP_OK(hipMemcpyAsync(c->args.p, R.ua.data(), R.ua.size() * sizeof(UnpackArgs), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->ev[EV_START], c->stream));
    for_z_chunks(R.ua.size(), [&](size_t z0, unsigned nz) {
        hipLaunchKernelGGL(R.irrev ? k_enc_unpack<true> : k_enc_unpack<false>,
                           dim3((unsigned)((R.maxw + 255) / 256), (unsigned)R.maxh, nz), dim3(256), 0, c->stream,
                           (const UnpackArgs *)c->args.p + z0, U);
    });
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(c->ev[EV_UNPACKED], c->stream));
    return 0;
}

static int round_transform(htj2k_enc_ctx *c, Round &R)
{
    std::vector<DwtRegion> regions;
    const float *d_steps = (const float *)((uint8_t *)c->args.p + R.q_steps);
    int qw = 0, qh = 0;
    for (int f = 0; f < R.nf; f++)
        for (int k = 0; k < R.nc; k++) {
            const EncFrame &F = R.frame(f);
            const float *steps = d_steps + R.qs.size();
            if (R.irrev)
                R.qs.insert(R.qs.end(), F.fstep[k], F.fstep[k] + ENC_MAX_BANDS);
            /* every tile-component is transformed on its own, in its rectangle of the component plane */
            for (int t = 0; t < F.ntiles; t++) {
                const htj2k_enc_tile &T = F.tile[t].t;
                const size_t at = R.plane_at(f, k) + (size_t)T.y0[k] * F.cw[k] + T.x0[k];
                int32_t *p = (int32_t *)c->coef.p + at;
                regions.push_back(DwtRegion{ p, (int32_t *)c->tmp.p + at, F.cw[k], T.x0[k], T.y0[k], T.x1[k], T.y1[k], F.nl });
                if (!R.irrev)
                    continue;
                R.qp.push_back(QuantPlane{ p, steps, F.cw[k], F.nl, T.x0[k], T.y0[k], T.x1[k], T.y1[k] });
                qw = std::max(qw, T.x1[k] - T.x0[k]);
                qh = std::max(qh, T.y1[k] - T.y0[k]);
            }
        }
    ENC_OK(run_fdwt(c, regions, R.dwt_args, R.dwt_tab, R.irrev));
    if (R.irrev && R.quality) {                        /* the error of the caller's quantiser, while the floats are there */
        for (int f = 0; f < R.nf; f++)
            for (int i = 0; i < R.frame(f).nblk; i++)
                R.rc_step.push_back(enc_block_step(&R.frame(f), &R.frame(f).blk[i]));
        HIP_OK(hipMemcpyAsync(c->rc.step.p, R.rc_step.data(), R.rc_step.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipEventRecord(c->ev[EV_BASE0], c->stream));
        ENC_OK(run_rc_base(c, (const EncBlk *)c->blk.p, R.nblk));
        HIP_OK(hipEventRecord(c->ev[EV_BASE1], c->stream));
    }
    if (R.irrev) {
        const QuantPlane *d_qp = (const QuantPlane *)((uint8_t *)c->args.p + R.q_args);
        HIP_OK(hipMemcpyAsync((void *)d_qp, R.qp.data(), R.qp.size() * sizeof(QuantPlane), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync((void *)d_steps, R.qs.data(), R.qs.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        for_z_chunks(R.qp.size(), [&](size_t z0, unsigned nz) {
            hipLaunchKernelGGL(k_quant97, dim3((unsigned)((qw + 255) / 256), (unsigned)qh, nz), dim3(256), 0, c->stream, d_qp + z0);
        });
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipEventRecord(c->ev[EV_TRANSFORMED], c->stream));
    return 0;
}

static int round_block_table(htj2k_enc_ctx *c, Round &R)
{
    HIP_OK(hipMemcpyAsync(c->blk.p, R.bt.data(), (size_t)R.nblk * sizeof(EncBlk), hipMemcpyHostToDevice, c->stream));
    return 0;
}

static double psnr_peak2(const EncFrame &F)
{
    const double peak = (double)(((uint64_t)1 << F.bits) - 1);
    return peak * peak;
}

/* the model PSNR of a frame of distortion d (infinity: none) */
static double model_psnr(const EncFrame &F, int nc, double d)
{
    double n = 0;
    for (int k = 0; k < nc; k++)
        n += (double)F.cw[k] * F.ch[k];
    return d > 0 ? 10.0 * log10(psnr_peak2(F) * n / d) : INFINITY;
}

static int round_select(htj2k_enc_ctx *c, Round &R)
{
    if (!R.rc)
        return 0;
    R.rc_w.resize((size_t)R.nblk + 1);
    R.rc_scale.assign((size_t)R.nblk + 1, 1.0);
    R.rc_fr.resize((size_t)R.nf);
    for (int f = 0; f < R.nf; f++) {
        const EncFrame &F = R.frame(f);
        for (int i = 0; i < F.nblk; i++) {
            const EncBlock &b = F.blk[i];
            R.rc_w[(size_t)R.blk0[f] + i] = enc_block_weight(&F, &b);
        }
        R.rc_fr[f] = RcFrame{ R.blk0[f], F.nblk, F.target - R.call.minsz[R.f0 + f], 1, 0 };
        if (R.quality) {
            double n = 0;
            for (int k = 0; k < R.nc; k++)
                n += (double)F.cw[k] * F.ch[k];
            R.q_fr.push_back(RcQFrame{ R.blk0[f], F.nblk, psnr_peak2(F) * n / pow(10.0, F.quality / 10.0) });
        }
    }
    if (R.quality)
        HIP_OK(hipMemcpyAsync(c->rc.qframes.p, R.q_fr.data(), (size_t)R.nf * sizeof(RcQFrame), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.w.p, R.rc_w.data(), (size_t)R.nblk * 8, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.scale.p, R.rc_scale.data(), (size_t)R.nblk * 8, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.frames.p, R.rc_fr.data(), (size_t)R.nf * sizeof(RcFrame), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->ev[EV_T0], c->stream));
    ENC_OK(run_rc_stats(c, R.nblk, RC_PLANES));
    HIP_OK(hipEventRecord(c->ev[EV_T1], c->stream));
    if (R.multi) {                                     /* htj2k_enc_ref_stage_ms' second figure */
        ENC_OK(run_rc_stats_passes(c, R.nblk, RC_PLANES));
        HIP_OK(hipEventRecord(c->ev[EV_STATS2], c->stream));
    }
    if (R.quality)
        ENC_OK(run_rc_select_q(c, (size_t)R.nf, R.maxpass(), R.irrev));
    else if (!R.group || R.budget)
        ENC_OK(run_rc_select(c, (size_t)R.nf, R.maxpass()));
    if (R.group) {                                     /* the frames' own caps give floors; then one slope for all */
        R.room = R.group;
        for (int f = 0; f < R.nf; f++)
            R.room -= R.call.minsz[R.f0 + f];
        HIP_OK(hipMemcpyAsync(c->rc.chunks.p, R.chunks.data(), R.chunks.size() * sizeof(RcChunk), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(c->rc.gframes.p, R.gframes.data(), R.gframes.size() * sizeof(RcGFrame), hipMemcpyHostToDevice, c->stream));
        if (R.budget)
            ENC_OK(run_rc_group_floors(c, nullptr, R.nf));
        else
            HIP_OK(hipMemsetAsync(c->rc.floors.p, 0, (size_t)R.nf * 8, c->stream));
        ENC_OK(run_rc_group(c, R.chunks.size(), R.nf, R.maxpass(), R.room, 1));
    }
    HIP_OK(hipEventRecord(c->ev[EV_SELECTED], c->stream));
    return 0;
}

static int round_code(htj2k_enc_ctx *c, Round &R)
{
    if (R.multi) {
        ENC_OK(run_refine_plan(c, (EncBlk *)c->blk.p, R.nblk, (EncRes *)c->res.p));
        HIP_OK(hipEventRecord(c->ev[EV_PLANNED], c->stream));
    }
    ENC_OK(run_ht(c, (const EncBlk *)c->blk.p, R.nblk, (EncRes *)c->res.p));
    HIP_OK(hipEventRecord(c->ev[EV_CODED], c->stream));
    if (R.multi) {
        ENC_OK(run_refine(c, (const EncBlk *)c->blk.p, R.nblk, (EncRes *)c->res.p));
        HIP_OK(hipEventRecord(c->ev[EV_REFINED], c->stream));
    }
    R.res.resize((size_t)R.nblk + 1);
    R.cur_plane.assign((size_t)R.nblk + 1, 0);
    R.sel_len.assign((size_t)R.nblk + 1, 0);
    R.sel.resize((size_t)R.nf + 1);
    HIP_OK(hipMemcpyAsync(R.res.data(), c->res.p, (size_t)R.nblk * sizeof(EncRes), hipMemcpyDeviceToHost, c->stream));
    if (R.rc) {
        HIP_OK(hipMemcpyAsync(R.cur_plane.data(), c->rc.planes.p, (size_t)R.nblk * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipMemcpyAsync(R.sel_len.data(), c->rc.sel_len.p, (size_t)R.nblk * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipMemcpyAsync(R.sel.data(), c->rc.sel.p, (size_t)R.nf * sizeof(RcSel), hipMemcpyDeviceToHost, c->stream));
    }
    if (R.group)
        HIP_OK(hipMemcpyAsync(&R.g, c->rc.group.p, sizeof R.g, hipMemcpyDeviceToHost, c->stream));
    R.qual.assign((size_t)R.nf + 1, RcQual());
    if (R.quality)
        HIP_OK(hipMemcpyAsync(R.qual.data(), c->rc.qual.p, (size_t)R.nf * sizeof(RcQual), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    ENC_OK(collect_stamps(c, R.nblk, R.multi));
    c->ms[0] += ev_ms(c->ev[EV_START], c->ev[EV_UNPACKED]);
    c->ms[1] += ev_ms(c->ev[EV_UNPACKED], c->ev[EV_TRANSFORMED]);
    c->ms[2] += ev_ms(c->ev[R.multi ? EV_PLANNED : R.rc ? EV_SELECTED : EV_TRANSFORMED], c->ev[EV_CODED]);
    if (R.multi)
        c->ref_ms[0] += ev_ms(c->ev[R.rc ? EV_SELECTED : EV_TRANSFORMED], c->ev[EV_PLANNED]) + ev_ms(c->ev[EV_CODED], c->ev[EV_REFINED]);
    if (R.rc) {
        c->rc_ms[0] += ev_ms(c->ev[EV_T0], c->ev[EV_T1]);
        (R.quality ? c->q_ms[1] : c->rc_ms[1]) += ev_ms(c->ev[R.multi ? EV_STATS2 : EV_T1], c->ev[EV_SELECTED]);
        if (R.group) {                                 /* the group kernels' time is its own figure */
            const float g = ev_ms(c->ev[EV_G0], c->ev[EV_G1]);
            c->group_ms += g;
            c->rc_ms[1] -= g;
        }
        if (R.quality && R.irrev)
            c->q_ms[0] += ev_ms(c->ev[EV_BASE0], c->ev[EV_BASE1]);
        if (R.multi)
            c->ref_ms[1] += ev_ms(c->ev[EV_T1], c->ev[EV_STATS2]);
    }
    ENC_OK(check_coded(c, R.res.data(), (size_t)R.nblk));
    R.info.assign((size_t)R.nf, htj2k_enc_rc());
    R.recoded.assign((size_t)R.nblk + 1, 0);
    for (int f = 0; f < R.nf; f++) {
        R.info[f].target_bytes = R.frame(f).target;
        R.info[f].nblocks = R.frame(f).nblk;
        R.info[f].ht_launches = 1;
        R.info[f].trial = R.rc ? R.sel[f].trial : 0;
        R.info[f].est_bytes = R.rc ? (int64_t)R.sel[f].est + R.call.minsz[R.f0 + f] : 0;
    }
    if (R.group) {
        R.ginfo.group_bytes = R.group;
        R.ginfo.est_bytes = (int64_t)R.g.est + (R.group - R.room);
        R.ginfo.lambda = R.g.lambda;
        R.ginfo.nframes = R.nf;
        R.ginfo.nblocks = R.nblk;
        R.ginfo.frames_capped = R.g.frames_capped;
        R.ginfo.ht_launches = 1;
        R.ginfo.trial = R.g.trial;
    }
    R.qinfo.assign((size_t)R.nf, htj2k_enc_quality());
    for (int f = 0; R.quality && f < R.nf; f++) {
        const EncFrame &F = R.frame(f);
        R.qinfo[f] = htj2k_enc_quality{ F.quality, model_psnr(F, R.nc, R.qual[f].dbase), model_psnr(F, R.nc, R.qual[f].d),
                                        R.qual[f].lambda, R.qual[f].short_of_target, 0 };
    }
    return 0;
}

/* frame f as its blocks stand (R.res, R.cur_plane): the guard bits they need, then its codestream appended to `o` */
static int frame_write(htj2k_enc_ctx *c, const Round &R, int f, EncOut *o)
{
    const EncFrame &F = R.frame(f);
    const EncRes *e = R.res.data() + R.blk0[f];
    const int32_t *pl = R.cur_plane.data() + R.blk0[f];
    std::vector<int> lcup((size_t)F.nblk), mu((size_t)F.nblk), lref, np, cp;
    for (int i = 0; i < F.nblk; i++) {
        lcup[i] = e[i].lcup;
        mu[i] = e[i].max_u;
    }
    if (R.multi) {                                     /* the cleanup pass of a block of several passes coded the plane above */
        lref.resize((size_t)F.nblk);
        np.resize((size_t)F.nblk);
        cp.resize((size_t)F.nblk);
        for (int i = 0; i < F.nblk; i++) {
            np[i] = e[i].lcup > 0 ? e[i].npasses : 1;
            lref[i] = np[i] > 1 ? e[i].lref : 0;
            cp[i] = pl[i] < 0 ? pl[i] : pl[i] + (np[i] > 1);
        }
        pl = cp.data();
    }
    const int guard = enc_guard_bits(&F, mu.data(), pl, enc_log, c);
    return guard < 0 ? guard : enc_write(&F, guard, lcup.data(), R.multi ? lref.data() : nullptr, R.multi ? np.data() : nullptr, pl, o);
}

/* exact bytes of that codestream (the headers are written and thrown away) */
static int64_t frame_size(htj2k_enc_ctx *c, const Round &R, int f)
{
    EncOut o = {};
    const int r = frame_write(c, R, f, &o);
    const int64_t n = r < 0 ? r : (int64_t)o.size;
    enc_out_free(&o);
    return n;
}

/* the frames coded in this launch that came out beyond their target */
static int rc_measure(htj2k_enc_ctx *c, const Round &R, int launch, std::vector<Over> &over)
{
    over.clear();
    for (int f = 0; f < R.nf; f++) {
        if (R.info[f].ht_launches != launch)
            continue;                                  /* it fitted in an earlier launch */
        const int64_t size = frame_size(c, R, f);
        if (size < 0)
            return (int)size;
        if (size > R.frame(f).target)
            over.push_back(Over{ f, size });
    }
    return 0;
}

/* the passes block b has, and its bytes: the cleanup segment and, behind it, the refinement segment */
static int blk_passes(const Round &R, size_t b) { return R.multi && R.res[b].lcup > 0 ? R.res[b].npasses : 1; }
static int blk_bytes(const Round &R, size_t b) { return R.res[b].lcup + (blk_passes(R, b) > 1 ? R.res[b].lref : 0); }

/* the distortion of the candidates of blocks [b0, b0 + n), from the statistics on the device (synchronous copies);
 * `with_base`: and, 9/7, k_rc_base97's figure (zeros otherwise) */
struct BlockDist {
    size_t b0 = 0;
    std::vector<uint64_t> dist, dist2, dist3;
    std::vector<double> dskip, base;
    int fetch(htj2k_enc_ctx *c, const Round &R, size_t first, size_t n, bool with_base)
    {
        const size_t rows = n * RC_PLANES;
        b0 = first;
        dist.resize(rows);
        dskip.resize(n);
        base.assign(n, 0.0);
        HIP_OK(hipMemcpy(dist.data(), c->rc.S.dist + b0 * RC_PLANES, rows * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(dskip.data(), c->rc.S.dskip + b0, n * 8, hipMemcpyDeviceToHost));
        if (R.multi) {
            dist2.resize(rows);
            dist3.resize(rows);
            HIP_OK(hipMemcpy(dist2.data(), c->rc.P.dist2 + b0 * RC_PLANES, rows * 8, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(dist3.data(), c->rc.P.dist3 + b0 * RC_PLANES, rows * 8, hipMemcpyDeviceToHost));
        }
        if (R.irrev && with_base)
            HIP_OK(hipMemcpy(base.data(), (const double *)c->rc.base.p + b0, n * 8, hipMemcpyDeviceToHost));
        return 0;
    }
    /* d of block b as it stands: left out, or the candidate of its passes at its plane */
    double at(const Round &R, size_t b) const
    {
        const int k = blk_passes(R, b);
        int p = R.cur_plane[b];
        if (p < 0)
            return dskip[b - b0];
        if (!R.xbase.empty())                          /* transcoding: the tables start at the block's base plane */
            p -= R.xbase[b];
        return (double)(k == 1 ? dist : k == 2 ? dist2 : dist3)[(b - b0) * RC_PLANES + std::min(p, RC_PLANES - 1)];
    }
};

/* last resort for frames [fa, fb), whose exact bytes size[0 .. fb - fa) add up to more than `limit`: coded blocks are
 * left out across these frames, least weighted distortion per byte saved first (enc_drop_take), a batch that saves what
 * the sum is over by at a time; then the frames that lost blocks are measured again (`size` is kept current) and carry
 * info.last_resort.  "Left out" has length 0, so the frames end inside the limit without another launch.  (Only the
 * bytes of a block's current plane are kept, so the planes of earlier launches are not candidates here.) */
static int rc_last_resort(htj2k_enc_ctx *c, Round &R, int fa, int fb, int64_t limit, int64_t *size)
{
    const size_t b0 = (size_t)R.blk0[fa], b1 = (size_t)R.blk0[fb];
    BlockDist D;
    ENC_OK(D.fetch(c, R, b0, b1 - b0, false));
    std::vector<EncDrop> drop;
    for (size_t b = b0; b < b1; b++)
        if (R.res[b].lcup > 0)
            drop.push_back(EncDrop{ R.rc_w[b] * (D.dskip[b - b0] - D.at(R, b)) / blk_bytes(R, b), (int32_t)b, blk_bytes(R, b) });
    int64_t total = 0;
    for (int f = fa; f < fb; f++)
        total += size[f - fa];
    size_t next = 0;
    while (total > limit && next < drop.size()) {
        int64_t saved = 0;
        const size_t from = next;
        next = enc_drop_take(drop.data(), drop.size(), next, total - limit, &saved);
        std::vector<uint8_t> dirty((size_t)(fb - fa), 0);
        for (size_t j = from; j < next; j++) {
            const size_t b = (size_t)drop[j].block;
            const int f = (int)(std::upper_bound(R.blk0.begin(), R.blk0.end(), drop[j].block) - R.blk0.begin()) - 1;
            R.res[b].lcup = 0;
            R.res[b].max_u = 0;
            R.res[b].lref = 0;
            R.res[b].npasses = 1;
            R.cur_plane[b] = -1;
            dirty[(size_t)(f - fa)] = 1;
            R.info[f].last_resort = 1;
        }
        for (int f = fa; f < fb; f++)
            if (dirty[(size_t)(f - fa)]) {
                const int64_t n = frame_size(c, R, f);
                if (n < 0)
                    return (int)n;
                total += n - size[f - fa];
                size[f - fa] = n;
            }
    }
    return total > limit ? HTJ2K_ERR_BUG : 0;
}

/* the scale of the coded blocks of frame f: their actual bytes over the estimate they were selected at */
static void rc_rescale(Round &R, int f)
{
    for (size_t b = (size_t)R.blk0[f]; b < (size_t)R.blk0[f + 1]; b++)
        if (R.res[b].lcup > 0 && R.sel_len[b] > 0)
            R.rc_scale[b] = (double)blk_bytes(R, b) / (double)R.sel_len[b];
}

/* behind a selection: its planes into R.new_plane, its passes (calls that ask for them) into R.new_pass, its estimates
 * into R.sel_len; waits for the stream */
static int rc_fetch_selection(htj2k_enc_ctx *c, Round &R)
{
    R.new_plane.resize((size_t)R.nblk + 1);
    R.new_pass.assign((size_t)R.nblk + 1, 1);
    HIP_OK(hipMemcpyAsync(R.new_plane.data(), c->rc.planes.p, (size_t)R.nblk * 4, hipMemcpyDeviceToHost, c->stream));
    if (R.multi)
        HIP_OK(hipMemcpyAsync(R.new_pass.data(), c->rc.passes.p, (size_t)R.nblk * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(R.sel_len.data(), c->rc.sel_len.p, (size_t)R.nblk * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    /* transcoding: the selection is in planes relative to the block's base; this is the one place the base is added.  A
     * block the source left out, or one that is empty at its source's form, stays as it is */
    for (size_t b = 0; b < R.xbase.size(); b++) {
        if (!R.xpass[b] || R.xzero[b]) {
            R.new_plane[b] = R.cur_plane[b];
            R.new_pass[b] = 1;
        } else if (R.new_plane[b] >= 0) {
            R.new_plane[b] += R.xbase[b];
        }
    }
    return 0;
}

/* select again: every coded block's estimates scaled by its own actual / estimated, the budget down by the overshoot.
 * `cap`: the frames a PSNR target took beyond the budget start again, with the selection of a budgeted call (R.sel2) */
static int rc_select_again(htj2k_enc_ctx *c, Round &R, const std::vector<Over> &over, bool cap = false)
{
    R.again.clear();
    for (const Over &o : over) {
        const int f = o.f;
        const EncFrame &F = R.frame(f);
        if (cap) {
            R.again.push_back(R.rc_fr[f]);
            continue;
        }
        rc_rescale(R, f);
        /* a transcoded frame behind its first launch was coded at its source's form, not at a selection for this
         * budget: what it is over by says nothing about the estimates, and the scales alone carry what was learnt */
        if (!(R.xc && R.info[f].ht_launches == 1))
            R.rc_fr[f].budget = std::max<int64_t>(0, R.rc_fr[f].budget - (o.size - F.target));
        R.rc_fr[f].allow_trial = 0;
        R.again.push_back(R.rc_fr[f]);
    }
    HIP_OK(hipMemcpyAsync(c->rc.scale.p, R.rc_scale.data(), (size_t)R.nblk * 8, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.frames.p, R.again.data(), R.again.size() * sizeof(RcFrame), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->ev[EV_T0], c->stream));
    ENC_OK(run_rc_select(c, R.again.size(), R.maxpass()));
    HIP_OK(hipEventRecord(c->ev[EV_T1], c->stream));
    R.sel2.resize(R.again.size());
    if (cap || R.xc)
        HIP_OK(hipMemcpyAsync(R.sel2.data(), c->rc.sel.p, R.again.size() * sizeof(RcSel), hipMemcpyDeviceToHost, c->stream));
    ENC_OK(rc_fetch_selection(c, R));
    c->rc_ms[1] += ev_ms(c->ev[EV_T0], c->ev[EV_T1]);
    return 0;
}

/* the blocks of frame f whose plane or passes changed (R.new_plane, R.new_pass) join the launch table R.bt2;
 * bt2[k] is block which[k].  -> whether any did */
static bool rc_collect(Round &R, int f, bool cap, std::vector<size_t> &which)
{
    const size_t before = R.bt2.size();
    for (int i = 0; i < R.frame(f).nblk; i++) {
        const size_t b = (size_t)R.blk0[f] + i;
        if (R.new_plane[b] == R.cur_plane[b] && (R.new_plane[b] < 0 || R.new_pass[b] == blk_passes(R, b)))
            continue;
        R.cur_plane[b] = R.new_plane[b];
        R.recoded[b] = !cap;
        R.bt2.push_back(R.bt[b]);
        R.bt2.back().plane = R.new_plane[b];
        R.bt2.back().npasses = R.new_pass[b];
        which.push_back(b);
    }
    return R.bt2.size() > before;
}

static int rc_code_again(htj2k_enc_ctx *c, Round &R, const std::vector<size_t> &which, bool cap);

/* code again the blocks whose plane changed; a block's earlier bytes stay valid for its earlier plane.  `cap`: this is
 * the frames' first launch as budgeted frames (launch 0): nothing counts as coded again, and the launch's time is HT time */
static int rc_recode(htj2k_enc_ctx *c, Round &R, int launch, std::vector<Over> &over, bool cap = false)
{
    std::vector<size_t> which;
    R.bt2.clear();
    for (Over &o : over) {
        const int f = o.f;
        if (rc_collect(R, f, cap, which) || cap)
            R.info[f].ht_launches = launch + 1;
        else                                           /* the same selection again: another round cannot help */
            ENC_OK(rc_last_resort(c, R, f, f + 1, R.frame(f).target, &o.size));
    }
    return rc_code_again(c, R, which, cap);
}

/* the launch over R.bt2 and its results into R.res */
static int rc_code_again(htj2k_enc_ctx *c, Round &R, const std::vector<size_t> &which, bool cap)
{
    if (R.bt2.empty())
        return 0;
    R.res2.resize(R.bt2.size());
    HIP_OK(hipMemcpyAsync(c->rc.blk2.p, R.bt2.data(), R.bt2.size() * sizeof(EncBlk), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->ev[EV_T0], c->stream));
    if (R.multi)
        ENC_OK(run_refine_plan(c, (EncBlk *)c->rc.blk2.p, (int)R.bt2.size(), (EncRes *)c->rc.res2.p));
    ENC_OK(run_ht(c, (const EncBlk *)c->rc.blk2.p, (int)R.bt2.size(), (EncRes *)c->rc.res2.p));
    if (R.multi)
        ENC_OK(run_refine(c, (const EncBlk *)c->rc.blk2.p, (int)R.bt2.size(), (EncRes *)c->rc.res2.p));
    HIP_OK(hipEventRecord(c->ev[EV_T1], c->stream));
    HIP_OK(hipMemcpyAsync(R.res2.data(), c->rc.res2.p, R.bt2.size() * sizeof(EncRes), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    (cap ? c->ms[2] : c->rc_ms[2]) += ev_ms(c->ev[EV_T0], c->ev[EV_T1]);
    ENC_OK(check_coded(c, R.res2.data(), R.res2.size()));
    for (size_t k = 0; k < which.size(); k++)
        R.res[which[k]] = R.res2[k];
    return 0;
}

/* D of frame f as its blocks stand, from the statistics on the device (the frames the cap decided; the others have
 * k_rc_select_q's own sum) */
static int frame_model_d(htj2k_enc_ctx *c, const Round &R, int f, double *d)
{
    BlockDist D;
    ENC_OK(D.fetch(c, R, (size_t)R.blk0[f], (size_t)R.frame(f).nblk, true));
    double sum = 0.0;
    for (size_t b = D.b0; b < D.b0 + (size_t)R.frame(f).nblk; b++)
        sum += R.rc_w[b] * (D.base[b - D.b0] + 0.25 * D.at(R, b));
    *d = sum;
    return 0;
}

/* calls with a PSNR target and a budget: a frame whose estimate or whose coded size is beyond the budget starts again as
 * the budgeted call starts it: k_rc_select on the same statistics, its blocks coded where that selection differs.  It
 * is then a budgeted frame in its first launch (round_enforce), and the quality selection's launch does not count */
static int round_cap(htj2k_enc_ctx *c, Round &R)
{
    if (!R.quality || !R.budget)
        return 0;
    std::vector<Over> over;
    for (int f = 0; f < R.nf; f++) {
        int64_t size = R.info[f].est_bytes;
        if (size <= R.frame(f).target && (size = frame_size(c, R, f)) < 0)
            return (int)size;
        if (size > R.frame(f).target)
            over.push_back(Over{ f, size });
    }
    if (over.empty())
        return 0;
    ENC_OK(rc_select_again(c, R, over, true));
    ENC_OK(rc_recode(c, R, 0, over, true));
    for (size_t j = 0; j < over.size(); j++) {
        const int f = over[j].f;
        R.info[f].trial = R.sel2[j].trial;
        R.info[f].est_bytes = (int64_t)R.sel2[j].est + R.call.minsz[R.f0 + f];
        R.qinfo[f].capped = 1;
        R.qinfo[f].lambda = R.sel2[j].lambda;
    }
    return 0;
}

static int round_enforce_group(htj2k_enc_ctx *c, Round &R);
static int round_xc_stats(htj2k_enc_ctx *c, Round &R, const std::vector<Over> &over);

/* The two enforce loops share their steps (rc_select_again, rc_collect, rc_code_again, rc_last_resort) and differ in
 * policy, which decides streams, so they stay two.  round_enforce: every frame stands alone.  It measures only the
 * frames coded in the current launch, and a frame whose selection came back unchanged goes to the last resort at once
 * (rc_recode) while the other frames go on.  round_enforce_group: the sum binds the frames together.  It measures all
 * frames in every launch, and goes to the last resort only when no block of any frame changed.
 *
 * budgeted calls: RC_MAX_LAUNCHES launches at most, then blocks are left out; a call that succeeds never exceeds the budget.
 * (The frames a PSNR target kept inside the budget are measured once more and found to fit.) */
static int round_enforce(htj2k_enc_ctx *c, Round &R)
{
    std::vector<Over> over;
    if (R.group)
        return round_enforce_group(c, R);
    for (int launch = 1; R.budget; launch++) {
        ENC_OK(rc_measure(c, R, launch, over));
        if (over.empty())
            break;
        if (launch == RC_MAX_LAUNCHES) {
            for (Over &o : over)
                ENC_OK(rc_last_resort(c, R, o.f, o.f + 1, R.frame(o.f).target, &o.size));
            break;
        }
        if (R.xc && launch == 1)                       /* the first launch was the plain transcode: the tables come in now */
            ENC_OK(round_xc_stats(c, R, over));
        ENC_OK(rc_select_again(c, R, over));
        for (size_t j = 0; R.xc && launch == 1 && j < over.size(); j++)
            R.info[over[j].f].est_bytes = (int64_t)R.sel2[j].est + R.call.minsz[R.f0 + over[j].f];
        ENC_OK(rc_recode(c, R, launch, over));
    }
    return 0;
}

/* the group selection again: every coded block's estimates scaled by its own actual / estimated, the room down by the
 * overshoot, the floors as they stand.  `over`: the frames rc_select_again has just dealt with; their scales are set,
 * and R.sel_len no longer holds the estimates of what they were coded at */
static int group_select_again(htj2k_enc_ctx *c, Round &R, int64_t overshoot, const std::vector<Over> &over)
{
    std::vector<uint8_t> done((size_t)R.nf, 0);
    for (const Over &o : over)
        done[(size_t)o.f] = 1;
    for (int f = 0; f < R.nf; f++)
        if (!done[(size_t)f])
            rc_rescale(R, f);
    R.room = std::max<int64_t>(0, R.room - overshoot);
    HIP_OK(hipMemcpyAsync(c->rc.scale.p, R.rc_scale.data(), (size_t)R.nblk * 8, hipMemcpyHostToDevice, c->stream));
    ENC_OK(run_rc_group(c, R.chunks.size(), R.nf, R.maxpass(), R.room, 0));
    ENC_OK(rc_fetch_selection(c, R));
    c->group_ms += ev_ms(c->ev[EV_G0], c->ev[EV_G1]);
    return 0;
}

/* calls with a budget over the group: as round_enforce, on the frames' own caps and on the sum.  Frames over their cap
 * are selected again first (new floors); when the sum is over, the group is; both feed one launch */
static int round_enforce_group(htj2k_enc_ctx *c, Round &R)
{
    std::vector<int64_t> size((size_t)R.nf);
    std::vector<Over> over;
    for (int launch = 1;; launch++) {
        int64_t total = 0;
        over.clear();
        for (int f = 0; f < R.nf; f++) {
            if ((size[(size_t)f] = frame_size(c, R, f)) < 0)
                return (int)size[(size_t)f];
            total += size[(size_t)f];
            if (R.budget && size[(size_t)f] > R.frame(f).target)
                over.push_back(Over{ f, size[(size_t)f] });
        }
        if (over.empty() && total <= R.group)
            break;
        bool changed = false;
        if (launch < RC_MAX_LAUNCHES) {
            if (!over.empty()) {
                ENC_OK(rc_select_again(c, R, over));
                R.which.clear();
                for (const Over &o : over)
                    R.which.push_back(o.f);
                HIP_OK(hipMemcpyAsync(c->rc.which.p, R.which.data(), R.which.size() * 4, hipMemcpyHostToDevice, c->stream));
                ENC_OK(run_rc_group_floors(c, (const int32_t *)c->rc.which.p, (int)R.which.size()));
            }
            std::vector<size_t> which;
            R.bt2.clear();
            if (total > R.group) {
                ENC_OK(group_select_again(c, R, total - R.group, over));
                for (int f = 0; f < R.nf; f++)
                    if (rc_collect(R, f, false, which))
                        R.info[f].ht_launches = launch + 1;
            } else {
                for (const Over &o : over)
                    if (rc_collect(R, o.f, false, which))
                        R.info[o.f].ht_launches = launch + 1;
            }
            changed = !which.empty();
            ENC_OK(rc_code_again(c, R, which, false));
            R.ginfo.ht_launches += changed;
        }
        if (changed)
            continue;
        /* after the third launch, or the same selection again: blocks are left out, per frame and then across the group */
        for (const Over &o : over)
            ENC_OK(rc_last_resort(c, R, o.f, o.f + 1, R.frame(o.f).target, &size[(size_t)o.f]));
        total = 0;
        for (int f = 0; f < R.nf; f++)
            total += size[(size_t)f];
        if (total > R.group) {
            R.ginfo.last_resort = 1;
            ENC_OK(rc_last_resort(c, R, 0, R.nf, R.group, size.data()));
        }
        break;
    }
    return 0;
}

static int round_headers(htj2k_enc_ctx *c, Round &R)
{
    EncOut &o = R.o;
    o.size = R.out_base;
    for (int f = 0; f < R.nf; f++) {
        const EncFrame &F = R.frame(f);
        const int32_t *pl = R.cur_plane.data() + R.blk0[f];
        const size_t p0 = o.npc, at = (size_t)o.size;
        R.call.offsets[R.f0 + f] = at;
        ENC_OK(frame_write(c, R, f, &o));
        R.info[f].final_bytes = (int64_t)(o.size - at);
        if (R.budget && R.info[f].final_bytes > F.target)
            return HTJ2K_ERR_BUG;                      /* the sizes were checked in round_enforce: cannot happen */
        for (int i = 0; i < F.nblk; i++) {
            R.info[f].blocks_left_out += pl[i] < 0;
            R.info[f].blocks_recoded += R.recoded[(size_t)R.blk0[f] + i];
        }
        c->last_planes[(size_t)(R.f0 + f)].assign(pl, pl + F.nblk);
        std::vector<int> &lp = c->last_passes[(size_t)(R.f0 + f)];
        lp.assign((size_t)F.nblk, 1);
        for (int i = 0; R.multi && i < F.nblk; i++)
            if (R.res[(size_t)R.blk0[f] + i].lcup > 0)
                lp[i] = R.res[(size_t)R.blk0[f] + i].npasses;
        c->last_rc[(size_t)(R.f0 + f)] = R.info[f];
        if (R.qinfo[f].capped) {                       /* the model's PSNR of what the budget left */
            double d = 0;
            ENC_OK(frame_model_d(c, R, f, &d));
            R.qinfo[f].model_psnr = model_psnr(F, R.nc, d);
        }
        c->last_q[(size_t)(R.f0 + f)] = R.qinfo[f];
        for (size_t p = p0; p < o.npc; p++)
            if (o.pc[p].block >= 0)
                o.pc[p].block += R.blk0[f];
    }
    if (o.size > R.call.cap) {
        enc_log(c, 16, "encoder: the codestreams do not fit the output buffer\n");
        return HTJ2K_ERR_ENOSPC;
    }
    R.call.offsets[R.f0 + R.nf] = (size_t)o.size;
    if (R.group) {
        R.ginfo.final_bytes = (int64_t)(o.size - R.out_base);
        if (R.ginfo.final_bytes > R.group)
            return HTJ2K_ERR_BUG;                      /* the sum was checked in round_enforce_group: cannot happen */
        c->last_group = R.ginfo;
    }
    return 0;
}

static int round_gather(htj2k_enc_ctx *c, Round &R)
{
    const EncOut &o = R.o;
    R.gp.resize(o.npc);
    for (size_t p = 0; p < o.npc; p++) {
        const EncPiece &pc = o.pc[p];
        const bool coded = pc.block >= 0;              /* from a block's region of the pool, or from the literals */
        R.gp[p] = GatherPiece{ pc.dst - R.out_base, coded ? R.bt[(size_t)pc.block].out : pc.src, pc.len, coded };
    }
    const size_t bytes = (size_t)(o.size - R.out_base), np = R.gp.size();
    if (c->lit.ensure(o.nlit + 16) < 0 || c->pieces.ensure(np * sizeof(GatherPiece) + 16) < 0 ||
        (!R.call.out_on_device && c->out.ensure(bytes + 16) < 0))
        return HTJ2K_ERR_ENOMEM;
    uint8_t *dst = R.call.out_on_device ? R.call.out + R.out_base : (uint8_t *)c->out.p;
    HIP_OK(hipMemcpyAsync(c->lit.p, o.lit, o.nlit, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->pieces.p, R.gp.data(), np * sizeof(GatherPiece), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->ev[EV_T0], c->stream));
    for (size_t p0 = 0; p0 < np; p0 += 1u << 30)
        hipLaunchKernelGGL(k_enc_gather, dim3((unsigned)std::min(np - p0, (size_t)1 << 30)), dim3(256), 0, c->stream,
                           (const GatherPiece *)c->pieces.p + p0, (const uint8_t *)c->lit.p, (const uint8_t *)c->pool.p, dst);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(c->ev[EV_GATHERED], c->stream));
    if (!R.call.out_on_device)
        HIP_OK(hipMemcpyAsync(R.call.out + R.out_base, c->out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

/* transcoding: the tile-component planes of the round's sources into the component planes (behind the decoder's block
 * stage), and the block table with what the rule gives every block */
static int round_fetch(htj2k_enc_ctx *c, Round &R)
{
    int mw = 0, mh = 0;
    for (int f = 0; f < R.nf; f++) {
        const EncFrame &F = R.frame(f);
        const XcFrame &X = R.call.xc[R.f0 + f];
        const J2kPlan *pl = htj2k_xc_plan_(R.call.dec, R.f0 + f);
        if (!pl || pl->ntilecomps != F.ntiles * R.nc)
            return HTJ2K_ERR_BUG;
        for (int t = 0; t < F.ntiles; t++)
            for (int k = 0; k < R.nc; k++) {
                const htj2k_enc_tile &T = F.tile[t].t;
                const J2kTileComp &tc = pl->tilecomps[t * R.nc + k];
                const int w = T.x1[k] - T.x0[k], h = T.y1[k] - T.y0[k];
                const int32_t *src = htj2k_xc_plane_(R.call.dec, R.f0 + f, t * R.nc + k);
                if (!src || tc.comp != k || tc.tile != t || tc.w != w || tc.h != h || tc.x0 != T.x0[k] || tc.y0 != T.y0[k])
                    return HTJ2K_ERR_BUG;
                R.xp.push_back(XcPlane{ src, (int32_t *)c->coef.p + R.plane_at(f, k) + (size_t)T.y0[k] * F.cw[k] + T.x0[k],
                                        w, h, F.cw[k], 0 });
                mw = std::max(mw, w);
                mh = std::max(mh, h);
            }
        for (int i = 0; i < F.nblk; i++) {
            EncBlk &e = R.bt[(size_t)R.blk0[f] + i];
            e.plane = X.plane[i];
            e.npasses = X.passes[i] > 1 ? X.passes[i] | ENC_BLK_KEEP : 1;
        }
    }
    if (c->xc.ensure(R.xp.size() * sizeof(XcPlane) + 16) < 0)
        return HTJ2K_ERR_ENOMEM;
    HIP_OK(hipMemcpyAsync(c->xc.p, R.xp.data(), R.xp.size() * sizeof(XcPlane), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamWaitEvent(c->stream, R.call.dec_done, 0));
    HIP_OK(hipEventRecord(c->ev[EV_START], c->stream));
    for_z_chunks(R.xp.size(), [&](size_t z0, unsigned nz) {
        hipLaunchKernelGGL(k_xc_scatter, dim3((unsigned)((mw + 255) / 256), (unsigned)std::min(mh, XC_ROWS), nz), dim3(256), 0,
                           c->stream, (const XcPlane *)c->xc.p + z0);
    });
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(c->ev[EV_UNPACKED], c->stream));
    HIP_OK(hipEventRecord(c->ev[EV_TRANSFORMED], c->stream));
    return 0;
}

/* ... and behind round_code the plane every block was coded from: the rule's, or, for a block that fell back to one
 * pass, its cleanup plane (the encoder's own fall-back codes the plane below: k_ht_refine_plan, ENC_BLK_KEEP) */
static void round_xc_planes(Round &R)
{
    for (int f = 0; f < R.nf; f++) {
        const XcFrame &X = R.call.xc[R.f0 + f];
        for (int i = 0; i < R.frame(f).nblk; i++) {
            const size_t b = (size_t)R.blk0[f] + i;
            R.cur_plane[b] = X.plane[i] + (X.passes[i] > 1 && X.plane[i] >= 0 && R.res[b].npasses == 1);
        }
    }
}

/* A budget per frame (htj2k_transcode_opts.target_bytes), when some frame of the round came out over it (`over`,
 * round_enforce): the statistics of every block of the round over |index| >> pr, pr the plane of its source's last pass,
 * so that the tables hold the source's form and everything coarser and nothing finer (k_xc_limit); the weight of a block
 * is its band's times 4^pr.  The coded blocks' scales follow from their bytes over the estimate of their own form
 * (rc_select_again), and from there on the frames over their budget are budgeted frames behind their first launch */
static int round_xc_stats(htj2k_enc_ctx *c, Round &R, const std::vector<Over> &over)
{
    const size_t nb = (size_t)R.nblk + 1;
    if (c->rc.ensure(R.nblk, R.nf, true) < 0 || c->rc.ensure_xc(R.nblk) < 0 || c->rc.blk2.ensure(nb * sizeof(EncBlk)) < 0 ||
        c->rc.res2.ensure(nb * sizeof(EncRes)) < 0)
        return HTJ2K_ERR_ENOMEM;
    R.xbase.assign(nb, 0);
    R.xpass.assign(nb, 0);
    R.xzero.assign(nb, 0);
    R.rc_w.assign(nb, 0.0);
    R.rc_scale.assign(nb, 1.0);
    R.rc_fr.resize((size_t)R.nf);
    for (int f = 0; f < R.nf; f++) {
        const EncFrame &F = R.frame(f);
        const XcFrame &X = R.call.xc[R.f0 + f];
        for (int i = 0; i < F.nblk; i++) {
            const size_t b = (size_t)R.blk0[f] + i;
            if (X.plane[i] < 0)
                continue;
            R.xbase[b] = X.plane[i];
            R.xpass[b] = X.passes[i];
            R.xzero[b] = R.res[b].lcup == 0;
            R.rc_w[b] = ldexp(enc_block_weight(&F, &F.blk[i]), 2 * X.plane[i]);
        }
        R.rc_fr[f] = RcFrame{ R.blk0[f], F.nblk, F.target - R.call.minsz[R.f0 + f], 0, 0 };
    }
    for (const Over &o : over)
        R.info[o.f].trial = 0;
    HIP_OK(hipMemcpyAsync(c->rc.xbase.p, R.xbase.data(), (size_t)R.nblk * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.xpass.p, R.xpass.data(), (size_t)R.nblk * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->rc.w.p, R.rc_w.data(), (size_t)R.nblk * 8, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->ev[EV_T0], c->stream));
    ENC_OK(run_rc_stats(c, R.nblk, RC_PLANES, (const int32_t *)c->rc.xbase.p));
    HIP_OK(hipEventRecord(c->ev[EV_T1], c->stream));
    ENC_OK(run_rc_stats_passes(c, R.nblk, RC_PLANES, (const int32_t *)c->rc.xbase.p));
    HIP_OK(hipEventRecord(c->ev[EV_STATS2], c->stream));
    ENC_OK(run_xc_limit(c, R.nblk));
    HIP_OK(hipEventRecord(c->ev[EV_SELECTED], c->stream));
    HIP_OK(hipMemcpyAsync(R.sel_len.data(), c->rc.sel_len.p, (size_t)R.nblk * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    c->rc_ms[0] += ev_ms(c->ev[EV_T0], c->ev[EV_T1]);
    c->ref_ms[1] += ev_ms(c->ev[EV_T1], c->ev[EV_STATS2]);
    c->rc_ms[1] += ev_ms(c->ev[EV_STATS2], c->ev[EV_SELECTED]);
    return 0;
}

static int transcode_round(htj2k_enc_ctx *c, const Call &call, int f0, int f1, uint64_t *at)
{
    Round R(call, f0, f1, *at);
    ENC_OK(round_layout(c, R));
    StreamWait wait{ c->stream };
    ENC_OK(round_fetch(c, R));
    ENC_OK(round_block_table(c, R));
    ENC_OK(round_code(c, R));
    round_xc_planes(R);
    for (int f = 0; R.budget && f < R.nf; f++)
        R.info[f].trial = 1;                           /* the source's own form is the trial; a frame that fits is final */
    ENC_OK(round_enforce(c, R));
    ENC_OK(round_headers(c, R));
    ENC_OK(round_gather(c, R));
    ENC_OK(wait.sync());
    c->ms[3] += ev_ms(c->ev[EV_T0], c->ev[EV_GATHERED]);
    *at = R.o.size;
    return 0;
}

static void reset_call_stats(htj2k_enc_ctx *c, int n)
{
    memset(c->ms, 0, sizeof c->ms);
    memset(c->rc_ms, 0, sizeof c->rc_ms);
    c->ref_ms[0] = c->ref_ms[1] = 0;
    c->q_ms[0] = c->q_ms[1] = 0;
    c->group_ms = 0;
    c->last_group = htj2k_enc_group();
    memset(c->ref_cycles, 0, sizeof c->ref_cycles);
    c->ref_stamped = 0;
    memset(c->cycles, 0, sizeof c->cycles);
    c->stamped = 0;
    c->last_planes.assign((size_t)n, std::vector<int>());
    c->last_passes.assign((size_t)n, std::vector<int>());
    c->last_rc.assign((size_t)n, htj2k_enc_rc());
    c->last_q.assign((size_t)n, htj2k_enc_quality());
    c->rounds = 0;
}

extern "C" int htj2k_enc_last_rounds(htj2k_enc_ctx *c) { return c ? c->rounds : HTJ2K_ERR_EINVAL; }

extern "C" void htj2k_transcode_opts_default(htj2k_transcode_opts *o)
{
    if (o) {
        memset(o, 0, sizeof *o);
        o->target_bytes = 0;
        o->ht_sources = 0;
    }
}

extern "C" int htj2k_transcode_batch(htj2k_ctx *dec, htj2k_enc_ctx *c, const uint8_t *const *pkts, const int *pkt_sizes, int n,
                                     uint8_t *out, size_t cap, int out_on_device, size_t *offsets)
{
    return htj2k_transcode_batch_opts(dec, c, pkts, pkt_sizes, n, nullptr, out, cap, out_on_device, offsets);
}

extern "C" int htj2k_transcode_batch_opts(htj2k_ctx *dec, htj2k_enc_ctx *c, const uint8_t *const *pkts, const int *pkt_sizes, int n,
                                          const htj2k_transcode_opts *opts, uint8_t *out, size_t cap, int out_on_device,
                                          size_t *offsets)
{
    const int64_t target = opts ? opts->target_bytes : 0;
    const int ht_sources = opts ? opts->ht_sources : 0;
    if (!dec || !c || !pkts || !pkt_sizes || n < 1 || !out || !offsets)
        return HTJ2K_ERR_EINVAL;
    ENC_OK(xc_ht_sources_ok(ht_sources, enc_log, c));
    if (target < 0) {
        enc_log(c, 16, "transcode: a budget is not negative\n");
        return HTJ2K_ERR_EINVAL;
    }
    for (int i = 0; i < n; i++)
        if (!pkts[i] || pkt_sizes[i] < 1)
            return HTJ2K_ERR_EINVAL;
    if (htj2k_xc_device_(dec) != c->device) {
        enc_log(c, 16, "transcode: the decoder and the encoder context are on different devices\n");
        return HTJ2K_ERR_EINVAL;
    }
    HIP_OK(hipSetDevice(c->device));
    /* every source is parsed and checked before anything runs: a call is refused whole */
    ENC_OK(htj2k_xc_parse_(dec, pkts, pkt_sizes, n, enc_log, c));
    std::vector<XcFrame> xf((size_t)n);
    std::vector<EncFrame> fr((size_t)n);
    std::vector<int64_t> minsz((size_t)n, 0);
    int r = 0, made = 0;
    for (int i = 0; i < n && !r; i++)
        if ((r = xc_frame_init(&xf[i], htj2k_xc_parser_(dec, i), htj2k_xc_plan_(dec, i), ht_sources, enc_log, c)) == 0) {
            xf[i].f.target = target;
            fr[made++] = xf[i].f;
        }
    /* a budget: the bands' weights, and no frame's smallest stream beyond it; nothing has run yet */
    for (int i = 0; i < made && !r && target > 0; i++) {
        if ((r = enc_rc_weights(&xf[i].f)) < 0)
            break;
        fr[i] = xf[i].f;
        if ((minsz[i] = enc_min_size(&fr[i])) < 0) {
            r = (int)minsz[i];
        } else if (target < minsz[i]) {
            char msg[160];
            snprintf(msg, sizeof msg, "transcode: a budget of %lld bytes is below the frame's smallest stream (%lld bytes of headers and empty packets)\n",
                     (long long)target, (long long)minsz[i]);
            enc_log(c, 16, msg);
            r = HTJ2K_ERR_EINVAL;
        }
    }
    void *done = nullptr;
    c->xc_ms = 0;
    if (!r) {
        const int bad = htj2k_xc_run_(dec, &done, &c->xc_ms);
        if (bad > 0) {
            char msg[128];
            snprintf(msg, sizeof msg, "transcode: %d code-blocks of the sources failed to decode\n", bad);
            enc_log(c, 16, msg);
        }
        r = bad < 0 ? bad : bad > 0 ? HTJ2K_ERR_INVALIDDATA : 0;
    }
    reset_call_stats(c, n);
    Call call = { nullptr, fr.data(), minsz.data(), 1, out_on_device, out, cap, offsets };
    call.xc = xf.data();
    call.dec = dec;
    call.dec_done = (hipEvent_t)done;
    uint64_t at = 0;
    for (int f0 = 0; f0 < n && !r;) {
        size_t ns = 0;
        int f1 = f0;
        while (f1 < n && fr[f1].ncomp == fr[f0].ncomp) {   /* a round's frames have their planes laid out alike */
            size_t s = 0;
            for (int k = 0; k < fr[f1].ncomp; k++)
                s += (size_t)fr[f1].cw[k] * fr[f1].ch[k];
            if (f1 > f0 && ns + s > c->round_samples)
                break;
            ns += s;
            f1++;
        }
        r = transcode_round(c, call, f0, f1, &at);
        c->rounds++;
        f0 = f1;
    }
    for (int i = 0; i < made; i++)
        xc_frame_free(&xf[i]);
    return r;
}

extern "C" int htj2k_transcode_frame(htj2k_ctx *dec, htj2k_enc_ctx *c, const uint8_t *pkt, int pkt_size,
                                     uint8_t *out, size_t cap, size_t *out_len)
{
    size_t off[2] = { 0, 0 };
    const uint8_t *pk[1] = { pkt };
    int sz[1] = { pkt_size };
    int r = htj2k_transcode_batch(dec, c, pk, sz, 1, out, cap, 0, off);
    if (out_len)
        *out_len = r < 0 ? 0 : off[1];
    return r;
}

extern "C" int htj2k_transcode_frame_opts(htj2k_ctx *dec, htj2k_enc_ctx *c, const uint8_t *pkt, int pkt_size,
                                          const htj2k_transcode_opts *opts, uint8_t *out, size_t cap, size_t *out_len)
{
    size_t off[2] = { 0, 0 };
    const uint8_t *pk[1] = { pkt };
    int sz[1] = { pkt_size };
    int r = htj2k_transcode_batch_opts(dec, c, pk, sz, 1, opts, out, cap, 0, off);
    if (out_len)
        *out_len = r < 0 ? 0 : off[1];
    return r;
}

extern "C" int htj2k_transcode_stage_ms(htj2k_enc_ctx *c, float ms[4])
{
    if (!c || !ms)
        return HTJ2K_ERR_EINVAL;
    ms[0] = c->xc_ms;
    ms[1] = c->ms[0];
    ms[2] = c->ms[2] + c->ref_ms[0];
    ms[3] = c->ms[3];
    return 0;
}

/* one round: frames [f0, f1) of the call, their codestreams from byte *at of the output on; *at moves behind them */
static int encode_round(htj2k_enc_ctx *c, const Call &call, int f0, int f1, uint64_t *at)
{
    Round R(call, f0, f1, *at);
    ENC_OK(round_layout(c, R));
    StreamWait wait{ c->stream };                      /* behind R: the stream is idle before R's memory goes */
    ENC_OK(round_unpack(c, R));
    ENC_OK(round_block_table(c, R));                   /* before the transform: k_rc_base97 reads it ahead of the quantiser */
    ENC_OK(round_transform(c, R));
    ENC_OK(round_select(c, R));
    ENC_OK(round_code(c, R));
    ENC_OK(round_cap(c, R));
    ENC_OK(round_enforce(c, R));
    ENC_OK(round_headers(c, R));
    ENC_OK(round_gather(c, R));
    ENC_OK(wait.sync());
    c->ms[3] += ev_ms(c->ev[EV_T0], c->ev[EV_GATHERED]);
    *at = R.o.size;
    return 0;
}

/* htj2k_encode_batch; quality: NULL, or per frame the PSNR target that takes the place of opts->target_psnr (every one > 0:
 * the rounds of htj2k_encode_batch_measured, whose frames each carry a target of their own) */
static int encode_batch(htj2k_enc_ctx *c, const htj2k_frame *in, int n, int bits, const htj2k_enc_opts *opts, const double *quality,
                        int in_on_device, uint8_t *out, size_t cap, int out_on_device, size_t *offsets, const TensorIn *tensor = nullptr)
{
    if (!c || !in || n < 1 || !out || !offsets)
        return HTJ2K_ERR_EINVAL;
    c->last_ssim.clear();                              /* a measured call fills it once its streams are final */
    HIP_OK(hipSetDevice(c->device));
    /* every frame of the call is checked here, so that a call is refused before any of its rounds runs */
    std::vector<EncFrame> fr((size_t)n);
    int r = 0, made = 0;
    for (int i = 0; i < n && !r; i++) {
        if (in[i].pix_fmt != in[0].pix_fmt) {
            enc_log(c, 16, "encoder: the frames of a batch share one layout\n");
            r = HTJ2K_ERR_EINVAL;
            break;
        }
        if ((r = enc_frame_init(&fr[i], in[i].width, in[i].height, in[i].pix_fmt, bits, opts, enc_log, c)) == 0) {
            made++;
            if (quality)
                fr[i].quality = quality[i];
        }
    }
    /* a budget below the frame's smallest stream */
    std::vector<int64_t> minsz((size_t)n, 0);
    for (int i = 0; i < made && !r && (fr[i].target > 0 || fr[i].quality > 0 || fr[i].group > 0); i++) {
        if ((minsz[i] = enc_min_size(&fr[i])) < 0) {
            r = (int)minsz[i];
        } else if (fr[i].target > 0 && fr[i].target < minsz[i]) {
            char msg[160];
            snprintf(msg, sizeof msg, "encoder: a budget of %lld bytes is below the frame's smallest stream (%lld bytes of headers and empty packets)\n",
                     (long long)fr[i].target, (long long)minsz[i]);
            enc_log(c, 16, msg);
            r = HTJ2K_ERR_EINVAL;
        }
    }
    /* a budget over the group: not with a PSNR target, not below the sum of the smallest streams, and one round */
    if (!r && made == n && fr[0].group > 0) {
        int64_t least = 0;
        size_t samples = 0;
        char msg[200];
        for (int i = 0; i < n; i++) {
            least += minsz[i];
            for (int k = 0; k < fr[i].ncomp; k++)
                samples += (size_t)fr[i].cw[k] * fr[i].ch[k];
        }
        if (fr[0].quality > 0) {
            enc_log(c, 16, "encoder: group_bytes does not go with target_psnr\n");
            r = HTJ2K_ERR_EINVAL;
        } else if (fr[0].group < least) {
            snprintf(msg, sizeof msg, "encoder: a group budget of %lld bytes is below the sum of the frames' smallest streams (%lld bytes)\n",
                     (long long)fr[0].group, (long long)least);
            enc_log(c, 16, msg);
            r = HTJ2K_ERR_EINVAL;
        } else if (n > 1 && samples > c->round_samples) {
            snprintf(msg, sizeof msg, "encoder: a group is selected in one round: the call has %zu samples, a round takes %zu\n",
                     samples, c->round_samples);
            enc_log(c, 16, msg);
            r = HTJ2K_ERR_EINVAL;
        }
    }
    /* the planes the layout reads: present, linesize not negative and not below the row */
    for (int i = 0; i < made && !r && !tensor; i++)
        for (int p = 0; p < in_planes(fr[i]) && !r; p++)
            if (!in[i].data[p] || in[i].linesize[p] < 0 || (size_t)in[i].linesize[p] < in_row(fr[i], p)) {
                enc_log(c, 16, "encoder: a plane is missing or its linesize is negative or too short\n");
                r = HTJ2K_ERR_EINVAL;
            }
    reset_call_stats(c, n);
    Call call = { in, fr.data(), minsz.data(), in_on_device, out_on_device, out, cap, offsets };
    call.tensor = tensor;
    uint64_t at = 0;
    for (int f0 = 0; f0 < n && !r;) {
        size_t ns = 0;
        int f1 = f0;
        while (f1 < n) {
            size_t s = 0;
            for (int k = 0; k < fr[f1].ncomp; k++)
                s += (size_t)fr[f1].cw[k] * fr[f1].ch[k];
            if (f1 > f0 && ns + s > c->round_samples)
                break;
            ns += s;
            f1++;
        }
        r = encode_round(c, call, f0, f1, &at);
        c->rounds++;
        f0 = f1;
    }
    for (int i = 0; i < made; i++)
        enc_frame_free(&fr[i]);
    return r;
}

extern "C" int htj2k_encode_batch(htj2k_enc_ctx *c, const htj2k_frame *in, int n, int bits, const htj2k_enc_opts *opts,
                                  int in_on_device, uint8_t *out, size_t cap, int out_on_device, size_t *offsets)
{
    return encode_batch(c, in, n, bits, opts, nullptr, in_on_device, out, cap, out_on_device, offsets);
}

/* htj2k_encode_tensor_curves (htj2k_encode_tensor_mix is it with NULL curves, htj2k_encode_tensor with a NULL mix as well): the refusals of its own arguments, then encode_batch over n frames that have a size and a layout
 * but no planes; the unpack stage reads the tensor (round_unpack_tensor) */
extern "C" int htj2k_encode_tensor_curves(htj2k_enc_ctx *c, const void *src, size_t src_bytes, int n, int width, int height, int pix_fmt,
                                          int bits, const htj2k_tensor_spec *spec, const htj2k_tensor_mix_in *mix,
                                          const htj2k_tensor_curves_in *curves, const htj2k_enc_opts *opts,
                                          uint8_t *out, size_t cap, int out_on_device, size_t *offsets)
{
    if (!src || !spec || !out || !offsets || n < 1 || width < 1 || height < 1)
        return HTJ2K_ERR_EINVAL;
    size_t image_bytes = 0;
    const int r = htj2k_tensor_image_size_curves_in_(pix_fmt, width, height, bits, spec, mix, curves, nullptr, &image_bytes);   /* layout, bits, dtype, layout, scale and bias or the mix, the curves */
    if (r < 0)
        return r;
    if (spec->out_w || spec->out_h)
        return HTJ2K_ERR_EINVAL;
    if (src_bytes / image_bytes < (size_t)n || (uintptr_t)src % (spec->dtype == HTJ2K_TENSOR_F32 ? 4 : 2))
        return HTJ2K_ERR_EINVAL;
    if (!c)
        return HTJ2K_ERR_ENOSYS;
    TensorIn T = { (const uint8_t *)src, image_bytes, spec->dtype, spec->layout == HTJ2K_TENSOR_NHWC, {}, {}, mix, curves };
    for (int k = 0; k < 4; k++) {
        T.scale[k] = spec->scale[k];
        T.bias[k] = spec->bias[k];
    }
    std::vector<htj2k_frame> in((size_t)n);
    for (htj2k_frame &f : in) {
        memset(&f, 0, sizeof f);
        f.width = width;
        f.height = height;
        f.pix_fmt = pix_fmt;
    }
    return encode_batch(c, in.data(), n, bits, opts, nullptr, 1, out, cap, out_on_device, offsets, &T);
}

extern "C" int htj2k_encode_tensor_mix(htj2k_enc_ctx *c, const void *src, size_t src_bytes, int n, int width, int height, int pix_fmt,
                                       int bits, const htj2k_tensor_spec *spec, const htj2k_tensor_mix_in *mix, const htj2k_enc_opts *opts,
                                       uint8_t *out, size_t cap, int out_on_device, size_t *offsets)
{
    return htj2k_encode_tensor_curves(c, src, src_bytes, n, width, height, pix_fmt, bits, spec, mix, nullptr, opts, out, cap, out_on_device, offsets);
}

extern "C" int htj2k_encode_tensor(htj2k_enc_ctx *c, const void *src, size_t src_bytes, int n, int width, int height, int pix_fmt,
                                   int bits, const htj2k_tensor_spec *spec, const htj2k_enc_opts *opts, uint8_t *out, size_t cap,
                                   int out_on_device, size_t *offsets)
{
    return htj2k_encode_tensor_mix(c, src, src_bytes, n, width, height, pix_fmt, bits, spec, nullptr, opts, out, cap, out_on_device, offsets);
}

/* ------------------------------------------------------------------ measured quality
 * htj2k_encode_batch_measured: the streams of htj2k_encode_batch, decoded by the product decoder as jobs on its device and
 * compared with the input where it lies (htj2k_job_compare); with close_loop the frames that measure short of target_psnr
 * are encoded again with a moved target.  The loop adds no coding path: every round is encode_batch. */
#define MEAS_STEP_DB        0.05       /* the least a correction moves a frame's target */
#define MEAS_ROUNDS_DEFAULT 8          /* the worst case over the 24 cases of tests/test_encode_measured_gpu.py, 7, plus one */

static size_t frame_samples(const htj2k_frame &f, int pix_fmt)
{
    const J2kPixDesc *pd = j2k_pix_desc(pix_fmt);
    size_t s = 0;
    for (int k = 0; pd && k < pd->nb_components; k++) {
        const int chroma = k == 1 || k == 2;
        s += (size_t)((f.width + (1 << (chroma ? pd->log2_chroma_w : 0)) - 1) >> (chroma ? pd->log2_chroma_w : 0)) *
             (size_t)((f.height + (1 << (chroma ? pd->log2_chroma_h : 0)) - 1) >> (chroma ? pd->log2_chroma_h : 0));
    }
    return s;
}

/* decodes streams[i] (host memory) on `dec` and compares them with in[i]: chunks of frames bounded by the encoder's round;
 * ssim (NULL without the switch): the same jobs once more through htj2k_job_compare_ssim */
static int measure_streams(htj2k_ctx *dec, htj2k_enc_ctx *c, const htj2k_frame *in, int n, int bits, int in_on_device,
                           const uint8_t *const *streams, const size_t *sizes, htj2k_frame_diff *diff, htj2k_frame_ssim *ssim)
{
    std::vector<std::vector<uint8_t>> padded;          /* a packet carries 64 bytes of zero padding */
    std::vector<const uint8_t *> pk;
    std::vector<int> sz;
    for (int f0 = 0; f0 < n;) {
        size_t ns = 0;
        int f1 = f0;
        while (f1 < n) {
            const size_t s = frame_samples(in[f1], in[0].pix_fmt);
            if (f1 > f0 && ns + s > c->round_samples)
                break;
            ns += s;
            f1++;
        }
        padded.assign((size_t)(f1 - f0), std::vector<uint8_t>());
        pk.clear();
        sz.clear();
        for (int i = f0; i < f1; i++) {
            if (sizes[i] > (size_t)INT32_MAX)
                return HTJ2K_ERR_PATCHWELCOME;
            std::vector<uint8_t> &p = padded[(size_t)(i - f0)];
            p.assign(sizes[i] + 64, 0);
            memcpy(p.data(), streams[i], sizes[i]);
            pk.push_back(p.data());
            sz.push_back((int)sizes[i]);
        }
        htj2k_job *job = nullptr;
        ENC_OK(htj2k_meas_decode_(dec, pk.data(), sz.data(), f1 - f0, in[0].pix_fmt, &job));
        const int r = htj2k_job_compare(dec, job, in + f0, in_on_device, bits, diff + f0);
        if (r < 0)
            return r == HTJ2K_ERR_EINVAL ? HTJ2K_ERR_BUG : r;          /* the decoder's frame is not the input's shape */
        if (ssim)
            ENC_OK(htj2k_job_compare_ssim(dec, job, in + f0, in_on_device, bits, ssim + f0));
        f0 = f1;
    }
    HIP_OK(hipSetDevice(c->device));
    return 0;
}

extern "C" int htj2k_encode_batch_measured(htj2k_ctx *dec, htj2k_enc_ctx *c, const htj2k_frame *in, int n, int bits,
                                           const htj2k_enc_opts *opts, const htj2k_enc_measure_opts *mopts, int in_on_device,
                                           uint8_t *out, size_t cap, int out_on_device, size_t *offsets, htj2k_enc_measured *res)
{
    if (!in || n < 1 || !out || !offsets || !res)
        return HTJ2K_ERR_EINVAL;
    if (mopts && (mopts->close_loop < 0 || mopts->close_loop > 1 || mopts->max_rounds < 0 || mopts->max_rounds > 16))
        return HTJ2K_ERR_EINVAL;
    if (!dec || !c)
        return HTJ2K_ERR_ENOSYS;
    if (htj2k_meas_reduction_(dec)) {
        enc_log(c, 16, "measured encode: a reduction factor on the decoder decodes another picture than the input\n");
        return HTJ2K_ERR_PATCHWELCOME;
    }
    if (htj2k_xc_device_(dec) != c->device) {
        enc_log(c, 16, "measured encode: the decoder and the encoder are on different devices\n");
        return HTJ2K_ERR_EINVAL;
    }
    htj2k_enc_opts o;
    enc_opts_resolve(opts, &o);
    const double T = o.target_psnr;
    const bool loop = mopts && mopts->close_loop && T > 0;
    const int max_rounds = mopts && mopts->max_rounds ? mopts->max_rounds : MEAS_ROUNDS_DEFAULT;
    std::vector<htj2k_frame_diff> diff((size_t)n);
    std::vector<htj2k_frame_ssim> ssim(c->measure_ssim ? (size_t)n : 0), ssim_final(ssim.size());
    htj2k_frame_ssim *const sp_ssim = c->measure_ssim ? ssim.data() : nullptr;
    std::vector<const uint8_t *> sp((size_t)n);
    std::vector<size_t> ss((size_t)n);
    memset(res, 0, (size_t)n * sizeof *res);

    if (!loop) {                                       /* report only: htj2k_encode_batch as it is, then the measurement */
        ENC_OK(encode_batch(c, in, n, bits, opts, nullptr, in_on_device, out, cap, out_on_device, offsets));
        std::unique_ptr<uint8_t[]> host;
        const uint8_t *base = out;
        if (out_on_device) {                           /* the parser reads host memory */
            host.reset(new (std::nothrow) uint8_t[offsets[n] + 1]);
            if (!host)
                return HTJ2K_ERR_ENOMEM;
            HIP_OK(hipMemcpy(host.get(), out, offsets[n], hipMemcpyDeviceToHost));
            base = host.get();
        }
        for (int i = 0; i < n; i++) {
            sp[i] = base + offsets[i];
            ss[i] = offsets[i + 1] - offsets[i];
        }
        ENC_OK(measure_streams(dec, c, in, n, bits, in_on_device, sp.data(), ss.data(), diff.data(), sp_ssim));
        c->last_ssim.swap(ssim);
        for (int i = 0; i < n; i++) {
            res[i].diff = diff[i];
            res[i].first_psnr = diff[i].psnr;
            res[i].target_used = T;
            res[i].rounds = 1;
            res[i].short_measured = T > 0 && !(diff[i].psnr >= T);
        }
        return 0;
    }

    /* closing the loop.  Every round is a batch of the frames still short, each with its own target, into a buffer of ours;
     * a frame's stream, measurement and records are those of the last round it took part in */
    size_t bound = 0;
    for (int i = 0; i < n; i++)
        bound += htj2k_encode_bound(in[i].width, in[i].height, in[0].pix_fmt, bits, opts);
    std::unique_ptr<uint8_t[]> buf(new (std::nothrow) uint8_t[bound + 1]);     /* (not cleared: only what a round writes is touched) */
    if (!buf)
        return HTJ2K_ERR_ENOMEM;
    std::vector<std::vector<uint8_t>> stream((size_t)n);
    std::vector<std::vector<int>> planes((size_t)n), passes((size_t)n);
    std::vector<htj2k_enc_rc> rcs((size_t)n);
    std::vector<htj2k_enc_quality> qs((size_t)n);
    std::vector<double> target((size_t)n, T);
    std::vector<int> todo((size_t)n);
    for (int i = 0; i < n; i++)
        todo[(size_t)i] = i;
    int total_rounds = 0;
    for (int round = 1; !todo.empty(); round++) {
        const bool fall_back = round > max_rounds;     /* still short: once more without the target, the finest the options allow */
        const int k = (int)todo.size();
        std::vector<htj2k_frame> sub((size_t)k);
        std::vector<double> q((size_t)k);
        std::vector<size_t> off((size_t)k + 1);
        for (int j = 0; j < k; j++) {
            sub[(size_t)j] = in[todo[(size_t)j]];
            q[(size_t)j] = target[(size_t)todo[(size_t)j]];
        }
        htj2k_enc_opts ro = o;
        if (fall_back)
            ro.target_psnr = 0;
        ENC_OK(encode_batch(c, sub.data(), k, bits, &ro, fall_back ? nullptr : q.data(), in_on_device, buf.get(), bound, 0, off.data()));
        total_rounds += c->rounds;
        for (int j = 0; j < k; j++) {
            sp[(size_t)j] = buf.get() + off[(size_t)j];
            ss[(size_t)j] = off[(size_t)j + 1] - off[(size_t)j];
        }
        ENC_OK(measure_streams(dec, c, sub.data(), k, bits, in_on_device, sp.data(), ss.data(), diff.data(), sp_ssim));
        std::vector<int> next;
        for (int j = 0; j < k; j++) {
            const size_t i = (size_t)todo[(size_t)j];
            if (sp_ssim)
                ssim_final[i] = ssim[(size_t)j];
            const double m = diff[(size_t)j].psnr;
            stream[i].assign(sp[(size_t)j], sp[(size_t)j] + ss[(size_t)j]);
            planes[i] = c->last_planes[(size_t)j];
            passes[i] = c->last_passes[(size_t)j];
            rcs[i] = c->last_rc[(size_t)j];
            qs[i] = c->last_q[(size_t)j];
            res[i].diff = diff[(size_t)j];
            if (round == 1)
                res[i].first_psnr = m;
            res[i].rounds = fall_back ? res[i].rounds : round;
            res[i].fell_back = fall_back;
            res[i].target_used = fall_back ? 0 : target[i];
            res[i].short_measured = !(m >= T);
            /* final: the target holds in pixels, the budget decided, or the stream is the plane-0 stream already */
            if (fall_back || m >= T || qs[i].capped || qs[i].short_of_target)
                continue;
            target[i] += std::max(T - m, MEAS_STEP_DB);
            next.push_back((int)i);
        }
        todo.swap(next);
    }
    /* the records speak of every frame's final round; the streams back to back */
    c->last_planes.swap(planes);
    c->last_passes.swap(passes);
    c->last_rc.swap(rcs);
    c->last_q.swap(qs);
    c->rounds = total_rounds;
    offsets[0] = 0;
    for (int i = 0; i < n; i++)
        offsets[i + 1] = offsets[i] + stream[(size_t)i].size();
    if (offsets[n] > cap)
        return HTJ2K_ERR_ENOSPC;
    c->last_ssim.swap(ssim_final);
    for (int i = 0; i < n; i++) {
        if (out_on_device)
            HIP_OK(hipMemcpy(out + offsets[i], stream[(size_t)i].data(), stream[(size_t)i].size(), hipMemcpyHostToDevice));
        else
            memcpy(out + offsets[i], stream[(size_t)i].data(), stream[(size_t)i].size());
    }
    return 0;
}

extern "C" int htj2k_encode_frame(htj2k_enc_ctx *c, const htj2k_frame *in, int bits, const htj2k_enc_opts *opts,
                                  uint8_t *out, size_t cap, size_t *out_len)
{
    size_t off[2] = { 0, 0 };
    int r = htj2k_encode_batch(c, in, 1, bits, opts, 0, out, cap, 0, off);
    if (out_len)
        *out_len = r < 0 ? 0 : off[1];
    return r;
}
