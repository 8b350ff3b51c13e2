/*
 * htj2k_encode.hip -- device layer of the HTJ2K encoder: the htj2k_enc_* entry points of
 * include/htj2k_amd.h that need a GPU.
 *
 * A call encodes its frames in rounds of at most ENC_ROUND_SAMPLES samples (HTJ2K_ENC_ROUND in the
 * environment of htj2k_enc_open: fewer, for tests; a round takes at least one frame); every stage of a
 * round is one launch over its frames (descriptor tables, as the decoder's jobs):
 *
 *   upload (host input only) -> k_enc_unpack -> per level k_fdwt_v + k_fdwt_h -> k_ht_encode
 *   -> read back the per-block table (Lcup, largest U) -> host: guard bits, headers, packet
 *   headers (j2k_enc.c) -> k_enc_gather into the final codestreams -> D2H (host output only)
 *
 * With a byte budget (htj2k_enc_opts.target_bytes) k_rc_stats and k_rc_select run in front of
 * k_ht_encode and give every block the bit-plane it is coded from; the host then knows the exact
 * sizes, and frames that came out too large go through up to two correction rounds (select again
 * with the lengths rescaled, code the blocks whose plane changed) and, if that is not enough, a
 * last step on the host that leaves blocks out.  A call that succeeds never exceeds the budget.
 *
 * Irreversible (9/7) frames run k_enc_unpack<true> (float planes, ICT), per level k_fdwt97_v +
 * k_fdwt97_h, then k_quant97 (int32 indices in the same planes) before k_ht_encode; the rest is
 * shared.  Built with -ffp-contract=off: the float stages must round as the vector factory does.
 *
 * The kernels are in enc_kernels.hpp.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "j2k_plan.h"
#include "j2k_enc.h"
#include "enc_kernels.hpp"

using namespace htj2k_enc;

#define ENC_ROUND_SAMPLES ((size_t)1 << 30)    /* samples of all components of the frames of one round */
#define ENC_MAX_LEVELS    32
#define ENC_EVENTS        8
#define RC_MAX_LAUNCHES   3                    /* HT cleanup launches a budgeted round of frames may take */

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t n)
    {
        if (n <= cap)
            return 0;
        if (p)
            (void)hipFree(p);
        p = nullptr;
        cap = 0;
        n = (n + 0xFFFF) & ~(size_t)0xFFFF;
        if (hipMalloc(&p, n) != hipSuccess) {
            p = nullptr;
            return HTJ2K_ERR_ENOMEM;
        }
        cap = n;
        return 0;
    }
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct htj2k_enc_ctx {
    int device = 0;
    int max_dyn_lds = 64 * 1024;
    htj2k_log_fn log = nullptr;
    void *log_opaque = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[ENC_EVENTS] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    float ms[4] = { 0, 0, 0, 0 };
    float rc_ms[3] = { 0, 0, 0 };      /* k_rc_stats, k_rc_select, the HT launches of the correction rounds */
    std::vector<std::vector<int>> last_planes;   /* of the last batch, per frame */
    std::vector<htj2k_enc_rc> last_rc;
    int stamps = 0;                    /* HTJ2K_ENC_STAMPS=1: k_ht_encode records the clock at its phase boundaries */
    size_t round_samples = ENC_ROUND_SAMPLES;   /* HTJ2K_ENC_ROUND=n: samples per round (tests: several rounds of small frames) */
    uint64_t cycles[ENC_STAMPS - 1] = { 0, 0, 0, 0, 0 };
    uint64_t stamped = 0;
    uint16_t *d_tab = nullptr;
    DevBuf in, coef, tmp, pool, args, blk, res, lit, pieces, out, st;
    DevBuf rc_dist, rc_len, rc_dskip, rc_low, rc_kmax, rc_w, rc_scale, rc_planes, rc_sel_len, rc_frames, rc_sel, blk2, res2;
};

static void enc_log(void *opaque, int level, const char *msg)
{
    htj2k_enc_ctx *c = (htj2k_enc_ctx *)opaque;
    if (c && c->log)
        c->log(c->log_opaque, level, msg);
}

#define HIP_OK(x) do { if ((x) != hipSuccess) return HTJ2K_ERR_EXTERNAL; } while (0)

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
    uint16_t tab[2 * 8 * 16 * 16];
    enc_cxtvlc_table(tab);
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&c->d_tab, sizeof tab) != hipSuccess ||
        hipMemcpy(c->d_tab, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess) {
        htj2k_enc_close(c);
        return HTJ2K_ERR_ENOSYS;
    }
    for (int i = 0; i < ENC_EVENTS; i++)
        if (hipEventCreate(&c->ev[i]) != hipSuccess) {
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
    if (c->d_tab)
        (void)hipFree(c->d_tab);
    c->in.release(); c->coef.release(); c->tmp.release(); c->pool.release(); c->args.release();
    c->blk.release(); c->res.release(); c->lit.release(); c->pieces.release(); c->out.release(); c->st.release();
    c->rc_dist.release(); c->rc_len.release(); c->rc_dskip.release(); c->rc_low.release(); c->rc_kmax.release();
    c->rc_w.release(); c->rc_scale.release(); c->rc_planes.release(); c->rc_sel_len.release(); c->rc_frames.release();
    c->rc_sel.release(); c->blk2.release(); c->res2.release();
    if (c->stream)
        (void)hipStreamDestroy(c->stream);
    delete c;
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

extern "C" int htj2k_enc_last_planes(htj2k_enc_ctx *c, int frame, int *planes, int cap)
{
    if (!c || frame < 0 || (size_t)frame >= c->last_planes.size())
        return HTJ2K_ERR_EINVAL;
    const std::vector<int> &v = c->last_planes[(size_t)frame];
    for (int i = 0; planes && i < cap && (size_t)i < v.size(); i++)
        planes[i] = v[(size_t)i];
    return (int)v.size();
}

extern "C" int htj2k_enc_rc_info(htj2k_enc_ctx *c, int frame, htj2k_enc_rc *info)
{
    if (!c || !info || frame < 0 || (size_t)frame >= c->last_rc.size())
        return HTJ2K_ERR_EINVAL;
    *info = c->last_rc[(size_t)frame];
    return 0;
}

extern "C" int htj2k_enc_ht_cycles(htj2k_enc_ctx *c, uint64_t cycles[5])
{
    memcpy(cycles, c->cycles, sizeof c->cycles);
    return (int)(c->stamped > INT32_MAX ? INT32_MAX : c->stamped);
}

static size_t region(int w, int h) { return (enc_block_bound(w, h) + 15) & ~(size_t)15; }

/* the forward DWT of `planes` (full-size w x h each, in place, scratch alongside) at `levels` levels; the launch tables go
 * to c->args from byte `args_off` on (the caller has sized it for planes.size() * ENC_MAX_LEVELS entries) through `tab`,
 * which the caller keeps until the stream is synchronised */
static int run_fdwt(htj2k_enc_ctx *c, const std::vector<DwtPlane> &planes, const std::vector<int> &levels, size_t args_off,
                    std::vector<DwtPlane> &tab, bool irrev)
{
    int maxl = 0;
    for (int l : levels)
        maxl = l > maxl ? l : maxl;
    tab.clear();
    std::vector<size_t> off, cnt;
    std::vector<int> gx, gy;
    for (int l = 0; l < maxl; l++) {
        int mw = 0, mh = 0;
        off.push_back(tab.size());
        for (size_t i = 0; i < planes.size(); i++) {
            if (l >= levels[i])
                continue;
            DwtPlane d = planes[i];
            d.lw = (int32_t)(((int64_t)planes[i].lw + ((int64_t)1 << l) - 1) >> l);
            d.lh = (int32_t)(((int64_t)planes[i].lh + ((int64_t)1 << l) - 1) >> l);
            if (d.lw <= 1 && d.lh <= 1 && !irrev)
                continue;                             /* one sample: 5/3 leaves it as it is (9/7 scales it, every level) */
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
    for (int l = 0; l < maxl; l++) {
        for (size_t z0 = 0; z0 < cnt[l]; z0 += 65535) {
            const unsigned nz = (unsigned)(cnt[l] - z0 < 65535 ? cnt[l] - z0 : 65535);
            const dim3 grid((unsigned)gx[l], (unsigned)gy[l], nz);
            hipLaunchKernelGGL(irrev ? k_fdwt97_v : k_fdwt_v, grid, dim3(256), 0, c->stream, d_tab + off[l] + z0);
            hipLaunchKernelGGL(irrev ? k_fdwt97_h : k_fdwt_h, grid, dim3(256), 0, c->stream, d_tab + off[l] + z0);
        }
    }
    HIP_OK(hipGetLastError());
    return 0;
}

/* c->st must hold nblk * ENC_STAMPS words when c->stamps is set (sized with the other buffers, before any launch) */
static int run_ht(htj2k_enc_ctx *c, const EncBlk *d_blk, int nblk, const int32_t *d_coef, uint8_t *d_pool, EncRes *d_res)
{
    if (ENC_LDS_BYTES > c->max_dyn_lds) {
        enc_log(c, 16, "encoder: the HT kernel needs more LDS than a workgroup may have\n");
        return HTJ2K_ERR_PATCHWELCOME;
    }
    uint64_t *st = c->stamps ? (uint64_t *)c->st.p : nullptr;
    if (st)
        HIP_OK(hipMemsetAsync(st, 0, (size_t)nblk * ENC_STAMPS * sizeof(uint64_t), c->stream));
    if (nblk > 0)
        hipLaunchKernelGGL(k_ht_encode, dim3((unsigned)nblk), dim3(64), ENC_LDS_BYTES, c->stream, d_blk, d_coef, d_pool, d_res,
                           (const uint16_t *)c->d_tab, st);
    HIP_OK(hipGetLastError());
    return 0;
}

/* after the stream is synchronised: the phase cycles of the last k_ht_encode, summed over the coded blocks */
static int collect_stamps(htj2k_enc_ctx *c, int nblk)
{
    if (!c->stamps || nblk <= 0)
        return 0;
    std::vector<uint64_t> v((size_t)nblk * ENC_STAMPS);
    HIP_OK(hipMemcpy(v.data(), c->st.p, v.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < nblk; i++) {
        const uint64_t *t = &v[(size_t)i * ENC_STAMPS];
        if (!t[ENC_STAMPS - 1])
            continue;                                  /* all-zero block: left before the phases */
        for (int k = 0; k < ENC_STAMPS - 1; k++)
            c->cycles[k] += t[k + 1] - t[k];
        c->stamped++;
    }
    return 0;
}

static int ensure_stamps(htj2k_enc_ctx *c, int nblk)
{
    return c->stamps ? c->st.ensure((size_t)(nblk + 1) * ENC_STAMPS * sizeof(uint64_t)) : 0;
}

extern "C" int htj2k_fdwt_plane(htj2k_enc_ctx *c, int32_t *plane, int w, int h, int levels)
{
    if (!c || !plane || w < 1 || h < 1 || w > 32768 || h > 32768 || levels < 0 || levels > 32)
        return HTJ2K_ERR_EINVAL;
    HIP_OK(hipSetDevice(c->device));
    const size_t n = (size_t)w * h;
    if (c->coef.ensure(n * 4) < 0 || c->tmp.ensure(n * 4) < 0 || c->args.ensure(ENC_MAX_LEVELS * sizeof(DwtPlane)) < 0)
        return HTJ2K_ERR_ENOMEM;
    HIP_OK(hipMemcpyAsync(c->coef.p, plane, n * 4, hipMemcpyHostToDevice, c->stream));
    std::vector<DwtPlane> planes(1), tab;
    planes[0].p = (int32_t *)c->coef.p;
    planes[0].t = (int32_t *)c->tmp.p;
    planes[0].stride = w;
    planes[0].lw = w;
    planes[0].lh = h;
    std::vector<int> lev(1, levels);
    int r = run_fdwt(c, planes, lev, 0, tab, false);
    if (r < 0)
        return r;
    HIP_OK(hipMemcpyAsync(plane, c->coef.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int htj2k_fdwt97_plane(htj2k_enc_ctx *c, float *plane, int w, int h, int levels)
{
    if (!c || !plane || w < 1 || h < 1 || w > 32768 || h > 32768 || levels < 0 || levels > 32)
        return HTJ2K_ERR_EINVAL;
    HIP_OK(hipSetDevice(c->device));
    const size_t n = (size_t)w * h;
    if (c->coef.ensure(n * 4) < 0 || c->tmp.ensure(n * 4) < 0 || c->args.ensure(ENC_MAX_LEVELS * sizeof(DwtPlane)) < 0)
        return HTJ2K_ERR_ENOMEM;
    HIP_OK(hipMemcpyAsync(c->coef.p, plane, n * 4, hipMemcpyHostToDevice, c->stream));
    std::vector<DwtPlane> planes(1), tab;
    planes[0].p = (int32_t *)c->coef.p;
    planes[0].t = (int32_t *)c->tmp.p;
    planes[0].stride = w;
    planes[0].lw = w;
    planes[0].lh = h;
    std::vector<int> lev(1, levels);
    int r = run_fdwt(c, planes, lev, 0, tab, true);
    if (r < 0)
        return r;
    HIP_OK(hipMemcpyAsync(plane, c->coef.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

/* the launch table of caller-given blocks of one plane; what k_ht_encode's and k_rc_stats' LDS hold: ENC_MAX_QUADS
 * quads, 4096 samples (every T.800 block size, clipped or not) */
static int block_table(const htj2k_enc_block *blocks, int nblocks, int plane_w, int plane_h, const int *planes,
                       std::vector<EncBlk> &tab, size_t *offsets, size_t *total)
{
    size_t at = 0;
    tab.assign((size_t)nblocks + 1, EncBlk());
    for (int i = 0; i < nblocks; i++) {
        const htj2k_enc_block &b = blocks[i];
        if (b.w < 1 || b.h < 1 || b.w > 1024 || b.h > 1024 || b.w * b.h > 4096 ||
            ((b.w + 1) >> 1) * ((b.h + 1) >> 1) > ENC_MAX_QUADS || b.x < 0 || b.y < 0 ||
            b.x + b.w > plane_w || b.y + b.h > plane_h || (planes && (planes[i] < 0 || planes[i] > 31)))
            return HTJ2K_ERR_EINVAL;
        tab[i].coef = (uint64_t)b.y * plane_w + b.x;
        tab[i].stride = plane_w;
        tab[i].w = (uint16_t)b.w;
        tab[i].h = (uint16_t)b.h;
        tab[i].plane = planes ? planes[i] : 0;
        tab[i].pad = 0;
        tab[i].out = at;
        if (offsets)
            offsets[i] = at;
        at += region(b.w, b.h);
    }
    if (offsets)
        offsets[nblocks] = at;
    *total = at;
    return 0;
}

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
    if (!coef || plane_w < 1 || plane_h < 1 || nblocks < 0 || (nblocks && (!blocks || !offsets || !lcup || !max_u)))
        return HTJ2K_ERR_EINVAL;
    std::vector<EncBlk> tab;
    size_t at = 0;
    if (block_table(blocks, nblocks, plane_w, plane_h, planes, tab, offsets, &at) < 0)
        return HTJ2K_ERR_EINVAL;
    if (at > cap)
        return HTJ2K_ERR_ENOSPC;
    if (!c)
        return HTJ2K_ERR_ENOSYS;                       /* the arguments are fine; there is no device to run on */
    HIP_OK(hipSetDevice(c->device));
    const size_t n = (size_t)plane_w * plane_h;
    if (c->coef.ensure(n * 4) < 0 || c->blk.ensure(tab.size() * sizeof(EncBlk)) < 0 ||
        c->res.ensure(tab.size() * sizeof(EncRes)) < 0 || c->pool.ensure(at + 16) < 0 || ensure_stamps(c, nblocks) < 0)
        return HTJ2K_ERR_ENOMEM;
    HIP_OK(hipMemcpyAsync(c->coef.p, coef, n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->blk.p, tab.data(), (size_t)nblocks * sizeof(EncBlk), hipMemcpyHostToDevice, c->stream));
    int r = run_ht(c, (const EncBlk *)c->blk.p, nblocks, (const int32_t *)c->coef.p, (uint8_t *)c->pool.p, (EncRes *)c->res.p);
    if (r < 0)
        return r;
    std::vector<EncRes> res((size_t)nblocks + 1);
    HIP_OK(hipMemcpyAsync(res.data(), c->res.p, (size_t)nblocks * sizeof(EncRes), hipMemcpyDeviceToHost, c->stream));
    if (at)
        HIP_OK(hipMemcpyAsync(out, c->pool.p, at, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    memset(c->cycles, 0, sizeof c->cycles);
    c->stamped = 0;
    if ((r = collect_stamps(c, nblocks)) < 0)
        return r;
    for (int i = 0; i < nblocks; i++) {
        lcup[i] = res[i].lcup;
        max_u[i] = res[i].max_u;
        if (res[i].lcup < 0)
            r = HTJ2K_ERR_BUG;
    }
    return r;
}

/* ------------------------------------------------------------------ rate control */
static int rc_ensure(htj2k_enc_ctx *c, int nblk, int nf, RcStats *S)
{
    const size_t n = (size_t)nblk + 1;
    if (c->rc_dist.ensure(n * RC_PLANES * 8) < 0 || c->rc_len.ensure(n * RC_PLANES * 4) < 0 || c->rc_dskip.ensure(n * 8) < 0 ||
        c->rc_low.ensure(n * 4) < 0 || c->rc_kmax.ensure(n * 4) < 0 || c->rc_w.ensure(n * 8) < 0 || c->rc_scale.ensure(n * 8) < 0 ||
        c->rc_planes.ensure(n * 4) < 0 || c->rc_sel_len.ensure(n * 4) < 0 ||
        c->rc_frames.ensure((size_t)(nf + 1) * sizeof(RcFrame)) < 0 || c->rc_sel.ensure((size_t)(nf + 1) * sizeof(RcSel)) < 0)
        return HTJ2K_ERR_ENOMEM;
    S->dist = (uint64_t *)c->rc_dist.p;
    S->len = (uint32_t *)c->rc_len.p;
    S->dskip = (double *)c->rc_dskip.p;
    S->low0 = (uint32_t *)c->rc_low.p;
    S->kmax = (int32_t *)c->rc_kmax.p;
    return 0;
}

extern "C" int htj2k_enc_rc_stats(htj2k_enc_ctx *c, const int32_t *coef, int plane_w, int plane_h,
                                  const htj2k_enc_block *blocks, int nblocks, int nplanes, uint64_t *dist, uint32_t *len_est)
{
    if (!coef || plane_w < 1 || plane_h < 1 || nblocks < 0 || nplanes < 1 || nplanes > RC_PLANES ||
        (nblocks && (!blocks || !dist || !len_est)))
        return HTJ2K_ERR_EINVAL;
    std::vector<EncBlk> tab;
    size_t at = 0;
    if (block_table(blocks, nblocks, plane_w, plane_h, nullptr, tab, nullptr, &at) < 0)
        return HTJ2K_ERR_EINVAL;
    if (!c)
        return HTJ2K_ERR_ENOSYS;
    if (!nblocks)
        return 0;
    HIP_OK(hipSetDevice(c->device));
    const size_t n = (size_t)plane_w * plane_h;
    RcStats S;
    if (c->coef.ensure(n * 4) < 0 || c->blk.ensure(tab.size() * sizeof(EncBlk)) < 0 || rc_ensure(c, nblocks, 1, &S) < 0)
        return HTJ2K_ERR_ENOMEM;
    HIP_OK(hipMemcpyAsync(c->coef.p, coef, n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->blk.p, tab.data(), (size_t)nblocks * sizeof(EncBlk), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rc_stats, dim3((unsigned)nblocks), dim3(64), 0, c->stream, (const EncBlk *)c->blk.p,
                       (const int32_t *)c->coef.p, (const uint16_t *)c->d_tab, nplanes, S);
    HIP_OK(hipGetLastError());
    std::vector<uint64_t> d((size_t)nblocks * RC_PLANES);
    std::vector<uint32_t> l((size_t)nblocks * RC_PLANES);
    HIP_OK(hipMemcpyAsync(d.data(), S.dist, d.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(l.data(), S.len, l.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < nblocks; i++)
        for (int p = 0; p < nplanes; p++) {
            dist[(size_t)i * nplanes + p] = d[(size_t)i * RC_PLANES + p];
            len_est[(size_t)i * nplanes + p] = l[(size_t)i * RC_PLANES + p];
        }
    return 0;
}

/* exact bytes of frame F's codestream for these lengths and planes (the headers are written and thrown away) */
static int64_t frame_size(const EncFrame &F, int guard, const int *lcup, const int *planes)
{
    EncOut o;
    memset(&o, 0, sizeof o);
    const int r = enc_write(&F, guard, lcup, planes, &o);
    const int64_t n = r < 0 ? r : (int64_t)o.size;
    enc_out_free(&o);
    return n;
}

static float ev_ms(hipEvent_t a, hipEvent_t b)
{
    float t = 0;
    return hipEventElapsedTime(&t, a, b) == hipSuccess ? t : 0.0f;
}

/* one round: frames [f0, f1) of the call */
static int encode_round(htj2k_enc_ctx *c, const htj2k_frame *in, const EncFrame *fr, int f0, int f1, int in_on_device,
                        uint8_t *out, size_t cap, int out_on_device, size_t *offsets, uint64_t out_base, uint64_t *out_end,
                        float *ms, const int64_t *minsz)
{
    const EncFrame &F0 = fr[f0];
    const bool rc = F0.target > 0;
    RcStats S = { nullptr, nullptr, nullptr, nullptr, nullptr };
    const int nf = f1 - f0, nc = F0.ncomp;
    std::vector<size_t> plane_off((size_t)nf * nc);
    std::vector<size_t> in_off((size_t)nf * 4);
    size_t ns = 0, nin = 0, npool = 0;
    int nblk = 0, maxw = 0, maxh = 0, r;
    for (int f = 0; f < nf; f++) {
        const EncFrame &F = fr[f0 + f];
        for (int k = 0; k < nc; k++) {
            plane_off[(size_t)f * nc + k] = ns;
            ns += ((size_t)F.cw[k] * F.ch[k] + 63) & ~(size_t)63;
        }
        const int nplanes = F.planar ? nc : 1;
        for (int p = 0; p < nplanes; p++) {
            const size_t row = (size_t)(F.planar ? F.cw[p] : F.w * F.step) * F.bytes;
            in_off[(size_t)f * 4 + p] = nin;
            nin += (row * (F.planar ? F.ch[p] : F.h) + 255) & ~(size_t)255;
        }
        for (int i = 0; i < F.nblk; i++)
            npool += region(F.blk[i].w, F.blk[i].h);
        nblk += F.nblk;
        maxw = F.w > maxw ? F.w : maxw;
        maxh = F.h > maxh ? F.h : maxh;
    }
    /* the args buffer: unpack table, DWT tables, then (9/7) the quantiser's plane table and step tables */
    const size_t dwt_args = ((size_t)nf * sizeof(UnpackArgs) + 255) & ~(size_t)255;
    const size_t q_args = dwt_args + (((size_t)nf * nc * ENC_MAX_LEVELS * sizeof(DwtPlane) + 255) & ~(size_t)255);
    const size_t q_steps = q_args + (((size_t)nf * nc * sizeof(QuantPlane) + 255) & ~(size_t)255);
    const size_t args_end = F0.irrev ? q_steps + (size_t)nf * nc * ENC_MAX_BANDS * sizeof(float) : q_args;
    if (c->coef.ensure(ns * 4) < 0 || c->tmp.ensure(ns * 4) < 0 || c->pool.ensure(npool + 16) < 0 ||
        c->blk.ensure((size_t)(nblk + 1) * sizeof(EncBlk)) < 0 || c->res.ensure((size_t)(nblk + 1) * sizeof(EncRes)) < 0 ||
        c->args.ensure(args_end) < 0 ||
        (!in_on_device && c->in.ensure(nin + 256) < 0) || ensure_stamps(c, nblk) < 0 ||
        (rc && (rc_ensure(c, nblk, nf, &S) < 0 || c->blk2.ensure((size_t)(nblk + 1) * sizeof(EncBlk)) < 0 ||
                c->res2.ensure((size_t)(nblk + 1) * sizeof(EncRes)) < 0)))
        return HTJ2K_ERR_ENOMEM;

    /* unpack */
    std::vector<UnpackArgs> ua((size_t)nf);
    for (int f = 0; f < nf; f++) {
        const EncFrame &F = fr[f0 + f];
        const htj2k_frame &I = in[f0 + f];
        UnpackArgs &A = ua[f];
        memset(&A, 0, sizeof A);
        A.w = F.w;
        A.h = F.h;
        const int nplanes = F.planar ? nc : 1;
        for (int p = 0; p < nplanes; p++) {
            const size_t row = (size_t)(F.planar ? F.cw[p] : F.w * F.step) * F.bytes;
            const int rows = F.planar ? F.ch[p] : F.h;
            if (!I.data[p] || I.linesize[p] < 0 || (size_t)I.linesize[p] < row) {
                enc_log(c, 16, "encoder: a plane is missing or its linesize is negative or too short\n");
                return HTJ2K_ERR_EINVAL;
            }
            if (in_on_device) {
                A.src[p] = I.data[p];
                A.linesize[p] = I.linesize[p];
            } else {
                uint8_t *d = (uint8_t *)c->in.p + in_off[(size_t)f * 4 + p];
                HIP_OK(hipMemcpy2DAsync(d, row, I.data[p], (size_t)I.linesize[p], row, (size_t)rows, hipMemcpyHostToDevice, c->stream));
                A.src[p] = d;
                A.linesize[p] = (int64_t)row;
            }
        }
        for (int k = 0; k < nc; k++) {
            A.dst[k] = (int32_t *)c->coef.p + plane_off[(size_t)f * nc + k];
            A.cw[k] = F.cw[k];
            A.ch[k] = F.ch[k];
        }
    }
    UnpackFmt U = { nc, F0.planar, F0.step, F0.bytes, F0.shift, F0.bits, F0.mct };
    HIP_OK(hipMemcpyAsync(c->args.p, ua.data(), ua.size() * sizeof(UnpackArgs), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->ev[0], c->stream));
    for (int z0 = 0; z0 < nf; z0 += 65535)
        hipLaunchKernelGGL(F0.irrev ? k_enc_unpack<true> : k_enc_unpack<false>,
                           dim3((unsigned)((maxw + 255) / 256), (unsigned)maxh, (unsigned)(nf - z0 < 65535 ? nf - z0 : 65535)),
                           dim3(256), 0, c->stream, (const UnpackArgs *)c->args.p + z0, U);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(c->ev[1], c->stream));

    /* forward DWT */
    std::vector<DwtPlane> planes;
    std::vector<int> lev;
    for (int f = 0; f < nf; f++)
        for (int k = 0; k < nc; k++) {
            const EncFrame &F = fr[f0 + f];
            DwtPlane d;
            d.p = (int32_t *)c->coef.p + plane_off[(size_t)f * nc + k];
            d.t = (int32_t *)c->tmp.p + plane_off[(size_t)f * nc + k];
            d.stride = F.cw[k];
            d.lw = F.cw[k];
            d.lh = F.ch[k];
            planes.push_back(d);
            lev.push_back(F.nl);
        }
    std::vector<DwtPlane> dwt_tab;
    if ((r = run_fdwt(c, planes, lev, dwt_args, dwt_tab, F0.irrev != 0)) < 0)
        return r;

    /* 9/7: float coefficients -> int32 indices, every plane in one launch (counted with the DWT) */
    std::vector<QuantPlane> qp;
    std::vector<float> qs;
    if (F0.irrev) {
        const float *d_steps = (const float *)((uint8_t *)c->args.p + q_steps);
        int qw = 0, qh = 0;
        for (int f = 0; f < nf; f++)
            for (int k = 0; k < nc; k++) {
                const EncFrame &F = fr[f0 + f];
                QuantPlane q;
                q.p = (int32_t *)c->coef.p + plane_off[(size_t)f * nc + k];
                q.step = d_steps + qs.size();
                q.w = F.cw[k];
                q.h = F.ch[k];
                q.nl = F.nl;
                qs.insert(qs.end(), F.fstep[k], F.fstep[k] + ENC_MAX_BANDS);
                qp.push_back(q);
                qw = q.w > qw ? q.w : qw;
                qh = q.h > qh ? q.h : qh;
            }
        HIP_OK(hipMemcpyAsync((uint8_t *)c->args.p + q_args, qp.data(), qp.size() * sizeof(QuantPlane), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync((uint8_t *)c->args.p + q_steps, qs.data(), qs.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        for (size_t z0 = 0; z0 < qp.size(); z0 += 65535)
            hipLaunchKernelGGL(k_quant97, dim3((unsigned)((qw + 255) / 256), (unsigned)qh, (unsigned)(qp.size() - z0 < 65535 ? qp.size() - z0 : 65535)),
                               dim3(256), 0, c->stream, (const QuantPlane *)((uint8_t *)c->args.p + q_args) + z0);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipEventRecord(c->ev[2], c->stream));

    /* HT cleanup pass of every block */
    std::vector<EncBlk> bt((size_t)nblk + 1);
    std::vector<int> blk0((size_t)nf + 1);
    {
        size_t at = 0;
        int bi = 0;
        for (int f = 0; f < nf; f++) {
            const EncFrame &F = fr[f0 + f];
            blk0[f] = bi;
            for (int i = 0; i < F.nblk; i++, bi++) {
                const EncBlock &b = F.blk[i];
                bt[bi].coef = plane_off[(size_t)f * nc + b.comp] + (uint64_t)b.y * F.cw[b.comp] + (uint64_t)b.x;
                bt[bi].stride = F.cw[b.comp];
                bt[bi].w = (uint16_t)b.w;
                bt[bi].h = (uint16_t)b.h;
                bt[bi].plane = 0;
                bt[bi].pad = 0;
                bt[bi].out = at;
                at += region(b.w, b.h);
            }
        }
        blk0[nf] = bi;
    }
    HIP_OK(hipMemcpyAsync(c->blk.p, bt.data(), (size_t)nblk * sizeof(EncBlk), hipMemcpyHostToDevice, c->stream));

    /* rate control: the statistics of every block, then the plane of every block (written into the launch table) */
    std::vector<double> rc_w, rc_scale;
    std::vector<RcFrame> rc_fr;
    std::vector<int64_t> budget((size_t)nf, 0);
    if (rc) {
        rc_w.resize((size_t)nblk + 1);
        rc_scale.assign((size_t)nblk + 1, 1.0);
        rc_fr.resize((size_t)nf);
        for (int f = 0; f < nf; f++) {
            const EncFrame &F = fr[f0 + f];
            for (int i = 0; i < F.nblk; i++) {
                const EncBlock &b = F.blk[i];
                rc_w[(size_t)blk0[f] + i] = F.wgt[b.comp][b.res ? 3 * (b.res - 1) + b.band : 0];
            }
            budget[f] = F.target - minsz[f0 + f];
            rc_fr[f].blk0 = blk0[f];
            rc_fr[f].nblk = F.nblk;
            rc_fr[f].budget = budget[f];
            rc_fr[f].allow_trial = 1;
            rc_fr[f].pad = 0;
        }
        HIP_OK(hipMemcpyAsync(c->rc_w.p, rc_w.data(), (size_t)nblk * 8, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(c->rc_scale.p, rc_scale.data(), (size_t)nblk * 8, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(c->rc_frames.p, rc_fr.data(), (size_t)nf * sizeof(RcFrame), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipEventRecord(c->ev[7], c->stream));
        if (nblk > 0)
            hipLaunchKernelGGL(k_rc_stats, dim3((unsigned)nblk), dim3(64), 0, c->stream, (const EncBlk *)c->blk.p,
                               (const int32_t *)c->coef.p, (const uint16_t *)c->d_tab, RC_PLANES, S);
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(c->ev[6], c->stream));
        hipLaunchKernelGGL(k_rc_select, dim3((unsigned)nf), dim3(RC_THREADS), 0, c->stream, (const RcFrame *)c->rc_frames.p, S,
                           (const double *)c->rc_w.p, (const double *)c->rc_scale.p, (EncBlk *)c->blk.p, (int32_t *)c->rc_planes.p,
                           (uint32_t *)c->rc_sel_len.p, (RcSel *)c->rc_sel.p);
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(c->ev[5], c->stream));
    }
    if ((r = run_ht(c, (const EncBlk *)c->blk.p, nblk, (const int32_t *)c->coef.p, (uint8_t *)c->pool.p, (EncRes *)c->res.p)) < 0)
        return r;
    HIP_OK(hipEventRecord(c->ev[3], c->stream));
    std::vector<EncRes> res((size_t)nblk + 1);
    std::vector<int32_t> cur_plane((size_t)nblk + 1, 0);
    std::vector<uint32_t> sel_len((size_t)nblk + 1, 0);
    std::vector<RcSel> sel((size_t)nf + 1);
    HIP_OK(hipMemcpyAsync(res.data(), c->res.p, (size_t)nblk * sizeof(EncRes), hipMemcpyDeviceToHost, c->stream));
    if (rc) {
        HIP_OK(hipMemcpyAsync(cur_plane.data(), c->rc_planes.p, (size_t)nblk * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipMemcpyAsync(sel_len.data(), c->rc_sel_len.p, (size_t)nblk * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipMemcpyAsync(sel.data(), c->rc_sel.p, (size_t)nf * sizeof(RcSel), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    if ((r = collect_stamps(c, nblk)) < 0)
        return r;
    ms[0] += ev_ms(c->ev[0], c->ev[1]);
    ms[1] += ev_ms(c->ev[1], c->ev[2]);
    ms[2] += ev_ms(c->ev[rc ? 5 : 2], c->ev[3]);
    if (rc) {
        c->rc_ms[0] += ev_ms(c->ev[7], c->ev[6]);
        c->rc_ms[1] += ev_ms(c->ev[6], c->ev[5]);
    }
    for (int i = 0; i < nblk; i++)
        if (res[(size_t)i].lcup < 0) {
            enc_log(c, 16, "encoder: a code-block could not be coded (MEL + VLC beyond 4079 bytes)\n");
            return HTJ2K_ERR_BUG;
        }

    /* the guarantee: exact sizes on the host; frames over budget are selected again and their changed blocks re-coded */
    std::vector<htj2k_enc_rc> info((size_t)nf);
    std::vector<uint8_t> recoded((size_t)nblk + 1, 0);
    memset(info.data(), 0, info.size() * sizeof(htj2k_enc_rc));
    for (int f = 0; f < nf; f++) {
        info[f].target_bytes = fr[f0 + f].target;
        info[f].nblocks = fr[f0 + f].nblk;
        info[f].ht_launches = 1;
        info[f].trial = rc ? sel[f].trial : 0;
        info[f].est_bytes = rc ? (int64_t)sel[f].est + minsz[f0 + f] : 0;
    }
    for (int launch = 1; rc; launch++) {
        std::vector<int> over;
        std::vector<int64_t> size((size_t)nf, 0);
        std::vector<int> lc, mu, pl;
        for (int f = 0; f < nf; f++) {
            const EncFrame &F = fr[f0 + f];
            if (info[f].ht_launches != launch)
                continue;                              /* it fitted in an earlier launch */
            lc.resize((size_t)F.nblk); mu.resize((size_t)F.nblk); pl.resize((size_t)F.nblk);
            for (int i = 0; i < F.nblk; i++) {
                lc[i] = res[(size_t)blk0[f] + i].lcup;
                mu[i] = res[(size_t)blk0[f] + i].max_u;
                pl[i] = cur_plane[(size_t)blk0[f] + i];
            }
            const int guard = enc_guard_bits(&F, mu.data(), pl.data(), enc_log, c);
            if (guard < 0)
                return guard;
            if ((size[f] = frame_size(F, guard, lc.data(), pl.data())) < 0)
                return (int)size[f];
            if (size[f] > F.target)
                over.push_back(f);
        }
        if (over.empty())
            break;
        /* last resort: leave blocks out, least distortion per byte saved first.  "Left out" has length 0, so the frame
         * ends inside the budget without another launch.  (Only the bytes of a block's current plane are kept, so the
         * planes of earlier launches are not candidates here.) */
        auto last_resort = [&](int f, int64_t size_f) -> int {
            const EncFrame &F = fr[f0 + f];
            std::vector<uint64_t> dist((size_t)F.nblk * RC_PLANES);
            std::vector<double> dskip((size_t)F.nblk);
            HIP_OK(hipMemcpy(dist.data(), S.dist + (size_t)blk0[f] * RC_PLANES, dist.size() * 8, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(dskip.data(), S.dskip + blk0[f], dskip.size() * 8, hipMemcpyDeviceToHost));
            std::vector<std::pair<double, int>> order;
            for (int i = 0; i < F.nblk; i++) {
                const size_t b = (size_t)blk0[f] + i;
                if (res[b].lcup > 0)
                    order.push_back({ rc_w[b] * (dskip[i] - (double)dist[(size_t)i * RC_PLANES + cur_plane[b]]) / res[b].lcup, i });
            }
            std::sort(order.begin(), order.end());
            size_t next = 0;
            info[f].last_resort = 1;
            while (size_f > F.target && next < order.size()) {
                int64_t saved = 0;
                while (next < order.size() && saved < size_f - F.target) {
                    const size_t b = (size_t)blk0[f] + order[next++].second;
                    saved += res[b].lcup;
                    res[b].lcup = 0;
                    res[b].max_u = 0;
                    cur_plane[b] = -1;
                }
                lc.resize((size_t)F.nblk); mu.resize((size_t)F.nblk); pl.resize((size_t)F.nblk);
                for (int i = 0; i < F.nblk; i++) {
                    lc[i] = res[(size_t)blk0[f] + i].lcup;
                    mu[i] = res[(size_t)blk0[f] + i].max_u;
                    pl[i] = cur_plane[(size_t)blk0[f] + i];
                }
                const int guard = enc_guard_bits(&F, mu.data(), pl.data(), enc_log, c);
                if (guard < 0)
                    return guard;
                if ((size_f = frame_size(F, guard, lc.data(), pl.data())) < 0)
                    return (int)size_f;
            }
            if (size_f > F.target)
                return HTJ2K_ERR_BUG;
            return 0;
        };
        if (launch == RC_MAX_LAUNCHES) {
            for (int f : over)
                if ((r = last_resort(f, size[f])) < 0)
                    return r;
            break;
        }
        /* select again: every coded block's estimates scaled by its own actual / estimated, the budget down by the overshoot */
        std::vector<RcFrame> again;
        for (int f : over) {
            const EncFrame &F = fr[f0 + f];
            for (int i = 0; i < F.nblk; i++) {
                const size_t b = (size_t)blk0[f] + i;
                if (res[b].lcup > 0 && sel_len[b] > 0)
                    rc_scale[b] = (double)res[b].lcup / (double)sel_len[b];
            }
            budget[f] -= size[f] - F.target;
            if (budget[f] < 0)
                budget[f] = 0;
            RcFrame a = rc_fr[f];
            a.budget = budget[f];
            a.allow_trial = 0;
            again.push_back(a);
        }
        std::vector<int32_t> new_plane((size_t)nblk + 1);
        HIP_OK(hipMemcpyAsync(c->rc_scale.p, rc_scale.data(), (size_t)nblk * 8, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(c->rc_frames.p, again.data(), again.size() * sizeof(RcFrame), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipEventRecord(c->ev[6], c->stream));
        hipLaunchKernelGGL(k_rc_select, dim3((unsigned)again.size()), dim3(RC_THREADS), 0, c->stream, (const RcFrame *)c->rc_frames.p, S,
                           (const double *)c->rc_w.p, (const double *)c->rc_scale.p, (EncBlk *)c->blk.p, (int32_t *)c->rc_planes.p,
                           (uint32_t *)c->rc_sel_len.p, (RcSel *)c->rc_sel.p);
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(c->ev[7], c->stream));
        HIP_OK(hipMemcpyAsync(new_plane.data(), c->rc_planes.p, (size_t)nblk * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipMemcpyAsync(sel_len.data(), c->rc_sel_len.p, (size_t)nblk * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        c->rc_ms[1] += ev_ms(c->ev[6], c->ev[7]);
        /* code again the blocks whose plane changed; a block's earlier bytes stay valid for its earlier plane */
        std::vector<EncBlk> bt2;
        std::vector<size_t> which;
        for (int f : over) {
            const size_t before = bt2.size();
            for (int i = 0; i < fr[f0 + f].nblk; i++) {
                const size_t b = (size_t)blk0[f] + i;
                if (new_plane[b] == cur_plane[b])
                    continue;
                cur_plane[b] = new_plane[b];
                recoded[b] = 1;
                EncBlk e = bt[b];
                e.plane = new_plane[b];
                bt2.push_back(e);
                which.push_back(b);
            }
            if (bt2.size() > before) {
                info[f].ht_launches = launch + 1;
            } else if ((r = last_resort(f, size[f])) < 0) {    /* the same selection again: another round cannot help */
                return r;
            }
        }
        if (!bt2.empty()) {
            std::vector<EncRes> res2(bt2.size());
            HIP_OK(hipMemcpyAsync(c->blk2.p, bt2.data(), bt2.size() * sizeof(EncBlk), hipMemcpyHostToDevice, c->stream));
            HIP_OK(hipEventRecord(c->ev[6], c->stream));
            if ((r = run_ht(c, (const EncBlk *)c->blk2.p, (int)bt2.size(), (const int32_t *)c->coef.p, (uint8_t *)c->pool.p,
                            (EncRes *)c->res2.p)) < 0)
                return r;
            HIP_OK(hipEventRecord(c->ev[7], c->stream));
            HIP_OK(hipMemcpyAsync(res2.data(), c->res2.p, bt2.size() * sizeof(EncRes), hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipStreamSynchronize(c->stream));
            c->rc_ms[2] += ev_ms(c->ev[6], c->ev[7]);
            for (size_t k = 0; k < which.size(); k++) {
                if (res2[k].lcup < 0) {
                    enc_log(c, 16, "encoder: a code-block could not be coded (MEL + VLC beyond 4079 bytes)\n");
                    return HTJ2K_ERR_BUG;
                }
                res[which[k]] = res2[k];
            }
        }
    }

    /* headers and packet headers on the host; the pieces of every codestream */
    EncOut o;
    memset(&o, 0, sizeof o);
    o.size = out_base;
    std::vector<int> lcup, mu;
    for (int f = 0; f < nf && !r; f++) {
        const EncFrame &F = fr[f0 + f];
        lcup.assign((size_t)F.nblk, 0);
        mu.assign((size_t)F.nblk, 0);
        for (int i = 0; i < F.nblk; i++) {
            const EncRes &e = res[(size_t)blk0[f] + i];
            if (e.lcup < 0) {
                enc_log(c, 16, "encoder: a code-block could not be coded (MEL + VLC beyond 4079 bytes)\n");
                r = HTJ2K_ERR_BUG;
            }
            lcup[i] = e.lcup;
            mu[i] = e.max_u;
        }
        if (r)
            break;
        const int32_t *pl = cur_plane.data() + blk0[f];
        const int guard = enc_guard_bits(&F, mu.data(), pl, enc_log, c);
        if (guard < 0) {
            r = guard;
            break;
        }
        const size_t p0 = o.npc;
        offsets[f0 + f] = (size_t)o.size;
        if ((r = enc_write(&F, guard, lcup.data(), pl, &o)) < 0)
            break;
        info[f].final_bytes = (int64_t)(o.size - offsets[f0 + f]);
        if (rc && info[f].final_bytes > F.target) {
            r = HTJ2K_ERR_BUG;                         /* the sizes were checked above: cannot happen */
            break;
        }
        for (int i = 0; i < F.nblk; i++) {
            info[f].blocks_left_out += pl[i] < 0;
            info[f].blocks_recoded += recoded[(size_t)blk0[f] + i];
        }
        c->last_planes[(size_t)(f0 + f)].assign(pl, pl + F.nblk);
        c->last_rc[(size_t)(f0 + f)] = info[f];
        for (size_t p = p0; p < o.npc; p++)
            if (o.pc[p].block >= 0)
                o.pc[p].block += blk0[f];
    }
    if (!r && o.size > cap) {
        enc_log(c, 16, "encoder: the codestreams do not fit the output buffer\n");
        r = HTJ2K_ERR_ENOSPC;
    }
    if (r) {
        enc_out_free(&o);
        return r;
    }
    offsets[f1] = (size_t)o.size;
    *out_end = o.size;

    /* gather */
    std::vector<GatherPiece> gp(o.npc);
    for (size_t p = 0; p < o.npc; p++) {
        gp[p].dst = o.pc[p].dst - out_base;
        gp[p].len = o.pc[p].len;
        gp[p].from_pool = o.pc[p].block >= 0;
        gp[p].src = o.pc[p].block >= 0 ? bt[(size_t)o.pc[p].block].out : o.pc[p].src;
    }
    const size_t bytes = (size_t)(o.size - out_base);
    if (c->lit.ensure(o.nlit + 16) < 0 || c->pieces.ensure(gp.size() * sizeof(GatherPiece) + 16) < 0 ||
        (!out_on_device && c->out.ensure(bytes + 16) < 0)) {
        enc_out_free(&o);
        return HTJ2K_ERR_ENOMEM;
    }
    uint8_t *dst = out_on_device ? out + out_base : (uint8_t *)c->out.p;
    if (hipMemcpyAsync(c->lit.p, o.lit, o.nlit, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        enc_out_free(&o);
        return HTJ2K_ERR_EXTERNAL;
    }
    r = hipMemcpyAsync(c->pieces.p, gp.data(), gp.size() * sizeof(GatherPiece), hipMemcpyHostToDevice, c->stream) == hipSuccess &&
        hipEventRecord(c->ev[3], c->stream) == hipSuccess ? 0 : HTJ2K_ERR_EXTERNAL;
    for (size_t p0 = 0; p0 < gp.size() && !r; p0 += 1u << 30)
        hipLaunchKernelGGL(k_enc_gather, dim3((unsigned)(gp.size() - p0 < (1u << 30) ? gp.size() - p0 : (1u << 30))), dim3(256), 0,
                           c->stream, (const GatherPiece *)c->pieces.p + p0, (const uint8_t *)c->lit.p, (const uint8_t *)c->pool.p, dst);
    if (!r && (hipGetLastError() != hipSuccess || hipEventRecord(c->ev[4], c->stream) != hipSuccess ||
               (!out_on_device && hipMemcpyAsync(out + out_base, c->out.p, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess)))
        r = HTJ2K_ERR_EXTERNAL;
    /* the literal bytes and the piece table are host memory the queued copies read: freed only behind the sync */
    if (hipStreamSynchronize(c->stream) != hipSuccess && !r)
        r = HTJ2K_ERR_EXTERNAL;
    enc_out_free(&o);
    if (r)
        return r;
    float t = 0;
    if (hipEventElapsedTime(&t, c->ev[3], c->ev[4]) == hipSuccess)
        ms[3] += t;
    return 0;
}

extern "C" int htj2k_encode_batch(htj2k_enc_ctx *c, const htj2k_frame *in, int n, int bits, const htj2k_enc_opts *opts,
                                  int in_on_device, uint8_t *out, size_t cap, int out_on_device, size_t *offsets)
{
    if (!c || !in || n < 1 || !out || !offsets)
        return HTJ2K_ERR_EINVAL;
    HIP_OK(hipSetDevice(c->device));
    std::vector<EncFrame> fr((size_t)n);
    int r = 0, made = 0;
    for (int i = 0; i < n && !r; i++) {
        if (in[i].pix_fmt != in[0].pix_fmt) {
            enc_log(c, 16, "encoder: the frames of a batch share one layout\n");
            r = HTJ2K_ERR_EINVAL;
            break;
        }
        if ((r = enc_frame_init(&fr[i], in[i].width, in[i].height, in[i].pix_fmt, bits, opts, enc_log, c)) == 0)
            made++;
    }
    /* a budget below the frame's smallest stream is refused before anything runs */
    std::vector<int64_t> minsz((size_t)n, 0);
    for (int i = 0; i < made && !r && fr[i].target > 0; i++) {
        if ((minsz[i] = enc_min_size(&fr[i])) < 0) {
            r = (int)minsz[i];
        } else if (fr[i].target < minsz[i]) {
            char msg[160];
            snprintf(msg, sizeof msg, "encoder: a budget of %lld bytes is below the frame's smallest stream (%lld bytes of headers and empty packets)\n",
                     (long long)fr[i].target, (long long)minsz[i]);
            enc_log(c, 16, msg);
            r = HTJ2K_ERR_EINVAL;
        }
    }
    memset(c->ms, 0, sizeof c->ms);
    memset(c->rc_ms, 0, sizeof c->rc_ms);
    memset(c->cycles, 0, sizeof c->cycles);
    c->stamped = 0;
    c->last_planes.assign((size_t)n, std::vector<int>());
    c->last_rc.assign((size_t)n, htj2k_enc_rc());
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
        r = encode_round(c, in, fr.data(), f0, f1, in_on_device, out, cap, out_on_device, offsets, at, &at, c->ms, minsz.data());
        f0 = f1;
    }
    for (int i = 0; i < made; i++)
        enc_frame_free(&fr[i]);
    return r;
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
