/*
 * curve_kernels.hpp -- frames as tensors through a transfer curve, a colour matrix and a second curve
 * (htj2k_frames_to_tensor_curves and the five calls beside it).  include/htj2k_amd.h has the definition ("frames as
 * tensors, with curves"); in short, for output pixel (x, y) of channel k of K:
 *     f_c   the mix calls' source value of component c (mix_kernels.hpp)
 *     g_c = E(f_c; in) where bit c of in_mask is set, else f_c
 *     t   = the mix of g: tensor_mix_sum's C terms in their order, then + b[k]
 *     v   = E(t; out) where bit k of out_mask is set, else t
 *     e   = v * gain[k] + offset[k], two rounded operations, stored as the plain call stores it
 * A curve is n knots t[0 .. n-1] at x0 + j / inv_dx; curve_eval is E, once, and every kernel here calls it.
 *
 *   k_frame_curves      the fast route: k_frame_mix's cut (MixShape, MixFrame, cmp_load_group, tensor_store_run, SHARE
 *                       and PART), so the same frames qualify.
 *   k_frame_curves_any  the general route: one pixel per lane and step, as k_frame_mix_any.
 *   k_tensor_curves     the second launch of a resized call: reads k_frame_resize's float32 scratch, as k_tensor_mix.
 *
 * Both tables live in dynamic LDS, staged once per workgroup with 16-byte loads before the grid-stride loop: the
 * in-table's n + 1 floats (t[n] = t[n-1], written by the host) padded to a multiple of four, then the out-table's
 * likewise; 32 800 bytes at the most.  A lookup reads t[i] and t[i+1], neighbours of one array (one ds_read2_b32), and
 * subtracts; a staged pair { t[i], d_i } would be one 8-byte read but twice the LDS and half the workgroups of a CU
 * ("Transfer curves").  The host sizes the grid so that a workgroup reads several times its tables' bytes
 * of source (curves_grid, htj2k_device.hip).  No atomics, no results.  grid.z is the frame, in chunks of what it takes.
 * A translation unit that wants curve_eval alone (htj2k_encode.hip, through curve_in_kernels.hpp) defines
 * HTJ2K_TENSOR_IN_ONLY, as for tensor_kernels.hpp.
 */
#pragma once
#ifdef HTJ2K_TENSOR_IN_ONLY
#include "tensor_kernels.hpp"
#else
#include "mix_kernels.hpp"
#endif

namespace htj2k_cmp {

struct CurveFmt {                   /* uniform over a call */
    const float *tab;               /* device, 16-byte aligned: the in-table, then the out-table at float `out_at` */
    uint32_t n_in, n_out;           /* knots; 0: no curve (its mask is then 0) */
    uint32_t out_at, nfloat;        /* multiples of 4; nfloat: floats of both tables */
    float    x0_in, inv_in, x0_out, inv_out;
    uint32_t in_mask, out_mask;
    float    gain[4], offset[4];
};

/* E(x; curve), the definition: t has n + 1 entries, t[n] = t[n-1].  fmaxf / fminf give the operand that is not NaN, so a
 * NaN becomes knot 0; the conversion truncates a value within 0 .. n - 1 */
__device__ __forceinline__ float curve_eval(float x, const float *__restrict__ t, uint32_t n, float x0, float inv_dx)
{
    float u = __fmul_rn(__fsub_rn(x, x0), inv_dx);
    u = fminf(fmaxf(u, 0.0f), (float)(n - 1));
    const int i = (int)u;
    const float r = __fsub_rn(u, (float)i);
    const float ti = t[i];
    const float d = __fsub_rn(t[i + 1], ti);
    return __fadd_rn(ti, __fmul_rn(r, d));
}

/* The grid of a launch with curves, either direction.  Every workgroup first stages the tables, so grid.x is what the work
 * asks for (`gx`) but no more than leaves a workgroup `per` times its tables' bytes of source to read; one workgroup
 * where the call is smaller.  Results do not depend on `per`; what was measured under it: DESIGN.md 3.5 */
static inline unsigned curve_grid(size_t gx, size_t src_bytes, size_t table_bytes, size_t per)
{
    const size_t cap = src_bytes / (per * table_bytes);
    return (unsigned)(gx < cap ? gx : cap < 1 ? 1 : cap);
}

#ifndef HTJ2K_TENSOR_IN_ONLY

/* both tables into LDS, 16 bytes a lane and step; every lane of the workgroup calls it once */
__device__ __forceinline__ void curve_stage(float *__restrict__ lds, const CurveFmt &Q)
{
    for (uint32_t q = threadIdx.x; q < Q.nfloat / 4; q += CMP_THREADS) ((uint4 *)lds)[q] = ((const uint4 *)Q.tab)[q];
    __syncthreads();
}

/* the in-curve on the components its mask names */
__device__ __forceinline__ void curve_in(float f[4], const CurveFmt &Q, const float *__restrict__ lds)
{
#pragma unroll
    for (int c = 0; c < 4; c++)
        if ((Q.in_mask >> c) & 1u) f[c] = curve_eval(f[c], lds, Q.n_in, Q.x0_in, Q.inv_in);
}

/* channel k from the pixel's g: mix, out-curve, normalisation, conversion */
template <int DT>
__device__ __forceinline__ typename TensorElem<DT>::type curve_channel(const float g[4], int C, const MixFmt &F, const CurveFmt &Q, int k,
                                                                       const float *__restrict__ lds)
{
    float t = __fadd_rn(tensor_mix_sum(g, C, F.m[k]), F.b[k]);
    if ((Q.out_mask >> k) & 1u) t = curve_eval(t, lds + Q.out_at, Q.n_out, Q.x0_out, Q.inv_out);
    return tensor_value_f<DT>(t, Q.gain[k], Q.offset[k]);
}

extern __shared__ __align__(16) float curve_lds[];

template <int BYTES, int STEP, int NPL, int SW, int DT, int NHWC>
__global__ void __launch_bounds__(CMP_THREADS)
k_frame_curves(const MixFrame *__restrict__ frames, uint8_t *__restrict__ dst, MixFmt F, CurveFmt Q)
{
    typedef typename TensorElem<DT>::type elem_t;
    typedef MixShape<BYTES, STEP, NPL, SW, DT> S;
    constexpr int C = S::C, GROUP = S::GROUP, NP = S::NP, SHARE = S::SHARE, PART = S::PART;
    const MixFrame P = frames[blockIdx.z];
    const uint32_t K = F.nout;
    const uint32_t gpr = (F.out_w + NP - 1) / NP;            /* groups per row, the last one perhaps short */
    const uint64_t total = (uint64_t)gpr * F.out_h * SHARE;
    const bool wide = P.wide != 0;
    elem_t *const img = (elem_t *)dst + P.dst_img;
    curve_stage(curve_lds, Q);

    for (uint64_t it = (uint64_t)blockIdx.x * CMP_THREADS + threadIdx.x; it < total; it += (uint64_t)gridDim.x * CMP_THREADS) {
        uint32_t y, g;
        const uint32_t sub = (uint32_t)it % SHARE;           /* SHARE neighbouring lanes take the same group */
        if (total <= 0xFFFFFFFFull) { const uint32_t q = (uint32_t)it / SHARE; y = q / gpr; g = q - y * gpr; }
        else                        { const uint64_t q = it / SHARE; y = (uint32_t)(q / gpr); g = (uint32_t)(q - (uint64_t)y * gpr); }
        const uint32_t npix = min((uint32_t)NP, F.out_w - g * NP);
        const uint32_t first = sub * PART;                   /* this lane's part of them */
        if (npix <= first) continue;
        const uint32_t n = min((uint32_t)PART, npix - first);
        uint32_t w[NPL][GROUP / 4];
#pragma unroll
        for (int p = 0; p < NPL; p++) {
            const bool chroma = NPL > 1 && (p == 1 || p == 2);
            const uint32_t sh = chroma ? F.sh : 0;
            const uint8_t *row = P.src[p] + (int64_t)((P.oy + y) >> sh) * P.ls[p];
            if (chroma && SW) {                              /* half a group: one 16-byte load for twice the luma pixels */
                uint32_t h[GROUP / 8];
                cmp_load_group<GROUP / 2>(row + (size_t)g * (GROUP / 2), ((npix + 1) >> 1) * BYTES, true, h);
#pragma unroll
                for (int q = 0; q < GROUP / 8; q++) w[p][q] = h[q];
            } else {
                cmp_load_group<GROUP>(row + (size_t)g * GROUP, npix * (uint32_t)(STEP * BYTES), true, w[p]);
            }
        }
        elem_t v[4][PART];
#pragma unroll
        for (int part = 0; part < SHARE; part++) {
            if (sub != (uint32_t)part) continue;
#pragma unroll
            for (int k = 0; k < PART; k++) {
                constexpr int per = 4 / BYTES;               /* samples per word */
                const int e = part * PART + k;               /* pixel of the group */
                float f[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const int p = NPL > 1 ? c : 0;
                    const int s = NPL > 1 ? (e >> ((c == 1 || c == 2) ? SW : 0)) : e * STEP + c;   /* sample of the plane's group */
                    const uint32_t raw = (w[p][s / per] >> ((s % per) * 8 * BYTES)) & (BYTES == 1 ? 0xFFu : 0xFFFFu);
                    f[c] = (float)((raw >> F.shift) & F.mask);
                }
                curve_in(f, Q, curve_lds);
#pragma unroll
                for (int kk = 0; kk < 4; kk++)
                    if ((uint32_t)kk < K) v[kk][k] = curve_channel<DT>(f, C, F, Q, kk, curve_lds);
            }
        }
        const uint64_t x0 = (uint64_t)g * NP + first;
        if constexpr (NHWC) {
            elem_t *o = img + ((uint64_t)y * F.out_w + x0) * K;
            switch (K) {
            case 2:  mix_store_nhwc<2, PART>(o, v, n, wide); break;
            case 3:  mix_store_nhwc<3, PART>(o, v, n, wide); break;
            default: mix_store_nhwc<4, PART>(o, v, n, wide); break;
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 4; kk++)
                if ((uint32_t)kk < K) tensor_store_run<PART>(img + ((uint64_t)kk * F.out_h + y) * F.out_w + x0, v[kk], n, wide);
        }
    }
}

/* one output pixel per lane and step, all its channels.  grid.x strides over the window, grid.z is the frame */
template <int DT>
__global__ void __launch_bounds__(CMP_THREADS)
k_frame_curves_any(const MixFrame *__restrict__ frames, uint8_t *__restrict__ dst, MixFmt F, CurveFmt Q)
{
    typedef typename TensorElem<DT>::type elem_t;
    const MixFrame P = frames[blockIdx.z];
    const uint64_t total = (uint64_t)F.out_w * F.out_h;
    elem_t *const img = (elem_t *)dst + P.dst_img;
    curve_stage(curve_lds, Q);

    for (uint64_t it = (uint64_t)blockIdx.x * CMP_THREADS + threadIdx.x; it < total; it += (uint64_t)gridDim.x * CMP_THREADS) {
        uint32_t x, y;
        if (total <= 0xFFFFFFFFull) { y = (uint32_t)it / F.out_w; x = (uint32_t)it - y * F.out_w; }
        else                        { y = (uint32_t)(it / F.out_w); x = (uint32_t)(it - (uint64_t)y * F.out_w); }
        float f[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if ((uint32_t)c >= F.ncomp) break;
            const bool chroma = F.planar && (c == 1 || c == 2);
            const uint32_t sx = (P.ox + x) >> (chroma ? F.sw : 0), sy = (P.oy + y) >> (chroma ? F.sh : 0);
            const int pl = F.planar ? c : 0;
            const uint8_t *p = P.src[pl] + (int64_t)sy * P.ls[pl] + ((uint64_t)sx * F.step + (F.planar ? 0 : c)) * F.bytes;
            uint32_t raw = p[0];
            if (F.bytes == 2) raw |= (uint32_t)p[1] << 8;
            f[c] = (float)((raw >> F.shift) & F.mask);
        }
        curve_in(f, Q, curve_lds);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((uint32_t)k >= F.nout) break;
            const uint64_t at = F.nhwc ? ((uint64_t)y * F.out_w + x) * F.nout + k : ((uint64_t)k * F.out_h + y) * F.out_w + x;
            img[at] = curve_channel<DT>(f, (int)F.ncomp, F, Q, k, curve_lds);
        }
    }
}

/* nimg images of C float32 channels (NCHW, out_w x out_h) at src -> their K channels at element dst_img of dst; one
 * pixel per lane and step.  grid.x strides over all pixels of all images */
template <int DT, int NHWC>
__global__ void __launch_bounds__(CMP_THREADS)
k_tensor_curves(const float *__restrict__ src, uint8_t *__restrict__ dst, uint64_t dst_img, uint32_t nimg, MixFmt F, CurveFmt Q)
{
    typedef typename TensorElem<DT>::type elem_t;
    const uint32_t npix = F.out_w * F.out_h;                 /* both at most 32768: below 2^31 */
    const uint64_t total = (uint64_t)npix * nimg;
    elem_t *const out = (elem_t *)dst + dst_img;
    curve_stage(curve_lds, Q);

    for (uint64_t it = (uint64_t)blockIdx.x * CMP_THREADS + threadIdx.x; it < total; it += (uint64_t)gridDim.x * CMP_THREADS) {
        const uint32_t i = (uint32_t)(it / npix), px = (uint32_t)(it - (uint64_t)i * npix);
        float f[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int c = 0; c < 4; c++)
            if ((uint32_t)c < F.ncomp) f[c] = src[((uint64_t)i * F.ncomp + c) * npix + px];
        curve_in(f, Q, curve_lds);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((uint32_t)k >= F.nout) break;
            const uint64_t at = NHWC ? ((uint64_t)i * npix + px) * F.nout + k : ((uint64_t)i * F.nout + k) * npix + px;
            out[at] = curve_channel<DT>(f, (int)F.ncomp, F, Q, k, curve_lds);
        }
    }
}

#endif /* HTJ2K_TENSOR_IN_ONLY */

} /* namespace htj2k_cmp */
