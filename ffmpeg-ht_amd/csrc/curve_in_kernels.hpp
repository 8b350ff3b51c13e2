/*
 * curve_in_kernels.hpp -- tensors as frames through a transfer curve, a colour matrix, a second curve and a gain
 * (htj2k_tensor_to_frames_curves, htj2k_encode_tensor_curves).  include/htj2k_amd.h has the definition ("tensors as
 * frames, with curves"); in short, for sample (x, y) of component c of a tensor of K channels:
 *     footprint  as the mix's (mix_in_kernels.hpp)
 *     in-curve   h_k = R(f_k; in) on every element of the footprint where bit k of in_mask is set, else f_k
 *     gather     the mix's rule on h: the corner, or the box sum in raster order times rcp_N
 *     mix        a = g_0 * m[c][0];  a = a + (g_k * m[c][k]), k = 1 .. K - 1;  u = a + b[c]
 *     out-curve  v = R(u; out) where bit c of out_mask is set, else u
 *     normalise  w = v * gain[c] + offset[c], two rounded operations
 *     sample     r = rintf(w); 0 unless r > 0; 2^bits - 1 where r reaches it; else (uint)r
 * R(x; curve) with root r: p = x (r = 0), else p = fmaxf(x, 0) square-rooted r times, each root correctly rounded; then
 * curve_eval's E(p) (curve_kernels.hpp).  curve_in_root and curve_in_sample are that arithmetic, once: the encoder's
 * k_enc_unpack_tensor_curves (enc_kernels.hpp) and k_tensor_frame_curves below both call them, so a codestream and a
 * frame made from one tensor cannot differ.  The roots are sqrtf, which this toolchain compiles to the correctly rounded
 * sequence (denormals included); __fsqrt_rn is v_sqrt_f32 alone here, one ulp off now and then, and is not used.
 *
 *   k_tensor_frame_curves   output-driven, as k_tensor_frame_mix: one sample word per lane and step.
 *
 * Both tables live in dynamic LDS, staged once per workgroup as curve_kernels.hpp stages them: n + 1 floats each
 * (t[n] = t[n-1], written by the host), padded to 16 bytes, 32 800 bytes at the most; every index is clamped to
 * 0 .. n - 1 by curve_eval, so no read leaves a table.  Every tensor load is one element.  No atomics.
 * A translation unit that wants the device functions alone (htj2k_encode.hip) defines HTJ2K_TENSOR_IN_ONLY.
 */
#pragma once
#include <string.h>
#include <vector>
#include "../../include/htj2k_amd.h"
#include "curve_kernels.hpp"
#include "mix_in_kernels.hpp"

namespace htj2k_cmp {

#define CURVE_IN_THREADS 256        /* of both kernels: four waves share one staging of the tables */

struct CurveInFmt {                 /* uniform over a call */
    const float *tab;               /* device, 16-byte aligned: the in-table, then the out-table at float `out_at` */
    uint32_t n_in, n_out;           /* knots; 0: no curve (its mask is then 0) */
    uint32_t out_at, nfloat;        /* multiples of 4; nfloat: floats of both tables */
    float    x0_in, inv_in, x0_out, inv_out;
    uint32_t root_in, root_out;     /* square roots taken before the lookup, 0 .. 3 */
    uint32_t in_mask, out_mask;     /* tensor channels; components */
    float    gain[4], offset[4];    /* per component */
};

/* floats of a table in the upload and in LDS: its n knots and t[n] = t[n-1], padded to 16 bytes; 0 without a curve */
static inline size_t curve_in_floats(const htj2k_tensor_curve_in &v) { return v.n ? ((size_t)v.n + 1 + 3) & ~(size_t)3 : 0; }

/* checked curves -> what the kernels get (tab is filled in by the caller once the tables are on the device) and the
 * tables as they are uploaded; C: components of the layout */
static inline CurveInFmt curve_in_fmt(const htj2k_tensor_curves_in &q, int C, std::vector<float> *tab)
{
    CurveInFmt Q;
    memset(&Q, 0, sizeof Q);
    const htj2k_tensor_curve_in *cv[2] = { &q.in, &q.out };
    tab->assign(curve_in_floats(q.in) + curve_in_floats(q.out), 0.0f);
    size_t at = 0;
    for (const htj2k_tensor_curve_in *v : cv) {
        const size_t nf = curve_in_floats(*v);
        for (size_t j = 0; j < nf; j++) (*tab)[at + j] = v->t[j < (size_t)v->n ? j : (size_t)v->n - 1];
        at += nf;
    }
    Q.n_in = (uint32_t)q.in.n; Q.n_out = (uint32_t)q.out.n;
    Q.out_at = (uint32_t)curve_in_floats(q.in); Q.nfloat = (uint32_t)tab->size();
    if (q.in.n)  { Q.x0_in = q.in.x0;   Q.inv_in = q.in.inv_dx;   Q.root_in = (uint32_t)q.in.root;   Q.in_mask = q.in_mask; }
    if (q.out.n) { Q.x0_out = q.out.x0; Q.inv_out = q.out.inv_dx; Q.root_out = (uint32_t)q.out.root; Q.out_mask = q.out_mask; }
    for (int c = 0; c < C; c++) { Q.gain[c] = q.gain[c]; Q.offset[c] = q.offset[c]; }
    return Q;
}

/* R(x; curve): the root, then E.  fmaxf gives the operand that is not NaN, so a NaN becomes 0 */
__device__ __forceinline__ float curve_in_root(float x, uint32_t root, const float *__restrict__ t, uint32_t n, float x0, float inv_dx)
{
    float p = x;
    if (root) {
        p = fmaxf(x, 0.0f);
        for (uint32_t r = 0; r < root; r++) p = sqrtf(p);
    }
    return curve_eval(p, t, n, x0, inv_dx);
}

/* both tables into LDS, 16 bytes a lane and step; every lane of the workgroup calls it once */
__device__ __forceinline__ void curve_in_stage(float *__restrict__ lds, const CurveInFmt &Q)
{
    for (uint32_t q = threadIdx.x; q < Q.nfloat / 4; q += CURVE_IN_THREADS) ((uint4 *)lds)[q] = ((const uint4 *)Q.tab)[q];
    __syncthreads();
}

/* mix_in_gather with the in-curve: every element's K values go through it as they are loaded, before they are added
 * and before `each` sees them, so a chroma sample is the mean of curved values */
template <int DT, int NHWC, class Each>
__device__ __forceinline__ void curve_in_gather(const void *__restrict__ img, uint32_t X0, uint32_t Y0, uint32_t nx, uint32_t ny, bool box,
                                                float rcp, uint32_t K, uint32_t W, uint32_t H, float g[4], const CurveInFmt &Q,
                                                const float *__restrict__ lds, Each each)
{
    g[0] = g[1] = g[2] = g[3] = 0.0f;
    for (uint32_t fy = 0; fy < ny; fy++)
        for (uint32_t fx = 0; fx < nx; fx++) {
            float f[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int k = 0; k < 4; k++)
                if ((uint32_t)k < K) {
                    f[k] = tensor_in_value<DT>(img, tensor_in_at<NHWC>((uint32_t)k, X0 + fx, Y0 + fy, K, W, H));
                    if ((Q.in_mask >> k) & 1u) f[k] = curve_in_root(f[k], Q.root_in, lds, Q.n_in, Q.x0_in, Q.inv_in);
                }
            const bool first = (fx | fy) == 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                g[k] = first ? f[k] : box ? __fadd_rn(g[k], f[k]) : g[k];
            each(fx, fy, f);
        }
    if (box && nx * ny > 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = __fmul_rn(g[k], rcp);
    }
}

/* the component's end: one row of the mix (all K terms in their order), the out-curve where `curved`, gain and offset,
 * then tensor_in_sample's rounding and clamp to `bits` bits, peak = 2^bits - 1 */
__device__ __forceinline__ uint32_t curve_in_sample(const float g[4], uint32_t K, const float *__restrict__ m, float b, bool curved,
                                                    const CurveInFmt &Q, const float *__restrict__ lds, float gain, float offset, uint32_t peak)
{
    float a = __fmul_rn(g[0], m[0]);
#pragma unroll
    for (int k = 1; k < 4; k++)
        if ((uint32_t)k < K) a = __fadd_rn(a, __fmul_rn(g[k], m[k]));
    float v = __fadd_rn(a, b);
    if (curved) v = curve_in_root(v, Q.root_out, lds + Q.out_at, Q.n_out, Q.x0_out, Q.inv_out);
    const float r = rintf(__fadd_rn(__fmul_rn(v, gain), offset));
    if (!(r > 0.0f)) return 0;
    if (r >= (float)peak) return peak;
    return (uint32_t)r;
}

extern __shared__ __align__(16) float curve_in_lds[];

#ifndef HTJ2K_TENSOR_IN_ONLY

/* k_tensor_frame_mix with curves: one sample word per lane and step, in the order of the plane's bytes; only the bytes
 * of samples are written.  grid.x strides over them, grid.z is the plane */
template <int DT>
__global__ void __launch_bounds__(CURVE_IN_THREADS)
k_tensor_frame_curves(const MixInPlane *__restrict__ planes, const uint8_t *__restrict__ src, TensorInFmt F, MixIn M, CurveInFmt Q)
{
    typedef typename TensorElem<DT>::type elem_t;
    const TensorInPlane P = planes[blockIdx.z].P;
    const MixInRcp R = planes[blockIdx.z].rcp;
    const uint64_t total = (uint64_t)P.step * P.pw * P.ph;
    const elem_t *const img = (const elem_t *)src + P.src_img;
    const uint32_t fw = 1u << P.sw, fh = 1u << P.sh;
    curve_in_stage(curve_in_lds, Q);

    for (uint64_t it = (uint64_t)blockIdx.x * CURVE_IN_THREADS + threadIdx.x; it < total; it += (uint64_t)gridDim.x * CURVE_IN_THREADS) {
        uint32_t x, y, c;
        if (total <= 0xFFFFFFFFull) {
            const uint32_t e = (uint32_t)it, r = e / P.step;
            c = e - r * P.step; y = r / P.pw; x = r - y * P.pw;
        } else {
            const uint64_t r = it / P.step;
            c = (uint32_t)(it - r * P.step); y = (uint32_t)(r / P.pw); x = (uint32_t)(r - (uint64_t)y * P.pw);
        }
        const uint32_t k = P.comp0 + c;
        const uint32_t X0 = x << P.sw, Y0 = y << P.sh;           /* inside the image: pw and ph are the ceilinged sizes */
        const uint32_t nx = M.box ? min(fw, F.w - X0) : 1, ny = M.box ? min(fh, F.h - Y0) : 1;   /* co-sited: the corner alone */
        float g[4];
        const auto nothing = [](uint32_t, uint32_t, const float *) {};
        if (F.nhwc) curve_in_gather<DT, 1>(img, X0, Y0, nx, ny, M.box != 0, mix_in_rcp(R, nx, ny, fw, fh), M.nin, F.w, F.h, g, Q, curve_in_lds, nothing);
        else        curve_in_gather<DT, 0>(img, X0, Y0, nx, ny, M.box != 0, mix_in_rcp(R, nx, ny, fw, fh), M.nin, F.w, F.h, g, Q, curve_in_lds, nothing);
        float row[4] = { M.m[0][0], M.m[0][1], M.m[0][2], M.m[0][3] }, off = M.b[0];    /* picked by comparisons: no indexed copy of M */
        float gain = Q.gain[0], offset = Q.offset[0];
#pragma unroll
        for (int q = 1; q < 4; q++)
            if (k == (uint32_t)q) {
                row[0] = M.m[q][0]; row[1] = M.m[q][1]; row[2] = M.m[q][2]; row[3] = M.m[q][3]; off = M.b[q];
                gain = Q.gain[q]; offset = Q.offset[q];
            }
        const uint32_t word = curve_in_sample(g, M.nin, row, off, ((Q.out_mask >> k) & 1u) != 0, Q, curve_in_lds, gain, offset, F.peak) << F.shift;
        uint8_t *p = P.dst + (int64_t)y * P.ls + ((uint64_t)x * P.step + c) * F.bytes;
        p[0] = (uint8_t)word;
        if (F.bytes == 2) p[1] = (uint8_t)(word >> 8);
    }
}

#endif /* HTJ2K_TENSOR_IN_ONLY */

} /* namespace htj2k_cmp */
