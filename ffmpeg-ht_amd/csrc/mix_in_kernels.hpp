/*
 * mix_in_kernels.hpp -- tensors as frames through a colour matrix and a chroma filter (htj2k_tensor_to_frames_mix,
 * htj2k_encode_tensor_mix).  include/htj2k_amd.h has the definition; in short, for sample (x, y) of component c of a
 * tensor of K channels:
 *     footprint  the elements (X, Y), x << sw_c <= X < min((x + 1) << sw_c, W), the same for Y: N of them, 1 .. 16
 *     gather     g_k = the element at the footprint's first corner (co-sited, or N = 1); or (box) the elements of channel k
 *                added in raster order, one binary32 addition each, times rcp_N, the binary32 nearest to 1 / N
 *     mix        a = g_0 * m[c][0];  a = a + (g_k * m[c][k]) for k = 1 .. K - 1 in this order;  u = a + b[c]
 *                every operation one binary32 operation rounded to nearest even, never contracted, no term left out
 *     sample     r = rintf(u); 0 unless r > 0; 2^bits - 1 where r reaches it; else (uint)r: tensor_in_sample's end
 * mix_in_gather and mix_in_sample are that arithmetic, once: the encoder's k_enc_unpack_tensor_mix (enc_kernels.hpp) and
 * k_tensor_frame_mix below both call them, so a codestream and a frame made from one tensor cannot differ.
 *
 *   k_tensor_frame_mix   output-driven, as k_tensor_frame: one sample word per lane and step, its footprint gathered
 *                        for that sample alone, s << shift as the one or two bytes of the sample, whatever the plane's
 *                        base and linesize.
 *
 * Every load is one element: no load is wider than the tensor's own alignment proves.  No atomics, no LDS.
 * A translation unit that wants the device functions alone (htj2k_encode.hip) defines HTJ2K_TENSOR_IN_ONLY, as for
 * tensor_kernels.hpp.
 */
#pragma once
#include "tensor_kernels.hpp"

namespace htj2k_cmp {

struct MixIn {                      /* the mix of a call, uniform over it */
    uint32_t nin;                   /* K: channels of an image of the tensor */
    uint32_t box;                   /* HTJ2K_CHROMA_BOX: footprints of more than one element are averaged */
    float    m[4][4], b[4];         /* m[c][k]: weight of channel k in component c */
};

/* rcp_N of the four footprints a plane can have: [rows clipped][columns clipped] */
struct MixInRcp { float r[2][2]; };

/* one footprint: nx x ny elements of every channel from (X0, Y0) on, of an image of K channels, H x W, whose first
 * element is `img` -> g[0 .. K).  `each(fx, fy, f)` sees every element's K values once, in raster order, as they are
 * loaded: the encoder takes its full-resolution components from there, so that no element is loaded twice.
 * The sum starts from the first element itself (not from 0 + it: -0 stays -0) */
template <int DT, int NHWC, class Each>
__device__ __forceinline__ void mix_in_gather(const void *__restrict__ img, uint32_t X0, uint32_t Y0, uint32_t nx, uint32_t ny, bool box,
                                              float rcp, uint32_t K, uint32_t W, uint32_t H, float g[4], Each each)
{
    g[0] = g[1] = g[2] = g[3] = 0.0f;
    for (uint32_t fy = 0; fy < ny; fy++)
        for (uint32_t fx = 0; fx < nx; fx++) {
            float f[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int k = 0; k < 4; k++)
                if ((uint32_t)k < K) f[k] = tensor_in_value<DT>(img, tensor_in_at<NHWC>((uint32_t)k, X0 + fx, Y0 + fy, K, W, H));
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

/* one row of the mix down to the sample of `bits` bits, peak = 2^bits - 1: all K terms in their order, then
 * tensor_in_sample's rounding and clamp */
__device__ __forceinline__ uint32_t mix_in_sample(const float g[4], uint32_t K, const float *__restrict__ m, float b, uint32_t peak)
{
    float a = __fmul_rn(g[0], m[0]);
#pragma unroll
    for (int k = 1; k < 4; k++)
        if ((uint32_t)k < K) a = __fadd_rn(a, __fmul_rn(g[k], m[k]));
    const float r = rintf(__fadd_rn(a, b));
    if (!(r > 0.0f)) return 0;
    if (r >= (float)peak) return peak;
    return (uint32_t)r;
}

/* rcp_N of a footprint of nx x ny elements in a plane whose full footprints are fw x fh */
__device__ __forceinline__ float mix_in_rcp(const MixInRcp &R, uint32_t nx, uint32_t ny, uint32_t fw, uint32_t fh)
{
    const float full_rows = nx == fw ? R.r[0][0] : R.r[0][1], cut_rows = nx == fw ? R.r[1][0] : R.r[1][1];
    return ny == fh ? full_rows : cut_rows;
}

#ifndef HTJ2K_TENSOR_IN_ONLY

struct MixInPlane {                 /* one destination plane of one frame */
    TensorInPlane P;
    MixInRcp rcp;                   /* of the plane's footprints (1 << sw) x (1 << sh), and clipped at the last column and row */
};

/* k_tensor_frame with a mix: one sample word per lane and step, in the order of the plane's bytes; only the bytes of
 * samples are written.  grid.x strides over them, grid.z is the plane */
template <int DT>
__global__ void __launch_bounds__(CMP_THREADS)
k_tensor_frame_mix(const MixInPlane *__restrict__ planes, const uint8_t *__restrict__ src, TensorInFmt F, MixIn M)
{
    typedef typename TensorElem<DT>::type elem_t;
    const TensorInPlane P = planes[blockIdx.z].P;
    const MixInRcp R = planes[blockIdx.z].rcp;
    const uint64_t total = (uint64_t)P.step * P.pw * P.ph;
    const elem_t *const img = (const elem_t *)src + P.src_img;
    const uint32_t fw = 1u << P.sw, fh = 1u << P.sh;

    for (uint64_t it = (uint64_t)blockIdx.x * CMP_THREADS + threadIdx.x; it < total; it += (uint64_t)gridDim.x * CMP_THREADS) {
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
        if (F.nhwc) mix_in_gather<DT, 1>(img, X0, Y0, nx, ny, M.box != 0, mix_in_rcp(R, nx, ny, fw, fh), M.nin, F.w, F.h, g, nothing);
        else        mix_in_gather<DT, 0>(img, X0, Y0, nx, ny, M.box != 0, mix_in_rcp(R, nx, ny, fw, fh), M.nin, F.w, F.h, g, nothing);
        float row[4] = { M.m[0][0], M.m[0][1], M.m[0][2], M.m[0][3] }, off = M.b[0];    /* picked by comparisons: no indexed copy of M */
#pragma unroll
        for (int q = 1; q < 4; q++)
            if (k == (uint32_t)q) { row[0] = M.m[q][0]; row[1] = M.m[q][1]; row[2] = M.m[q][2]; row[3] = M.m[q][3]; off = M.b[q]; }
        const uint32_t word = mix_in_sample(g, M.nin, row, off, F.peak) << F.shift;
        uint8_t *p = P.dst + (int64_t)y * P.ls + ((uint64_t)x * P.step + c) * F.bytes;
        p[0] = (uint8_t)word;
        if (F.bytes == 2) p[1] = (uint8_t)(word >> 8);
    }
}

#endif /* HTJ2K_TENSOR_IN_ONLY */

} /* namespace htj2k_cmp */
