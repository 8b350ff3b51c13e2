/*
 * mix_kernels.hpp -- frames as tensors through a colour matrix (htj2k_frames_to_tensor_mix and the five calls beside
 * it).  include/htj2k_amd.h has the definition; in short, for output pixel (x, y) of channel k of K:
 *     f_c = (float)s_c, s_c the sample of component c that htj2k_frames_to_tensor reads at that pixel (the same shift, mask
 *           and nearest replication of sub-sampled chroma); or the resampled value of htj2k_frames_to_tensor_resized
 *     a = f_0 * m[k][0];  a = a + (f_c * m[k][c]) for c = 1 .. C - 1 in this order;  t = a + b[k]
 *           every operation one binary32 operation rounded to nearest even, never contracted, no term left out
 *     stored as the plain call stores t: binary32, binary16 or bfloat16, NCHW or NHWC with K in the place of C
 * tensor_mix_value is that arithmetic, once; every kernel here calls it.
 *
 * The plain kernels are cut per frame, not per plane: a mix needs every component of a pixel in one lane.
 *
 *   k_frame_mix      the fast route.  A row of the window is cut into groups of NP pixels (MixShape): what 16 bytes of
 *                    an interleaved plane hold (48 for three interleaved components), 16 bytes of every plane of a planar
 *                    layout without horizontal chroma shift, and with a shift of 1 the pixels of one 16-byte load of each
 *                    chroma plane: two 16-byte loads of luma (and alpha).  A vertical shift is only a choice of row.  Full
 *                    groups are read with 16-byte loads (cmp_load_group), a row's last group byte by byte, only the bytes
 *                    that hold samples.  A group's pixels go out as runs of consecutive elements, NCHW one run per
 *                    channel, NHWC one run of pixels times K; where a group is two or more 16-byte stores per channel,
 *                    SHARE neighbouring lanes take the same group and each converts and stores PART pixels, as
 *                    k_frame_tensor does, so that a wave's store instruction writes side by side.  16-byte stores under
 *                    the frame's `wide` (mix_wide, htj2k_device.hip), else element by element.
 *   k_frame_mix_any  the general route, output-driven: one pixel per lane and step, any origin, chroma shift, alignment
 *                    and layout; a sample is read as its one or two bytes.
 *   k_tensor_mix     the second launch of a resized call with a mix: k_frame_resize has written f_c as float32 NCHW into
 *                    the context's scratch; one pixel per lane and step reads its C values and writes its K elements.
 *
 * No atomics, no LDS, no results.  grid.x strides over a frame's work, grid.z is the frame (tables are launched in chunks
 * of what grid.z takes).  Destination offsets are 64-bit element indices.
 */
#pragma once
#include "tensor_kernels.hpp"

namespace htj2k_cmp {

struct MixFrame {                   /* one frame of a call */
    const uint8_t *src[4];          /* its planes; fast route: the window's first column folded in (ox >> sw_p) */
    int64_t  ls[4];                 /* linesizes, bytes */
    uint64_t dst_img;               /* element index of the frame's image in the destination */
    uint32_t ox, oy;                /* the window's corner, in pixels of the frame (fast route: ox is 0) */
    uint32_t wide;                  /* fast route: every full run of a lane may be written in 16-byte stores */
    uint32_t pad_;
};

struct MixFmt {                     /* uniform over a call */
    uint32_t shift, mask;
    uint32_t out_w, out_h;
    uint32_t ncomp, nout;           /* C components read, K channels written */
    uint32_t bytes;                 /* per sample */
    uint32_t step;                  /* interleaved components of a plane */
    uint32_t planar;                /* component c lives in plane c (else all in plane 0) */
    uint32_t sw, sh;                /* chroma shifts of components 1 and 2 */
    uint32_t nhwc;
    float    m[4][4], b[4];
};

/* the mix, the definition: C terms in their order, each product and each sum rounded on its own, then the element */
template <int DT>
__device__ __forceinline__ typename TensorElem<DT>::type tensor_mix_value(const float f[4], int C, const float *__restrict__ m, float b)
{
    float a = __fmul_rn(f[0], m[0]);
#pragma unroll
    for (int c = 1; c < 4; c++)
        if (c < C) a = __fadd_rn(a, __fmul_rn(f[c], m[c]));
    return tensor_value_f<DT>(a, 1.0f, b);               /* a * 1 is a, whatever a is: t = a + b, then the plain call's conversion */
}

/* the fast route's cut.  NPL planes of STEP interleaved components each (a planar layout: STEP 1; any other: NPL 1), SW
 * the horizontal chroma shift of planes 1 and 2 (0, 1) */
template <int BYTES, int STEP, int NPL, int SW, int DT> struct MixShape {
    static constexpr int C = NPL > 1 ? NPL : STEP;
    static constexpr int GROUP = NPL > 1 ? (16 << SW) : (STEP == 3 ? 48 : 16);   /* bytes of a group in a full-size plane */
    static constexpr int NP = GROUP / (STEP * BYTES);            /* pixels of a group */
    static constexpr int PER = DT == TENSOR_F32 ? 4 : 8;         /* elements of a 16-byte store */
    static constexpr int SHARE = (NP % PER == 0 && NP / PER >= 2) ? NP / PER : 1;
    static constexpr int PART = NP / SHARE;                      /* pixels a lane converts */
};

/* a lane's PART pixels of K channels as one NHWC run */
template <int K, int PART, class T>
__device__ __forceinline__ void mix_store_nhwc(T *o, const T (&v)[4][PART], uint32_t n, bool wide)
{
    T u[PART * K];
#pragma unroll
    for (int p = 0; p < PART; p++)
#pragma unroll
        for (int k = 0; k < K; k++) u[p * K + k] = v[k][p];
    tensor_store_run<PART * K>(o, u, n * K, wide);
}

template <int BYTES, int STEP, int NPL, int SW, int DT, int NHWC>
__global__ void __launch_bounds__(CMP_THREADS)
k_frame_mix(const MixFrame *__restrict__ frames, uint8_t *__restrict__ dst, MixFmt F)
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
        /* the part's samples are picked with indices known at compile time: one branch per part, the stores after them */
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
#pragma unroll
                for (int kk = 0; kk < 4; kk++)
                    if ((uint32_t)kk < K) v[kk][k] = tensor_mix_value<DT>(f, C, F.m[kk], F.b[kk]);
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
k_frame_mix_any(const MixFrame *__restrict__ frames, uint8_t *__restrict__ dst, MixFmt F)
{
    typedef typename TensorElem<DT>::type elem_t;
    const MixFrame P = frames[blockIdx.z];
    const uint64_t total = (uint64_t)F.out_w * F.out_h;
    elem_t *const img = (elem_t *)dst + P.dst_img;

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
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((uint32_t)k >= F.nout) break;
            const uint64_t at = F.nhwc ? ((uint64_t)y * F.out_w + x) * F.nout + k : ((uint64_t)k * F.out_h + y) * F.out_w + x;
            img[at] = tensor_mix_value<DT>(f, (int)F.ncomp, F.m[k], F.b[k]);
        }
    }
}

/* nimg images of C float32 channels (NCHW, out_w x out_h) at src -> their K channels at element dst_img of dst; one
 * pixel per lane and step.  grid.x strides over all pixels of all images */
template <int DT, int NHWC>
__global__ void __launch_bounds__(CMP_THREADS)
k_tensor_mix(const float *__restrict__ src, uint8_t *__restrict__ dst, uint64_t dst_img, uint32_t nimg, MixFmt F)
{
    typedef typename TensorElem<DT>::type elem_t;
    const uint32_t npix = F.out_w * F.out_h;                 /* both at most 32768: below 2^31 */
    const uint64_t total = (uint64_t)npix * nimg;
    elem_t *const out = (elem_t *)dst + dst_img;

    for (uint64_t it = (uint64_t)blockIdx.x * CMP_THREADS + threadIdx.x; it < total; it += (uint64_t)gridDim.x * CMP_THREADS) {
        const uint32_t i = (uint32_t)(it / npix), px = (uint32_t)(it - (uint64_t)i * npix);
        float f[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int c = 0; c < 4; c++)
            if ((uint32_t)c < F.ncomp) f[c] = src[((uint64_t)i * F.ncomp + c) * npix + px];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((uint32_t)k >= F.nout) break;
            const uint64_t at = NHWC ? ((uint64_t)i * npix + px) * F.nout + k : ((uint64_t)i * F.nout + k) * npix + px;
            out[at] = tensor_mix_value<DT>(f, (int)F.ncomp, F.m[k], F.b[k]);
        }
    }
}

} /* namespace htj2k_cmp */
