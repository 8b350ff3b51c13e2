/*
 * enc_kernels.hpp -- device stages of the HTJ2K encoder (htj2k_encode.hip).
 *
 *   k_enc_unpack   frame samples -> int32 component planes: the inverse of the decoder's pack
 *                  stage (pack_kernels.hpp: value >> (precision - cbps)), DC level shift and the
 *                  forward RCT (T.800 G.2.1) of components 0..2; with IRREV float planes and the
 *                  forward ICT (T.800 G.3) instead
 *   k_enc_unpack_tensor  the same stage for a call whose input is a float tensor, NCHW or NHWC (htj2k_encode_tensor)
 *   k_enc_unpack_tensor_mix  ... through a colour matrix and a chroma filter (htj2k_encode_tensor_mix), a lane per
 *                  chroma footprint
 *   k_enc_unpack_tensor_curves  ... with a transfer curve before the matrix and one after it (htj2k_encode_tensor_curves):
 *                  the tables staged into LDS, a workgroup walking a frame's footprints in a grid-stride loop
 *   k_fdwt97_v/_h  one forward 9/7 level, laid out as the 5/3 one: float lifting, every step
 *                  x + c * (left + right) on whole-sample symmetric extension, one output per
 *                  thread (fdwt97_out); a line of one sample is scaled by 1 / X at an even position,
 *                  by 2 / K at an odd one
 *   k_quant97      float 9/7 coefficients -> signed int32 indices in place, each band of every
 *                  tile-component by the decoder's step for it (dead zone, float64 division)
 *   k_fdwt_v/_h    one forward 5/3 level (T.800 F.4.8.2, symmetric extension) of the LL region of
 *                  every tile-component, whatever its origin: vertical into a scratch plane,
 *                  horizontal back, the samples at even positions (low-pass) first -- the Mallat
 *                  layout of the decoder's coefficient planes.  Each output sample is computed from
 *                  its five input neighbours in closed form.
 *   k_ht_encode    the HT cleanup pass of one code-block per wavefront (T.814 clause 7 read
 *                  backwards), byte for byte what the reference vector factory writes:
 *                    1. exponents E of every sample (lanes over quads) into LDS
 *                    2. per quad: context, kappa, U, u, eps and the CxtVLC codeword (lanes)
 *                    3. MagSgn bits: per-lane bit counts, a wave prefix sum, and every field
 *                       OR'ed into an LDS bit array at its offset (lanes)
 *                    4. the byte-after-0xFF rule: lanes cut the unstuffed array into bytes, 64 per
 *                       window, up to the next full 0xFF; the next window starts behind it with 7
 *                       bits in its first byte (a window per 64 bytes or per 0xFF)
 *                    5. MEL and VLC (lane 0; their order is inherently sequential), Scup patch
 *                  A block may be coded from a higher bit-plane (EncBlk.plane, rate control): mag_at
 *                  shifts the magnitude at the two coefficient reads, nothing else changes.
 *                  What stages 1, 2 and 5 code is stated by the quad rules (mag_at, enc_expn, quad_code,
 *                  uvlc_split, uvlc_pair), device functions on register values that k_rc_stats counts by.
 *   k_ht_refine_plan / k_ht_refine_encode
 *                  blocks of 2 or 3 passes: which of them fall back to one pass (before k_ht_encode), and the
 *                  SigProp and MagRef passes of the others, a wave per block, behind the cleanup segment
 *   k_rc_stats     rate control: per block and bit-plane p the distortion of dropping p planes and an
 *                  estimate of the cleanup segment's length, from one read of the coefficients
 *   k_rc_select    rate control: per frame the plane of every block (or "left out") that minimises the
 *                  weighted distortion under the byte budget, by bisection on the slope
 *   k_rc_group_sweep / _step / _apply, k_rc_select_q
 *                  the same search under one budget over the frames of a call, and under a PSNR target.  Every
 *                  selection takes a block's candidate from rc_cand (rc_pick and the plane-0 rules) and writes it
 *                  with rc_store; the sums are rc_wave_sum and rc_block_sum, the maximum rc_block_max
 *   k_enc_gather   headers and block bytes into the final codestreams (a workgroup per piece)
 *   k_xc_scatter   transcoding: the block decoder's tile-component planes into the component planes
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#define HTJ2K_TENSOR_IN_ONLY        /* the definition of a sample from a tensor element, without the decoder side's kernels */
#include "tensor_kernels.hpp"
#include "mix_in_kernels.hpp"
#include "curve_in_kernels.hpp"

namespace htj2k_enc {

struct UnpackArgs {                 /* one frame */
    const uint8_t *src[4];          /* planes of the input layout */
    int64_t  linesize[4];
    int32_t *dst[4];                /* component planes, row stride cw */
    int32_t  cw[4], ch[4];
    int32_t  w, h;
};

struct UnpackFmt {                  /* uniform over a batch */
    int32_t ncomp, planar, step, bytes, shift, bits, mct;
};

/* IRREV: float samples and the ICT (the planes of `dst` then hold floats) */
template <bool IRREV>
__global__ void __launch_bounds__(256)
k_enc_unpack(const UnpackArgs *__restrict__ frames, UnpackFmt F)
{
    const UnpackArgs &A = frames[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= A.w || y >= A.h)
        return;
    int v[4] = { 0, 0, 0, 0 };
    bool in[4] = { false, false, false, false };
    const uint32_t mask = (1u << F.bits) - 1;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (c >= F.ncomp || x >= A.cw[c] || y >= A.ch[c])
            continue;
        const int p = F.planar ? c : 0;
        const uint8_t *row = A.src[p] + (size_t)y * A.linesize[p];
        const size_t idx = F.planar ? (size_t)x : (size_t)x * F.step + c;
        const uint32_t s = F.bytes == 1 ? row[idx] : (uint32_t)row[2 * idx] | ((uint32_t)row[2 * idx + 1] << 8);
        v[c] = (int)((s >> F.shift) & mask) - (1 << (F.bits - 1));
        in[c] = true;
    }
    if (IRREV) {
        float f[4] = { (float)v[0], (float)v[1], (float)v[2], (float)v[3] };
        if (F.mct) {                                     /* ICT: the constants and operand order of the vector factory */
            const float r = f[0], g = f[1], b = f[2];
            f[0] =  0.299f * r + 0.587f * g + 0.114f * b;
            f[1] = -0.168736f * r - 0.331264f * g + 0.5f * b;
            f[2] =  0.5f * r - 0.418688f * g - 0.081312f * b;
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (in[c])
                ((float *)A.dst[c])[(size_t)y * A.cw[c] + x] = f[c];
        return;
    }
    if (F.mct) {                                         /* RCT: Y = (R + 2G + B) >> 2, Cb = B - G, Cr = R - G */
        const int r = v[0], g = v[1], b = v[2];
        v[0] = (r + 2 * g + b) >> 2;
        v[1] = b - g;
        v[2] = r - g;
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
        if (in[c])
            A.dst[c][(size_t)y * A.cw[c] + x] = v[c];
}

struct UnpackTensorArgs {           /* one frame of a tensor call, or a band of UNPACK_ROWS rows of it */
    const void *src;                /* the frame's image in the tensor: its first element */
    int32_t *dst[4];                /* component planes from the band's first row on, row stride cw */
    int32_t  cw[4], ch[4];          /* ch: the component's rows from the band's first row on */
    int32_t  w, h;                  /* the image's width; its rows from the band's first row on */
    int32_t  y0, ih;                /* the band's first row (of every component, in the component's own rows); the image's rows */
};

struct UnpackTensorFmt {            /* uniform over a batch */
    int32_t ncomp, bits, mct, pad_;
    int32_t sw[4], sh[4];           /* chroma shifts per component */
    float   scale[4], bias[4];
};

/* k_enc_unpack for a call whose input is a float tensor (htj2k_encode_tensor): the same grid, the same thread per
 * position, the same component transform and stores; the sample comes from tensor_in_sample (tensor_kernels.hpp),
 * the definition that htj2k_tensor_to_frames writes frames by.  DT the element, NHWC the tensor's layout */
template <bool IRREV, int DT, int NHWC>
__global__ void __launch_bounds__(256)
k_enc_unpack_tensor(const UnpackTensorArgs *__restrict__ frames, UnpackTensorFmt F)
{
    const UnpackTensorArgs &A = frames[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= A.w || y >= A.h)
        return;
    int v[4] = { 0, 0, 0, 0 };
    bool in[4] = { false, false, false, false };
    const uint32_t peak = (1u << F.bits) - 1;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (c >= F.ncomp || x >= A.cw[c] || y >= A.ch[c])
            continue;
        const uint64_t at = htj2k_cmp::tensor_in_at<NHWC>((uint32_t)c, (uint32_t)x << F.sw[c], (uint32_t)(A.y0 + y) << F.sh[c],
                                                          (uint32_t)F.ncomp, (uint32_t)A.w, (uint32_t)A.ih);
        v[c] = (int)htj2k_cmp::tensor_in_sample<DT>(A.src, at, F.scale[c], F.bias[c], peak) - (1 << (F.bits - 1));
        in[c] = true;
    }
    /* from here on k_enc_unpack, line for line: the equality tests of tests/test_tensor_in_gpu.py hold the two together */
    if (IRREV) {
        float f[4] = { (float)v[0], (float)v[1], (float)v[2], (float)v[3] };
        if (F.mct) {                                     /* ICT: the constants and operand order of the vector factory */
            const float r = f[0], g = f[1], b = f[2];
            f[0] =  0.299f * r + 0.587f * g + 0.114f * b;
            f[1] = -0.168736f * r - 0.331264f * g + 0.5f * b;
            f[2] =  0.5f * r - 0.418688f * g - 0.081312f * b;
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (in[c])
                ((float *)A.dst[c])[(size_t)y * A.cw[c] + x] = f[c];
        return;
    }
    if (F.mct) {                                         /* RCT: Y = (R + 2G + B) >> 2, Cb = B - G, Cr = R - G */
        const int r = v[0], g = v[1], b = v[2];
        v[0] = (r + 2 * g + b) >> 2;
        v[1] = b - g;
        v[2] = r - g;
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
        if (in[c])
            A.dst[c][(size_t)y * A.cw[c] + x] = v[c];
}

struct UnpackTensorMixFmt {         /* uniform over a batch with a mix */
    int32_t ncomp, bits, mct;
    int32_t sw, sh;                 /* the layout's chroma shifts: a footprint is (1 << sw) x (1 << sh) pixels */
    htj2k_cmp::MixIn mix;
    htj2k_cmp::MixInRcp rcp;
};

/* one sample of a component plane: the int32 of the 5/3 path, or (IRREV) its float */
template <bool IRREV>
__device__ __forceinline__ void unpack_store(int32_t *plane, size_t at, int v)
{
    if (IRREV) ((float *)plane)[at] = (float)v;
    else       plane[at] = v;
}

/* k_enc_unpack_tensor for a call with a mix (htj2k_encode_tensor_mix).  The stage is cut by chroma footprint: a lane owns
 * the (1 << sw) x (1 << sh) pixels of one footprint of the layout (one pixel where nothing is sub-sampled), loads each of
 * their K elements once (mix_in_gather), gives every pixel its sample of the full-resolution components as it passes,
 * and the footprint its one sample of each chroma component.  The table's entries are bands of footprint rows:
 * A.y0 is the band's first footprint row, A.h the footprint rows from there on, A.w and A.ih the image's size, A.dst[c]
 * the component's plane from the band's first row of its own on.  blockIdx.x * 256 + threadIdx.x is the footprint's
 * column.  The samples are mix_in_sample's, which htj2k_tensor_to_frames_mix writes frames by */
template <bool IRREV, int DT, int NHWC>
__global__ void __launch_bounds__(256)
k_enc_unpack_tensor_mix(const UnpackTensorArgs *__restrict__ frames, UnpackTensorMixFmt F)
{
    const UnpackTensorArgs &A = frames[blockIdx.z];
    const uint32_t fw = 1u << F.sw, fh = 1u << F.sh;
    const uint32_t x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const uint32_t X0 = x << F.sw, Y0 = ((uint32_t)A.y0 + y) << F.sh;
    if (X0 >= (uint32_t)A.w || y >= (uint32_t)A.h)
        return;
    const uint32_t nx = min(fw, (uint32_t)A.w - X0), ny = min(fh, (uint32_t)A.ih - Y0);
    const uint32_t peak = (1u << F.bits) - 1, K = F.mix.nin;
    const int dc = 1 << (F.bits - 1);
    const bool box = F.mix.box != 0;
    const float rcp = htj2k_cmp::mix_in_rcp(F.rcp, nx, ny, fw, fh);
    float g[4];
    if (F.sw | F.sh) {
        /* sub-sampled: components 0 and 3 at every pixel as it is loaded, 1 and 2 once from the gathered footprint.  No
         * component transform here: the encoder has one for the RGB family alone, which has no chroma shift */
        const size_t row0 = (size_t)(y << F.sh);
        htj2k_cmp::mix_in_gather<DT, NHWC>(A.src, X0, Y0, nx, ny, box, rcp, K, (uint32_t)A.w, (uint32_t)A.ih, g,
            [&](uint32_t fx, uint32_t fy, const float *f) {
                const size_t at = (row0 + fy) * A.cw[0] + X0 + fx;
                unpack_store<IRREV>(A.dst[0], at, (int)htj2k_cmp::mix_in_sample(f, K, F.mix.m[0], F.mix.b[0], peak) - dc);
                if (F.ncomp > 3)
                    unpack_store<IRREV>(A.dst[3], at, (int)htj2k_cmp::mix_in_sample(f, K, F.mix.m[3], F.mix.b[3], peak) - dc);
            });
#pragma unroll
        for (int c = 1; c < 3; c++)
            unpack_store<IRREV>(A.dst[c], (size_t)y * A.cw[c] + x, (int)htj2k_cmp::mix_in_sample(g, K, F.mix.m[c], F.mix.b[c], peak) - dc);
        return;
    }
    htj2k_cmp::mix_in_gather<DT, NHWC>(A.src, X0, Y0, 1, 1, box, rcp, K, (uint32_t)A.w, (uint32_t)A.ih, g, [](uint32_t, uint32_t, const float *) {});
    int v[4] = { 0, 0, 0, 0 };
    bool in[4] = { false, false, false, false };
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (c >= F.ncomp)
            continue;
        v[c] = (int)htj2k_cmp::mix_in_sample(g, K, F.mix.m[c], F.mix.b[c], peak) - dc;
        in[c] = true;
    }
    /* from here on k_enc_unpack, line for line: the equality tests of tests/test_tensor_mix_in_gpu.py hold the two together */
    if (IRREV) {
        float f[4] = { (float)v[0], (float)v[1], (float)v[2], (float)v[3] };
        if (F.mct) {                                     /* ICT: the constants and operand order of the vector factory */
            const float r = f[0], g = f[1], b = f[2];
            f[0] =  0.299f * r + 0.587f * g + 0.114f * b;
            f[1] = -0.168736f * r - 0.331264f * g + 0.5f * b;
            f[2] =  0.5f * r - 0.418688f * g - 0.081312f * b;
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (in[c])
                ((float *)A.dst[c])[(size_t)y * A.cw[c] + x] = f[c];
        return;
    }
    if (F.mct) {                                         /* RCT: Y = (R + 2G + B) >> 2, Cb = B - G, Cr = R - G */
        const int r = v[0], g = v[1], b = v[2];
        v[0] = (r + 2 * g + b) >> 2;
        v[1] = b - g;
        v[2] = r - g;
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
        if (in[c])
            A.dst[c][(size_t)y * A.cw[c] + x] = v[c];
}

/* k_enc_unpack_tensor_mix with transfer curves (htj2k_encode_tensor_curves).  The cut is the same, by chroma footprint:
 * a lane loads the K x N elements of a footprint once, curves each once (curve_in_gather), stores the N samples of every
 * full-resolution component and one sample of each chroma component; the samples are curve_in_sample's, which
 * htj2k_tensor_to_frames_curves writes frames by.  What differs is the grid: every workgroup first stages both tables
 * into LDS (32.8 KB at the most), so a workgroup is not 256 footprints of a row but walks the frame's footprints, in
 * raster order, in a grid-stride loop; the host gives a frame no more workgroups than leave each several times its
 * tables' bytes of tensor to read (round_unpack_tensor_curves, htj2k_encode.hip; curve_grid).  A table entry is a whole frame: A.y0 is 0,
 * A.h its footprint rows, A.w and A.ih the image's size; the footprint index is 64-bit where the frame needs it.
 * blockIdx.z is the frame, in chunks of what grid.z takes */
template <bool IRREV, int DT, int NHWC>
__global__ void __launch_bounds__(CURVE_IN_THREADS)
k_enc_unpack_tensor_curves(const UnpackTensorArgs *__restrict__ frames, UnpackTensorMixFmt F, htj2k_cmp::CurveInFmt Q)
{
    using htj2k_cmp::curve_in_lds;
    const UnpackTensorArgs &A = frames[blockIdx.z];
    const uint32_t fw = 1u << F.sw, fh = 1u << F.sh;
    const uint32_t fcols = ((uint32_t)A.w + fw - 1) >> F.sw;
    const uint64_t total = (uint64_t)fcols * (uint32_t)A.h;
    const uint32_t peak = (1u << F.bits) - 1, K = F.mix.nin;
    const int dc = 1 << (F.bits - 1);
    const bool box = F.mix.box != 0;
    htj2k_cmp::curve_in_stage(curve_in_lds, Q);

    for (uint64_t it = (uint64_t)blockIdx.x * CURVE_IN_THREADS + threadIdx.x; it < total; it += (uint64_t)gridDim.x * CURVE_IN_THREADS) {
        uint32_t x, y;
        if (total <= 0xFFFFFFFFull) { y = (uint32_t)it / fcols; x = (uint32_t)it - y * fcols; }
        else                        { y = (uint32_t)(it / fcols); x = (uint32_t)(it - (uint64_t)y * fcols); }
        const uint32_t X0 = x << F.sw, Y0 = y << F.sh;           /* inside the image: fcols and A.h are the ceilinged counts */
        const uint32_t nx = min(fw, (uint32_t)A.w - X0), ny = min(fh, (uint32_t)A.ih - Y0);
        const float rcp = htj2k_cmp::mix_in_rcp(F.rcp, nx, ny, fw, fh);
        float g[4];
        if (F.sw | F.sh) {
            /* sub-sampled: components 0 and 3 at every pixel as it is loaded and curved, 1 and 2 once from the gathered
             * footprint.  No component transform here, as in k_enc_unpack_tensor_mix */
            htj2k_cmp::curve_in_gather<DT, NHWC>(A.src, X0, Y0, nx, ny, box, rcp, K, (uint32_t)A.w, (uint32_t)A.ih, g, Q, curve_in_lds,
                [&](uint32_t fx, uint32_t fy, const float *f) {
                    const size_t at = ((size_t)Y0 + fy) * A.cw[0] + X0 + fx;
                    unpack_store<IRREV>(A.dst[0], at, (int)htj2k_cmp::curve_in_sample(f, K, F.mix.m[0], F.mix.b[0], (Q.out_mask & 1u) != 0, Q, curve_in_lds,
                                                                                     Q.gain[0], Q.offset[0], peak) - dc);
                    if (F.ncomp > 3)
                        unpack_store<IRREV>(A.dst[3], at, (int)htj2k_cmp::curve_in_sample(f, K, F.mix.m[3], F.mix.b[3], (Q.out_mask & 8u) != 0, Q, curve_in_lds,
                                                                                         Q.gain[3], Q.offset[3], peak) - dc);
                });
#pragma unroll
            for (int c = 1; c < 3; c++)
                unpack_store<IRREV>(A.dst[c], (size_t)y * A.cw[c] + x,
                                    (int)htj2k_cmp::curve_in_sample(g, K, F.mix.m[c], F.mix.b[c], ((Q.out_mask >> c) & 1u) != 0, Q, curve_in_lds,
                                                                    Q.gain[c], Q.offset[c], peak) - dc);
            continue;
        }
        htj2k_cmp::curve_in_gather<DT, NHWC>(A.src, X0, Y0, 1, 1, box, rcp, K, (uint32_t)A.w, (uint32_t)A.ih, g, Q, curve_in_lds,
                                             [](uint32_t, uint32_t, const float *) {});
        int v[4] = { 0, 0, 0, 0 };
        bool in[4] = { false, false, false, false };
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (c >= F.ncomp)
                continue;
            v[c] = (int)htj2k_cmp::curve_in_sample(g, K, F.mix.m[c], F.mix.b[c], ((Q.out_mask >> c) & 1u) != 0, Q, curve_in_lds,
                                                   Q.gain[c], Q.offset[c], peak) - dc;
            in[c] = true;
        }
        /* from here on k_enc_unpack, line for line: the equality tests of tests/test_curves_in_gpu.py hold the two together */
        if (IRREV) {
            float f[4] = { (float)v[0], (float)v[1], (float)v[2], (float)v[3] };
            if (F.mct) {                                 /* ICT: the constants and operand order of the vector factory */
                const float r = f[0], g = f[1], b = f[2];
                f[0] =  0.299f * r + 0.587f * g + 0.114f * b;
                f[1] = -0.168736f * r - 0.331264f * g + 0.5f * b;
                f[2] =  0.5f * r - 0.418688f * g - 0.081312f * b;
            }
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (in[c])
                    ((float *)A.dst[c])[(size_t)y * A.cw[c] + x] = f[c];
            continue;
        }
        if (F.mct) {                                     /* RCT: Y = (R + 2G + B) >> 2, Cb = B - G, Cr = R - G */
            const int r = v[0], g = v[1], b = v[2];
            v[0] = (r + 2 * g + b) >> 2;
            v[1] = b - g;
            v[2] = r - g;
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (in[c])
                A.dst[c][(size_t)y * A.cw[c] + x] = v[c];
    }
}

struct DwtPlane {                   /* one tile-component at one level */
    int32_t *p;                     /* its first sample in the component plane (row stride `stride`); its LL region is lw x lh */
    int32_t *t;                     /* the same place in the scratch plane */
    int32_t  stride, lw, lh;
    int32_t  px, py;                /* parity of the LL region's origin at this level: ceil(x0 / 2^l) & 1, ceil(y0 / 2^l) & 1 */
};

/* sample j of a line of n, counted from the line's first sample (symmetric extension about 0 and n - 1: reflection
 * keeps the parity of a position) */
__device__ __forceinline__ int fdwt_ref(int j, int n)
{
    j = j < 0 ? -j : j;
    return j >= n ? 2 * (n - 1) - j : j;
}

/* Where output i of a line of n samples whose first sample is at a position of parity `par` comes from: the nl samples
 * at even positions are low-pass and come first (nl = ceil(i1 / 2) - ceil(i0 / 2)), the ones at odd positions follow.
 * -> the sample's index in the line; *high: it is at an odd position */
__device__ __forceinline__ int fdwt_src(int n, int par, int i, bool *high)
{
    const int nl = (n + 1 - par) >> 1;
    *high = i >= nl;
    return *high ? 2 * (i - nl) + 1 - par : 2 * i + par;
}

/* output i of the forward 5/3 lifting of a line of n >= 2 samples, x(j) = line[j * step], the first at parity `par` */
__device__ __forceinline__ int32_t fdwt_out(const int32_t *line, size_t step, int n, int par, int i)
{
    bool high;
    const int j = fdwt_src(n, par, i, &high);
#define X(j) line[(size_t)fdwt_ref((j), n) * step]
#define D(j) (X(j) - ((X((j) - 1) + X((j) + 1)) >> 1))
    if (high)
        return D(j);
    const int dl = fdwt_ref(j - 1, n), dr = fdwt_ref(j + 1, n);  /* odd positions, reflected */
    return X(j) + ((D(dl) + D(dr) + 2) >> 2);
#undef D
#undef X
}

__global__ void __launch_bounds__(256)
k_fdwt_v(const DwtPlane *__restrict__ planes)
{
    const DwtPlane &P = planes[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= P.lw || y >= P.lh)
        return;
    const int32_t *col = P.p + x;                    /* one sample: as it is at an even position, doubled at an odd one */
    P.t[(size_t)y * P.stride + x] = P.lh == 1 ? col[0] * (1 + P.py) : fdwt_out(col, (size_t)P.stride, P.lh, P.py, y);
}

__global__ void __launch_bounds__(256)
k_fdwt_h(const DwtPlane *__restrict__ planes)
{
    const DwtPlane &P = planes[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= P.lw || y >= P.lh)
        return;
    const int32_t *row = P.t + (size_t)y * P.stride;
    P.p[(size_t)y * P.stride + x] = P.lw == 1 ? row[0] * (1 + P.px) : fdwt_out(row, 1, P.lw, P.px, x);
}

/* ------------------------------------------------------------------ forward 9/7 */
/* The lifting steps -alpha, -beta, gamma, delta and the 1-sample scale of the vector factory's fwd97_1d (un-normalised:
 * no K scaling for lines of two or more).  Symmetric extension maps every lifting step's input onto itself, so each
 * intermediate at a reflected position equals the one at the position it reflects: computing them per position with
 * reflected indices gives the extend-then-lift result bit for bit.  Each step rounds as x + c * (left + right); the
 * translation unit is built with -ffp-contract=off so that no multiply-add is fused. */
#define ENC_A97 1.586134342059924f
#define ENC_B97 0.052980118572961f
#define ENC_G97 0.882911075530934f
#define ENC_D97 0.443506852043971f
#define ENC_X97 0.812893066115961f
#define ENC_K97 1.230174104914001f

/* a line of one sample at a position of parity `par` */
__device__ __forceinline__ float fdwt97_one(float v, int par)
{
    return par ? v * (2.0f / ENC_K97) : v * (1.0f / ENC_X97);
}

/* output i of the forward 9/7 lifting of a line of n >= 2 floats, x(j) = line[j * step], the first at parity `par`:
 * low-pass outputs end in the delta step (even positions), high-pass ones in the gamma step (odd positions) */
__device__ __forceinline__ float fdwt97_out(const float *line, size_t step, int n, int par, int i)
{
    bool high;
    const int j = fdwt_src(n, par, i, &high);
#define X(j) line[(size_t)fdwt_ref((j), n) * step]
    /* step 1 (odd positions), step 2 (even ones), step 3 (odd ones), all at in-range j */
    auto s1 = [&](int j) { return X(j) + (-ENC_A97) * (X(j - 1) + X(j + 1)); };
    auto s2 = [&](int j) { return X(j) + (-ENC_B97) * (s1(fdwt_ref(j - 1, n)) + s1(fdwt_ref(j + 1, n))); };
    auto s3 = [&](int j) { return s1(j) + ENC_G97 * (s2(fdwt_ref(j - 1, n)) + s2(fdwt_ref(j + 1, n))); };
#undef X
    if (high)
        return s3(j);
    return s2(j) + ENC_D97 * (s3(fdwt_ref(j - 1, n)) + s3(fdwt_ref(j + 1, n)));
}

__global__ void __launch_bounds__(256)
k_fdwt97_v(const DwtPlane *__restrict__ planes)
{
    const DwtPlane &P = planes[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= P.lw || y >= P.lh)
        return;
    const float *col = (const float *)P.p + x;
    ((float *)P.t)[(size_t)y * P.stride + x] = P.lh == 1 ? fdwt97_one(col[0], P.py) : fdwt97_out(col, (size_t)P.stride, P.lh, P.py, y);
}

__global__ void __launch_bounds__(256)
k_fdwt97_h(const DwtPlane *__restrict__ planes)
{
    const DwtPlane &P = planes[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= P.lw || y >= P.lh)
        return;
    const float *row = (const float *)P.t + (size_t)y * P.stride;
    ((float *)P.p)[(size_t)y * P.stride + x] = P.lw == 1 ? fdwt97_one(row[0], P.px) : fdwt97_out(row, 1, P.lw, P.px, x);
}

/* ------------------------------------------------------------------ 9/7 quantiser */
struct QuantPlane {                 /* one tile-component of one frame, after the forward 9/7 */
    int32_t *p;                     /* its first sample in the component plane: floats in, int32 indices out (in place) */
    const float *step;              /* the decoder's step of each band: 0 LL, then HL LH HH from the lowest resolution */
    int32_t  stride, nl;
    int32_t  x0, y0, x1, y1;        /* the tile-component's rectangle (it decides where the bands lie) */
};

/* smallest level l in 1 .. nl whose high-pass part holds position x of the Mallat layout of a line i0 .. i1 - 1: x is
 * low-pass at level l exactly when x < ceil(i1 / 2^l) - ceil(i0 / 2^l); nl + 1: low-pass at every level */
__device__ __forceinline__ int quant_level(int x, int i0, int i1, int nl)
{
    int l = 1;
    while (l <= nl && x < (int)((((int64_t)i1 - 1) >> l) - (((int64_t)i0 - 1) >> l)))
        l++;
    return l;
}

__global__ void __launch_bounds__(256)
k_quant97(const QuantPlane *__restrict__ planes)
{
    const QuantPlane &Q = planes[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= Q.x1 - Q.x0 || y >= Q.y1 - Q.y0)
        return;
    /* the band of (x, y) in the Mallat layout: its level is the first at which x or y is high-pass */
    const int lx = quant_level(x, Q.x0, Q.x1, Q.nl), ly = quant_level(y, Q.y0, Q.y1, Q.nl), l = lx < ly ? lx : ly;
    const int g = l > Q.nl ? 0 : 3 * (Q.nl - l) + (lx == l ? 1 : 0) + (ly == l ? 2 : 0);
    int32_t *at = Q.p + (size_t)y * Q.stride + x;
    const float v = *(const float *)at;
    double m = floor(fabs((double)v) / (double)Q.step[g]);
    if (m > 2147483000.0)
        m = 2147483000.0;
    *at = v < 0 ? -(int32_t)m : (int32_t)m;
}

/* ------------------------------------------------------------------ HT cleanup encoder */
struct EncBlk {
    uint64_t coef;                  /* sample offset of the block's top-left in the coefficient buffer */
    uint64_t out;                   /* byte offset of its region in the pool (enc_block_bound bytes) */
    int32_t  stride;
    uint16_t w, h;
    int32_t  plane;                 /* the block is coded from sign(v) * (|v| >> plane); -1: left out (Lcup 0) */
    int32_t  npasses;               /* 0, 1: the cleanup pass alone.  2, 3: k_ht_refine_plan takes `plane` as the refinement
                                     * plane p and leaves the cleanup plane p + 1 there (or one pass at p: the fallback;
                                     * with ENC_BLK_KEEP or'ed in, one pass at p + 1) */
};
#define ENC_BLK_KEEP 0x100          /* EncBlk.npasses, transcoding: a block that falls back stays at its cleanup plane, for the
                                     * plane below holds bits its source never had */

struct EncRes {
    int32_t lcup;                   /* 0: all zero, left out; < 0: the block could not be coded */
    int32_t max_u;
    int32_t lref;                   /* bytes of the refinement segment behind Dcup (k_ht_refine_encode) */
    int32_t npasses;                /* the passes the block has (k_ht_refine_plan); both only where a call asks for passes */
};

/* LDS of one wave: exponents (4 bytes a quad), two words a quad, the MagSgn bit array, MEL + VLC, scratch */
#define ENC_MAX_QUADS  1024
#define ENC_MS_WORDS   (4096 + 8)
#define ENC_MV_BYTES   4096
#define ENC_LDS_BYTES  (4 * ENC_MAX_QUADS + 8 * ENC_MAX_QUADS + 4 * ENC_MS_WORDS + ENC_MV_BYTES + 4 * 8)

struct MelW { int n, rem, k, run; uint32_t tmp; };
struct VlcW { int n, used, gt8f; uint32_t tmp; };

__device__ __forceinline__ void mv_mel_bit(uint8_t *mv, MelW &m, int bit, bool &ovf, const VlcW &v)
{
    m.tmp = (m.tmp << 1) | (uint32_t)(bit & 1);
    if (--m.rem == 0) {
        if (m.n + v.n < ENC_MV_BYTES) mv[m.n] = (uint8_t)m.tmp; else ovf = true;
        m.n++;
        m.rem = (m.tmp & 0xFF) == 0xFF ? 7 : 8;
        m.tmp = 0;
    }
}

__device__ __forceinline__ void mv_mel_sym(uint8_t *mv, MelW &m, int sym, bool &ovf, const VlcW &v)
{
    const int E = m.k < 3 ? 0 : m.k < 6 ? 1 : m.k < 9 ? 2 : m.k < 11 ? 3 : m.k < 12 ? 4 : 5;   /* MEL_E, T.814 Table 2 */
    if (!sym) {
        if (++m.run >= (1 << E)) {
            mv_mel_bit(mv, m, 1, ovf, v);
            m.run = 0;
            m.k = min(12, m.k + 1);
        }
    } else {
        mv_mel_bit(mv, m, 0, ovf, v);
        for (int i = E - 1; i >= 0; i--)
            mv_mel_bit(mv, m, (m.run >> i) & 1, ovf, v);
        m.run = 0;
        m.k = max(0, m.k - 1);
    }
}

/* VLC bytes grow downwards from the end of the MEL/VLC buffer: byte k at mv[ENC_MV_BYTES - 1 - k] */
__device__ __forceinline__ void mv_vlc_byte(uint8_t *mv, VlcW &v, const MelW &m, uint32_t b, bool &ovf)
{
    if (m.n + v.n < ENC_MV_BYTES) mv[ENC_MV_BYTES - 1 - v.n] = (uint8_t)b; else ovf = true;
    v.n++;
}

__device__ __forceinline__ void mv_vlc_put(uint8_t *mv, VlcW &v, const MelW &m, uint32_t cwd, int len, bool &ovf)
{
    while (len > 0) {
        int avail = 8 - v.gt8f - v.used;
        const int t = min(avail, len);
        v.tmp |= (cwd & ((1u << t) - 1)) << v.used;
        v.used += t; avail -= t; len -= t; cwd >>= t;
        if (avail == 0) {
            if (v.gt8f && v.tmp != 0x7F) {              /* the 7 LSBs are not all ones: the 8th bit is usable */
                v.gt8f = 0;
                continue;
            }
            mv_vlc_byte(mv, v, m, v.tmp, ovf);
            v.gt8f = v.tmp > 0x8F;
            v.tmp = 0; v.used = 0;
        }
    }
}

/* ------------------------------------------------------------------ the quad rules
 * What a quad's codewords are, stated once on register values: k_ht_encode writes the bits these functions name,
 * k_rc_stats counts them.  The budget holds cheaply only while the two agree bit for bit. */

/* a sample coded from bit-plane sh: mag = |v| >> sh and, where mag > 0, vv = 2 (mag - 1) + sign (MagSgn carries it) */
struct MagV { uint32_t mag, vv; };
__device__ __forceinline__ MagV mag_at(int32_t v, int sh)
{
    const uint32_t mag = (v < 0 ? 0u - (uint32_t)v : (uint32_t)v) >> sh;
    return { mag, 2 * (mag - 1) + (v < 0) };
}

/* the exponent of a sample of magnitude mag: the bits of vv, whatever the sign; 0: not significant */
__device__ __forceinline__ uint32_t enc_expn(uint32_t mag)
{
    return mag ? 32u - (uint32_t)__clz((int)(((mag - 1) << 1) | 1u)) : 0u;
}

/* The code of one quad from exponents, a byte per sample (e4: its own; left, nw, n, ne: its neighbours', 0 where
 * there is none): significance pattern rho, context, U, u = U - kappa, the pattern eps of the samples at U, and the
 * CxtVLC table entry t (vlc: the quad has a codeword at all). */
struct QuadCode { int rho, ctx, U, u, eps; uint32_t t; bool vlc; };
__device__ __forceinline__ QuadCode quad_code(uint32_t e4, uint32_t left, uint32_t nw, uint32_t n, uint32_t ne, bool first_row,
                                              const uint16_t *__restrict__ tab)
{
    QuadCode c = { 0, 0, 0, 0, 0, 0, false };
    int emax = 0, kappa = 1;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int e = (e4 >> (8 * i)) & 0xFF;
        c.rho |= (e != 0) << i;
        emax = max(emax, e);
    }
    if (first_row) {
        c.ctx = ((left & 0xFFFF) != 0) + (((left & 0xFF0000) != 0) << 1) + (((left >> 24) != 0) << 2);
    } else {
        const int En = (n >> 8) & 0xFF, Ene = n >> 24, Enw = nw >> 24, Enf = (ne >> 8) & 0xFF;
        const int gamma = __popc(c.rho) > 1;
        c.ctx = ((En | Enw) != 0) + (((left >> 16) != 0) << 1) + (((Ene | Enf) != 0) << 2);
        kappa = max(1, gamma * (max(max(En, Ene), max(Enw, Enf)) - 1));
    }
    c.U = max(emax, kappa);
    c.u = c.U - kappa;
    if (c.u > 0)
#pragma unroll
        for (int i = 0; i < 4; i++)
            c.eps |= ((int)((e4 >> (8 * i)) & 0xFF) == c.U) << i;
    c.vlc = c.ctx != 0 || c.rho != 0;
    if (c.vlc)
        c.t = tab[(((first_row ? 0 : 1) * 8 + c.ctx) * 16 + c.rho) * 16 + c.eps];
    return c;
}

/* U-VLC (T.814 7.3.6) of u: prefix, suffix, extension; nothing for u = 0.  Selects, no branches: k_rc_stats asks
 * every lane for the lengths. */
struct UVlc { uint32_t pfx, sfx, ext; int pl, sl, el, pv; };
__device__ __forceinline__ UVlc uvlc_split(int u)
{
    UVlc r;
    r.pv  = u <= 0 ? 0 : u <= 2 ? u : u <= 4 ? 3 : 5;
    r.pfx = u <= 0 ? 0u : u <= 2 ? (uint32_t)u : u <= 4 ? 4u : 0u;
    r.pl  = u <= 0 ? 0 : u <= 2 ? u : 3;
    r.sfx = u <= 2 ? 0u : u <= 4 ? (uint32_t)(u - 3) : u <= 32 ? (uint32_t)(u - 5) : 28 + (uint32_t)((u - 33) & 3);
    r.sl  = u <= 2 ? 0 : u <= 4 ? 1 : 5;
    r.ext = u <= 32 ? 0u : (uint32_t)((u - 33) >> 2);
    r.el  = u <= 32 ? 0 : 4;
    return r;
}

__device__ __forceinline__ int uvlc_len(int u)
{
    const UVlc s = uvlc_split(u);
    return s.pl + s.sl + s.el;
}

/* How the u of two quads side by side are coded (u = 0: that quad has none, or is not there).  v[k] is what quad k's
 * U-VLC codes; mel is the MEL symbol in front of them (-1: none); one_bit: quad 1's v - 1 goes as one bit where its
 * prefix would, and nothing else of it.  The fields go out prefixes, suffixes, extensions, quad 0 first in each. */
struct UPair { int v[2], mel; bool one_bit; };
__device__ __forceinline__ UPair uvlc_pair(int u0, int u1, bool first_row)
{
    const bool rule = first_row && u0 > 0 && u1 > 0;    /* else both are coded plainly */
    const bool both = rule && u0 > 2 && u1 > 2;
    return { { both ? u0 - 2 : u0, both ? u1 - 2 : u1 }, rule ? (int)both : -1, rule && !both && uvlc_split(u0).pv > 2 };
}

/* bits [pos, pos + n) of the LDS bit array, n <= 8 */
__device__ __forceinline__ uint32_t ms_bits(const uint32_t *ms, uint32_t pos, int n)
{
    const uint64_t w = (uint64_t)ms[pos >> 5] | ((uint64_t)ms[(pos >> 5) + 1] << 32);
    return (uint32_t)(w >> (pos & 31)) & ((1u << n) - 1);
}

/* The byte-after-0xFF rule (T.814 7.1.2 backwards) over the `total` bits of the LDS bit array MS, into `out`: after an
 * 0xFF byte the next one carries 7 bits.  The wave cuts the unstuffed bits into bytes 64 at a time, lane k one byte:
 * byte 0 of a window takes `mb` bits (7 right behind an 0xFF), the others 8.  All bytes up to the first full 0xFF are
 * final; the next window starts behind it with mb = 7.  A window so advances 64 bytes, or to the next 0xFF.
 * PAD_ONES (MagSgn): a partial last byte is padded with 1s, and dropped if that makes it 0xFF; else (SigProp) it is
 * padded with 0s and stays.  -> the bytes written */
template <bool PAD_ONES>
__device__ __forceinline__ uint32_t ms_stuff(const uint32_t *MS, uint32_t total, uint8_t *out, int lane)
{
    uint32_t o = 0, p = 0;
    int mb = 8;
    for (;;) {
        const uint32_t start = lane ? p + (uint32_t)mb + 8u * (uint32_t)(lane - 1) : p;
        const int nb = lane ? 8 : mb;
        const bool full = start + (uint32_t)nb <= total;
        const uint32_t byte = full ? ms_bits(MS, start, nb) : 0;
        const uint64_t ff = __ballot(full && byte == 0xFF);
        const uint64_t fl = __ballot(full);
        if (ff) {
            const int f = __ffsll((unsigned long long)ff) - 1;
            if (lane <= f)
                out[o + lane] = (uint8_t)byte;
            o += (uint32_t)f + 1;
            p = (f ? p + (uint32_t)mb + 8u * (uint32_t)(f - 1) : p) + (f ? 8u : (uint32_t)mb);
            mb = 7;
            continue;
        }
        const int nfull = fl == ~0ull ? 64 : __ffsll((unsigned long long)~fl) - 1;   /* full bytes lead the window */
        if (lane < nfull)
            out[o + lane] = (uint8_t)byte;
        if (nfull == 64) {
            o += 64;
            p += (uint32_t)mb + 8u * 63u;
            mb = 8;
            continue;
        }
        /* the window reached the end: a partial byte */
        const uint32_t tstart = nfull ? p + (uint32_t)mb + 8u * (uint32_t)(nfull - 1) : p;
        const int tbits = nfull ? 8 : mb;
        o += (uint32_t)nfull;
        if (tstart < total) {
            const int rem = (int)(total - tstart);
            const uint32_t t = ms_bits(MS, tstart, rem) | (PAD_ONES ? (0xFFu << rem) & ((1u << tbits) - 1) : 0u);
            if (!PAD_ONES || t != 0xFF) {
                if (lane == 0)
                    out[o] = (uint8_t)t;
                o++;
            }
        }
        break;
    }
    return o;
}

/* quad word 0: cwd | len << 8 | ek << 12 | rho << 16 | mel << 20 | vlc << 21 | uoff << 22 | bad << 23
 *      word 1: U | u << 8 */
#define ENC_STAMPS 6                /* phase boundaries a block's wave records when `stamps` is given (clock64) */

__global__ void __launch_bounds__(64)
k_ht_encode(const EncBlk *__restrict__ blks, const int32_t *__restrict__ coef, uint8_t *__restrict__ pool,
            EncRes *__restrict__ res, const uint16_t *__restrict__ tab, uint64_t *__restrict__ stamps)
{
    uint64_t st[ENC_STAMPS];
    if (stamps)
        st[0] = clock64();
    extern __shared__ uint32_t lds[];
    uint32_t *E4 = lds;                                  /* per quad: E of its 4 samples, a byte each (0 = not significant) */
    uint32_t *Q = E4 + ENC_MAX_QUADS;                    /* 2 words per quad */
    uint32_t *MS = Q + 2 * ENC_MAX_QUADS;                /* MagSgn bits, LSB first */
    uint8_t *MV = (uint8_t *)(MS + ENC_MS_WORDS);        /* MEL forwards, VLC backwards */
    int32_t *SC = (int32_t *)(MV + ENC_MV_BYTES);        /* results of lane 0 */
    const int lane = threadIdx.x;
    const EncBlk B = blks[blockIdx.x];
    const int w = B.w, h = B.h, qw = (w + 1) >> 1, qh = (h + 1) >> 1, nq = qw * qh;
    const int32_t *src = coef + B.coef;
    uint8_t *out = pool + B.out;
    const int sh = B.plane;                              /* bit-planes dropped (rate control); 0 otherwise */
    if (sh < 0) {                                        /* left out by the allocation */
        if (lane == 0) { res[blockIdx.x].lcup = 0; res[blockIdx.x].max_u = 0; }
        return;
    }

    /* 1. exponents */
    int any = 0;
    for (int q = lane; q < nq; q += 64) {
        const int qy = q / qw, qx = q - qy * qw;
        uint32_t e4 = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int y = 2 * qy + (i & 1), x = 2 * qx + (i >> 1);
            if (y < h && x < w)
                e4 |= enc_expn(mag_at(src[(size_t)y * B.stride + x], sh).mag) << (8 * i);
        }
        E4[q] = e4;
        any |= e4 != 0;
    }
    if (!__any(any)) {
        if (lane == 0) { res[blockIdx.x].lcup = 0; res[blockIdx.x].max_u = 0; }
        return;
    }
    __syncthreads();

    /* 2. contexts, exponent bounds, codewords */
    int maxU = 0, bad = 0;
    for (int q = lane; q < nq; q += 64) {
        const int qy = q / qw, qx = q - qy * qw;
        const bool first = qx == 0, last = qx == qw - 1;
        const uint32_t left = first ? 0 : E4[q - 1];
        uint32_t nw = 0, n = 0, ne = 0;
        if (qy) {
            const int qa = q - qw;
            n = E4[qa];
            nw = first ? 0 : E4[qa - 1];
            ne = last ? 0 : E4[qa + 1];
        }
        const QuadCode C = quad_code(E4[q], left, nw, n, ne, qy == 0, tab);
        if (C.vlc && !(C.t >> 15))
            bad = 1;
        const uint32_t cw = C.vlc ? (C.t & 0xFF) | ((C.t >> 8) & 7) << 8 | ((C.t >> 11) & 15) << 12 : 0;
        Q[2 * q] = cw | (uint32_t)C.rho << 16 | (uint32_t)(C.ctx == 0) << 20 | (uint32_t)C.vlc << 21 | (uint32_t)(C.u > 0) << 22;
        Q[2 * q + 1] = (uint32_t)C.U | (uint32_t)C.u << 8;
        maxU = max(maxU, C.U);
    }
    /* wave reductions */
    for (int off = 32; off > 0; off >>= 1) {
        maxU = max(maxU, __shfl_xor(maxU, off, 64));
        bad |= __shfl_xor(bad, off, 64);
    }
    __syncthreads();                                     /* stage 3 reads quads other lanes wrote */
    if (stamps)
        st[1] = clock64();

    /* 3. MagSgn: m = sigma * U - e_k bits per sample, in quad order, sample order 0..3 */
    const int chunk = (nq + 63) >> 6, q0 = min(nq, lane * chunk), q1 = min(nq, q0 + chunk);
    uint32_t mine = 0;
    for (int q = q0; q < q1; q++) {
        const uint32_t e4 = E4[q], U = Q[2 * q + 1] & 0xFF, ek = (Q[2 * q] >> 12) & 15;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if ((e4 >> (8 * i)) & 0xFF)
                mine += U - ((ek >> i) & 1);
    }
    uint32_t incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off)
            incl += t;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    const uint32_t nwords = (total >> 5) + 2;
    for (uint32_t i = lane; i < nwords; i += 64)
        MS[i] = 0;
    __syncthreads();
    uint32_t pos = incl - mine;
    for (int q = q0; q < q1; q++) {
        const uint32_t e4 = E4[q], U = Q[2 * q + 1] & 0xFF, ek = (Q[2 * q] >> 12) & 15;
        const int qy = q / qw, qx = q - qy * qw;
        for (int i = 0; i < 4; i++) {
            if (!((e4 >> (8 * i)) & 0xFF))
                continue;
            const int m = (int)U - (int)((ek >> i) & 1);
            if (m <= 0)
                continue;
            const int y = 2 * qy + (i & 1), x = 2 * qx + (i >> 1);
            const uint32_t vv = mag_at(src[(size_t)y * B.stride + x], sh).vv & (m >= 32 ? 0xFFFFFFFFu : ((1u << m) - 1));
            const uint64_t s = (uint64_t)vv << (pos & 31);
            atomicOr(&MS[pos >> 5], (uint32_t)s);
            if (s >> 32)
                atomicOr(&MS[(pos >> 5) + 1], (uint32_t)(s >> 32));
            pos += (uint32_t)m;
        }
    }
    __syncthreads();

    if (stamps)
        st[2] = clock64();

    /* 4. the byte-after-0xFF rule */
    const uint32_t o = ms_stuff<true>(MS, total, out, lane);
    if (stamps)
        st[3] = clock64();

    if (lane == 0) {
        /* 5. MEL and VLC in quad-pair order */
        MelW m = { 0, 8, 0, 0, 0 };
        VlcW v = { 0, 4, 1, 0xF };
        bool ovf = false;
        mv_vlc_byte(MV, v, m, 0xFF, ovf);               /* Scup placeholder */
        for (int qy = 0; qy < qh; qy++)
            for (int qx = 0; qx < qw; qx += 2) {
                const int npair = qx + 1 < qw ? 2 : 1;
                int u[2] = { 0, 0 };
                for (int k = 0; k < npair; k++) {
                    const int q = qy * qw + qx + k;
                    const uint32_t a = Q[2 * q];
                    u[k] = (int)(Q[2 * q + 1] >> 8);
                    if ((a >> 20) & 1)
                        mv_mel_sym(MV, m, ((a >> 16) & 15) != 0, ovf, v);
                    if ((a >> 21) & 1)
                        mv_vlc_put(MV, v, m, a & 0xFF, (int)((a >> 8) & 7), ovf);
                }
                if (!(u[0] | u[1]))
                    continue;
                const UPair P = uvlc_pair(u[0], u[1], qy == 0);
                const UVlc A = uvlc_split(P.v[0]);
                UVlc Bv = uvlc_split(P.v[1]);
                if (P.one_bit)
                    Bv = { (uint32_t)(P.v[1] - 1), 0, 0, 1, 0, 0, 0 };
                if (P.mel >= 0)
                    mv_mel_sym(MV, m, P.mel, ovf, v);
                mv_vlc_put(MV, v, m, A.pfx, A.pl, ovf); mv_vlc_put(MV, v, m, Bv.pfx, Bv.pl, ovf);
                mv_vlc_put(MV, v, m, A.sfx, A.sl, ovf); mv_vlc_put(MV, v, m, Bv.sfx, Bv.sl, ovf);
                mv_vlc_put(MV, v, m, A.ext, A.el, ovf); mv_vlc_put(MV, v, m, Bv.ext, Bv.el, ovf);
            }
        /* MEL: an open run completes; a partial byte is flushed */
        if (m.run > 0)
            mv_mel_bit(MV, m, 1, ovf, v);
        {
            const int full = (m.n && m.n <= ENC_MV_BYTES && MV[m.n - 1] == 0xFF) ? 7 : 8;
            if (m.rem != full) {
                if (m.n + v.n < ENC_MV_BYTES) MV[m.n] = (uint8_t)(m.tmp << m.rem); else ovf = true;
                m.n++;
            }
        }
        if (v.used)
            mv_vlc_byte(MV, v, m, v.tmp, ovf);
        if (v.n < 2)
            mv_vlc_byte(MV, v, m, 0x0F, ovf);
        const int scup = m.n + v.n;
        if (ovf || scup > 4079 || bad) {
            SC[0] = -1;
        } else {
            MV[ENC_MV_BYTES - 1] = (uint8_t)(scup >> 4);
            MV[ENC_MV_BYTES - 2] = (uint8_t)((MV[ENC_MV_BYTES - 2] & 0xF0) | (scup & 0xF));
            SC[0] = (int)o;
            SC[1] = m.n;
            SC[2] = v.n;
        }
    }
    __syncthreads();
    if (stamps)
        st[4] = clock64();
    const int ms_len = SC[0];
    if (ms_len < 0) {
        if (lane == 0) { res[blockIdx.x].lcup = -1; res[blockIdx.x].max_u = maxU; }
        return;
    }
    const int mel_n = SC[1], vlc_n = SC[2];
    for (int j = lane; j < mel_n; j += 64)
        out[ms_len + j] = MV[j];
    for (int j = lane; j < vlc_n; j += 64)
        out[ms_len + mel_n + j] = MV[ENC_MV_BYTES - vlc_n + j];
    if (lane == 0) {
        res[blockIdx.x].lcup = ms_len + mel_n + vlc_n;
        res[blockIdx.x].max_u = maxU;
        if (stamps) {
            st[5] = clock64();
            for (int k = 0; k < ENC_STAMPS; k++)
                stamps[(size_t)blockIdx.x * ENC_STAMPS + k] = st[k];
        }
    }
}

/* ------------------------------------------------------------------ HT refinement passes
 * A block of 2 or 3 passes is the cleanup pass at plane p + 1 and, at plane p, SigProp (pass 2) and MagRef (pass 3) in
 * one segment Dref behind Dcup (T.814 7.4, 7.5 read backwards; byte for byte the vector factory's ht_refine_encode).
 * With m = |v| >> p and sigma = (m >> 1) != 0, a sample's byte in the LDS map ST (a border of zeros around the block): */
#define REF_SIGMA  1                /* significant after the cleanup pass */
#define REF_ONE    2                /* sigma = 0 and m == 1: the bit SigProp would write is 1 */
#define REF_MEMBER 4                /* SigProp visits it */
#define REF_SIGN   8
#define REF_MRBIT  16               /* m & 1: what MagRef writes */
#define REF_NEWSIG 32               /* REF_MEMBER and REF_ONE: significant from its visit on */
#define REF_ST_BYTES 6160           /* (w + 2) * (h + 2) <= 1026 * 6 for every block the table accepts */
#define REF_SP_WORDS 264            /* SigProp: 2 bits a sample at most */
#define REF_MR_WORDS 136            /* MagRef: 1 */
#define REF_MR_BYTES 640            /* 4096 bits, 7 to a byte at worst */
#define REF_STAMPS   7              /* phase boundaries k_ht_refine_encode records when `stamps` is given (clock64) */

/* k_ht_refine_plan: before k_ht_encode, the blocks of a call that asks for passes.  An entry of 2 or 3 passes comes
 * with its refinement plane p; it leaves as cleanup plane p + 1, or, where nothing is significant at p + 1 or Dref
 * would be empty (two passes and every sample significant: SigProp visits none), as one pass at p (at p + 1 for an entry
 * with ENC_BLK_KEEP).  Dref is not empty
 * otherwise: a block with significant and insignificant samples has a member, and MagRef writes every significant one. */
__global__ void __launch_bounds__(64)
k_ht_refine_plan(EncBlk *__restrict__ blks, const int32_t *__restrict__ coef, EncRes *__restrict__ res)
{
    const int lane = threadIdx.x;
    const EncBlk B = blks[blockIdx.x];
    const int w = B.w, h = B.h, n = w * h;
    const bool keep = (B.npasses & ENC_BLK_KEEP) != 0;
    int np = (B.npasses & 0xFF) < 2 || B.plane < 0 ? 1 : B.npasses & 0xFF;
    bool fell = false;
    if (np > 1) {
        const int32_t *src = coef + B.coef;
        int nsig = 0;
        for (int i = lane; i < n; i += 64) {
            const int y = i / w, x = i - y * w;
            nsig += (mag_at(src[(size_t)y * B.stride + x], B.plane).mag >> 1) != 0;
        }
        for (int off = 32; off > 0; off >>= 1)
            nsig += __shfl_xor(nsig, off, 64);
        if (nsig == 0 || (np == 2 && nsig == n)) {
            np = 1;
            fell = true;
        }
    }
    if (lane == 0) {
        if (np > 1 || (fell && keep))
            blks[blockIdx.x].plane = B.plane + 1;
        blks[blockIdx.x].npasses = np;
        res[blockIdx.x].lref = 0;
        res[blockIdx.x].npasses = np;
    }
}

/* the bits one 4 x 4 group (gw x gh at its corner c of ST, row stride bs) gives SigProp: a bit per member, column by
 * column, then the signs of its newly significant members in that order -> the bits, *len of them (at most 32) */
__device__ __forceinline__ uint32_t ref_sp_group(const uint8_t *c, int bs, int gw, int gh, int *len)
{
    uint32_t bits = 0, sg = 0;
    int nb = 0, ns = 0;
    for (int dx = 0; dx < gw; dx++)
        for (int dy = 0; dy < gh; dy++) {
            const uint32_t me = c[dy * bs + dx];
            if (!(me & REF_MEMBER))
                continue;
            bits |= ((me >> 1) & 1) << nb++;
            if (me & REF_ONE)
                sg |= ((me >> 3) & 1) << ns++;
        }
    *len = nb + ns;
    return nb < 32 ? bits | sg << nb : bits;            /* nb = 32 cannot be: 16 samples */
}

/* and MagRef: a bit per significant sample, column by column (at most 16) */
__device__ __forceinline__ uint32_t ref_mr_group(const uint8_t *c, int bs, int gw, int gh, int *len)
{
    uint32_t bits = 0;
    int nb = 0;
    for (int dx = 0; dx < gw; dx++)
        for (int dy = 0; dy < gh; dy++) {
            const uint32_t me = c[dy * bs + dx];
            if (me & REF_SIGMA)
                bits |= ((me >> 4) & 1) << nb++;
        }
    *len = nb;
    return bits;
}

__device__ __forceinline__ uint32_t ref_wave_scan(uint32_t mine, int lane, uint32_t *total)
{
    uint32_t incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off)
            incl += t;
    }
    *total = __shfl(incl, 63, 64);
    return incl - mine;
}

__device__ __forceinline__ void ref_or_bits(uint32_t *A, uint32_t pos, uint32_t bits)
{
    const uint64_t s = (uint64_t)bits << (pos & 31);
    if ((uint32_t)s)
        atomicOr(&A[pos >> 5], (uint32_t)s);
    if (s >> 32)
        atomicOr(&A[(pos >> 5) + 1], (uint32_t)(s >> 32));
}

/* stage 1 of the refinement kernels: the map of a w x h block at refinement plane p, border included; ends in a barrier */
__device__ __forceinline__ void ref_map(uint8_t *ST, const int32_t *src, int stride, int w, int h, int p, int lane)
{
    const int bs = w + 2, n = w * h, nst = (bs * (h + 2) + 3) >> 2;
    for (int i = lane; i < nst; i += 64)
        ((uint32_t *)ST)[i] = 0;
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const int y = i / w, x = i - y * w;
        const int32_t v = src[(size_t)y * stride + x];
        const uint32_t m = mag_at(v, p).mag;
        ST[(y + 1) * bs + x + 1] = (uint8_t)((m >> 1 ? REF_SIGMA : 0) | (m == 1 ? REF_ONE : 0) | (v < 0 ? REF_SIGN : 0) |
                                             (m & 1 ? REF_MRBIT : 0));
    }
    __syncthreads();
}

/* stage 2: membership to the fixed point; the lane sweeps its groups g0 .. g1 - 1 in scan order; ends in a barrier */
__device__ __forceinline__ void ref_members(uint8_t *ST, int w, int h, int g0, int g1)
{
    const int bs = w + 2, gwn = (w + 3) >> 2;
    for (;;) {
        int changed = 0;
        for (int g = g0; g < g1; g++) {
            const int s = g / gwn, x0 = 4 * (g - s * gwn), y0 = 4 * s, gw = min(4, w - x0), gh = min(4, h - y0);
            for (int dx = 0; dx < gw; dx++)
                for (int dy = 0; dy < gh; dy++) {
                    uint8_t *c = ST + (y0 + dy + 1) * bs + x0 + dx + 1;
                    const uint32_t me = c[0];
                    if (me & (REF_SIGMA | REF_MEMBER))
                        continue;
                    const uint32_t a = c[-bs - 1], b = c[-bs], d = c[-bs + 1], l = c[-1], r = c[1], e = c[bs - 1], f = c[bs],
                                   k = c[bs + 1];
                    /* earlier in scan order: the row above, the column to the left inside the stripe, and up right
                     * where that is the stripe above */
                    const uint32_t early = a | b | l | (dy == 0 ? d : 0u) | (dy < gh - 1 ? e : 0u);
                    if (((a | b | d | l | r | e | f | k) & REF_SIGMA) | (early & REF_NEWSIG)) {
                        c[0] = (uint8_t)(me | REF_MEMBER | ((me & REF_ONE) << 4));
                        changed = 1;
                    }
                }
        }
        __syncthreads();
        if (!__any(changed))
            break;
    }
}

/* k_ht_refine_encode: a wave per block, after k_ht_encode has coded the block from plane p + 1; blocks of one pass
 * leave at once.  Scan order (T.814 7.4) is stripes of 4 rows and, in a stripe, column by column: the 4 x 4 groups in
 * raster order, columns first inside one.  Every lane owns a run of consecutive groups.
 *   1. the map ST
 *   2. membership.  A sample with sigma = 0 is a member when a neighbour has sigma = 1 or is a newly significant member
 *      earlier in scan order.  The wave sweeps to the fixed point: a lane walks its groups in scan order, so a chain
 *      runs through a lane's run in one sweep and crosses at least one run per sweep (at most 65 sweeps; a typical
 *      block takes two).  Flags are only ever set, and a sample's flag is set by its own lane alone.
 *   3. SigProp bits at positions from a wave prefix sum over the groups' lengths, into an LDS bit array
 *   4. the byte-after-0xFF rule (ms_stuff, as MagSgn; zero padding)
 *   5. three passes: MagRef bits likewise, then lane 0 cuts them into bytes by the VLC writer's rule (after a byte above
 *      0x8F the next one takes 7 bits, or 8 when those 7 are not all ones; the byte behind the segment counts as 0xFF);
 *      the bytes go out backwards from the segment's end
 * `stamps` (measurements only): the clock at the boundaries of map, membership, SigProp bits, ms_stuff, MagRef bits and
 * MagRef bytes, for every block that has a Dref */
__global__ void __launch_bounds__(64)
k_ht_refine_encode(const EncBlk *__restrict__ blks, const int32_t *__restrict__ coef, uint8_t *__restrict__ pool,
                   EncRes *__restrict__ res, uint64_t *__restrict__ stamps)
{
    uint64_t st[REF_STAMPS];
    __shared__ __attribute__((aligned(16))) uint8_t ST[REF_ST_BYTES];
    __shared__ uint32_t SP[REF_SP_WORDS], MR[REF_MR_WORDS];
    __shared__ uint8_t RB[REF_MR_BYTES];
    const int lane = threadIdx.x;
    const EncBlk B = blks[blockIdx.x];
    const int lcup = res[blockIdx.x].lcup;
    if (B.npasses < 2 || B.plane < 1 || lcup <= 0)
        return;
    const int w = B.w, h = B.h, bs = w + 2, p = B.plane - 1;
    const int32_t *src = coef + B.coef;
    uint8_t *out = pool + B.out + lcup;
    if (stamps)
        st[0] = clock64();

    /* 1. the map, 2. membership */
    for (int i = lane; i < REF_SP_WORDS; i += 64)
        SP[i] = 0;
    for (int i = lane; i < REF_MR_WORDS; i += 64)
        MR[i] = 0;
    ref_map(ST, src, B.stride, w, h, p, lane);
    if (stamps)
        st[1] = clock64();
    const int gwn = (w + 3) >> 2, ng = gwn * ((h + 3) >> 2);
    const int chunk = (ng + 63) >> 6, g0 = min(ng, lane * chunk), g1 = min(ng, g0 + chunk);
    ref_members(ST, w, h, g0, g1);
    if (stamps)
        st[2] = clock64();

    /* 3. SigProp bits */
    uint32_t mine = 0, total;
    for (int g = g0; g < g1; g++) {
        const int s = g / gwn, x0 = 4 * (g - s * gwn), y0 = 4 * s;
        int len;
        ref_sp_group(ST + (y0 + 1) * bs + x0 + 1, bs, min(4, w - x0), min(4, h - y0), &len);
        mine += (uint32_t)len;
    }
    uint32_t pos = ref_wave_scan(mine, lane, &total);
    for (int g = g0; g < g1; g++) {
        const int s = g / gwn, x0 = 4 * (g - s * gwn), y0 = 4 * s;
        int len;
        const uint32_t bits = ref_sp_group(ST + (y0 + 1) * bs + x0 + 1, bs, min(4, w - x0), min(4, h - y0), &len);
        ref_or_bits(SP, pos, bits);
        pos += (uint32_t)len;
    }
    __syncthreads();
    if (stamps)
        st[3] = clock64();

    /* 4. the byte-after-0xFF rule */
    const uint32_t nsp = ms_stuff<false>(SP, total, out, lane);
    if (stamps)
        st[4] = st[5] = clock64();

    /* 5. MagRef */
    int nmr = 0;
    if (B.npasses > 2) {
        uint32_t mtotal;
        mine = 0;
        for (int g = g0; g < g1; g++) {
            const int s = g / gwn, x0 = 4 * (g - s * gwn), y0 = 4 * s;
            int len;
            ref_mr_group(ST + (y0 + 1) * bs + x0 + 1, bs, min(4, w - x0), min(4, h - y0), &len);
            mine += (uint32_t)len;
        }
        pos = ref_wave_scan(mine, lane, &mtotal);
        for (int g = g0; g < g1; g++) {
            const int s = g / gwn, x0 = 4 * (g - s * gwn), y0 = 4 * s;
            int len;
            const uint32_t bits = ref_mr_group(ST + (y0 + 1) * bs + x0 + 1, bs, min(4, w - x0), min(4, h - y0), &len);
            ref_or_bits(MR, pos, bits);
            pos += (uint32_t)len;
        }
        __syncthreads();
        if (stamps)
            st[5] = clock64();
        if (lane == 0) {
            uint32_t at = 0;
            bool gt8f = true;
            while (at < mtotal && nmr < REF_MR_BYTES) {
                const int left = (int)min(mtotal - at, 8u);
                int take = gt8f ? 7 : 8;
                if (left < take) {                      /* the last, partial byte */
                    RB[nmr++] = (uint8_t)ms_bits(MR, at, left);
                    break;
                }
                if (gt8f && left > 7 && ms_bits(MR, at, 7) != 0x7F)
                    take = 8;                           /* the 7 LSBs are not all ones: the 8th bit is usable */
                const uint32_t byte = ms_bits(MR, at, take);
                RB[nmr++] = (uint8_t)byte;
                at += (uint32_t)take;
                gt8f = byte > 0x8F;
            }
        }
        nmr = __shfl(nmr, 0, 64);
        __syncthreads();
        for (int j = lane; j < nmr; j += 64)
            out[nsp + (uint32_t)(nmr - 1 - j)] = RB[j];
    }
    if (lane == 0) {
        res[blockIdx.x].lref = (int)nsp + nmr;
        if (stamps) {
            st[6] = clock64();
            for (int k = 0; k < REF_STAMPS; k++)
                stamps[(size_t)blockIdx.x * REF_STAMPS + k] = st[k];
        }
    }
}

/* ------------------------------------------------------------------ rate control
 * k_rc_stats: one wave per block.  The magnitudes go to LDS once, in quad order (16 KB); then, for every bit-plane p
 * below the block's highest, lanes walk the quad pairs and ask the quad rules (enc_expn, quad_code, uvlc_pair: the
 * functions k_ht_encode codes by) for the code of sign * (m >> p), and sum exact bit counts of MagSgn (sum of
 * U - e_k), of the CxtVLC codewords and of the U-VLC fields, and the numbers of MEL symbols.  Only the MEL run lengths
 * depend on the order of the symbols; they are estimated from the two counts.  No bit is written and nothing is
 * serial.  Exponents of neighbour quads are recomputed from the magnitudes (a shift and a count of leading zeros), so
 * the planes need no array of their own and no barrier.
 * BASED (transcoding, a budget per frame): the block is read as |v| >> base[block], so that plane p of the tables is
 * plane base + p of the indices and nothing below the base is seen; the encoder launches the instantiation without. */
#define RC_PLANES 16
#define RC_SKIP   RC_PLANES         /* candidate index of "left out" */

struct RcStats {                    /* outputs, per block */
    uint64_t *dist;                 /* [RC_PLANES] */
    uint32_t *len;                  /* [RC_PLANES] */
    double   *dskip;                /* distortion of leaving the block out: sum of (2 m + 1)^2 */
    uint32_t *low0;                 /* a lower bound of the exact length at plane 0 */
    int32_t  *kmax;                 /* bit length of the largest magnitude: planes kmax and above are all zero */
};

/* exponents of the 4 samples of quad q at plane p, a byte each (k_ht_encode's E4) */
__device__ __forceinline__ uint32_t rc_e4(uint4 m, int p)
{
    return enc_expn(m.x >> p) | enc_expn(m.y >> p) << 8 | enc_expn(m.z >> p) << 16 | enc_expn(m.w >> p) << 24;
}

__device__ __forceinline__ uint32_t rc_e4(const uint32_t *M, int q, int p)
{
    return rc_e4(*(const uint4 *)(M + 4 * q), p);
}

/* the sum over the wave, in every lane (a butterfly: in doubles every lane ends with the same bits) */
template <typename T>
__device__ __forceinline__ T rc_wave_sum(T v)
{
    for (int off = 32; off > 0; off >>= 1)
        v += (T)__shfl_xor(v, off, 64);
    return v;
}

template <bool BASED>
__global__ void __launch_bounds__(64)
k_rc_stats(const EncBlk *__restrict__ blks, const int32_t *__restrict__ coef, const uint16_t *__restrict__ tab, int nplanes,
           RcStats S, const int32_t *__restrict__ base)
{
    __shared__ __attribute__((aligned(16))) uint32_t M[4 * ENC_MAX_QUADS];
    const int lane = threadIdx.x;
    const EncBlk B = blks[blockIdx.x];
    const int w = B.w, h = B.h, qw = (w + 1) >> 1, qh = (h + 1) >> 1, nq = qw * qh;
    const int32_t *src = coef + B.coef;
    const size_t row = (size_t)blockIdx.x * RC_PLANES;
    const int sh = BASED ? base[blockIdx.x] : 0;

    uint32_t mx = 0;
    /* sum of (2 m + 1)^2; exact while m < 2^15.  That suffices: it is stored only for planes p >= kmax, where every
     * m < 2^p, and p < nplanes <= 16 */
    uint64_t s64 = 0;
    double sd = 0.0;                                     /* the same in double, lanes in a fixed order */
    for (int q = lane; q < nq; q += 64) {
        const int qy = q / qw, qx = q - qy * qw;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int y = 2 * qy + (i & 1), x = 2 * qx + (i >> 1);
            uint32_t m = 0;
            if (y < h && x < w) {
                const int32_t v = src[(size_t)y * B.stride + x];
                m = (v < 0 ? 0u - (uint32_t)v : (uint32_t)v) >> sh;
            }
            M[4 * q + i] = m;
            mx = max(mx, m);
            if (m) {
                const uint64_t t = 2 * (uint64_t)m + 1;
                s64 += t * t;
                sd += (double)t * (double)t;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
        sd += __shfl_xor(sd, off, 64);
    }
    s64 = rc_wave_sum(s64);
    const int kmax = 32 - __clz((int)mx);               /* 0 for an all-zero block */
    const int nuse = min(nplanes, kmax);
    if (lane == 0) {
        S.dskip[blockIdx.x] = sd;
        S.kmax[blockIdx.x] = kmax;
        if (!nuse)
            S.low0[blockIdx.x] = 0;
    }
    for (int p = nuse + lane; p < nplanes; p += 64) {    /* all zero from here on: the distortion of leaving it out */
        S.dist[row + p] = s64;
        S.len[row + p] = 0;
    }
    __syncthreads();

    const int pw = (qw + 1) >> 1, npair = pw * qh;
    for (int p = 0; p < nuse; p++) {
        uint64_t dist = 0;
        uint32_t msb = 0, vlcb = 0, n0 = 0, n1 = 0;
        for (int pr = lane; pr < npair; pr += 64) {
            const int qy = pr / pw, qx0 = 2 * (pr - qy * pw);
            const int two = qx0 + 1 < qw;
            int u[2] = { 0, 0 };
            uint32_t left = qx0 > 0 ? rc_e4(M, qy * qw + qx0 - 1, p) : 0;
            /* the row above: quads qx0 - 1 .. qx0 + 2 */
            uint32_t ab[4] = { 0, 0, 0, 0 };
            if (qy > 0)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int x = qx0 - 1 + k;
                    if (x >= 0 && x < qw)
                        ab[k] = rc_e4(M, (qy - 1) * qw + x, p);
                }
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (k && !two)
                    break;
                const int q = qy * qw + qx0 + k;
                const uint4 m4 = *(const uint4 *)(M + 4 * q);
                const uint32_t mm[4] = { m4.x, m4.y, m4.z, m4.w };
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t m = mm[i], s = m >> p;
                    if (m) {
                        const int64_t d = s ? (int64_t)(2 * (uint64_t)m + 1) - (int64_t)(2 * ((uint64_t)s << p)) - ((int64_t)1 << p)
                                            : (int64_t)(2 * (uint64_t)m + 1);
                        dist += (uint64_t)(d * d);
                    }
                }
                const uint32_t e4 = rc_e4(m4, p);
                const QuadCode C = quad_code(e4, left, ab[k], ab[k + 1], ab[k + 2], qy == 0, tab);
                u[k] = C.u;
                if (C.vlc) {
                    vlcb += (C.t >> 8) & 7;
                    msb += (uint32_t)(__popc(C.rho) * C.U - __popc((int)((C.t >> 11) & 15) & C.rho));
                }
                if (C.ctx == 0) {
                    if (C.rho) n1++; else n0++;
                }
                left = e4;
            }
            const UPair P = uvlc_pair(u[0], u[1], qy == 0);
            if (P.mel >= 0) {
                if (P.mel) n1++; else n0++;
            }
            vlcb += (uint32_t)(uvlc_len(P.v[0]) + (P.one_bit ? 1 : uvlc_len(P.v[1])));
        }
        dist = rc_wave_sum(dist);
        const uint64_t packed = rc_wave_sum((uint64_t)msb | (uint64_t)vlcb << 32);
        const uint64_t mel = rc_wave_sum((uint64_t)n0 | (uint64_t)n1 << 32);
        if (lane == 0) {
            const uint32_t ms = (uint32_t)packed, vl = (uint32_t)(packed >> 32);
            const uint32_t z = (uint32_t)mel, o = (uint32_t)(mel >> 32);
            /* MEL: a 1 costs 1 + E bits, a 0 costs 2^-E, and the coder's state settles where 2^E is about the run length */
            const uint32_t run = z / (o ? o : 1u);
            const int E = min(5, 32 - __clz((int)run));
            const uint32_t melb = o * (uint32_t)(1 + E) + (z >> E);
            const uint32_t vbytes = max(2u, (vl + 12 + 7) >> 3);        /* 12 bits of Scup lead the VLC bytes */
            S.dist[row + p] = dist;
            S.len[row + p] = ((ms + 7) >> 3) + vbytes + ((melb + 7) >> 3);
            if (p == 0)
                S.low0[blockIdx.x] = (ms >> 3) + vbytes;                /* stuffing, MEL and padding only add */
        }
    }
}

/* k_rc_stats_passes: the sibling of k_rc_stats for calls that ask for passes, a wave per block.  For every refinement
 * plane p that leaves something significant at p + 1 (p <= kmax - 2) it builds the map and the membership as
 * k_ht_refine_encode does (ref_map, ref_members) and sums, exactly: the distortion of "cleanup at p + 1, SigProp at p"
 * (dist2) and of "... and MagRef at p" (dist3) in the units of k_rc_stats -- d = 2 m + 1 - 2 recon, with recon what the
 * decoder makes of a significant sample (the mid-point of the planes it has), of a newly significant member (3/2 2^p)
 * and of every other sample (0) -- and the bits of the two passes: a bit per member and a sign per newly significant
 * one; a bit per significant sample.  Planes without a candidate get 0 everywhere. */
struct RcPassStats {                /* outputs, per block, [RC_PLANES] each; all null in a call of one pass */
    uint64_t *dist2, *dist3;
    uint32_t *spbits, *mrbits;
};

template <bool BASED>
__global__ void __launch_bounds__(64)
k_rc_stats_passes(const EncBlk *__restrict__ blks, const int32_t *__restrict__ coef, int nplanes, RcPassStats P,
                  const int32_t *__restrict__ base)
{
    __shared__ __attribute__((aligned(16))) uint8_t ST[REF_ST_BYTES];
    const int lane = threadIdx.x;
    const EncBlk B = blks[blockIdx.x];
    const int w = B.w, h = B.h, n = w * h, bs = w + 2;
    const int32_t *src = coef + B.coef;
    const size_t row = (size_t)blockIdx.x * RC_PLANES;
    const int sh = BASED ? base[blockIdx.x] : 0;        /* as k_rc_stats: the block is |v| >> sh */
    uint32_t mx = 0;
    for (int i = lane; i < n; i += 64) {
        const int y = i / w, x = i - y * w;
        mx = max(mx, mag_at(src[(size_t)y * B.stride + x], sh).mag);
    }
    for (int off = 32; off > 0; off >>= 1)
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
    const int kmax = 32 - __clz((int)mx), nuse = min(nplanes, max(kmax - 1, 0));
    for (int p = nuse + lane; p < nplanes; p += 64) {
        P.dist2[row + p] = 0; P.dist3[row + p] = 0;
        P.spbits[row + p] = 0; P.mrbits[row + p] = 0;
    }
    const int gwn = (w + 3) >> 2, ng = gwn * ((h + 3) >> 2);
    const int chunk = (ng + 63) >> 6, g0 = min(ng, lane * chunk), g1 = min(ng, g0 + chunk);
    for (int p = 0; p < nuse; p++) {
        ref_map(ST, src, B.stride, w, h, sh + p, lane);
        ref_members(ST, w, h, g0, g1);
        uint64_t d2 = 0, d3 = 0;
        uint32_t sp = 0, mr = 0;
        for (int i = lane; i < n; i += 64) {
            const int y = i / w, x = i - y * w;
            const uint64_t m = mag_at(src[(size_t)y * B.stride + x], sh).mag;
            const uint32_t me = ST[(y + 1) * bs + x + 1];
            if (!m)
                continue;
            const int64_t full = (int64_t)(2 * m + 1);
            int64_t a = full, b = full;                  /* a sample SigProp does not reach, or whose bit is 0, decodes to 0 */
            if (me & REF_SIGMA) {
                a = full - (int64_t)(2 * ((m >> (p + 1)) << (p + 1))) - ((int64_t)2 << p);
                b = full - (int64_t)(2 * ((m >> p) << p)) - ((int64_t)1 << p);
                mr++;
            } else if (me & REF_NEWSIG) {
                a = b = full - ((int64_t)3 << p);
            }
            d2 += (uint64_t)(a * a);
            d3 += (uint64_t)(b * b);
        }
        for (int g = g0; g < g1; g++) {
            const int s = g / gwn, x0 = 4 * (g - s * gwn), y0 = 4 * s;
            int len;
            ref_sp_group(ST + (y0 + 1) * bs + x0 + 1, bs, min(4, w - x0), min(4, h - y0), &len);
            sp += (uint32_t)len;
        }
        d2 = rc_wave_sum(d2);
        d3 = rc_wave_sum(d3);
        const uint64_t bits = rc_wave_sum((uint64_t)sp | (uint64_t)mr << 32);
        if (lane == 0) {
            P.dist2[row + p] = d2; P.dist3[row + p] = d3;
            P.spbits[row + p] = (uint32_t)bits; P.mrbits[row + p] = (uint32_t)(bits >> 32);
        }
        __syncthreads();                                 /* the map is rebuilt for the next plane */
    }
}

/* k_rc_select: one workgroup per frame.  Every block has the candidates "plane p" (p below its highest, at most
 * RC_PLANES) and "left out"; for a slope lambda it takes the candidate with the least weight * dist + lambda * len
 * (ties to the smaller p; "left out" last), which is always a point of the lower convex hull of its (len, dist) set.
 * RC_STEPS bisection steps on lambda find the smallest slope whose estimated size fits the budget, ending on the
 * feasible side.  Lengths are the estimates times the block's scale (actual / estimated of an earlier launch, 1 at
 * first), rounded to bytes, plus an allowance for the block's share of the packet header; sums are integers.
 * A frame whose lower bounds at plane 0 fit the budget takes plane 0 throughout ("trial": it may fit as it is).
 * A call that asks for passes (maxpass 2 or 3) adds to every block the candidates of k_rc_stats_passes: rc_pick. */
#define RC_STEPS   64
#define RC_THREADS 1024

struct RcFrame {
    int32_t blk0, nblk;
    int64_t budget;                 /* bytes left for block segments and their packet-header share */
    int32_t allow_trial, pad;
};

struct RcSel {                      /* per frame */
    uint64_t est;                   /* estimated bytes of the selection (segments + header share) */
    double   lambda;
    int32_t  trial, pad;
};

__device__ __forceinline__ uint32_t rc_scaled(uint32_t len, double scale)
{
    if (!len)
        return 0;
    const double v = floor((double)len * scale + 0.5);
    return v < 1.0 ? 1u : v > 1.0e9 ? 1000000000u : (uint32_t)v;
}

/* bits of the packet header a block of L bytes accounts for: inclusion, zero bit-planes, passes, Lblock, length */
__device__ __forceinline__ uint32_t rc_hdr_bits(uint32_t L)
{
    return L ? 8u + 2u * (uint32_t)(32 - __clz((int)L)) : 0u;
}

/* what the second length field and the longer pass count add to a block's share of the packet header */
__device__ __forceinline__ uint32_t rc_hdr_bits(uint32_t L, int passes)
{
    return rc_hdr_bits(L) + (L && passes > 1 ? 3u + (uint32_t)(32 - __clz((int)L)) : 0u);
}

/* estimated bytes of the candidate "cleanup at p + 1, `passes` - 1 refinement passes at p" of block b (unscaled); 0: the
 * block has no such candidate (nothing significant at p + 1, or SigProp alone would write nothing) */
__device__ __forceinline__ uint32_t rc_pass_len(const RcStats &S, const RcPassStats &P, int b, int p, int passes)
{
    const size_t at = (size_t)b * RC_PLANES + p;
    const uint32_t sp = P.spbits[at], mr = P.mrbits[at];
    if (p + 1 >= RC_PLANES || !mr || (passes == 2 && !sp))
        return 0;
    return S.len[at + 1] + ((sp + 7) >> 3) + (passes > 2 ? (mr + 7) >> 3 : 0u);
}

/* the candidate block b takes at slope lambda -> its plane (RC_SKIP: left out), *len its scaled length, *passes its
 * passes.  maxpass > 1 adds, for every plane p, "cleanup at p + 1 and SigProp at p" and (3) "... and MagRef"; among
 * equals the fewer passes, then the smaller p */
__device__ __forceinline__ int rc_pick(const RcStats &S, const RcPassStats &P, int maxpass, const double *weight,
                                       const double *scale, int b, double lambda, uint32_t *len, int *passes)
{
    const int n = min(S.kmax[b], RC_PLANES);
    const double wt = weight[b], sc = scale[b];
    double best = wt * S.dskip[b];
    int at = RC_SKIP;
    uint32_t bl = 0;
    int bk = 1;
    for (int p = n - 1; p >= 0; p--) {                  /* downwards with <=: ties go to the smaller p */
        for (int k = maxpass; k > 1; k--) {
            const uint32_t raw = rc_pass_len(S, P, b, p, k);
            if (!raw)
                continue;
            const uint32_t L = rc_scaled(raw, sc);
            const uint64_t d = (k == 2 ? P.dist2 : P.dist3)[(size_t)b * RC_PLANES + p];
            const double J = wt * (double)d + lambda * (double)(L + ((rc_hdr_bits(L, k) + 7) >> 3));
            if (J <= best) {
                best = J;
                at = p;
                bl = L;
                bk = k;
            }
        }
        const uint32_t L = rc_scaled(S.len[(size_t)b * RC_PLANES + p], sc);
        const double J = wt * (double)S.dist[(size_t)b * RC_PLANES + p] + lambda * (double)(L + ((rc_hdr_bits(L) + 7) >> 3));
        if (J <= best) {
            best = J;
            at = p;
            bl = L;
            bk = 1;
        }
    }
    *len = bl;
    *passes = bk;
    return at;
}

/* the candidate of a block: its plane (RC_SKIP: left out), its passes, its scaled length */
struct RcCand { int at, passes; uint32_t len; };

/* block b's candidate at slope lambda: rc_pick's, or plane 0 where `plane0` says so for the whole frame (a frame on
 * trial, a frame short of its PSNR target) and for an all-zero block, which is not "left out": it keeps plane 0 */
__device__ __forceinline__ RcCand rc_cand(const RcStats &S, const RcPassStats &P, int maxpass, const double *weight,
                                          const double *scale, int b, double lambda, bool plane0)
{
    RcCand c = { 0, 1, 0 };
    if (plane0 || S.kmax[b] == 0)
        c.len = rc_scaled(S.len[(size_t)b * RC_PLANES], scale[b]);
    else
        c.at = rc_pick(S, P, maxpass, weight, scale, b, lambda, &c.len, &c.passes);
    return c;
}

/* what a selection leaves of block b's candidate: the plane (-1: left out) for the host and in the launch table, the
 * unscaled estimate of its bytes, and in calls that ask for passes the passes (k_ht_refine_plan reads them) */
__device__ __forceinline__ void rc_store(const RcStats &S, const RcPassStats &P, int maxpass, int b, const RcCand &c,
                                         EncBlk *blks, int32_t *planes, int32_t *passes, uint32_t *sel_len)
{
    const int p = c.at == RC_SKIP ? -1 : c.at;
    planes[b] = p;
    sel_len[b] = p < 0 ? 0 : c.passes > 1 ? rc_pass_len(S, P, b, p, c.passes) : S.len[(size_t)b * RC_PLANES + p];
    blks[b].plane = p;
    if (maxpass > 1) {
        passes[b] = c.passes;
        blks[b].npasses = c.passes;
    }
}

/* the sum over a workgroup of RC_THREADS threads, in every thread: the waves (rc_wave_sum), then the waves' sums in
 * index order; red: a word per wave */
template <typename T>
__device__ __forceinline__ T rc_block_sum(T v, T *red)
{
    v = rc_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = 0;
    for (int i = 0; i < RC_THREADS / 64; i++)
        t += red[i];
    return t;
}

/* the maximum over a workgroup of WAVES waves of values that are not negative, in every thread */
template <int WAVES>
__device__ __forceinline__ double rc_block_max(double v, double *red)
{
    for (int off = 32; off > 0; off >>= 1)
        v = fmax(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < WAVES; i++)
        t = fmax(t, red[i]);
    return t;
}

__global__ void __launch_bounds__(RC_THREADS)
k_rc_select(const RcFrame *__restrict__ frames, RcStats S, RcPassStats P, int maxpass, const double *__restrict__ weight,
            const double *__restrict__ scale, EncBlk *__restrict__ blks, int32_t *__restrict__ planes,
            int32_t *__restrict__ passes, uint32_t *__restrict__ sel_len, RcSel *__restrict__ sel)
{
    __shared__ uint64_t red[RC_THREADS / 64];
    __shared__ double redd[RC_THREADS / 64];
    const RcFrame F = frames[blockIdx.x];
    const int tid = threadIdx.x;

    /* plane 0 throughout when the frame may fit as it is */
    uint64_t low = 0;
    double top = 0.0;
    for (int i = tid; i < F.nblk; i += RC_THREADS) {
        const int b = F.blk0 + i;
        low += S.low0[b];
        top = fmax(top, weight[b] * S.dskip[b]);
    }
    low = rc_block_sum(low, red);
    top = rc_block_max<RC_THREADS / 64>(top, redd);
    const bool trial = F.allow_trial && (int64_t)low <= F.budget;

    double lo = 0.0, hi = top + 1.0, lambda = 0.0;       /* at hi every coded candidate costs more than leaving out */
    if (!trial) {
        for (int step = -1; step < RC_STEPS; step++) {
            const double mid = step < 0 ? 0.0 : 0.5 * (lo + hi);
            uint64_t sum = 0, bits = 0;
            for (int i = tid; i < F.nblk; i += RC_THREADS) {
                uint32_t L;
                int k;
                rc_pick(S, P, maxpass, weight, scale, F.blk0 + i, mid, &L, &k);
                sum += L;
                bits += rc_hdr_bits(L, k);
            }
            const uint64_t tsum = rc_block_sum(sum, red), tbits = rc_block_sum(bits, red);
            const bool fits = (int64_t)(tsum + ((tbits + 7) >> 3)) <= F.budget;
            if (step < 0) {
                if (fits) {
                    hi = 0.0;
                    break;
                }
            } else if (fits) {
                hi = mid;
            } else {
                lo = mid;
            }
        }
        lambda = hi;
    }
    uint64_t sum = 0, bits = 0;
    for (int i = tid; i < F.nblk; i += RC_THREADS) {
        const int b = F.blk0 + i;
        const RcCand c = rc_cand(S, P, maxpass, weight, scale, b, lambda, trial);
        rc_store(S, P, maxpass, b, c, blks, planes, passes, sel_len);
        sum += c.len;
        bits += rc_hdr_bits(c.len, c.passes);
    }
    const uint64_t tsum = rc_block_sum(sum, red), tbits = rc_block_sum(bits, red);
    if (tid == 0) {
        sel[blockIdx.x].est = tsum + ((tbits + 7) >> 3);
        sel[blockIdx.x].lambda = lambda;
        sel[blockIdx.x].trial = trial;
    }
}

/* ------------------------------------------------------------------ a budget over a group of frames
 * htj2k_enc_opts.group_bytes: one slope for the blocks of all frames of a call.  est_f(lambda) is what k_rc_select sums
 * for frame f (scaled lengths of rc_pick's candidates plus the header bits, rounded to bytes per frame; an all-zero
 * block counts at its plane-0 length), E(lambda) = sum over f of est_f(max(lambda, floor_f)) with floor_f the slope the
 * frame's own cap gave (0: none), and the bisection is k_rc_select's on E.  One workgroup cannot walk a quarter of a
 * million blocks 65 times, so the work has another shape:
 *   k_rc_group_sweep  a workgroup per chunk of RC_GROUP_CHUNK blocks of one frame, a thread per block.  It evaluates
 *                     the 2^k - 1 midpoints of the next k = RC_GROUP_LEVELS bisection levels (all computable from the
 *                     bracket: the tree of "fits" / "does not fit" outcomes; k from the measured sweep time,
 *                     DESIGN.md 3.5) and writes, per chunk and midpoint, the
 *                     sum of lengths and header bits as one packed integer.  The first sweep evaluates slope 0 alone
 *                     and also sums low0 and takes the maximum of weight * dskip.
 *   k_rc_group_step   one workgroup between two sweeps: sums the partials per frame (integers: any order gives the same
 *                     sums), rounds the bits per frame, adds the frames, walks the k levels and moves the bracket, which
 *                     lives in device memory (RcGroup).  The host enqueues all launches at once and never looks.
 *   k_rc_group_apply  a thread per block: rc_cand at max(lambda_g, floor_f), written by rc_store as k_rc_select does.
 * No workgroup waits for another inside a kernel; the kernel boundary is the only synchronisation.  The midpoints are
 * 0.5 * (lo + hi) along the same paths as the sequential steps take, so lambda comes out bit for bit the same. */
#define RC_GROUP_LEVELS 2
#define RC_GROUP_SLOTS  (1 << RC_GROUP_LEVELS)      /* 2^k - 1 midpoints per sweep; the last slot is spare */
#define RC_GROUP_CHUNK  256
#define RC_GROUP_LBITS  40                          /* a partial: lengths below, header bits above (256 blocks: < 2^38, < 2^24) */
enum { RC_GROUP_INIT, RC_GROUP_STEP, RC_GROUP_FINISH };

struct RcChunk { int32_t blk0, n, frame, pad; };
struct RcGFrame { int32_t chunk0, nchunk; };
struct RcGroupAux { uint64_t low; double top; };   /* per chunk, of the first sweep */
struct RcGroup {                    /* the bracket and the result, in device memory */
    double   lo, hi, lambda;
    uint64_t est;                   /* sum of est_f of the selection */
    int64_t  room;                  /* bytes for block segments and their header share, all frames */
    int32_t  step, done;            /* bisection steps taken; 1: lambda is final */
    int32_t  trial, allow_trial;
    int32_t  frames_capped, pad;    /* frames whose floor is above lambda */
};

/* the midpoint at node `node` (1: the root; 2 n: "fits", hi = mid; 2 n + 1: "does not fit", lo = mid) of the tree below (lo, hi) */
__device__ __forceinline__ double rc_group_mid(double lo, double hi, int node)
{
    for (int i = 30 - __clz(node); i >= 0; i--) {
        const double mid = 0.5 * (lo + hi);
        if ((node >> i) & 1)
            lo = mid;
        else
            hi = mid;
    }
    return 0.5 * (lo + hi);
}

/* what a candidate adds to est_f: scaled length | header bits << RC_GROUP_LBITS */
__device__ __forceinline__ uint64_t rc_group_cost(const RcCand &c)
{
    return (uint64_t)c.len | (uint64_t)rc_hdr_bits(c.len, c.passes) << RC_GROUP_LBITS;
}

__global__ void __launch_bounds__(RC_GROUP_CHUNK)
k_rc_group_sweep(const RcGroup *__restrict__ G, const RcChunk *__restrict__ chunks, const double *__restrict__ floors,
                 RcStats S, RcPassStats P, int maxpass, const double *__restrict__ weight, const double *__restrict__ scale,
                 int first, uint64_t *__restrict__ partial, RcGroupAux *__restrict__ aux)
{
    __shared__ double mids[RC_GROUP_SLOTS];
    __shared__ uint64_t red[RC_GROUP_CHUNK / 64][RC_GROUP_SLOTS];
    __shared__ uint64_t redl[RC_GROUP_CHUNK / 64];
    __shared__ double redt[RC_GROUP_CHUNK / 64];
    const int tid = threadIdx.x;
    const RcChunk C = chunks[blockIdx.x];
    int nslot = 1;
    if (first) {
        if (tid == 0)
            mids[0] = 0.0;
    } else {
        if (G->done)
            return;
        nslot = (1 << min(RC_GROUP_LEVELS, RC_STEPS - G->step)) - 1;
        if (tid < nslot)
            mids[tid] = rc_group_mid(G->lo, G->hi, tid + 1);
    }
    __syncthreads();
    const bool has = tid < C.n;
    const int b = C.blk0 + tid;
    const double fl = floors[C.frame];
    for (int s = 0; s < nslot; s++) {
        uint64_t v = 0;
        if (has)
            v = rc_group_cost(rc_cand(S, P, maxpass, weight, scale, b, fmax(mids[s], fl), false));
        v = rc_wave_sum(v);
        if ((tid & 63) == 0)
            red[tid >> 6][s] = v;
    }
    double top = 0.0;
    if (first) {
        const uint64_t low = rc_wave_sum<uint64_t>(has ? S.low0[b] : 0);
        if ((tid & 63) == 0)
            redl[tid >> 6] = low;
        top = rc_block_max<RC_GROUP_CHUNK / 64>(has ? weight[b] * S.dskip[b] : 0.0, redt);
    }
    __syncthreads();
    if (tid < nslot) {
        uint64_t t = 0;
        for (int i = 0; i < RC_GROUP_CHUNK / 64; i++)
            t += red[i][tid];
        partial[(size_t)blockIdx.x * RC_GROUP_SLOTS + tid] = t;
    }
    if (first && tid == 0) {
        RcGroupAux A = { 0, top };
        for (int i = 0; i < RC_GROUP_CHUNK / 64; i++)
            A.low += redl[i];
        aux[blockIdx.x] = A;
    }
}

/* one workgroup.  RC_GROUP_INIT, behind the first sweep: the trial rule, slope 0, or the first bracket.  RC_GROUP_STEP,
 * behind every other sweep: up to RC_GROUP_LEVELS steps.  RC_GROUP_FINISH, behind k_rc_group_apply: per frame `sel` as
 * k_rc_select fills it (lambda: the slope the frame's blocks took), the sum, and the frames their floor decided.
 * fsum: nframes * (RC_GROUP_SLOTS - 1) words of scratch */
__global__ void __launch_bounds__(RC_THREADS)
k_rc_group_step(RcGroup *__restrict__ G, const RcGFrame *__restrict__ gf, int nframes, int nchunks,
                const double *__restrict__ floors, const uint64_t *__restrict__ partial, const RcGroupAux *__restrict__ aux,
                uint64_t *__restrict__ fsum, int mode, RcSel *__restrict__ sel)
{
    __shared__ uint64_t E[RC_GROUP_SLOTS];
    __shared__ uint64_t red[RC_THREADS / 64];
    __shared__ double redd[RC_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (mode == RC_GROUP_STEP && G->done)
        return;
    const int nlev = mode == RC_GROUP_STEP ? min(RC_GROUP_LEVELS, RC_STEPS - G->step) : 1;
    const int nslot = (1 << nlev) - 1;
    /* est_f of every slot: a wave per (frame, slot), its lanes over the frame's chunks */
    for (size_t q = (size_t)wave; q < (size_t)nframes * nslot; q += RC_THREADS / 64) {
        const size_t f = q / nslot, s = q - f * nslot;
        const RcGFrame F = gf[f];
        uint64_t len = 0, bits = 0;
        for (int i = lane; i < F.nchunk; i += 64) {
            const uint64_t v = partial[(size_t)(F.chunk0 + i) * RC_GROUP_SLOTS + s];
            len += v & (((uint64_t)1 << RC_GROUP_LBITS) - 1);
            bits += v >> RC_GROUP_LBITS;
        }
        len = rc_wave_sum(len);
        bits = rc_wave_sum(bits);
        if (lane == 0)
            fsum[q] = len + ((bits + 7) >> 3);
    }
    __syncthreads();
    if (wave < nslot) {
        uint64_t e = 0;
        for (int f = lane; f < nframes; f += 64)
            e += fsum[(size_t)f * nslot + wave];
        e = rc_wave_sum(e);
        if (lane == 0)
            E[wave] = e;
    }
    __syncthreads();

    if (mode == RC_GROUP_INIT) {
        uint64_t low = 0;
        double top = 0.0;
        for (int i = tid; i < nchunks; i += RC_THREADS) {
            low += aux[i].low;
            top = fmax(top, aux[i].top);
        }
        int floored = 0;
        for (int f = tid; f < nframes; f += RC_THREADS)
            floored |= floors[f] > 0.0;
        floored = __syncthreads_or(floored);
        low = rc_block_sum(low, red);
        top = rc_block_max<RC_THREADS / 64>(top, redd);
        if (tid == 0) {
            const bool trial = G->allow_trial && !floored && (int64_t)low <= G->room;
            const bool fits = (int64_t)E[0] <= G->room;
            G->trial = trial;
            G->done = trial || fits;
            G->lambda = 0.0;
            G->lo = 0.0;
            G->hi = top + 1.0;                          /* at hi every coded candidate costs more than leaving out */
            G->step = 0;
        }
    } else if (mode == RC_GROUP_STEP) {
        if (tid == 0) {
            double lo = G->lo, hi = G->hi;
            int node = 1;
            for (int l = 0; l < nlev; l++) {
                const double mid = 0.5 * (lo + hi);
                const bool fits = (int64_t)E[node - 1] <= G->room;
                if (fits)
                    hi = mid;
                else
                    lo = mid;
                node = 2 * node + !fits;
            }
            G->lo = lo;
            G->hi = hi;
            G->step += nlev;
            if (G->step >= RC_STEPS) {
                G->lambda = hi;
                G->done = 1;
            }
        }
    } else {
        const int trial = G->trial;
        const double lambda = G->lambda;
        uint64_t capped = 0;
        for (int f = tid; f < nframes; f += RC_THREADS) {
            const bool own = !trial && floors[f] > lambda;
            sel[f].est = fsum[f];
            sel[f].lambda = trial ? 0.0 : own ? floors[f] : lambda;
            sel[f].trial = trial;
            capped += own;
        }
        capped = rc_block_sum(capped, red);
        if (tid == 0) {
            G->est = E[0];
            G->frames_capped = (int32_t)capped;
        }
    }
}

__global__ void __launch_bounds__(RC_GROUP_CHUNK)
k_rc_group_apply(const RcGroup *__restrict__ G, const RcChunk *__restrict__ chunks, const double *__restrict__ floors,
                 RcStats S, RcPassStats P, int maxpass, const double *__restrict__ weight, const double *__restrict__ scale,
                 EncBlk *__restrict__ blks, int32_t *__restrict__ planes, int32_t *__restrict__ passes,
                 uint32_t *__restrict__ sel_len, uint64_t *__restrict__ partial)
{
    __shared__ uint64_t red[RC_GROUP_CHUNK / 64];
    const int tid = threadIdx.x;
    const RcChunk C = chunks[blockIdx.x];
    const int b = C.blk0 + tid;
    uint64_t v = 0;
    if (tid < C.n) {
        const RcCand c = rc_cand(S, P, maxpass, weight, scale, b, fmax(G->lambda, floors[C.frame]), G->trial != 0);
        rc_store(S, P, maxpass, b, c, blks, planes, passes, sel_len);
        v = rc_group_cost(c);
    }
    v = rc_wave_sum(v);
    if ((tid & 63) == 0)
        red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        uint64_t t = 0;
        for (int i = 0; i < RC_GROUP_CHUNK / 64; i++)
            t += red[i];
        partial[(size_t)blockIdx.x * RC_GROUP_SLOTS] = t;
    }
}

/* the floors of the frames k_rc_select has just selected: entry j of `sel` is frame which[j] (null: frame j); a frame
 * on trial has no floor */
__global__ void __launch_bounds__(256)
k_rc_group_floors(const RcSel *__restrict__ sel, const int32_t *__restrict__ which, int n, double *__restrict__ floors)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n)
        floors[which ? which[j] : j] = sel[j].trial ? 0.0 : sel[j].lambda;
}

/* ------------------------------------------------------------------ constant quality
 * The dual of rate control (htj2k_amd.h, "constant quality"): the same candidates and the same slope search, on the
 * constraint D = sum of w (base + d / 4) <= D_target instead of the bytes.  Double sums run in a fixed order: strided per
 * thread, the wave (a butterfly: every lane ends with the same bits), then the waves in order (rc_block_sum).
 *
 * k_rc_base97: one wave per block, over the float plane between the forward 9/7 and the quantiser, which then
 * overwrites it.  base = sum of e^2 in index units, e the error of the caller's quantiser against its own mid-point
 * reconstruction (the whole magnitude where the index is 0); c and m are formed as k_quant97 forms them. */
__global__ void __launch_bounds__(64)
k_rc_base97(const EncBlk *__restrict__ blks, const float *__restrict__ coef, const float *__restrict__ step,
            double *__restrict__ base)
{
    const int lane = threadIdx.x;
    const EncBlk B = blks[blockIdx.x];
    const int w = B.w, n = w * B.h;
    const float *src = coef + B.coef;
    const double st = (double)step[blockIdx.x];
    double s = 0.0;
    for (int i = lane; i < n; i += 64) {                 /* consecutive lanes read consecutive samples of a row */
        const int y = i / w, x = i - y * w;
        const double c = fabs((double)src[(size_t)y * B.stride + x]) / st;
        double m = floor(c);
        if (m > 2147483000.0)
            m = 2147483000.0;
        const double e = m > 0.0 ? c - (m + 0.5) : c;
        s += e * e;
    }
    s = rc_wave_sum(s);
    if (lane == 0)
        base[blockIdx.x] = s;
}

/* k_rc_select_q: the sibling of k_rc_select, one workgroup per frame.  Every block takes rc_pick's candidate at slope
 * lambda; the frame's D is the sum of w base (once) and of w d / 4 of the candidates.  RC_STEPS bisection steps between
 * 0 and top + 1 find the largest slope with D <= dtarget, ending on the feasible side.  Slope 0 is every block at plane
 * 0 (d = 0): when that is not enough the frame is short of its target and takes plane 0 throughout.  When the upper
 * end is feasible every block is left out.  Lengths only steer the candidates (estimates, scale 1). */
struct RcQFrame {
    int32_t blk0, nblk;
    double  dtarget;                /* peak^2 N / 10^(target_psnr / 10) */
};

struct RcQual {                     /* per frame */
    double  d, dbase;               /* D of the selection; of plane 0 throughout (sum of w base) */
    double  lambda;
    int32_t short_of_target, pad;
};

/* d of candidate (at, k) of block b, as rc_pick reports it */
__device__ __forceinline__ double rc_cand_dist(const RcStats &S, const RcPassStats &P, int b, int at, int k)
{
    if (at == RC_SKIP)
        return S.dskip[b];
    const size_t i = (size_t)b * RC_PLANES + at;
    return (double)(k == 1 ? S.dist[i] : k == 2 ? P.dist2[i] : P.dist3[i]);
}

__global__ void __launch_bounds__(RC_THREADS)
k_rc_select_q(const RcQFrame *__restrict__ frames, RcStats S, RcPassStats P, int maxpass, const double *__restrict__ weight,
              const double *__restrict__ scale, const double *__restrict__ base, EncBlk *__restrict__ blks,
              int32_t *__restrict__ planes, int32_t *__restrict__ passes, uint32_t *__restrict__ sel_len,
              RcSel *__restrict__ sel, RcQual *__restrict__ qual)
{
    __shared__ uint64_t red[RC_THREADS / 64];
    __shared__ double redd[RC_THREADS / 64];
    const RcQFrame F = frames[blockIdx.x];
    const int tid = threadIdx.x;

    double dbase = 0.0, top = 0.0;
    for (int i = tid; i < F.nblk; i += RC_THREADS) {
        const int b = F.blk0 + i;
        if (base)                                        /* 5/3: the caller's quantiser has no error */
            dbase += weight[b] * base[b];
        top = fmax(top, weight[b] * S.dskip[b]);
    }
    dbase = rc_block_sum(dbase, redd);
    top = rc_block_max<RC_THREADS / 64>(top, redd);

    double lo = 0.0, hi = top + 1.0, lambda = 0.0;       /* at hi every coded candidate costs more than leaving out */
    bool shortof = false;
    for (int step = -2; step < RC_STEPS; step++) {       /* the two ends first, then the bisection */
        const double mid = step == -2 ? 0.0 : step == -1 ? hi : 0.5 * (lo + hi);
        double sum = 0.0;
        for (int i = tid; i < F.nblk; i += RC_THREADS) {
            const int b = F.blk0 + i;
            uint32_t L;
            int k;
            const int at = rc_pick(S, P, maxpass, weight, scale, b, mid, &L, &k);
            sum += weight[b] * (0.25 * rc_cand_dist(S, P, b, at, k));
        }
        const bool meets = dbase + rc_block_sum(sum, redd) <= F.dtarget;
        if (step == -2) {
            if (!meets) {
                shortof = true;
                break;
            }
        } else if (step == -1) {
            if (meets) {
                lo = hi;
                break;
            }
        } else if (meets) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    lambda = lo;

    uint64_t len = 0, bits = 0;
    double dsum = 0.0;
    for (int i = tid; i < F.nblk; i += RC_THREADS) {
        const int b = F.blk0 + i;
        const RcCand c = rc_cand(S, P, maxpass, weight, scale, b, lambda, shortof);
        rc_store(S, P, maxpass, b, c, blks, planes, passes, sel_len);
        len += c.len;
        bits += rc_hdr_bits(c.len, c.passes);
        dsum += weight[b] * (0.25 * rc_cand_dist(S, P, b, c.at, c.passes));
    }
    const uint64_t tlen = rc_block_sum(len, red), tbits = rc_block_sum(bits, red);
    const double d = dbase + rc_block_sum(dsum, redd);
    if (tid == 0) {
        sel[blockIdx.x].est = tlen + ((tbits + 7) >> 3);
        sel[blockIdx.x].lambda = lambda;
        sel[blockIdx.x].trial = 0;
        qual[blockIdx.x] = RcQual{ d, dbase, lambda, shortof ? 1 : 0, 0 };
    }
}

/* ------------------------------------------------------------------ gather */
struct GatherPiece {
    uint64_t dst;
    uint64_t src;                   /* byte offset in the literal buffer, or in the pool */
    uint32_t len, from_pool;
};

__global__ void __launch_bounds__(256)
k_enc_gather(const GatherPiece *__restrict__ pieces, const uint8_t *__restrict__ lit, const uint8_t *__restrict__ pool,
             uint8_t *__restrict__ out)
{
    const GatherPiece P = pieces[blockIdx.x];
    const uint8_t *s = (P.from_pool ? pool : lit) + P.src;
    uint8_t *d = out + P.dst;
    for (uint32_t i = threadIdx.x; i < P.len; i += 256)
        d[i] = s[i];
}

/* ------------------------------------------------------------------ transcoding
 * The block decoder keeps a plane per tile-component, the encoder one per component with every tile-component in its
 * rectangle: entry z copies a w x h plane (row stride w) to dst (row stride `stride`). */
#define XC_ROWS 4096                 /* rows of k_xc_scatter's grid at most */
struct XcPlane {
    const int32_t *src;
    int32_t *dst;
    int32_t w, h, stride, pad;
};

__global__ void __launch_bounds__(256)
k_xc_scatter(const XcPlane *__restrict__ planes)
{
    const XcPlane P = planes[blockIdx.z];
    const int x = (int)(blockIdx.x * 256 + threadIdx.x);
    if (x >= P.w)
        return;
    for (int y = (int)blockIdx.y; y < P.h; y += (int)gridDim.y)    /* the grid has XC_ROWS rows at most: planes may be taller */
        P.dst[(size_t)y * P.stride + x] = P.src[(size_t)y * P.w + x];
}

/* k_xc_limit: a budget per frame over the source's indices (htj2k_transcode_opts.target_bytes), a thread per block, behind
 * k_rc_stats<true> and k_rc_stats_passes<true> run at the base plane of every block: the plane pr of its source's last
 * pass.  The tables are then in planes relative to pr, and plane 0 offers forms the source cannot back: with k = 2
 * passes in the source one pass at pr, or a MagRef there, would state bits the source never coded; with k = 3 one pass
 * at pr would state bit pr of samples SigProp did not reach.  Those entries get the distortion UINT64_MAX, which
 * rc_pick never takes (weight * dskip is finite).  The block's own form -- k passes at relative plane 0, or, where
 * k_ht_refine_plan falls back, one pass at relative plane 1 -- goes to the selection's outputs as if it had been
 * selected: `planes` and `passes` for rc_collect, `sel_len` for rc_rescale to divide by.  src_passes[b] < 1: a block the
 * source left out; it has no form. */
__global__ void __launch_bounds__(256)
k_xc_limit(int n, const int32_t *__restrict__ src_passes, RcStats S, RcPassStats P, int32_t *__restrict__ planes,
           int32_t *__restrict__ passes, uint32_t *__restrict__ sel_len)
{
    const int b = (int)(blockIdx.x * 256 + threadIdx.x);
    if (b >= n)
        return;
    const size_t row = (size_t)b * RC_PLANES;
    const int k = src_passes[b];
    int plane = 0, np = 1;
    uint32_t own = 0;
    if (k < 1) {                                        /* whatever its samples hold, it offers the selection nothing */
        plane = -1;
        S.kmax[b] = 0;
        S.len[row] = 0;
        S.low0[b] = 0;
        S.dskip[b] = 0.0;
    } else if (k == 1) {
        own = S.len[row];
    } else {
        own = rc_pass_len(S, P, b, 0, k);               /* before the entries change: it reads the bits, not the distortions */
        S.dist[row] = UINT64_MAX;
        if (k == 2)
            P.dist3[row] = UINT64_MAX;
        if (own) {
            np = k;
        } else {
            plane = 1;
            own = S.len[row + 1];
        }
    }
    planes[b] = plane;
    passes[b] = np;
    sel_len[b] = own;
}

}  // namespace htj2k_enc
