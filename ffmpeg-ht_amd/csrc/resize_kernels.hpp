/*
 * resize_kernels.hpp -- windows of decoded frames resampled to one size as float images (htj2k_frames_to_tensor_resized,
 * htj2k_job_to_tensor_resized, htj2k_pipe_receive_tensor_resized).  include/htj2k_amd.h has the definition; in short, for
 * output pixel (x, y) of channel c of an out_w x out_h image resampled from the window (ox, oy, ww, wh):
 *     s(X, Y) = component c at ((ox + X) >> sw_c, (oy + Y) >> sh_c), read as the plain call reads it
 *     acc     = sum_Y qy_Y * sum_X qx_X * s(X, Y)     14-bit integer weights of either axis (resize_weights, below)
 *     f       = (float)((double)acc * 2^-28)          one rounding to nearest even
 *     t       = f * scale[c] + bias[c], stored as the plain call stores it (tensor_value_f, tensor_kernels.hpp)
 * Everything in front of f is integer arithmetic: the result does not depend on the order of the sums, on the tile or on
 * the rows a step takes.
 *
 *   resize_weights  the definition of an axis' weights, for the host (htj2k_resize_weights) and the kernel alike
 *   k_frame_resize  separable, streaming source rows.  A workgroup takes a tile of RS_TW x RS_TH output pixels of one
 *                   plane (all interleaved components of it).  It computes the tile's x and y weights once, in integers,
 *                   into LDS (one lane an output column or row); then it walks the source rows its tile needs, `rows` of
 *                   them a step: a lane forms the horizontal sums (< 2^30) of one output column and source row, the plane's
 *                   interleaved components side by side, from global memory into LDS, and after a barrier every lane adds
 *                   qy * h into the 64-bit accumulators of its RS_PY output pixels.  LDS is RS_LDS_BYTES whatever the reduction; no scratch, no atomics.
 *                   Samples are read as the general route reads them, one or two bytes; a two-byte sample is one load
 *                   where the plane's base and linesize are even (`pair`).
 *                   grid.x strides over a plane's tiles, grid.z is the plane.  Destination offsets are 64-bit.
 *   k_frame_rescale the same cut for htj2k_resize_frames, which writes frames: every plane is resampled from its own
 *                   window on its own grid (a chroma sample is read once, no `>> sw` on the source index), the table
 *                   entry holds the destination plane and its size, and the epilogue is r = (acc + 2^27) >> 28 stored as
 *                   the sample word in one or two bytes.  Both kernels are one body (resize_plane_tiles) with the epilogue
 *                   as its policy; the same two knobs, the same LDS, no scratch, no atomics.
 */
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace htj2k_cmp {

enum { RESIZE_NEAREST = 0, RESIZE_BILINEAR = 1, RESIZE_TRIANGLE = 2 };
enum { RS_MAX_SIZE = 32768, RS_MAX_REDUCTION = 64, RS_MAX_TAPS = 129, RS_ONE = 1 << 14 };

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD static inline
#endif

/* The taps of output index x of an axis that resamples `win` source pixels to `out`: -> their number, *first the first
 * source index, q[0 .. n) the weights, whose sum is RS_ONE.  1 <= win, out <= RS_MAX_SIZE, and win <= 64 out for
 * RESIZE_TRIANGLE: then n <= RS_MAX_TAPS, and every intermediate fits 32 bits -- a centre (2X + 1) * out and
 * cx = (2x + 1) * win are below 2^31 (at most 65535 * 32768), their difference is taken of two non-negative int32, S <= 2^16
 * so a << 14 < 2^31, and A < 2^23.  cx + S may pass 2^31 and is never formed. */
RS_HD int resize_weights(int win, int out, int filter, int x, int32_t *first, uint16_t *q)
{
    const int32_t cx = (int32_t)((uint32_t)(2 * x + 1) * (uint32_t)win);
    if (filter == RESIZE_NEAREST) {
        *first = (int32_t)((uint32_t)cx / (uint32_t)(2 * out));
        q[0] = (uint16_t)RS_ONE;
        return 1;
    }
    const int32_t S = filter == RESIZE_BILINEAR ? 2 * out : 2 * (out > win ? out : win);
    /* the first X >= 0 whose centre is above cx - S: 2X + 1 > lo / out, X = ceil(floor(lo / out) / 2) */
    const int32_t lo = cx - S;
    const int32_t X0 = lo < 0 ? 0 : (lo / out + 1) >> 1;
    uint32_t A = 0, best = 0;
    int n = 0, at = 0;
    for (int32_t X = X0; X < win && n < RS_MAX_TAPS; X++, n++) {
        const int32_t d = (int32_t)((uint32_t)(2 * X + 1) * (uint32_t)out) - cx;
        const int32_t a = S - (d < 0 ? -d : d);
        if (a <= 0) break;
        A += (uint32_t)a;
        if ((uint32_t)a > best) { best = (uint32_t)a; at = n; }
    }
    uint32_t sum = 0;
    for (int k = 0; k < n; k++) {
        const int32_t d = (int32_t)((uint32_t)(2 * (X0 + k) + 1) * (uint32_t)out) - cx;
        const uint32_t a = (uint32_t)(S - (d < 0 ? -d : d));
        const uint32_t w = (a << 14) / A;
        q[k] = (uint16_t)w;
        sum += w;
    }
    q[at] = (uint16_t)(q[at] + (RS_ONE - sum));
    *first = X0;
    return n;
}

} /* namespace htj2k_cmp */

#if defined(__HIPCC__)
#include "tensor_kernels.hpp"

namespace htj2k_cmp {

enum {
    RS_TW = 32, RS_TH = 16,                 /* a workgroup's tile of output pixels */
    RS_PY = RS_TW * RS_TH / CMP_THREADS,    /* output pixels of a lane: rows ty, ty + RS_TH / RS_PY, ... of column tx */
    RS_ROWS_MAX = 16, RS_ROWS_DEFAULT = 8,  /* source rows of a step (knob "resize_rows") */
    RS_LDS_BYTES = (RS_TW + RS_TH) * ((RS_MAX_TAPS + 1) * 2 + 8) + RS_ROWS_MAX * RS_TW * 4 * 4   /* 21 056 */
};
static_assert(RS_PY * CMP_THREADS == RS_TW * RS_TH && RS_TH % RS_PY == 0 && RS_TW + RS_TH <= CMP_THREADS, "the tile's cut");

struct ResizePlane {                /* one source plane of one frame */
    const uint8_t *src;             /* the plane */
    int64_t  ls;                    /* linesize, bytes */
    uint64_t dst_img;               /* element index of the frame's image in the destination */
    uint32_t ox, oy, ww, wh;        /* the window, in pixels of the frame */
    uint32_t comp0;                 /* component of the plane's first sample (planar layouts: the plane's; else 0) */
    uint32_t step;                  /* interleaved components of the plane */
    uint32_t sw, sh;                /* the plane's chroma shifts */
    uint32_t pair;                  /* two-byte samples may be read with one load: base and linesize are even */
    uint32_t share;                 /* log2 of the lanes that share a horizontal sum's taps, 0 .. 5 (resize_share) */
};

struct ResizeFmt {                  /* uniform over a call: TensorFmt, the filter and the rows of a step */
    TensorFmt T;
    uint32_t filter, rows;
};

/* What both kernels do for one plane: its tiles, blockIdx.x striding over them; for each, the weights into LDS, the source
 * rows streamed `rows` a step into horizontal sums, and the 64-bit accumulators of a lane's RS_PY output samples.  The plane
 * is `out_w x out_h` samples resampled from the ww x wh at (ox, oy), source sample X read at (ox + X) >> sw (and rows
 * likewise): k_frame_resize passes the frame's window and the plane's chroma shifts, k_frame_rescale the plane's own
 * window and no shift.  epi(x, y, c, acc) stores component c of output sample (x, y). */
template <class Epi>
__device__ __forceinline__ void resize_plane_tiles(const uint8_t *__restrict__ src, int64_t ls, uint32_t ox, uint32_t oy, uint32_t ww, uint32_t wh,
                                                   uint32_t sw, uint32_t sh, uint32_t step, uint32_t pair, uint32_t share, uint32_t out_w,
                                                   uint32_t out_h, uint32_t bytes, uint32_t shift, uint32_t mask, uint32_t filter, uint32_t rows,
                                                   const Epi &epi)
{
    /* taps of the tile's columns, then of its rows: weights, first source index, number */
    __shared__ uint16_t s_q[RS_TW + RS_TH][RS_MAX_TAPS + 1];
    __shared__ int32_t  s_first[RS_TW + RS_TH];
    __shared__ int32_t  s_n[RS_TW + RS_TH];
    __shared__ uint32_t s_h[RS_ROWS_MAX][RS_TW * 4];     /* horizontal sums of a step's rows: [row][column * step + c] */
    static_assert(sizeof(s_q) + sizeof(s_first) + sizeof(s_n) + sizeof(s_h) <= RS_LDS_BYTES, "the stated bound");

    const uint32_t tiles_x = (out_w + RS_TW - 1) / RS_TW, tiles_y = (out_h + RS_TH - 1) / RS_TH;
    const uint32_t tiles = tiles_x * tiles_y;            /* at most 1024 * 2048 */
    const uint32_t t = threadIdx.x, tx = t % RS_TW, ty = t / RS_TW;

    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t x0 = (tile % tiles_x) * RS_TW, y0 = (tile / tiles_x) * RS_TH;
        const uint32_t nx = min((uint32_t)RS_TW, out_w - x0), ny = min((uint32_t)RS_TH, out_h - y0);
        __syncthreads();                                 /* the last tile's readers are done */
        if (t < nx) s_n[t] = resize_weights((int)ww, (int)out_w, (int)filter, (int)(x0 + t), &s_first[t], s_q[t]);
        else if (t >= RS_TW && t - RS_TW < ny)
            s_n[t] = resize_weights((int)wh, (int)out_h, (int)filter, (int)(y0 + t - RS_TW), &s_first[t], s_q[t]);
        __syncthreads();
        /* first taps and last taps do not decrease along an axis: the tile's source rows are Y0 .. Y1 - 1 */
        const uint32_t Y0 = (uint32_t)s_first[RS_TW], Y1 = (uint32_t)(s_first[RS_TW + ny - 1] + s_n[RS_TW + ny - 1]);
        uint64_t acc[RS_PY][4];
#pragma unroll
        for (int p = 0; p < RS_PY; p++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[p][c] = 0;

        for (uint32_t Yb = Y0; Yb < Y1; Yb += rows) {
            const uint32_t nr = min(rows, Y1 - Yb);
            /* horizontal sums: an item is (row, column); the plane's components are summed side by side, so that a tap's
             * weight and address are found once.  2^share neighbouring lanes of a wave take an item's taps in turn -- they
             * read neighbouring pixels -- and add their sums up: integers, so the order does not show.  An item's lanes
             * are all there or all not: the items of a step are a multiple of the wave */
            const uint32_t G = 1u << share;
            for (uint32_t it = t; it < (nr * RS_TW) << share; it += CMP_THREADS) {
                const uint32_t g = it & (G - 1), item = it >> share, r = item / RS_TW, x = item % RS_TW;
                if (x >= nx) continue;
                const uint32_t sy = (oy + Yb + r) >> sh;
                const uint8_t *row = src + (int64_t)sy * ls;
                const uint32_t X = ox + (uint32_t)s_first[x];
                const int n = s_n[x];
                uint32_t h[4] = { 0, 0, 0, 0 };
                for (int k = (int)g; k < n; k += (int)G) {
                    const uint8_t *p = row + (uint64_t)((X + (uint32_t)k) >> sw) * (step * bytes);
                    const uint32_t q = s_q[x][k];
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        if ((uint32_t)c >= step) continue;
                        uint32_t raw;
                        if (bytes == 2) raw = pair ? (uint32_t)((const uint16_t *)p)[c] : (uint32_t)p[2 * c] | (uint32_t)p[2 * c + 1] << 8;
                        else raw = p[c];
                        h[c] += q * ((raw >> shift) & mask);
                    }
                }
                for (uint32_t d = G >> 1; d; d >>= 1) {
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        if ((uint32_t)c < step) h[c] += (uint32_t)__shfl_xor((int)h[c], (int)d);
                }
                if (g) continue;
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if ((uint32_t)c < step) s_h[r][x * step + c] = h[c];
            }
            __syncthreads();
            if (tx < nx) {
#pragma unroll
                for (int p = 0; p < RS_PY; p++) {
                    const uint32_t yy = ty + p * (RS_TH / RS_PY);
                    if (yy >= ny) continue;
                    /* the rows of the step that are taps of this output row: tap k is source row first + k */
                    const int32_t k0 = (int32_t)Yb - s_first[RS_TW + yy], n = s_n[RS_TW + yy];
                    const int32_t r0 = max(0, -k0), r1 = min((int32_t)nr, n - k0);
                    for (int32_t r = r0; r < r1; r++) {
                        const uint64_t qy = s_q[RS_TW + yy][k0 + r];
#pragma unroll
                        for (int c = 0; c < 4; c++)
                            if ((uint32_t)c < step) acc[p][c] += qy * s_h[r][tx * step + c];
                    }
                }
            }
            __syncthreads();
        }

        if (tx < nx) {
#pragma unroll
            for (int p = 0; p < RS_PY; p++) {
                const uint32_t yy = ty + p * (RS_TH / RS_PY);
                if (yy >= ny) continue;
                const uint32_t x = x0 + tx, y = y0 + yy;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    if ((uint32_t)c >= step) continue;
                    epi(x, y, c, acc[p][c]);
                }
            }
        }
    }
}

/* the float epilogue: one rounding of the sum, then scale and bias, stored where the tensor has channel comp0 + c */
template <int DT>
struct ResizeToTensor {
    typename TensorElem<DT>::type *img;
    const TensorFmt &F;
    uint32_t comp0;
    __device__ __forceinline__ void operator()(uint32_t x, uint32_t y, int c, uint64_t acc) const
    {
        const uint32_t k = comp0 + c;
        const float f = (float)((double)acc * 0x1p-28);
        const uint64_t at = F.nhwc ? ((uint64_t)y * F.out_w + x) * F.ncomp + k : ((uint64_t)k * F.out_h + y) * F.out_w + x;
        img[at] = tensor_value_f<DT>(f, F.scale[k & 3], F.bias[k & 3]);
    }
};

template <int DT>
__global__ void __launch_bounds__(CMP_THREADS)
k_frame_resize(const ResizePlane *__restrict__ planes, uint8_t *__restrict__ dst, ResizeFmt R)
{
    typedef typename TensorElem<DT>::type elem_t;
    const TensorFmt &F = R.T;
    const ResizePlane P = planes[blockIdx.z];
    const ResizeToTensor<DT> epi = { (elem_t *)dst + P.dst_img, F, P.comp0 };
    resize_plane_tiles(P.src, P.ls, P.ox, P.oy, P.ww, P.wh, P.sw, P.sh, P.step, P.pair, P.share, F.out_w, F.out_h, F.bytes, F.shift, F.mask,
                       R.filter, R.rows, epi);
}

/* ---- resized frames (htj2k_resize_frames): every plane of a destination frame resampled from the source plane's own
 * window, on the plane's own grid, and stored as sample words.  The table entry holds both planes and both sizes, so
 * planes of unlike size (luma and chroma, frames of a batch) go into one launch: grid.x strides over the tiles of the
 * plane with the most, grid.z is the plane. */
struct RescalePlane {               /* one plane of one frame, source and destination */
    const uint8_t *src;             /* the source plane */
    int64_t  ls;                    /* its linesize, bytes */
    uint8_t *dst;                   /* the destination plane */
    int64_t  dls;                   /* its linesize, bytes */
    uint32_t ox, oy, pw, ph;        /* the window in samples of the source plane: (ox >> sw, oy >> sh), ceilinged sizes */
    uint32_t dw, dh;                /* the destination plane, samples */
    uint32_t step;                  /* interleaved components of the plane */
    uint32_t pair;                  /* two-byte samples may be read with one load: source base and linesize are even */
    uint32_t dpair;                 /* and written with one store: destination base and linesize are even */
    uint32_t share;                 /* as ResizePlane::share, from the plane's own taps */
    uint32_t pad[2];
};
static_assert(sizeof(RescalePlane) == 80, "the table entry");

struct RescaleFmt {                 /* uniform over a call */
    uint32_t bytes, shift, mask;    /* of a sample word: 1 or 2 bytes, the sample at `shift`, 2^bits - 1 */
    uint32_t filter, rows;
};

/* the integer epilogue: r = (acc + 2^27) >> 28, at most the mask because the weights sum to 2^28; the word r << shift with
 * every other bit zero, in one or two bytes, byte by byte where a two-byte store would be misaligned.  Only bytes of
 * samples are written: x < dw and y < dh */
struct RescaleToFrame {
    uint8_t *dst;
    int64_t dls;
    uint32_t step, bytes, shift, dpair;
    __device__ __forceinline__ void operator()(uint32_t x, uint32_t y, int c, uint64_t acc) const
    {
        const uint32_t word = (uint32_t)((acc + (1ull << 27)) >> 28) << shift;
        uint8_t *p = dst + (int64_t)y * dls + (uint64_t)(x * step + (uint32_t)c) * bytes;
        if (bytes == 1) p[0] = (uint8_t)word;
        else if (dpair) *(uint16_t *)p = (uint16_t)word;
        else { p[0] = (uint8_t)word; p[1] = (uint8_t)(word >> 8); }
    }
};

__global__ void __launch_bounds__(CMP_THREADS)
k_frame_rescale(const RescalePlane *__restrict__ planes, RescaleFmt R)
{
    const RescalePlane P = planes[blockIdx.z];
    const RescaleToFrame epi = { P.dst, P.dls, P.step, R.bytes, R.shift, P.dpair };
    resize_plane_tiles(P.src, P.ls, P.ox, P.oy, P.pw, P.ph, 0u, 0u, P.step, P.pair, P.share, P.dw, P.dh, R.bytes, R.shift, R.mask, R.filter,
                       R.rows, epi);
}

} /* namespace htj2k_cmp */
#endif
