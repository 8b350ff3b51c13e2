/*
 * tensor_kernels.hpp -- decoded frames as float images for a framework (htj2k_frames_to_tensor, htj2k_job_to_tensor,
 * htj2k_pipe_receive_tensor).  include/htj2k_amd.h has the definition; in short, for output pixel (x, y) of channel c of
 * an out_w x out_h window whose corner is the source pixel (ox, oy):
 *     s = component c at ((ox + x) >> sw_c, (oy + y) >> sh_c), read as k_frame_diff reads it ((word >> shift) & mask)
 *     t = (float)s * scale[c] + bias[c]      one binary32 multiplication, then one binary32 addition, never fused
 *     stored as binary32, binary16 or bfloat16 (both rounded to nearest even), NCHW or NHWC, contiguous
 *
 *   k_frame_tensor      the fast route, input-driven on k_frame_diff's cut: a lane takes one group of a row of the window,
 *                       16 bytes or 48 for three interleaved components, so that the component of every byte is known when
 *                       the kernel is compiled and no lane divides by three.  Full groups are one (three) 16-byte loads
 *                       (cmp_load_group); a row's last group may be short and is read byte by byte, only the bytes that
 *                       hold samples.  A group's samples go out as runs of consecutive elements: NCHW one run of
 *                       NP = NS / STEP pixels per component, NHWC one run of all NS samples; runs longer than one
 *                       16-byte store are shared by neighbouring lanes, a store each (TensorShape).  A run goes
 *                       out in 16-byte stores where the plane's `wide` says every full run of the plane starts on a
 *                       multiple of 16 (the rule: tensor_wide, htj2k_device.hip), else element by element; a short run
 *                       writes its valid elements only.  Planes on this route have no chroma shift, a base and a linesize
 *                       that are multiples of 16, and a window that starts on a group boundary of the source row: the
 *                       host folds the origin into `src`.
 *   k_frame_tensor_any  the general route, output-driven: one output element per lane and step, any origin, chroma shift,
 *                       alignment and layout.  A sample is read as its one or two bytes, nothing else of the row.
 *
 * Both give the same bits: the same read, the same two rounded operations (__fmul_rn, __fadd_rn: the compiler may not
 * contract them, whatever -ffp-contract says), the same conversion.  binary16 is v_cvt_f16_f32 under the code object's
 * modes (round to nearest even, denormals kept); bfloat16 is the definition's integer formula, three VALU operations:
 * t is never NaN here (finite scale and bias, a finite sample), and the formula is right for infinities.
 * No atomics, no LDS, no results: grid.x strides over a plane's work, grid.z is the plane (tensor tables are launched in
 * chunks of what grid.z takes, as the comparisons').  Destination offsets are 64-bit element indices.
 *
 * The other direction, tensors as frames (htj2k_encode_tensor, htj2k_tensor_to_frames): sample (x, y) of component c is
 *     e = the tensor element at (x << sw_c, y << sh_c), the co-sited top-left element of a chroma sample's footprint
 *     r = rintf((float)e * scale[c] + bias[c])    the same two rounded operations, then round to nearest, ties to even
 *     s = 0 unless r > 0 (NaN, -inf, negatives, -0); 2^bits - 1 where r >= 2^bits - 1 (+inf); else (uint)r
 * tensor_in_sample is that definition, once: the encoder's k_enc_unpack_tensor (enc_kernels.hpp) and k_tensor_frame
 * below both call it, so a codestream and a frame made from one tensor cannot differ.  tensor_in_value is its first
 * step, the element widened to binary32, which the calls with a mix (mix_in_kernels.hpp) start from as well.
 *
 *   k_tensor_frame      output-driven, one sample word per lane and step: s << shift as the one or two bytes of the
 *                       sample, nothing else of the row, whatever the plane's base and linesize.
 *
 * A translation unit that wants the definition alone (htj2k_encode.hip) defines HTJ2K_TENSOR_IN_ONLY before it includes
 * this file: cmp_kernels.hpp and the kernels that build on it are then left out.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <type_traits>
#ifndef HTJ2K_TENSOR_IN_ONLY
#include "cmp_kernels.hpp"
#endif

namespace htj2k_cmp {

enum { TENSOR_F32 = 0, TENSOR_F16 = 1, TENSOR_BF16 = 2 };

template <int DT> struct TensorElem { typedef uint16_t type; };
template <> struct TensorElem<TENSOR_F32> { typedef uint32_t type; };

/* element `at` of the tensor widened to binary32 */
template <int DT>
__device__ __forceinline__ float tensor_in_value(const void *__restrict__ tensor, uint64_t at)
{
    const typename TensorElem<DT>::type e = ((const typename TensorElem<DT>::type *)tensor)[at];
    if constexpr (DT == TENSOR_F32) return __uint_as_float(e);
    else if constexpr (DT == TENSOR_F16) return __half2float(__ushort_as_half(e));
    else return __uint_as_float((uint32_t)e << 16);
}

/* tensors as frames, the definition: element `at` of the tensor -> the sample of `bits` bits, peak = 2^bits - 1.  The
 * element's value as binary32 is exact for all three types (binary16 subnormals included: v_cvt_f32_f16 keeps them);
 * the product and the sum are rounded separately, whatever -ffp-contract says; rintf is v_rndne_f32.  peak <= 65535 is
 * exact in binary32, and 0 < r < peak converts without rounding. */
template <int DT>
__device__ __forceinline__ uint32_t tensor_in_sample(const void *__restrict__ tensor, uint64_t at, float scale, float bias, uint32_t peak)
{
    const float f = tensor_in_value<DT>(tensor, at);
    const float r = rintf(__fadd_rn(__fmul_rn(f, scale), bias));
    if (!(r > 0.0f)) return 0;
    if (r >= (float)peak) return peak;
    return (uint32_t)r;
}

/* where that element is: pixel (X, Y) of channel c of an image of C channels, H x W, from the image's first element */
template <int NHWC>
__device__ __forceinline__ uint64_t tensor_in_at(uint32_t c, uint32_t X, uint32_t Y, uint32_t C, uint32_t W, uint32_t H)
{
    return NHWC ? ((uint64_t)Y * W + X) * C + c : ((uint64_t)c * H + Y) * W + X;
}

#ifndef HTJ2K_TENSOR_IN_ONLY

struct TensorPlane {                /* one source plane of one frame */
    const uint8_t *src;             /* fast route: the window's first byte in the plane; general: the plane's */
    int64_t  ls;                    /* linesize, bytes */
    uint64_t dst_img;               /* element index of the frame's image in the destination */
    uint32_t ox, oy;                /* general route: the window's corner, in pixels of the frame */
    uint32_t comp0;                 /* component of the plane's first sample (planar layouts: the plane's; else 0) */
    uint32_t step;                  /* interleaved components of the plane */
    uint32_t sw, sh;                /* the plane's chroma shifts */
    uint32_t wide;                  /* fast route: every full run of the plane may be written in 16-byte stores */
    uint32_t pad_;
};

struct TensorFmt {                  /* uniform over a call */
    uint32_t shift, mask;
    uint32_t out_w, out_h;
    uint32_t ncomp;                 /* C: channels of an image */
    uint32_t bytes;                 /* per sample */
    uint32_t nhwc;
    uint32_t pad_;
    float    scale[4], bias[4];
};

/* the element's bits from a sample's value: an integer sample (tensor_value), or a resampled one (resize_kernels.hpp) */
template <int DT>
__device__ __forceinline__ typename TensorElem<DT>::type tensor_value_f(float f, float scale, float bias)
{
    const float t = __fadd_rn(__fmul_rn(f, scale), bias);
    if constexpr (DT == TENSOR_F32) {
        return __float_as_uint(t);
    } else if constexpr (DT == TENSOR_F16) {
        return __half_as_ushort(__float2half_rn(t));
    } else {
        const uint32_t u = __float_as_uint(t);
        return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
    }
}

/* the element's bits from a sample */
template <int DT>
__device__ __forceinline__ typename TensorElem<DT>::type tensor_value(uint32_t s, float scale, float bias)
{
    return tensor_value_f<DT>((float)s, scale, bias);
}

/* N consecutive elements of which the first n are there; `wide`: o is a multiple of 16 when the run is full */
template <int N, class T>
__device__ __forceinline__ void tensor_store_run(T *o, const T (&v)[N], uint32_t n, bool wide)
{
    constexpr int PER = 16 / (int)sizeof(T);
    if constexpr (N % PER == 0) {
        if (wide && n == (uint32_t)N) {
#pragma unroll
            for (int q = 0; q < N / PER; q++) {
                uint4 w;
                if constexpr (sizeof(T) == 4) {
                    w = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
                } else {
                    w = make_uint4((uint32_t)v[8 * q] | (uint32_t)v[8 * q + 1] << 16, (uint32_t)v[8 * q + 2] | (uint32_t)v[8 * q + 3] << 16,
                                   (uint32_t)v[8 * q + 4] | (uint32_t)v[8 * q + 5] << 16, (uint32_t)v[8 * q + 6] | (uint32_t)v[8 * q + 7] << 16);
                }
                /* as one vector value: stored through HIP's uint4 struct, the float16 NCHW instantiations came out as
                 * global_store_dwordx3 and two 2-byte stores */
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 x = { w.x, w.y, w.z, w.w };
                ((u32x4 *)o)[q] = x;
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < N; k++)
        if ((uint32_t)k < n) o[k] = v[k];
}

/* the fast route's cut.  A group's run (NCHW: its NP pixels of one component; NHWC: all its NS samples) is RUN elements;
 * where that is two or more 16-byte stores, SHARE neighbouring lanes take the same group (the same loads, out of the
 * cache for all but one) and each converts and stores one 16-byte PART of every run: a wave's store instruction then
 * writes 1 KiB side by side.  With one lane a group the same instruction wrote 16 bytes every 32 or 64, and rgb24 and
 * rgb48le to float32 ran at 0.49 and 0.69 of the copy kernel's rate; shared, at 0.87 and 0.91 ("Frames
 * as tensors") */
template <int BYTES, int STEP, int DT, int NHWC> struct TensorShape {
    static constexpr int GROUP = STEP == 3 ? 48 : 16;
    static constexpr int NS = GROUP / BYTES, NP = NS / STEP;     /* samples and pixels of a group */
    static constexpr int PER = DT == TENSOR_F32 ? 4 : 8;         /* elements of a 16-byte store */
    static constexpr int RUN = NHWC ? NS : NP;
    static constexpr int SHARE = (RUN % PER == 0 && RUN / PER >= 2) ? RUN / PER : 1;
    static constexpr int PART = RUN / SHARE;
};

/* BYTES per sample (1, 2), STEP interleaved components per plane (1 .. 4), DT the element, NHWC only with STEP equal to
 * the image's channels (then a group's samples are consecutive elements).  grid.x strides over the (group, part) items
 * of a plane's window, grid.z is the plane */
template <int BYTES, int STEP, int DT, int NHWC>
__global__ void __launch_bounds__(CMP_THREADS)
k_frame_tensor(const TensorPlane *__restrict__ planes, uint8_t *__restrict__ dst, TensorFmt F)
{
    typedef typename TensorElem<DT>::type elem_t;
    typedef TensorShape<BYTES, STEP, DT, NHWC> S;
    constexpr int GROUP = S::GROUP, NP = S::NP, SHARE = S::SHARE, PART = S::PART;
    constexpr int NRUN = NHWC ? 1 : STEP;                /* runs a lane writes */
    const TensorPlane P = planes[blockIdx.z];
    const uint32_t rowbytes = F.out_w * (uint32_t)(STEP * BYTES);
    const uint32_t gpr = (rowbytes + GROUP - 1) / GROUP;     /* groups per row, the last one perhaps short */
    const uint64_t total = (uint64_t)gpr * F.out_h * SHARE;
    const bool wide = P.wide != 0;
    float sc[STEP], bi[STEP];
#pragma unroll
    for (int c = 0; c < STEP; c++) { sc[c] = F.scale[(P.comp0 + c) & 3]; bi[c] = F.bias[(P.comp0 + c) & 3]; }
    elem_t *const img = (elem_t *)dst + P.dst_img;

    for (uint64_t it = (uint64_t)blockIdx.x * CMP_THREADS + threadIdx.x; it < total; it += (uint64_t)gridDim.x * CMP_THREADS) {
        uint32_t y, g;
        const uint32_t sub = (uint32_t)it % SHARE;       /* SHARE neighbouring lanes take the same group */
        if (total <= 0xFFFFFFFFull) { const uint32_t q = (uint32_t)it / SHARE; y = q / gpr; g = q - y * gpr; }
        else                        { const uint64_t q = it / SHARE; y = (uint32_t)(q / gpr); g = (uint32_t)(q - (uint64_t)y * gpr); }
        const uint32_t off = g * GROUP;
        const uint32_t nvalid = min((uint32_t)GROUP, rowbytes - off);
        const uint32_t nrun = nvalid / (uint32_t)(NHWC ? BYTES : STEP * BYTES);   /* elements of the group's run(s) that are there */
        const uint32_t first = sub * PART;               /* this lane's part of them */
        const uint32_t n = nrun > first ? min((uint32_t)PART, nrun - first) : 0;
        uint32_t w[GROUP / 4];
        cmp_load_group<GROUP>(P.src + (int64_t)y * P.ls + off, nvalid, true, w);
        elem_t v[NRUN][PART];
        /* the part's samples are picked with indices known at compile time: one branch per part, the stores after them,
         * so that the lanes of a wave store side by side in one instruction */
#pragma unroll
        for (int part = 0; part < SHARE; part++) {
            if (sub != (uint32_t)part) continue;
#pragma unroll
            for (int r = 0; r < NRUN; r++) {
#pragma unroll
                for (int k = 0; k < PART; k++) {
                    constexpr int per = 4 / BYTES;       /* samples per word */
                    const int e = part * PART + k;       /* element of the run */
                    const int s = NHWC ? e : e * STEP + r;   /* sample of the group */
                    const int c = NHWC ? e % STEP : r;
                    const uint32_t raw = (w[s / per] >> ((s % per) * 8 * BYTES)) & (BYTES == 1 ? 0xFFu : 0xFFFFu);
                    v[r][k] = tensor_value<DT>((raw >> F.shift) & F.mask, sc[c], bi[c]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < NRUN; r++) {
            elem_t *o = NHWC ? img + ((uint64_t)y * F.out_w + (uint64_t)g * NP) * STEP + first
                             : img + ((uint64_t)(P.comp0 + r) * F.out_h + y) * F.out_w + (uint64_t)g * NP + first;
            tensor_store_run<PART>(o, v[r], n, wide);
        }
    }
}

/* one output element per lane and step, in the order of the destination within the plane's share of the image (NCHW: a
 * component's rows; NHWC: pixels, the plane's components together).  grid.x strides over them, grid.z is the plane */
template <int DT>
__global__ void __launch_bounds__(CMP_THREADS)
k_frame_tensor_any(const TensorPlane *__restrict__ planes, uint8_t *__restrict__ dst, TensorFmt F)
{
    typedef typename TensorElem<DT>::type elem_t;
    const TensorPlane P = planes[blockIdx.z];
    const uint64_t total = (uint64_t)P.step * F.out_w * F.out_h;
    elem_t *const img = (elem_t *)dst + P.dst_img;

    for (uint64_t it = (uint64_t)blockIdx.x * CMP_THREADS + threadIdx.x; it < total; it += (uint64_t)gridDim.x * CMP_THREADS) {
        uint32_t x, y, c;
        if (total <= 0xFFFFFFFFull) {
            const uint32_t e = (uint32_t)it;
            if (F.nhwc) { const uint32_t r = e / P.step; c = e - r * P.step; y = r / F.out_w; x = r - y * F.out_w; }
            else        { const uint32_t r = e / F.out_w; x = e - r * F.out_w; c = r / F.out_h; y = r - c * F.out_h; }
        } else {
            if (F.nhwc) { const uint64_t r = it / P.step; c = (uint32_t)(it - r * P.step); y = (uint32_t)(r / F.out_w); x = (uint32_t)(r - (uint64_t)y * F.out_w); }
            else        { const uint64_t r = it / F.out_w; x = (uint32_t)(it - r * F.out_w); c = (uint32_t)(r / F.out_h); y = (uint32_t)(r - (uint64_t)c * F.out_h); }
        }
        const uint32_t sx = (P.ox + x) >> P.sw, sy = (P.oy + y) >> P.sh;
        const uint8_t *p = P.src + (int64_t)sy * P.ls + ((uint64_t)sx * P.step + c) * F.bytes;
        uint32_t raw = p[0];
        if (F.bytes == 2) raw |= (uint32_t)p[1] << 8;
        const uint32_t k = P.comp0 + c;
        const elem_t v = tensor_value<DT>((raw >> F.shift) & F.mask, F.scale[k & 3], F.bias[k & 3]);
        const uint64_t at = F.nhwc ? ((uint64_t)y * F.out_w + x) * F.ncomp + k : ((uint64_t)k * F.out_h + y) * F.out_w + x;
        img[at] = v;
    }
}

/* ---- tensors as frames */
struct TensorInPlane {              /* one destination plane of one frame */
    uint8_t *dst;                   /* the plane */
    int64_t  ls;                    /* linesize, bytes */
    uint64_t src_img;               /* element index of the frame's image in the tensor */
    uint32_t comp0;                 /* component of the plane's first sample (planar layouts: the plane's; else 0) */
    uint32_t step;                  /* interleaved components of the plane */
    uint32_t sw, sh;                /* the plane's chroma shifts */
    uint32_t pw, ph;                /* pixels of a row of the plane and its rows: the component's ceilinged size */
};

struct TensorInFmt {                /* uniform over a call */
    uint32_t shift, peak;           /* the word is s << shift; 2^bits - 1 */
    uint32_t w, h;                  /* of the images */
    uint32_t ncomp;                 /* C: channels of an image */
    uint32_t bytes;                 /* per sample */
    uint32_t nhwc;
    uint32_t pad_;
    float    scale[4], bias[4];
};

/* one sample word per lane and step, in the order of the plane's bytes; only the bytes of samples are written.  grid.x
 * strides over them, grid.z is the plane */
template <int DT>
__global__ void __launch_bounds__(CMP_THREADS)
k_tensor_frame(const TensorInPlane *__restrict__ planes, const uint8_t *__restrict__ src, TensorInFmt F)
{
    typedef typename TensorElem<DT>::type elem_t;
    const TensorInPlane P = planes[blockIdx.z];
    const uint64_t total = (uint64_t)P.step * P.pw * P.ph;
    const elem_t *const img = (const elem_t *)src + P.src_img;

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
        const uint64_t at = F.nhwc ? tensor_in_at<1>(k, x << P.sw, y << P.sh, F.ncomp, F.w, F.h)
                                   : tensor_in_at<0>(k, x << P.sw, y << P.sh, F.ncomp, F.w, F.h);
        const uint32_t word = tensor_in_sample<DT>(img, at, F.scale[k & 3], F.bias[k & 3], F.peak) << F.shift;
        uint8_t *p = P.dst + (int64_t)y * P.ls + ((uint64_t)x * P.step + c) * F.bytes;
        p[0] = (uint8_t)word;
        if (F.bytes == 2) p[1] = (uint8_t)(word >> 8);
    }
}

#endif /* HTJ2K_TENSOR_IN_ONLY */

} /* namespace htj2k_cmp */
