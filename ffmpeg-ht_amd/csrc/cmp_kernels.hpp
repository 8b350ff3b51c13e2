/*
 * cmp_kernels.hpp -- comparing two frames on the device (htj2k_compare_frames, htj2k_job_compare).
 *
 *   k_frame_diff   per component of every frame of a call: the sum of (a - b)^2, the number of samples that differ
 *                  and the largest |a - b|, over samples read as k_enc_unpack reads them
 *                  ((word >> shift) & mask).  A streaming reduction: two reads per sample, no writes but the sums.
 *
 * Work is cut into groups of GROUP bytes of a row, one group per lane and step: 16 bytes, or 48 for layouts of three
 * interleaved components (rgb24, rgb48le, xyz12le), so that byte k of a group belongs to a component that is known
 * when the kernel is compiled -- (k / BYTES) % STEP -- and no lane divides by three.  A plane whose two bases and two
 * linesizes are multiples of 16 has its full groups read with 16-byte loads; the tail of a row, and planes that are
 * not aligned, are read byte by byte, only the bytes that hold samples (padding is never read), the rest of the group
 * taken as zero on both sides, which adds nothing to any sum.
 * Lane sums are 64-bit (two 16-bit samples overflow 32 bits); they are reduced across the wave, then across the
 * workgroup through LDS, and one set of 64-bit integer atomics per workgroup and component goes into the frame's slot:
 * integer sums do not depend on the order of arrival, so the result is exact and repeatable.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace htj2k_cmp {

struct CmpPlane {                   /* one plane of one pair of frames */
    const uint8_t *a, *b;
    int64_t  lsa, lsb;              /* linesizes, bytes */
    uint32_t rowbytes;              /* bytes of a row that hold samples */
    uint32_t rows;
    uint32_t slot;                  /* the pair's entry in the results */
    uint32_t comp0;                 /* component of the plane's first sample (planar layouts: the plane's; else 0) */
    uint32_t aligned;               /* both bases and both linesizes are multiples of 16 */
    uint32_t pad_;
};

struct CmpSums {                    /* one pair of frames */
    unsigned long long sse[4], ndiff[4], max_abs[4];
};

struct CmpFmt {                     /* uniform over a call */
    uint32_t shift, mask;
};

#define CMP_THREADS 256

template <int GROUP>
__device__ __forceinline__ void cmp_load_group(const uint8_t *p, uint32_t nvalid, bool aligned, uint32_t (&w)[GROUP / 4])
{
    if (aligned && nvalid == GROUP) {
#pragma unroll
        for (int q = 0; q < GROUP / 16; q++) {
            const uint4 v = ((const uint4 *)p)[q];
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < GROUP / 4; q++)
        w[q] = 0;
#pragma unroll
    for (int k = 0; k < GROUP; k++)
        if ((uint32_t)k < nvalid)
            w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
}

__device__ __forceinline__ unsigned long long cmp_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ uint32_t cmp_wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v = max(v, (uint32_t)__shfl_down((int)v, o, 64));
    return v;
}

/* BYTES per sample (1, 2), STEP interleaved components per plane (1 .. 4).  grid.x strides over the groups of a plane,
 * grid.z is the plane (the host launches in chunks of what grid.z takes; z0: the chunk's first entry is planes[0]) */
template <int BYTES, int STEP>
__global__ void __launch_bounds__(CMP_THREADS)
k_frame_diff(const CmpPlane *__restrict__ planes, CmpSums *__restrict__ sums, CmpFmt F)
{
    constexpr int GROUP = STEP == 3 ? 48 : 16;
    constexpr int NS = GROUP / BYTES;                    /* samples of a group */
    const CmpPlane P = planes[blockIdx.z];
    const uint32_t gpr = (P.rowbytes + GROUP - 1) / GROUP;   /* groups per row, the last one perhaps short */
    const uint64_t total = (uint64_t)gpr * P.rows;
    unsigned long long sse[STEP], nd[STEP];
    uint32_t mx[STEP];
#pragma unroll
    for (int c = 0; c < STEP; c++) { sse[c] = 0; nd[c] = 0; mx[c] = 0; }

    for (uint64_t it = (uint64_t)blockIdx.x * CMP_THREADS + threadIdx.x; it < total; it += (uint64_t)gridDim.x * CMP_THREADS) {
        uint32_t y, g;
        if (total <= 0xFFFFFFFFull) { y = (uint32_t)it / gpr; g = (uint32_t)it - y * gpr; }
        else                        { y = (uint32_t)(it / gpr); g = (uint32_t)(it - (uint64_t)y * gpr); }
        const uint32_t off = g * GROUP;
        const uint32_t nvalid = min((uint32_t)GROUP, P.rowbytes - off);
        uint32_t wa[GROUP / 4], wb[GROUP / 4];
        cmp_load_group<GROUP>(P.a + (int64_t)y * P.lsa + off, nvalid, P.aligned != 0, wa);
        cmp_load_group<GROUP>(P.b + (int64_t)y * P.lsb + off, nvalid, P.aligned != 0, wb);
        uint32_t s2[STEP], n2[STEP];                    /* of this group: at most 24 samples a component, (2^16 - 1)^2 each */
        unsigned long long s2w[STEP];
#pragma unroll
        for (int c = 0; c < STEP; c++) { s2[c] = 0; n2[c] = 0; s2w[c] = 0; }
#pragma unroll
        for (int s = 0; s < NS; s++) {
            constexpr int per = 4 / BYTES;               /* samples per word */
            const int sh = (s % per) * 8 * BYTES;
            const uint32_t ra = (wa[s / per] >> sh) & (BYTES == 1 ? 0xFFu : 0xFFFFu);
            const uint32_t rb = (wb[s / per] >> sh) & (BYTES == 1 ? 0xFFu : 0xFFFFu);
            const int va = (int)((ra >> F.shift) & F.mask), vb = (int)((rb >> F.shift) & F.mask);
            const uint32_t d = (uint32_t)abs(va - vb);
            const int c = s % STEP;
            if (BYTES == 1) s2[c] += d * d;              /* 48 * 255^2 fits */
            else            s2w[c] += (unsigned long long)d * d;
            n2[c] += d != 0;
            mx[c] = max(mx[c], d);
        }
#pragma unroll
        for (int c = 0; c < STEP; c++) {
            sse[c] += BYTES == 1 ? (unsigned long long)s2[c] : s2w[c];
            nd[c] += n2[c];
        }
    }

    __shared__ unsigned long long red[CMP_THREADS / 64][3 * STEP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < STEP; c++) {
        const unsigned long long a = cmp_wave_sum(sse[c]), n = cmp_wave_sum(nd[c]);
        const uint32_t m = cmp_wave_max(mx[c]);
        if (lane == 0) { red[wave][3 * c] = a; red[wave][3 * c + 1] = n; red[wave][3 * c + 2] = m; }
    }
    __syncthreads();
    if (threadIdx.x < STEP) {
        const int c = threadIdx.x;
        unsigned long long a = 0, n = 0, m = 0;
        for (int w = 0; w < CMP_THREADS / 64; w++) {
            a += red[w][3 * c]; n += red[w][3 * c + 1]; m = max(m, red[w][3 * c + 2]);
        }
        if (n) {                                         /* nothing differs: nothing to add */
            CmpSums *S = sums + P.slot;
            const int k = (int)P.comp0 + c;
            atomicAdd(&S->sse[k], a);
            atomicAdd(&S->ndiff[k], n);
            atomicMax(&S->max_abs[k], m);
        }
    }
}

} /* namespace htj2k_cmp */
