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
 *
 *   k_frame_ssim   per component of every frame of a call: the sum over its 8x8 windows at stride 4 of
 *                  rint(ssim * 2^32), libavfilter's vf_ssim.c in integers (include/htj2k_amd.h has the definition).
 *
 * The same planes, table and sample read.  A lane's group holds whole 4-sample block columns of every component of its
 * plane: 16 bytes, 24 (8-bit) or 48 (16-bit) for three interleaved components, 32 for four 16-bit ones -- 1, 2 or 4
 * block columns a lane (rgb24 with 48 bytes would be 4 of them: 200 registers and two waves a SIMD).  A wave
 * takes 64 groups of a row and walks a strip of block rows downwards: per block row four rows of loads, the 4x4 block
 * sums, each block added to its right neighbour (the lane's next block, or block 0 of the next lane by a cross-lane
 * move), that pair added to the pair of the block row above, which stays in registers: one window.  Seams: lane 63 of a
 * wave only lends its block 0 (the next wave starts on that group, so every load keeps its alignment of 16 or 8), and
 * a strip reads the last block row of the strip above again: (R + 1) / R of the rows at 64 / 63 of the groups.
 * Each window's value is three IEEE double operations and a rint on exact integers; lanes sum them as int64, and the
 * reduction is k_frame_diff's: wave, workgroup, one 64-bit integer atomic per workgroup and component.
 *
 *   k_frame_adler  per plane of every frame of a call: the two sums of Adler-32 seeded with 0 over the plane's bytes,
 *                  rows packed (include/htj2k_amd.h has the definition): A = sum d_i and B = sum (L - i) d_i, both to be
 *                  taken mod 65521 by the host, which also combines the planes of a frame.
 *
 * One operand, the same cut: 16-byte groups of a row whatever the layout (bytes are hashed, not samples), 16-byte loads
 * where base and linesize allow, the valid bytes one by one elsewhere.  A group at byte offset o of its packed plane adds
 * A_g = sum d_k to A and (w + 65521) A_g - sum k d_k to B, w = (L - o) mod 65521: never negative (k <= 15), below 2^29
 * (A_g <= 16 * 255, w + 65521 < 2^17), so a 64-bit accumulator is exact for planes below 2^38 bytes; the decoder's
 * largest plane has 2^33.  The weight stays in 32 bits: ((rows - y) mod M)(rowbytes mod M) < 2^32, the modulus is a
 * constant, nothing divides in 64 bits.  The byte sums are v_sad_u8 and v_dot4_u32_u8 (weights 0 .. 3) on the four words.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

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

struct SsimSums {                   /* one pair of frames */
    unsigned long long q[4];        /* two's complement: the sums are signed */
};

struct SsimFmt {                    /* uniform over a call */
    uint32_t shift, mask;
    uint32_t strip;                 /* block rows of windows per strip, at least 1 */
    uint32_t pad_;
    long long c1, c2;
};

#define CMP_THREADS 256
#define SSIM_LANES  63              /* lanes of a wave that own windows */

template <int GROUP>
__device__ __forceinline__ void cmp_load_group(const uint8_t *p, uint32_t nvalid, bool aligned, uint32_t (&w)[GROUP / 4])
{
    if (aligned && nvalid == GROUP) {
        if constexpr (GROUP % 16 == 0) {
#pragma unroll
            for (int q = 0; q < GROUP / 16; q++) {
                const uint4 v = ((const uint4 *)p)[q];
                w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
            }
        } else {                                         /* k_frame_ssim's 24-byte groups: a multiple of 8 into the row */
#pragma unroll
            for (int q = 0; q < GROUP / 8; q++) {
                const uint2 v = ((const uint2 *)p)[q];
                w[2 * q] = v.x; w[2 * q + 1] = v.y;
            }
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

/* bytes of a lane's group, of four samples of every interleaved component, block columns per group */
template <int BYTES, int STEP> struct SsimShape {
    static constexpr int UNIT = 4 * STEP * BYTES;
    static constexpr int GROUP = STEP == 3 ? (BYTES == 1 ? 24 : 48) : (UNIT > 16 ? UNIT : 16);
    static constexpr int NB = GROUP / UNIT;
};

/* one window from its sums: s1, s2 at most 64 * 65535, ss and s12 below 2^40; A .. D below 2^46, exact as doubles */
__device__ __forceinline__ long long ssim_window_q(uint32_t s1, uint32_t s2, unsigned long long ss, unsigned long long s12,
                                                   long long c1, long long c2)
{
    const long long p11 = (long long)((unsigned long long)s1 * s1), p22 = (long long)((unsigned long long)s2 * s2);
    const long long p12 = (long long)((unsigned long long)s1 * s2);
    const long long vars = 64 * (long long)ss - p11 - p22, covar = 64 * (long long)s12 - p12;
    const double A = (double)(2 * p12 + c1), B = (double)(2 * covar + c2), C = (double)(p11 + p22 + c1), D = (double)(vars + c2);
    const double v = (A * B) / (C * D);
    return (long long)rint(v * 4294967296.0);
}

/* grid.x strides over the (strip, 63 groups of a row) items of a plane, a wave per item; grid.z is the plane, as above.
 * Planes without a window (fewer than two block columns or block rows) must not be in the table. */
template <int BYTES, int STEP>
__global__ void __launch_bounds__(CMP_THREADS)
k_frame_ssim(const CmpPlane *__restrict__ planes, SsimSums *__restrict__ sums, SsimFmt F)
{
    constexpr int UNIT = SsimShape<BYTES, STEP>::UNIT, GROUP = SsimShape<BYTES, STEP>::GROUP, NB = SsimShape<BYTES, STEP>::NB;
    constexpr int NS = GROUP / BYTES, WAVES = CMP_THREADS / 64;
    typedef typename std::conditional<BYTES == 1, uint32_t, unsigned long long>::type wide_t;   /* 32 * 2 * 255^2 fits 32 bits */
    const CmpPlane P = planes[blockIdx.z];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t bw = P.rowbytes / UNIT, bh = P.rows >> 2;     /* samples beyond them are not read */
    long long acc[STEP];
#pragma unroll
    for (int c = 0; c < STEP; c++) acc[c] = 0;

    if (bw >= 2 && bh >= 2) {
        const uint32_t gw = (bw - 1 + NB - 1) / NB;              /* groups that own a window */
        const uint32_t nw = (gw + SSIM_LANES - 1) / SSIM_LANES, ns = (bh - 1 + F.strip - 1) / F.strip;
        const uint64_t items = (uint64_t)ns * nw, used = (uint64_t)bw * UNIT;
        for (uint64_t it = (uint64_t)blockIdx.x * WAVES + wave; it < items; it += (uint64_t)gridDim.x * WAVES) {
            const uint32_t strip = (uint32_t)(it / nw), wc = (uint32_t)(it - (uint64_t)strip * nw);
            const uint64_t g = (uint64_t)wc * SSIM_LANES + lane, off = g * GROUP;
            const uint32_t nvalid = off < used ? (uint32_t)min((uint64_t)GROUP, used - off) : 0;
            const uint32_t j0 = strip * F.strip, j1 = min(j0 + F.strip, bh - 1);     /* window rows j0 .. j1 - 1 */
            uint32_t p1[STEP][NB], p2[STEP][NB];                /* the block row above: blocks paired with their right neighbours */
            wide_t pss[STEP][NB], p12[STEP][NB];
            for (uint32_t br = j0; br <= j1; br++) {
                uint32_t s1[STEP][NB], s2[STEP][NB];
                wide_t ss[STEP][NB], s12[STEP][NB];
#pragma unroll
                for (int c = 0; c < STEP; c++)
#pragma unroll
                    for (int k = 0; k < NB; k++) { s1[c][k] = 0; s2[c][k] = 0; ss[c][k] = 0; s12[c][k] = 0; }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t y = (int64_t)br * 4 + r;
                    uint32_t wa[GROUP / 4], wb[GROUP / 4];
                    cmp_load_group<GROUP>(P.a + y * P.lsa + off, nvalid, P.aligned != 0, wa);
                    cmp_load_group<GROUP>(P.b + y * P.lsb + off, nvalid, P.aligned != 0, wb);
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        constexpr int per = 4 / BYTES;
                        const int sh = (s % per) * 8 * BYTES;
                        const uint32_t ra = (wa[s / per] >> sh) & (BYTES == 1 ? 0xFFu : 0xFFFFu);
                        const uint32_t rb = (wb[s / per] >> sh) & (BYTES == 1 ? 0xFFu : 0xFFFFu);
                        const uint32_t va = (ra >> F.shift) & F.mask, vb = (rb >> F.shift) & F.mask;
                        const int c = s % STEP, k = (s / STEP) / 4;
                        s1[c][k] += va;
                        s2[c][k] += vb;
                        ss[c][k] += (wide_t)va * va + (wide_t)vb * vb;
                        s12[c][k] += (wide_t)va * vb;
                    }
                }
#pragma unroll
                for (int c = 0; c < STEP; c++) {
                    /* block 0 of the next lane; lane 63 gets nothing of use and owns no window */
                    const uint32_t n1 = (uint32_t)__shfl_down((int)s1[c][0], 1, 64), n2 = (uint32_t)__shfl_down((int)s2[c][0], 1, 64);
                    const wide_t nss = __shfl_down(ss[c][0], 1, 64), n12 = __shfl_down(s12[c][0], 1, 64);
#pragma unroll
                    for (int k = 0; k < NB; k++) {
                        const bool last = k + 1 == NB;
                        const uint32_t h1 = s1[c][k] + (last ? n1 : s1[c][last ? 0 : k + 1]);
                        const uint32_t h2 = s2[c][k] + (last ? n2 : s2[c][last ? 0 : k + 1]);
                        const wide_t hss = ss[c][k] + (last ? nss : ss[c][last ? 0 : k + 1]);
                        const wide_t h12 = s12[c][k] + (last ? n12 : s12[c][last ? 0 : k + 1]);
                        if (br > j0 && lane < SSIM_LANES && g * NB + k + 1 < bw)
                            acc[c] += ssim_window_q(h1 + p1[c][k], h2 + p2[c][k], (unsigned long long)hss + pss[c][k],
                                                    (unsigned long long)h12 + p12[c][k], F.c1, F.c2);
                        p1[c][k] = h1; p2[c][k] = h2; pss[c][k] = hss; p12[c][k] = h12;
                    }
                }
            }
        }
    }

    __shared__ unsigned long long red[CMP_THREADS / 64][STEP];
#pragma unroll
    for (int c = 0; c < STEP; c++) {
        const unsigned long long a = cmp_wave_sum((unsigned long long)acc[c]);
        if (lane == 0) red[wave][c] = a;
    }
    __syncthreads();
    if (threadIdx.x < STEP) {
        const int c = threadIdx.x;
        unsigned long long a = 0;
        for (int w = 0; w < CMP_THREADS / 64; w++) a += red[w][c];
        if (a) atomicAdd(&sums[P.slot].q[(int)P.comp0 + c], a);
    }
}

struct HashPlane {                  /* one plane of one frame */
    const uint8_t *p;
    int64_t  ls;                    /* linesize, bytes */
    uint32_t rowbytes;              /* bytes of a row that are hashed */
    uint32_t rows;
    uint32_t slot;                  /* the frame's entry in the results */
    uint32_t plane;                 /* its index in the frame */
    uint32_t aligned;               /* base and linesize are multiples of 16 */
    uint32_t pad_;
};

struct HashSums {                   /* one frame; the host takes them mod ADLER_MOD */
    unsigned long long a[4], b[4];
};

#define ADLER_MOD 65521u

/* where group g of row y lies, how many of its 16 bytes are there (0 when y is beyond the plane) and its weight: bytes
 * from the group's first to the plane's end, (rows - y) rowbytes - off, mod M */
__device__ __forceinline__ const uint8_t *adler_locate(const HashPlane &P, uint32_t y, uint32_t g, uint32_t rowmod,
                                                       uint32_t &nvalid, uint32_t &wgt)
{
    nvalid = 0; wgt = 0;
    if (y >= P.rows) return P.p;
    const uint32_t off = g * 16;
    nvalid = min(16u, P.rowbytes - off);
    const uint32_t left = (((P.rows - y) % ADLER_MOD) * rowmod) % ADLER_MOD;
    wgt = (left + ADLER_MOD - off % ADLER_MOD) % ADLER_MOD;
    return P.p + (int64_t)y * P.ls + off;
}

/* the valid bytes of a group one by one, the rest zero: tails of rows and planes that are not aligned */
__device__ __forceinline__ uint4 adler_bytes(const uint8_t *p, uint32_t nvalid)
{
    uint32_t w[4];
    cmp_load_group<16>(p, nvalid, false, w);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

/* a group's shares of A (the sum of its bytes) and of B (the file comment) */
__device__ __forceinline__ void adler_sums(const uint4 v, uint32_t wgt, uint32_t &ag, uint32_t &bg)
{
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
    uint32_t kg = 0;                                     /* sum k d_k */
    ag = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t s = __builtin_amdgcn_sad_u8(w[q], 0u, 0u);
        ag += s;
        kg = __builtin_amdgcn_udot4(w[q], 0x03020100u, kg, false) + 4 * q * s;
    }
    bg = (wgt + ADLER_MOD) * ag - kg;
}

/* grid.x strides over the groups of a plane, two a lane and step, both loads issued before either is used (one operand:
 * as many bytes in flight as k_frame_diff has); grid.z is the plane, as above.  A lane divides once, to find its first
 * group; after that it walks (row, group) by the grid's stride as (dy, dg) with one carry: the division per group that
 * k_frame_diff hides behind its per-sample work would be a third of this kernel's instructions */
__global__ void __launch_bounds__(CMP_THREADS)
k_frame_adler(const HashPlane *__restrict__ planes, HashSums *__restrict__ sums)
{
    const HashPlane P = planes[blockIdx.z];
    const uint32_t gpr = (P.rowbytes + 15) / 16;             /* groups per row, the last one perhaps short */
    const uint32_t stride = gridDim.x * CMP_THREADS, first = blockIdx.x * CMP_THREADS + threadIdx.x;   /* at most 2^19 */
    const uint32_t dy = stride / gpr, dg = stride - dy * gpr;
    const bool aligned = P.aligned != 0;
    const uint32_t rowmod = P.rowbytes % ADLER_MOD;
    uint32_t y = first / gpr, g = first - y * gpr;           /* y + dy + 1 stays below 2^32: rows < 2^31 */
    unsigned long long a = 0, b = 0;
    while (y < P.rows) {
        uint32_t n0, n1, w0, w1;
        const uint8_t *p0 = adler_locate(P, y, g, rowmod, n0, w0);
        y += dy; g += dg;
        if (g >= gpr) { g -= gpr; y++; }
        const uint8_t *p1 = adler_locate(P, y, g, rowmod, n1, w1);
        y += dy; g += dg;
        if (g >= gpr) { g -= gpr; y++; }
        const bool full0 = aligned && n0 == 16, full1 = aligned && n1 == 16;
        uint4 v0 = make_uint4(0, 0, 0, 0), v1 = make_uint4(0, 0, 0, 0);
        if (full0) v0 = *(const uint4 *)p0;
        if (full1) v1 = *(const uint4 *)p1;
        if (!full0 && n0) v0 = adler_bytes(p0, n0);
        if (!full1 && n1) v1 = adler_bytes(p1, n1);
        uint32_t a0, b0, a1, b1;
        adler_sums(v0, w0, a0, b0);
        adler_sums(v1, w1, a1, b1);
        a += a0 + a1;                                    /* 2 * 4080 */
        b += (unsigned long long)b0 + b1;
    }

    __shared__ unsigned long long red[CMP_THREADS / 64][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    a = cmp_wave_sum(a);
    b = cmp_wave_sum(b);
    if (lane == 0) { red[wave][0] = a; red[wave][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = 0; b = 0;
        for (int w = 0; w < CMP_THREADS / 64; w++) { a += red[w][0]; b += red[w][1]; }
        if (a) {                                         /* all bytes zero: nothing to add to either sum */
            atomicAdd(&sums[P.slot].a[P.plane], a);
            atomicAdd(&sums[P.slot].b[P.plane], b);
        }
    }
}

} /* namespace htj2k_cmp */
