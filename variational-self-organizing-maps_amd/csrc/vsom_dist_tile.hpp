// vsom_dist_tile.hpp -- the distance tile of the exact search, written once for the chunk queries (gfx950).
//
// vsom_dist_tile computes every (row, node) distance of a 16 * TI-row x 64-node tile in the reference's fp32 order (8 class
// accumulators + Eigen's reduction tree, the remainder in Eigen's order) on the VALU and hands each one to the
// caller's epilogue.  Its callers: bmd_tile_kernel (vsom_bmd.hip), topk_tile_kernel (vsom_topk.hip) and masked_tile_kernel
// (vsom_masked.hip).  They differ in the validity mask (a policy, below) and in what becomes of a distance (the epilogue);
// the operations and their order are the same for all of them, hence the same bits.  bmu_tile_body (vsom_bmu.hip) holds
// the one remaining copy, with row and node lists: see there for why.
#pragma once
#include "vsom_device.hpp"
#include <type_traits>

#define LDT 36  // LDS row stride in floats: 16-B aligned, lane rows land on distinct 4-bank slots
#define MSK_LDV (VSOM_TK / 4)   // dwords per row of the validity tile

// r where the column is valid (m = ~0), +0 where it is not (m = 0): whatever r holds, a NaN included
template <bool ON = true>
__device__ __forceinline__ float masked_sel(float r, int m)
{
    return ON ? __int_as_float(__float_as_int(r) & m) : r;
}

// the 4 validity bytes of w (0xFF / 0x00) applied to the 4 columns of v
__device__ __forceinline__ float4 masked_sel4(float4 v, int w)
{
    return make_float4(masked_sel(v.x, (int)((unsigned)w << 24) >> 24), masked_sel(v.y, (int)((unsigned)w << 16) >> 24),
                       masked_sel(v.z, (int)((unsigned)w << 8) >> 24), masked_sel(v.w, w >> 24));
}

// Mask policies.  The masked ones take vp: the packed validity rows of the slice, vld bytes each, 0xFF = valid, 0x00 =
// invalid or padding (Standard / Median only).
//  VsomMaskNone : every column counts.  No select, no validity tile.
//  VsomMaskRows : one validity row per sample (row s - s0 at vp + (s - s0) * vld), staged as a byte tile in LDS beside the
//                 sample tile; every residual becomes r_d = valid ? m_d - x_d : +0 (a select on the bits) before it is
//                 squared, in the inner loop and in the remainder.  The thread stages 8 validity bytes per K-chunk.
//  VsomMaskOne  : the one row at vp holds for every sample, so it is applied to BOTH operands when a K-chunk is staged
//                 (x' = valid ? x : +0, m' = valid ? m : +0, hence m' - x' = +0 at an invalid column and the untouched
//                 m - x at a valid one): the inner loop is the unmasked one and there is no validity tile -- the thread
//                 fetches the 4 bytes of the columns it stages.
struct VsomMaskNone {
};
struct VsomMaskRows {
    const unsigned char *vsrc;
    bool vload;
    __device__ VsomMaskRows(const unsigned char *vp, int vld, int tid, int sbase, int s0, int s1)
        : vsrc(vp + (size_t)(sbase + (tid >> 2) - s0) * vld + (tid & 3) * 8), vload(sbase + (tid >> 2) < s1)
    {
    }
};
struct VsomMaskOne {
    const unsigned char *vsrc;
    __device__ VsomMaskOne(const unsigned char *vp, int, int tid, int, int, int) : vsrc(vp + (tid & 7) * 4) {}
};

// One tile: sample rows [sbase, sbase + 16 * TI) below s1 against nodes [nbase, nbase + 64) below N; rows and nodes past
// the ends read as zeros.  Every thread of the 256 calls it (it holds barriers); thread tid owns the pairs
// (row ty + 16 * i, node tx + 16 * j), tx = tid & 15, ty = tid >> 4, and epi(i, j, res) receives their distances with i
// outer and j inner.  The caller puts a barrier between two tiles (the remainder reads the last chunk from LDS).
//
// TI = sample rows per thread: 4 for Standard / Median (64 x 64 tile, 128 accumulators per thread).  The CLR
// residual needs two more operand arrays (y', B): with 4 x 4 pairs the kernel sat at 256 VGPRs with 46 spilled
// dwords in the hot loop and no room to prefetch (r2: VALU 54 % busy, 2.3 ms at C5).  CLR therefore takes
// TI = 2 -- a 32-sample x 64-node tile, 64 accumulators -- which leaves registers for the next K-chunk's loads
// in flight while the current one is consumed and lets three workgroups share a CU.
template <bool CLR, int TI, class Mask, class Epi>
__device__ __forceinline__ void vsom_dist_tile(const DistArgs &a, int tid, int sbase, int s1, int nbase, int N,
                                               const Mask &mask, Epi epi)
{
    constexpr bool ROWS = std::is_same<Mask, VsomMaskRows>::value, ONE = std::is_same<Mask, VsomMaskOne>::value;
    static_assert(!CLR || (!ROWS && !ONE), "the masked tiles are Standard / Median only");
    constexpr int TS = 16 * TI;                 // samples per tile
    constexpr int NX = TS * 8 / 256;            // float4 of a sample operand per thread and K-chunk (1 or 2)
    __shared__ __attribute__((aligned(16))) float sx[TILE * LDT];   // TS rows used
    __shared__ __attribute__((aligned(16))) float sm[TILE * LDT];
    __shared__ __attribute__((aligned(16))) float sy[CLR ? TS * LDT : 4];
    __shared__ __attribute__((aligned(16))) float sb[CLR ? TILE * LDT : 4];
    __shared__ __attribute__((aligned(16))) int sv[ROWS ? TS * MSK_LDV : 4];    // the validity tile, bytes

    const int tx = tid & 15, ty = tid >> 4;
    const int L = a.L, L8 = L & ~7;
    const int nchunks = (L + VSOM_TK - 1) / VSOM_TK;

    float acc[TI][4][8];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k)
                acc[i][j][k] = 0.f;

    // global -> register staging of one K-chunk; the NEXT chunk's loads stay in flight while the current one is
    // consumed (register prefetch: the loads used to be issued and waited for between the two barriers, with
    // only two wavefronts per SIMD to cover them)
    float4 gx[NX], gm[2], gy[NX], gb[2];
    uint2 gv;
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            int f = tid + 256 * i;
            int row = f >> 3, c4 = (f & 7) * 4;
            int s = sbase + row;
            gx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            gy[i] = gx[i];
            if (s < s1) {
                gx[i] = *reinterpret_cast<const float4 *>(a.xa + (size_t)s * a.ldx + k0 + c4);
                if (CLR)
                    gy[i] = *reinterpret_cast<const float4 *>(a.xb + (size_t)s * a.ldx + k0 + c4);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int f = tid + 256 * i;
            int row = f >> 3, c4 = (f & 7) * 4;
            int n = nbase + row;
            gm[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            gb[i] = gm[i];
            if (n < N) {
                gm[i] = *reinterpret_cast<const float4 *>(a.ma + (size_t)n * a.ldm + k0 + c4);
                if (CLR)
                    gb[i] = *reinterpret_cast<const float4 *>(a.mb + (size_t)n * a.ldm + k0 + c4);
            }
        }
        gv = make_uint2(0u, 0u);
        if constexpr (ONE)
            gv.x = *reinterpret_cast<const unsigned *>(mask.vsrc + k0);
        if constexpr (ROWS)
            if (mask.vload)
                gv = *reinterpret_cast<const uint2 *>(mask.vsrc + k0);
    };
    gload(0);
    int dk = 0;
    for (int ch = 0; ch < nchunks; ++ch, dk += VSOM_TK) {
        if (ch > 0)
            __syncthreads();
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            int f = tid + 256 * i;
            int row = f >> 3, c4 = (f & 7) * 4;
            if constexpr (ONE)
                gx[i] = masked_sel4(gx[i], (int)gv.x);
            *reinterpret_cast<float4 *>(&sx[row * LDT + c4]) = gx[i];
            if (CLR)
                *reinterpret_cast<float4 *>(&sy[row * LDT + c4]) = gy[i];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int f = tid + 256 * i;
            int row = f >> 3, c4 = (f & 7) * 4;
            if constexpr (ONE)
                gm[i] = masked_sel4(gm[i], (int)gv.x);
            *reinterpret_cast<float4 *>(&sm[row * LDT + c4]) = gm[i];
            if (CLR)
                *reinterpret_cast<float4 *>(&sb[row * LDT + c4]) = gb[i];
        }
        if (ROWS)
            *reinterpret_cast<uint2 *>(&sv[tid * 2]) = gv;     // row tid >> 2, bytes 8 * (tid & 3) ..
        __syncthreads();
        if (ch + 1 < nchunks)
            gload(dk + VSOM_TK);
#pragma unroll
        for (int kk = 0; kk < VSOM_TK; kk += 8) {
            if (dk + kk < L8) {   // whole 8-blocks only; the remainder is handled in Eigen's order below
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    float4 xv[TI], mv[4], yv[TI], bv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        mv[j] = *reinterpret_cast<const float4 *>(&sm[(tx + 16 * j) * LDT + kk + 4 * h]);
                        if (CLR)
                            bv[j] = *reinterpret_cast<const float4 *>(&sb[(tx + 16 * j) * LDT + kk + 4 * h]);
                    }
#pragma unroll
                    for (int i = 0; i < TI; ++i) {
                        xv[i] = *reinterpret_cast<const float4 *>(&sx[(ty + 16 * i) * LDT + kk + 4 * h]);
                        if (CLR)
                            yv[i] = *reinterpret_cast<const float4 *>(&sy[(ty + 16 * i) * LDT + kk + 4 * h]);
                    }
#pragma unroll
                    for (int i = 0; i < TI; ++i) {
                        // VsomMaskRows: the row's 4 validity bytes -> 0 / ~0 per column
                        const int w = ROWS ? sv[(ty + 16 * i) * MSK_LDV + (kk >> 2) + h] : 0;
                        const int m[4] = {(int)((unsigned)w << 24) >> 24, (int)((unsigned)w << 16) >> 24,
                                          (int)((unsigned)w << 8) >> 24, w >> 24};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float r0 = masked_sel<ROWS>(vsom_resid<CLR>(xv[i].x, CLR ? yv[i].x : 0.f, mv[j].x, CLR ? bv[j].x : 0.f),
                                                        m[0]);
                            float r1 = masked_sel<ROWS>(vsom_resid<CLR>(xv[i].y, CLR ? yv[i].y : 0.f, mv[j].y, CLR ? bv[j].y : 0.f),
                                                        m[1]);
                            float r2 = masked_sel<ROWS>(vsom_resid<CLR>(xv[i].z, CLR ? yv[i].z : 0.f, mv[j].z, CLR ? bv[j].z : 0.f),
                                                        m[2]);
                            float r3 = masked_sel<ROWS>(vsom_resid<CLR>(xv[i].w, CLR ? yv[i].w : 0.f, mv[j].w, CLR ? bv[j].w : 0.f),
                                                        m[3]);
                            float p0 = r0 * r0, p1 = r1 * r1, p2 = r2 * r2, p3 = r3 * r3;
                            acc[i][j][4 * h + 0] = acc[i][j][4 * h + 0] + p0;
                            acc[i][j][4 * h + 1] = acc[i][j][4 * h + 1] + p1;
                            acc[i][j][4 * h + 2] = acc[i][j][4 * h + 2] + p2;
                            acc[i][j][4 * h + 3] = acc[i][j][4 * h + 3] + p3;
                        }
                    }
                }
            }
        }
    }

    // reduction tree + remainder (the last chunk is still in LDS)
    const int rem = L - L8;
    const int roff = L8 - (nchunks - 1) * VSOM_TK;   // column of element L8 inside the last chunk
    const signed char *svb = reinterpret_cast<const signed char *>(sv);
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float q0 = acc[i][j][0] + acc[i][j][4];
            float q1 = acc[i][j][1] + acc[i][j][5];
            float q2 = acc[i][j][2] + acc[i][j][6];
            float q3 = acc[i][j][3] + acc[i][j][7];
            const int xr = (ty + 16 * i) * LDT + roff, mr = (tx + 16 * j) * LDT + roff;
            const int vr = ROWS ? (ty + 16 * i) * VSOM_TK + roff : 0;
            int t = 0;
            if (rem >= 4) {
                float r0 = masked_sel<ROWS>(vsom_resid<CLR>(sx[xr + 0], CLR ? sy[xr + 0] : 0.f, sm[mr + 0], CLR ? sb[mr + 0] : 0.f),
                                            (int)svb[vr + 0]);
                float r1 = masked_sel<ROWS>(vsom_resid<CLR>(sx[xr + 1], CLR ? sy[xr + 1] : 0.f, sm[mr + 1], CLR ? sb[mr + 1] : 0.f),
                                            (int)svb[vr + 1]);
                float r2 = masked_sel<ROWS>(vsom_resid<CLR>(sx[xr + 2], CLR ? sy[xr + 2] : 0.f, sm[mr + 2], CLR ? sb[mr + 2] : 0.f),
                                            (int)svb[vr + 2]);
                float r3 = masked_sel<ROWS>(vsom_resid<CLR>(sx[xr + 3], CLR ? sy[xr + 3] : 0.f, sm[mr + 3], CLR ? sb[mr + 3] : 0.f),
                                            (int)svb[vr + 3]);
                float p0 = r0 * r0, p1 = r1 * r1, p2 = r2 * r2, p3 = r3 * r3;
                q0 = q0 + p0;
                q1 = q1 + p1;
                q2 = q2 + p2;
                q3 = q3 + p3;
                t = 4;
            }
            float t02 = q0 + q2, t13 = q1 + q3;
            float res = t02 + t13;
            for (; t < rem; ++t) {
                float r = masked_sel<ROWS>(vsom_resid<CLR>(sx[xr + t], CLR ? sy[xr + t] : 0.f, sm[mr + t], CLR ? sb[mr + t] : 0.f),
                                           (int)svb[vr + t]);
                float p = r * r;
                res = res + p;
            }
            epi(i, j, res);
        }
}
