// vsom_masked.hip -- Som::findRestrictedBmu (Som.cpp:313-332) over the VALID columns of every chunk row in [r0, r1), the
// distance Som::euclidianWeightedDist documents (Som.cpp:112-141, the masked form of :139), and the imputed record
// (gfx950; Standard / Median).
//
//  masked_pack_kernel   : the caller's validity bytes (rows x J, or J with one_mask) -> rows of xpitch bytes, 0xFF = valid,
//                         0x00 = invalid or padding: aligned 8-byte loads for the tile, one sign extension per mask word
//  masked_tile_kernel   : the distance tile of bmd_tile_kernel (vsom_bmd.hip: 64 rows x 64 nodes, 8 class accumulators +
//                         Eigen's reduction tree, the same operations in the same order) with a validity tile staged in LDS
//                         beside the sample tile: r_d = valid ? m_d - x_d : +0 (a select on the bits: an AND with 0 / ~0),
//                         squared and accumulated as in the unmasked tile.  A workgroup walks G consecutive node tiles and
//                         every thread keeps the smallest key of its 4 rows over the nodes that qualify (node 0, or
//                         bmuHits >= min_hits); one key per (row, node group) leaves the workgroup.  It also flags the rows
//                         whose d_0 is NaN.  No rows x N matrix.  With one_mask the mask is applied to both operands as a
//                         K-chunk is staged instead (see the kernel): no validity tile, the unmasked inner loop.
//  masked_reduce_kernel : one wavefront per row: the smallest of the row's group keys, the node-0 rule, the count of valid
//                         columns
//  masked_fill_kernel   : x where valid, map[bmu] where not, row-major (consecutive lanes, consecutive columns)
// The validity tile stays bytes in LDS (32 per row and K-chunk): the 16 lanes of a wavefront that share a row read one
// dword (a broadcast) and the four rows of a wavefront lie 8 banks apart, so the byte-wide tile has no bank conflict; a
// tile widened to 0 / 1 floats at staging time would cost a second 16-byte LDS read per sample row and 4 columns -- as much
// LDS traffic again as the sample tile -- to save one v_bfe_i32 per column, shared by the 4 nodes of the thread.
// The distance body is a copy of bmd_tile_kernel's: no existing kernel changes.
#include "vsom_device.hpp"
#include <algorithm>
#include <cstdlib>

#define TILE 64
#define LDT 36
#define MSK_LDV (VSOM_TK / 4)   // dwords per row of the validity tile
#define MSK_MAXG 64             // node groups per row at most: one reduce lane each
#define MSK_SCRATCH ((size_t)64 << 20)

// r where the column is valid (m = ~0), +0 where it is not (m = 0): whatever r holds, a NaN included
template <bool ON = true>
__device__ __forceinline__ float masked_sel(float r, int m)
{
    return ON ? __int_as_float(__float_as_int(r) & m) : r;
}

__device__ __forceinline__ float4 masked_sel4(float4 v, int w)
{
    return make_float4(masked_sel(v.x, (int)((unsigned)w << 24) >> 24), masked_sel(v.y, (int)((unsigned)w << 16) >> 24),
                       masked_sel(v.z, (int)((unsigned)w << 8) >> 24), masked_sel(v.w, w >> 24));
}

// rows x J bytes (any non-zero = valid) -> rows x vld bytes of 0xFF / 0x00, four columns per thread
__global__ __launch_bounds__(256) void masked_pack_kernel(const unsigned char *__restrict__ raw, int J, int vld,
                                                          unsigned *__restrict__ packed)
{
    const size_t row = blockIdx.x;
    const unsigned char *src = raw + row * (size_t)J;
    unsigned *dst = packed + row * (size_t)(vld / 4);
    for (int w = threadIdx.x; w < vld / 4; w += 256) {
        unsigned v = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int d = 4 * w + e;
            if (d < J && src[d])
                v |= 0xFFu << (8 * e);
        }
        dst[w] = v;
    }
}

// vp: the packed validity rows of the slice (row s - s0 at vp + (s - s0) * vld; ONE: the one row every sample shares).
// ONE: the mask does not depend on the row, so it is applied to BOTH operands when a K-chunk is staged (x' = valid ? x : +0,
// m' = valid ? m : +0, hence m' - x' = +0 at an invalid column and the untouched m - x at a valid one): the inner loop is
// the unmasked tile's, and there is no validity tile -- each thread loads the dword of its 4 staged columns per K-chunk.
template <bool ONE>
__global__ __launch_bounds__(256, 2) void masked_tile_kernel(DistArgs a, const unsigned char *__restrict__ vp, int vld,
                                                             int s0, int s1, int N, int G, const u64 *__restrict__ hits,
                                                             u64 min_hits, u64 *__restrict__ part,
                                                             unsigned char *__restrict__ nan0)
{
    constexpr int TI = 4;
    constexpr int TS = 16 * TI;                 // samples per tile
    constexpr int NX = TS * 8 / 256;            // float4 of a sample operand per thread and K-chunk
    __shared__ __attribute__((aligned(16))) float sx[TILE * LDT];
    __shared__ __attribute__((aligned(16))) float sm[TILE * LDT];
    __shared__ __attribute__((aligned(16))) int sv[ONE ? 4 : TS * MSK_LDV];     // the validity tile, bytes (ONE: unused)
    __shared__ u64 sbest[TS * 16];              // every thread's smallest qualifying key of its 4 rows so far (kept out of
                                                // the registers the distance tile needs)

    const int tid0 = threadIdx.x;
    const int sbase0 = s0 + blockIdx.y * TS;
    const int L = a.L, L8 = L & ~7;
    const int nchunks = (L + VSOM_TK - 1) / VSOM_TK;

#pragma unroll
    for (int i = 0; i < TI; ++i)
        sbest[tid0 + 256 * i] = ~0ull;          // (a slot has one owner: no barrier until the final reduction)

    for (int t = 0; t < G; ++t) {
        const int nbase = (blockIdx.x * G + t) * TILE;
        if (nbase >= N)
            break;                              // (workgroup-uniform)
        if (t > 0)
            __syncthreads();                    // the previous tile's remainder pass is done with the last chunk
        // opaque per tile: the tile's addresses are formed anew instead of hoisted out of the tile loop (held across the
        // distance tile, they cost scratch)
        int tid = tid0, sbase = sbase0;
        asm volatile("" : "+v"(tid));
        asm volatile("" : "+s"(sbase));
        const int tx = tid & 15, ty = tid >> 4;
        // this thread stages 8 validity bytes per K-chunk (ONE: fetches the 4 bytes of the columns it stages)
        const bool vload = ONE || sbase + (tid >> 2) < s1;
        const unsigned char *vsrc = vp + (ONE ? (tid & 7) * 4 : (size_t)(sbase + (tid >> 2) - s0) * vld + (tid & 3) * 8);

        float acc[TI][4][8];
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    acc[i][j][k] = 0.f;

        float4 gx[NX], gm[2];
        uint2 gv;
        auto gload = [&](int k0) {
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                int f = tid + 256 * i;
                int row = f >> 3, c4 = (f & 7) * 4;
                int s = sbase + row;
                gx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (s < s1)
                    gx[i] = *reinterpret_cast<const float4 *>(a.xa + (size_t)s * a.ldx + k0 + c4);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int f = tid + 256 * i;
                int row = f >> 3, c4 = (f & 7) * 4;
                int n = nbase + row;
                gm[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (n < N)
                    gm[i] = *reinterpret_cast<const float4 *>(a.ma + (size_t)n * a.ldm + k0 + c4);
            }
            gv = make_uint2(0u, 0u);
            if (ONE)
                gv.x = *reinterpret_cast<const unsigned *>(vsrc + k0);
            else if (vload)
                gv = *reinterpret_cast<const uint2 *>(vsrc + k0);
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
                *reinterpret_cast<float4 *>(&sx[row * LDT + c4]) = ONE ? masked_sel4(gx[i], (int)gv.x) : gx[i];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int f = tid + 256 * i;
                int row = f >> 3, c4 = (f & 7) * 4;
                *reinterpret_cast<float4 *>(&sm[row * LDT + c4]) = ONE ? masked_sel4(gm[i], (int)gv.x) : gm[i];
            }
            if (!ONE)
                *reinterpret_cast<uint2 *>(&sv[tid * 2]) = gv;     // row tid >> 2, bytes 8 * (tid & 3) ..
            __syncthreads();
            if (ch + 1 < nchunks)
                gload(dk + VSOM_TK);
#pragma unroll
            for (int kk = 0; kk < VSOM_TK; kk += 8) {
                if (dk + kk < L8) {   // whole 8-blocks only; the remainder is handled in Eigen's order below
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        float4 xv[TI], mv[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            mv[j] = *reinterpret_cast<const float4 *>(&sm[(tx + 16 * j) * LDT + kk + 4 * h]);
#pragma unroll
                        for (int i = 0; i < TI; ++i)
                            xv[i] = *reinterpret_cast<const float4 *>(&sx[(ty + 16 * i) * LDT + kk + 4 * h]);
#pragma unroll
                        for (int i = 0; i < TI; ++i) {
                            // the row's 4 validity bytes -> 0 / ~0 per column (ONE: the operands are masked already)
                            const int w = ONE ? 0 : sv[(ty + 16 * i) * MSK_LDV + (kk >> 2) + h];
                            const int m[4] = {(int)((unsigned)w << 24) >> 24, (int)((unsigned)w << 16) >> 24,
                                              (int)((unsigned)w << 8) >> 24, w >> 24};
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                float r0 = masked_sel<!ONE>(vsom_resid<false>(xv[i].x, 0.f, mv[j].x, 0.f), m[0]);
                                float r1 = masked_sel<!ONE>(vsom_resid<false>(xv[i].y, 0.f, mv[j].y, 0.f), m[1]);
                                float r2 = masked_sel<!ONE>(vsom_resid<false>(xv[i].z, 0.f, mv[j].z, 0.f), m[2]);
                                float r3 = masked_sel<!ONE>(vsom_resid<false>(xv[i].w, 0.f, mv[j].w, 0.f), m[3]);
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

        // reduction tree + remainder (the last chunk is still in LDS); the thread's best qualifying key per row
        const int rem = L - L8;
        const int roff = L8 - (nchunks - 1) * VSOM_TK;   // column of element L8 inside the last chunk
        const signed char *svb = reinterpret_cast<const signed char *>(sv);
#pragma unroll
        for (int i = 0; i < TI; ++i) {
            u64 best = sbest[tid + 256 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float q0 = acc[i][j][0] + acc[i][j][4];
                float q1 = acc[i][j][1] + acc[i][j][5];
                float q2 = acc[i][j][2] + acc[i][j][6];
                float q3 = acc[i][j][3] + acc[i][j][7];
                const int xr = (ty + 16 * i) * LDT + roff, mr = (tx + 16 * j) * LDT + roff;
                const int vr = ONE ? 0 : (ty + 16 * i) * VSOM_TK + roff;
                int e = 0;
                if (rem >= 4) {
                    float r0 = masked_sel<!ONE>(vsom_resid<false>(sx[xr + 0], 0.f, sm[mr + 0], 0.f), (int)svb[vr + 0]);
                    float r1 = masked_sel<!ONE>(vsom_resid<false>(sx[xr + 1], 0.f, sm[mr + 1], 0.f), (int)svb[vr + 1]);
                    float r2 = masked_sel<!ONE>(vsom_resid<false>(sx[xr + 2], 0.f, sm[mr + 2], 0.f), (int)svb[vr + 2]);
                    float r3 = masked_sel<!ONE>(vsom_resid<false>(sx[xr + 3], 0.f, sm[mr + 3], 0.f), (int)svb[vr + 3]);
                    float p0 = r0 * r0, p1 = r1 * r1, p2 = r2 * r2, p3 = r3 * r3;
                    q0 = q0 + p0;
                    q1 = q1 + p1;
                    q2 = q2 + p2;
                    q3 = q3 + p3;
                    e = 4;
                }
                float t02 = q0 + q2, t13 = q1 + q3;
                float res = t02 + t13;
                for (; e < rem; ++e) {
                    float r = masked_sel<!ONE>(vsom_resid<false>(sx[xr + e], 0.f, sm[mr + e], 0.f), (int)svb[vr + e]);
                    float p = r * r;
                    res = res + p;
                }
                // findRestrictedBmu (Som.cpp:316-322): node 0 seeds unconditionally, the others need the hits -- honoured
                // here, so that a node without them cannot shadow a qualifying one of its group
                const int n = nbase + tx + 16 * j;
                const bool allowed = n < N && (n == 0 || hits[n] >= min_hits);
                const u64 k = allowed ? vsom_key(res, (uint32_t)n) : ~0ull;
                best = k < best ? k : best;
                // node 0's NaN flag: `cur < NaN` is never true, so a NaN at node 0 pins the BMU to 0 (Som.cpp:314-322)
                if (j == 0 && n == 0) {
                    const int s = sbase + ty + 16 * i;
                    if (s < s1)
                        nan0[s - s0] = res != res;
                }
            }
            sbest[tid + 256 * i] = best;
        }
    }

    __syncthreads();
    if (tid0 < TS) {
        const int tid = tid0;
        const int s = sbase0 + tid;
        if (s < s1) {
            u64 kmin = ~0ull;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const u64 k = sbest[tid * 16 + t];
                kmin = k < kmin ? k : kmin;
            }
            part[(size_t)(s - s0) * gridDim.x + blockIdx.x] = kmin;
        }
    }
}

// One wavefront per row of the slice (4 per workgroup): lane g holds the key of node group g.  dist: a NaN distance is
// stored as 0x7FC00000, the quiet NaN vsom_bmu_batch's sqres holds.
__global__ __launch_bounds__(256) void masked_reduce_kernel(const u64 *__restrict__ part, int ng,
                                                            const unsigned char *__restrict__ nan0,
                                                            const unsigned *__restrict__ packed, int vld, int one, int rows,
                                                            u64 *__restrict__ bmu, float *__restrict__ dist,
                                                            unsigned *__restrict__ nvalid)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows)
        return;                                 // (wavefront-uniform)
    u64 key = lane < ng ? part[(size_t)row * ng + lane] : ~0ull;
    const unsigned *v = packed + (one ? 0 : (size_t)row * (vld / 4));
    unsigned cnt = 0;
    for (int w = lane; w < vld / 4; w += 64)
        cnt += __popc(v[w] & 0x01010101u);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const u64 o = __shfl_xor(key, m);
        key = o < key ? o : key;
        cnt += __shfl_xor(cnt, m);
    }
    if (lane == 0) {
        if (nan0[row]) {
            bmu[row] = 0;
            dist[row] = __uint_as_float(0x7FC00000u);
        } else {
            bmu[row] = key & 0xFFFFFFFFull;
            dist[row] = __uint_as_float((uint32_t)(key >> 32));
        }
        nvalid[row] = cnt;
    }
}

// fill[row * J + d] = the bits of x[s0 + row][d] where valid, of map[bmu[row]][d] where not
__global__ __launch_bounds__(256) void masked_fill_kernel(const unsigned *__restrict__ x, int ldx,
                                                          const unsigned *__restrict__ map, int ldm,
                                                          const u64 *__restrict__ bmu,
                                                          const unsigned char *__restrict__ packed, int vld, int one, int s0,
                                                          int J, unsigned *__restrict__ fill)
{
    const int row = blockIdx.x, d = blockIdx.y * 256 + threadIdx.x;
    if (d >= J)
        return;
    const bool valid = packed[(one ? 0 : (size_t)row * vld) + d] != 0;
    fill[(size_t)row * J + d] = valid ? x[(size_t)(s0 + row) * ldx + d] : map[(size_t)bmu[row] * ldm + d];
}

// Rows per slice.  Per row of a slice the scratch holds J raw and xpitch packed validity bytes, at most MSK_MAXG keys,
// 17 bytes of results and, with fill, J floats: a slice stays within 64 MiB (one row, where one row alone needs more).
// VSOM_MASKED_SLICE_ROWS (development, read at every call) forces a smaller slice so that tests cross slice boundaries
// on small chunks.
static size_t vsom_masked_slice_rows(const vsom_ctx *c, bool fill)
{
    const size_t per_row = (size_t)c->J + c->xpitch + MSK_MAXG * 8 + 17 + (fill ? (size_t)c->J * 4 : 0);
    size_t s = std::max<size_t>(1, MSK_SCRATCH / per_row);
    if (const char *e = std::getenv("VSOM_MASKED_SLICE_ROWS")) {
        const long v = std::atol(e);
        if (v > 0 && (size_t)v < s)
            s = (size_t)v;
    }
    return s;
}

int launch_masked(vsom_ctx *c, u64 min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask,
                  const vsom_masked_out *out)
{
    TimerScope ts(c, VSOM_T_BMU);
    const size_t N = c->N, J = c->J, vld = c->xpitch, rows = r1 - r0;
    if (rows == 0)
        return VSOM_OK;
    const bool one = one_mask != 0;
    const size_t slice = std::min(vsom_masked_slice_rows(c, out->fill != nullptr), rows);
    const size_t ntiles = (N + TILE - 1) / TILE;
    // node groups: enough workgroups to fill the chip (2048: four rounds of two per CU) and at most MSK_MAXG keys per row
    // to reduce; G consecutive node tiles per group
    const size_t rtiles = (slice + TILE - 1) / TILE;
    const size_t want = std::min<size_t>({(size_t)MSK_MAXG, ntiles, std::max<size_t>(1, (2048 + rtiles - 1) / rtiles)});
    const size_t G = (ntiles + want - 1) / want, ng = (ntiles + G - 1) / G;
    const size_t vrows = one ? 1 : slice;
    // grow-only: a member keeps what it has when this call needs less
    VSOM_ALLOC_CHECK(vsom_grow_set(
        c->stream, VSOM_BUF_SYNC,
        {vsom_member(c->msk_raw, std::max(c->msk_raw.cap, vrows * J)), vsom_member(c->msk_valid, std::max(c->msk_valid.cap, vrows * vld)),
         vsom_member(c->msk_part, std::max(c->msk_part.cap, slice * ng)), vsom_member(c->msk_bmu, std::max(c->msk_bmu.cap, slice)),
         vsom_member(c->msk_dist, std::max(c->msk_dist.cap, slice)), vsom_member(c->msk_nvalid, std::max(c->msk_nvalid.cap, slice)),
         vsom_member(c->msk_nan0, std::max(c->msk_nan0.cap, slice)),
         vsom_member(c->msk_fill, std::max(c->msk_fill.cap, out->fill ? slice * J : 0))}));

    DistArgs a;
    a.xa = c->Xs.p;
    a.xb = c->Xs.p;
    a.ldx = (int)c->xpitch;
    a.ma = c->map.p;
    a.mb = c->map.p;
    a.ldm = (int)c->pitch;
    a.L = (int)c->part_len;
    unsigned *packed = reinterpret_cast<unsigned *>(c->msk_valid.p);
    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0, off = s0 - r0;
        if (!one || s0 == r0) {     // (a column mask is packed once)
            const size_t vr = one ? 1 : n;
            VSOM_HIP_CHECK(hipMemcpyAsync(c->msk_raw.p, valid_host + (one ? 0 : off * J), vr * J, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(masked_pack_kernel, dim3((unsigned)vr), dim3(256), 0, c->stream, c->msk_raw.p, (int)J, (int)vld,
                               packed);
        }
        dim3 grid((unsigned)ng, (unsigned)((n + TILE - 1) / TILE));
        if (one)
            hipLaunchKernelGGL(masked_tile_kernel<true>, grid, dim3(256), 0, c->stream, a, c->msk_valid.p, (int)vld, (int)s0,
                               (int)s1, (int)N, (int)G, c->hits.p, min_hits, c->msk_part.p, c->msk_nan0.p);
        else
            hipLaunchKernelGGL(masked_tile_kernel<false>, grid, dim3(256), 0, c->stream, a, c->msk_valid.p, (int)vld, (int)s0,
                               (int)s1, (int)N, (int)G, c->hits.p, min_hits, c->msk_part.p, c->msk_nan0.p);
        hipLaunchKernelGGL(masked_reduce_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, c->msk_part.p, (int)ng,
                           c->msk_nan0.p, packed, (int)vld, (int)one, (int)n, c->msk_bmu.p, c->msk_dist.p, c->msk_nvalid.p);
        if (out->fill)
            hipLaunchKernelGGL(masked_fill_kernel, dim3((unsigned)n, (unsigned)((J + 255) / 256)), dim3(256), 0, c->stream,
                               reinterpret_cast<const unsigned *>(c->Xs.p), (int)c->xpitch,
                               reinterpret_cast<const unsigned *>(c->map.p), (int)c->pitch, c->msk_bmu.p, c->msk_valid.p, (int)vld,
                               (int)one, (int)s0, (int)J, reinterpret_cast<unsigned *>(c->msk_fill.p));
        VSOM_HIP_CHECK(hipGetLastError());
        if (out->bmu)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->bmu + off, c->msk_bmu.p, n * 8, hipMemcpyDeviceToHost, c->stream));
        if (out->dist)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->dist + off, c->msk_dist.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->nvalid)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->nvalid + off, c->msk_nvalid.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->fill)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->fill + off * J, c->msk_fill.p, n * J * 4, hipMemcpyDeviceToHost, c->stream));
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}
