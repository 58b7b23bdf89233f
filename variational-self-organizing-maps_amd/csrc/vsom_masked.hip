// vsom_masked.hip -- Som::findRestrictedBmu (Som.cpp:313-332) over the VALID columns of every chunk row in [r0, r1), the
// distance Som::euclidianWeightedDist documents (Som.cpp:112-141, the masked form of :139), and the imputed record
// (gfx950; Standard / Median).
//
//  masked_pack_kernel   : the caller's validity bytes (rows x J, or J with one_mask) -> rows of xpitch bytes, 0xFF = valid,
//                         0x00 = invalid or padding: aligned 8-byte loads for the tile, one sign extension per mask word
//  masked_tile_kernel   : the shared distance tile (vsom_dist_tile.hpp: 64 rows x 64 nodes, 8 class accumulators + Eigen's
//                         reduction tree, the exact search's operations in its order) with a validity tile staged in LDS
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
// (The mask policies themselves, VsomMaskRows and VsomMaskOne, live with the tile in vsom_dist_tile.hpp.)
#include "vsom_dist_tile.hpp"
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#define MSK_MAXG 64             // node groups per row at most: one reduce lane each
#define MSK_SCRATCH ((size_t)64 << 20)

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
// ONE selects the tile's mask policy: VsomMaskOne (the mask applied to both operands as a K-chunk is staged, the unmasked
// inner loop) or VsomMaskRows (a validity tile in LDS, a select on every residual).
template <bool ONE>
__global__ __launch_bounds__(256, 2) void masked_tile_kernel(DistArgs a, const unsigned char *__restrict__ vp, int vld,
                                                             int s0, int s1, int N, int G, const u64 *__restrict__ hits,
                                                             u64 min_hits, u64 *__restrict__ part,
                                                             unsigned char *__restrict__ nan0)
{
    constexpr int TI = 4;
    constexpr int TS = 16 * TI;                 // samples per tile
    __shared__ u64 sbest[TS * 16];              // every thread's smallest qualifying key of its 4 rows so far (kept out of
                                                // the registers the distance tile needs)

    const int tid0 = threadIdx.x;
    const int sbase0 = s0 + blockIdx.y * TS;

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
        const std::conditional_t<ONE, VsomMaskOne, VsomMaskRows> mask(vp, vld, tid, sbase, s0, s1);

        // the thread's best qualifying key per row
        u64 best = 0;
        vsom_dist_tile<false, TI>(a, tid, sbase, s1, nbase, N, mask, [&](int i, int j, float res) {
            if (j == 0)
                best = sbest[tid + 256 * i];
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
            if (j == 3)
                sbest[tid + 256 * i] = best;
        });
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
    key = vsom_wave_min(key);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        cnt += __shfl_xor(cnt, m);
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

// Rows of J validity bytes as the caller gives them -> rows of xpitch packed bytes (enqueues only)
void vsom_masked_pack_enqueue(vsom_ctx *c, const unsigned char *raw_dev, size_t rows, unsigned char *packed_dev)
{
    hipLaunchKernelGGL(masked_pack_kernel, dim3((unsigned)rows), dim3(256), 0, c->stream, raw_dev, (int)c->J, (int)c->xpitch,
                       reinterpret_cast<unsigned *>(packed_dev));
}

size_t vsom_masked_search_slice_rows(const vsom_ctx *c) { return vsom_masked_slice_rows(c, false); }

// node groups of a slice's tile walk: at most MSK_MAXG keys per row to reduce
VsomNodeGroups vsom_masked_groups(const vsom_ctx *c, size_t slice)
{
    return vsom_node_groups(((size_t)c->N + TILE - 1) / TILE, (slice + TILE - 1) / TILE, MSK_MAXG);
}

// The search of chunk rows [s0, s1) over the packed validity rows vp (row s - s0 at vp + (s - s0) * xpitch; one: the row
// every sample shares): tile walk and reduction, entry s - s0 of bmu / dist / nvalid (device) belongs to row s.  part holds
// (s1 - s0) * grp.ng keys, nan0 s1 - s0 bytes.  Enqueues only.
int vsom_masked_search_enqueue(vsom_ctx *c, u64 min_hits, size_t s0, size_t s1, const unsigned char *vp, bool one,
                               const VsomNodeGroups &grp, u64 *part, unsigned char *nan0, u64 *bmu, float *dist,
                               unsigned *nvalid)
{
    const size_t N = c->N, vld = c->xpitch, n = s1 - s0;
    const DistArgs a = vsom_dist_args(c);     // (Standard / Median: the rows themselves)
    dim3 grid((unsigned)grp.ng, (unsigned)((n + TILE - 1) / TILE));
    if (one)
        hipLaunchKernelGGL(masked_tile_kernel<true>, grid, dim3(256), 0, c->stream, a, vp, (int)vld, (int)s0, (int)s1, (int)N,
                           (int)grp.G, c->hits.p, min_hits, part, nan0);
    else
        hipLaunchKernelGGL(masked_tile_kernel<false>, grid, dim3(256), 0, c->stream, a, vp, (int)vld, (int)s0, (int)s1, (int)N,
                           (int)grp.G, c->hits.p, min_hits, part, nan0);
    hipLaunchKernelGGL(masked_reduce_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, part, (int)grp.ng, nan0,
                       reinterpret_cast<const unsigned *>(vp), (int)vld, (int)one, (int)n, bmu, dist, nvalid);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}

// The search scratch of one slice, for the callers that keep a slice's units on the device (launch_masked, the masked scorers)
VsomMaskedSearch vsom_masked_search_add(const vsom_ctx *c, vsom_layout &lay, bool one, size_t slice)
{
    VsomMaskedSearch ms;
    ms.one = one;
    ms.slice = slice;
    ms.grp = vsom_masked_groups(c, slice);
    const size_t vrows = one ? 1 : slice;
    ms.raw = lay.add<unsigned char>(vrows * c->J);
    ms.packed = lay.add<unsigned char>(vrows * c->xpitch);
    ms.nan0 = lay.add<unsigned char>(slice);
    ms.part = lay.add<u64>(slice * ms.grp.ng);
    ms.bmu = lay.add<u64>(slice);
    ms.dist = lay.add<float>(slice);
    ms.nvalid = lay.add<unsigned>(slice);
    return ms;
}

// Slice [s0, s1) of a call over [r0, ...): its validity bytes up and packed (a column mask once, with the first slice), then
// the search into ms.bmu / ms.dist / ms.nvalid.  Enqueues only.
int vsom_masked_slice_enqueue(vsom_ctx *c, const vsom_layout &lay, const VsomMaskedSearch &ms, u64 min_hits, size_t r0,
                              size_t s0, size_t s1, const uint8_t *valid_host)
{
    const size_t J = c->J;
    if (!ms.one || s0 == r0) {
        const size_t vr = ms.one ? 1 : s1 - s0;
        VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(ms.raw), valid_host + (ms.one ? 0 : (s0 - r0) * J), vr * J, hipMemcpyHostToDevice,
                                      c->stream));
        vsom_masked_pack_enqueue(c, lay.at(ms.raw), vr, lay.at(ms.packed));
    }
    return vsom_masked_search_enqueue(c, min_hits, s0, s1, lay.at(ms.packed), ms.one, ms.grp, lay.at(ms.part), lay.at(ms.nan0),
                                      lay.at(ms.bmu), lay.at(ms.dist), lay.at(ms.nvalid));
}

int launch_masked(vsom_ctx *c, u64 min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask,
                  const vsom_masked_out *out)
{
    TimerScope ts(c, VSOM_T_BMU);
    const size_t J = c->J, vld = c->xpitch, rows = r1 - r0;
    if (rows == 0)
        return VSOM_OK;
    const size_t slice = std::min(vsom_masked_slice_rows(c, out->fill != nullptr), rows);
    // a slice's validity bytes as given and packed (0xFF / 0x00, xpitch per row), node-group keys, results and imputed rows
    vsom_layout lay;
    const VsomMaskedSearch ms = vsom_masked_search_add(c, lay, one_mask != 0, slice);
    const auto fill = lay.add<float>(out->fill ? slice * J : 0);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));

    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0, off = s0 - r0;
        if (int rc = vsom_masked_slice_enqueue(c, lay, ms, min_hits, r0, s0, s1, valid_host))
            return rc;
        if (out->fill)
            hipLaunchKernelGGL(masked_fill_kernel, dim3((unsigned)n, (unsigned)((J + 255) / 256)), dim3(256), 0, c->stream,
                               reinterpret_cast<const unsigned *>(c->Xs.p), (int)c->xpitch,
                               reinterpret_cast<const unsigned *>(c->map.p), (int)c->pitch, lay.at(ms.bmu), lay.at(ms.packed),
                               (int)vld, (int)ms.one, (int)s0, (int)J, reinterpret_cast<unsigned *>(lay.at(fill)));
        VSOM_HIP_CHECK(hipGetLastError());
        if (out->bmu)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->bmu + off, lay.at(ms.bmu), n * 8, hipMemcpyDeviceToHost, c->stream));
        if (out->dist)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->dist + off, lay.at(ms.dist), n * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->nvalid)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->nvalid + off, lay.at(ms.nvalid), n * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->fill)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->fill + off * J, lay.at(fill), n * J * 4, hipMemcpyDeviceToHost, c->stream));
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}
