// vsom_topk.hip -- the k best matching units of every chunk row in [r0, r1): the k smallest keys vsom_key(d_i, i) over
// every node, with findBmu's node-0 rule in front (Som.cpp:291-309) (gfx950).
//
//  topk_tile_kernel  : the shared distance tile (vsom_dist_tile.hpp: 64 (CLR: 32) rows x 64 nodes per tile, 8 class
//                      accumulators + Eigen's reduction tree, the exact search's operations in its order), walked over G
//                      consecutive node tiles per workgroup.  Every row keeps a sorted list of its k smallest keys in LDS;
//                      after each tile the keys below the row's k-th key are merged into it by rank (position = rank in
//                      the list + rank among the accepted keys: keys are unique, so positions are), and at the end the
//                      workgroup stores k keys per row for its node group.  It also flags the rows whose d_0 is NaN.
//  topk_merge_kernel : one wavefront per row selects the k smallest keys of the node groups' sorted lists (staged in LDS;
//                      lane g holds the head of list g), applies the node-0 rule and stores idx (u64) and the distance
//                      row-major.  Where the heads run out before k entries (the masked call under min_hits) it pads.
// vsom_bmu_topk_masked_batch runs the same two kernels over the VALID columns, the tile walk with a mask policy of the
// distance tile (VsomMaskRows / VsomMaskOne) and findRestrictedBmu's candidates (node 0, or bmuHits >= min_hits), and
//  topk_blend_kernel : one wavefront per row: the record imputed from the row's k units, weighted as the BMD weights
//                      units (q_j = exp(-(d_j^2 - d_first^2) / 2) in double), x itself at the valid columns.
#include "vsom_dist_tile.hpp"
#include <algorithm>
#include <type_traits>

#define TOPK_KMAX 64       // largest k (vsom_bmu_topk_batch refuses more)
#define TOPK_MAXG 64       // node groups per row at most: one merge lane each
#define TOPK_NONE (~0ull)  // above every key (a key's node is < 2^32 - 1)

// The list passes of one tile (every thread of the workgroup calls it): the keys the tile accepted for row lr (amask) are
// merged into the row's sorted list.  Kept out of line: inlined into the tile loop, it pushed the distance tile's
// registers into scratch.  One instantiation per mask policy, so that each has one caller: a function with one caller is
// compiled for that caller's LDS addresses; shared between the unmasked and the masked walks, topk_list_merge<64> grew by
// more than 200 instructions for all of them (663 as it is).
template <int TS, class Mask>
__device__ __attribute__((noinline)) void topk_list_merge(u64 (*top)[TOPK_KMAX + 1], float (*sd)[TILE + 1],
                                                          unsigned char (*cpos)[TILE], u64 *amask, u64 *omask, int lr,
                                                          int q, int k, int nbase)
{
    constexpr int Q = 256 / TS;
    // list pass 1: the merged position of each accepted key (this thread's share: accepted keys c = q, q + Q, ...)
    const u64 A = amask[lr];
    if (A) {
        u64 rest = A;
        for (int c = 0; rest; ++c, rest &= rest - 1) {
            if (c % Q != q)
                continue;
            const int nl = __ffsll((unsigned long long)rest) - 1;
            const u64 key = vsom_key(sd[lr][nl], (uint32_t)(nbase + nl));
            int lo = 0, hi = k;             // rank in the list
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (top[lr][mid] < key)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            int pos = lo;                   // + rank among the accepted keys (stops once out of the list)
            for (u64 o = A; o && pos < k; o &= o - 1) {
                const int ol = __ffsll((unsigned long long)o) - 1;
                pos += vsom_key(sd[lr][ol], (uint32_t)(nbase + ol)) < key;
            }
            cpos[lr][nl] = (unsigned char)(pos < k ? pos : 255);
            if (pos < k)
                atomicOr(&omask[lr], 1ull << pos);
        }
    }
    __syncthreads();
    // list pass 2: the list's own keys fill the positions the accepted keys left free, in order
    u64 keep[TOPK_KMAX / Q];
    const u64 O = omask[lr];
    if (A) {
#pragma unroll
        for (int i = 0; i < TOPK_KMAX / Q; ++i) {
            const int p = q + Q * i;
            if (p < k && !((O >> p) & 1))
                keep[i] = top[lr][p - __popcll(O & ((1ull << p) - 1))];
        }
    }
    __syncthreads();
    if (A) {
#pragma unroll
        for (int i = 0; i < TOPK_KMAX / Q; ++i) {
            const int p = q + Q * i;
            if (p < k && !((O >> p) & 1))
                top[lr][p] = keep[i];
        }
        u64 rest = A;
        for (int c = 0; rest; ++c, rest &= rest - 1) {
            if (c % Q != q)
                continue;
            const int nl = __ffsll((unsigned long long)rest) - 1;
            const int pos = cpos[lr][nl];
            if (pos < k)
                top[lr][pos] = vsom_key(sd[lr][nl], (uint32_t)(nbase + nl));
        }
    }
}

// What the masked walk takes beside the unmasked one's arguments: the packed validity rows of the slice (vld bytes each,
// 0xFF = valid; row s - s0 at vp + (s - s0) * vld, VsomMaskOne: the one row every sample shares) and the hit restriction.
// Nothing for VsomMaskNone.
template <class Mask> struct TopkMaskSrc {
    const unsigned char *vp;
    int vld;
    const u64 *hits;
    u64 min_hits;
};
template <> struct TopkMaskSrc<VsomMaskNone> {
};

// Mask = VsomMaskRows / VsomMaskOne (Standard / Median): the distance over the VALID columns, r_d = valid ? m_d - x_d : +0
// by select -- the distance of masked_tile_kernel (vsom_masked.hip) -- and findRestrictedBmu's candidates only
template <bool CLR, int TI, class Mask = VsomMaskNone>
__global__ __launch_bounds__(256, 2) void topk_tile_kernel(DistArgs a, int s0, int s1, int N, int k, int G,
                                                           u64 *__restrict__ part, unsigned char *__restrict__ nan0,
                                                           TopkMaskSrc<Mask> ms)
{
    constexpr bool MASKED = !std::is_same<Mask, VsomMaskNone>::value;
    constexpr int TS = 16 * TI;                 // samples per tile
    constexpr int Q = 256 / TS;                 // threads per row in the list passes
    __shared__ float sd[TS][TILE + 1];          // the tile's distances
    __shared__ u64 top[TS][TOPK_KMAX + 1];      // each row's k smallest keys so far, ascending (padded against bank aliasing)
    __shared__ unsigned char cpos[TS][TILE];    // merged position of an accepted key (255: out of the list)
    __shared__ u64 amask[TS], omask[TS];        // accepted tile nodes / list positions they take

    const int tid0 = threadIdx.x;
    const int lr = tid0 % TS, q = tid0 / TS;      // list passes: row lr, share q of Q
    const int sbase0 = s0 + blockIdx.y * TS;

    for (int j = q; j < k; j += Q)
        top[lr][j] = TOPK_NONE;
    if (q == 0)
        amask[lr] = omask[lr] = 0;

    for (int t = 0; t < G; ++t) {
        const int nbase = (blockIdx.x * G + t) * TILE;
        if (nbase >= N)
            break;                              // (workgroup-uniform)
        __syncthreads();                        // the previous tile's list passes are done with sd / top / the masks
        // opaque per tile: the tile's addresses are formed anew instead of hoisted out of the tile loop (held across the
        // list passes, they cost scratch)
        int tid = tid0, sbase = sbase0;
        asm volatile("" : "+v"(tid));
        asm volatile("" : "+s"(sbase));
        const int tx = tid & 15, ty = tid >> 4;

        const Mask mask = [&] {
            if constexpr (MASKED)
                return Mask(ms.vp, ms.vld, tid, sbase, s0, s1);
            else
                return VsomMaskNone();
        }();
        vsom_dist_tile<CLR, TI>(a, tid, sbase, s1, nbase, N, mask,
                                [&](int i, int j, float res) { sd[ty + 16 * i][tx + 16 * j] = res; });
        __syncthreads();

        // accept: the keys below the row's current k-th key (this thread's share of the row: nodes q, q + Q, ...)
        {
            const u64 kth = top[lr][k - 1];
            u64 mine = 0;
            for (int nl = q; nl < TILE && nbase + nl < N; nl += Q) {
                if constexpr (MASKED) {
                    // findRestrictedBmu (Som.cpp:316-322): node 0 seeds unconditionally, the others need the hits
                    const int n = nbase + nl;
                    if (n != 0 && ms.hits[n] < ms.min_hits)
                        continue;
                }
                if (vsom_key(sd[lr][nl], (uint32_t)(nbase + nl)) < kth)
                    mine |= 1ull << nl;
            }
            if (mine)
                atomicOr(&amask[lr], mine);
            if (nbase == 0 && q == 0 && sbase0 + lr < s1)
                nan0[sbase0 + lr - s0] = sd[lr][0] != sd[lr][0];
        }
        __syncthreads();

        topk_list_merge<TS, Mask>(top, sd, cpos, amask, omask, lr, q, k, nbase);
        if (q == 0)
            amask[lr] = omask[lr] = 0;          // (every reader of A / O is past the barrier above)
    }
    __syncthreads();
    const int s = sbase0 + lr;
    if (s < s1) {
        u64 *dst = part + ((size_t)(s - s0) * gridDim.x + blockIdx.x) * k;
        for (int j = q; j < k; j += Q)
            dst[j] = top[lr][j];
    }
}

// One wavefront per row of the slice: the row's ng sorted lists of k keys are staged in LDS (ng * k <= 4096 keys), lane g
// holds the head of list g, and every round takes the wavefront's smallest head.  The node-0 rule: when d_0 is NaN, node 0
// comes first and is skipped where the lists hold it.  dist: NULL = not wanted; a NaN distance is stored as 0x7FC00000,
// the quiet NaN vsom_bmu_batch's sqres holds.  A row whose lists hold fewer than k keys (the masked walk under min_hits)
// is padded: idx = UINT64_MAX, dist = 0x7FC00000 from entry count on.  count: NULL = not wanted.  packed: NULL, or the
// slice's packed validity rows (vld bytes each; one: the row every sample shares) counted into nvalid.
__global__ __launch_bounds__(64) void topk_merge_kernel(const u64 *__restrict__ part, const unsigned char *__restrict__ nan0,
                                                        int ng, int k, u64 *__restrict__ idx, float *__restrict__ dist,
                                                        unsigned *__restrict__ count, const unsigned *__restrict__ packed,
                                                        int vld, int one, unsigned *__restrict__ nvalid)
{
    extern __shared__ u64 lists[];
    const int row = blockIdx.x, lane = threadIdx.x;
    const u64 *src = part + (size_t)row * ng * k;
    for (int e = lane; e < ng * k; e += 64)
        lists[e] = src[e];
    __syncthreads();
    const bool nan_first = nan0[row] != 0;
    const u64 key0 = (u64)0xFFFFFFFFu << 32;    // vsom_key(NaN, 0)
    int ptr = 0;
    u64 head = lane < ng ? lists[lane * k] : TOPK_NONE;
    u64 mine = TOPK_NONE;                       // entry `lane` of the result
    int cnt = 0;
    if (nan_first) {
        if (lane == 0)
            mine = key0;
        cnt = 1;
    }
    // (unmasked, k <= N: the lists hold the k smallest keys, so every counted round takes a real key; every round consumes
    // one key.  Masked: the candidates may be fewer than k -- the heads run out and the rest of the row is padding)
    while (cnt < k) {
        const u64 m = vsom_wave_min(head);
        if (m == TOPK_NONE)
            break;                              // (wavefront-uniform) every head is spent
        if (head == m) {                        // real keys are unique: one lane
            ++ptr;
            head = ptr < k ? lists[lane * k + ptr] : TOPK_NONE;
        }
        if (nan_first && m == key0)
            continue;
        if (lane == cnt)
            mine = m;
        ++cnt;
    }
    if (lane < k) {
        const uint32_t bits = (uint32_t)(mine >> 32);
        idx[(size_t)row * k + lane] = mine == TOPK_NONE ? TOPK_NONE : mine & 0xFFFFFFFFull;
        if (dist)
            dist[(size_t)row * k + lane] = __uint_as_float(bits == 0xFFFFFFFFu ? 0x7FC00000u : bits);
    }
    if (count && lane == 0)
        count[row] = (unsigned)cnt;
    if (packed) {
        const unsigned *v = packed + (one ? 0 : (size_t)row * (vld / 4));
        unsigned nv = 0;
        for (int w = lane; w < vld / 4; w += 64)
            nv += __popc(v[w] & 0x01010101u);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
            nv += __shfl_xor(nv, m);
        if (lane == 0)
            nvalid[row] = nv;
    }
}

// The record imputed from the k units of a row, one wavefront per slice row.  Lane j forms q_j from the row's stored
// distance, in double: a_j = (double)d_j * (double)d_j, t = the a of the first entry whose distance is not NaN (entry 0, or
// entry 1 under the node-0 rule), q_j = exp(-(a_j - t) / 2) for a finite d_j and 0 otherwise; the row has mass iff that
// first entry exists and is finite.  The (unit, q) pairs go to LDS, then lane = column: every lane walks the entries in list
// order, Q = ((0 + q_0) + q_1) + ... and num_d = ((0 + q_0 * m[0][d]) + q_1 * m[1][d]) + ..., the terms with q_j == 0
// skipped (not multiplied: an inf or NaN model entry of such a unit has no effect); consecutive lanes read consecutive
// columns of one model row.  blend[row][d] = (double)x at a valid column (a select), num_d / Q at an invalid one, the
// quiet NaN where the row has no mass.  Nothing is contracted (csrc/build.sh: -ffp-contract=off).
__global__ __launch_bounds__(64) void topk_blend_kernel(const u64 *__restrict__ idx, const float *__restrict__ dist,
                                                        const unsigned *__restrict__ count, int k,
                                                        const float *__restrict__ x, int ldx, const float *__restrict__ map,
                                                        int ldm, const unsigned char *__restrict__ packed, int vld, int one,
                                                        int s0, int J, double *__restrict__ blend)
{
    __shared__ double sq[TOPK_KMAX];
    __shared__ unsigned sn[TOPK_KMAX];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int cnt = (int)count[row];            // <= k <= TOPK_KMAX
    const bool real = lane < cnt;
    const float d = real ? dist[(size_t)row * k + lane] : 0.f;
    const double a = (double)d * (double)d;
    const u64 notnan = __ballot(real && d == d);
    const int first = notnan ? __ffsll((unsigned long long)notnan) - 1 : 0;
    const double t = __shfl(a, first);
    const float dfirst = __shfl(d, first);
    const bool mass = notnan != 0 && __builtin_isfinite(dfirst);
    double qj = 0.0;
    if (real && __builtin_isfinite(d))
        qj = exp(-(a - t) / 2);
    sq[lane] = qj;
    sn[lane] = real ? (unsigned)idx[(size_t)row * k + lane] : 0u;
    __syncthreads();
    double Q = 0.0;
    for (int j = 0; j < cnt; ++j)
        if (sq[j] != 0.0)
            Q = Q + sq[j];
    const unsigned char *v = packed + (one ? 0 : (size_t)row * vld);
    const float *xr = x + (size_t)(s0 + row) * ldx;
    for (int c = lane; c < J; c += 64) {
        double out;
        if (v[c]) {
            out = (double)xr[c];
        } else if (!mass) {
            out = __longlong_as_double(0x7FF8000000000000ll);
        } else {
            double num = 0.0;
            for (int j = 0; j < cnt; ++j) {
                const double w = sq[j];
                if (w != 0.0)
                    num = num + w * (double)map[(size_t)sn[j] * ldm + c];
            }
            out = num / Q;
        }
        blend[(size_t)row * J + c] = out;
    }
}

// rows per slice: the partial lists of a slice (at most TOPK_MAXG groups of k keys per row) stay within 64 MiB
static size_t vsom_topk_slice_rows(uint32_t k)
{
    return ((size_t)64 << 20) / ((size_t)TOPK_MAXG * k * 8);
}

int launch_topk(vsom_ctx *c, uint32_t k, size_t r0, size_t r1, uint64_t *idx_out, float *dist_out)
{
    TimerScope ts(c, VSOM_T_BMU);
    const size_t N = c->N, rows = r1 - r0;
    if (rows == 0)
        return VSOM_OK;
    const size_t slice = std::min(vsom_topk_slice_rows(k), rows);
    const int TS = c->transform == VSOM_CLR ? 32 : TILE;
    // node groups: at most TOPK_MAXG lists per row to merge
    const VsomNodeGroups grp = vsom_node_groups((N + TILE - 1) / TILE, (slice + TS - 1) / TS, TOPK_MAXG);
    const size_t G = grp.G, ng = grp.ng;
    // every node group's k keys per row of a slice, the slice's idx / dist and its node-0 NaN flags
    vsom_layout lay;
    const auto part = lay.add<u64>(slice * ng * k), idx = lay.add<u64>(slice * k);
    const auto dist = lay.add<float>(dist_out ? slice * k : 0);
    const auto nan0 = lay.add<unsigned char>(slice);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    const DistArgs a = vsom_dist_args(c);
    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0, off = s0 - r0;
        dim3 grid((unsigned)ng, (unsigned)((n + TS - 1) / TS));
        if (c->transform == VSOM_CLR)
            hipLaunchKernelGGL((topk_tile_kernel<true, 2>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1, (int)N,
                               (int)k, (int)G, lay.at(part), lay.at(nan0), TopkMaskSrc<VsomMaskNone>{});
        else
            hipLaunchKernelGGL((topk_tile_kernel<false, 4>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1, (int)N,
                               (int)k, (int)G, lay.at(part), lay.at(nan0), TopkMaskSrc<VsomMaskNone>{});
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)n), dim3(64), ng * k * 8, c->stream, lay.at(part),
                           lay.at(nan0), (int)ng, (int)k, lay.at(idx), dist_out ? lay.at(dist) : nullptr,
                           (unsigned *)nullptr, (const unsigned *)nullptr, 0, 0, (unsigned *)nullptr);
        VSOM_HIP_CHECK(hipGetLastError());
        VSOM_HIP_CHECK(hipMemcpyAsync(idx_out + off * k, lay.at(idx), n * k * 8, hipMemcpyDeviceToHost, c->stream));
        if (dist_out)
            VSOM_HIP_CHECK(hipMemcpyAsync(dist_out + off * k, lay.at(dist), n * k * 4, hipMemcpyDeviceToHost, c->stream));
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

// vsom_bmu_topk_masked_batch.  A slice is the smallest of the top-k rule (the partial lists within 64 MiB), the masked
// search's validity rule (VSOM_MASKED_SLICE_ROWS honoured) and, with blend, 64 MiB / (8 J) rows -- one row where a single
// row needs more.  Tile and merge are timed under VSOM_T_BMU, the blend under VSOM_T_FINISH.
int launch_topk_masked(vsom_ctx *c, uint32_t k, u64 min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask,
                       const vsom_topk_masked_out *out)
{
    const size_t N = c->N, J = c->J, vld = c->xpitch, rows = r1 - r0;
    if (rows == 0)
        return VSOM_OK;
    size_t slice = std::min({vsom_topk_slice_rows(k), vsom_masked_search_slice_rows(c), rows});
    if (out->blend)
        slice = std::min(slice, ((size_t)64 << 20) / (8 * std::max<size_t>(J, 1)));
    slice = std::max<size_t>(slice, 1);
    const VsomNodeGroups grp = vsom_node_groups((N + TILE - 1) / TILE, (slice + TILE - 1) / TILE, TOPK_MAXG);
    const size_t G = grp.G, ng = grp.ng;
    const bool want_dist = out->dist || out->blend;
    // every node group's k keys per row of a slice, the slice's idx / dist / count / nvalid and its node-0 NaN flags, its
    // validity bytes as given and packed, its imputed rows
    vsom_layout lay;
    const auto part = lay.add<u64>(slice * ng * k), idx = lay.add<u64>(slice * k);
    const auto dist = lay.add<float>(want_dist ? slice * k : 0);
    const auto count = lay.add<unsigned>(slice), nvalid = lay.add<unsigned>(slice);
    const auto nan0 = lay.add<unsigned char>(slice);
    const auto blend = lay.add<double>(out->blend ? slice * J : 0);
    const VsomBmdMask mask = vsom_bmd_mask_add(c, lay, valid_host, one_mask != 0, slice);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    const DistArgs a = vsom_dist_args(c);     // (Standard / Median: the rows themselves)
    const unsigned char *vp = lay.at(mask.packed);
    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0, off = s0 - r0;
        {
            TimerScope ts(c, VSOM_T_BMU);
            if (int rc = vsom_bmd_mask_slice_enqueue(c, lay, mask, r0, s0, s1, valid_host))
                return rc;
            dim3 grid((unsigned)ng, (unsigned)((n + TILE - 1) / TILE));
            if (mask.one)
                hipLaunchKernelGGL((topk_tile_kernel<false, 4, VsomMaskOne>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1,
                                   (int)N, (int)k, (int)G, lay.at(part), lay.at(nan0),
                                   TopkMaskSrc<VsomMaskOne>{vp, (int)vld, c->hits.p, min_hits});
            else
                hipLaunchKernelGGL((topk_tile_kernel<false, 4, VsomMaskRows>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1,
                                   (int)N, (int)k, (int)G, lay.at(part), lay.at(nan0),
                                   TopkMaskSrc<VsomMaskRows>{vp, (int)vld, c->hits.p, min_hits});
            hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)n), dim3(64), ng * k * 8, c->stream, lay.at(part),
                               lay.at(nan0), (int)ng, (int)k, lay.at(idx), want_dist ? lay.at(dist) : nullptr, lay.at(count),
                               reinterpret_cast<const unsigned *>(vp), (int)vld, (int)mask.one, lay.at(nvalid));
            VSOM_HIP_CHECK(hipGetLastError());
        }
        if (out->blend) {
            TimerScope ts(c, VSOM_T_FINISH);
            hipLaunchKernelGGL(topk_blend_kernel, dim3((unsigned)n), dim3(64), 0, c->stream, lay.at(idx), lay.at(dist),
                               lay.at(count), (int)k, c->Xs.p, (int)c->xpitch, c->map.p, (int)c->pitch, vp, (int)vld,
                               (int)mask.one, (int)s0, (int)J, lay.at(blend));
            VSOM_HIP_CHECK(hipGetLastError());
        }
        VSOM_HIP_CHECK(hipMemcpyAsync(out->idx + off * k, lay.at(idx), n * k * 8, hipMemcpyDeviceToHost, c->stream));
        if (out->dist)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->dist + off * k, lay.at(dist), n * k * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->count)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->count + off, lay.at(count), n * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->nvalid)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->nvalid + off, lay.at(nvalid), n * 4, hipMemcpyDeviceToHost, c->stream));
        if (out->blend)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->blend + off * J, lay.at(blend), n * J * 8, hipMemcpyDeviceToHost, c->stream));
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}
