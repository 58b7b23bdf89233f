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
//                      row-major.
#include "vsom_dist_tile.hpp"
#include <algorithm>

#define TOPK_KMAX 64       // largest k (vsom_bmu_topk_batch refuses more)
#define TOPK_MAXG 64       // node groups per row at most: one merge lane each
#define TOPK_NONE (~0ull)  // above every key (a key's node is < 2^32 - 1)

// The list passes of one tile (every thread of the workgroup calls it): the keys the tile accepted for row lr (amask) are
// merged into the row's sorted list.  Kept out of line: inlined into the tile loop, it pushed the distance tile's
// registers into scratch.
template <int TS>
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

template <bool CLR, int TI>
__global__ __launch_bounds__(256, 2) void topk_tile_kernel(DistArgs a, int s0, int s1, int N, int k, int G,
                                                           u64 *__restrict__ part, unsigned char *__restrict__ nan0)
{
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

        vsom_dist_tile<CLR, TI>(a, tid, sbase, s1, nbase, N, VsomMaskNone(),
                                [&](int i, int j, float res) { sd[ty + 16 * i][tx + 16 * j] = res; });
        __syncthreads();

        // accept: the keys below the row's current k-th key (this thread's share of the row: nodes q, q + Q, ...)
        {
            const u64 kth = top[lr][k - 1];
            u64 mine = 0;
            for (int nl = q; nl < TILE && nbase + nl < N; nl += Q)
                if (vsom_key(sd[lr][nl], (uint32_t)(nbase + nl)) < kth)
                    mine |= 1ull << nl;
            if (mine)
                atomicOr(&amask[lr], mine);
            if (nbase == 0 && q == 0 && sbase0 + lr < s1)
                nan0[sbase0 + lr - s0] = sd[lr][0] != sd[lr][0];
        }
        __syncthreads();

        topk_list_merge<TS>(top, sd, cpos, amask, omask, lr, q, k, nbase);
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
// the quiet NaN vsom_bmu_batch's sqres holds.
__global__ __launch_bounds__(64) void topk_merge_kernel(const u64 *__restrict__ part, const unsigned char *__restrict__ nan0,
                                                        int ng, int k, u64 *__restrict__ idx, float *__restrict__ dist)
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
    // (k <= N: the lists hold the k smallest keys, so every counted round takes a real key; every round consumes one key)
    while (cnt < k) {
        const u64 m = vsom_wave_min(head);
        if (head == m) {                        // keys are unique: one lane
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
        idx[(size_t)row * k + lane] = mine & 0xFFFFFFFFull;
        if (dist)
            dist[(size_t)row * k + lane] = __uint_as_float(bits == 0xFFFFFFFFu ? 0x7FC00000u : bits);
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
                               (int)k, (int)G, lay.at(part), lay.at(nan0));
        else
            hipLaunchKernelGGL((topk_tile_kernel<false, 4>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1, (int)N,
                               (int)k, (int)G, lay.at(part), lay.at(nan0));
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)n), dim3(64), ng * k * 8, c->stream, lay.at(part),
                           lay.at(nan0), (int)ng, (int)k, lay.at(idx), dist_out ? lay.at(dist) : nullptr);
        VSOM_HIP_CHECK(hipGetLastError());
        VSOM_HIP_CHECK(hipMemcpyAsync(idx_out + off * k, lay.at(idx), n * k * 8, hipMemcpyDeviceToHost, c->stream));
        if (dist_out)
            VSOM_HIP_CHECK(hipMemcpyAsync(dist_out + off * k, lay.at(dist), n * k * 4, hipMemcpyDeviceToHost, c->stream));
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}
