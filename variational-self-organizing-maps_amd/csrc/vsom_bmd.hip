// vsom_bmd.hip -- Som::findRestrictedBmd (Som.cpp:457-487) for a range of chunk rows, and one draw per row (gfx950).
//
//  bmd_tile_kernel : the shared distance tile (vsom_dist_tile.hpp: 64 (CLR: 32) rows x 64 nodes per workgroup, 8 class
//                    accumulators + Eigen's reduction tree, the exact search's operations in its order) with a
//                    distribution epilogue: p = hits >= min_hits ? exp(-(double)d * d / 2) : 0 (Som.cpp:468-479),
//                    stored node-major inside the row slice, P[node * ppitch + row].  With the mask policies of the
//                    masked search, VsomMaskRows / VsomMaskOne, the same kernel over the VALID columns
//                    (vsom_bmd_masked_batch)
//  bmd_sum_kernel  : one lane per row walks the nodes in ascending order, C = ((0 + p_0) + p_1) + ... (Som.cpp:463-476),
//                    keeping the running sum at every BMD_NC-node boundary; the draw re-walks the one BMD_NC-node chunk
//                    that holds the first running sum above t = u * C with the same adds
//  bmd_prob_kernel : p_i / C (Som.cpp:483-484), transposed to row-major for the copy-out
//  bmd_draws_kernel: many draws from ONE row's distribution (vsom_generate_batch, VSOM_GENERATE_AS_WRITTEN): one thread per
//                    uniform, the chunk search and the re-walk of bmd_sum_kernel's draw (bmd_find_chunk / bmd_walk_chunk)
//  bmd_row_draws_kernel: K draws from EVERY row's distribution (vsom_generate_masked_batch), bmd_draws_kernel's steps
//                    (one device function, bmd_draw_row, serves both)
#include "vsom_dist_tile.hpp"
#include <algorithm>

#define BMD_R 8        // rows per workgroup of the row pass
#define BMD_NC 256     // nodes per chunk of the row pass (one per thread)

// Where a tile's mask policy (vsom_dist_tile.hpp) comes from: nothing for VsomMaskNone; for VsomMaskRows / VsomMaskOne
// (vsom_bmd_masked_batch, Standard / Median) the packed validity rows of the slice, vld bytes each, 0xFF = valid (row s - s0
// at vp + (s - s0) * vld; VsomMaskOne: the one row every sample shares)
template <class Mask> struct BmdMaskSrc {
    const unsigned char *vp;
    int vld;
};
template <> struct BmdMaskSrc<VsomMaskNone> {
};

// Mask = VsomMaskRows / VsomMaskOne: the tile over the VALID columns, r_d = valid ? m_d - x_d : +0 by select -- the distance
// of masked_tile_kernel (vsom_masked.hip) -- under the same epilogue
template <bool CLR, int TI, class Mask = VsomMaskNone>
__global__ __launch_bounds__(256, 2) void bmd_tile_kernel(DistArgs a, int s0, int s1, int N, double *__restrict__ P,
                                                          int ppitch, const u64 *__restrict__ hits, u64 min_hits,
                                                          BmdMaskSrc<Mask> ms)
{
    constexpr int TS = 16 * TI;                 // samples per tile
    __shared__ double sp[TILE][TS + 1];         // the tile's p, node-major, for coalesced stores

    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int nbase = blockIdx.x * TILE;
    const int sbase = s0 + blockIdx.y * TS;
    const Mask mask = [&] {
        if constexpr (std::is_same<Mask, VsomMaskNone>::value)
            return VsomMaskNone();
        else
            return Mask(ms.vp, ms.vld, tid, sbase, s0, s1);
    }();

    // Som.cpp:468-479: the distance as a double, exp(-d * d / 2) for the nodes with enough hits, 0 for the others
    vsom_dist_tile<CLR, TI>(a, tid, sbase, s1, nbase, N, mask,
                            [&](int i, int j, float res) {
                                const int n = nbase + tx + 16 * j;
                                const double d = (double)res;
                                sp[tx + 16 * j][ty + 16 * i] = (n < N && hits[n] >= min_hits) ? exp(-d * d / 2) : 0.0;
                            });
    __syncthreads();
    // node-major stores: consecutive lanes write consecutive rows of one node
#pragma unroll
    for (int k = 0; k < TILE * TS / 256; ++k) {
        const int f = tid + 256 * k, nl = f / TS, rl = f % TS;
        const int n = nbase + nl, s = sbase + rl;
        if (n < N && s < s1)
            P[(size_t)n * ppitch + (s - s0)] = sp[nl][rl];
    }
}

// The two steps of a draw, shared by bmd_sum_kernel and bmd_draws_kernel.
// The first chunk whose closing running sum exceeds t, or -1; cum(k) = the running sum after chunk k.
template <class F> __device__ __forceinline__ int bmd_find_chunk(F cum, int nch, double t)
{
    for (int k = 0; k < nch; ++k)
        if (cum(k) > t)
            return k;
    return -1;
}
// The walk of that chunk from the running sum s in front of it, with the adds of the row pass: the first node whose running
// sum exceeds t, or `none`; p(j) = the chunk's j-th value.
template <class F> __device__ __forceinline__ u64 bmd_walk_chunk(F p, double s, int n0, int cnt, double t, u64 none)
{
    for (int j = 0; j < cnt; ++j) {
        s = s + p(j);                           // the same adds as the row pass
        if (s > t)
            return (u64)(n0 + j);
    }
    return none;
}

// BMD_R rows per workgroup: the 256 threads stage BMD_NC nodes x BMD_R rows of P per step (the next step's loads in
// flight while the current one is summed), lanes 0..BMD_R-1 of the first wavefront add them up in node order.
// ppitch is a multiple of BMD_R, so a thread's BMD_R values of one node are one aligned 64-byte run.
// cum[k * ppitch + r] = the running sum after chunk k; draw: NULL = no draws (u is not read).
__global__ __launch_bounds__(256) void bmd_sum_kernel(const double *__restrict__ P, int ppitch, int rows, int N,
                                                      double *__restrict__ cum, const double *__restrict__ u,
                                                      double *__restrict__ norm, u64 *__restrict__ draw)
{
    __shared__ double sp[BMD_R][BMD_NC + 1];
    __shared__ int schunk[BMD_R];
    const int tid = threadIdx.x;
    const int rb = blockIdx.x * BMD_R;
    const int nch = (N + BMD_NC - 1) / BMD_NC;
    double g[BMD_R];
    auto load = [&](int k) {
        const int n = k * BMD_NC + tid;
        if (n < N) {
            const double2 *src = reinterpret_cast<const double2 *>(P + (size_t)n * ppitch + rb);
#pragma unroll
            for (int q = 0; q < BMD_R / 2; ++q) {
                const double2 v = src[q];
                g[2 * q] = v.x;
                g[2 * q + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int q = 0; q < BMD_R; ++q)
                g[q] = 0.0;
        }
    };
    const int row = rb + tid;
    const bool mine = tid < BMD_R && row < rows;
    double C = 0.0;                             // Som.cpp:463
    int lastpos = -1;                           // the largest node with p > 0
    load(0);
    for (int k = 0; k < nch; ++k) {
        if (k > 0)
            __syncthreads();
#pragma unroll
        for (int q = 0; q < BMD_R; ++q)
            sp[q][tid] = g[q];
        __syncthreads();
        if (k + 1 < nch)
            load(k + 1);
        if (tid < BMD_R) {
            const int n0 = k * BMD_NC, cnt = N - n0 < BMD_NC ? N - n0 : BMD_NC;
            for (int j = 0; j < cnt; ++j) {
                const double p = sp[tid][j];
                C = C + p;                      // Som.cpp:476 (a masked node adds 0: C unchanged)
                lastpos = p > 0.0 ? n0 + j : lastpos;
            }
            if (mine && draw)
                cum[(size_t)k * ppitch + row] = C;
        }
    }
    if (mine)
        norm[row] = C;
    if (!draw)
        return;                                 // (grid-uniform)
    // the chunk holding the first running sum above t; no mass: UINT64_MAX; no running sum above t (u close to 1):
    // the last node with mass
    double t = 0.0;
    int kc = -1;
    u64 result = ~0ull;
    if (mine && C > 0.0 && __builtin_isfinite(C)) {
        t = u[row] * C;
        kc = bmd_find_chunk([&](int k) { return cum[(size_t)k * ppitch + row]; }, nch, t);
        if (kc < 0)
            result = (u64)lastpos;
    }
    __syncthreads();                            // everyone is done with sp
    if (tid < BMD_R)
        schunk[tid] = kc;
    __syncthreads();
    {
        const int lr = tid >> 5, l = tid & 31;  // 32 threads per row
        const int k = schunk[lr];
        if (k >= 0) {
#pragma unroll
            for (int q = 0; q < BMD_NC / 32; ++q) {
                const int j = l + 32 * q, n = k * BMD_NC + j;
                sp[lr][j] = n < N ? P[(size_t)n * ppitch + rb + lr] : 0.0;
            }
        }
    }
    __syncthreads();
    if (mine && kc >= 0) {
        const double s = kc > 0 ? cum[(size_t)(kc - 1) * ppitch + row] : 0.0;
        const int n0 = kc * BMD_NC, cnt = N - n0 < BMD_NC ? N - n0 : BMD_NC;
        result = bmd_walk_chunk([&](int j) { return sp[tid][j]; }, s, n0, cnt, t, result);
    }
    if (mine)
        draw[row] = result;
}

// One draw from the distribution of slice row `row`, whose P column, running sums (cum) and mass (norm) a bmd_sum_kernel
// launch with draws has left: what that launch would have drawn for the row with the uniform u.  The BMD_NC values of a
// chunk are read straight from P.
__device__ __forceinline__ u64 bmd_draw_row(const double *__restrict__ P, int ppitch, int row, int N,
                                            const double *__restrict__ cum, const double *__restrict__ norm, double u)
{
    const int nch = (N + BMD_NC - 1) / BMD_NC;
    const double C = norm[row];
    u64 result = ~0ull;
    if (C > 0.0 && __builtin_isfinite(C)) {
        const double t = u * C;
        const int kc = bmd_find_chunk([&](int k) { return cum[(size_t)k * ppitch + row]; }, nch, t);
        if (kc < 0) {
            // no running sum above t (u close to 1): the last node with mass (C > 0: there is one)
            for (int n = N - 1; n >= 0; --n)
                if (P[(size_t)n * ppitch + row] > 0.0) {
                    result = (u64)n;
                    break;
                }
        } else {
            const double s = kc > 0 ? cum[(size_t)(kc - 1) * ppitch + row] : 0.0;
            const int n0 = kc * BMD_NC, cnt = N - n0 < BMD_NC ? N - n0 : BMD_NC;
            result = bmd_walk_chunk([&](int j) { return P[(size_t)(n0 + j) * ppitch + row]; }, s, n0, cnt, t, result);
        }
    }
    return result;
}

// ndraws draws from the distribution of the ONE slice row `row` (vsom_generate_batch, VSOM_GENERATE_AS_WRITTEN): one thread
// per uniform, draw[i] from u[i]; every thread reads the same few lines of P.
__global__ __launch_bounds__(256) void bmd_draws_kernel(const double *__restrict__ P, int ppitch, int row, int N,
                                                        const double *__restrict__ cum, const double *__restrict__ norm,
                                                        const double *__restrict__ u, int ndraws, u64 *__restrict__ draw)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= ndraws)
        return;
    draw[i] = bmd_draw_row(P, ppitch, row, N, cum, norm, u[i]);
}

// K draws from the distribution of EVERY slice row (vsom_generate_masked_batch): thread i serves row i / K with the
// uniform u[i]; the K threads of a row read the same lines of P.
__global__ __launch_bounds__(256) void bmd_row_draws_kernel(const double *__restrict__ P, int ppitch, int N, int K,
                                                            const double *__restrict__ cum, const double *__restrict__ norm,
                                                            const double *__restrict__ u, size_t ndraws,
                                                            u64 *__restrict__ draw)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ndraws)
        return;
    draw[i] = bmd_draw_row(P, ppitch, (int)(i / (size_t)K), N, cum, norm, u[i]);
}

// rows [q0, q0 + nrows) of the slice: out[r * N + n] = P[n * ppitch + q0 + r] / C (Som.cpp:483-484), 32 x 32 per workgroup
__global__ __launch_bounds__(256) void bmd_prob_kernel(const double *__restrict__ P, int ppitch, int q0, int nrows, int N,
                                                       const double *__restrict__ norm, double *__restrict__ out)
{
    __shared__ double t[32][33];
    const int n0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8) {
        const int n = n0 + k, r = r0 + tx;
        if (n < N && r < nrows)
            t[k][tx] = P[(size_t)n * ppitch + q0 + r] / norm[q0 + r];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, n = n0 + tx;
        if (n < N && r < nrows)
            out[(size_t)r * N + n] = t[tx][k];
    }
}

// rows per slice: the node-major p of a slice stays within 256 MiB
static size_t vsom_bmd_slice_rows(size_t N)
{
    const size_t s = ((size_t)256 << 20) / (8 * N);
    return s > 0 ? s : 1;
}

size_t vsom_bmd_pitch(size_t rows) { return (rows + BMD_R - 1) / BMD_R * BMD_R; }
size_t vsom_bmd_chunks(size_t N) { return (N + BMD_NC - 1) / BMD_NC; }

// the validity scratch of one slice of a masked distribution: the caller's bytes and the packed rows (vsom_internal.hpp)
VsomBmdMask vsom_bmd_mask_add(const vsom_ctx *c, vsom_layout &lay, const uint8_t *valid_host, bool one, size_t slice)
{
    VsomBmdMask m;
    m.on = valid_host != nullptr;
    m.one = one;
    const size_t vrows = !m.on ? 0 : one ? 1 : slice;
    m.raw = lay.add<unsigned char>(vrows * c->J);
    m.packed = lay.add<unsigned char>(vrows * c->xpitch);
    return m;
}

// slice [s0, s1) of a call over rows from r0: its validity bytes up and packed (a column mask once, with the first slice)
int vsom_bmd_mask_slice_enqueue(vsom_ctx *c, const vsom_layout &lay, const VsomBmdMask &m, size_t r0, size_t s0, size_t s1,
                                const uint8_t *valid_host)
{
    if (!m.on || (m.one && s0 != r0))
        return VSOM_OK;
    const size_t J = c->J, vr = m.one ? 1 : s1 - s0;
    VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(m.raw), valid_host + (m.one ? 0 : (s0 - r0) * J), vr * J, hipMemcpyHostToDevice,
                                  c->stream));
    vsom_masked_pack_enqueue(c, lay.at(m.raw), vr, lay.at(m.packed));
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}

// the tile and the row pass of slice rows [s0, s1) on the context's stream (vsom_internal.hpp); vp: the slice's packed
// validity rows (one: the row every sample shares), null = every column counts
int vsom_bmd_enqueue(vsom_ctx *c, u64 min_hits, size_t s0, size_t s1, double *P, size_t ppitch, double *cum,
                     const double *u_dev, double *norm_dev, u64 *draw_dev, const unsigned char *vp, bool one)
{
    const size_t N = c->N, n = s1 - s0;
    const DistArgs a = vsom_dist_args(c);
    const int TS = c->transform == VSOM_CLR ? 32 : TILE;
    dim3 grid((unsigned)((N + TILE - 1) / TILE), (unsigned)((n + TS - 1) / TS));
    if (vp && one)
        hipLaunchKernelGGL((bmd_tile_kernel<false, 4, VsomMaskOne>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1, (int)N, P,
                           (int)ppitch, c->hits.p, min_hits, BmdMaskSrc<VsomMaskOne>{vp, (int)c->xpitch});
    else if (vp)
        hipLaunchKernelGGL((bmd_tile_kernel<false, 4, VsomMaskRows>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1, (int)N,
                           P, (int)ppitch, c->hits.p, min_hits, BmdMaskSrc<VsomMaskRows>{vp, (int)c->xpitch});
    else if (c->transform == VSOM_CLR)
        hipLaunchKernelGGL((bmd_tile_kernel<true, 2>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1, (int)N, P,
                           (int)ppitch, c->hits.p, min_hits, BmdMaskSrc<VsomMaskNone>{});
    else
        hipLaunchKernelGGL((bmd_tile_kernel<false, 4>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1, (int)N, P,
                           (int)ppitch, c->hits.p, min_hits, BmdMaskSrc<VsomMaskNone>{});
    hipLaunchKernelGGL(bmd_sum_kernel, dim3((unsigned)((n + BMD_R - 1) / BMD_R)), dim3(256), 0, c->stream, P, (int)ppitch,
                       (int)n, (int)N, cum, u_dev, norm_dev, draw_dev);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}

int vsom_bmd_enqueue_draws(vsom_ctx *c, const double *P, size_t ppitch, size_t row, const double *cum, const double *norm_dev,
                           const double *u_dev, size_t ndraws, u64 *draw_dev)
{
    hipLaunchKernelGGL(bmd_draws_kernel, dim3((unsigned)((ndraws + 255) / 256)), dim3(256), 0, c->stream, P, (int)ppitch,
                       (int)row, (int)c->N, cum, norm_dev, u_dev, (int)ndraws, draw_dev);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}

int vsom_bmd_enqueue_row_draws(vsom_ctx *c, const double *P, size_t ppitch, size_t rows, size_t K, const double *cum,
                               const double *norm_dev, const double *u_dev, u64 *draw_dev)
{
    const size_t ndraws = rows * K;
    hipLaunchKernelGGL(bmd_row_draws_kernel, dim3((unsigned)((ndraws + 255) / 256)), dim3(256), 0, c->stream, P, (int)ppitch,
                       (int)c->N, (int)K, cum, norm_dev, u_dev, ndraws, draw_dev);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}

// valid_host: null (vsom_bmd_batch) or the validity bytes of vsom_bmd_masked_batch
int launch_bmd(vsom_ctx *c, u64 min_hits, size_t r0, size_t r1, const double *u_host, uint64_t *draw_out, double *norm_out,
               double *prob_out, const uint8_t *valid_host, int one_mask)
{
    TimerScope ts(c, VSOM_T_BMU);
    const size_t N = c->N, rows = r1 - r0;
    if (rows == 0)
        return VSOM_OK;
    size_t slice = std::min(vsom_bmd_slice_rows(N), rows);
    if (valid_host)
        slice = std::min(slice, vsom_masked_search_slice_rows(c));
    const size_t ppitch = (slice + BMD_R - 1) / BMD_R * BMD_R;
    const size_t nch = (N + BMD_NC - 1) / BMD_NC;
    const size_t prow = std::min(slice, std::max<size_t>(1, ((size_t)32 << 20) / (8 * N)));   // rows per prob copy-out
    // the slice's p (node-major), running sums at chunk boundaries, uniforms | norms and draws; one copy-out piece of prob;
    // the slice's validity bytes
    vsom_layout lay;
    const auto p = lay.add<double>(ppitch * N), cum = lay.add<double>(nch * ppitch), vec = lay.add<double>(2 * ppitch),
               prob = lay.add<double>(prob_out ? prow * N : 0);
    const auto draw = lay.add<u64>(ppitch);
    const VsomBmdMask mask = vsom_bmd_mask_add(c, lay, valid_host, one_mask != 0, slice);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    double *P = lay.at(p), *u_dev = lay.at(vec), *norm_dev = lay.at(vec) + ppitch;
    u64 *draw_dev = draw_out ? lay.at(draw) : nullptr;
    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0, off = s0 - r0;
        if (draw_out)
            VSOM_HIP_CHECK(hipMemcpyAsync(u_dev, u_host + off, n * 8, hipMemcpyHostToDevice, c->stream));
        if (int rc = vsom_bmd_mask_slice_enqueue(c, lay, mask, r0, s0, s1, valid_host))
            return rc;
        if (int rc = vsom_bmd_enqueue(c, min_hits, s0, s1, P, ppitch, lay.at(cum), u_dev, norm_dev, draw_dev,
                                      mask.on ? lay.at(mask.packed) : nullptr, mask.one))
            return rc;
        if (norm_out)
            VSOM_HIP_CHECK(hipMemcpyAsync(norm_out + off, norm_dev, n * 8, hipMemcpyDeviceToHost, c->stream));
        if (draw_out)
            VSOM_HIP_CHECK(hipMemcpyAsync(draw_out + off, draw_dev, n * 8, hipMemcpyDeviceToHost, c->stream));
        for (size_t q0 = 0; prob_out && q0 < n; q0 += prow) {
            const size_t m = std::min(prow, n - q0);
            hipLaunchKernelGGL(bmd_prob_kernel, dim3((unsigned)((N + 31) / 32), (unsigned)((m + 31) / 32)), dim3(256), 0,
                               c->stream, P, (int)ppitch, (int)q0, (int)m, (int)N, norm_dev, lay.at(prob));
            VSOM_HIP_CHECK(hipGetLastError());
            VSOM_HIP_CHECK(hipMemcpyAsync(prob_out + (off + q0) * N, lay.at(prob), m * N * 8, hipMemcpyDeviceToHost,
                                          c->stream));
        }
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}
