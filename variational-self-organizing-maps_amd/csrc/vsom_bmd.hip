// vsom_bmd.hip -- Som::findRestrictedBmd (Som.cpp:457-487) for a range of chunk rows, and one draw per row (gfx950).
//
//  bmd_tile_kernel : the shared distance tile (vsom_dist_tile.hpp: 64 (CLR: 32) rows x 64 nodes per workgroup, 8 class
//                    accumulators + Eigen's reduction tree, the exact search's operations in its order) with a
//                    distribution epilogue: p = hits >= min_hits ? exp(-(double)d * d / 2) : 0 (Som.cpp:468-479),
//                    stored node-major inside the row slice, P[node * ppitch + row]
//  bmd_sum_kernel  : one lane per row walks the nodes in ascending order, C = ((0 + p_0) + p_1) + ... (Som.cpp:463-476),
//                    keeping the running sum at every BMD_NC-node boundary; the draw re-walks the one BMD_NC-node chunk
//                    that holds the first running sum above t = u * C with the same adds
//  bmd_prob_kernel : p_i / C (Som.cpp:483-484), transposed to row-major for the copy-out
//  bmd_draws_kernel: many draws from ONE row's distribution (vsom_generate_batch, VSOM_GENERATE_AS_WRITTEN): one thread per
//                    uniform, the chunk search and the re-walk of bmd_sum_kernel's draw (bmd_find_chunk / bmd_walk_chunk)
#include "vsom_dist_tile.hpp"
#include <algorithm>

#define BMD_R 8        // rows per workgroup of the row pass
#define BMD_NC 256     // nodes per chunk of the row pass (one per thread)

template <bool CLR, int TI>
__global__ __launch_bounds__(256, 2) void bmd_tile_kernel(DistArgs a, int s0, int s1, int N, double *__restrict__ P,
                                                          int ppitch, const u64 *__restrict__ hits, u64 min_hits)
{
    constexpr int TS = 16 * TI;                 // samples per tile
    __shared__ double sp[TILE][TS + 1];         // the tile's p, node-major, for coalesced stores

    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int nbase = blockIdx.x * TILE;
    const int sbase = s0 + blockIdx.y * TS;

    // Som.cpp:468-479: the distance as a double, exp(-d * d / 2) for the nodes with enough hits, 0 for the others
    vsom_dist_tile<CLR, TI>(a, tid, sbase, s1, nbase, N, VsomMaskNone(),
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

// ndraws draws from the distribution of slice row `row`, whose P column, running sums (cum) and mass (norm) a
// bmd_sum_kernel launch with draws has left: draw[i] is what that launch would have drawn for the row with uniform u[i].
// One thread per draw; the BMD_NC values of a chunk are read straight from P (every thread reads the same few lines).
__global__ __launch_bounds__(256) void bmd_draws_kernel(const double *__restrict__ P, int ppitch, int row, int N,
                                                        const double *__restrict__ cum, const double *__restrict__ norm,
                                                        const double *__restrict__ u, int ndraws, u64 *__restrict__ draw)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= ndraws)
        return;
    const int nch = (N + BMD_NC - 1) / BMD_NC;
    const double C = norm[row];
    u64 result = ~0ull;
    if (C > 0.0 && __builtin_isfinite(C)) {
        const double t = u[i] * C;
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
    draw[i] = result;
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

// the tile and the row pass of slice rows [s0, s1) on the context's stream (vsom_internal.hpp)
int vsom_bmd_enqueue(vsom_ctx *c, u64 min_hits, size_t s0, size_t s1, double *P, size_t ppitch, double *cum,
                     const double *u_dev, double *norm_dev, u64 *draw_dev)
{
    const size_t N = c->N, n = s1 - s0;
    const DistArgs a = vsom_dist_args(c);
    const int TS = c->transform == VSOM_CLR ? 32 : TILE;
    dim3 grid((unsigned)((N + TILE - 1) / TILE), (unsigned)((n + TS - 1) / TS));
    if (c->transform == VSOM_CLR)
        hipLaunchKernelGGL((bmd_tile_kernel<true, 2>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1, (int)N, P,
                           (int)ppitch, c->hits.p, min_hits);
    else
        hipLaunchKernelGGL((bmd_tile_kernel<false, 4>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1, (int)N, P,
                           (int)ppitch, c->hits.p, min_hits);
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

int launch_bmd(vsom_ctx *c, u64 min_hits, size_t r0, size_t r1, const double *u_host, uint64_t *draw_out, double *norm_out,
               double *prob_out)
{
    TimerScope ts(c, VSOM_T_BMU);
    const size_t N = c->N, rows = r1 - r0;
    if (rows == 0)
        return VSOM_OK;
    const size_t slice = std::min(vsom_bmd_slice_rows(N), rows);
    const size_t ppitch = (slice + BMD_R - 1) / BMD_R * BMD_R;
    const size_t nch = (N + BMD_NC - 1) / BMD_NC;
    const size_t prow = std::min(slice, std::max<size_t>(1, ((size_t)32 << 20) / (8 * N)));   // rows per prob copy-out
    // the slice's p (node-major), running sums at chunk boundaries, uniforms | norms and draws; one copy-out piece of prob
    vsom_layout lay;
    const auto p = lay.add<double>(ppitch * N), cum = lay.add<double>(nch * ppitch), vec = lay.add<double>(2 * ppitch),
               prob = lay.add<double>(prob_out ? prow * N : 0);
    const auto draw = lay.add<u64>(ppitch);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    double *P = lay.at(p), *u_dev = lay.at(vec), *norm_dev = lay.at(vec) + ppitch;
    u64 *draw_dev = draw_out ? lay.at(draw) : nullptr;
    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0, off = s0 - r0;
        if (draw_out)
            VSOM_HIP_CHECK(hipMemcpyAsync(u_dev, u_host + off, n * 8, hipMemcpyHostToDevice, c->stream));
        if (int rc = vsom_bmd_enqueue(c, min_hits, s0, s1, P, ppitch, lay.at(cum), u_dev, norm_dev, draw_dev))
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
