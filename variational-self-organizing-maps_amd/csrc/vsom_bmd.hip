// vsom_bmd.hip -- Som::findRestrictedBmd (Som.cpp:457-487) for a range of chunk rows, and one draw per row (gfx950).
//
//  bmd_tile_kernel : the distance tile of bmu_tile_kernel (vsom_bmu.hip: 64 (CLR: 32) rows x 64 nodes per workgroup,
//                    8 class accumulators + Eigen's reduction tree, the same operations in the same order) with a
//                    distribution epilogue: p = hits >= min_hits ? exp(-(double)d * d / 2) : 0 (Som.cpp:468-479),
//                    stored node-major inside the row slice, P[node * ppitch + row]
//  bmd_sum_kernel  : one lane per row walks the nodes in ascending order, C = ((0 + p_0) + p_1) + ... (Som.cpp:463-476),
//                    keeping the running sum at every BMD_NC-node boundary; the draw re-walks the one BMD_NC-node chunk
//                    that holds the first running sum above t = u * C with the same adds
//  bmd_prob_kernel : p_i / C (Som.cpp:483-484), transposed to row-major for the copy-out
// The body of the tile is a copy of bmu_tile_body without its row / node lists: no existing kernel changes.
#include "vsom_device.hpp"
#include <algorithm>

#define TILE 64
#define LDT 36
#define BMD_R 8        // rows per workgroup of the row pass
#define BMD_NC 256     // nodes per chunk of the row pass (one per thread)

template <bool CLR, int TI>
__global__ __launch_bounds__(256, 2) void bmd_tile_kernel(DistArgs a, int s0, int s1, int N, double *__restrict__ P,
                                                          int ppitch, const u64 *__restrict__ hits, u64 min_hits)
{
    constexpr int TS = 16 * TI;                 // samples per tile
    constexpr int NX = TS * 8 / 256;            // float4 of a sample operand per thread and K-chunk (1 or 2)
    __shared__ __attribute__((aligned(16))) float sx[TILE * LDT];
    __shared__ __attribute__((aligned(16))) float sm[TILE * LDT];
    __shared__ __attribute__((aligned(16))) float sy[CLR ? TS * LDT : 4];
    __shared__ __attribute__((aligned(16))) float sb[CLR ? TILE * LDT : 4];
    __shared__ double sp[TILE][TS + 1];         // the tile's p, node-major, for coalesced stores

    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int nbase = blockIdx.x * TILE;
    const int sbase = s0 + blockIdx.y * TS;
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

    float4 gx[NX], gm[2], gy[NX], gb[2];
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
            *reinterpret_cast<float4 *>(&sx[row * LDT + c4]) = gx[i];
            if (CLR)
                *reinterpret_cast<float4 *>(&sy[row * LDT + c4]) = gy[i];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int f = tid + 256 * i;
            int row = f >> 3, c4 = (f & 7) * 4;
            *reinterpret_cast<float4 *>(&sm[row * LDT + c4]) = gm[i];
            if (CLR)
                *reinterpret_cast<float4 *>(&sb[row * LDT + c4]) = gb[i];
        }
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
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float r0 = vsom_resid<CLR>(xv[i].x, CLR ? yv[i].x : 0.f, mv[j].x, CLR ? bv[j].x : 0.f);
                            float r1 = vsom_resid<CLR>(xv[i].y, CLR ? yv[i].y : 0.f, mv[j].y, CLR ? bv[j].y : 0.f);
                            float r2 = vsom_resid<CLR>(xv[i].z, CLR ? yv[i].z : 0.f, mv[j].z, CLR ? bv[j].z : 0.f);
                            float r3 = vsom_resid<CLR>(xv[i].w, CLR ? yv[i].w : 0.f, mv[j].w, CLR ? bv[j].w : 0.f);
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
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float q0 = acc[i][j][0] + acc[i][j][4];
            float q1 = acc[i][j][1] + acc[i][j][5];
            float q2 = acc[i][j][2] + acc[i][j][6];
            float q3 = acc[i][j][3] + acc[i][j][7];
            const int xr = (ty + 16 * i) * LDT + roff, mr = (tx + 16 * j) * LDT + roff;
            int t = 0;
            if (rem >= 4) {
                float r0 = vsom_resid<CLR>(sx[xr + 0], CLR ? sy[xr + 0] : 0.f, sm[mr + 0], CLR ? sb[mr + 0] : 0.f);
                float r1 = vsom_resid<CLR>(sx[xr + 1], CLR ? sy[xr + 1] : 0.f, sm[mr + 1], CLR ? sb[mr + 1] : 0.f);
                float r2 = vsom_resid<CLR>(sx[xr + 2], CLR ? sy[xr + 2] : 0.f, sm[mr + 2], CLR ? sb[mr + 2] : 0.f);
                float r3 = vsom_resid<CLR>(sx[xr + 3], CLR ? sy[xr + 3] : 0.f, sm[mr + 3], CLR ? sb[mr + 3] : 0.f);
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
                float r = vsom_resid<CLR>(sx[xr + t], CLR ? sy[xr + t] : 0.f, sm[mr + t], CLR ? sb[mr + t] : 0.f);
                float p = r * r;
                res = res + p;
            }
            // Som.cpp:468-479: the distance as a double, exp(-d * d / 2) for the nodes with enough hits, 0 for the others
            const int n = nbase + tx + 16 * j;
            const double d = (double)res;
            sp[tx + 16 * j][ty + 16 * i] = (n < N && hits[n] >= min_hits) ? exp(-d * d / 2) : 0.0;
        }
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
        for (int k = 0; k < nch; ++k)
            if (cum[(size_t)k * ppitch + row] > t) {
                kc = k;
                break;
            }
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
        double s = kc > 0 ? cum[(size_t)(kc - 1) * ppitch + row] : 0.0;
        const int n0 = kc * BMD_NC, cnt = N - n0 < BMD_NC ? N - n0 : BMD_NC;
        for (int j = 0; j < cnt; ++j) {
            s = s + sp[tid][j];                 // the same adds as the walk above
            if (s > t) {
                result = (u64)(n0 + j);
                break;
            }
        }
    }
    if (mine)
        draw[row] = result;
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

static DistArgs bmd_dist_args(const vsom_ctx *c)
{
    DistArgs a;
    if (c->transform == VSOM_CLR) {
        a.xa = c->XP.p;
        a.xb = c->YP.p;
        a.ldx = (int)c->part_pitch;
        a.ma = c->map.p;
        a.mb = c->map.p + c->part_pitch;
    } else {
        a.xa = c->Xs.p;
        a.xb = c->Xs.p;
        a.ldx = (int)c->xpitch;
        a.ma = c->map.p;
        a.mb = c->map.p;
    }
    a.ldm = (int)c->pitch;
    a.L = (int)c->part_len;
    return a;
}

// rows per slice: the node-major p of a slice stays within 256 MiB
static size_t vsom_bmd_slice_rows(size_t N)
{
    const size_t s = ((size_t)256 << 20) / (8 * N);
    return s > 0 ? s : 1;
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
    VSOM_ALLOC_CHECK(vsom_grow_set(c->stream, VSOM_BUF_SYNC,
                                   {vsom_member(c->bmd_p, ppitch * N), vsom_member(c->bmd_cum, nch * ppitch),
                                    vsom_member(c->bmd_vec, 2 * ppitch), vsom_member(c->bmd_draw, ppitch),
                                    vsom_member(c->bmd_prob, prob_out ? prow * N : 0)}));
    double *P = c->bmd_p.p, *u_dev = c->bmd_vec.p, *norm_dev = c->bmd_vec.p + ppitch;
    u64 *draw_dev = draw_out ? c->bmd_draw.p : nullptr;
    const DistArgs a = bmd_dist_args(c);
    const int TS = c->transform == VSOM_CLR ? 32 : TILE;
    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0, off = s0 - r0;
        if (draw_out)
            VSOM_HIP_CHECK(hipMemcpyAsync(u_dev, u_host + off, n * 8, hipMemcpyHostToDevice, c->stream));
        dim3 grid((unsigned)((N + TILE - 1) / TILE), (unsigned)((n + TS - 1) / TS));
        if (c->transform == VSOM_CLR)
            hipLaunchKernelGGL((bmd_tile_kernel<true, 2>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1, (int)N, P,
                               (int)ppitch, c->hits.p, min_hits);
        else
            hipLaunchKernelGGL((bmd_tile_kernel<false, 4>), grid, dim3(256), 0, c->stream, a, (int)s0, (int)s1, (int)N, P,
                               (int)ppitch, c->hits.p, min_hits);
        hipLaunchKernelGGL(bmd_sum_kernel, dim3((unsigned)((n + BMD_R - 1) / BMD_R)), dim3(256), 0, c->stream, P, (int)ppitch,
                           (int)n, (int)N, c->bmd_cum.p, u_dev, norm_dev, draw_dev);
        VSOM_HIP_CHECK(hipGetLastError());
        if (norm_out)
            VSOM_HIP_CHECK(hipMemcpyAsync(norm_out + off, norm_dev, n * 8, hipMemcpyDeviceToHost, c->stream));
        if (draw_out)
            VSOM_HIP_CHECK(hipMemcpyAsync(draw_out + off, draw_dev, n * 8, hipMemcpyDeviceToHost, c->stream));
        for (size_t q0 = 0; prob_out && q0 < n; q0 += prow) {
            const size_t m = std::min(prow, n - q0);
            hipLaunchKernelGGL(bmd_prob_kernel, dim3((unsigned)((N + 31) / 32), (unsigned)((m + 31) / 32)), dim3(256), 0,
                               c->stream, P, (int)ppitch, (int)q0, (int)m, (int)N, norm_dev, c->bmd_prob.p);
            VSOM_HIP_CHECK(hipGetLastError());
            VSOM_HIP_CHECK(hipMemcpyAsync(prob_out + (off + q0) * N, c->bmd_prob.p, m * N * 8, hipMemcpyDeviceToHost,
                                          c->stream));
        }
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}
