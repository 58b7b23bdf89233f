// vsom_online_masked.hip -- the online chunk loop over the VALID entries of the rows only (gfx950; Standard / Median):
// the kernels of vsom_train_online_chunk_masked (its entry point and preamble are vsom_online.hip's).
//
// The exact-scan chunk loop of vsom_online.hip with a validity row per sample (packed bytes, 0xFF = valid, xpitch a row,
// or ONE row every sample shares):
//   search   the distance of vsom_bmu_masked_batch, r_d = valid ? m_d - x_d : +0 (masked_group_dist, vsom_masked_dist.hpp)
//   window   weightMap and the scalars of the step are the unmasked step's; map / SMap / sigmaMap of a VALID column get the
//            unmasked step's float operations, those of an invalid column are not written (their bits stay, NaN included)
//   post     the masked distance to the updated BMU row, MSE, addBmu, lastBMU
// As in vsom_online.hip one sample is two launches (sigma > 1) or one (sigma <= 1), enqueued back to back:
//   online_scan_masked_kernel        online_scan_kernel<false, POSTWG = true> on the masked distance: same key, same slots by
//                                    sample parity, same node-0-NaN flag; its last workgroup finishes the PREVIOUS sample and
//                                    therefore takes that sample's validity row too.  do_scan = 0 ends the chunk.
//   online_window_masked_kernel      one workgroup per node of the maximal window (online_window_kernel<KIND, POST = false>)
//   online_small_masked_kernel       sigma <= 1: findLocalBmu's walk on the masked distance (vsom_local_walk_with, as
//                                    masked_local_kernel), the <= 6 x 6 window and the post in one launch
// The validity row is J bytes read by every node group of a scan: it stays in cache, the scan remains bound by the 4 N D
// bytes of the map.  Nothing of size N x J is staged.
#include "vsom_online.hpp"
#include "vsom_masked_dist.hpp"
#include <cmath>
#include <algorithm>

// online_post (vsom_online.hip:185-205) on the masked distance; the chunk loop's form: no residual row, the hit counts
__device__ __forceinline__ void online_post_masked(const OnlineArgs &a, const float *x, const unsigned char *v, u64 bmu,
                                                   int lane, u64 *hits, u64 *lastbmu_out, float fB)
{
    const float dist = masked_group_dist(x, v, a.d.ma + (size_t)bmu * a.d.ldm, a.d.L, lane & 7);
    if (lane == 0) {
        a.fstate[0] = dist;
        float q = dist / fB;                 // residual.squaredNorm() / epochSize  (:1167)
        a.fstate[1] = a.fstate[1] + q;
        hits[bmu] += 1ull;                   // addBmu (:1165, :1189-1192)
        *lastbmu_out = bmu;                  // lastBMU = by*W + bx (:895)
    }
}

// online_node_update<KIND, BLOCK_SYNC> (vsom_online.hpp:58-148, the Standard / Median branch :125-146) with a validity byte
// per column: weightMap[n], scM, tw and twf are computed exactly as there (the node's weight counts the sample whatever its
// columns); a valid column gets the same float operations in the same order, an invalid one is neither stepped nor
// written.  v: the sample's packed validity row.  The workgroup form requests its first four elements before the barrier
// as the original does, the validity bytes with them: all of them travel in one round trip, and what was fetched for an
// invalid column is dropped.
template <int KIND, bool BLOCK_SYNC>
__device__ __forceinline__ void online_node_update_masked(size_t n, double h, int tid, int nthr, const float *__restrict__ xs,
                                                          const unsigned char *__restrict__ v, int D, int pitch, double eta,
                                                          int decay_fn, float *map, float *Smap, float *sigmap, float *weight)
{
    static_assert(KIND == VSOM_STANDARD || KIND == VSOM_MEDIAN, "the masked step is Standard / Median only");
    float *M = map + n * pitch, *S = Smap + n * pitch, *sg = sigmap + n * pitch;
    constexpr bool PRE = BLOCK_SYNC;
    float px[4], pm[4], ps[4];
    unsigned char pv[4];
    if (PRE) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = tid + u * nthr;
            const bool ok = d < D;
            pv[u] = ok ? v[d] : (unsigned char)0;
            px[u] = ok ? xs[d] : 0.f;
            pm[u] = ok ? M[d] : 0.f;
            ps[u] = ok ? S[d] : 0.f;
        }
    }
    const float wold = weight[n];
    float wnew, scM;
    if (decay_fn == VSOM_EXPONENTIAL) {
        wnew = wold + (float)(h * eta);              // :924
        scM = (float)(h * eta);                      // double scalar narrowed before the fp32 product :925
    } else {
        wnew = wold + (float)h;                      // :930
        double tw = wnew == 0 ? 1.0 : h / (double)wnew;   // :933
        scM = (float)tw;
    }
    const double tw2 = wnew == 0 ? 0.000001 : (double)wnew;   // :939
    const float twf = (float)tw2, hf = (float)h;
    if (BLOCK_SYNC)
        __syncthreads();   // every thread has read weight[n]
    if (tid == 0)
        weight[n] = wnew;

    for (int d = tid, u = 0; d < D; d += nthr, ++u) {
        const bool pre = PRE && u < 4;
        if (!(pre ? pv[u < 4 ? u : 0] : v[d]))
            continue;                                    // invalid: map, SMap and sigmaMap keep their bits
        const float x = pre ? px[u < 4 ? u : 0] : xs[d];
        float m = pre ? pm[u < 4 ? u : 0] : M[d];
        const float s_old = pre ? ps[u < 4 ? u : 0] : S[d];
        float dl = x - m;                                // Stepper :912
        if (KIND == VSOM_MEDIAN)
            dl = onl_sign(dl);
        float t = scM * dl;
        m = m + t;                                       // :925 / :935
        float dl2 = x - m;                               // Stepper(v, map_new) :941
        if (KIND == VSOM_MEDIAN)
            dl2 = onl_sign(dl2);
        float pr = dl * dl2;
        float uu = hf * pr;
        float s = s_old + uu;                            // :941
        M[d] = m;
        S[d] = s;
        sg[d] = sqrtf(fabsf(s / twf));                   // :942
    }
}

// a.d.xa: the sample's row, v its validity row; a.pxa, pv: those of the sample being finished
__global__ __launch_bounds__(256) void online_scan_masked_kernel(OnlineArgs a, const unsigned char *__restrict__ v,
                                                                 const unsigned char *__restrict__ pv, u64 *hits,
                                                                 u64 *lastbmu_out, float fB)
{
    __shared__ u64 skey[4];
    if (blockIdx.x == gridDim.x - 1) {
        if (a.do_post && threadIdx.x < 64) {
            const u64 bmu = online_resolve(a.state, a.par ^ 1);
            online_post_masked(a, a.pxa, pv, bmu, (int)threadIdx.x, hits, lastbmu_out, fB);
            if (threadIdx.x < ONL_SLOTS)
                *online_slot(a.state, a.par ^ 1, (int)threadIdx.x) = ~0ull;   // the key set of the sample after this one
        }
        return;
    }
    if (!a.do_scan)
        return;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int node = gid >> 3, k = threadIdx.x & 7;
    const int nc = node < a.N ? node : a.N - 1;
    const float d = masked_group_dist(a.d.xa, v, a.d.ma + (size_t)nc * a.d.ldm, a.d.L, k);
    u64 key = (node < a.N) ? vsom_key(d, (uint32_t)node) : ~0ull;
    if (node == 0 && k == 0)
        a.state[ONL_FLAG + a.par] = (d != d) ? 1ull : 0ull;
    // wave min, then block min, then one atomic per block
    for (int off = 32; off >= 8; off >>= 1) {
        u64 o = __shfl_xor(key, off);
        key = o < key ? o : key;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
        skey[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 m = skey[0];
        for (int i = 1; i < 4; ++i)
            m = skey[i] < m ? skey[i] : m;
        atomicMin(online_slot(a.state, a.par, (int)(blockIdx.x % ONL_SLOTS)), m);
    }
}

// one workgroup per node of the (maximal) window; nodes outside the actual window exit.  The next search launch (or the
// chunk's tail launch) finishes the sample.
template <int KIND>
__global__ __launch_bounds__(256) void online_window_masked_kernel(
    OnlineArgs a, const float *__restrict__ xs, const unsigned char *__restrict__ v, const double *__restrict__ lutd, int lutw,
    int D, int pitch, double eta, double sigma, int decay_fn, float *map, float *Smap, float *sigmap, float *weight)
{
    const u64 bmu = online_resolve(a.state, a.par);
    int bx, by;
    u64 startX, startY, endX, endY;
    online_window(bmu, a.W, a.H, sigma, bx, by, startX, startY, endX, endY);
    const u64 i = startX + blockIdx.x, j = startY + blockIdx.y;
    if (i >= endX || j >= endY)
        return;
    const size_t n = (size_t)(j * (u64)a.W + i);
    int dx = (int)i - bx, dy = (int)j - by;
    dx = dx < 0 ? -dx : dx;
    dy = dy < 0 ? -dy : dy;
    const double h = lutd[(size_t)dy * lutw + dx];   // calculateNeighbourhoodWeight(i,j,bx,by,sigma) :915
    online_node_update_masked<KIND, true>(n, h, threadIdx.x, blockDim.x, xs, v, D, pitch, eta, decay_fn, map, Smap, sigmap,
                                          weight);
}

// sigma <= 1: the whole step in one launch of one workgroup -- wave 0 walks the local search on the masked distance, each
// wave then updates window nodes round-robin, the wave that rewrote the BMU's row finishes the sample
template <int KIND>
__global__ __launch_bounds__(1024) void online_small_masked_kernel(
    OnlineArgs a, const float *__restrict__ xs, const unsigned char *__restrict__ v, const double *__restrict__ lutd, int lutw,
    int D, int pitch, double eta, double sigma, int decay_fn, float *map, float *Smap, float *sigmap, float *weight, u64 *hits,
    u64 *lastbmu_io, float fB)   // no __restrict__: a.d.ma aliases map, lastbmu_io is read and written
{
    __shared__ u64 sbmu;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave == 0) {
        u64 b;
        float dmin;
        vsom_local_walk_with(
            [&](u64 node, int k) { return masked_group_dist(a.d.xa, v, a.d.ma + (size_t)node * a.d.ldm, a.d.L, k); },
            (u64)a.W, (u64)a.H, *lastbmu_io, lane, b, dmin);
        if (lane == 0)
            sbmu = b;
    }
    __syncthreads();
    const u64 bmu = sbmu;
    int bx, by;
    u64 startX, startY, endX, endY;
    online_window(bmu, a.W, a.H, sigma, bx, by, startX, startY, endX, endY);
    const u64 nx = endX > startX ? endX - startX : 0, ny = endY > startY ? endY - startY : 0;
    for (u64 idx = (u64)wave; idx < nx * ny; idx += (u64)(blockDim.x >> 6)) {
        const u64 i = startX + idx % nx, j = startY + idx / nx;
        int dx = (int)i - bx, dy = (int)j - by;
        dx = dx < 0 ? -dx : dx;
        dy = dy < 0 ? -dy : dy;
        const double h = lutd[(size_t)dy * lutw + dx];
        const size_t n = (size_t)(j * (u64)a.W + i);
        online_node_update_masked<KIND, false>(n, h, lane, 64, xs, v, D, pitch, eta, decay_fn, map, Smap, sigmap, weight);
        if (n == (size_t)bmu) {
            __threadfence_block();
            online_post_masked(a, a.d.xa, v, bmu, lane, hits, lastbmu_io, fB);
        }
    }
    // sigma < 0.4 truncates the window to nothing (:899-903): the BMU is not updated, the sample still counts
    const bool inside = (u64)bx >= startX && (u64)bx < endX && (u64)by >= startY && (u64)by < endY;
    if (!inside && wave == 0)
        online_post_masked(a, a.d.xa, v, bmu, lane, hits, lastbmu_io, fB);
}

// The chunk loop: B samples in load order, each with its packed validity row (vp + j * xpitch, or vp for every sample with
// `one`).  The caller has run online_init_kernel; enqueues only.
int enqueue_chunk_masked(vsom_ctx *c, double eta, double sigma, int decay_fn, const double *lutd, int lutw,
                         const unsigned char *vp, bool one)
{
    const size_t B = c->B, vld = one ? 0 : c->xpitch;
    const float fB = (float)B;
    const bool median = c->transform == VSOM_MEDIAN;
    const int D = (int)c->D, pitch = (int)c->pitch;
    if (!(sigma > 1)) {   // SIGMA_SWITCH_TO_LOCAL (SOM.hpp:37, Som.cpp:891)
        const auto k = median ? online_small_masked_kernel<VSOM_MEDIAN> : online_small_masked_kernel<VSOM_STANDARD>;
        for (size_t j = 0; j < B; ++j) {
            const float *xs = c->Xs.p + j * c->xpitch;
            const OnlineArgs a = vsom_onl_args(c, xs, nullptr, nullptr);
            hipLaunchKernelGGL(k, dim3(1), dim3(1024), 0, c->stream, a, xs, vp + j * vld, lutd, lutw, D, pitch, eta, sigma,
                               decay_fn, c->map.p, c->S.p, c->sigma.p, c->weight.p, c->hits.p, c->lastbmu.p + j, fB);
        }
        return VSOM_OK;
    }
    // the grids of enqueue_single (vsom_online.hip): the scan's workgroups + the one that finishes sample j-1; the maximal
    // window extents trunc(b+2.5s) - trunc(b-2.5s) <= floor(5s)+1, clipped to the map
    const unsigned sgrid = (unsigned)(((size_t)c->N * 8 + 255) / 256) + 1u;
    const double ext = std::floor(5.0 * sigma) + 2.0;
    const unsigned gx = (unsigned)std::min<double>((double)c->W, ext), gy = (unsigned)std::min<double>((double)c->H, ext);
    const dim3 wgrid(gx ? gx : 1, gy ? gy : 1);
    int bs = D >= 256 ? 256 : ((D + 63) / 64) * 64;
    if (bs < 64)
        bs = 64;
    const auto wk = median ? online_window_masked_kernel<VSOM_MEDIAN> : online_window_masked_kernel<VSOM_STANDARD>;
    const float *pxs = nullptr;
    const unsigned char *pv = nullptr;
    for (size_t j = 0; j < B; ++j) {
        const float *xs = c->Xs.p + j * c->xpitch;
        const unsigned char *v = vp + j * vld;
        OnlineArgs a = vsom_onl_args(c, xs, nullptr, nullptr);
        a.par = (int)(j & 1);
        a.pxa = a.pxb = pxs;
        a.do_post = j > 0;
        hipLaunchKernelGGL(online_scan_masked_kernel, dim3(sgrid), dim3(256), 0, c->stream, a, v, pv, c->hits.p,
                           j ? c->lastbmu.p + (j - 1) : nullptr, fB);
        hipLaunchKernelGGL(wk, wgrid, dim3(bs), 0, c->stream, a, xs, v, lutd, lutw, D, pitch, eta, sigma, decay_fn, c->map.p,
                           c->S.p, c->sigma.p, c->weight.p);
        pxs = xs;
        pv = v;
    }
    if (B > 0) {          // the chunk's tail: finish its last sample; no search
        OnlineArgs a = vsom_onl_args(c, pxs, nullptr, nullptr);
        a.par = (int)((B - 1) & 1) ^ 1;      // the post workgroup works on parity par ^ 1
        a.pxa = a.pxb = pxs;
        a.do_scan = 0;
        a.do_post = 1;
        hipLaunchKernelGGL(online_scan_masked_kernel, dim3(1), dim3(256), 0, c->stream, a, pv, pv, c->hits.p,
                           c->lastbmu.p + (B - 1), fB);
    }
    return VSOM_OK;
}
