// vsom_online.hip -- online path: Som::trainSingle (Som.cpp:885-947) and the per-chunk loop of
// Som::trainBasicSom (Som.cpp:1159-1171) on gfx950.  This file is the index of the family; its siblings:
//   vsom_online.hpp       what the files share: the onl_state layout, OnlineArgs, the window update of one node
//   vsom_online_i8.hip    the image-bounded search of the chunk loop (sigma > 1, Standard / Median): onl_fused_kernel,
//                         onl_refine_kernel and their per-chunk passes, enqueue_chunk_i8, vsom_get_online_search_stats
//   vsom_online_tiny.hip  tiny maps: the whole chunk loop in one launch of one workgroup, plain (online_tiny_chunk_kernel)
//                         and over the valid entries of the rows only (online_tiny_masked_chunk_kernel), and one
//                         workgroup per map for ensembles (vsom_onl_tiny_*)
//   vsom_online_masked.hip the chunk loop over the valid entries of the rows only (Standard / Median): the masked scan,
//                         window and one-launch step of vsom_train_online_chunk_masked, enqueue_chunk_masked
//   vsom_single.hip       single-vector queries: vsom_find_bmu, vsom_find_restricted_bmu, vsom_distances_single,
//                         vsom_dist_single, vsom_find_local_bmu; stage_single
// Here: the per-sample kernels, the neighbourhood tables (lutd), and the entry points vsom_train_online_chunk* (which pick
// one of the four chunk loops) and vsom_train_single.
//
// The path is strictly sequential in samples (sample j's BMU search reads the map sample j-1
// wrote), so one sample = two launches (sigma > 1) or one (sigma <= 1) enqueued back to back on
// the context stream, without host synchronisation:
//   online_scan_kernel    sigma > 1: Som::findBmu, 8 lanes per node (one per Eigen accumulator
//                         class), atomicMin on an order-preserving (distance, index) key.  Key and node-0-NaN flag are double-buffered by
//                         sample parity, so no launch is needed to resolve / re-arm them.
//   online_window_kernel  the +-2.5 sigma window (Som.cpp:899-944): one workgroup per window
//                         node, elementwise over the model vector; weightMap / map / SMap /
//                         sigmaMap updated with the reference's double->float narrowing (Q11).
//                         The workgroup that owns the BMU node then does the post step: residual
//                         + distance of the BMU after the update (:946), addBmu (:1189-1192), MSE
//                         running sum (:1167), lastBMU (:895), re-arming the other parity's key.
//   online_small_kernel   sigma <= 1: Som::findLocalBmu + <=6x6 window + post in one launch of one
//                         1024-thread workgroup (16 wavefronts share the window's nodes: 15.0 vs 17.9 us
//                         with 4; staging the walk's candidate rows through LDS was measured slower, 20 us)
// The bandwidth roofline of one sample is 4*N*D (scan) + 20*k*D (k window nodes) bytes.
#include "vsom_online.hpp"
#include <cmath>
#include <algorithm>
#include <cstring>

template <bool CLR>
__device__ __forceinline__ void online_post(const OnlineArgs &a, const float *xa, const float *xb, u64 bmu, int lane, u64 *hits,
                                            u64 *lastbmu_out, float *residual, float fB, int add_hit);

// POSTWG: the chunk loop's form.  The LAST workgroup does not search: it finishes the PREVIOUS sample (residual and
// distance of its BMU after the window update :946, addBmu, MSE, lastBMU) and re-arms that sample's key set -- 2-3 us of
// dependent row reads that used to sit at the end of the window launch's critical path, now hidden beside the 9.6 us
// search (the window launch of the previous sample has completed: kernel boundary; the next window launch has not
// started).  After the last sample of a chunk the kernel is launched once more with do_scan = 0.
template <bool CLR, bool POSTWG>
__global__ __launch_bounds__(256) void online_scan_kernel(OnlineArgs a, u64 *hits, u64 *lastbmu_out, float fB, int add_hit)
{
    __shared__ u64 skey[4];
    if (POSTWG && blockIdx.x == gridDim.x - 1) {
        if (a.do_post && threadIdx.x < 64) {
            const u64 bmu = online_resolve(a.state, a.par ^ 1);
            online_post<CLR>(a, a.pxa, a.pxb, bmu, (int)threadIdx.x, hits, lastbmu_out, nullptr, fB, add_hit);
            if (threadIdx.x < ONL_SLOTS)
                *online_slot(a.state, a.par ^ 1, (int)threadIdx.x) = ~0ull;   // the key set of the sample after this one
        }
        return;
    }
    if (POSTWG && !a.do_scan)
        return;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int node = gid >> 3, k = threadIdx.x & 7;
    const int nc = node < a.N ? node : a.N - 1;
    float d = vsom_group_dist<CLR, VSOM_SCAN_UNR>(a.d.xa, a.d.xb, a.d.ma + (size_t)nc * a.d.ldm,
                                                  a.d.mb + (size_t)nc * a.d.ldm, a.d.L, k);
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

// g-th candidate of the walk's first step: the 8 neighbours of `from`, wrap-then-clamp (Som.cpp:362-385)
__device__ __forceinline__ u64 online_first_try_node(u64 from, int g, u64 width, u64 height)
{
    const u64 m1 = ~0ull;
    const u64 fsx = (g == 0 || g >= 6) ? m1 : ((g == 1 || g == 5) ? 0ull : 1ull);
    const u64 fsy = (g <= 2) ? 1ull : ((g == 3 || g == 7) ? 0ull : m1);
    u64 cx = from % width + fsx;
    cx = cx < width - 1 ? cx : width - 1;
    u64 cy = from / width + fsy;
    cy = cy < height - 1 ? cy : height - 1;
    return cy * width + cx;
}

// single-sample Som::findLocalBmu (same walk as bmu_local_kernel in vsom_bmu.hip).  The distance of
// the starting node (own) and of the first step's 8 neighbours (dfirst, one per lane group) do not
// depend on each other; the caller may have them evaluated side by side by two wavefronts and pass
// them in (own != nullptr), which takes one of the walk's latency-bound distance passes off its path.
template <bool CLR>
__device__ __forceinline__ u64 online_local_search(const OnlineArgs &a, const u64 *lastbmu, int lane,
                                                   const float *own = nullptr, float dfirst = 0.f)
{
    const int g = lane >> 3, k = lane & 7;
    const u64 width = (u64)a.W, height = (u64)a.H;
    const float *xa = a.d.xa, *xb = a.d.xb;
    u64 lastBMU = *lastbmu;
    float minDist;
    if (own) {
        minDist = *own;
    } else {
        minDist = vsom_group_dist_lat<CLR>(xa, xb, a.d.ma + (size_t)lastBMU * a.d.ldm,
                                           a.d.mb + (size_t)lastBMU * a.d.ldm, a.d.L, k);
        minDist = __shfl(minDist, 0);
    }
    bool precomputed = own != nullptr;
    u64 minIndex = lastBMU, lastMeasured = lastBMU;
    for (;;) {
        const u64 lmX = lastMeasured % width, lmY = lastMeasured / width;
        const u64 lbX = lastBMU % width;
        if (lastMeasured == lastBMU) {
            const u64 node = online_first_try_node(lastMeasured, g, width, height);
            float d;
            if (precomputed) {
                d = dfirst;
                precomputed = false;
            } else {
                d = vsom_group_dist_lat<CLR>(xa, xb, a.d.ma + (size_t)node * a.d.ldm,
                                             a.d.mb + (size_t)node * a.d.ldm, a.d.L, k);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float di = __shfl(d, i * 8);
                u64 ni = __shfl(node, i * 8);
                if (di < minDist) {
                    minDist = di;
                    minIndex = ni;
                }
            }
            if (minIndex == lastBMU)
                break;
            lastMeasured = minIndex;
        } else {
            if (lmX - lbX) {
                u64 cx = lmX + lmX - lbX;
                cx = cx < width - 1 ? cx : width - 1;
                u64 off = (u64)(long long)((g < 3 ? g : 0) - 1);
                u64 cy = lmY + off;
                cy = cy < height - 1 ? cy : height - 1;
                u64 node = cy * width + cx;
                float d = vsom_group_dist_lat<CLR>(xa, xb, a.d.ma + (size_t)node * a.d.ldm,
                                               a.d.mb + (size_t)node * a.d.ldm, a.d.L, k);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    float di = __shfl(d, i * 8);
                    u64 ni = __shfl(node, i * 8);
                    if (di < minDist) {
                        minDist = di;
                        minIndex = ni;
                    }
                }
            }
            if (minIndex == lastMeasured)
                break;
            lastBMU = lastMeasured;
            lastMeasured = minIndex;
        }
    }
    return minIndex;   // identical in every lane
}

// residual / distance of the BMU after the update (:946), addBmu, MSE, lastBMU
template <bool CLR>
__device__ __forceinline__ void online_post(const OnlineArgs &a, const float *xa, const float *xb, u64 bmu, int lane, u64 *hits,
                                            u64 *lastbmu_out, float *residual, float fB, int add_hit)
{
    const int k = lane & 7;
    const float *ma = a.d.ma + (size_t)bmu * a.d.ldm, *mb = a.d.mb + (size_t)bmu * a.d.ldm;
    if (residual) {
        for (int d = lane; d < a.d.L; d += 64)
            residual[d] = vsom_resid<CLR>(xa[d], CLR ? xb[d] : 0.f, ma[d], CLR ? mb[d] : 0.f);
    }
    float dist = vsom_group_dist_lat<CLR>(xa, xb, ma, mb, a.d.L, k);
    if (lane == 0) {
        a.fstate[0] = dist;
        float q = dist / fB;                 // residual.squaredNorm() / epochSize  (:1167)
        a.fstate[1] = a.fstate[1] + q;
        if (add_hit)
            hits[bmu] += 1ull;               // addBmu (:1165, :1189-1192)
        *lastbmu_out = bmu;                  // lastBMU = by*W + bx (:895)
    }
}

// one workgroup per node of the (maximal) window; nodes outside the actual window exit.  The
// workgroup of the BMU node finishes the sample (post step) once its own update is visible.
template <int KIND, bool POST>
__global__ __launch_bounds__(256) void online_window_kernel(
    OnlineArgs a, const float *__restrict__ xs, const float *__restrict__ xp, const float *__restrict__ yp,
    const double *__restrict__ lutd, int lutw, int D, int P, int ppitch, int pitch, double eta, double sigma,
    int decay_fn, float *map, float *Smap, float *sigmap, float *weight, u64 *hits, u64 *lastbmu_out,
    float *residual, float fB, int add_hit)   // no __restrict__: a.d.ma aliases map
{
    constexpr bool CLR = KIND == VSOM_CLR;
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
    online_node_update<KIND, true>(n, h, threadIdx.x, blockDim.x, xs, xp, yp, D, P, ppitch, pitch, eta, decay_fn,
                                   map, Smap, sigmap, weight);
    if (!POST || n != (size_t)bmu)   // (chunk loop: the next search launch finishes the sample; the BMU always lies inside
        return;                      //  its own window, sigma > 1)
    __syncthreads();             // this workgroup's writes of the BMU row are visible to its wave 0
    if (threadIdx.x < 64) {
        online_post<CLR>(a, a.d.xa, a.d.xb, bmu, threadIdx.x, hits, lastbmu_out, residual, fB, add_hit);
        if (threadIdx.x < ONL_SLOTS)
            *online_slot(a.state, a.par ^ 1, (int)threadIdx.x) = ~0ull;   // arm the next sample's key (nobody reads it during this launch)
    }
}

// sigma <= 1 (Som.cpp:891: findLocalBmu, indicator neighbourhood, window of at most 6x6 nodes):
// the whole trainSingle step in ONE small launch -- wave 0 walks the local search, each wave then
// updates window nodes round-robin, wave 0 finishes with the residual / bookkeeping.
template <int KIND>
__global__ __launch_bounds__(1024) void online_small_kernel(
    OnlineArgs a, const float *__restrict__ xs, const float *__restrict__ xp, const float *__restrict__ yp,
    const double *__restrict__ lutd, int lutw, int D, int P, int ppitch, int pitch, double eta, double sigma,
    int decay_fn, float *map, float *Smap, float *sigmap, float *weight, u64 *hits, u64 *lastbmu_io,
    float *residual, float fB, int add_hit)   // no __restrict__: a.d.ma aliases map, lastbmu_io is read and written
{
    constexpr bool CLR = KIND == VSOM_CLR;
    __shared__ u64 sbmu;
    __shared__ float sown;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the walk's starting distance (wavefront 1) beside its first step's 8 neighbours (wavefront 0)
    float dfirst = 0.f;
    if (wave <= 1) {
        const u64 from = *lastbmu_io;
        const u64 node = wave == 0 ? online_first_try_node(from, lane >> 3, (u64)a.W, (u64)a.H) : from;
        const float d = vsom_group_dist_lat<CLR>(a.d.xa, a.d.xb, a.d.ma + (size_t)node * a.d.ldm,
                                                 a.d.mb + (size_t)node * a.d.ldm, a.d.L, lane & 7);
        if (wave == 0)
            dfirst = d;
        else if (lane == 0)
            sown = d;
    }
    __syncthreads();
    if (wave == 0) {
        const u64 b = online_local_search<CLR>(a, lastbmu_io, lane, &sown, dfirst);
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
        online_node_update<KIND, false>(n, h, lane, 64, xs, xp, yp, D, P, ppitch, pitch,
                                        eta, decay_fn, map, Smap, sigmap, weight);
        if (n == (size_t)bmu) {        // the wavefront that rewrote the BMU's row finishes the sample while
            __threadfence_block();     // the others update their nodes
            online_post<CLR>(a, a.d.xa, a.d.xb, bmu, lane, hits, lastbmu_io, residual, fB, add_hit);
        }
    }
    // sigma < 0.4 truncates the window to nothing (:899-903): the BMU is not updated, the sample still counts
    const bool inside = (u64)bx >= startX && (u64)bx < endX && (u64)by >= startY && (u64)by < endY;
    if (!inside && wave == 0)
        online_post<CLR>(a, a.d.xa, a.d.xb, bmu, lane, hits, lastbmu_io, residual, fB, add_hit);
}

__global__ void online_init_kernel(u64 *state, float *fstate, int keep_mse)
{
    for (int s = 0; s < 2 * ONL_SLOTS; ++s)
        state[s * 16] = ~0ull;
    state[ONL_FLAG] = 0ull;
    state[ONL_FLAG + 1] = 0ull;
    fstate[0] = 0.f;
    if (!keep_mse)
        fstate[1] = 0.f;   // else: the epoch's running MSE continues across chunks (Som.cpp:1153,1167)
}

// double-precision table of calculateNeighbourhoodWeight for the online path (the batch path uses its float cast), cached per
// sigma.  The schedule changes sigma every epoch (Som.cpp:1146), so a training run builds one table per epoch: the host image
// goes into one of two pinned slots and from there to the device by a copy ENQUEUED on the stream -- ordered behind the
// kernels that still read the previous table, no stream wait, no pageable staging (a synchronous copy was ~20 us of the
// 10 x 10 x 9 scenario's epoch).
int ensure_lutd_host(vsom_ctx *c, double sigma, const double **out, int *slot_out)
{
    const uint32_t lw = c->W, lh = c->H;
    const size_t need = (size_t)lw * lh;
    if (2 * need > c->lutd_host.cap) {
        VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
        VSOM_ALLOC_CHECK(vsom_grow(c->lutd_host, 2 * need, c->stream));
        c->lutd_host_sigma[0] = c->lutd_host_sigma[1] = -1.0;
        c->lutd_ev_valid[0] = c->lutd_ev_valid[1] = false;
    }
    for (int k = 0; k < 2; ++k)
        if (c->lutd_host_sigma[k] == sigma) {
            *out = c->lutd_host.p + (size_t)k * need;
            *slot_out = k;
            return VSOM_OK;
        }
    const int k = c->lutd_slot ^= 1;
    if (!c->lutd_ev[k])
        VSOM_HIP_CHECK(hipEventCreateWithFlags(&c->lutd_ev[k], hipEventDisableTiming));
    if (c->lutd_ev_valid[k])
        VSOM_HIP_CHECK(hipEventSynchronize(c->lutd_ev[k]));      // its last reader (two tables ago): long done
    double *host = c->lutd_host.p + (size_t)k * need;
    c->lutd_host_sigma[k] = -1.0;
    for (uint32_t dy = 0; dy < lh; ++dy)
        for (uint32_t dx = 0; dx < lw; ++dx)
            host[(size_t)dy * lw + dx] = vsom_neighbourhood_weight(dx, dy, 0, 0, sigma);
    c->lutd_host_sigma[k] = sigma;
    *out = host;
    *slot_out = k;
    return VSOM_OK;
}

// (behind the last enqueued reader of host slot k)
static int lutd_host_used(vsom_ctx *c, int k)
{
    VSOM_HIP_CHECK(hipEventRecord(c->lutd_ev[k], c->stream));
    c->lutd_ev_valid[k] = true;
    return VSOM_OK;
}

static int ensure_lutd(vsom_ctx *c, double sigma, const double **out, int *lutw)
{
    const uint32_t lw = c->W, lh = c->H;
    const size_t need = (size_t)lw * lh;
    *lutw = (int)lw;
    if (c->lutd.p && c->lutd_sigma == sigma) {
        *out = c->lutd.p;
        return VSOM_OK;
    }
    VSOM_ALLOC_CHECK(vsom_grow(c->lutd, need, c->stream, VSOM_BUF_SYNC));
    const double *host = nullptr;
    int k = 0;
    if (int rc = ensure_lutd_host(c, sigma, &host, &k))
        return rc;
    c->lutd_sigma = -1.0;
    VSOM_HIP_CHECK(hipMemcpyAsync(c->lutd.p, host, need * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (int rc = lutd_host_used(c, k))
        return rc;
    c->lutd_sigma = sigma;
    *out = c->lutd.p;
    return VSOM_OK;
}

// the kernel arguments of one sample, and the one launcher of the scan (both described in vsom_online.hpp)
OnlineArgs vsom_onl_args(const vsom_ctx *c, const float *xs, const float *xp, const float *yp)
{
    const bool clr = c->transform == VSOM_CLR;
    OnlineArgs a;
    a.d = vsom_dist_args(c);       // the model rows; the sample is ONE row, not the staged chunk
    a.d.xa = clr ? xp : xs;
    a.d.xb = clr ? yp : xs;
    a.d.ldx = 0;
    a.state = c->onl_state.p;
    a.fstate = c->onl_f.p;         // {distance of the BMU, MSE running sum}
    a.N = (int)c->N;
    a.W = (int)c->W;
    a.H = (int)c->H;
    a.par = 0;
    a.pxa = a.pxb = nullptr;
    a.do_scan = 1;
    a.do_post = 0;
    return a;
}

void launch_online_scan(vsom_ctx *c, const OnlineArgs &a, bool postwg, unsigned grid, u64 *lastbmu_out, float fB, int add_hit)
{
    const bool clr = c->transform == VSOM_CLR;
    auto *k = postwg ? (clr ? online_scan_kernel<true, true> : online_scan_kernel<false, true>)
                     : (clr ? online_scan_kernel<true, false> : online_scan_kernel<false, false>);
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, c->stream, a, c->hits.p, lastbmu_out, fB, add_hit);
}

// enqueue one trainSingle on sample rows (xs / xp / yp), lastBMU in/out at `lastbmu_dev`
// chunk = true: the chunk loop's pipelined form (sigma > 1) -- this search launch also finishes the PREVIOUS sample
// (rows pxs / pxp / pyp, lastBMU out at lastbmu_dev - 1; j = 0: nothing to finish) and the window launch leaves its own
// sample unfinished; the caller ends the chunk with enqueue_chunk_tail
static int enqueue_single(vsom_ctx *c, const float *xs, const float *xp, const float *yp,
                          double eta, double sigma, int decay_fn, u64 *lastbmu_dev,
                          float *residual_dev, float fB, int add_hit, const double *lutd, int lutw, int par,
                          float *fstate = nullptr, bool chunk = false, const float *pxs = nullptr, const float *pxp = nullptr,
                          const float *pyp = nullptr)
{
    OnlineArgs a = vsom_onl_args(c, xs, xp, yp);
    a.par = par & 1;
    const bool clr = c->transform == VSOM_CLR;
    a.pxa = clr ? pxp : pxs;
    a.pxb = clr ? pyp : pxs;
    a.do_post = chunk && pxs != nullptr;
    if (fstate)
        a.fstate = fstate;

    if (sigma > 1) {   // SIGMA_SWITCH_TO_LOCAL (SOM.hpp:37, Som.cpp:891)
        const unsigned grid = (unsigned)(((size_t)c->N * 8 + 255) / 256) + (chunk ? 1u : 0u);   // + the workgroup that finishes sample j-1
        u64 *lb_prev = chunk && lastbmu_dev ? lastbmu_dev - 1 : nullptr;
        launch_online_scan(c, a, chunk, grid, lb_prev, fB, add_hit);
    } else {
        // sigma <= 1: one fused launch (local search + <=6x6 window + post)
#define LAUNCH_SMALL(KIND)                                                                                  \
    hipLaunchKernelGGL(online_small_kernel<KIND>, dim3(1), dim3(1024), 0, c->stream, a, xs, xp, yp, lutd, lutw, \
                       (int)c->D, (int)c->part_len, (int)c->part_pitch, (int)c->pitch, eta, sigma, decay_fn, \
                       c->map.p, c->S.p, c->sigma.p, c->weight.p, c->hits.p, lastbmu_dev, residual_dev, fB, add_hit)
        if (c->transform == VSOM_CLR)
            LAUNCH_SMALL(VSOM_CLR);
        else if (c->transform == VSOM_MEDIAN)
            LAUNCH_SMALL(VSOM_MEDIAN);
        else
            LAUNCH_SMALL(VSOM_STANDARD);
#undef LAUNCH_SMALL
        return VSOM_OK;
    }
    // maximal window extents: trunc(b+2.5s) - trunc(b-2.5s) <= floor(5s)+1, clipped to the map
    double ext = std::floor(5.0 * sigma) + 2.0;
    unsigned gx = (unsigned)std::min<double>((double)c->W, ext), gy = (unsigned)std::min<double>((double)c->H, ext);
    dim3 wgrid(gx ? gx : 1, gy ? gy : 1);
    const int L = (int)c->part_len;
    int bs = L >= 256 ? 256 : ((L + 63) / 64) * 64;
    if (bs < 64)
        bs = 64;
#define LAUNCH_WIN(KIND, POST)                                                                              \
    hipLaunchKernelGGL((online_window_kernel<KIND, POST>), wgrid, dim3(bs), 0, c->stream, a, xs, xp, yp, lutd, lutw, \
                       (int)c->D, (int)c->part_len, (int)c->part_pitch, (int)c->pitch, eta, sigma, decay_fn, \
                       c->map.p, c->S.p, c->sigma.p, c->weight.p, c->hits.p, lastbmu_dev, residual_dev, fB, add_hit)
    if (chunk) {
        if (c->transform == VSOM_CLR)
            LAUNCH_WIN(VSOM_CLR, false);
        else if (c->transform == VSOM_MEDIAN)
            LAUNCH_WIN(VSOM_MEDIAN, false);
        else
            LAUNCH_WIN(VSOM_STANDARD, false);
    } else {
        if (c->transform == VSOM_CLR)
            LAUNCH_WIN(VSOM_CLR, true);
        else if (c->transform == VSOM_MEDIAN)
            LAUNCH_WIN(VSOM_MEDIAN, true);
        else
            LAUNCH_WIN(VSOM_STANDARD, true);
    }
#undef LAUNCH_WIN
    return VSOM_OK;
}

// end of a pipelined chunk (sigma > 1): finish its last sample (rows pxs / pxp / pyp, parity par_last); no search
static int enqueue_chunk_tail(vsom_ctx *c, const float *pxs, const float *pxp, const float *pyp, u64 *lastbmu_last, float fB,
                              int par_last)
{
    OnlineArgs a = vsom_onl_args(c, pxs, pxp, pyp);
    a.par = (par_last & 1) ^ 1;      // the post workgroup works on parity par ^ 1
    a.pxa = a.d.xa;
    a.pxb = a.d.xb;
    a.do_scan = 0;
    a.do_post = 1;
    launch_online_scan(c, a, true, 1, lastbmu_last, fB, 1);
    return VSOM_OK;
}

extern "C" {

// lb_host != NULL: the caller wants lastBMU back in this call -- *lb_in_pinned = the one-launch kernel has stored it into
// c->out_pinned.p itself (else the caller fetches it with vsom_get_last_bmu)
// masked: vsom_train_online_chunk_masked -- the same preamble with the validity bytes valid_host (B x J, or J with one_mask)
// copied into the query arena, then one of two loops: where vsom_online_masked_tiny_applies holds, the one-launch chunk of
// vsom_online_tiny.hip, which reads those bytes as they are (one H2D copy and one launch; lastBMU and the MSE come
// back through pinned memory as in the unmasked call); otherwise the exact-scan loop of vsom_online_masked.hip over their
// packed copy.  member: the caller is the ensemble the context has joined (vsom_online_chunk_masked_member).
static int train_online_chunk_impl(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk, float *mse_out,
                                   bool want_lb, bool *lb_in_pinned, bool masked = false, const uint8_t *valid_host = nullptr,
                                   int one_mask = 0, bool member = false)
{
    if (lb_in_pinned)
        *lb_in_pinned = false;
    CHECK_CTX_NOJOIN(c);
    if (masked) {
        VSOM_CUSTOM_REFUSE(c, "vsom_train_online_chunk_masked");
        if (c->transform == VSOM_CLR)
            return vsom_fail(VSOM_ERR_INVALID, "vsom_train_online_chunk_masked: CLR contexts are not supported (residual and step run over column pairs)");
        if (c->in_group || (c->sigma_shared && !member))
            return vsom_fail(VSOM_ERR_INVALID, "vsom_train_online_chunk_masked: the context has joined a group or an ensemble");
        if (!valid_host)
            return vsom_fail(VSOM_ERR_INVALID, "valid_host is null");
    }
    if (c->cu) {
        int rc = vsom_custom_train_online_chunk(c, eta, sigma, decay_fn, first_chunk);
        if (rc || !mse_out)
            return rc;
        VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
        *mse_out = *static_cast<volatile float *>(c->mse.p);
        return VSOM_OK;
    }
    // CHECK_CTX and CHECK_ROWS in pieces: a custom context leaves above, before the join, and rows_free_valid is cleared only
    // behind the argument checks, so a call refused for its arguments or its chunk does not clear it
    if (int jrc = vsom_join_aux(c))
        return jrc;
    if (decay_fn != VSOM_EXPONENTIAL && decay_fn != VSOM_INVERSE_PROPORTIONAL)
        return vsom_fail(VSOM_ERR_INVALID, "online training needs Exponential or InverseProportional");
    if (!c->chunk_loaded)   // an empty chunk is a no-op for the sample loop (Som.cpp:1161)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    CHECK_ROWS(c);
    c->rows_free_valid = false;   // (the chunk below reads the staged rows, a later stage-ahead must not take them)
    const double *lutd = nullptr;
    int lutw = (int)c->W, lslot = 0, rc;
    const bool tiny_masked = masked && vsom_online_masked_tiny_applies(c, sigma, one_mask);
    bool tiny = tiny_masked || (!masked && online_tiny_applies(c, sigma));
    if (tiny)                                 // one launch reads the table once, into LDS: straight from the pinned slot
        rc = ensure_lutd_host(c, sigma, &lutd, &lslot);
    else
        rc = ensure_lutd(c, sigma, &lutd, &lutw);
    if (rc)
        return rc;
    const bool one = one_mask != 0;
    const unsigned char *packed = nullptr, *vraw = nullptr;
    if (masked && c->B > 0) {     // the validity bytes as given and, for the loop, packed (0xFF / 0x00, xpitch a row), before any kernel
        const size_t vrows = one ? 1 : c->B;
        vsom_layout lay;
        const auto raw = lay.add<unsigned char>(vrows * c->J);
        const auto pk = lay.add<unsigned char>(tiny_masked ? 0 : vrows * c->xpitch);   // (the one-launch chunk needs no packed copy)
        VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
        TimerScope ts(c, VSOM_T_STAGE);
        VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(raw), valid_host, vrows * c->J, hipMemcpyHostToDevice, c->stream));
        vraw = lay.at(raw);
        if (!tiny_masked) {
            vsom_masked_pack_enqueue(c, lay.at(raw), vrows, lay.at(pk));
            VSOM_HIP_CHECK(hipGetLastError());
            packed = lay.at(pk);
        }
    }
    {
        TimerScope ts(c, VSOM_T_ONLINE);
        if (!tiny)                            // (the one-launch chunk starts the running MSE itself and uses no key slots)
            hipLaunchKernelGGL(online_init_kernel, dim3(1), dim3(1), 0, c->stream, c->onl_state.p, c->onl_f.p,
                               first_chunk ? 0 : 1);
        if (tiny) {
            u64 *lbh = nullptr;
            if (want_lb && c->B <= 8192) {
                VSOM_ALLOC_CHECK(vsom_grow(c->out_pinned, 8192, c->stream));
                lbh = c->out_pinned.p;
            }
            rc = enqueue_chunk_tiny(c, eta, sigma, decay_fn, lutd, lutw, first_chunk, lbh, tiny_masked ? vraw : nullptr, one);
            if (rc || (rc = lutd_host_used(c, lslot)))
                return rc;
            if (lbh && lb_in_pinned)
                *lb_in_pinned = true;
        } else if (masked) {
            if ((rc = enqueue_chunk_masked(c, eta, sigma, decay_fn, lutd, lutw, packed, one)))
                return rc;
        } else if (onl_i8_applies(c, sigma)) {
            if ((rc = enqueue_chunk_i8(c, eta, sigma, decay_fn, lutd, lutw)))
                return rc;
        } else {
            const float fB = (float)c->B;
            const bool pipelined = sigma > 1;     // the search launch of sample j finishes sample j-1 (online_scan_kernel)
            const float *pxs = nullptr, *pxp = nullptr, *pyp = nullptr;
            for (size_t j = 0; j < c->B; ++j) {
                const float *xs = c->Xs.p + j * c->xpitch;
                const float *xp = c->XP.p ? c->XP.p + j * c->part_pitch : nullptr;
                const float *yp = c->YP.p ? c->YP.p + j * c->part_pitch : nullptr;
                rc = enqueue_single(c, xs, xp, yp, eta, sigma, decay_fn, c->lastbmu.p + j, nullptr, fB, 1,
                                    lutd, lutw, (int)(j & 1), nullptr, pipelined, pxs, pxp, pyp);
                if (rc)
                    return rc;
                pxs = xs;
                pxp = xp;
                pyp = yp;
            }
            if (pipelined && c->B > 0 &&
                (rc = enqueue_chunk_tail(c, pxs, pxp, pyp, c->lastbmu.p + (c->B - 1), fB, (int)((c->B - 1) & 1))))
                return rc;
        }
        VSOM_HIP_CHECK(hipGetLastError());
    }
    // vsom_get_mse reports the chunk's MSE for callers that passed mse_out = NULL (asynchronous use)
    if (!tiny)
        VSOM_HIP_CHECK(hipMemcpyAsync(c->mse.p, c->onl_f.p + 1, 4, hipMemcpyDefault, c->stream));   // (c->mse.p: pinned host memory)
    if (mse_out) {
        VSOM_HIP_CHECK(hipMemcpyAsync(mse_out, c->onl_f.p + 1, 4, hipMemcpyDeviceToHost, c->stream));
        VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    return VSOM_OK;
}

int vsom_train_online_chunk_acc(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk,
                                float *mse_out)
{
    return train_online_chunk_impl(c, eta, sigma, decay_fn, first_chunk, mse_out, false, nullptr);
}

// the chunk is enqueued: one stream wait, lastBMU (in_pinned: the one-launch kernel stored it into c->out_pinned) and the MSE
static int online_chunk_fetch(vsom_ctx *c, bool in_pinned, uint64_t *lastbmu_out, float *mse_out)
{
    int rc;
    if (lastbmu_out && !in_pinned) {
        if ((rc = vsom_get_last_bmu(c, lastbmu_out)))      // (synchronises)
            return rc;
    } else {
        VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (lastbmu_out)
            std::memcpy(lastbmu_out, c->out_pinned.p, c->B * sizeof(uint64_t));
    }
    if (mse_out)
        *mse_out = *static_cast<volatile float *>(c->mse.p);  // pinned host memory; written in stream order before the wait above
    return VSOM_OK;
}

int vsom_train_online_chunk_fetch(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk,
                                  uint64_t *lastbmu_out, float *mse_out)
{
    bool in_pinned = false;
    if (int rc = train_online_chunk_impl(c, eta, sigma, decay_fn, first_chunk, nullptr, lastbmu_out != nullptr, &in_pinned))
        return rc;
    return online_chunk_fetch(c, in_pinned, lastbmu_out, mse_out);
}

int vsom_train_online_chunk_masked(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk,
                                   const uint8_t *valid_host, int one_mask, uint64_t *lastbmu_out, float *mse_out)
{
    bool in_pinned = false;
    if (int rc = train_online_chunk_impl(c, eta, sigma, decay_fn, first_chunk, nullptr, lastbmu_out != nullptr, &in_pinned, true,
                                         valid_host, one_mask))
        return rc;
    return online_chunk_fetch(c, in_pinned, lastbmu_out, mse_out);
}

int vsom_train_online_chunk(vsom_ctx *c, double eta, double sigma, int decay_fn, float *mse_out)
{
    return vsom_train_online_chunk_acc(c, eta, sigma, decay_fn, 1, mse_out);
}

// vsom_train_single with the vector's validity bytes (custom contexts only): value_weight = valid .* column weights
int vsom_train_single_valid(vsom_ctx *c, const float *v_host, const uint8_t *valid_host, double eta, double sigma,
                            uint64_t *last_bmu, int decay_fn, float *residual_out, float *dist_out, uint64_t *bmu_out)
{
    VSOM_CUSTOM_ONLY(c, "vsom_train_single_valid");
    CHECK_CTX_NOJOIN(c);
    return vsom_custom_train_single(c, v_host, valid_host, eta, sigma, last_bmu, decay_fn, residual_out, dist_out, bmu_out);
}

int vsom_train_single(vsom_ctx *c, const float *v_host, double eta, double sigma, uint64_t *last_bmu,
                      int decay_fn, float *residual_out, float *dist_out, uint64_t *bmu_out)
{
    CHECK_CTX_NOJOIN(c);
    if (c->cu)
        return vsom_custom_train_single(c, v_host, nullptr, eta, sigma, last_bmu, decay_fn, residual_out, dist_out, bmu_out);
    // not CHECK_CTX: a custom context leaves before the join, and the step reads its own copy of the vector, not the staged
    // rows, so rows_free_valid stays as it is
    if (int jrc = vsom_join_aux(c))
        return jrc;
    if (!v_host || !last_bmu)
        return vsom_fail(VSOM_ERR_INVALID, "null argument");
    if (decay_fn != VSOM_EXPONENTIAL && decay_fn != VSOM_INVERSE_PROPORTIONAL)
        return vsom_fail(VSOM_ERR_INVALID, "online training needs Exponential or InverseProportional");
    if (*last_bmu >= c->N)
        return vsom_fail(VSOM_ERR_INVALID, "lastBMU out of range");
    int rc = stage_single(c, v_host);
    if (rc)
        return rc;
    const size_t xs_n = c->xpitch, pp = c->part_pitch;
    const double *lutd = nullptr;
    int lutw = 0;
    rc = ensure_lutd(c, sigma, &lutd, &lutw);
    if (rc)
        return rc;
    // The sample's rows are copied into HBM (thousands of wavefronts read them); lastBMU in, residual + {bmu, distance, mse}
    // out go straight through the pinned buffer, which the device addresses: written / read by single wavefronts of the
    // step's kernels -- one copy and one synchronisation per call (three copies before: 36 us per call)
    float *xs = c->v_dev.p, *xp = c->v_dev.p + xs_n, *yp = xp + pp;
    float *res = c->v_pinned.p + xs_n + 2 * pp, *tail = res + pp;
    u64 *lb = reinterpret_cast<u64 *>(tail);
    float *pout = res;
    std::memcpy(tail, last_bmu, 8);
    tail[2] = 0.f;
    tail[3] = 0.f;
    {
        TimerScope ts(c, VSOM_T_ONLINE);
        hipLaunchKernelGGL(online_init_kernel, dim3(1), dim3(1), 0, c->stream, c->onl_state.p, c->onl_f.p, 1);
        rc = enqueue_single(c, xs, xp, yp, eta, sigma, decay_fn, lb, res, 1.0f, 0, lutd, lutw, 0, tail + 2);
        if (rc)
            return rc;
        VSOM_HIP_CHECK(hipGetLastError());
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    uint64_t bmu = 0;
    std::memcpy(&bmu, pout + pp, 8);
    if (residual_out)
        std::memcpy(residual_out, pout, (size_t)c->part_len * 4);
    if (dist_out)
        *dist_out = pout[pp + 2];
    *last_bmu = bmu;
    if (bmu_out)
        *bmu_out = bmu;
    return VSOM_OK;
}

}   // extern "C"

// vsom_train_online_chunk_masked for a member of an ensemble (vsom_ensemble_train_online_chunk_masked): the single call with
// every refusal but that of the membership
int vsom_online_chunk_masked_member(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk,
                                    const uint8_t *valid_host, int one_mask, uint64_t *lastbmu_out, float *mse_out)
{
    bool in_pinned = false;
    if (int rc = train_online_chunk_impl(c, eta, sigma, decay_fn, first_chunk, nullptr, lastbmu_out != nullptr, &in_pinned, true,
                                         valid_host, one_mask, true))
        return rc;
    return online_chunk_fetch(c, in_pinned, lastbmu_out, mse_out);
}
