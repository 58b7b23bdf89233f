// vsom_single.hip -- queries of ONE host vector against the map, without touching the staged chunk: Som::findBmu
// (vsom_find_bmu), Som::findRestrictedBmu (vsom_find_restricted_bmu), the distances Som::findRestrictedBmd walks
// (vsom_distances_single), Som::euclidianWeightedDist (vsom_dist_single) and Som::findLocalBmu (vsom_find_local_bmu).
//
// The vector is staged by stage_single into the context's single-sample rows, which vsom_train_single (vsom_online.hip, the
// index of the family) uses too.  The searches over every node fold their minimum into the key slots of onl_state
// (vsom_online.hpp) and the host decodes the slots' image; vsom_find_bmu's scan is online_scan_kernel, launched through
// launch_online_scan.  None of these calls enqueues a reader of the staged rows, so none clears rows_free_valid: their gate
// is CHECK_CTX_NOJOIN and the join, not CHECK_CTX.
#include "vsom_online.hpp"
#include <cstring>
#include <algorithm>

// ---- Som::euclidianWeightedDist / Som::findLocalBmu of ONE host vector --------------------------------------------
// one wavefront; results into the 16-byte tail behind the single-sample rows: {u64 index, float distance}
template <bool CLR>
__global__ __launch_bounds__(64) void single_dist_kernel(DistArgs d, u64 node, u64 *out_idx, float *out_dist)
{
    const int lane = threadIdx.x;
    const float v = vsom_group_dist_lat<CLR>(d.xa, d.xb, d.ma + (size_t)node * d.ldm, d.mb + (size_t)node * d.ldm, d.L, lane & 7);
    if (lane == 0) {
        *out_idx = node;
        *out_dist = v;
    }
}

template <bool CLR>
__global__ __launch_bounds__(64) void single_local_kernel(DistArgs d, u64 W, u64 H, u64 start, u64 *out_idx, float *out_dist)
{
    u64 idx;
    float dist;
    vsom_local_walk<CLR>(d, d.xa, d.xb, W, H, start, (int)threadIdx.x, idx, dist);
    if (threadIdx.x == 0) {
        *out_idx = idx;
        *out_dist = dist;
    }
}

// Som::findRestrictedBmu / the distances of Som::findRestrictedBmd for ONE vector: online_scan_kernel's evaluation (8 lanes
// per node, the (distance, index) key, the node-0-NaN flag) with the hit-count filter of Som.cpp:316-322 -- node 0 seeds
// the search whatever its hits, any other node needs bmuHits >= min_hits -- and, optionally, every node's distance kept.
template <bool CLR>
__global__ __launch_bounds__(256) void single_scan_kernel(OnlineArgs a, const u64 *__restrict__ hits, u64 min_hits, int use_hits,
                                                          float *__restrict__ all_dist)
{
    __shared__ u64 skey[4];
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int node = gid >> 3, k = threadIdx.x & 7;
    const int nc = node < a.N ? node : a.N - 1;
    const float d = vsom_group_dist<CLR, VSOM_SCAN_UNR>(a.d.xa, a.d.xb, a.d.ma + (size_t)nc * a.d.ldm, a.d.mb + (size_t)nc * a.d.ldm,
                                                        a.d.L, k);
    if (all_dist && node < a.N && k == 0)
        all_dist[node] = d;
    const bool allowed = node < a.N && (!use_hits || node == 0 || hits[nc] >= min_hits);
    u64 key = allowed ? vsom_key(d, (uint32_t)node) : ~0ull;
    if (node == 0 && k == 0)
        a.state[ONL_FLAG + a.par] = (d != d) ? 1ull : 0ull;
    for (int off = 32; off >= 8; off >>= 1) {
        const u64 o = __shfl_xor(key, off);
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

// one host vector -> the single-sample device rows [xs | xp | yp | residual] (v_dev), through a pinned
// host buffer; CLR expands x'/y' (Transformation.cpp:94-101).  The copy is enqueued on the stream.
// copy = false: the rows stay in the pinned buffer only -- single-wavefront kernels read them from there (below)
int stage_single(vsom_ctx *c, const float *v_host, bool copy)
{
    const size_t xs_n = c->xpitch, pp = c->part_pitch;
    const size_t nstage = xs_n + 2 * pp;
    // device: [xs | xp | yp | residual(pp) | tail(16)]; tail = {u64 lastBMU/bmu, float dist, float mse}
    // pinned: the same rows, 32 floats of tails, and an image of onl_state for vsom_find_bmu
    // (once allocated, the previous call's copy out of the pinned buffer has been waited for: every caller synchronises
    // the stream before returning)
    VSOM_ALLOC_CHECK(vsom_grow_set(c->stream, 0, {vsom_member(c->v_dev, xs_n + 3 * pp + 16), vsom_member(c->res_dev, 16),
                                                vsom_member(c->v_pinned, xs_n + 3 * pp + 32 + ONL_STATE_BYTES / sizeof(float))}));
    float *host = c->v_pinned.p;
    std::fill(host, host + nstage, 0.f);
    for (uint32_t d = 0; d < c->J; ++d)
        host[d] = v_host[d];
    if (c->transform == VSOM_CLR) {
        size_t p = 0;
        for (uint32_t i = 0; i < c->J; ++i)
            for (uint32_t j = i + 1; j < c->J; ++j) {
                host[xs_n + p] = v_host[i];
                host[xs_n + pp + p] = v_host[j];
                ++p;
            }
    }
    if (copy)
        VSOM_HIP_CHECK(hipMemcpyAsync(c->v_dev.p, host, nstage * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return VSOM_OK;
}

// the pinned image of onl_state (behind the rows and tails of stage_single; 8-byte aligned: pitches are multiples of 32 floats)
static u64 *onl_state_image(const vsom_ctx *c)
{
    return reinterpret_cast<u64 *>(c->v_pinned.p + c->xpitch + 3 * c->part_pitch + 32);
}

// (bmu, distance bits) of a search of parity 0 from that image: the minimum over the key slots, unless a NaN distance at
// node 0 pins the BMU to 0 (Som.cpp:293-299; :316-322: `cur < NaN` never holds)
static void onl_state_decode(const u64 *st, uint64_t *bmu_out, float *dist_out)
{
    uint64_t key = ~0ull;
    for (int sl = 0; sl < ONL_SLOTS; ++sl)
        key = std::min<uint64_t>(key, st[sl * 16]);
    const bool nan0 = st[ONL_FLAG] != 0;
    if (bmu_out)
        *bmu_out = nan0 ? 0ull : (key & 0xFFFFFFFFull);
    if (dist_out) {
        const uint32_t bits = nan0 ? 0x7FC00000u : (uint32_t)(key >> 32);
        std::memcpy(dist_out, &bits, 4);
    }
}

extern "C" {

// Som::findBmu(v) for ONE host vector (Som.cpp:283-309) without touching the staged chunk: copy,
// one scan launch (8 lanes per node, atomicMin on the (distance, index) key), 32 bytes back.
int vsom_find_bmu(vsom_ctx *c, const float *v_host, uint64_t *bmu_out, float *dist_out)
{
    CHECK_CTX_NOJOIN(c);
    if (c->cu)
        return vsom_custom_find(c, v_host, nullptr, 0, 0, bmu_out, dist_out);
    if (int jrc = vsom_join_aux(c))
        return jrc;
    if (!v_host)
        return vsom_fail(VSOM_ERR_INVALID, "null argument");
    int rc = stage_single(c, v_host);
    if (rc)
        return rc;
    float *xs = c->v_dev.p, *xp = xs + c->xpitch, *yp = xp + c->part_pitch;
    const OnlineArgs a = vsom_onl_args(c, xs, xp, yp);
    VSOM_HIP_CHECK(hipMemsetAsync(c->onl_state.p, 0xFF, ONL_SLOTS * 16 * sizeof(u64), c->stream));   // arm the keys of parity 0
    launch_online_scan(c, a, false, (unsigned)(((size_t)c->N * 8 + 255) / 256), nullptr, 1.f, 0);
    VSOM_HIP_CHECK(hipGetLastError());
    u64 *st = onl_state_image(c);
    VSOM_HIP_CHECK(hipMemcpyAsync(st, c->onl_state.p, ONL_STATE_BYTES, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    onl_state_decode(st, bmu_out, dist_out);
    return VSOM_OK;
}

// shared by the two single-vector queries below: stage v, launch `which` (0: distance to `node`; 1: local search from
// `node`), 16 bytes back -- one synchronisation, no allocation, the staged chunk untouched
static int single_query(vsom_ctx *c, const float *v_host, uint64_t node, int which, uint64_t *idx_out, float *dist_out)
{
    CHECK_CTX_NOJOIN(c);
    if (int jrc = vsom_join_aux(c))   // (CHECK_CTX less its last line: no reader of the staged rows is enqueued)
        return jrc;
    if (!v_host)
        return vsom_fail(VSOM_ERR_INVALID, "null argument");
    if (node >= c->N)
        return vsom_fail(VSOM_ERR_INVALID, "node index out of range");
    // The distance: ONE wavefront reads the vector once and writes 16 bytes -- both go straight through the pinned buffer
    // (host memory the device addresses): no copy in, no copy out, the call is a launch and a synchronisation (18.2 -> 14.9 us).
    // The local walk evaluates up to a few dozen distances and would read the vector across the bus each time (no gain
    // measured): its vector is copied into HBM first, only its 16 bytes of results go through pinned memory.  (Kernels of
    // thousands of wavefronts that all read the vector -- vsom_find_bmu -- keep their copy too.)
    const bool zero_copy_in = which == 0;
    int rc = stage_single(c, v_host, !zero_copy_in);
    if (rc)
        return rc;
    const bool clr = c->transform == VSOM_CLR;
    const size_t xs_n = c->xpitch, pp = c->part_pitch;
    float *rows = zero_copy_in ? c->v_pinned.p : c->v_dev.p;
    float *xs = rows, *xp = rows + xs_n, *yp = xp + pp, *tail = c->v_pinned.p + xs_n + 3 * pp;
    const DistArgs d = vsom_onl_args(c, xs, xp, yp).d;
    u64 *oi = reinterpret_cast<u64 *>(tail);
    float *od = tail + 2;
    if (which == 0) {
        if (clr)
            hipLaunchKernelGGL(single_dist_kernel<true>, dim3(1), dim3(64), 0, c->stream, d, (u64)node, oi, od);
        else
            hipLaunchKernelGGL(single_dist_kernel<false>, dim3(1), dim3(64), 0, c->stream, d, (u64)node, oi, od);
    } else {
        if (clr)
            hipLaunchKernelGGL(single_local_kernel<true>, dim3(1), dim3(64), 0, c->stream, d, (u64)c->W, (u64)c->H, (u64)node, oi, od);
        else
            hipLaunchKernelGGL(single_local_kernel<false>, dim3(1), dim3(64), 0, c->stream, d, (u64)c->W, (u64)c->H, (u64)node, oi, od);
    }
    VSOM_HIP_CHECK(hipGetLastError());
    float *pout = tail;
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (idx_out)
        std::memcpy(idx_out, pout, 8);
    if (dist_out)
        *dist_out = pout[2];
    return VSOM_OK;
}

// one host vector against every node: restricted (or plain) BMU through the key slots, optionally all N distances
static int single_scan(vsom_ctx *c, const float *v_host, int use_hits, uint64_t min_hits, uint64_t *bmu_out, float *dist_out,
                       float *all_out_host)
{
    CHECK_CTX_NOJOIN(c);
    if (int jrc = vsom_join_aux(c))   // (as single_query)
        return jrc;
    if (!v_host)
        return vsom_fail(VSOM_ERR_INVALID, "null argument");
    int rc = stage_single(c, v_host);
    if (rc)
        return rc;
    float *all_dev = nullptr;
    if (all_out_host) {
        vsom_layout lay;
        const auto hall = lay.add<float>(c->N);
        VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
        all_dev = lay.at(hall);
    }
    const bool clr = c->transform == VSOM_CLR;
    float *xs = c->v_dev.p, *xp = xs + c->xpitch, *yp = xp + c->part_pitch;
    const OnlineArgs a = vsom_onl_args(c, xs, xp, yp);
    VSOM_HIP_CHECK(hipMemsetAsync(c->onl_state.p, 0xFF, ONL_SLOTS * 16 * sizeof(u64), c->stream));   // arm the keys of parity 0
    dim3 grid((unsigned)(((size_t)c->N * 8 + 255) / 256));
    if (clr)
        hipLaunchKernelGGL(single_scan_kernel<true>, grid, dim3(256), 0, c->stream, a, c->hits.p, (u64)min_hits, use_hits, all_dev);
    else
        hipLaunchKernelGGL(single_scan_kernel<false>, grid, dim3(256), 0, c->stream, a, c->hits.p, (u64)min_hits, use_hits, all_dev);
    VSOM_HIP_CHECK(hipGetLastError());
    u64 *st = onl_state_image(c);
    VSOM_HIP_CHECK(hipMemcpyAsync(st, c->onl_state.p, ONL_STATE_BYTES, hipMemcpyDeviceToHost, c->stream));
    if (all_out_host)
        VSOM_HIP_CHECK(hipMemcpyAsync(all_out_host, all_dev, (size_t)c->N * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    onl_state_decode(st, bmu_out, dist_out);
    return VSOM_OK;
}

// Som::findRestrictedBmu(v, ..., minBmuHits, ...) for ONE host vector (Som.cpp:313-332)
int vsom_find_restricted_bmu(vsom_ctx *c, const float *v_host, uint64_t min_hits, uint64_t *bmu_out, float *dist_out)
{
    VSOM_CUSTOM_REFUSE(c, "vsom_find_restricted_bmu");
    return single_scan(c, v_host, 1, min_hits, bmu_out, dist_out, nullptr);
}

// euclidianWeightedDist(i, v) of ONE host vector to every node i (what Som::findRestrictedBmd walks, Som.cpp:457-487)
int vsom_distances_single(vsom_ctx *c, const float *v_host, float *dist_out_host)
{
    VSOM_CUSTOM_REFUSE(c, "vsom_distances_single");
    if (!dist_out_host)
        return vsom_fail(VSOM_ERR_INVALID, "null output");
    return single_scan(c, v_host, 0, 0, nullptr, nullptr, dist_out_host);
}

// Som::euclidianWeightedDist(pos, v, ...) for ONE host vector (Som.cpp:124-141)
int vsom_dist_single(vsom_ctx *c, const float *v_host, uint64_t node, float *dist_out)
{
    if (c && c->cu && hipSetDevice(c->device) == hipSuccess)
        return vsom_custom_dist_single(c, v_host, nullptr, node, dist_out);
    return single_query(c, v_host, node, 0, nullptr, dist_out);
}

// Som::findLocalBmu(v, ..., lastBMU, ...) for ONE host vector (Som.cpp:335-454)
int vsom_find_local_bmu(vsom_ctx *c, const float *v_host, uint64_t last_bmu, uint64_t *bmu_out, float *dist_out)
{
    if (c && c->cu && hipSetDevice(c->device) == hipSuccess)
        return vsom_custom_find(c, v_host, nullptr, 1, last_bmu, bmu_out, dist_out);
    return single_query(c, v_host, last_bmu, 1, bmu_out, dist_out);
}

// the three searches above with the vector's validity bytes (custom contexts only): value_weight = valid .* column weights
int vsom_find_bmu_valid(vsom_ctx *c, const float *v_host, const uint8_t *valid_host, uint64_t *bmu_out, float *dist_out)
{
    VSOM_CUSTOM_ONLY(c, "vsom_find_bmu_valid");
    CHECK_CTX_NOJOIN(c);
    return vsom_custom_find(c, v_host, valid_host, 0, 0, bmu_out, dist_out);
}

int vsom_find_local_bmu_valid(vsom_ctx *c, const float *v_host, const uint8_t *valid_host, uint64_t last_bmu, uint64_t *bmu_out,
                              float *dist_out)
{
    VSOM_CUSTOM_ONLY(c, "vsom_find_local_bmu_valid");
    CHECK_CTX_NOJOIN(c);
    return vsom_custom_find(c, v_host, valid_host, 1, last_bmu, bmu_out, dist_out);
}

int vsom_dist_single_valid(vsom_ctx *c, const float *v_host, const uint8_t *valid_host, uint64_t node, float *dist_out)
{
    VSOM_CUSTOM_ONLY(c, "vsom_dist_single_valid");
    CHECK_CTX_NOJOIN(c);
    return vsom_custom_dist_single(c, v_host, valid_host, node, dist_out);
}

}   // extern "C"
