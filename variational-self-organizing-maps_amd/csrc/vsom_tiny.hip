// vsom_tiny.hip -- Som::trainBatchSomEpoch (Som.cpp:756-879) for maps so small that the dozen launches
// of the general path cost more than the work (the reference's own perf-harness scenario is a 10x10
// map with 20 nine-dimensional rows, tests/performance/perf_tests.cpp:74-112): ONE workgroup does the
// whole epoch in one launch --
//   phase 1  every (sample, node) distance by 8-lane groups in Eigen's order (vsom_group_dist), argmin
//            through an LDS atomicMin on the (distance, index) key -- or the findLocalBmu walk, one
//            wavefront per sample (vsom_local_walk);  bmuHits;  MSE summed in sample order
//   phase 2  one thread per (node, dim) chain [CLR: per (node, pair)]: the neighbourhood weight from
//            the host table, the fp32 prefix W, c = w/W, and the mean / sigma^2 recurrences, every
//            operation rounded separately like the general kernels
// so the results are bit-identical to those kernels and to the oracle.
#include "vsom_device.hpp"
#include <cmath>
#include <cstring>

struct TinyArgs {
    DistArgs d;                  // search operands: Xs (Standard/Median) or XP,YP (CLR); map parts
    float *map, *sigma, *weight;
    u64 *hits, *lastbmu;
    float *sqres, *mse;
    const float *lut;
    int lutw;
    int N, W, H, Dc, pitch, ppitch, B, is_first;   // Dc: chains per node (D, or P for CLR)
    int stage_x;                                    // samples fit into LDS
    int luth;                                       // table rows (the table is copied into LDS)
};

__device__ __forceinline__ float tiny_sign(float a)   // Transformation::Stepper's sign (Transformation.cpp:49-50):
{                                                     // +-1; a zero or a NaN comes back as it is
    const float one = __builtin_copysignf(1.f, a);
    return (a < 0.f || a > 0.f) ? one : a;
}

template <int KIND>
__global__ __launch_bounds__(256) void tiny_batch_epoch_kernel(TinyArgs a)
{
#include "vsom_tiny_batch_body.inc"
}

// one map per workgroup (vsom_ensemble.hip): the same body on the workgroup's descriptor (the index is uniform: scalar
// loads).  The body is included as text rather than called: the single-map kernel above is then compiled from the very
// tokens it had before the ensemble existed, and its code object is unchanged instruction for instruction (an inlined
// device function taking the args struct gives the same instructions in another order)
template <int KIND>
__global__ __launch_bounds__(256) void tiny_batch_epoch_many_kernel(const TinyArgs *__restrict__ args)
{
    const TinyArgs a = args[blockIdx.x];
#include "vsom_tiny_batch_body.inc"
}

// the fused path applies when the whole epoch is a handful of microseconds of work for one workgroup
bool vsom_tiny_applies(const vsom_ctx *c)
{
    const size_t chains = (size_t)c->N * c->part_len;
    return c->use_tiny && c->B > 0 && c->B <= 256 && chains <= 4096 && (size_t)c->B * c->N <= 16384 &&
           chains * c->B <= 262144;
}

// the descriptor of one epoch reading the table `lut` of lut_w x lut_h values; returns the dynamic LDS it needs
static size_t fill_tiny_args(vsom_ctx *c, int is_first, TinyArgs &a, const float *lut, uint32_t lut_w, uint32_t lut_h)
{
    const bool clr = c->transform == VSOM_CLR;
    a.d.xa = clr ? c->XP.p : c->Xs.p;
    a.d.xb = clr ? c->YP.p : c->Xs.p;
    a.d.ldx = (int)(clr ? c->part_pitch : c->xpitch);
    a.d.ma = c->map.p;
    a.d.mb = clr ? c->map.p + c->part_pitch : c->map.p;
    a.d.ldm = (int)c->pitch;
    a.d.L = (int)c->part_len;
    a.map = c->map.p;
    a.sigma = c->sigma.p;
    a.weight = c->weight.p;
    a.hits = c->hits.p;
    a.lastbmu = c->lastbmu.p;
    a.sqres = c->sqres.p;
    a.mse = c->mse.p;
    a.lut = lut;
    a.lutw = (int)lut_w;
    a.N = (int)c->N;
    a.W = (int)c->W;
    a.H = (int)c->H;
    a.Dc = (int)c->part_len;
    a.pitch = (int)c->pitch;
    a.ppitch = (int)c->part_pitch;
    a.B = (int)c->B;
    a.is_first = is_first;
    size_t smem = c->B * (sizeof(u64) + sizeof(int2) + sizeof(float) + sizeof(int));
    const size_t xfloats = c->B * (size_t)c->part_len * (clr ? 2 : 1);
    a.stage_x = xfloats <= 10240 ? 1 : 0;            // 40 KB on top of the per-sample arrays (< 64 KB in all)
    if (a.stage_x)
        smem += xfloats * sizeof(float);
    a.luth = (int)lut_h;
    smem += (size_t)lut_w * lut_h * sizeof(float);          // N <= 4096 here: at most 16 KB
    return smem;
}

int launch_tiny_epoch(vsom_ctx *c, double sigma, int is_first)
{
    int rc = ensure_lut(c, sigma);
    if (rc)
        return rc;
    TinyArgs a;
    const size_t smem = fill_tiny_args(c, is_first, a, c->lut.p, c->lut_w, c->lut_h);   // (current: ensure_lut)
    TimerScope ts(c, VSOM_T_UPDATE);
    if (c->transform == VSOM_CLR)
        hipLaunchKernelGGL(tiny_batch_epoch_kernel<VSOM_CLR>, dim3(1), dim3(256), smem, c->stream, a);
    else if (c->transform == VSOM_MEDIAN)
        hipLaunchKernelGGL(tiny_batch_epoch_kernel<VSOM_MEDIAN>, dim3(1), dim3(256), smem, c->stream, a);
    else
        hipLaunchKernelGGL(tiny_batch_epoch_kernel<VSOM_STANDARD>, dim3(1), dim3(256), smem, c->stream, a);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}

// ---- the same epoch for many maps in one launch per kind, one workgroup per map (vsom_ensemble.hip) -------------------
size_t vsom_tiny_desc_bytes() { return sizeof(TinyArgs); }

int vsom_tiny_prepare(vsom_ctx *c, double sigma, int is_first, size_t lds_limit, void *desc, int *group, size_t *smem)
{
    *group = -1;
    if (!vsom_tiny_applies(c))
        return VSOM_OK;                                     // the ordinary path
    if (int rc = ensure_lut(c, sigma))                      // (enqueues the table's copy on the member's stream; the
        return rc;                                          //  ordinary path, if this member takes it, finds it current)
    TinyArgs a;
    const size_t need = fill_tiny_args(c, is_first, a, c->lut.p, c->lut_w, c->lut_h);
    if (need > lds_limit)
        return VSOM_OK;
    std::memcpy(desc, &a, sizeof(a));
    *group = c->transform;                                  // VSOM_STANDARD, VSOM_MEDIAN, VSOM_CLR
    *smem = need;
    return VSOM_OK;
}

int vsom_tiny_launch_many(int group, const void *desc_dev, unsigned count, size_t smem, hipStream_t s)
{
    const TinyArgs *args = static_cast<const TinyArgs *>(desc_dev);
    if (group == VSOM_CLR)
        hipLaunchKernelGGL(tiny_batch_epoch_many_kernel<VSOM_CLR>, dim3(count), dim3(256), smem, s, args);
    else if (group == VSOM_MEDIAN)
        hipLaunchKernelGGL(tiny_batch_epoch_many_kernel<VSOM_MEDIAN>, dim3(count), dim3(256), smem, s, args);
    else
        hipLaunchKernelGGL(tiny_batch_epoch_many_kernel<VSOM_STANDARD>, dim3(count), dim3(256), smem, s, args);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}

// ---- a whole schedule of such epochs in one launch (vsom_batch_schedule) ------------------------
// The epoch body keeps nothing between epochs that another workgroup needs, so the loop over the epochs moves into the
// kernel: per epoch a local copy of the descriptor with that epoch's is_first, table and MSE slot.  Between two epochs
// one barrier: the chains of phase 2 stored map rows (a.map) that the next phase 1 reads (a.d.ma) from other threads of
// this workgroup, and the LDS arrays (keys, sq, bxy, the staged rows, the table) are written again.  All of a map's
// traffic is vector loads and stores of one CU, which one L1 serves; the map pointers stay plain (no __restrict__, no
// __ldg) so that no load of them goes through the scalar cache, which vector stores do not update.
struct TinySchedArgs {
    TinyArgs t;                  // lut: the first table of the schedule's table buffer; mse: slot 0 of this launch
    const unsigned *tab;         // [epochs] each epoch's table, in floats from t.lut
    int epochs;                  // of this launch (0: nothing to do)
    int first;                   // this launch starts the schedule: its epoch 0 is the exact search
    int reset_bmu;               // lastBMU := 0 before every epoch but the schedule's first
    int pad;
};

// epoch ep of the launch: the barrier behind the previous epoch, the lastBMU reset, and the epoch's descriptor
__device__ __forceinline__ TinyArgs tiny_schedule_epoch(const TinySchedArgs &s, int ep)
{
    TinyArgs a = s.t;
    a.is_first = (s.first && ep == 0) ? 1 : 0;
    a.lut = s.t.lut + s.tab[ep];
    a.mse = s.t.mse + ep;
    if (ep > 0)
        __syncthreads();                     // the previous epoch's phase 2: map rows stored, LDS free
    if (!a.is_first && s.reset_bmu) {
        for (int i = threadIdx.x; i < a.B; i += 256)
            a.lastbmu[i] = 0ull;             // DataSet.cpp:136-137
        __syncthreads();
    }
    return a;
}

template <int KIND>
__global__ __launch_bounds__(256) void tiny_batch_schedule_kernel(TinySchedArgs s)
{
    for (int ep = 0; ep < s.epochs; ++ep) {
        const TinyArgs a = tiny_schedule_epoch(s, ep);
#include "vsom_tiny_batch_body.inc"
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void tiny_batch_schedule_many_kernel(const TinySchedArgs *__restrict__ args)
{
    const TinySchedArgs s = args[blockIdx.x];
    for (int ep = 0; ep < s.epochs; ++ep) {
        const TinyArgs a = tiny_schedule_epoch(s, ep);
#include "vsom_tiny_batch_body.inc"
    }
}

void vsom_lut_dims(const vsom_ctx *c, uint32_t *lw, uint32_t *lh)   // as ensure_lut
{
    const uint32_t ymax = c->N ? (c->N - c->W) / c->H : 0;
    *lh = ymax + 1;
    *lw = c->W;
}

size_t VsomSchedTables::add(uint32_t w, uint32_t h, double sigma)
{
    uint64_t bits;
    std::memcpy(&bits, &sigma, sizeof(bits));
    const auto r = at.emplace(std::make_tuple(w, h, bits), floats);
    if (r.second)
        floats += (size_t)w * h;
    return r.first->second;
}

void VsomSchedTables::tabulate(float *host) const
{
    for (const auto &kv : at) {
        const uint32_t w = std::get<0>(kv.first), h = std::get<1>(kv.first);
        double sigma;
        std::memcpy(&sigma, &std::get<2>(kv.first), sizeof(sigma));
        float *t = host + kv.second;
        for (uint32_t dy = 0; dy < h; ++dy)
            for (uint32_t dx = 0; dx < w; ++dx)
                t[(size_t)dy * w + dx] = (float)vsom_neighbourhood_weight(dx, dy, 0, 0, sigma);
    }
}

bool vsom_tiny_schedule_applies(const vsom_ctx *c, const double *sigma, size_t epochs, size_t lds_limit)
{
    if (c->cu || !vsom_tiny_applies(c))
        return false;
    for (size_t ep = 0; ep < epochs; ++ep)
        if (!std::isfinite(sigma[ep]))
            return false;
    uint32_t lw, lh;
    vsom_lut_dims(c, &lw, &lh);
    TinyArgs a;
    return fill_tiny_args(const_cast<vsom_ctx *>(c), 0, a, nullptr, lw, lh) <= lds_limit;
}

size_t vsom_tiny_sched_desc_bytes() { return sizeof(TinySchedArgs); }

int vsom_tiny_sched_fill(vsom_ctx *c, const float *lut_dev, const unsigned *tab_dev, float *mse, size_t epochs, int first,
                         int reset_bmu, void *desc, size_t *smem)
{
    uint32_t lw, lh;
    vsom_lut_dims(c, &lw, &lh);
    TinySchedArgs s;
    *smem = fill_tiny_args(c, 0, s.t, lut_dev, lw, lh);
    s.t.mse = mse;
    s.tab = tab_dev;
    s.epochs = (int)epochs;
    s.first = first;
    s.reset_bmu = reset_bmu ? 1 : 0;
    s.pad = 0;
    std::memcpy(desc, &s, sizeof(s));
    return c->transform;
}

int vsom_tiny_sched_launch_many(int group, const void *desc_dev, unsigned count, size_t smem, hipStream_t s)
{
    const TinySchedArgs *args = static_cast<const TinySchedArgs *>(desc_dev);
    if (group == VSOM_CLR)
        hipLaunchKernelGGL(tiny_batch_schedule_many_kernel<VSOM_CLR>, dim3(count), dim3(256), smem, s, args);
    else if (group == VSOM_MEDIAN)
        hipLaunchKernelGGL(tiny_batch_schedule_many_kernel<VSOM_MEDIAN>, dim3(count), dim3(256), smem, s, args);
    else
        hipLaunchKernelGGL(tiny_batch_schedule_many_kernel<VSOM_STANDARD>, dim3(count), dim3(256), smem, s, args);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}

// the contract itself: what every context off the fast path runs
int vsom_schedule_loop(vsom_ctx *c, const double *sigma, size_t epochs, int reset_bmu, float *mse_out)
{
    for (size_t ep = 0; ep < epochs; ++ep) {
        if (ep > 0 && reset_bmu && c->B) {
            VSOM_HIP_CHECK(hipSetDevice(c->device));
            VSOM_HIP_CHECK(hipMemsetAsync(c->lastbmu.p, 0, c->B * sizeof(u64), c->stream));
        }
        if (int rc = vsom_batch_epoch(c, sigma[ep], ep == 0, &mse_out[ep]))
            return rc;
    }
    return VSOM_OK;
}

const char *vsom_schedule_refusal(const vsom_ctx *c)
{
    if (!c->chunk_loaded)        // (custom contexts keep chunk_loaded and ahead_rows like every other)
        return "no chunk loaded";
    if (c->ahead_rows)
        return "the next chunk is staged ahead over the current chunk's rows: vsom_commit_chunk first";
    return nullptr;
}

int vsom_batch_schedule(vsom_ctx *c, const double *sigma, size_t epochs, int reset_bmu, float *mse_out)
{
    if (!c)
        return vsom_fail(VSOM_ERR_INVALID, "null context");
    if (epochs == 0)
        return VSOM_OK;
    if (!sigma || !mse_out)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_schedule: null sigma or mse_out");
    if (const char *why = vsom_schedule_refusal(c))
        return vsom_fail(VSOM_ERR_INVALID, why);
    if (!vsom_tiny_schedule_applies(c, sigma, epochs, (size_t)64 << 10))
        return vsom_schedule_loop(c, sigma, epochs, reset_bmu, mse_out);

    VSOM_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = vsom_join_aux(c))
        return rc;
    c->rows_free_valid = false;   // (as every entry point that reads the staged rows)
    // Launch by launch (no launch runs more than VSOM_SCHEDULE_MAX_EPOCHS epochs, and the tables of one launch are at most
    // 1024 x 16 KB): the launch's tables, one per distinct sigma, then each epoch's offset -- one pinned image, one copy.
    // A schedule within the cap is one copy, one launch and one wait; a longer one waits before it rewrites the image.
    uint32_t lw, lh;
    vsom_lut_dims(c, &lw, &lh);
    VSOM_ALLOC_CHECK(vsom_grow(c->sch_mse, epochs, c->stream, VSOM_BUF_SYNC));
    std::vector<unsigned> tab;
    for (size_t e0 = 0; e0 < epochs; e0 += VSOM_SCHEDULE_MAX_EPOCHS) {
        const size_t cnt = std::min(epochs - e0, (size_t)VSOM_SCHEDULE_MAX_EPOCHS);
        if (e0)
            VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));   // the previous launch's copy has left the pinned image
        VsomSchedTables tabs;
        tab.resize(cnt);
        for (size_t ep = 0; ep < cnt; ++ep)
            tab[ep] = (unsigned)tabs.add(lw, lh, sigma[e0 + ep]);   // (below 1024 * 4096 floats)
        const size_t bytes = (tabs.floats + cnt) * sizeof(float);
        VSOM_ALLOC_CHECK(vsom_grow_set(c->stream, VSOM_BUF_SYNC, {vsom_member(c->sch_host, bytes), vsom_member(c->sch_dev, bytes)}));
        tabs.tabulate(reinterpret_cast<float *>(c->sch_host.p));
        std::memcpy(c->sch_host.p + tabs.floats * sizeof(float), tab.data(), cnt * sizeof(unsigned));
        VSOM_HIP_CHECK(hipMemcpyAsync(c->sch_dev.p, c->sch_host.p, bytes, hipMemcpyHostToDevice, c->stream));
        const float *lut_dev = reinterpret_cast<const float *>(c->sch_dev.p);
        const unsigned *tab_dev = reinterpret_cast<const unsigned *>(c->sch_dev.p + tabs.floats * sizeof(float));
        TimerScope ts(c, VSOM_T_UPDATE);
        TinySchedArgs s;
        size_t smem = 0;
        vsom_tiny_sched_fill(c, lut_dev, tab_dev, c->sch_mse.p + e0, cnt, e0 == 0, reset_bmu, &s, &smem);
        if (c->transform == VSOM_CLR)
            hipLaunchKernelGGL(tiny_batch_schedule_kernel<VSOM_CLR>, dim3(1), dim3(256), smem, c->stream, s);
        else if (c->transform == VSOM_MEDIAN)
            hipLaunchKernelGGL(tiny_batch_schedule_kernel<VSOM_MEDIAN>, dim3(1), dim3(256), smem, c->stream, s);
        else
            hipLaunchKernelGGL(tiny_batch_schedule_kernel<VSOM_STANDARD>, dim3(1), dim3(256), smem, c->stream, s);
        VSOM_HIP_CHECK(hipGetLastError());
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    vsom_schedule_results(c, epochs, mse_out);
    return VSOM_OK;
}

// after the wait: the per-epoch MSE words the kernel stored, and the last one into the word vsom_get_mse reads
void vsom_schedule_results(vsom_ctx *c, size_t epochs, float *mse_out)
{
    const volatile float *m = c->sch_mse.p;
    for (size_t ep = 0; ep < epochs; ++ep)
        mse_out[ep] = m[ep];
    *static_cast<volatile float *>(c->mse.p) = mse_out[epochs - 1];
}
