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
// so the results are bit-identical to those kernels and to the oracle.  Also here: whole schedules of such epochs in one
// launch (tiny_batch_schedule_kernel), and vsom_schedule_rounds, the host routine that runs a single context's schedule
// round by round for this flavour and for the masked one (vsom_tiny_masked.hip); the round's image is
// vsom_sched_round.hpp's.
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
// (TinySched and tiny_schedule_epoch: vsom_device.hpp.  A struct of its own rather than an alias, so that the kernels'
// parameter type keeps its name)
struct TinySchedArgs : TinySched<TinyArgs> {};

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
        return vsom_schedule_loop(c, epochs, reset_bmu,
                                  [&](size_t ep) { return vsom_batch_epoch(c, sigma[ep], ep == 0, &mse_out[ep]); });
    return vsom_schedule_rounds(c, sigma, epochs, reset_bmu, nullptr, 0, mse_out,
                                [](vsom_ctx *ctx, const unsigned char *, int, const float *lut_dev, const unsigned *tab_dev,
                                   float *mse, size_t cnt, int first, int reset) {
                                    TinySchedArgs s;
                                    size_t smem = 0;
                                    vsom_tiny_sched_fill(ctx, lut_dev, tab_dev, mse, cnt, first, reset, &s, &smem);
                                    if (ctx->transform == VSOM_CLR)
                                        hipLaunchKernelGGL(tiny_batch_schedule_kernel<VSOM_CLR>, dim3(1), dim3(256), smem, ctx->stream, s);
                                    else if (ctx->transform == VSOM_MEDIAN)
                                        hipLaunchKernelGGL(tiny_batch_schedule_kernel<VSOM_MEDIAN>, dim3(1), dim3(256), smem, ctx->stream, s);
                                    else
                                        hipLaunchKernelGGL(tiny_batch_schedule_kernel<VSOM_STANDARD>, dim3(1), dim3(256), smem, ctx->stream, s);
                                    VSOM_HIP_CHECK(hipGetLastError());
                                    return (int)VSOM_OK;
                                });
}

int vsom_schedule_rounds(vsom_ctx *c, const double *sigma, size_t epochs, int reset_bmu, const uint8_t *valid_host,
                         int one_mask, float *mse_out, VsomSchedLaunch launch)
{
    VSOM_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = vsom_join_aux(c))
        return rc;
    c->rows_free_valid = false;   // (as every entry point that reads the staged rows)
    // the validity bytes: one copy per call into the query arena, read by every epoch of every launch
    const unsigned char *valid_dev = nullptr;
    if (valid_host) {
        const size_t vbytes = (one_mask ? 1 : c->B) * (size_t)c->J;
        vsom_layout lay;
        const auto vraw = lay.add<unsigned char>(vbytes);
        VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
        TimerScope ts(c, VSOM_T_STAGE);
        VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(vraw), valid_host, vbytes, hipMemcpyHostToDevice, c->stream));
        valid_dev = lay.at(vraw);
    }
    // Launch by launch (no launch runs more than VSOM_SCHEDULE_MAX_EPOCHS epochs, and the tables of one launch are at most
    // 1024 x 16 KB, below 2^32 values): the round's image -- its tables, one per distinct sigma, then each epoch's offset --
    // pinned, one copy.  A schedule within the cap is one copy, one launch and one wait; a longer one waits before it
    // rewrites the image.
    VsomSchedMember m;
    vsom_lut_dims(c, &m.lw, &m.lh);
    m.valid = nullptr;
    m.vbytes = 0;
    VSOM_ALLOC_CHECK(vsom_grow(c->sch_mse, epochs, c->stream, VSOM_BUF_SYNC));
    VsomSchedRound round;
    for (size_t e0 = 0; e0 < epochs; e0 += VSOM_SCHEDULE_MAX_EPOCHS) {
        m.sigma = sigma + e0;
        m.epochs = std::min(epochs - e0, (size_t)VSOM_SCHEDULE_MAX_EPOCHS);
        if (e0)
            VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));   // the previous launch's copy has left the pinned image
        round.plan(&m, 1);
        const size_t bytes = round.bytes();
        VSOM_ALLOC_CHECK(vsom_grow_set(c->stream, VSOM_BUF_SYNC, {vsom_member(c->sch_host, bytes), vsom_member(c->sch_dev, bytes)}));
        round.write(c->sch_host.p, &m);
        VSOM_HIP_CHECK(hipMemcpyAsync(c->sch_dev.p, c->sch_host.p, bytes, hipMemcpyHostToDevice, c->stream));
        const float *lut_dev = reinterpret_cast<const float *>(c->sch_dev.p);
        const unsigned *tab_dev = reinterpret_cast<const unsigned *>(c->sch_dev.p + round.table_bytes());
        TimerScope ts(c, VSOM_T_UPDATE);
        if (int rc = launch(c, valid_dev, one_mask, lut_dev, tab_dev, c->sch_mse.p + e0, m.epochs, e0 == 0, reset_bmu))
            return rc;
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
