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

__device__ __forceinline__ float tiny_sign(float a)   // as vsom_update.hip's vsom_sign (see there)
{
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

// the descriptor of one epoch (the table must be current: ensure_lut); returns the dynamic LDS it needs
static size_t fill_tiny_args(vsom_ctx *c, int is_first, TinyArgs &a)
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
    a.lut = c->lut.p;
    a.lutw = (int)c->lut_w;
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
    a.luth = (int)c->lut_h;
    smem += (size_t)c->lut_w * c->lut_h * sizeof(float);    // N <= 4096 here: at most 16 KB
    return smem;
}

int launch_tiny_epoch(vsom_ctx *c, double sigma, int is_first)
{
    int rc = ensure_lut(c, sigma);
    if (rc)
        return rc;
    TinyArgs a;
    const size_t smem = fill_tiny_args(c, is_first, a);
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
    const size_t need = fill_tiny_args(c, is_first, a);
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
