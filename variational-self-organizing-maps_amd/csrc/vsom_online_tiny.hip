// vsom_online_tiny.hip -- tiny maps: the whole chunk loop of Som::trainBasicSom (Som.cpp:1159-1171) in ONE launch of ONE
// workgroup, and the same body with one workgroup per map for ensembles (vsom_onl_tiny_*, called by vsom_ensemble.hip).
// One of the four chunk loops vsom_train_online_chunk* picks from (vsom_online.hip, the index of the family).
//
// The reference's own performance scenario trains a 10 x 10 map on 20 nine-dimensional rows (tests/performance/
// perf_tests.cpp:74-112): two dependent launches per sample were 220-260 us per epoch there against 50 us of one CPU thread.
// For maps of at most 4096 values (N D) and 1024 nodes, Standard / Median: every thread owns U = 1, 2 or 4 model values
// (M, S) IN REGISTERS for the whole chunk, plus a copy of its node's weight -- the window update of Som.cpp:911-943 is
// elementwise, so nothing of it crosses threads -- and per sample the workgroup meets at two barriers:
//   B  one thread per node adds its row's squares in Eigen's order (the eight accumulator classes, the tree, the tail:
//      vsom_group_dist's arithmetic); per wavefront a DPP minimum of the distances' bit patterns, the lowest lane that holds
//      it (strict <: the lowest index wins), one LDS atomic minimum of the (distance, index) key.  Meanwhile the LAST thread
//      finishes the PREVIOUS sample: the distance after the update (:946), the MSE running sum (:1167), addBmu, lastBMU.
//      sigma <= 1 (:891): the distances go to LDS and, behind one more barrier, one thread walks findLocalBmu over them.
//   -- barrier --
//   C  every thread reads the BMU, applies online_window's bounds (a per-BMU table) and the neighbourhood table and updates
//      its values with online_node_update's operations (same expressions, same order: same bits)
//   D  the BMU's threads publish their new squares (double-buffered: read by the post step beside the next sample's B)
//   A  squares p = fl(fl(m - x)^2) of the NEXT sample against every value, into LDS
//   -- barrier --
// sigmaMap is written once at the end, from the final S and weight, for the nodes some window touched (the value of the
// node's last update: onl_sigma_kernel's argument).  Results are bit-identical to the per-sample kernels and the oracle.
// The kernel is bound by instruction issue (16 wavefronts on 4 SIMDs) and LDS latency: 0.95 us per sample at 10 x 10 x 9.
#include "vsom_online_tiny.hpp"
#include <cstring>
#include <array>
#include <mutex>

#ifdef VSOM_DEVELOPMENT
// cycle stamps of one sample of the one-launch chunk (sample 5 of the chunk; s_memtime): [2 w + p] = wavefront w (0: first,
// 1: last) at phase boundary p (tools/exp/tiny_stamps.py)
__device__ unsigned long long vsom_tiny_stamps[64];
#define TINY_STAMP(p) do { if (j == 5 && (tid == 0 || tid == 1023)) vsom_tiny_stamps[(tid ? 16 : 0) + (p)] = __builtin_readcyclecounter(); } while (0)
extern "C" int vsom_dev_tiny_stamps(unsigned long long *out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(vsom_tiny_stamps), sizeof(vsom_tiny_stamps)) == hipSuccess ? 0 : -2;
}
#else
#define TINY_STAMP(p) ((void)0)
#endif
template <int KIND, bool LOCAL, int U>     // U = values per thread (1, 2, 4): N D <= 1024 U
__global__ __launch_bounds__(1024) void online_tiny_chunk_kernel(OnlTinyArgs a)
{
#include "vsom_tiny_online_body.inc"
}

// one map per workgroup (vsom_ensemble.hip): the same body on the workgroup's descriptor (the index is uniform: scalar
// loads).  Included as text, not called, so that the single-map kernel's code object stays instruction for instruction
// what it was (see tiny_batch_epoch_many_kernel)
template <int KIND, bool LOCAL, int U>
__global__ __launch_bounds__(1024) void online_tiny_chunk_many_kernel(const OnlTinyArgs *__restrict__ args)
{
    const OnlTinyArgs a = args[blockIdx.x];
#include "vsom_tiny_online_body.inc"
}

size_t online_tiny_lds_bytes(const vsom_ctx *c)
{
    const size_t N = c->N, D = c->part_len;
    return N * (16 + 8 + 8) + (N * (D | 1) + 2 * ((D + 3) & ~(size_t)3) + TINY_XBLOCK) * sizeof(float) + N * 8 +
           (c->B + 8) * sizeof(unsigned short);
}

bool online_tiny_applies(const vsom_ctx *c, double sigma)
{
    return c->use_tiny && c->transform != VSOM_CLR && sigma == sigma && c->B > 0 && c->N <= 1024 &&
           (size_t)c->N * c->part_len <= 4096 && c->part_len <= 512 && c->B <= 4096 && c->bmu_mode == VSOM_BMU_AUTO;   // (EXACT / SHORTLIST name the per-sample forms)
}

void fill_chunk_tiny_args(vsom_ctx *c, double eta, double sigma, int decay_fn, const double *lutd, int lutw,
                          int first_chunk, u64 *lastbmu_host, OnlTinyArgs &a)
{
    a.X = c->Xs.p;
    a.ldx = (int)c->xpitch;
    a.B = (int)c->B;
    a.N = (int)c->N;
    a.W = (int)c->W;
    a.H = (int)c->H;
    a.D = (int)c->part_len;
    a.pitch = (int)c->pitch;
    a.map = c->map.p;
    a.Smap = c->S.p;
    a.sigmap = c->sigma.p;
    a.weight = c->weight.p;
    a.hits = c->hits.p;
    a.lastbmu = c->lastbmu.p;
    a.fstate = c->onl_f.p;
    a.lutd = lutd;
    a.lutw = lutw;
    a.eta = eta;
    a.sigma = sigma;
    a.decay_fn = decay_fn;
    a.fB = (float)c->B;
    a.keep_mse = first_chunk ? 0 : 1;
    a.mse_out = c->mse.p;
    a.lastbmu_host = lastbmu_host;
}

// the kernel instantiation a map takes: (Median ? 6 : 0) + (local ? 3 : 0) + (0, 1, 2 for U = 1, 2, 4)
int chunk_tiny_group(const vsom_ctx *c, double sigma)
{
    const bool local = !(sigma > 1);                  // SIGMA_SWITCH_TO_LOCAL (SOM.hpp:37, Som.cpp:891)
    const size_t nd = (size_t)c->N * c->part_len;
    const int ui = nd <= 1024 ? 0 : (nd <= 2048 ? 1 : 2);
    return (c->transform == VSOM_MEDIAN ? 6 : 0) + (local ? 3 : 0) + ui;
}

int enqueue_chunk_tiny(vsom_ctx *c, double eta, double sigma, int decay_fn, const double *lutd, int lutw, int first_chunk,
                              u64 *lastbmu_host)
{
    OnlTinyArgs a;
    fill_chunk_tiny_args(c, eta, sigma, decay_fn, lutd, lutw, first_chunk, lastbmu_host, a);
    const size_t smem = online_tiny_lds_bytes(c);
    const bool local = !(sigma > 1);                  // SIGMA_SWITCH_TO_LOCAL (SOM.hpp:37, Som.cpp:891)
    const size_t nd = (size_t)c->N * c->part_len;
    const int upt = nd <= 1024 ? 1 : (nd <= 2048 ? 2 : 4);     // values per thread (the kernel is bound by instruction issue)
#define VSOM_TINY_LAUNCH(KIND, LOC, UU)                                                                                             \
    do {                                                                                                                            \
        if (!c->tiny_lds_attr[(LOC ? 3 : 0) + (UU == 1 ? 0 : (UU == 2 ? 1 : 2))]) {                                                 \
            /* (more than the 64 KiB a launch may ask for by default; 160 KiB per CU) */                                            \
            VSOM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(online_tiny_chunk_kernel<KIND, LOC, UU>),             \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 96 << 10));                              \
            c->tiny_lds_attr[(LOC ? 3 : 0) + (UU == 1 ? 0 : (UU == 2 ? 1 : 2))] = true;                                            \
        }                                                                                                                           \
        hipLaunchKernelGGL((online_tiny_chunk_kernel<KIND, LOC, UU>), dim3(1), dim3(1024), smem, c->stream, a);                     \
    } while (0)
#define VSOM_TINY_LAUNCH_U(KIND, LOC)                                                                                               \
    do {                                                                                                                            \
        if (upt == 1)                                                                                                               \
            VSOM_TINY_LAUNCH(KIND, LOC, 1);                                                                                         \
        else if (upt == 2)                                                                                                          \
            VSOM_TINY_LAUNCH(KIND, LOC, 2);                                                                                         \
        else                                                                                                                        \
            VSOM_TINY_LAUNCH(KIND, LOC, 4);                                                                                         \
    } while (0)
    if (c->transform == VSOM_MEDIAN) {
        if (local)
            VSOM_TINY_LAUNCH_U(VSOM_MEDIAN, true);
        else
            VSOM_TINY_LAUNCH_U(VSOM_MEDIAN, false);
    } else {
        if (local)
            VSOM_TINY_LAUNCH_U(VSOM_STANDARD, true);
        else
            VSOM_TINY_LAUNCH_U(VSOM_STANDARD, false);
    }
#undef VSOM_TINY_LAUNCH_U
#undef VSOM_TINY_LAUNCH
    return VSOM_OK;
}

// ---- the same chunk for many maps in one launch per instantiation, one workgroup per map (vsom_ensemble.hip) -------------
size_t vsom_onl_tiny_desc_bytes() { return sizeof(OnlTinyArgs); }

int vsom_onl_tiny_prepare(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk, bool want_lb,
                          size_t lds_limit, void *desc, int *group, size_t *smem, int *lut_slot)
{
    *group = -1;
    const size_t need = online_tiny_lds_bytes(c);
    if (!online_tiny_applies(c, sigma) || need + 2 * sizeof(u64) > lds_limit)    // (+ the kernel's static key slots)
        return VSOM_OK;                                                          // the ordinary path
    const double *lutd = nullptr;
    int lslot = 0;
    if (int rc = ensure_lutd_host(c, sigma, &lutd, &lslot))     // as train_online_chunk_impl: the kernel reads the pinned slot
        return rc;
    u64 *lbh = nullptr;
    if (want_lb) {                                               // (B <= 4096 here)
        VSOM_ALLOC_CHECK(vsom_grow(c->out_pinned, 8192, c->stream));
        lbh = c->out_pinned.p;
    }
    OnlTinyArgs a;
    fill_chunk_tiny_args(c, eta, sigma, decay_fn, lutd, (int)c->W, first_chunk, lbh, a);
    std::memcpy(desc, &a, sizeof(a));
    *group = chunk_tiny_group(c, sigma);
    *smem = need;
    *lut_slot = lslot;
    return VSOM_OK;
}

// the launch that read the member's table slot has completed (the caller has waited for it): the slot is free again --
// what lutd_host_used's event would say once it has completed, without an event record per member
void vsom_onl_tiny_done(vsom_ctx *c, int lut_slot) { c->lutd_ev_valid[lut_slot] = false; }

static const void *onl_tiny_many_fn(int group)
{
#define VSOM_TINY_MANY(KIND, LOC, UU) reinterpret_cast<const void *>(online_tiny_chunk_many_kernel<KIND, LOC, UU>)
    switch (group) {
    case 0: return VSOM_TINY_MANY(VSOM_STANDARD, false, 1);
    case 1: return VSOM_TINY_MANY(VSOM_STANDARD, false, 2);
    case 2: return VSOM_TINY_MANY(VSOM_STANDARD, false, 4);
    case 3: return VSOM_TINY_MANY(VSOM_STANDARD, true, 1);
    case 4: return VSOM_TINY_MANY(VSOM_STANDARD, true, 2);
    case 5: return VSOM_TINY_MANY(VSOM_STANDARD, true, 4);
    case 6: return VSOM_TINY_MANY(VSOM_MEDIAN, false, 1);
    case 7: return VSOM_TINY_MANY(VSOM_MEDIAN, false, 2);
    case 8: return VSOM_TINY_MANY(VSOM_MEDIAN, false, 4);
    case 9: return VSOM_TINY_MANY(VSOM_MEDIAN, true, 1);
    case 10: return VSOM_TINY_MANY(VSOM_MEDIAN, true, 2);
    case 11: return VSOM_TINY_MANY(VSOM_MEDIAN, true, 4);
    default: return nullptr;
    }
#undef VSOM_TINY_MANY
}

// The dynamic LDS limit of a *_many instantiation (more than the 64 KiB a launch may ask for by default).  The attribute
// belongs to the function, process-wide, so its record does too: per device and instantiation, raised only -- to the
// device's limit less the kernel's static key slots, which every member admitted by vsom_onl_tiny_prepare fits -- and
// never lowered, so no ensemble can take away what another one's launch relies on.
static std::mutex g_onl_many_lds_mu;
static std::vector<std::array<size_t, VSOM_ONL_TINY_GROUPS>> g_onl_many_lds;   // [device][group]: bytes set

int vsom_onl_tiny_ready(int group, int device, size_t lds_limit)
{
    const void *fn = onl_tiny_many_fn(group);
    if (!fn || device < 0 || lds_limit <= 2 * sizeof(u64))
        return vsom_fail(VSOM_ERR_INVALID, "bad one-launch chunk group");
    const size_t want = lds_limit - 2 * sizeof(u64);
    std::lock_guard<std::mutex> lock(g_onl_many_lds_mu);
    if ((size_t)device >= g_onl_many_lds.size())
        g_onl_many_lds.resize((size_t)device + 1, std::array<size_t, VSOM_ONL_TINY_GROUPS>{});
    size_t &set = g_onl_many_lds[(size_t)device][(size_t)group];
    if (set >= want)
        return VSOM_OK;
    VSOM_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want));
    set = want;
    return VSOM_OK;
}

int vsom_onl_tiny_launch_many(int group, const void *desc_dev, unsigned count, size_t smem, hipStream_t s)
{
    const void *fn = onl_tiny_many_fn(group);
    if (!fn)
        return vsom_fail(VSOM_ERR_INVALID, "bad one-launch chunk group");
    const OnlTinyArgs *args = static_cast<const OnlTinyArgs *>(desc_dev);
    void *argv[] = {&args};
    VSOM_HIP_CHECK(hipLaunchKernel(fn, dim3(count), dim3(1024), argv, smem, s));
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}
