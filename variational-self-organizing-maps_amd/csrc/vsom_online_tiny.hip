// vsom_online_tiny.hip -- tiny maps: the whole chunk loop of Som::trainBasicSom (Som.cpp:1159-1171) in ONE launch of ONE
// workgroup.  One family of kernels from one body (vsom_tiny_online_body.inc): flavour {plain, over the valid entries only
// (vsom_train_online_chunk_masked)} x form {the context's own launch, one workgroup per map for
// ensembles (vsom_onl_tiny_*, called by vsom_ensemble.hip)} x the 12 instantiations (kind, local, U).  One table holds their
// addresses, one registry their raised LDS limits.  Two of the chunk loops vsom_train_online_chunk* picks from
// (vsom_online.hip, the index of the family).
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
//
// Over the valid entries (the arithmetic of vsom_online_masked.hip's per-sample loop, bit for bit):
//   validity   the bytes as the caller gave them (B x J, nonzero = valid; or ONE row of J): staged into LDS beside each block
//              of TINY_XBLOCK / D rows -- no pack launch, no packed copy
//   A, D       the square of a value is valid ? fl(fl(m - x)^2) : +0, a select (x at an invalid position may be NaN or +-inf);
//              the row sums keep Eigen's order (onl_tiny_row_sum), the post step's distance is the masked one
//   C          the node's weight and the scalars of the step (scM, tw, hf) are the unmasked step's for every node of the
//              window, whatever the column's validity; m, S and the sigmaMap value are stepped at the valid columns only
//   sigmaMap   online_node_update_masked writes sigmaMap[n, d] with the weight of the step that stepped column d; a later
//              visit of node n with d invalid raises the weight and leaves sigmaMap[n, d].  So every value keeps the weight of
//              its last VALID step in a register and the write-back takes sqrt(|S / that weight|), only for values that had a
//              valid step
//   bits       a value no valid step touched is not written back: map, SMap and sigmaMap keep its bits, NaN payloads included
#include "vsom_online_tiny.hpp"
#include <cstring>
#include <map>
#include <mutex>

#ifdef VSOM_DEVELOPMENT
// cycle stamps of one sample of the one-launch chunk (sample 5 of the chunk; s_memtime): [2 w + p] = wavefront w (0: first,
// 1: last) at phase boundary p (tools/exp/tiny_stamps.py)
__device__ unsigned long long vsom_tiny_stamps[64];
#define TINY_STAMP(p) do { if (!MASKED && j == 5 && (tid == 0 || tid == 1023)) vsom_tiny_stamps[(tid ? 16 : 0) + (p)] = __builtin_readcyclecounter(); } while (0)
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
    constexpr bool MASKED = false;
#include "vsom_tiny_online_body.inc"
}

// one map per workgroup (vsom_ensemble.hip): the same body on the workgroup's descriptor (the index is uniform: scalar
// loads).  Included as text, not called, so that the single-map kernel's code object stays instruction for instruction
// what it was (see tiny_batch_epoch_many_kernel)
template <int KIND, bool LOCAL, int U>
__global__ __launch_bounds__(1024) void online_tiny_chunk_many_kernel(const OnlTinyArgs *__restrict__ args)
{
    constexpr bool MASKED = false;
    const OnlTinyArgs a = args[blockIdx.x];
#include "vsom_tiny_online_body.inc"
}

template <int KIND, bool LOCAL, int U>
__global__ __launch_bounds__(1024) void online_tiny_masked_chunk_kernel(OnlTinyMaskedArgs a)
{
    constexpr bool MASKED = true;
#include "vsom_tiny_online_body.inc"
}

template <int KIND, bool LOCAL, int U>
__global__ __launch_bounds__(1024) void online_tiny_masked_chunk_many_kernel(const OnlTinyMaskedArgs *__restrict__ args)
{
    constexpr bool MASKED = true;
    const OnlTinyMaskedArgs a = args[blockIdx.x];
#include "vsom_tiny_online_body.inc"
}

// ---- the family's table: [masked][many][group] -> the kernel's address, built once from the template parameters ---------
// group = (Median ? 6 : 0) + (local ? 3 : 0) + (0, 1, 2 for U = 1, 2, 4); chunk_tiny_group is the one place that maps a
// context and a sigma to it
struct OnlTinyKernels {
    const void *fn[2][2][VSOM_ONL_TINY_GROUPS];
};

template <int G>
static void onl_tiny_fill(OnlTinyKernels &t)
{
    constexpr int KIND = G >= 6 ? VSOM_MEDIAN : VSOM_STANDARD, U = 1 << (G % 3);
    constexpr bool LOCAL = G % 6 >= 3;
    t.fn[0][0][G] = reinterpret_cast<const void *>(online_tiny_chunk_kernel<KIND, LOCAL, U>);
    t.fn[0][1][G] = reinterpret_cast<const void *>(online_tiny_chunk_many_kernel<KIND, LOCAL, U>);
    t.fn[1][0][G] = reinterpret_cast<const void *>(online_tiny_masked_chunk_kernel<KIND, LOCAL, U>);
    t.fn[1][1][G] = reinterpret_cast<const void *>(online_tiny_masked_chunk_many_kernel<KIND, LOCAL, U>);
    if constexpr (G + 1 < VSOM_ONL_TINY_GROUPS)
        onl_tiny_fill<G + 1>(t);
}

static const void *onl_tiny_fn(bool masked, bool many, int group)
{
    static const OnlTinyKernels t = [] {
        OnlTinyKernels k;
        onl_tiny_fill<0>(k);
        return k;
    }();
    return group >= 0 && group < VSOM_ONL_TINY_GROUPS ? t.fn[masked][many][group] : nullptr;
}

static int chunk_tiny_group(const vsom_ctx *c, double sigma)
{
    const bool local = !(sigma > 1);                  // SIGMA_SWITCH_TO_LOCAL (SOM.hpp:37, Som.cpp:891)
    const size_t nd = (size_t)c->N * c->part_len;
    const int ui = nd <= 1024 ? 0 : (nd <= 2048 ? 1 : 2);      // values per thread (the kernel is bound by instruction issue)
    return (c->transform == VSOM_MEDIAN ? 6 : 0) + (local ? 3 : 0) + ui;
}

// The dynamic LDS limit of a kernel (more than the 64 KiB a launch may ask for by default; 160 KiB per CU).  The attribute
// belongs to the function, process-wide, so its record does too: per device and kernel, raised only and never lowered, so
// no context or ensemble can take away what another one's launch relies on.
static int onl_tiny_raise_lds(const void *fn, int device, size_t want)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> set;   // (device, kernel) -> bytes set
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = set[std::make_pair(device, fn)];
    if (have >= want)
        return VSOM_OK;
    VSOM_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want));
    have = want;
    return VSOM_OK;
}

constexpr size_t ONL_TINY_SINGLE_LDS = 96 << 10;   // the dynamic LDS limit the context's own launch sets
constexpr size_t ONL_TINY_KEYS = 2 * sizeof(u64);  // the kernels' static key slots

// the chunk's dynamic LDS: the tables, the squares, a block of staged rows (masked: and their validity bytes), the counts
static size_t online_tiny_lds_bytes(const vsom_ctx *c, bool masked)
{
    const size_t N = c->N, D = c->part_len;
    return N * (16 + 8 + 8) + (N * (D | 1) + 2 * ((D + 3) & ~(size_t)3) + TINY_XBLOCK) * sizeof(float) + N * 8 +
           (c->B + 8) * sizeof(unsigned short) + (masked ? TINY_XBLOCK : 0);
}

bool online_tiny_applies(const vsom_ctx *c, double sigma)
{
    return c->use_tiny && c->transform != VSOM_CLR && sigma == sigma && c->B > 0 && c->N <= 1024 &&
           (size_t)c->N * c->part_len <= 4096 && c->part_len <= 512 && c->B <= 4096 && c->bmu_mode == VSOM_BMU_AUTO;   // (EXACT / SHORTLIST name the per-sample forms)
}

bool vsom_onl_tiny_fits(const vsom_ctx *c, double sigma, bool masked, size_t lds_limit)
{
    return c && c->chunk_loaded && !c->cu && online_tiny_applies(c, sigma) &&
           online_tiny_lds_bytes(c, masked) + ONL_TINY_KEYS <= lds_limit;
}

extern "C" int vsom_online_masked_tiny_applies(const vsom_ctx *c, double sigma, int one_mask)
{
    (void)one_mask;   // (one row or B: the validity block in LDS has one size)
    return vsom_onl_tiny_fits(c, sigma, true, ONL_TINY_SINGLE_LDS) ? 1 : 0;
}

// the descriptor from the context; valid_dev null: the plain chunk, whose descriptor ends before the validity fields
static void fill_chunk_tiny_args(vsom_ctx *c, double eta, double sigma, int decay_fn, const double *lutd, int lutw,
                                 int first_chunk, u64 *lastbmu_host, const unsigned char *valid_dev, bool one,
                                 OnlTinyMaskedArgs &a)
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
    a.V = valid_dev;
    a.ldv = (int)c->J;
    a.one = one ? 1 : 0;
}

int enqueue_chunk_tiny(vsom_ctx *c, double eta, double sigma, int decay_fn, const double *lutd, int lutw, int first_chunk,
                       u64 *lastbmu_host, const unsigned char *valid_dev, bool one)
{
    const bool masked = valid_dev != nullptr;
    OnlTinyMaskedArgs a;
    fill_chunk_tiny_args(c, eta, sigma, decay_fn, lutd, lutw, first_chunk, lastbmu_host, valid_dev, one, a);
    const void *fn = onl_tiny_fn(masked, false, chunk_tiny_group(c, sigma));
    if (int rc = onl_tiny_raise_lds(fn, c->device, ONL_TINY_SINGLE_LDS))
        return rc;
    void *argv[] = {&a};     // (the plain kernel takes the OnlTinyArgs the descriptor begins with)
    VSOM_HIP_CHECK(hipLaunchKernel(fn, dim3(1), dim3(1024), argv, online_tiny_lds_bytes(c, masked), c->stream));
    return VSOM_OK;
}

// ---- the same chunk for many maps in one launch per instantiation, one workgroup per map (vsom_ensemble.hip) -------------
size_t vsom_onl_tiny_desc_bytes(bool masked) { return masked ? sizeof(OnlTinyMaskedArgs) : sizeof(OnlTinyArgs); }

int vsom_onl_tiny_prepare(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk, bool want_lb,
                          const unsigned char *valid_dev, int one_mask, void *desc, int *group, size_t *smem, int *lut_slot)
{
    const bool masked = valid_dev != nullptr;
    *group = -1;
    const double *lutd = nullptr;
    int lslot = 0;
    if (int rc = ensure_lutd_host(c, sigma, &lutd, &lslot))     // as train_online_chunk_impl: the kernel reads the pinned slot
        return rc;
    u64 *lbh = nullptr;
    if (want_lb) {                                               // (B <= 4096 here)
        VSOM_ALLOC_CHECK(vsom_grow(c->out_pinned, 8192, c->stream));
        lbh = c->out_pinned.p;
    }
    OnlTinyMaskedArgs a;
    fill_chunk_tiny_args(c, eta, sigma, decay_fn, lutd, (int)c->W, first_chunk, lbh, valid_dev, one_mask != 0, a);
    std::memcpy(desc, &a, vsom_onl_tiny_desc_bytes(masked));
    *group = chunk_tiny_group(c, sigma);
    *smem = online_tiny_lds_bytes(c, masked);
    *lut_slot = lslot;
    return VSOM_OK;
}

// the launch that read the member's table slot has completed (the caller has waited for it): the slot is free again --
// what lutd_host_used's event would say once it has completed, without an event record per member
void vsom_onl_tiny_done(vsom_ctx *c, int lut_slot) { c->lutd_ev_valid[lut_slot] = false; }

// every member admitted by vsom_onl_tiny_fits fits the device's limit less the kernels' static key slots
int vsom_onl_tiny_ready(bool masked, int group, int device, size_t lds_limit)
{
    const void *fn = onl_tiny_fn(masked, true, group);
    if (!fn || device < 0 || lds_limit <= ONL_TINY_KEYS)
        return vsom_fail(VSOM_ERR_INVALID, "bad one-launch chunk group");
    return onl_tiny_raise_lds(fn, device, lds_limit - ONL_TINY_KEYS);
}

int vsom_onl_tiny_launch_many(bool masked, int group, const void *desc_dev, unsigned count, size_t smem, hipStream_t s)
{
    const void *fn = onl_tiny_fn(masked, true, group);
    if (!fn)
        return vsom_fail(VSOM_ERR_INVALID, "bad one-launch chunk group");
    void *argv[] = {&desc_dev};
    VSOM_HIP_CHECK(hipLaunchKernel(fn, dim3(count), dim3(1024), argv, smem, s));
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}
