// vsom_online_tiny_masked.hip -- tiny maps: the chunk loop of vsom_train_online_chunk_masked in ONE launch of ONE workgroup,
// and the same body with one workgroup per map for ensembles (vsom_onl_tiny_masked_*, called by vsom_ensemble.hip;
// DESIGN.md section 4u).  The fourth chunk loop vsom_train_online_chunk* picks from (vsom_online.hip, the index of the family).
//
// The kernel is online_tiny_chunk_kernel (vsom_online_tiny.hip: 1024 threads, U = 1, 2 or 4 model values per thread in
// registers for the whole chunk, two barriers per sample plus the walk's for sigma <= 1, the same instantiation grid) with
// the arithmetic of vsom_online_masked.hip:
//   validity   the bytes as the caller gave them (B x J, nonzero = valid; or ONE row of J): staged into LDS beside each block
//              of TINY_XBLOCK / D rows -- no pack launch, no packed copy
//   A, D       the square of a value is valid ? fl(fl(m - x)^2) : +0, a select (x at an invalid position may be NaN or +-inf);
//              the row sums keep Eigen's order (onl_tiny_row_sum), the post step's distance is the masked one
//   C          the node's weight and the scalars of the step (scM, tw, hf) are the unmasked step's for every node of the
//              window, whatever the column's validity; m, S and the sigmaMap value are stepped at the valid columns only
//   sigmaMap   online_node_update_masked writes sigmaMap[n, d] with the weight of the step that stepped column d; a later
//              visit of node n with d invalid raises the weight and leaves sigmaMap[n, d].  So every value keeps the weight of
//              its last VALID step in a register and the write-back takes sqrt(|S / that weight|) -- not the final weight, as
//              the plain chunk may -- and only for values that had a valid step
//   bits       a value no valid step touched is not written back: map, SMap and sigmaMap keep its bits, NaN payloads included
// Results are those of the per-sample loop of vsom_online_masked.hip bit for bit: map, SMap, sigmaMap, weightMap, bmuHits,
// lastBMU, the MSE and the MSE word.
#include "vsom_online_tiny.hpp"
#include <cstring>
#include <array>
#include <mutex>

// OnlTinyArgs and the validity bytes (a descriptor of its own: the stride of OnlTinyArgs stays)
struct OnlTinyMaskedArgs : OnlTinyArgs {
    const unsigned char *V;  // validity bytes on the device: B rows of ldv bytes, or one row (one != 0)
    int ldv, one;
};

template <int KIND, bool LOCAL, int U>     // U = values per thread (1, 2, 4): N D <= 1024 U
__global__ __launch_bounds__(1024) void online_tiny_masked_chunk_kernel(OnlTinyMaskedArgs a)
{
#include "vsom_tiny_online_masked_body.inc"
}

// one map per workgroup (vsom_ensemble.hip): the same body on the workgroup's descriptor, included as text
template <int KIND, bool LOCAL, int U>
__global__ __launch_bounds__(1024) void online_tiny_masked_chunk_many_kernel(const OnlTinyMaskedArgs *__restrict__ args)
{
    const OnlTinyMaskedArgs a = args[blockIdx.x];
#include "vsom_tiny_online_masked_body.inc"
}

// the plain chunk's arrays and the block's validity bytes (every per-value record of the masked step is in registers)
static size_t online_tiny_masked_lds_bytes(const vsom_ctx *c) { return online_tiny_lds_bytes(c) + TINY_XBLOCK; }

constexpr size_t ONL_TINY_MASKED_LDS = 96 << 10;   // the dynamic LDS limit the single launch sets (160 KiB per CU)
constexpr size_t ONL_TINY_KEYS = 2 * sizeof(u64);  // the kernel's static key slots

// the one-launch masked chunk applies and its LDS need (dynamic + the static key slots) is within lds_limit
bool vsom_onl_tiny_masked_fits(const vsom_ctx *c, double sigma, size_t lds_limit)
{
    return c && c->chunk_loaded && !c->cu && online_tiny_applies(c, sigma) &&
           online_tiny_masked_lds_bytes(c) + ONL_TINY_KEYS <= lds_limit;
}

extern "C" int vsom_online_masked_tiny_applies(const vsom_ctx *c, double sigma, int one_mask)
{
    (void)one_mask;   // (one row or B: the validity block in LDS has one size)
    return vsom_onl_tiny_masked_fits(c, sigma, ONL_TINY_MASKED_LDS) ? 1 : 0;
}

static void fill_masked_args(vsom_ctx *c, double eta, double sigma, int decay_fn, const double *lutd, int lutw,
                             int first_chunk, u64 *lastbmu_host, const unsigned char *valid_dev, bool one,
                             OnlTinyMaskedArgs &a)
{
    fill_chunk_tiny_args(c, eta, sigma, decay_fn, lutd, lutw, first_chunk, lastbmu_host, a);
    a.V = valid_dev;
    a.ldv = (int)c->J;
    a.one = one ? 1 : 0;
}

int enqueue_chunk_tiny_masked(vsom_ctx *c, double eta, double sigma, int decay_fn, const double *lutd, int lutw,
                              int first_chunk, u64 *lastbmu_host, const unsigned char *valid_dev, bool one)
{
    OnlTinyMaskedArgs a;
    fill_masked_args(c, eta, sigma, decay_fn, lutd, lutw, first_chunk, lastbmu_host, valid_dev, one, a);
    const size_t smem = online_tiny_masked_lds_bytes(c);
    const bool local = !(sigma > 1);                  // SIGMA_SWITCH_TO_LOCAL (SOM.hpp:37, Som.cpp:891)
    const size_t nd = (size_t)c->N * c->part_len;
    const int upt = nd <= 1024 ? 1 : (nd <= 2048 ? 2 : 4);     // values per thread
#define VSOM_TINY_LAUNCH(KIND, LOC, UU)                                                                                             \
    do {                                                                                                                            \
        if (!c->tiny_masked_lds_attr[(LOC ? 3 : 0) + (UU == 1 ? 0 : (UU == 2 ? 1 : 2))]) {                                          \
            /* (more than the 64 KiB a launch may ask for by default) */                                                            \
            VSOM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(online_tiny_masked_chunk_kernel<KIND, LOC, UU>),      \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)ONL_TINY_MASKED_LDS));              \
            c->tiny_masked_lds_attr[(LOC ? 3 : 0) + (UU == 1 ? 0 : (UU == 2 ? 1 : 2))] = true;                                     \
        }                                                                                                                           \
        hipLaunchKernelGGL((online_tiny_masked_chunk_kernel<KIND, LOC, UU>), dim3(1), dim3(1024), smem, c->stream, a);              \
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
size_t vsom_onl_tiny_masked_desc_bytes() { return sizeof(OnlTinyMaskedArgs); }

// the caller has found vsom_onl_tiny_masked_fits(c, sigma, lds_limit); valid_dev: the member's validity bytes on the device
int vsom_onl_tiny_masked_prepare(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk, bool want_lb,
                                 const unsigned char *valid_dev, int one_mask, void *desc, int *group, size_t *smem,
                                 int *lut_slot)
{
    *group = -1;
    const double *lutd = nullptr;
    int lslot = 0;
    if (int rc = ensure_lutd_host(c, sigma, &lutd, &lslot))     // the kernel reads the pinned slot
        return rc;
    u64 *lbh = nullptr;
    if (want_lb) {                                               // (B <= 4096 here)
        VSOM_ALLOC_CHECK(vsom_grow(c->out_pinned, 8192, c->stream));
        lbh = c->out_pinned.p;
    }
    OnlTinyMaskedArgs a;
    fill_masked_args(c, eta, sigma, decay_fn, lutd, (int)c->W, first_chunk, lbh, valid_dev, one_mask != 0, a);
    std::memcpy(desc, &a, sizeof(a));
    *group = chunk_tiny_group(c, sigma);
    *smem = online_tiny_masked_lds_bytes(c);
    *lut_slot = lslot;
    return VSOM_OK;
}

static const void *onl_tiny_masked_many_fn(int group)
{
#define VSOM_TINY_MANY(KIND, LOC, UU) reinterpret_cast<const void *>(online_tiny_masked_chunk_many_kernel<KIND, LOC, UU>)
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

// the dynamic LDS limit of a *_many instantiation: per device and instantiation, raised only (vsom_onl_tiny_ready)
static std::mutex g_onl_masked_many_lds_mu;
static std::vector<std::array<size_t, VSOM_ONL_TINY_GROUPS>> g_onl_masked_many_lds;   // [device][group]: bytes set

int vsom_onl_tiny_masked_ready(int group, int device, size_t lds_limit)
{
    const void *fn = onl_tiny_masked_many_fn(group);
    if (!fn || device < 0 || lds_limit <= ONL_TINY_KEYS)
        return vsom_fail(VSOM_ERR_INVALID, "bad one-launch masked chunk group");
    const size_t want = lds_limit - ONL_TINY_KEYS;
    std::lock_guard<std::mutex> lock(g_onl_masked_many_lds_mu);
    if ((size_t)device >= g_onl_masked_many_lds.size())
        g_onl_masked_many_lds.resize((size_t)device + 1, std::array<size_t, VSOM_ONL_TINY_GROUPS>{});
    size_t &set = g_onl_masked_many_lds[(size_t)device][(size_t)group];
    if (set >= want)
        return VSOM_OK;
    VSOM_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want));
    set = want;
    return VSOM_OK;
}

int vsom_onl_tiny_masked_launch_many(int group, const void *desc_dev, unsigned count, size_t smem, hipStream_t s)
{
    const void *fn = onl_tiny_masked_many_fn(group);
    if (!fn)
        return vsom_fail(VSOM_ERR_INVALID, "bad one-launch masked chunk group");
    const OnlTinyMaskedArgs *args = static_cast<const OnlTinyMaskedArgs *>(desc_dev);
    void *argv[] = {&args};
    VSOM_HIP_CHECK(hipLaunchKernel(fn, dim3(count), dim3(1024), argv, smem, s));
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}
