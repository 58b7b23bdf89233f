// vsom_tiny_masked.hip -- the masked flavour of the one-workgroup batch epochs (vsom_tiny.hip is the plain one): for maps
// so small that the dozen launches of vsom_batch_epoch_masked (vsom_masked_train.hip) cost more than the work, ONE workgroup
// runs whole masked epochs in one launch (gfx950; Standard / Median, strict arithmetic: this translation unit is built with
// the strict flags).  The two flavours share the schedule descriptor and its epoch step (TinySched, tiny_schedule_epoch:
// vsom_device.hpp), the round image (vsom_sched_round.hpp) and the host's round loop (vsom_schedule_rounds, vsom_tiny.hip).
//   phase 1  every (sample, node) masked distance by 8-lane groups (masked_group_dist: r_d = valid ? m_d - x_d : +0), the
//            argmin through an LDS atomicMin on the (distance, index) key -- or findLocalBmu's walk on the same distance,
//            one wavefront per sample;  bmuHits;  MSE summed in sample order
//   phase 2  one thread per (node, column) chain over the rows in load order: Wall sums w over ALL rows (weightMap), a row
//            valid at the column takes the step of the unmasked chain with the column's own weight sum W_d, an invalid
//            one is skipped; map = M, sigmaMap = sqrt(S / W_d)
// so the results are those of vsom_batch_epoch_masked bit for bit.  The kernels run a schedule of epochs (a single epoch is
// a schedule of one): vsom_batch_schedule_masked here, vsom_ensemble_batch_epoch_masked and
// vsom_ensemble_batch_schedule_masked in vsom_ensemble.hip (one workgroup per map).
#include "vsom_masked_dist.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

struct TinyMaskedArgs {
    DistArgs d;                  // search operands: Xs rows, map rows
    float *map, *sigma, *weight;
    u64 *hits, *lastbmu;
    float *sqres, *mse;
    const float *lut;
    const unsigned char *valid;  // B x J validity bytes as given (one: J bytes for every row); nonzero = valid
    int lutw, luth;              // the table (copied into LDS)
    int N, W, H, Dc, pitch, B, is_first;
    int stage_x;                 // samples fit into LDS
    int one;                     // one validity row for every sample
    int nw;                      // validity words per column in LDS: ceil(B / 32), or 1 with `one`
};

// The loop over the epochs is in the kernel, as in tiny_batch_schedule_kernel (vsom_tiny.hip): between two epochs one
// barrier -- phase 2 stored map rows (a.map) that the next phase 1 reads (a.d.ma) from other threads of this workgroup, and
// the LDS arrays are written again.  The map pointers stay plain (no __restrict__, no __ldg): no load of them may go
// through the scalar cache, which vector stores do not update.
// (TinySched and tiny_schedule_epoch: vsom_device.hpp.  A struct of its own rather than an alias, so that the kernels'
// parameter type keeps its name)
struct TinyMaskedSchedArgs : TinySched<TinyMaskedArgs> {};

template <int KIND>
__global__ __launch_bounds__(256) void tiny_masked_schedule_kernel(TinyMaskedSchedArgs s)
{
    for (int ep = 0; ep < s.epochs; ++ep) {
        const TinyMaskedArgs a = tiny_schedule_epoch(s, ep);
#include "vsom_tiny_masked_body.inc"
    }
}

// one map per workgroup (vsom_ensemble.hip): the same on the workgroup's descriptor (the index is uniform: scalar loads)
template <int KIND>
__global__ __launch_bounds__(256) void tiny_masked_schedule_many_kernel(const TinyMaskedSchedArgs *__restrict__ args)
{
    const TinyMaskedSchedArgs s = args[blockIdx.x];
    for (int ep = 0; ep < s.epochs; ++ep) {
        const TinyMaskedArgs a = tiny_schedule_epoch(s, ep);
#include "vsom_tiny_masked_body.inc"
    }
}

const char *vsom_masked_train_refusal(const vsom_ctx *c)
{
    if (c->cu)
        return "a custom context has no masked epoch (vsom_batch_epoch_masked)";
    if (c->transform == VSOM_CLR)
        return "CLR contexts are not supported by the masked epoch (residual and step run over column pairs)";
    if (c->update_mode != VSOM_UPDATE_STRICT)
        return "the masked chains exist in the strict update mode only";
    return nullptr;
}

// The dynamic LDS of one epoch: the per-sample arrays, the staged rows, the table, the validity bits.  The rows are staged
// when they are at most 40 KB (as in the unmasked body) and everything still fits lds_limit beside them; *stage_x says so.
static size_t tinym_lds_bytes(const vsom_ctx *c, int one_mask, uint32_t lut_w, uint32_t lut_h, size_t lds_limit, int *stage_x)
{
    const size_t B = c->B, J = c->part_len;
    const size_t nw = one_mask ? 1 : (B + 31) / 32;
    size_t smem = B * (sizeof(u64) + sizeof(int2) + sizeof(float) + sizeof(int));
    smem += (size_t)lut_w * lut_h * sizeof(float);          // N <= 4096 here: at most 16 KB
    smem += J * nw * sizeof(unsigned);
    const size_t xbytes = B * J * sizeof(float);
    *stage_x = B * J <= 10240 && smem + xbytes <= lds_limit ? 1 : 0;
    return smem + (*stage_x ? xbytes : 0);
}

bool vsom_tiny_masked_applies(const vsom_ctx *c, int one_mask, size_t lds_limit)
{
    if (vsom_masked_train_refusal(c) || !vsom_tiny_applies(c))
        return false;
    uint32_t lw, lh;
    vsom_lut_dims(c, &lw, &lh);
    int stage;
    return tinym_lds_bytes(c, one_mask, lw, lh, lds_limit, &stage) <= lds_limit;
}

bool vsom_tiny_masked_schedule_applies(const vsom_ctx *c, int one_mask, const double *sigma, size_t epochs, size_t lds_limit)
{
    for (size_t ep = 0; ep < epochs; ++ep)
        if (!std::isfinite(sigma[ep]))
            return false;
    return vsom_tiny_masked_applies(c, one_mask, lds_limit);
}

size_t vsom_tiny_masked_sched_desc_bytes() { return sizeof(TinyMaskedSchedArgs); }

int vsom_tiny_masked_sched_fill(vsom_ctx *c, const unsigned char *valid_dev, int one_mask, size_t lds_limit, const float *lut_dev,
                                const unsigned *tab_dev, float *mse, size_t epochs, int first, int reset_bmu, void *desc,
                                size_t *smem)
{
    uint32_t lw, lh;
    vsom_lut_dims(c, &lw, &lh);
    TinyMaskedSchedArgs s;
    TinyMaskedArgs &a = s.t;
    *smem = tinym_lds_bytes(c, one_mask, lw, lh, lds_limit, &a.stage_x);
    a.d.xa = a.d.xb = c->Xs.p;
    a.d.ldx = (int)c->xpitch;
    a.d.ma = a.d.mb = c->map.p;
    a.d.ldm = (int)c->pitch;
    a.d.L = (int)c->part_len;
    a.map = c->map.p;
    a.sigma = c->sigma.p;
    a.weight = c->weight.p;
    a.hits = c->hits.p;
    a.lastbmu = c->lastbmu.p;
    a.sqres = c->sqres.p;
    a.mse = mse;
    a.lut = lut_dev;
    a.valid = valid_dev;
    a.lutw = (int)lw;
    a.luth = (int)lh;
    a.N = (int)c->N;
    a.W = (int)c->W;
    a.H = (int)c->H;
    a.Dc = (int)c->part_len;
    a.pitch = (int)c->pitch;
    a.B = (int)c->B;
    a.is_first = 0;
    a.one = one_mask ? 1 : 0;
    a.nw = one_mask ? 1 : (int)((c->B + 31) / 32);
    s.tab = tab_dev;
    s.epochs = (int)epochs;
    s.first = first ? 1 : 0;
    s.reset_bmu = reset_bmu ? 1 : 0;
    s.pad = 0;
    std::memcpy(desc, &s, sizeof(s));
    return c->transform;
}

int vsom_tiny_masked_sched_launch_many(int group, const void *desc_dev, unsigned count, size_t smem, hipStream_t s)
{
    const TinyMaskedSchedArgs *args = static_cast<const TinyMaskedSchedArgs *>(desc_dev);
    if (group == VSOM_MEDIAN)
        hipLaunchKernelGGL(tiny_masked_schedule_many_kernel<VSOM_MEDIAN>, dim3(count), dim3(256), smem, s, args);
    else
        hipLaunchKernelGGL(tiny_masked_schedule_many_kernel<VSOM_STANDARD>, dim3(count), dim3(256), smem, s, args);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}

int vsom_masked_tiny_applies(const vsom_ctx *c, int one_mask)
{
    return c && c->chunk_loaded && vsom_tiny_masked_applies(c, one_mask, (size_t)64 << 10) ? 1 : 0;
}

int vsom_batch_schedule_masked(vsom_ctx *c, const double *sigma, size_t epochs, int reset_bmu, const uint8_t *valid_host,
                               int one_mask, float *mse_out)
{
    if (!c)
        return vsom_fail(VSOM_ERR_INVALID, "null context");
    if (epochs == 0)
        return VSOM_OK;
    if (!sigma || !mse_out)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_schedule_masked: null sigma or mse_out");
    if (!valid_host)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_schedule_masked: valid_host is null");
    if (const char *why = vsom_masked_train_refusal(c))
        return vsom_fail(VSOM_ERR_INVALID, std::string("vsom_batch_schedule_masked: ") + why);
    if (const char *why = vsom_schedule_refusal(c))
        return vsom_fail(VSOM_ERR_INVALID, why);
    const size_t lds_cap = (size_t)64 << 10;     // (no attribute is raised for the batch kernels)
    if (!vsom_tiny_masked_schedule_applies(c, one_mask, sigma, epochs, lds_cap))
        return vsom_schedule_loop(c, epochs, reset_bmu, [&](size_t ep) {
            return vsom_batch_epoch_masked(c, sigma[ep], ep == 0, valid_host, one_mask, &mse_out[ep]);
        });
    return vsom_schedule_rounds(c, sigma, epochs, reset_bmu, valid_host, one_mask, mse_out,
                                [](vsom_ctx *ctx, const unsigned char *valid_dev, int one, const float *lut_dev,
                                   const unsigned *tab_dev, float *mse, size_t cnt, int first, int reset) {
                                    TinyMaskedSchedArgs s;
                                    size_t smem = 0;
                                    vsom_tiny_masked_sched_fill(ctx, valid_dev, one, (size_t)64 << 10, lut_dev, tab_dev, mse, cnt,
                                                                first, reset, &s, &smem);
                                    if (ctx->transform == VSOM_MEDIAN)
                                        hipLaunchKernelGGL(tiny_masked_schedule_kernel<VSOM_MEDIAN>, dim3(1), dim3(256), smem, ctx->stream, s);
                                    else
                                        hipLaunchKernelGGL(tiny_masked_schedule_kernel<VSOM_STANDARD>, dim3(1), dim3(256), smem, ctx->stream, s);
                                    VSOM_HIP_CHECK(hipGetLastError());
                                    return (int)VSOM_OK;
                                });
}
