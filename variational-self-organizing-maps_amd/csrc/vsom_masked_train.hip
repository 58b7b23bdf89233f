// vsom_masked_train.hip -- Som::trainBatchSomEpoch (Som.cpp:756-879) over the VALID entries of the chunk only (gfx950;
// Standard / Median, strict arithmetic): vsom_batch_epoch_masked.
//
// Phase 1 is the search on the distance of vsom_masked.hip (r_d = valid ? m_d - x_d : +0): the masked tile walk for the
// first epoch, findLocalBmu's walk (vsom_local_walk_with) on the same distance afterwards, both straight into lastBMU and
// sqres; the finish step is the unmasked one.  Phase 2 runs the unmasked phase 2 over the whole map first -- it yields
// weightMap (the sum of w over ALL rows) and, bit for bit, every column that has no invalid entry in the chunk -- and then
// recomputes the "dirty" columns, those with at least one invalid entry, with a per-column weight sum:
//
//  vsom_bxy_kernel      : SomIndex(lastBMU[j]) of every row, once (the chains read it as a scalar pair); the accumulated
//                         epoch (vsom_accum.hip) runs it too
//  masked_bits_kernel   : packed validity bytes (rows x xpitch, or the one shared row) -> bits[column][row / 32], 32 rows
//                         to a word, rows past the chunk read as invalid
//  masked_dirty_kernel  : one workgroup: the columns with an invalid entry among the chunk's rows, in ascending order, and
//                         their count (ballot compaction; no host round trip)
//  masked_chain_kernel  : lane = node, one wavefront per block of CH_CB dirty columns, M, S and W_d of every column in
//                         registers.  The rows are walked in load order in groups of CH_U: the group's BMU coordinates,
//                         sample values and validity word are wave-uniform (scalar loads), w comes from the neighbourhood
//                         table the unmasked path built for this sigma.  For a valid (row, column):
//                             W_d += w ; delta = Stepper(x, M) ; M = M + (w / W_d) * delta ; S = S + (w * delta) * delta
//                         (one rounding per operation, a correctly rounded division: this translation unit is built with
//                         the strict flags), an invalid one is skipped: what x holds there is loaded and never used.  At
//                         the end map = M, sigmaMap = sqrt(S / W_d): a column without a valid row is +0 / NaN.  No atomics,
//                         no LDS; workgroups past the dirty count leave at once.
// The walk, its step, the Stepper, the table lookup and the compaction round are vsom_chain.hpp's, shared with
// vsom_accum.hip and vsom_accum_masked.hip.
#include "vsom_chain.hpp"
#include "vsom_masked_dist.hpp"
#include <algorithm>

__global__ __launch_bounds__(256) void vsom_bxy_kernel(const u64 *__restrict__ lastbmu, int B, u64 W, u64 H,
                                                       int2 *__restrict__ bxy)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= B)
        return;
    int bx, by;
    vsom_somindex(lastbmu[j], W, H, bx, by);        // SomIndex(*this, lastBMU[j]) (Som.cpp:847-849)
    bxy[j] = make_int2(bx, by);
}

// thread = (column, word): consecutive lanes read consecutive bytes of a packed row
__global__ __launch_bounds__(256) void masked_bits_kernel(const unsigned char *__restrict__ packed, int vld, int one, int J,
                                                          int B, int nwords, unsigned *__restrict__ bits)
{
    const int d = blockIdx.y * 256 + threadIdx.x, w = blockIdx.x;
    if (d >= J)
        return;
    unsigned v = 0;
    const int nt = B - 32 * w < 32 ? B - 32 * w : 32;
    for (int t = 0; t < nt; ++t)
        if (packed[(one ? 0 : (size_t)(32 * w + t) * vld) + d])
            v |= 1u << t;
    bits[(size_t)d * nwords + w] = v;
}

// dcols[0 .. *ndirty): the columns with an invalid entry in rows [0, B), ascending
__global__ __launch_bounds__(256) void masked_dirty_kernel(const unsigned *__restrict__ bits, int J, int B, int nwords,
                                                           int *__restrict__ dcols, unsigned *__restrict__ ndirty)
{
    __shared__ unsigned wcnt[4];
    unsigned base = 0;
    for (int d0 = 0; d0 < J; d0 += 256) {
        const int d = d0 + (int)threadIdx.x;
        bool dirty = false;
        if (d < J)
            for (int w = 0; w < nwords; ++w) {
                const int nt = B - 32 * w < 32 ? B - 32 * w : 32;
                const unsigned full = nt == 32 ? ~0u : (1u << nt) - 1u;
                dirty = dirty || bits[(size_t)d * nwords + w] != full;
            }
        vsom_compact_round(dirty, d, dcols, wcnt, base);
    }
    if (threadIdx.x == 0)
        *ndirty = base;
}

// bmu_local_kernel (vsom_bmu.hip) on the masked distance (masked_group_dist, vsom_masked_dist.hpp): one wavefront per row
__global__ __launch_bounds__(256) void masked_local_kernel(DistArgs a, const unsigned char *__restrict__ vp, int vld, int one,
                                                           int B, u64 width, u64 height, u64 *__restrict__ lastbmu,
                                                           float *__restrict__ sqres)
{
    const int s = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (s >= B)
        return;   // wave-uniform
    const float *x = a.xa + (size_t)s * a.ldx;
    const unsigned char *v = vp + (one ? 0 : (size_t)s * vld);
    u64 minIndex;
    float minDist;
    vsom_local_walk_with([&](u64 node, int k) { return masked_group_dist(x, v, a.ma + (size_t)node * a.ldm, a.L, k); },
                         width, height, lastbmu[s], lane, minIndex, minDist);
    if (lane == 0) {
        lastbmu[s] = minIndex;
        sqres[s] = minDist;
    }
}

template <bool MEDIAN>
__global__ __launch_bounds__(256) void masked_chain_kernel(const float *__restrict__ Xs, int ldx, const int2 *__restrict__ bxy,
                                                           int B, const unsigned *__restrict__ bits, int nwords,
                                                           const int *__restrict__ dcols,
                                                           const unsigned *__restrict__ ndirty,
                                                           const float *__restrict__ lut, int lutw, int luth, int W, int H,
                                                           int N, float *__restrict__ map, float *__restrict__ sigma,
                                                           int pitch)
{
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int first = ((int)blockIdx.y * 4 + wv) * CH_CB;     // position of the wavefront's first column in the dirty list
    const int nd = (int)*ndirty;
    if (first >= nd)
        return;                                                // (wavefront-uniform; the kernel has no barrier)
    const int lane = threadIdx.x & 63;
    const int node = (int)blockIdx.x * 64 + lane;
    int cx, cy;
    vsom_somindex((u64)(node < N ? node : 0), (u64)W, (u64)H, cx, cy);     // SomIndex(*this, index) (Som.cpp:816)

    int col[CH_CB];                                            // (uniform) -1: no column
#pragma unroll
    for (int c = 0; c < CH_CB; ++c)
        col[c] = first + c < nd ? dcols[first + c] : -1;
    float M[CH_CB], S[CH_CB], Wd[CH_CB];
#pragma unroll
    for (int c = 0; c < CH_CB; ++c)
        M[c] = S[c] = Wd[c] = 0.f;                             // :840, :843-844

    vsom_masked_walk<MEDIAN, false, CH_CB, CH_U>(Xs, ldx, bxy, B, bits, nwords, lut, lutw, luth, cx, cy, col, M, S, Wd);
    if (node < N) {
#pragma unroll
        for (int c = 0; c < CH_CB; ++c)
            if (col[c] >= 0) {
                map[(size_t)node * pitch + col[c]] = M[c];                      // :870
                sigma[(size_t)node * pitch + col[c]] = sqrtf(S[c] / Wd[c]);     // :873
            }
    }
}

void vsom_bxy_enqueue(vsom_ctx *c, int2 *bxy)
{
    hipLaunchKernelGGL(vsom_bxy_kernel, dim3((unsigned)((c->B + 255) / 256)), dim3(256), 0, c->stream, c->lastbmu.p, (int)c->B,
                       (u64)c->W, (u64)c->H, bxy);
}

VsomMaskedScratch vsom_masked_scratch_add(const vsom_ctx *c, vsom_layout &lay, bool one, bool first)
{
    const size_t B = c->B, J = c->J;
    VsomMaskedScratch ms;
    ms.one = one;
    ms.first = first;
    ms.vrows = one ? 1 : B;
    ms.nwords = (B + 31) / 32;
    ms.slice = std::min(vsom_masked_search_slice_rows(c), B);
    ms.grp = vsom_masked_groups(c, ms.slice);
    ms.raw = lay.add<unsigned char>(ms.vrows * J);
    ms.packed = lay.add<unsigned char>(ms.vrows * c->xpitch);
    ms.bits = lay.add<unsigned>(J * ms.nwords);
    ms.dcols = lay.add<int>(J);
    ms.ndirty = lay.add<unsigned>(1);
    // (the valid-column counts of the search's reduction are not used)
    ms.part = lay.add<u64>(first ? ms.slice * ms.grp.ng : 0);
    ms.nan0 = lay.add<unsigned char>(first ? ms.slice : 0);
    ms.nvalid = lay.add<unsigned>(first ? ms.slice : 0);
    return ms;
}

void vsom_masked_prepare_enqueue(vsom_ctx *c, const vsom_layout &lay, const VsomMaskedScratch &ms)
{
    const size_t B = c->B, J = c->J;
    vsom_masked_pack_enqueue(c, lay.at(ms.raw), ms.vrows, lay.at(ms.packed));
    hipLaunchKernelGGL(masked_bits_kernel, dim3((unsigned)ms.nwords, (unsigned)((J + 255) / 256)), dim3(256), 0, c->stream,
                       lay.at(ms.packed), (int)c->xpitch, (int)ms.one, (int)J, (int)B, (int)ms.nwords, lay.at(ms.bits));
    hipLaunchKernelGGL(masked_dirty_kernel, dim3(1), dim3(256), 0, c->stream, lay.at(ms.bits), (int)J, (int)B, (int)ms.nwords,
                       lay.at(ms.dcols), lay.at(ms.ndirty));
}

int vsom_masked_phase1_enqueue(vsom_ctx *c, const vsom_layout &lay, const VsomMaskedScratch &ms)
{
    const size_t B = c->B, vld = c->xpitch;
    const unsigned char *packed = lay.at(ms.packed);
    if (ms.first) {
        for (size_t s0 = 0; s0 < B; s0 += ms.slice) {
            const size_t s1 = std::min(B, s0 + ms.slice);
            if (int rc = vsom_masked_search_enqueue(c, 0, s0, s1, packed + (ms.one ? 0 : s0 * vld), ms.one, ms.grp,
                                                    lay.at(ms.part), lay.at(ms.nan0), c->lastbmu.p + s0, c->sqres.p + s0,
                                                    lay.at(ms.nvalid)))
                return rc;
        }
    } else {
        hipLaunchKernelGGL(masked_local_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, c->stream, vsom_dist_args(c),
                           packed, (int)vld, (int)ms.one, (int)B, (u64)c->W, (u64)c->H, c->lastbmu.p, c->sqres.p);
        VSOM_HIP_CHECK(hipGetLastError());
    }
    return VSOM_OK;
}

int launch_batch_epoch_masked(vsom_ctx *c, double sigma, int is_first, const uint8_t *valid_host, int one_mask)
{
    const size_t B = c->B, N = c->N, J = c->J;
    int rc;
    if (B == 0) {       // the epoch of an empty chunk reads no validity
        if ((rc = launch_finish(c)) || (rc = launch_phase2(c, sigma, 0, N)))
            return rc;
        VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
        return VSOM_OK;
    }
    vsom_layout lay;
    const VsomMaskedScratch ms = vsom_masked_scratch_add(c, lay, one_mask != 0, is_first != 0);
    const auto bxy = lay.add<int2>(B);      // BMU coordinates
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));

    {
        TimerScope ts(c, VSOM_T_STAGE);
        VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(ms.raw), valid_host, ms.vrows * J, hipMemcpyHostToDevice, c->stream));
        vsom_masked_prepare_enqueue(c, lay, ms);
        VSOM_HIP_CHECK(hipGetLastError());
    }
    {   // phase 1 (:762-806) on the masked distance, results where phase 1 stores them
        TimerScope ts(c, VSOM_T_BMU);
        if ((rc = vsom_masked_phase1_enqueue(c, lay, ms)))
            return rc;
    }
    if ((rc = launch_finish(c)))
        return rc;
    // phase 2 (:809-876) as it is: weightMap and every clean column; it builds the neighbourhood table of this sigma
    if ((rc = launch_phase2(c, sigma, 0, N)))
        return rc;
    c->rows_free_valid = false;     // the chains below read the staged rows
    {
        TimerScope ts(c, VSOM_T_UPDATE);
        vsom_bxy_enqueue(c, lay.at(bxy));
        const auto k = c->transform == VSOM_MEDIAN ? masked_chain_kernel<true> : masked_chain_kernel<false>;
        hipLaunchKernelGGL(k, dim3((unsigned)((N + 63) / 64), (unsigned)(((J + CH_CB - 1) / CH_CB + 3) / 4)), dim3(256), 0,
                           c->stream, c->Xs.p, (int)c->xpitch, lay.at(bxy), (int)B, lay.at(ms.bits), (int)ms.nwords,
                           lay.at(ms.dcols), lay.at(ms.ndirty), c->lut.p, (int)c->lut_w, (int)c->lut_h, (int)c->W, (int)c->H,
                           (int)N, c->map.p, c->sigma.p, (int)c->pitch);
        VSOM_HIP_CHECK(hipGetLastError());
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}
