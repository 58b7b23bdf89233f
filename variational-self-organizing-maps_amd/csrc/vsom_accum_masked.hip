// vsom_accum_masked.hip -- the masked chunks of an accumulated batch epoch (gfx950; Standard / Median, strict arithmetic):
// vsom_batch_accum_chunk_masked.
//
// vsom_batch_epoch_masked recomputes, per column with an invalid entry, the chain over the rows valid at that column with
// the column's own weight sum W_d.  Over several chunks such a column is one that was dirty in ANY chunk so far ("ever
// dirty"): its M_d, S_d and W_d are carried in side buffers ([column][node]), next to the accumulators of vsom_accum.hip,
// which go on over all columns and whose values at ever-dirty columns are dead.  A column that becomes dirty in chunk k
// ("fresh") has had no row skipped so far: it starts from acc_M, acc_S and W_d = acc_W as chunks 0..k-1 left them, which
// is why the chains here run before the chunk's carried neighbourhood pass and chains.  Per masked chunk, after the
// validity bits and dirty columns of vsom_masked_train.hip:
//
//  accum_masked_fold_kernel  : one workgroup: the chunk's dirty columns into the ever-dirty flags, the fresh flags of this
//                              chunk, and the ever-dirty columns in ascending order with their count (ballot compaction; no
//                              host round trip)
//  accum_masked_chain_kernel : masked_chain_kernel's walk (vsom_masked_walk, vsom_chain.hpp) between a load and a store
//                              of the carried state.  lane = node, one wavefront per block of CH_CB ever-dirty columns;
//                              rows in load order in groups of CH_U:
//                              BMU coordinates, sample values and the validity word are wave-uniform, w comes from the
//                              neighbourhood table of the epoch's sigma.  For a valid (row, column):
//                                  W_d += w ; delta = Stepper(x, M) ; M = M + (w / W_d) * delta ; S = S + (w * delta) * delta
//                              (one rounding per operation, a correctly rounded division: strict flags); an invalid one is
//                              skipped, what x holds there is loaded and never used.  A chunk without a mask in an epoch
//                              that has ever-dirty columns runs it with every entry valid.  No atomics, no LDS; workgroups
//                              past the ever-dirty count leave at once.
// and at the end of the epoch, after accum_end_kernel,
//  accum_masked_end_kernel   : map = M_d, sigmaMap = sqrt(S_d / W_d) at the ever-dirty columns (no valid row: +0 / NaN)
#include "vsom_chain.hpp"
#include <algorithm>
#include <string.h>

__global__ __launch_bounds__(256) void accum_masked_fold_kernel(const int *__restrict__ dcols,
                                                                const unsigned *__restrict__ ndirty, int J,
                                                                unsigned char *ever, unsigned char *fresh,
                                                                int *__restrict__ ecols, unsigned *__restrict__ ecount)
{
    __shared__ unsigned wcnt[4];
    for (int d = (int)threadIdx.x; d < J; d += 256)
        fresh[d] = 0;
    __syncthreads();
    const int nd = (int)*ndirty;                   // <= J: masked_dirty_kernel's count
    for (int t = (int)threadIdx.x; t < nd; t += 256) {
        const int d = dcols[t];                    // (distinct columns: one thread per flag)
        if (!ever[d]) {
            ever[d] = 1;
            fresh[d] = 1;
        }
    }
    __syncthreads();
    unsigned base = 0;
    for (int d0 = 0; d0 < J; d0 += 256) {
        const int d = d0 + (int)threadIdx.x;
        vsom_compact_round(d < J && ever[d], d, ecols, wcnt, base);
    }
    if (threadIdx.x == 0)
        *ecount = base;
}

// sM / sS / sW: [column][ldn], ldn = N rounded up to 64.  bits null: every entry of the chunk valid (and fresh null)
template <bool MEDIAN>
__global__ __launch_bounds__(256) void accum_masked_chain_kernel(
    const float *__restrict__ Xs, int ldx, const int2 *__restrict__ bxy, int B, const unsigned *__restrict__ bits, int nwords,
    const int *__restrict__ ecols, const unsigned *__restrict__ ecount, const unsigned char *__restrict__ fresh,
    const float *__restrict__ lut, int lutw, int luth, int W, int H, int N, const float *__restrict__ accM,
    const float *__restrict__ accS, const float *__restrict__ accW, int pitch, float *__restrict__ sM, float *__restrict__ sS,
    float *__restrict__ sW, int ldn)
{
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int first = ((int)blockIdx.y * 4 + wv) * CH_CB;     // position of the wavefront's first column in the ever-dirty list
    const int ne = (int)*ecount;
    if (first >= ne || B <= 0)
        return;                                                // (wavefront-uniform; the kernel has no barrier)
    const int lane = threadIdx.x & 63;
    const int node = (int)blockIdx.x * 64 + lane;
    const bool live = node < N;
    const int ln = live ? node : 0;                            // nodes >= N: row 0, stored nowhere
    int cx, cy;
    vsom_somindex((u64)ln, (u64)W, (u64)H, cx, cy);            // SomIndex(*this, index) (Som.cpp:816)

    int col[CH_CB];                                            // (uniform) -1: no column
    float M[CH_CB], S[CH_CB], Wd[CH_CB];
#pragma unroll
    for (int c = 0; c < CH_CB; ++c) {
        col[c] = first + c < ne ? ecols[first + c] : -1;
        M[c] = S[c] = Wd[c] = 0.f;
        if (col[c] >= 0) {
            if (fresh && fresh[col[c]]) {                      // (uniform) no row skipped so far: the accumulators' state
                M[c] = accM[(size_t)ln * pitch + col[c]];
                S[c] = accS[(size_t)ln * pitch + col[c]];
                Wd[c] = accW[ln];
            } else {
                const size_t at = (size_t)col[c] * ldn + ln;
                M[c] = sM[at];
                S[c] = sS[at];
                Wd[c] = sW[at];
            }
        }
    }

    vsom_masked_walk<MEDIAN, true, CH_CB, CH_U>(Xs, ldx, bxy, B, bits, nwords, lut, lutw, luth, cx, cy, col, M, S, Wd);
    if (live) {
#pragma unroll
        for (int c = 0; c < CH_CB; ++c)
            if (col[c] >= 0) {
                const size_t at = (size_t)col[c] * ldn + node;
                sM[at] = M[c];
                sS[at] = S[c];
                sW[at] = Wd[c];
            }
    }
}

// thread = node, blockIdx.y = position in the ever-dirty list: :870, :873 with the column's own weight sum
__global__ __launch_bounds__(256) void accum_masked_end_kernel(const int *__restrict__ ecols,
                                                               const unsigned *__restrict__ ecount,
                                                               const float *__restrict__ sM, const float *__restrict__ sS,
                                                               const float *__restrict__ sW, int ldn, int N, int pitch,
                                                               float *__restrict__ map, float *__restrict__ sigma)
{
    const int node = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (node >= N)
        return;
    const unsigned ne = *ecount;
    for (unsigned pos = blockIdx.y; pos < ne; pos += gridDim.y) {
        const int d = ecols[pos];
        const size_t at = (size_t)d * ldn + node;
        map[(size_t)node * pitch + d] = sM[at];
        sigma[(size_t)node * pitch + d] = sqrtf(sS[at] / sW[at]);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

int vsom_accum_masked_ensure(vsom_ctx *c, size_t vbytes)
{
    const size_t J = c->J, ldn = vsom_node_pitch(c->N);
    const bool had = c->acm_ever.p != nullptr;
    VSOM_ALLOC_CHECK(vsom_grow_set(c->stream, VSOM_BUF_SYNC,
                                   {vsom_member(c->acm_M, J * ldn), vsom_member(c->acm_S, J * ldn), vsom_member(c->acm_W, J * ldn),
                                    vsom_member(c->acm_ever, J), vsom_member(c->acm_fresh, J), vsom_member(c->acm_cols, J),
                                    vsom_member(c->acm_meta, 1)}));
    if (!had) {     // (the shape of a context is fixed: allocated once) no ever-dirty column yet
        if (int rc = vsom_accum_masked_reset(c))
            return rc;
    }
    if (c->acm_valid.cap < 2 * vbytes) {
        // (the halves' events: the stream is synchronised before the old staging is freed)
        VSOM_ALLOC_CHECK(vsom_grow(c->acm_valid, 2 * vbytes, c->stream, VSOM_BUF_SYNC));
        c->acm_ev_valid[0] = c->acm_ev_valid[1] = false;
    }
    return VSOM_OK;
}

// no ever-dirty column (vsom_batch_accum_begin, once the buffers exist)
int vsom_accum_masked_reset(vsom_ctx *c)
{
    if (!c->acm_ever.p)
        return VSOM_OK;
    VSOM_HIP_CHECK(hipMemsetAsync(c->acm_ever.p, 0, c->J, c->stream));
    VSOM_HIP_CHECK(hipMemsetAsync(c->acm_meta.p, 0, sizeof(unsigned), c->stream));
    return VSOM_OK;
}

int vsom_accum_masked_stage(vsom_ctx *c, const uint8_t *valid_host, size_t vbytes, unsigned char *raw_dev)
{
    const int k = c->acm_slot;
    c->acm_slot ^= 1;
    if (!c->acm_ev[k])
        VSOM_HIP_CHECK(hipEventCreateWithFlags(&c->acm_ev[k], hipEventDisableTiming));
    if (c->acm_ev_valid[k])
        VSOM_HIP_CHECK(hipEventSynchronize(c->acm_ev[k]));     // the copy of two masked chunks ago
    unsigned char *host = c->acm_valid.p + (size_t)k * (c->acm_valid.cap / 2);
    memcpy(host, valid_host, vbytes);
    VSOM_HIP_CHECK(hipMemcpyAsync(raw_dev, host, vbytes, hipMemcpyHostToDevice, c->stream));
    VSOM_HIP_CHECK(hipEventRecord(c->acm_ev[k], c->stream));
    c->acm_ev_valid[k] = true;
    return VSOM_OK;
}

int vsom_accum_masked_fold(vsom_ctx *c, const int *dcols, const unsigned *ndirty)
{
    hipLaunchKernelGGL(accum_masked_fold_kernel, dim3(1), dim3(256), 0, c->stream, dcols, ndirty, (int)c->J, c->acm_ever.p,
                       c->acm_fresh.p, c->acm_cols.p, c->acm_meta.p);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}

int vsom_accum_masked_chains(vsom_ctx *c, const int2 *bxy, const unsigned *bits, size_t nwords)
{
    const size_t N = c->N, J = c->J, ldn = vsom_node_pitch(N);
    const unsigned char *fresh = bits ? c->acm_fresh.p : nullptr;
    const dim3 grid((unsigned)(ldn / 64), (unsigned)(((J + CH_CB - 1) / CH_CB + 3) / 4));
    const auto k = c->transform == VSOM_MEDIAN ? accum_masked_chain_kernel<true> : accum_masked_chain_kernel<false>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, c->stream, c->Xs.p, (int)c->xpitch, bxy, (int)c->B, bits, (int)nwords,
                       c->acm_cols.p, c->acm_meta.p, fresh, c->lut.p, (int)c->lut_w, (int)c->lut_h, (int)c->W, (int)c->H,
                       (int)N, c->acc_M.p, c->acc_S.p, c->acc_W.p, (int)c->pitch, c->acm_M.p, c->acm_S.p, c->acm_W.p,
                       (int)ldn);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}

int vsom_accum_masked_end(vsom_ctx *c)
{
    const size_t N = c->N, ldn = vsom_node_pitch(N);
    hipLaunchKernelGGL(accum_masked_end_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)std::min<size_t>(c->J, 65535)), dim3(256), 0, c->stream,
                       c->acm_cols.p, c->acm_meta.p, c->acm_M.p, c->acm_S.p, c->acm_W.p, (int)ldn, (int)N, (int)c->pitch,
                       c->map.p, c->sigma.p);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}
