// vsom_accum.hip -- a batch epoch over a data set that loads in several chunks (gfx950; Standard / Median, strict
// arithmetic): vsom_batch_accum_begin / _chunk / _end / _abort.
//
// Phase 2 of Som::trainBatchSomEpoch (Som.cpp:809-876) is, per node, one strictly sequential walk over the rows in load
// order that carries W and, per column, M_d and S_d.  Cutting the walk at the chunk borders and carrying those values in
// accW / accM / accS changes no operation, so K chunks accumulated equal one epoch on the concatenated rows bit for bit.
// The search of every chunk runs against `map`, which keeps the epoch-start values until _end.  Per chunk:
//
//  phase 1               : launch_bmu_full / launch_bmu_local, unchanged, into lastBMU and sqres
//  accum_finish_kernel   : bmuHits[lastBMU[s]] += 1; the MSE word continues in sample order with the divisor of the whole
//                          epoch, mse = mse + sqres[s] / (float)total_rows
//  vsom_bxy_kernel       : SomIndex(lastBMU[j]) of every row, once (vsom_masked_train.hip's)
//  accum_cw_kernel       : the carried neighbourhood pass.  Thread = node: W = accW[i], then the rows in groups of AC_PU --
//                          the group's w from the table ensure_lut built (independent loads), the fp32 prefix W += w (the
//                          only dependent part), c = w / W (correctly rounded, 0/0 -> NaN; off the chain) -> cw[j][i] =
//                          (c, w), row-major over nodes so that the chains' loads are coalesced; accW[i] = W at the end
//  accum_chain_kernel    : lane = node, one wavefront per block of AC_CB columns, accM / accS of the block in 2 AC_CB
//                          registers, loaded at entry and stored at exit.  Rows in groups of AC_U: the group's sample
//                          values are wave-uniform (one 32-byte scalar load per row from the staged rows), its (c, w) one
//                          8-byte vector load per row, fetched a group ahead of the dependent steps
//                              delta = Stepper(x, M) ; M = M + c * delta ; S = S + (w * delta) * delta
//                          (one rounding per operation: this translation unit is built with the strict flags).  No atomics,
//                          no LDS, no scratch.
// and at the end of the epoch
//  accum_end_kernel      : map = accM, sigmaMap = sqrt(accS / accW), weightMap = accW; pad columns zero
// A chunk may come with validity bytes (vsom_batch_accum_chunk_masked): the columns that had an invalid entry in some chunk
// of the epoch are carried beside these accumulators by vsom_accum_masked.hip; the kernels here run
// over all columns either way.  The Stepper and the table lookup are vsom_chain.hpp's.
#include "vsom_chain.hpp"
#include <algorithm>

#define AC_CB 8     // columns per wavefront: one s_load_dwordx8 of a staged row (rows are 128-byte aligned)
#define AC_U 8      // rows per group of the chains
#define AC_PU 16    // rows per group of the neighbourhood pass

typedef vsom_f2 ac_f2;
typedef float ac_f8 __attribute__((ext_vector_type(8)));

// workgroup 0: the running MSE; workgroups 1..: bmuHits of 256 rows each (integer atomics: any order gives the same sum)
#define AC_FIN_TILE 4096
__global__ __launch_bounds__(256) void accum_finish_kernel(const float *__restrict__ sqres, int B, float ftotal,
                                                           float *__restrict__ run_dev, float *__restrict__ mse,
                                                           const u64 *__restrict__ lastbmu, u64 *__restrict__ hits)
{
    if (blockIdx.x > 0) {
        const int s = ((int)blockIdx.x - 1) * 256 + (int)threadIdx.x;
        if (s < B)
            atomicAdd(&hits[lastbmu[s]], (u64)1);
        return;
    }
    // the sum is serial by definition (fp32, sample order); the divisions are not: all threads fill a tile, thread 0 adds it
    __shared__ float q[AC_FIN_TILE];
    float run = *run_dev;
    for (int base = 0; base < B; base += AC_FIN_TILE) {
        const int n = B - base < AC_FIN_TILE ? B - base : AC_FIN_TILE;
        for (int i = (int)threadIdx.x; i < n; i += 256)
            q[i] = sqres[base + i] / ftotal;        // squaredNorm()/(float)epochSize :781, the epoch being all chunks
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < n; ++i)
                run = run + q[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *run_dev = run;
        *mse = run;                                 // the word vsom_get_mse reads (pinned host memory)
    }
}

__global__ __launch_bounds__(64) void accum_cw_kernel(const int2 *__restrict__ bxy, int B, int W, int H, int N,
                                                      const float *__restrict__ lut, int lutw, int luth,
                                                      float *__restrict__ accW, float2 *__restrict__ cw, int ldn)
{
    const int node = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (node >= N)
        return;
    int cx, cy;
    vsom_somindex((u64)node, (u64)W, (u64)H, cx, cy);          // SomIndex(*this, index) (Som.cpp:816)
    float Wr = accW[node];                                      // :840, carried over the chunk border
    const int last = B - 1;
    for (int j0 = 0; j0 < B; j0 += AC_PU) {
        float w[AC_PU], Wp[AC_PU];
#pragma unroll
        for (int u = 0; u < AC_PU; ++u)                         // rows past the chunk: clamped re-reads, never consumed
            w[u] = vsom_nbh_weight(lut, lutw, luth, cx, cy, bxy[j0 + u < last ? j0 + u : last]);
#pragma unroll
        for (int u = 0; u < AC_PU; ++u) {
            if (j0 + u < B)                                     // (uniform)
                Wr = Wr + w[u];                                 // :857
            Wp[u] = Wr;
        }
#pragma unroll
        for (int u = 0; u < AC_PU; ++u)
            if (j0 + u < B)
                cw[(size_t)(j0 + u) * ldn + node] = make_float2(w[u] / Wp[u], w[u]);   // :864 (0/0 -> NaN, Q7)
    }
    accW[node] = Wr;
}

// rows [j0, j0 + n) of one group, n = AC_U when FULL: M and S of the wavefront's AC_CB columns, as column pairs
template <bool MEDIAN, bool FULL>
__device__ __forceinline__ void accum_steps(const float2 (&q)[AC_U], const ac_f8 (&x)[AC_U], int n, ac_f2 (&M)[AC_CB / 2],
                                            ac_f2 (&S)[AC_CB / 2])
{
#pragma unroll
    for (int u = 0; u < AC_U; ++u) {
        if (FULL || u < n) {                                    // (uniform)
            const ac_f2 c2 = {q[u].x, q[u].x}, w2 = {q[u].y, q[u].y};
#pragma unroll
            for (int p = 0; p < AC_CB / 2; ++p) {
                const ac_f2 xv = {x[u][2 * p], x[u][2 * p + 1]};
                const ac_f2 dl = vsom_stepper<MEDIAN>(xv, M[p]);    // :861
                const ac_f2 t = c2 * dl;
                M[p] = M[p] + t;                                // :864
                ac_f2 v = w2 * dl;                              // :867
                v = v * dl;
                S[p] = S[p] + v;
            }
        }
    }
}

template <bool MEDIAN>
__global__ __launch_bounds__(256) void accum_chain_kernel(const float *__restrict__ Xs, int ldx, int B,
                                                          const float2 *__restrict__ cw, int ldn, int N, int J,
                                                          float *__restrict__ accM, float *__restrict__ accS, int pitch)
{
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col0 = ((int)blockIdx.y * 4 + wv) * AC_CB;       // (uniform) the wavefront's first column
    if (col0 >= J || B <= 0)
        return;                                                 // (wavefront-uniform; the kernel has no barrier)
    const int lane = threadIdx.x & 63;
    const int node = (int)blockIdx.x * 64 + lane;              // < ldn: the (c,w) rows are padded to whole wavefronts
    const bool live = node < N;
    // pitch and col0 are multiples of AC_CB: the block lies within the row; its columns >= J are pad columns, read as
    // the zeros they are and never stored
    ac_f2 M[AC_CB / 2], S[AC_CB / 2];
    {
        const size_t at = (size_t)(live ? node : 0) * pitch + col0;
        const float4 m0 = *(const float4 *)(accM + at), m1 = *(const float4 *)(accM + at + 4);
        const float4 s0 = *(const float4 *)(accS + at), s1 = *(const float4 *)(accS + at + 4);
        M[0] = ac_f2{m0.x, m0.y}, M[1] = ac_f2{m0.z, m0.w}, M[2] = ac_f2{m1.x, m1.y}, M[3] = ac_f2{m1.z, m1.w};
        S[0] = ac_f2{s0.x, s0.y}, S[1] = ac_f2{s0.z, s0.w}, S[2] = ac_f2{s1.x, s1.y}, S[3] = ac_f2{s1.z, s1.w};
    }
    static_assert(AC_CB == 8, "the entry loads and exit stores are written for 8 columns");

    const int last = B - 1;
    const float2 *cwn = cw + node;
    float2 qn[AC_U];
#pragma unroll
    for (int u = 0; u < AC_U; ++u)
        qn[u] = cwn[(size_t)(u < last ? u : last) * ldn];
    for (int j0 = 0; j0 < B; j0 += AC_U) {
        float2 q[AC_U];
        ac_f8 x[AC_U];
#pragma unroll
        for (int u = 0; u < AC_U; ++u)
            q[u] = qn[u];
        // this group's sample values (scalar) and the next group's (c,w); rows past the chunk are clamped re-reads of the
        // last row, never consumed
#pragma unroll
        for (int u = 0; u < AC_U; ++u) {
            const int j = j0 + u < last ? j0 + u : last;
            x[u] = *(const ac_f8 *)(Xs + (size_t)j * ldx + col0);
        }
#pragma unroll
        for (int u = 0; u < AC_U; ++u) {
            const int j = j0 + AC_U + u < last ? j0 + AC_U + u : last;
            qn[u] = cwn[(size_t)j * ldn];
        }
        if (j0 + AC_U <= B)
            accum_steps<MEDIAN, true>(q, x, AC_U, M, S);
        else
            accum_steps<MEDIAN, false>(q, x, B - j0, M, S);
    }
    if (live) {
        float *pm = accM + (size_t)node * pitch + col0, *ps = accS + (size_t)node * pitch + col0;
#pragma unroll
        for (int p = 0; p < AC_CB / 2; ++p) {
            if (col0 + 2 * p < J) {
                pm[2 * p] = M[p].x;
                ps[2 * p] = S[p].x;
            }
            if (col0 + 2 * p + 1 < J) {
                pm[2 * p + 1] = M[p].y;
                ps[2 * p + 1] = S[p].y;
            }
        }
    }
}

// thread = (node, column of the pitch): :870, :873, :875; the pad columns as every epoch leaves them, zero
__global__ __launch_bounds__(256) void accum_end_kernel(const float *__restrict__ accM, const float *__restrict__ accS,
                                                        const float *__restrict__ accW, int N, int J, int pitch,
                                                        float *__restrict__ map, float *__restrict__ sigma,
                                                        float *__restrict__ weight, const float *__restrict__ run_dev,
                                                        float *__restrict__ mse)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0)
        *mse = *run_dev;                            // (an epoch without rows has stored none yet)
    if (i >= (size_t)N * pitch)
        return;
    const int node = (int)(i / pitch), col = (int)(i % pitch);
    const float Wf = accW[node];
    if (col < J) {
        map[i] = accM[i];
        sigma[i] = sqrtf(accS[i] / Wf);             // an epoch without rows: sqrt(0/0) = NaN, literally
    } else {
        map[i] = 0.f;
        sigma[i] = 0.f;
    }
    if (col == 0)
        weight[node] = Wf;
}

// ---- host side: the entry points' arguments and the epoch's state are checked in vsom_capi.hip -------------------------

int launch_accum_begin(vsom_ctx *c)
{
    const size_t nd = (size_t)c->N * c->pitch;
    VSOM_ALLOC_CHECK(vsom_grow_set(c->stream, VSOM_BUF_SYNC,
                                   {vsom_member(c->acc_M, nd), vsom_member(c->acc_S, nd), vsom_member(c->acc_W, c->N),
                                    vsom_member(c->acc_mse, 1)}));
    VSOM_HIP_CHECK(hipMemsetAsync(c->acc_M.p, 0, nd * sizeof(float), c->stream));       // :843
    VSOM_HIP_CHECK(hipMemsetAsync(c->acc_S.p, 0, nd * sizeof(float), c->stream));       // :844
    VSOM_HIP_CHECK(hipMemsetAsync(c->acc_W.p, 0, (size_t)c->N * sizeof(float), c->stream));   // :840
    VSOM_HIP_CHECK(hipMemsetAsync(c->acc_mse.p, 0, sizeof(float), c->stream));
    c->ac.masked = false;
    return vsom_accum_masked_reset(c);      // no ever-dirty column (nothing to do before the first masked chunk)
}

// the loaded chunk (B > 0 rows) into the open epoch; enqueues only.  valid_host: the masked call --
// the search runs on the masked distance, and the columns that are dirty in this chunk join the ever-dirty columns, whose
// chains (vsom_accum_masked.hip) run before the carried pass below touches the accumulators.  Without a mask the launches
// are the ones listed at the top of this file, plus -- once the epoch has had a masked chunk -- the ever-dirty columns'
// chains with every entry valid (the unmasked search equals the masked one on an all-valid mask bit for bit).
int launch_accum_chunk(vsom_ctx *c, const uint8_t *valid_host, int one_mask)
{
    const size_t B = c->B, N = c->N, J = c->J, ldn = vsom_node_pitch(N);
    const bool masked = valid_host != nullptr;
    int rc;
    vsom_layout lay;
    const auto bxy = lay.add<int2>(B);
    const auto cw = lay.add<float2>(B * ldn);
    VsomMaskedScratch ms{};     // the masked call's own
    if (masked)
        ms = vsom_masked_scratch_add(c, lay, one_mask != 0, c->ac.is_first);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    if (masked) {
        if ((rc = vsom_accum_masked_ensure(c, ms.vrows * J)))
            return rc;
        {
            TimerScope ts(c, VSOM_T_STAGE);
            if ((rc = vsom_accum_masked_stage(c, valid_host, ms.vrows * J, lay.at(ms.raw))))
                return rc;
            vsom_masked_prepare_enqueue(c, lay, ms);
            c->ac.masked = true;
            if ((rc = vsom_accum_masked_fold(c, lay.at(ms.dcols), lay.at(ms.ndirty))))
                return rc;
        }
        TimerScope ts(c, VSOM_T_BMU);      // phase 1 on the masked distance, as vsom_batch_epoch_masked runs it
        if ((rc = vsom_masked_phase1_enqueue(c, lay, ms)))
            return rc;
    } else if ((rc = c->ac.is_first ? launch_bmu_full(c, 0, B) : launch_bmu_local(c, 0, B)))   // phase 1 (:762-806)
        return rc;
    if ((rc = ensure_lut(c, c->ac.sigma)))
        return rc;
    {
        TimerScope ts(c, VSOM_T_FINISH);
        hipLaunchKernelGGL(accum_finish_kernel, dim3(1u + (unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, c->sqres.p,
                           (int)B, (float)c->ac.total, c->acc_mse.p, c->mse.p, c->lastbmu.p, c->hits.p);
        VSOM_HIP_CHECK(hipGetLastError());
    }
    {
        TimerScope ts(c, VSOM_T_CW);
        vsom_bxy_enqueue(c, lay.at(bxy));
        VSOM_HIP_CHECK(hipGetLastError());
    }
    if (c->ac.masked) {     // the ever-dirty columns first: a fresh one starts from the accumulators as they stand
        TimerScope ts(c, VSOM_T_UPDATE);
        if ((rc = vsom_accum_masked_chains(c, lay.at(bxy), masked ? lay.at(ms.bits) : nullptr, (B + 31) / 32)))
            return rc;
    }
    {
        TimerScope ts(c, VSOM_T_CW);
        hipLaunchKernelGGL(accum_cw_kernel, dim3((unsigned)(ldn / 64)), dim3(64), 0, c->stream, lay.at(bxy), (int)B,
                           (int)c->W, (int)c->H, (int)N, c->lut.p, (int)c->lut_w, (int)c->lut_h, c->acc_W.p, lay.at(cw),
                           (int)ldn);
        VSOM_HIP_CHECK(hipGetLastError());
    }
    {
        TimerScope ts(c, VSOM_T_UPDATE);
        const auto k = c->transform == VSOM_MEDIAN ? accum_chain_kernel<true> : accum_chain_kernel<false>;
        hipLaunchKernelGGL(k, dim3((unsigned)(ldn / 64), (unsigned)(((J + AC_CB - 1) / AC_CB + 3) / 4)), dim3(256), 0,
                           c->stream, c->Xs.p, (int)c->xpitch, (int)B, lay.at(cw), (int)ldn, (int)N, (int)J, c->acc_M.p,
                           c->acc_S.p, (int)c->pitch);
        VSOM_HIP_CHECK(hipGetLastError());
    }
    return VSOM_OK;
}

int launch_accum_end(vsom_ctx *c)
{
    TimerScope ts(c, VSOM_T_SIGMA);
    const size_t nd = (size_t)c->N * c->pitch;
    hipLaunchKernelGGL(accum_end_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, c->stream, c->acc_M.p, c->acc_S.p,
                       c->acc_W.p, (int)c->N, (int)c->J, (int)c->pitch, c->map.p, c->sigma.p, c->weight.p, c->acc_mse.p,
                       c->mse.p);
    VSOM_HIP_CHECK(hipGetLastError());
    if (c->ac.masked)       // the ever-dirty columns from their own state
        return vsom_accum_masked_end(c);
    return VSOM_OK;
}
