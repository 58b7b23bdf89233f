// vsom_online.hpp -- what the files of the online family share (private to them): vsom_online.hip (the index of the
// family), vsom_online_i8.hip, vsom_online_tiny.hip, vsom_online_masked.hip and vsom_single.hip.
//
// The layout of onl_state and the kernel arguments built on it, the window update of one node with the helpers it is made
// of, and the host functions that cross those files.  What only one of the files uses stays in that file.  Every
// __global__ kernel and every instantiation of one lives in exactly one of them: a file that needs a kernel of another
// goes through that file's host launcher, declared at the end of this header.
#pragma once
#include "vsom_device.hpp"

// onl_state (u64): the argmin key of a sample lives in ONL_SLOTS slots, one 128-byte line each (slot s
// of parity p at [(p * ONL_SLOTS + s) * 16]); a workgroup of the scan folds its minimum into slot
// blockIdx % ONL_SLOTS and the reader takes the minimum over the slots.  With ONE slot the 512
// same-address device-scope atomics of a 128x128 scan serialise and cost 4.5 of its 13.5 us
// (tools/exp/scan_bw_bench.hip: 8.9 us without the atomic, 13.5 with one slot, 9.1-9.4 with 8-64).
// The node-0-NaN flags of the two parities sit at [ONL_FLAG], [ONL_FLAG + 1].
// onl_f: [0] dist, [1] mse sum
constexpr int ONL_SLOTS = 16;
constexpr int ONL_FLAG = 2 * ONL_SLOTS * 16;
constexpr size_t ONL_STATE_BYTES = (ONL_FLAG + 16) * sizeof(u64);
static_assert(ONL_STATE_BYTES <= VSOM_ONL_STATE_BYTES, "vsom_create allocates VSOM_ONL_STATE_BYTES");
__device__ __forceinline__ u64 *online_slot(u64 *state, int par, int s) { return state + (par * ONL_SLOTS + s) * 16; }
// BMU of the sample from its scan results; a NaN distance at node 0 pins it to 0 (Som.cpp:293-299)
// (whole wavefronts call this: the slots are read by 16 lanes and folded with shuffles)
__device__ __forceinline__ u64 online_resolve(const u64 *state, int par)
{
    u64 key = state[(par * ONL_SLOTS + ((int)threadIdx.x & (ONL_SLOTS - 1))) * 16];
#pragma unroll
    for (int off = ONL_SLOTS / 2; off >= 1; off >>= 1) {
        const u64 o = __shfl_xor(key, off);
        key = o < key ? o : key;
    }
    return state[ONL_FLAG + par] ? 0ull : (key & 0xFFFFFFFFull);
}

struct OnlineArgs {
    DistArgs d;          // xa/xb point at the sample's row(s)
    u64 *state;
    float *fstate;
    int N, W, H;
    int par;             // sample parity: which key / flag this sample uses
    // chunk loop: the search launch of sample j also finishes sample j-1 (its extra workgroup, online_scan_kernel)
    const float *pxa, *pxb;   // rows of the sample being finished
    int do_scan, do_post;
};

#ifndef VSOM_SCAN_UNR
#define VSOM_SCAN_UNR 14
#endif

__device__ __forceinline__ float onl_sign(float a)
{
    return a > 0.f ? 1.f : (a < 0.f ? -1.f : (a != a ? a : 0.f));
}

// update of ONE window node (Som.cpp:911-943) by the `nthr` threads tid = 0..nthr-1 of a group
// (a workgroup with BLOCK_SYNC, or a single wavefront running in lockstep without)
// store flavours of the window update's rows: 0 plain; 1 nontemporal; 2 write-through (sc1: the line does not stay dirty in
// the XCD's L2 until the end-of-kernel write-back)
template <int ST>
__device__ __forceinline__ void onl_store(float *p, float v)
{
    if (ST == 1)
        __builtin_nontemporal_store(v, p);
    else if (ST == 2)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}

template <int KIND, bool BLOCK_SYNC, int ST = 0, bool SIG = true>   // SIG = false: sigmaMap is written later (onl_sigma_kernel)
__device__ __forceinline__ void online_node_update(size_t n, double h, int tid, int nthr,
                                                   const float *__restrict__ xs, const float *__restrict__ xp,
                                                   const float *__restrict__ yp, int D, int P, int ppitch, int pitch,
                                                   double eta, int decay_fn, float *map, float *Smap, float *sigmap,
                                                   float *weight, float *mkeep = nullptr)   // mkeep[4]: the new M of elements tid + u * nthr
{
    float *M = map + n * pitch, *S = Smap + n * pitch, *sg = sigmap + n * pitch;
    // workgroup form, Standard / Median: this thread's first four elements are requested BEFORE the barrier below, so that
    // weightMap[n], the table entry h and the rows travel in ONE memory round trip (the barrier waits for all of them)
    constexpr bool PRE = BLOCK_SYNC && KIND != VSOM_CLR;
    float px[4], pm[4], ps[4];
    if (PRE) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = tid + u * nthr;
            const bool ok = d < D;
            px[u] = ok ? xs[d] : 0.f;
            pm[u] = ok ? M[d] : 0.f;
            ps[u] = ok ? S[d] : 0.f;
        }
    }
    const float wold = weight[n];
    float wnew, scM;
    if (decay_fn == VSOM_EXPONENTIAL) {
        wnew = wold + (float)(h * eta);              // :924
        scM = (float)(h * eta);                      // double scalar narrowed before the fp32 product :925
    } else {
        wnew = wold + (float)h;                      // :930
        double tw = wnew == 0 ? 1.0 : h / (double)wnew;   // :933
        scM = (float)tw;
    }
    const double tw2 = wnew == 0 ? 0.000001 : (double)wnew;   // :939
    const float twf = (float)tw2, hf = (float)h;
    if (BLOCK_SYNC)
        __syncthreads();   // every thread has read weight[n]
    if (tid == 0)
        weight[n] = wnew;

    if (KIND == VSOM_CLR) {
        for (int p = tid; p < P; p += nthr) {
            const float x1 = xp[p], y1 = yp[p];
            float A = M[p], Bv = M[ppitch + p];
            float inner = A * x1;
            inner = inner + Bv;
            inner = inner - y1;
            float m2 = -2.f * inner;
            float dA = m2 * x1, dB = m2;                     // Stepper :912
            float tA = scM * dA, tB = scM * dB;
            A = A + tA;                                      // :925 / :935
            Bv = Bv + tB;
            float in2 = A * x1;
            in2 = in2 + Bv;
            in2 = in2 - y1;
            float n2 = -2.f * in2;
            float dA2 = n2 * x1, dB2 = n2;                   // Stepper(v, map_new) :941
            float pa = dA * dA2, pb = dB * dB2;
            float ua = hf * pa, ub = hf * pb;
            float SA = S[p] + ua, SB = S[ppitch + p] + ub;   // :941
            M[p] = A;
            M[ppitch + p] = Bv;
            S[p] = SA;
            S[ppitch + p] = SB;
            sg[p] = sqrtf(fabsf(SA / twf));                  // :942
            sg[ppitch + p] = sqrtf(fabsf(SB / twf));
        }
    } else {
        for (int d = tid, u = 0; d < D; d += nthr, ++u) {
            const float x = PRE && u < 4 ? px[u < 4 ? u : 0] : xs[d];
            float m = PRE && u < 4 ? pm[u < 4 ? u : 0] : M[d];
            const float s_old = PRE && u < 4 ? ps[u < 4 ? u : 0] : S[d];
            float dl = x - m;                                // Stepper :912
            if (KIND == VSOM_MEDIAN)
                dl = onl_sign(dl);
            float t = scM * dl;
            m = m + t;                                       // :925 / :935
            float dl2 = x - m;                               // Stepper(v, map_new) :941
            if (KIND == VSOM_MEDIAN)
                dl2 = onl_sign(dl2);
            float pr = dl * dl2;
            float uu = hf * pr;
            float s = s_old + uu;                            // :941
            onl_store<ST>(M + d, m);
            onl_store<ST>(S + d, s);
            if (SIG)
                onl_store<ST>(sg + d, sqrtf(fabsf(s / twf)));    // :942
            if (mkeep && u < 4)
                mkeep[u < 4 ? u : 0] = m;
        }
    }
}

// window bounds of Som.cpp:899-903 (truncating, asymmetric, Q6)
__device__ __forceinline__ void online_window(u64 bmu, int W, int H, double sigma, int &bx, int &by,
                                              u64 &startX, u64 &startY, u64 &endX, u64 &endY)
{
    bx = (int)(bmu % (u64)W);
    by = (int)(bmu / (u64)W);   // bmu.getX()/getY() (:306)
    const double sxd = fmax((double)bx - 2.5 * sigma, 0.), syd = fmax((double)by - 2.5 * sigma, 0.);
    const double exd = fmin((double)bx + 2.5 * sigma, (double)W), eyd = fmin((double)by + 2.5 * sigma, (double)H);
    startX = (u64)sxd;
    startY = (u64)syd;
    endX = (u64)exd;
    endY = (u64)eyd;
}

// ---- host functions that cross the family's files ------------------------------------------------------------------
// vsom_online.hip
// The kernel arguments of ONE sample whose rows are xs / xp / yp: d, state, fstate, N, W and H from the context (CLR reads
// the pair rows xp / yp, the others xs), par = 0, pxa = pxb = nullptr, do_scan = 1, do_post = 0.  A caller sets only what
// differs; one that needs the distance operands alone takes .d.  The model half of d is vsom_dist_args' (vsom_bmu.hip),
// which describes the staged CHUNK: rows Xs / XP / YP a pitch apart.  Here it is one row and ldx = 0.
OnlineArgs vsom_onl_args(const vsom_ctx *c, const float *xs, const float *xp, const float *yp);
// online_scan_kernel<CLR of the context, postwg> on `grid` workgroups: the one place that instantiates the kernel
void launch_online_scan(vsom_ctx *c, const OnlineArgs &a, bool postwg, unsigned grid, u64 *lastbmu_out, float fB, int add_hit);
int ensure_lutd_host(vsom_ctx *c, double sigma, const double **out, int *slot_out);
// vsom_online_i8.hip: does the chunk loop of this context search through the image, and that loop
bool onl_i8_applies(const vsom_ctx *c, double sigma);
int enqueue_chunk_i8(vsom_ctx *c, double eta, double sigma, int decay_fn, const double *lutd, int lutw);
// vsom_online_tiny.hip: does the chunk take the one-launch kernel, and that launch.  valid_dev null: the plain chunk;
// otherwise the chunk over valid entries (vsom_online_masked_tiny_applies holds) and the validity bytes as given (B x J, or
// J with one)
bool online_tiny_applies(const vsom_ctx *c, double sigma);
int enqueue_chunk_tiny(vsom_ctx *c, double eta, double sigma, int decay_fn, const double *lutd, int lutw, int first_chunk,
                       u64 *lastbmu_host, const unsigned char *valid_dev, bool one);
// vsom_online_masked.hip: the exact-scan chunk loop over valid entries (Standard / Median), vp: the packed validity rows
int enqueue_chunk_masked(vsom_ctx *c, double eta, double sigma, int decay_fn, const double *lutd, int lutw,
                         const unsigned char *vp, bool one);
// vsom_single.hip
int stage_single(vsom_ctx *c, const float *v_host, bool copy = true);
