// vsom_chain.hpp -- device helpers of the strict HIP batch chains (vsom_masked_train.hip, vsom_accum.hip,
// vsom_accum_masked.hip): the one spelling of Transformation::Stepper, of the neighbourhood-table lookup, of the masked
// step and of the masked walk over a chunk's rows, and the block compaction of a column flag.  Everything is force-inlined
// into kernels of translation units built with the strict flags (one rounding per operation, correctly rounded division).
#pragma once
#include "vsom_device.hpp"

#define CH_CB 4     // columns per wavefront of the masked chains
#define CH_U 8      // rows per group of the masked chains (operands fetched together before the dependent steps)

typedef float vsom_f2 __attribute__((ext_vector_type(2)));

// Transformation::Stepper (Transformation.cpp:11-12, 49-50); sign(): NaN -> NaN, else (a > 0) - (a < 0)
__device__ __forceinline__ float vsom_sign(float dl) { return dl != dl ? dl : (float)((dl > 0.f) - (dl < 0.f)); }

template <bool MEDIAN>
__device__ __forceinline__ float vsom_stepper(float x, float M)
{
    const float dl = x - M;
    return MEDIAN ? vsom_sign(dl) : dl;
}

// the same on a column pair (accum_chain_kernel keeps its state as pairs)
template <bool MEDIAN>
__device__ __forceinline__ vsom_f2 vsom_stepper(vsom_f2 x, vsom_f2 M)
{
    vsom_f2 dl = x - M;
    if (MEDIAN) {
        dl.x = vsom_sign(dl.x);
        dl.y = vsom_sign(dl.y);
    }
    return dl;
}

// w of node (cx, cy) for a row whose BMU is b, from the table ensure_lut built for the epoch's sigma (lutw x luth entries,
// distances past the table clamped to its last entry)
__device__ __forceinline__ float vsom_nbh_weight(const float *lut, int lutw, int luth, int cx, int cy, int2 b)
{
    int dx = cx - b.x, dy = cy - b.y;
    dx = dx < 0 ? -dx : dx;
    dy = dy < 0 ? -dy : dy;
    dx = dx < lutw ? dx : lutw - 1;
    dy = dy < luth ? dy : luth - 1;
    return lut[dy * lutw + dx];                                // (float)calculateNeighbourhoodWeight(...) :851
}

// one valid (row, column) of Som::trainBatchSomEpoch's phase 2 with the column's own weight sum
template <bool MEDIAN>
__device__ __forceinline__ void vsom_masked_step(float w, float x, float &Wd, float &M, float &S)
{
    Wd = Wd + w;                                               // :857
    const float cc = w / Wd;                                   // :864 (0/0 -> NaN, Q7)
    const float dl = vsom_stepper<MEDIAN>(x, M);               // :861
    const float t = cc * dl;
    M = M + t;                                                 // :864
    float q = w * dl;                                          // :867
    q = q * dl;
    S = S + q;
}

// The masked walk: rows [0, B) of the staged chunk in load order, in groups of U, into (M, S, Wd) of the wavefront's CB
// columns col[] (-1: no column) for the node at (cx, cy).  The group's BMU coordinates, sample values and validity words
// are wave-uniform; bits[column][row / 32] are the chunk's own words (row 0 of the chunk is bit 0).  NULLABLE: a null
// `bits` means every entry of the chunk is valid.
template <bool MEDIAN, bool NULLABLE, int CB, int U>
__device__ __forceinline__ void vsom_masked_walk(const float *Xs, int ldx, const int2 *bxy, int B,
                                                 const unsigned *bits, int nwords,
                                                 const float *lut, int lutw, int luth, int cx, int cy,
                                                 const int (&col)[CB], float (&M)[CB], float (&S)[CB], float (&Wd)[CB])
{
    static_assert(32 % U == 0, "a group of rows lies within one validity word");
    const int last = B - 1;
    for (int j0 = 0; j0 < B; j0 += U) {
        // the group's operands first: rows past the chunk are clamped re-reads of the last row, never consumed.  j0 is a
        // multiple of U, so the group stays within one word
        float w[U], x[U][CB];
        unsigned vb[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c)
            vb[c] = col[c] >= 0 ? (!NULLABLE || bits ? bits[(size_t)col[c] * nwords + (j0 >> 5)] >> (j0 & 31) : ~0u) : 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u < last ? j0 + u : last;
            w[u] = vsom_nbh_weight(lut, lutw, luth, cx, cy, bxy[j]);
#pragma unroll
            for (int c = 0; c < CB; ++c)
                x[u][c] = Xs[(size_t)j * ldx + (col[c] >= 0 ? col[c] : 0)];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (j0 + u < B && ((vb[c] >> u) & 1u))         // (uniform) a row invalid at the column is skipped
                    vsom_masked_step<MEDIAN>(w[u], x[u][c], Wd[c], M[c], S[c]);
        }
    }
}

// One round of a 256-thread ballot compaction: the threads whose flag `on` is set append their d to list[] in thread
// order behind the `base` entries of the earlier rounds; base advances by the round's count.  All 256 threads call it
// (two barriers); wcnt: the workgroup's four per-wavefront counts in LDS.
__device__ __forceinline__ void vsom_compact_round(bool on, int d, int *list, unsigned (&wcnt)[4], unsigned &base)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 m = __ballot(on);
    if (lane == 0)
        wcnt[wv] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned at = base;
    for (int i = 0; i < wv; ++i)
        at += wcnt[i];
    if (on)
        list[at + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = d;
    base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
}
