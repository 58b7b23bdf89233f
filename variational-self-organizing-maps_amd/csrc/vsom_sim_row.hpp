// vsom_sim_row.hpp -- the row body of Som::measureSimilarity's per-record report (Som.cpp:631-714), shared by the kernels
// that score a row against its unit with one wavefront: similarity_kernel (vsom_similarity.hip) and the epilogue of
// ensemble_masked_many_kernel (vsom_ensemble.hip).  One spelling of the column arithmetic and of the wave reductions, so
// the two give the same bits: a lane feeds its columns to sim_column in ascending order, whichever columns it owns, and
// the statements of vsom_sim_reduce.inc take the row's results over the 64 lanes.  (The reduction is a body included as
// text, not a function: as an inlined function it changed similarity_kernel's instruction schedule, and that kernel is
// kept byte for byte.)
#pragma once
#include "vsom_device.hpp"

#define SIM_NONE 0xFFFFFFFFu

struct SimArgs {
    const float *x;             // staged rows (Xs), pitch ldx
    const float *map, *sigma;   // model rows, pitch ldm
    const u64 *lastbmu;         // per chunk row; MASKED: the slice's search results, entry r - s0 for row r
    const float *sqres;
    const unsigned *nvalid;     // MASKED only: the slice's counts of valid columns
    const unsigned char *valid; // rows [r0, r1) x J, or null: every column valid; MASKED: the slice's packed rows, vstride
                                // bytes apart (0: the one row every sample shares)
    float *delta;               // the slice's dense report, rows x C, or null
    unsigned *rows;             // per-row results of [r0, r1): SIM_ROW_WORDS arrays of R entries
    int ldx, ldm, part_len, part_pitch;
    int J, C, N, R, vstride;
    float k;
    int floor_rule;
};

// order-preserving image of a float that is not NaN (-0 taken as +0: the two compare equal)
__device__ __forceinline__ uint32_t sim_ord(float v)
{
    const uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ u64 sim_wave_max(u64 v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const u64 o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

struct SimLane {
    float dmax_v, first_v, amax_v;
    uint32_t dmax_c, first_c, amax_c, outside;
};

// a lane that has seen no column
__device__ __forceinline__ void sim_lane_init(SimLane &l)
{
    l.dmax_v = -__builtin_inff();
    l.first_v = __uint_as_float(0x7FC00000u);
    l.amax_v = 0.f;
    l.dmax_c = l.first_c = l.amax_c = SIM_NONE;
    l.outside = 0;
}

// column d of the row into the lane's candidates (of `a` only k and floor_rule are read); returns the dense report's entry
template <bool MASKED>
__device__ __forceinline__ float sim_column(SimLane &l, const SimArgs &a, uint32_t d, float x, float m, float s, bool valid)
{
    const float eps = 0.00001f;
    const float sM = a.floor_rule ? (s > eps ? s : eps) : (s > eps ? eps : s);
    const float t = x - m;
    const float q = t / sM;
    float delta = q / a.k;
    if constexpr (MASKED)
        delta = valid ? delta : __uint_as_float(0x7FC00000u);
    const float sk = sM * a.k;
    const float lo = m - sk, hi = m + sk;
    if (delta == delta && (l.dmax_c == SIM_NONE || delta > l.dmax_v)) {
        l.dmax_v = delta;
        l.dmax_c = d;
    }
    if (l.first_c == SIM_NONE && delta > -99999999.f) {
        l.first_v = delta;
        l.first_c = d;
    }
    const float ad = fabsf(delta);
    const bool finite = ad < __builtin_inff();     // (false for NaN)
    if (valid && finite && (l.amax_c == SIM_NONE || ad > l.amax_v)) {
        l.amax_v = ad;
        l.amax_c = d;
    }
    if (valid && (x < lo || x > hi))
        ++l.outside;
    return finite ? delta : 0.f;
}
