// vsom_eval_row.hpp -- the row body of Som::evaluate's binary error (Som.cpp:505-519), shared by the kernels that score a
// row against its unit with eight lanes: evaluate_kernel (vsom_evaluate.hip) and phase 2 of ensemble_evaluate_many_kernel
// (vsom_ensemble.hip).  One spelling of the column arithmetic (ev_zero, ev_square) and, in vsom_eval_row.inc, of the column
// rule, the column walk, the tail and the reduction in Eigen's packet order, so the two give the same bits: the same
// operations in the same order on the same logf.  (The walk is a body included as text, not a function, as
// vsom_sim_reduce.inc is: evaluate_kernel is kept byte for byte.)
#pragma once
#include "vsom_device.hpp"
#include <cmath>

#define EV_LANES 8          // lanes per row: one per element of the two Packet4f accumulators
#define EV_ROWS_PER_WG 32   // four wavefronts of eight rows
#define EV_ROW_WORDS 5      // bmu (2), dist, bsum, nrepl
#define EV_MROW_WORDS 6     // ... and nvalid (vsom_evaluate_masked_batch)
#define EV_STEPS 4          // steps whose loads are in flight together

// the factor of a column is an exact zero: t = +-0 for every finite be
__device__ __forceinline__ bool ev_zero(float fb, float val)
{
    const float inf = __builtin_inff();
    return (fb == 0.f && fabsf(val) < inf) || (val == 0.f && fabsf(fb) < inf);
}

// t * t of one column; counts a replaced term whose factor is non-zero
__device__ __forceinline__ float ev_square(float x, float m, float fb, float val, uint32_t &nrepl)
{
    const float lm = logf(m);
    const float om = 1.0f - m;
    const float l1 = logf(om);
    const float ox = 1.0f - x;
    const float a = lm * x;
    const float b = l1 * ox;
    float be = a + b;
    const bool repl = !(fabsf(be) < __builtin_inff());      // NaN or +-inf
    be = repl ? -99999.0f : be;
    const float tb = be * fb;
    const float t = tb * val;
    nrepl += (repl && fb != 0.f && val != 0.f) ? 1u : 0u;
    return t * t;
}

// Som.cpp:519, the running mean in row order
static inline double ev_running_mean(const float *dist, const float *bsum, size_t rows)
{
    double error = 0;
    for (size_t i = 0; i < rows; ++i)
        error += 1.0 / ((double)i + 1.0) * ((double)dist[i] + std::sqrt((double)bsum[i]) - error);
    return error;
}
