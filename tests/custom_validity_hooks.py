"""Device source of custom Transformation hooks that USE their value_weight argument (include/vsom_hip.h, "value_weight"):
the chunk's validity and the column weights reach the result through it alone.  Every branch on value_weight is a select,
so a NaN at an invalid position of x reaches nothing."""

# Comparer = vw .* (model - x) over the valid entries, Stepper = x - model over the valid entries
SELECT = r"""
__device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
                              const float *value_weight, uint32_t J, uint32_t D)
{
    return value_weight[r] != 0.f ? value_weight[r] * (model[r] - x[r]) : 0.f;
}
__device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
                           uint32_t J, uint32_t D)
{
    return value_weight[d] != 0.f ? x[d] - model[d] : 0.f;
}
"""

# SELECT with the residual also divided by the dispersion (the distance passes the floored sigmaMap: the 1e-5 floor)
SCALED = r"""
__device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
                              const float *value_weight, uint32_t J, uint32_t D)
{
    return value_weight[r] != 0.f ? (value_weight[r] * (model[r] - x[r])) / dispersion[r] : 0.f;
}
__device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
                           uint32_t J, uint32_t D)
{
    return value_weight[d] != 0.f ? x[d] - model[d] : 0.f;
}
"""

# SELECT without the factor value_weight[r]: select(valid, model - x, +0), what the masked family computes
PLAIN_SELECT = r"""
__device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
                              const float *value_weight, uint32_t J, uint32_t D)
{
    return value_weight[r] != 0.f ? model[r] - x[r] : 0.f;
}
__device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
                           uint32_t J, uint32_t D)
{
    return value_weight[d] != 0.f ? x[d] - model[d] : 0.f;
}
"""

SOURCES = {"select": SELECT, "scaled": SCALED, "plain_select": PLAIN_SELECT}
