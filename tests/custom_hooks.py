"""Device source of custom Transformation hooks for the tests: the three built-ins restated through the hook contract
of include/vsom_hip.h (vsom_create_custom), and one that is not a built-in."""

# Transformation.cpp:3-39: Comparer = model - value, Stepper = value - model
STANDARD = r"""
__device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
                              const float *value_weight, uint32_t J, uint32_t D)
{
    return model[r] - x[r];
}
__device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
                           uint32_t J, uint32_t D)
{
    return x[d] - model[d];
}
"""

# Transformation.cpp:41-77: Stepper = sign(value - model), NaN passes through
MEDIAN = r"""
__device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
                              const float *value_weight, uint32_t J, uint32_t D)
{
    return model[r] - x[r];
}
__device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
                           uint32_t J, uint32_t D)
{
    const float a = x[d] - model[d];
    return (a != a) ? a : (float)((a > 0.f) - (a < 0.f));
}
"""

# Transformation.cpp:79-167: pairs i < j lexicographic, model = [A(P) | B(P)], residual A.*x_i + B - x_j,
# Stepper = [-2 r_p x_i | -2 r_p]
CLR = r"""
__device__ void clr_pair(uint32_t p, uint32_t J, uint32_t &i, uint32_t &j)
{
    i = 0;
    while (p >= J - 1 - i) {
        p -= J - 1 - i;
        ++i;
    }
    j = i + 1 + p;
}
__device__ float clr_inner(uint32_t p, const float *x, const float *model, uint32_t J, uint32_t D)
{
    uint32_t i, j;
    clr_pair(p, J, i, j);
    float t = model[p] * x[i];
    t = t + model[D / 2 + p];
    t = t - x[j];
    return t;
}
__device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
                              const float *value_weight, uint32_t J, uint32_t D)
{
    return clr_inner(r, x, model, J, D);
}
__device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
                           uint32_t J, uint32_t D)
{
    const uint32_t P = D / 2, p = d < P ? d : d - P;
    const float m2 = -2.f * clr_inner(p, x, model, J, D);
    if (d >= P)
        return m2;
    uint32_t i, j;
    clr_pair(p, J, i, j);
    return m2 * x[i];
}
"""

# not a built-in: the sigma-normalised residual (x - m) / dispersion, Stepper = x - m
SIGMA_NORMALISED = r"""
__device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
                              const float *value_weight, uint32_t J, uint32_t D)
{
    return (x[r] - model[r]) / dispersion[r];
}
__device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
                           uint32_t J, uint32_t D)
{
    return x[d] - model[d];
}
"""

SOURCES = {"standard": STANDARD, "median": MEDIAN, "clr": CLR}


def shape(kind, J):
    """(depth, residual length) of a restated built-in over samples of J values"""
    return (J * (J - 1), J * (J - 1) // 2) if kind == "clr" else (J, J)
