// vsom_masked_dist.hpp -- the masked distance of one (sample, node) pair by a group of 8 lanes, shared by the kernels that
// search sample by sample over valid columns: masked_local_kernel (vsom_masked_train.hip) and the masked online chunk
// (vsom_online_masked.hip).  The tile walks of vsom_masked.hip have their own spelling (vsom_dist_tile.hpp).
#pragma once
#include "vsom_device.hpp"

// vsom_group_dist (vsom_device.hpp) with the residual +0 at invalid columns: the same operations in the same order per
// accumulator class, the same reduction tree.  v: the row's packed validity bytes.
__device__ __forceinline__ float masked_resid(float x, unsigned char v, float m) { return v ? m - x : 0.f; }

__device__ __forceinline__ float masked_group_dist(const float *x, const unsigned char *v, const float *m, int L, int k)
{
    const int L8 = L & ~7;
    float acc = 0.f;
#pragma unroll 14
    for (int d = k; d < L8; d += 8) {
        const float r = masked_resid(x[d], v[d], m[d]);
        const float p = r * r;
        acc = acc + p;
    }
    float q = acc + __shfl_xor(acc, 4);
    const int rem = L - L8;
    if (rem >= 4) {
        const int d = L8 + (k & 3);
        const float r = masked_resid(x[d], v[d], m[d]);
        const float p = r * r;
        q = q + p;
    }
    const float t = q + __shfl_xor(q, 2);
    float res = t + __shfl_xor(t, 1);
    for (int tt = (rem >= 4 ? 4 : 0); tt < rem; ++tt) {
        const int d = L8 + tt;
        const float r = masked_resid(x[d], v[d], m[d]);
        const float p = r * r;
        res = res + p;
    }
    return res;
}
