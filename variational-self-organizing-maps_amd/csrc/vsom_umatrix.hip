// vsom_umatrix.hip -- Som::updateUMatrix (Som.cpp:999-1111) as one stencil launch.
//
// U[n] is the mean of euclidianWeightedDistRaw(n, map[m]) (Som.cpp:143-157) over the 3 / 5 / 8 in-grid neighbours m of
// node n, diagonals weighted 0.3.  The distance is raw_dist_kernel's with from_map = 1 (vsom_bmu.hip): per logical
// element s = sigma[n][d] < 1e-5 ? 1e-5 : sigma[n][d], a = (map[n][d] - map[m][d]) / s, the products a * a summed in
// Eigen's reduction order by 8 lanes, one per accumulator class d mod 8.  Here one 8-lane group carries ALL neighbours
// of its node -- eight accumulators per lane, the centre's value and s read once per element -- and the combination in
// double, in the reference's order of additions, happens in lane 0 of the group.  Nothing is uploaded per call.
//
// umatrix_tile_kernel: a workgroup owns a TH x TW tile of the grid.  It walks the model vectors in blocks of 64 logical
// columns: the block of the tile's (TH + 2) x (TW + 2) map rows (the tile and its halo) and of the tile's sigma rows
// (the select applied) is staged in LDS with coalesced loads, one group per node reads it from there.  The next block's
// values are fetched into registers before the current block is evaluated.  A row is read from memory once per tile
// that holds it or touches it, not once per neighbour.
// umatrix_many_kernel: one workgroup per map of an ensemble, the map's model and sigma rows in LDS whole.
#include "vsom_internal.hpp"

#include <algorithm>

namespace {

constexpr int UM_CB = 64;           // logical columns per LDS block (a multiple of 8: a reduction packet never straddles)
constexpr int UM_LS = UM_CB + 8;    // LDS row stride: the 8 groups of a wavefront sit on consecutive rows, 8 banks apart

// neighbour slots in the order the reference adds them for an interior node (Som.cpp:1017-1024):
// W, E, S(i+1), N(i-1), NW(i-1,j-1), SW(i+1,j-1), NE(i-1,j+1), SE(i+1,j+1)
__device__ __forceinline__ int um_di(int q) { return q == 2 || q == 5 || q == 7 ? 1 : (q == 3 || q == 4 || q == 6 ? -1 : 0); }
__device__ __forceinline__ int um_dj(int q) { return q == 0 || q == 4 || q == 5 ? -1 : (q == 1 || q == 6 || q == 7 ? 1 : 0); }

// physical column of logical element d: CLR rows are stored [A(P) | pad | B(P) | pad]
template <bool CLR>
__device__ __forceinline__ int um_col(int d, int P, int ppitch)
{
    return CLR ? (d < P ? d : ppitch + (d - P)) : d;
}

__device__ __forceinline__ float um_select(float s) { return s < 0.00001f ? 0.00001f : s; }   // Som.cpp:150

// the end of Eigen's reduction (raw_dist_kernel): acc = this lane's class sum over d < (D & ~7), prod(d) = a further product
template <typename Prod>
__device__ __forceinline__ float um_finish(float acc, int D, int k, Prod prod)
{
    const int D8 = D & ~7, rem = D - D8;
    float q = acc + __shfl_xor(acc, 4);
    if (rem >= 4)
        q = q + prod(D8 + (k & 3));
    float t = q + __shfl_xor(q, 2);
    float res = t + __shfl_xor(t, 1);
    for (int tt = (rem >= 4 ? 4 : 0); tt < rem; ++tt)
        res = res + prod(D8 + tt);
    return res;
}

// Som.cpp:1013-1108 (vsom_host.cpp, Som::updateUMatrix): the nine position classes, additions left to right in double
__device__ __forceinline__ double um_combine(const float (&r)[8], int i, int j, int W, int H)
{
    const double f = 0.3;
    const double w = r[0], e = r[1], s = r[2], n = r[3], nw = r[4], sw = r[5], ne = r[6], se = r[7];
    if (j > 0 && i > 0 && j < W - 1 && i < H - 1)
        return (w + e + s + n + nw * f + sw * f + ne * f + se * f) / 8;
    if (i == 0 && j > 0 && j < W - 1)
        return (w + e + s + sw * f + se * f) / 5;
    if (i == H - 1 && j > 0 && j < W - 1)
        return (w + e + n + nw * f + ne * f) / 5;
    if (j == 0 && i > 0 && i < H - 1)
        return (e + s + n + ne * f + se * f) / 5;
    if (j == W - 1 && i > 0 && i < H - 1)
        return (w + s + n + nw * f + sw * f) / 5;
    if (j == 0 && i == 0)
        return (e + s + se * f) / 3;
    if (j == W - 1 && i == 0)
        return (w + s + sw * f) / 3;
    if (j == 0 && i == H - 1)
        return (e + n + ne * f) / 3;
    if (j == W - 1 && i == H - 1)
        return (w + n + nw * f) / 3;
    return 0;
}

template <int TH, int TW, bool CLR>
__global__ __launch_bounds__(TH *TW * 8) void umatrix_tile_kernel(const float *__restrict__ map, const float *__restrict__ sigma,
                                                                  int ldm, int D, int P, int ppitch, int W, int H,
                                                                  double *__restrict__ U)
{
    constexpr int NT = TH * TW * 8, HW = TW + 2, HR = (TH + 2) * HW, CR = TH * TW;
    constexpr int RPI = NT / UM_CB;                       // rows one pass of the loaders covers
    constexpr int MI = (HR + RPI - 1) / RPI, SI = (CR + RPI - 1) / RPI;
    static_assert(NT % UM_CB == 0, "the loaders cover whole rows of a block");
    __shared__ float mt[HR * UM_LS];                      // map: the tile and its halo
    __shared__ float st[CR * UM_LS];                      // sigma of the tile, select applied
    const int tid = threadIdx.x, g = tid >> 3, k = tid & 7;
    const int i0 = blockIdx.y * TH, j0 = blockIdx.x * TW;

    // loader role: column lc of rows lr, lr + RPI, ... ; the grid node behind each row, -1 outside the grid
    const int lc = tid % UM_CB, lr = tid / UM_CB;
    int mnode[MI], snode[SI];
#pragma unroll
    for (int it = 0; it < MI; ++it) {
        const int hr = lr + it * RPI, i = i0 - 1 + hr / HW, j = j0 - 1 + hr % HW;
        mnode[it] = (hr < HR && i >= 0 && i < H && j >= 0 && j < W) ? i * W + j : -1;
    }
#pragma unroll
    for (int it = 0; it < SI; ++it) {
        const int cr = lr + it * RPI, i = i0 + cr / TW, j = j0 + cr % TW;
        snode[it] = (cr < CR && i < H && j < W) ? i * W + j : -1;
    }
    float pm[MI], ps[SI];
    auto fetch = [&](int l0) {
        const int d = l0 + lc;
        const int col = d < D ? um_col<CLR>(d, P, ppitch) : -1;
#pragma unroll
        for (int it = 0; it < MI; ++it)
            pm[it] = (mnode[it] >= 0 && col >= 0) ? map[(size_t)mnode[it] * ldm + col] : 0.f;
#pragma unroll
        for (int it = 0; it < SI; ++it)
            ps[it] = (snode[it] >= 0 && col >= 0) ? sigma[(size_t)snode[it] * ldm + col] : 0.f;
    };

    // group role: node (i, j); LDS rows of its centre and of its neighbours (the centre's where there is none)
    const int gi = g / TW, gj = g % TW, i = i0 + gi, j = j0 + gj;
    const bool valid = i < H && j < W;
    const int co = ((gi + 1) * HW + gj + 1) * UM_LS, so = g * UM_LS;
    int nbo[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int ni = i + um_di(q), nj = j + um_dj(q);
        const bool in = valid && ni >= 0 && ni < H && nj >= 0 && nj < W;
        nbo[q] = in ? ((gi + 1 + um_di(q)) * HW + gj + 1 + um_dj(q)) * UM_LS : co;
    }

    const int D8 = D & ~7, nblk = (D + UM_CB - 1) / UM_CB;
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
        acc[q] = 0.f;
    if (nblk > 0)
        fetch(0);
    for (int b = 0; b < nblk; ++b) {
        const int l0 = b * UM_CB;
        __syncthreads();                                  // the previous block has been evaluated
#pragma unroll
        for (int it = 0; it < MI; ++it)
            if (HR % RPI == 0 || lr + it * RPI < HR)
                mt[(lr + it * RPI) * UM_LS + lc] = pm[it];
#pragma unroll
        for (int it = 0; it < SI; ++it)
            if (CR % RPI == 0 || lr + it * RPI < CR)
                st[(lr + it * RPI) * UM_LS + lc] = um_select(ps[it]);
        __syncthreads();
        if (b + 1 < nblk)
            fetch(l0 + UM_CB);                            // in flight while this block is evaluated
        const int cend = D8 - l0 < UM_CB ? D8 - l0 : UM_CB;
#pragma unroll 2
        for (int c = k; c < cend; c += 8) {
            const float m = mt[co + c], s = st[so + c];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float r = m - mt[nbo[q] + c];
                const float a = r / s;
                acc[q] = acc[q] + a * a;
            }
        }
    }
    // the last block is still in LDS: it holds every element from D8 on
    const int l0 = nblk > 0 ? (nblk - 1) * UM_CB : 0;
    float res[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
        res[q] = um_finish(acc[q], D, k, [&](int d) {
            const float r = mt[co + d - l0] - mt[nbo[q] + d - l0];
            const float a = r / st[so + d - l0];
            return a * a;
        });
    if (valid && k == 0) {
        const double u = um_combine(res, i, j, W, H);
        U[(size_t)i * W + j] = u;
    }
}

// one workgroup per map: model rows and selected sigma rows in LDS by logical element, 32 nodes at a time
template <bool CLR>
__global__ __launch_bounds__(256) void umatrix_many_kernel(const VsomUmDesc *__restrict__ descs)
{
    const VsomUmDesc a = descs[blockIdx.x];
    extern __shared__ __attribute__((aligned(16))) float um_smem[];
    const int W = a.W, H = a.H, N = W * H, D = a.D;
    float *ml = um_smem, *sl = um_smem + (size_t)N * D;
    const int tid = threadIdx.x, g = tid >> 3, k = tid & 7;
    for (int e = tid; e < N * D; e += 256) {
        const int n = e / D, d = e - n * D;
        const size_t at = (size_t)n * a.ldm + um_col<CLR>(d, a.P, a.ppitch);
        ml[e] = a.map[at];
        sl[e] = um_select(a.sigma[at]);
    }
    __syncthreads();
    const int D8 = D & ~7;
    for (int base = 0; base < N; base += 32) {            // (workgroup-uniform trip count: the shuffles below need every lane)
        const bool valid = base + g < N;
        const int n = valid ? base + g : N - 1, i = n / W, j = n - i * W;
        const float *mc = ml + (size_t)n * D, *sc = sl + (size_t)n * D;
        const float *nb[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int ni = i + um_di(q), nj = j + um_dj(q);
            nb[q] = (ni >= 0 && ni < H && nj >= 0 && nj < W) ? ml + (size_t)(ni * W + nj) * D : mc;
        }
        float acc[8];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            acc[q] = 0.f;
        for (int d = k; d < D8; d += 8) {
            const float m = mc[d], s = sc[d];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float r = m - nb[q][d];
                const float t = r / s;
                acc[q] = acc[q] + t * t;
            }
        }
        float res[8];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            res[q] = um_finish(acc[q], D, k, [&](int d) {
                const float r = mc[d] - nb[q][d];
                const float t = r / sc[d];
                return t * t;
            });
        if (valid && k == 0) {
            const double u = um_combine(res, i, j, W, H);
            a.u[n] = u;
            if (a.out)
                a.out[n] = u;
        }
    }
}

template <int TH, int TW>
void um_launch_tile(vsom_ctx *c)
{
    const dim3 grid((c->W + TW - 1) / TW, (c->H + TH - 1) / TH), block(TH * TW * 8);
    if (c->transform == VSOM_CLR)
        hipLaunchKernelGGL((umatrix_tile_kernel<TH, TW, true>), grid, block, 0, c->stream, c->map.p, c->sigma.p, (int)c->pitch,
                           (int)c->D, (int)c->part_len, (int)c->part_pitch, (int)c->W, (int)c->H, c->umatrix.p);
    else
        hipLaunchKernelGGL((umatrix_tile_kernel<TH, TW, false>), grid, block, 0, c->stream, c->map.p, c->sigma.p, (int)c->pitch,
                           (int)c->D, (int)c->part_len, (int)c->part_pitch, (int)c->W, (int)c->H, c->umatrix.p);
}

}   // namespace

const char *vsom_umatrix_refusal(const vsom_ctx *c)
{
    if (c->cu)
        return "vsom_umatrix is not available on a custom-transformation context";
    if (c->W < 2 || c->H < 2)
        return "vsom_umatrix needs width >= 2 and height >= 2 (the reference indexes outside the map otherwise)";
    return nullptr;
}

int vsom_umatrix_ensure(vsom_ctx *c)
{
    // (first use only: N is fixed for the life of a context)
    VSOM_ALLOC_CHECK(vsom_grow(c->umatrix, (size_t)c->N, c->stream, VSOM_BUF_SYNC));
    return VSOM_OK;
}

// Tile shape: 4 x 8 nodes per workgroup (256 threads; tile + halo + sigma = 2.9 row reads per node).  A 2 x 8 tile (3.5 row
// reads per node, twice the workgroups) was measured beside it and was never faster, from 10 x 10 x 9 to 128 x 128 x 784
// (DESIGN.md section 4f), so there is one shape.
int launch_umatrix(vsom_ctx *c)
{
    if (int rc = vsom_umatrix_ensure(c))
        return rc;
    um_launch_tile<4, 8>(c);
    VSOM_HIP_CHECK(hipGetLastError());
    c->um_valid = true;
    return VSOM_OK;
}

size_t vsom_umatrix_many_smem(const vsom_ctx *c) { return (size_t)c->N * c->D * 2 * sizeof(float); }

int vsom_umatrix_launch_many(int clr, const VsomUmDesc *desc_dev, unsigned count, size_t smem, hipStream_t s)
{
    if (clr)
        hipLaunchKernelGGL(umatrix_many_kernel<true>, dim3(count), dim3(256), smem, s, desc_dev);
    else
        hipLaunchKernelGGL(umatrix_many_kernel<false>, dim3(count), dim3(256), smem, s, desc_dev);
    VSOM_HIP_CHECK(hipGetLastError());
    return VSOM_OK;
}
