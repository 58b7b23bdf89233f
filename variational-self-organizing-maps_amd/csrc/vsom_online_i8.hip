// vsom_online_i8.hip -- image-bounded search of the online chunk loop (sigma > 1, Standard / Median, rows of at most 1024
// values).  One of the three chunk loops vsom_train_online_chunk* picks from (vsom_online.hip, the index
// of the family): kernels, host side (onl_i8_applies, enqueue_chunk_i8) and vsom_get_online_search_stats.
//
// The exact scan streams the fp32 map once per SAMPLE (4 N D bytes: 51 MB at 128 x 128 x 784).  Here the search reads a
// one-digit image of it instead -- one byte per model value, u = q + 128 with M_nk = s_n q_nk + r_nk, s_n a power of two,
// q in [-127, 127], plus four scalars per node -- and only PRUNES with it: every index and distance still comes from an
// exact-order evaluation (onl_refine_kernel: vsom_group_dist's arithmetic on the fp32 rows of the nodes that survive),
// so results are bit-identical to the exact scan's.  Two launches per sample, as before, but differently cut:
//
//   onl_fused_kernel    window update of sample j  ||  image scan for sample j + 1.  The window workgroups rewrite their
//                       node's fp32 rows exactly as online_window_kernel does, then re-digit the row they hold in
//                       registers and score it against sample j + 1; the scan workgroups score the nodes OUTSIDE the window
//                       from the image (8 lanes per node, 16 bytes per load, every load of a lane in flight at once).  A
//                       score is an interval [L_n, U_n] that provably contains the exact-order fp32 distance e_n (minus
//                       the sample's |x|^2): L_n goes to onl_lb[n], min_n U_n into 64 line-sized slots.
//   onl_refine_kernel   candidates {n : L_n <= min U} (the argmin of the exact-order distances is always one of them: its
//                       L is below its own e, which is below every e_m <= U_m), evaluated in the reference's order, argmin
//                       by the same (distance, index) key and node-0-NaN flag as online_scan_kernel; its extra workgroup
//                       finishes sample j - 1 (residual / distance after the update, addBmu, MSE, lastBMU).
//
// Bound.  u = 2^-24, K = columns.  Per node (stored by the digit passes): s_n, nM_n ~ |M_n|^2, eps_n = max_k |r_nk|,
// rho_n >= |r_n|_2; per sample (onl_prep_kernel): l1 >= |x|_1, nx ~ |x|^2, sx = sum x.  With T' the fp32 value of
// <x, q_n> (scan: fma chain of x_k * float(u_nk) over <= 128 elements per lane + 3 adds, then - 128 sx; |T' - <x,q>| <=
// 35000 u l1) and A_n = fma(-2 s_n, T', nM_n):
//     |A_n - (d_n - |x|^2)| <= w_n := 2 min(l1 eps_n, |x|_2 rho_n) + s_n l1 (2 * 35000 + 256) u + 25 u nM_n
//     |e_n - d_n| <= g2 d_n,  g2 = (K / 8 + 16) u        (exact-order evaluation: products + Eigen's sum tree)
//     e_n - |x|^2 in [A_n - slack_n, A_n + slack_n],  slack_n = 1.01 w_n + 1.05 g2 (max(A_n + nx, 0) + w_n) + 4 u |A_n| + 1e-30
// Anything non-finite on the way (a NaN / inf in the row or in the sample, an overflow) gives L = -inf, U = +inf: the
// node is always a candidate and never lowers the threshold -- a sample with a NaN then costs a full exact evaluation,
// spread over the refinement's workgroups.  Node 0 is always evaluated (Som.cpp:293-299: a NaN there pins the BMU).
#include "vsom_online.hpp"
#include <cmath>
#include <algorithm>
#include <cstdlib>

#ifdef VSOM_DEVELOPMENT
// phase stamps of the two kernels (100 MHz wall clock), one writer per role: tools/exp/onl_stamps.py
__device__ unsigned long long vsom_onl_stamps[32];
#define ONL_STAMP(i) (vsom_onl_stamps[i] = wall_clock64())
extern "C" int vsom_dev_onl_stamps(unsigned long long *out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(vsom_onl_stamps), sizeof(vsom_onl_stamps)) == hipSuccess ? 0 : -2;
}
// entry / exit time of every workgroup of the last fused launch that had both roles
__device__ unsigned long long vsom_onl_trace[2 * 4096];
#define ONL_TRACE(slot) do { if (f.do_scan && f.do_window && threadIdx.x == 0 && blockIdx.x < 4096) vsom_onl_trace[2 * blockIdx.x + (slot)] = wall_clock64(); } while (0)
extern "C" int vsom_dev_onl_trace(unsigned long long *out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(vsom_onl_trace), sizeof(vsom_onl_trace)) == hipSuccess ? 0 : -2;
}
#else
#define ONL_STAMP(i) ((void)0)
#define ONL_TRACE(slot) ((void)0)
#endif
constexpr int ONL_USLOTS = 32;                           // min U: 32 line-sized slots per parity
constexpr size_t ONL_U_BYTES = 2 * ONL_USLOTS * 128;
constexpr int ONL_KSLOTS = 2;                            // exact keys of a refinement: ~40 workgroups have one, two slots do
constexpr int ONL_REF_NODES = 32;                        // nodes per refinement workgroup (one wavefront per candidate)

struct OnlI8 {
    unsigned char *img;      // [N][ipitch] u = q + 128 (pad bytes 128)
    float4 *nsc;             // [N] {s, nM, eps, rho}; s = NaN: row holds a non-finite value
    float *lb;               // [N] L_n of the sample being searched
    unsigned *uslots;        // [2][ONL_USLOTS][32]
    const float4 *xsc;       // [B] {l1, nx, sx, -}
    int ipitch, ni;          // ni = ipitch / 128: 16-byte pieces per lane
    int nref;                // refinement workgroups = ceil(N / 32): the layout of lb
    float cT, g2c;           // (2 * 35000 + 256) u ; 1.05 (K / 8 + 16) u
    u64 *stats;              // [0] samples searched, [1] nodes evaluated exactly, [2] refinement workgroups with work
    unsigned char *dirty;    // [N] the node's sigmaMap row is owed
};

// order-preserving key of a (signed, finite) float for the unsigned atomicMin; 0xFFFFFFFF = "no finite U yet"
__device__ __forceinline__ unsigned onl_fkey(float v)
{
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float onl_funkey(unsigned k)
{
    if (k == 0xFFFFFFFFu)
        return __uint_as_float(0x7F800000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// [L, U] of a node from its approximate value A and the bound terms; non-finite -> (-inf, +inf)
__device__ __forceinline__ void onl_interval(float A, float s, float nM, float eps, float rho, float4 xs, float cT, float g2c,
                                             float &L, float &U)
{
    const float l1 = xs.x, nx = xs.y;
    const float x2 = sqrtf(nx * 1.0001f) * 1.0001f;
    const float w = (2.f * fminf(l1 * eps, x2 * rho) + s * l1 * cT + 1.5e-6f * nM) * 1.01f;     // 25 u = 1.49e-6
    const float dpos = fmaxf(A + nx * 1.0001f, 0.f);
    const float slack = w + g2c * (dpos + w) + 2.4e-7f * fabsf(A) + 1e-30f;
    const bool ok = slack < 3.0e38f && fabsf(A) < 3.0e38f;                                       // NaN fails both
    const float inf = __uint_as_float(0x7F800000u);
    L = ok ? A - slack : -inf;
    U = ok ? A + slack : inf;
}

// scale 2^E of a row whose largest finite magnitude is mx: |M| / s < 128 (rows below 2^-44 keep E = -50)
__device__ __forceinline__ void onl_row_scale(float mx, float &s, float &is)
{
    int e = mx > 0.f ? (int)((__float_as_uint(mx) >> 23) & 0xFF) - 127 : -100;
    e = mx > 0.f && ((__float_as_uint(mx) >> 23) & 0xFF) == 0 ? -126 : e;
    int E = e - 6;
    E = E < -50 ? -50 : E;
    s = __uint_as_float((unsigned)(E + 127) << 23);
    is = __uint_as_float((unsigned)(127 - E) << 23);
}

// digit of one value on the grid of scale s: q in [-127, 127]; r = m - q s is exact in fp32 (Sterbenz: q s and m are
// within a factor of two of each other whenever q != 0)
__device__ __forceinline__ void onl_digit(float m, float s, float is, float &q, float &r)
{
    const float mm = fabsf(m) <= 3.0e38f ? m : 0.f;
    float t = rintf(mm * is);
    t = fminf(fmaxf(t, -127.f), 127.f);
    q = t;
    r = mm - t * s;
}

// per chunk: the whole map -> image + node scalars.  One wavefront per node (rows of at most 1024 values: 16 per lane).
__global__ __launch_bounds__(256) void onl_digit_kernel(const float *__restrict__ map, int ldm, int D, int N, OnlI8 o)
{
    const int n = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N)
        return;
    const float *row = map + (size_t)n * ldm;
    float v[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = lane * 16 + 4 * j;                 // rows are zero padded to a multiple of 32 floats
        const float4 t = d < D ? *reinterpret_cast<const float4 *>(row + d) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[4 * j] = t.x;
        v[4 * j + 1] = t.y;
        v[4 * j + 2] = t.z;
        v[4 * j + 3] = t.w;
    }
    float mx = 0.f, nm = 0.f;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float a = fabsf(v[i]);
        const bool fin = a <= 3.0e38f;
        bad |= !fin;
        mx = (fin && a > mx) ? a : mx;
        nm = nm + v[i] * v[i];
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(mx, off);
        mx = om > mx ? om : mx;
        nm += __shfl_xor(nm, off);
    }
    bad = __ballot(bad) != 0ull;
    float s, is;
    onl_row_scale(mx, s, is);
    float eps = 0.f, r2 = 0.f;
    unsigned w4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned pk = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float q, r;
            onl_digit(v[4 * j + i], s, is, q, r);
            const int d = lane * 16 + 4 * j + i;
            const unsigned ub = d < D ? (unsigned)((int)q + 128) : 128u;
            pk |= ub << (8 * i);
            const float ar = fabsf(r);
            eps = ar > eps ? ar : eps;
            r2 = r2 + r * r;
        }
        w4[j] = pk;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float oe = __shfl_xor(eps, off);
        eps = oe > eps ? oe : eps;
        r2 += __shfl_xor(r2, off);
    }
    if (lane * 16 < o.ipitch)
        *reinterpret_cast<uint4 *>(o.img + (size_t)n * o.ipitch + lane * 16) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
    if (lane == 0)
        o.nsc[n] = make_float4(bad ? __uint_as_float(0x7FC00000u) : s, nm, eps, sqrtf(r2 * 1.0001f) * 1.0001f);
}

// per chunk: the bound terms of every sample.  One wavefront per sample.
__global__ __launch_bounds__(256) void onl_prep_kernel(const float *__restrict__ X, int ldx, int D, int B, float4 *__restrict__ xsc)
{
    const int s = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= B)
        return;
    const float *row = X + (size_t)s * ldx;
    float l1 = 0.f, nx = 0.f;
    double sx = 0.0;
    for (int d = lane; d < D; d += 64) {
        const float v = row[d];
        l1 += fabsf(v);
        nx += v * v;
        sx += (double)v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        l1 += __shfl_xor(l1, off);
        nx += __shfl_xor(nx, off);
        sx += __shfl_xor(sx, off);
    }
    if (lane == 0)
        xsc[s] = make_float4(l1 * 1.0001f, nx, (float)sx, 0.f);   // (a NaN / inf in the row makes l1 / nx non-finite: every interval opens)
}

// BMU of the sample of parity `par` from the refinement's key slots (whole wavefronts call this)
__device__ __forceinline__ u64 onl_resolve_i8(const u64 *state, int par)
{
    u64 key = state[(par * ONL_SLOTS + ((int)threadIdx.x & (ONL_KSLOTS - 1))) * 16];
    for (int off = ONL_KSLOTS / 2; off >= 1; off >>= 1) {
        const u64 o = __shfl_xor(key, off);
        key = o < key ? o : key;
    }
    return state[ONL_FLAG + par] ? 0ull : (key & 0xFFFFFFFFull);
}

// onl_lb is stored in the REFINEMENT's order: workgroup b of nref owns the nodes b + t nref (t < 32), and its 32 bounds sit
// side by side (one 128-byte line per workgroup instead of 32 lines 4 nref bytes apart)
__device__ __forceinline__ int onl_lb_index(int n, int nref) { return (n % nref) * ONL_REF_NODES + n / nref; }

// min U of the sample of parity `par` (whole wavefronts call this: one slot per lane)
__device__ __forceinline__ float onl_umin(const unsigned *uslots, int par)
{
    unsigned k = uslots[(par * ONL_USLOTS + ((int)threadIdx.x & (ONL_USLOTS - 1))) * 32];
    for (int off = ONL_USLOTS / 2; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)k, off);
        k = o < k ? o : k;
    }
    return onl_funkey(k);
}

struct OnlFusedArgs {
    OnlineArgs a;            // a.d.xa = row of sample j (the window's sample), a.par = parity of sample j
    const float *xnext;      // row of sample j + 1 (the one being scored)
    int jnext;               // its index into xsc
    int do_window, do_scan;
    int nwin_x, nwin_y;      // maximal window extents = window workgroups (do_window)
    int nscan, passes;       // scan workgroups (do_scan), groups of 32 nodes each of them scores
};

template <int KIND, int ST, int PASSES>   // PASSES: groups of 32 nodes per scan workgroup (compile-time: the one-group form keeps 64 VGPRs)
__global__ __launch_bounds__(256, PASSES == 1 ? 8 : 1) void onl_fused_kernel(
    OnlFusedArgs f, OnlI8 o, const double *__restrict__ lutd, int lutw, int D, int pitch, double eta, double sigma, int decay_fn,
    float *map, float *Smap, float *sigmap, float *weight)   // no __restrict__: f.a.d.ma aliases map
{
    __shared__ __attribute__((aligned(16))) float s_x[1024];
    __shared__ float s_red[4][4];
    __shared__ unsigned s_u[4];
    const OnlineArgs &a = f.a;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    ONL_TRACE(0);
    // The scan workgroups come FIRST in dispatch order: their loads are in flight from the start, and a window larger than
    // one round of resident workgroups does not keep them waiting.  (Window first, 512 scan workgroups behind 1764 window
    // workgroups at sigma = 8: the chip holds 2048, the last 228 scan workgroups started when window workgroups ended and
    // the launch took the SUM of both roles, 11.3 us under the profiler against 5.1 + 5.7 alone.)
    const int nscan = f.do_scan ? f.nscan : 0;
    const int parn = a.par ^ 1;                          // parity of the sample being scored
    const float inf = __uint_as_float(0x7F800000u);
    if ((int)blockIdx.x >= nscan) {
        const int wb = (int)blockIdx.x - nscan;
        const bool st_ = tid == 0 && wb == (f.nwin_x * f.nwin_y) / 2 + f.nwin_x / 2;
        if (st_)
            ONL_STAMP(8);
        if (tid == 0 && blockIdx.x == gridDim.x - 1 && f.do_scan)
            ONL_STAMP(21);
        const float4 xs = o.xsc[f.do_scan ? f.jnext : 0];   // (uniform address, requested before anything depends on it)
        // ---- window role: one workgroup per node of the (maximal) window of sample j
        float xn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                    // (independent of the BMU: in flight beside the resolve)
            const int d = tid + u * 256;
            xn[u] = (f.do_scan && d < D) ? f.xnext[d] : 0.f;
        }
        const u64 bmu = onl_resolve_i8(a.state, a.par);
        if (st_)
            ONL_STAMP(9);
        int bx, by;
        u64 startX, startY, endX, endY;
        online_window(bmu, a.W, a.H, sigma, bx, by, startX, startY, endX, endY);
        const u64 i = startX + (u64)(wb % f.nwin_x), j = startY + (u64)(wb / f.nwin_x);
        if (i >= endX || j >= endY) {
            ONL_TRACE(1);
            return;
        }
        const size_t n = (size_t)(j * (u64)a.W + i);
        int dx = (int)i - bx, dy = (int)j - by;
        dx = dx < 0 ? -dx : dx;
        dy = dy < 0 ? -dy : dy;
        const double h = lutd[(size_t)dy * lutw + dx];   // calculateNeighbourhoodWeight(i,j,bx,by,sigma) :915
        float mk[4] = {0.f, 0.f, 0.f, 0.f};
        online_node_update<KIND, true, ST, false>(n, h, tid, 256, a.d.xa, nullptr, nullptr, D, 0, 0, pitch, eta, decay_fn,
                                                  map, Smap, sigmap, weight, mk);
        if (tid == 0)
            o.dirty[n] = 1;                              // sigmaMap[n] = sqrt(|S / w|) is owed (onl_sigma_kernel, end of the chunk)
        if (st_)
            ONL_STAMP(10);
        if (!f.do_scan)
            return;
        // re-digit the row this workgroup holds and score it against sample j + 1
        float mx = 0.f;
        bool bad = false;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float av = fabsf(mk[u]);
            const bool fin = av <= 3.0e38f;
            bad |= !fin;
            mx = (fin && av > mx) ? av : mx;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float om = __shfl_xor(mx, off);
            mx = om > mx ? om : mx;
        }
        bad = __ballot(bad) != 0ull;
        if (lane == 0) {
            s_red[wave][0] = mx;
            s_u[wave] = bad ? 1u : 0u;
        }
        __syncthreads();
        mx = fmaxf(fmaxf(s_red[0][0], s_red[1][0]), fmaxf(s_red[2][0], s_red[3][0]));
        bad = (s_u[0] | s_u[1] | s_u[2] | s_u[3]) != 0u;
        __syncthreads();
        float s, is;
        onl_row_scale(mx, s, is);
        float dot = 0.f, nm = 0.f, r2 = 0.f, eps = 0.f;
        unsigned char *irow = o.img + n * (size_t)o.ipitch;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = tid + u * 256;
            float q, r;
            onl_digit(mk[u], s, is, q, r);
            if (d < D) {
                irow[d] = (unsigned char)((int)q + 128);
                dot = fmaf(xn[u], q, dot);
                nm = nm + mk[u] * mk[u];
                r2 = r2 + r * r;
                const float ar = fabsf(r);
                eps = ar > eps ? ar : eps;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            dot += __shfl_xor(dot, off);
            nm += __shfl_xor(nm, off);
            r2 += __shfl_xor(r2, off);
            const float oe = __shfl_xor(eps, off);
            eps = oe > eps ? oe : eps;
        }
        if (lane == 0) {
            s_red[wave][0] = dot;
            s_red[wave][1] = nm;
            s_red[wave][2] = r2;
            s_red[wave][3] = eps;
        }
        __syncthreads();
        if (st_)
            ONL_STAMP(11);
        if (tid == 0) {
            dot = (s_red[0][0] + s_red[1][0]) + (s_red[2][0] + s_red[3][0]);
            nm = (s_red[0][1] + s_red[1][1]) + (s_red[2][1] + s_red[3][1]);
            r2 = (s_red[0][2] + s_red[1][2]) + (s_red[2][2] + s_red[3][2]);
            eps = fmaxf(fmaxf(s_red[0][3], s_red[1][3]), fmaxf(s_red[2][3], s_red[3][3]));
            const float rho = sqrtf(r2 * 1.0001f) * 1.0001f;
            const float sn = bad ? __uint_as_float(0x7FC00000u) : s;
            o.nsc[n] = make_float4(sn, nm, eps, rho);
            const float A = fmaf(-2.f * sn, dot, nm);
            float L, U;
            onl_interval(A, sn, nm, eps, rho, xs, o.cT, o.g2c, L, U);
            o.lb[onl_lb_index((int)n, o.nref)] = L;
            if (U < inf)
                atomicMin(&o.uslots[(parn * ONL_USLOTS + (wb & (ONL_USLOTS - 1))) * 32], onl_fkey(U));
            if (st_)
                ONL_STAMP(12);
            if (blockIdx.x == gridDim.x - 1)
                ONL_STAMP(22);
        }
        ONL_TRACE(1);
        return;
    }
    // ---- scan role: f.passes groups of 32 nodes per workgroup, one after the other; 8 lanes per node, from the image
    const int sb = (int)blockIdx.x;
    const bool st_ = tid == 0 && sb == nscan / 2;
    if (st_)
        ONL_STAMP(16);
    if (tid == 0 && sb == 0)
        ONL_STAMP(20);
    if (sb == 0 && tid < ONL_USLOTS)                     // nobody reads or writes the other parity's slots during this launch
        o.uslots[((a.par) * ONL_USLOTS + tid) * 32] = 0xFFFFFFFFu;
    const int k = tid & 7;
    {
        const int d = tid * 4;
        const float4 t = d < D ? *reinterpret_cast<const float4 *>(f.xnext + d) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(s_x + d) = t;        // rows are zero padded to a multiple of 32 floats
    }
    const float4 xs = o.xsc[f.jnext];
    u64 startX = 0, startY = 0, endX = 0, endY = 0;       // (no window: empty)
    uint4 pc[8];
    // (nodes of the window are scored by their own workgroups: their image rows are not even loaded.  Requesting the rows
    // BEFORE the window is known -- a tenth of them read for nothing at sigma = 8, the workgroup through one round trip
    // earlier -- measured no faster: 14.68-14.73 against 14.54-14.66 us per sample.)
    if (f.do_window) {
        const u64 bmu = onl_resolve_i8(a.state, a.par);
        int bx, by;
        online_window(bmu, a.W, a.H, sigma, bx, by, startX, startY, endX, endY);
    }
    const unsigned wx0 = (unsigned)startX, wx1 = (unsigned)endX, wy0 = (unsigned)startY, wy1 = (unsigned)endY, mapw = (unsigned)a.W;
    auto in_window = [&](int nc) {                       // (32-bit: the bounds are at most the map's sides)
        const unsigned ny_ = (unsigned)nc / mapw, nx_ = (unsigned)nc - ny_ * mapw;
        return nx_ >= wx0 && nx_ < wx1 && ny_ >= wy0 && ny_ < wy1;
    };
    auto issue = [&](int n_, bool live) {
        const unsigned char *irow = o.img + (size_t)(n_ < a.N ? n_ : a.N - 1) * o.ipitch + 16 * k;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < o.ni)                                // (the last round of a row is ragged: 16-byte pieces past it are not read)
                pc[i] = (live && 128 * i + 16 * k < o.ipitch) ? *reinterpret_cast<const uint4 *>(irow + 128 * i) : make_uint4(0u, 0u, 0u, 0u);
    };
    int node = sb * 32 * PASSES + (tid >> 3);
    issue(node, node < a.N && !in_window(node));
    __syncthreads();
    if (st_)
        ONL_STAMP(17);
    unsigned ukmin = 0xFFFFFFFFu;
#pragma unroll 1
    for (int pass = 0; pass < PASSES; ++pass, node += 32) {
        const int nc = node < a.N ? node : a.N - 1;
        const float4 nsc = o.nsc[nc];
        float t0 = 0.f, t1 = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < o.ni) {
                const float4 *xp = reinterpret_cast<const float4 *>(s_x + (i * 8 + k) * 16);
                const unsigned wv[4] = {pc[i].x, pc[i].y, pc[i].z, pc[i].w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float4 xv = xp[c];
                    const unsigned w = wv[c];
                    t0 = fmaf(xv.x, (float)(w & 0xFFu), t0);
                    t1 = fmaf(xv.y, (float)((w >> 8) & 0xFFu), t1);
                    t0 = fmaf(xv.z, (float)((w >> 16) & 0xFFu), t0);
                    t1 = fmaf(xv.w, (float)(w >> 24), t1);
                }
            }
        }
        if (pass + 1 < PASSES)                           // the next group's rows travel while this one's interval is formed
            issue(node + 32, node + 32 < a.N && !in_window(node + 32));
        float T = t0 + t1;
        T += __shfl_xor(T, 1);
        T += __shfl_xor(T, 2);
        T += __shfl_xor(T, 4);
        const float Tq = fmaf(-128.f, xs.z, T);          // <x, q> = <x, u> - 128 sum x
        const float A = fmaf(-2.f * nsc.x, Tq, nsc.y);
        float L, U;
        onl_interval(A, nsc.x, nsc.y, nsc.z, nsc.w, xs, o.cT, o.g2c, L, U);
        const bool mine = node < a.N && !in_window(nc);
        if (mine && k == 0)
            o.lb[onl_lb_index(node, o.nref)] = L;
        const unsigned uk = (mine && U < inf) ? onl_fkey(U) : 0xFFFFFFFFu;
        ukmin = uk < ukmin ? uk : ukmin;
    }
    if (st_)
        ONL_STAMP(18);
    for (int off = 32; off >= 8; off >>= 1) {
        const unsigned ou = (unsigned)__shfl_xor((int)ukmin, off);
        ukmin = ou < ukmin ? ou : ukmin;
    }
    if (lane == 0)
        s_u[wave] = ukmin;
    __syncthreads();
    if (tid == 0) {
        const unsigned uk = min(min(s_u[0], s_u[1]), min(s_u[2], s_u[3]));
        if (uk != 0xFFFFFFFFu)
            atomicMin(&o.uslots[(parn * ONL_USLOTS + (sb & (ONL_USLOTS - 1))) * 32], uk);
    }
    ONL_TRACE(1);
}

// Exact-order distance of ONE (sample, node) pair by ONE wavefront.  The reference's sum runs eight sequential accumulator
// chains (Eigen's packet classes, vsom_group_dist) -- that part cannot be spread over more lanes -- but the loads and the
// squares can: the 64 lanes fetch the model row as float4 (at most four each: ONE memory round trip, coalesced), form
// p = fl(fl(m - x)^2) exactly as vsom_resid / vsom_group_dist do, and park the squares in LDS; eight lanes' worth of chains
// (every group of eight lanes runs the same ones) then only add LDS values in the reference's order.  8 lanes per
// candidate with 98 strided loads each took 7.9 us per pass through clamped 64-bit addresses and 3.2 us through a buffer
// descriptor (profiles/EXPERIMENTS.md); this form is bound by one round trip + 98 dependent additions.
//   mrow: the node's row (pitch a multiple of 32 floats, pad columns zero); x: the sample's row in LDS (1024 floats, zero
//   beyond L); sp: this wavefront's 1024-float LDS scratch.
__device__ __forceinline__ float onl_wave_dist(const float *__restrict__ mrow, const float *__restrict__ x, float *__restrict__ sp, int L,
                                               int lane)
{
    float4 mv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int d = (lane + 64 * t) * 4;
        mv[t] = d < L ? *reinterpret_cast<const float4 *>(mrow + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int d = (lane + 64 * t) * 4;
        if (d < L) {
            const float4 xv = *reinterpret_cast<const float4 *>(x + d);
            float4 r, p;
            r.x = mv[t].x - xv.x;
            r.y = mv[t].y - xv.y;
            r.z = mv[t].z - xv.z;
            r.w = mv[t].w - xv.w;
            p.x = r.x * r.x;
            p.y = r.y * r.y;
            p.z = r.z * r.z;
            p.w = r.w * r.w;
            *reinterpret_cast<float4 *>(sp + d) = p;
        }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);                  // lgkmcnt(0): this wavefront's LDS writes have landed
    __builtin_amdgcn_wave_barrier();
    const int k = lane & 7, L8 = L & ~7, ni = L8 >> 3;
    const float *pk = sp + k;
    float acc = 0.f;
#pragma unroll 14
    for (int u = 0; u < ni; ++u)
        acc = acc + pk[8 * u];
    float q = acc + __shfl_xor(acc, 4);                  // p0_k + p1_k
    const int rem = L - L8;
    if (rem >= 4)
        q = q + sp[L8 + (k & 3)];
    const float t2 = q + __shfl_xor(q, 2);
    float res = t2 + __shfl_xor(t2, 1);
    for (int tt = (rem >= 4 ? 4 : 0); tt < rem; ++tt)
        res = res + sp[L8 + tt];
    __builtin_amdgcn_wave_barrier();                     // (the next evaluation overwrites sp)
    return res;
}

// refinement of sample j (a.par, row a.d.xa) + the post step of sample j - 1 (rows a.pxa) in the last workgroup
__global__ __launch_bounds__(256) void onl_refine_kernel(OnlineArgs a, OnlI8 o, int do_refine, u64 *hits, u64 *lastbmu_out, float fB,
                                                         int add_hit)
{
    __shared__ __attribute__((aligned(16))) float s_x[1024];
    __shared__ __attribute__((aligned(16))) float s_p[4][1024];
    __shared__ int s_list[ONL_REF_NODES];
    __shared__ int s_cnt;
    __shared__ u64 skey[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (blockIdx.x == gridDim.x - 1) {
        if (a.do_post && tid < 64) {
            if (tid == 0)
                ONL_STAMP(5);
            const u64 bmu = onl_resolve_i8(a.state, a.par ^ 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {                // the row of the sample being finished (this wavefront only uses it)
                const int d = (i * 64 + tid) * 4;
                const float4 t = d < a.d.L ? *reinterpret_cast<const float4 *>(a.pxa + d) : make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4 *>(s_x + d) = t;
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            // residual / distance of the BMU after the update (:946), addBmu, MSE, lastBMU -- online_post's steps
            const float dist = onl_wave_dist(a.d.ma + (size_t)bmu * a.d.ldm, s_x, s_p[0], a.d.L, tid);
            if (tid == 0) {
                a.fstate[0] = dist;
                const float q = dist / fB;               // residual.squaredNorm() / epochSize  (:1167)
                a.fstate[1] = a.fstate[1] + q;
                if (add_hit)
                    hits[bmu] += 1ull;                   // addBmu (:1165, :1189-1192)
                *lastbmu_out = bmu;                      // lastBMU = by*W + bx (:895)
                ONL_STAMP(6);
            }
            if (tid < ONL_SLOTS)
                *online_slot(a.state, a.par ^ 1, tid) = ~0ull;    // the key set of the sample after this one
        }
        return;
    }
    if (!do_refine)
        return;
    // Workgroup b owns the nodes b + t * nref (t < 32), NOT 32 consecutive ones: the candidates of a sample are its BMU's
    // neighbours on the map -- consecutive indices -- and one wavefront evaluates one candidate at a time; with consecutive
    // ownership the BMU's own row segment put 20-30 candidates into one workgroup (5-8 rounds of 1.4 us while 500
    // workgroups sat idle: the next launch started 6 us after workgroup 0 was done).
    const int nref = (int)gridDim.x - 1;
    if (tid == 0 && blockIdx.x == 0)
        ONL_STAMP(0);
    {
        const int d = tid * 4;
        const float4 t = d < a.d.L ? *reinterpret_cast<const float4 *>(a.d.xa + d) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(s_x + d) = t;
    }
    if (wave == 0) {
        const float umin = onl_umin(o.uslots, a.par);
        bool cand = false;
        const int n = (int)blockIdx.x + lane * nref;
        if (lane < ONL_REF_NODES && n < a.N) {
            const float L = o.lb[(int)blockIdx.x * ONL_REF_NODES + lane];
            cand = !(L > umin) || n == 0;                // (node 0 seeds the reference's search, Som.cpp:293-299)
        }
        const u64 bm = __ballot(cand);
        if (cand)
            s_list[__popcll(bm & ((1ull << lane) - 1ull))] = n;
        if (lane == 0)
            s_cnt = __popcll(bm);
    }
    __syncthreads();
    const int cnt = s_cnt;
    if (cnt == 0)
        return;
    if (tid == 0) {          // diagnostics (vsom_get_online_search_stats): a few workgroups per sample get here
        atomicAdd(&o.stats[1], (u64)cnt);
        atomicAdd(&o.stats[2], 1ull);
        if (blockIdx.x == 0) {
            atomicAdd(&o.stats[0], 1ull);                // (node 0 is always a candidate of workgroup 0)
            ONL_STAMP(2);
        }
    }
    u64 best = ~0ull;
    for (int c = wave; c < cnt; c += 4) {                // one wavefront per candidate
        const int node = s_list[c];
        const float d = onl_wave_dist(a.d.ma + (size_t)node * a.d.ldm, s_x, s_p[wave], a.d.L, lane);
        const u64 key = vsom_key(d, (uint32_t)node);
        best = key < best ? key : best;
        if (node == 0 && lane == 0)
            a.state[ONL_FLAG + a.par] = (d != d) ? 1ull : 0ull;
    }
    if (tid == 0 && blockIdx.x == 0)
        ONL_STAMP(3);
    if (lane == 0)
        skey[wave] = best;
    __syncthreads();
    if (tid == 0) {
        u64 m = skey[0];
        for (int i = 1; i < 4; ++i)
            m = skey[i] < m ? skey[i] : m;
        if (m != ~0ull)
            atomicMin(online_slot(a.state, a.par, (int)(blockIdx.x % ONL_KSLOTS)), m);
        if (blockIdx.x == 0)
            ONL_STAMP(4);
    }
}

// End of a chunk: sigmaMap rows of the nodes its windows rewrote.  Som.cpp:942 writes sqrt(|S / w|) at every update of a
// node; nothing of the training reads sigmaMap, and S and weightMap change at the node's updates only, so the value after the
// node's LAST update -- computed here from the final S and weight with :939's and :942's operations -- is the same bits,
// for a fifth fewer bytes per window (5 of the 25 N_w D per sample).  Nodes no window touched keep what they had.
__global__ __launch_bounds__(256) void onl_sigma_kernel(const float *__restrict__ Smap, float *__restrict__ sigmap,
                                                        const float *__restrict__ weight, unsigned char *__restrict__ dirty, int D,
                                                        int pitch, int N)
{
    const int n = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N || !dirty[n])
        return;
    const float wnew = weight[n];
    const double tw2 = wnew == 0 ? 0.000001 : (double)wnew;   // :939
    const float twf = (float)tw2;
    const float *S = Smap + (size_t)n * pitch;
    float *sg = sigmap + (size_t)n * pitch;
    for (int d = lane; d < D; d += 64)
        sg[d] = sqrtf(fabsf(S[d] / twf));                // :942
    __builtin_amdgcn_wave_barrier();
    if (lane == 0)
        dirty[n] = 0;
}

__global__ void onl_uslots_init_kernel(unsigned *uslots)
{
    const int t = threadIdx.x;
    if (t < 2 * ONL_USLOTS)
        uslots[t * 32] = 0xFFFFFFFFu;
}

// ---- host side of the image-bounded search ------------------------------------------------------------------------
// Does the chunk loop of this context search through the image?  VSOM_BMU_EXACT: never; VSOM_BMU_SHORTLIST: whenever the
// kernels apply (Standard / Median, rows of at most 1024 values, sigma > 1); VSOM_BMU_AUTO: where it pays.  Measured on
// MI355X (tools/online_sweep.py, profiles/r6_online_sweep.jsonl; microseconds per sample, image minus exact):
//     +3.3 (the refinement launch and its boundary)  - 0.43e-6 N D (three of the scan's four bytes per value saved)
//     + 0.55e-3 k (re-digiting and scoring each of the k window nodes)
// e.g. 128 x 128 x 784: -2.2 at sigma 2, -1.0 at sigma 8, +1.3 at sigma 16, +6.6 at sigma 32; 192 x 192 x 784: -9.0 ... -1.1;
// 64 x 64 x 784 and below: 0 ... +5; rows of 256 values or fewer lose 2-5 us everywhere (the per-node costs of the refinement
// and of the slots outweigh the bytes).  AUTO takes the image where that estimate gains at least 0.3 us, for rows of at
// least 512 values and chunks long enough to repay the per-chunk passes over the map (digit pass in, sigmaMap pass out).
bool onl_i8_applies(const vsom_ctx *c, double sigma)
{
    if (c->transform == VSOM_CLR || c->part_len > 1024 || !(sigma > 1) || c->bmu_mode == VSOM_BMU_EXACT || c->B == 0)
        return false;
    if (c->bmu_mode == VSOM_BMU_SHORTLIST)
        return true;
    if (c->part_len < 512 || c->B < 64)
        return false;
    const double ext = std::floor(5.0 * sigma) + 2.0;
    const double k = std::min<double>((double)c->W, ext) * std::min<double>((double)c->H, ext);
    return 0.43e-6 * (double)c->N * (double)c->part_len - 0.55e-3 * k > 3.6;
}

static int onl_i8_ensure(vsom_ctx *c, OnlI8 *o)
{
    const uint32_t ipitch = (c->part_len + 15) / 16 * 16;    // rows of 16-byte pieces
    if (!c->onl_img.p) {
        // (onl_u: the slots + 64 bytes of stats, which start at zero)
        VSOM_ALLOC_CHECK(vsom_grow_set(c->stream, 0,
                                     {vsom_member(c->onl_img, (size_t)c->N * ipitch), vsom_member(c->onl_nsc, c->N),
                                      vsom_member(c->onl_lb, ((size_t)c->N + ONL_REF_NODES - 1) / ONL_REF_NODES * ONL_REF_NODES),
                                      vsom_member(c->onl_u, (ONL_U_BYTES + 64) / sizeof(unsigned)),
                                      vsom_member(c->onl_dirty, c->N, VSOM_BUF_ZERO)}));
        VSOM_HIP_CHECK(hipMemsetAsync((char *)c->onl_u.p + ONL_U_BYTES, 0, 64, c->stream));
    }
    if (c->onl_xsc.cap < c->B) {
        VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
        VSOM_ALLOC_CHECK(vsom_grow(c->onl_xsc, c->Bcap, c->stream));
    }
    const double u = 5.9604644775390625e-8;
    o->img = c->onl_img.p;
    o->nsc = c->onl_nsc.p;
    o->lb = c->onl_lb.p;
    o->uslots = c->onl_u.p;
    o->stats = reinterpret_cast<u64 *>((char *)c->onl_u.p + ONL_U_BYTES);
    o->xsc = c->onl_xsc.p;
    o->dirty = c->onl_dirty.p;
    o->ipitch = (int)ipitch;
    o->ni = (int)((ipitch + 127) / 128);
    o->nref = (int)((c->N + ONL_REF_NODES - 1) / ONL_REF_NODES);
    o->cT = (float)((2.0 * 35000.0 + 256.0) * u);
    o->g2c = (float)(1.05 * ((double)c->part_len / 8.0 + 16.0) * u);
    return VSOM_OK;
}

// the chunk loop through the image: per chunk a digit pass over the map and the samples' bound terms, then per sample
// onl_refine_kernel (sample j; finishes sample j - 1) and onl_fused_kernel (window of sample j || image scan for j + 1)
int enqueue_chunk_i8(vsom_ctx *c, double eta, double sigma, int decay_fn, const double *lutd, int lutw)
{
    OnlI8 o;
    if (int rc = onl_i8_ensure(c, &o))
        return rc;
    const int N = (int)c->N, D = (int)c->part_len;
    const size_t B = c->B;
    hipLaunchKernelGGL(onl_digit_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, c->stream, c->map.p, (int)c->pitch, D, N, o);
    hipLaunchKernelGGL(onl_prep_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, c->stream, c->Xs.p, (int)c->xpitch, D, (int)B,
                       c->onl_xsc.p);
    hipLaunchKernelGGL(onl_uslots_init_kernel, dim3(1), dim3(128), 0, c->stream, c->onl_u.p);
    const OnlineArgs a = vsom_onl_args(c, nullptr, nullptr, nullptr);   // (each launch below sets its sample's row and parity)
    const float fB = (float)B;
    double ext = std::floor(5.0 * sigma) + 2.0;          // maximal window extents (enqueue_single)
    const int gx = (int)std::min<double>((double)c->W, ext), gy = (int)std::min<double>((double)c->H, ext);
    // scan workgroups: the window launch of sigma = 8 on a 128 x 128 map is 1764 workgroups and the chip holds 2048 of
    // them; two groups of 32 nodes per scan workgroup keep the launch one round (256 + 1764)
    // One group of 32 nodes per scan workgroup (64 VGPRs: eight workgroups per CU; at sigma = 8 on a 128 x 128 map 512 +
    // 1764 workgroups, 2048 resident: the last window workgroups take the scan workgroups' places -- 14.75 us per sample;
    // two groups per workgroup, one round but 86 VGPRs = five per CU: 15.2) and write-through (sc1) stores of the window's
    // rows (nothing re-reads them from this XCD's L2 before the next launch, and dirty lines are written back at the
    // kernel's end: plain 16.05 us per sample, nontemporal 15.7, write-through 15.3 -- profiles/EXPERIMENTS.md).
#ifdef VSOM_DEVELOPMENT
    static const int passes_env = std::getenv("VSOM_ONL_PASSES") ? std::atoi(std::getenv("VSOM_ONL_PASSES")) : 0;
    static const int store_env = std::getenv("VSOM_ONL_STORE") ? std::atoi(std::getenv("VSOM_ONL_STORE")) : 2;
    const int passes = passes_env == 2 ? 2 : 1, store_kind = store_env;
#else
    const int passes = 1, store_kind = 2;
#endif
    const unsigned nscan = (unsigned)((N + 32 * passes - 1) / (32 * passes)),
                   nref = (unsigned)((N + ONL_REF_NODES - 1) / ONL_REF_NODES);
    const bool med = c->transform == VSOM_MEDIAN;
    auto fused = [&](const float *xs_j, int par_j, const float *xs_next, size_t jnext, bool win, bool scan) {
        OnlFusedArgs f;
        f.a = a;
        f.a.d.xa = f.a.d.xb = xs_j;
        f.a.par = par_j;
        f.xnext = xs_next;
        f.jnext = (int)jnext;
        f.do_window = win ? 1 : 0;
        f.do_scan = scan ? 1 : 0;
        f.nwin_x = gx > 0 ? gx : 1;
        f.nwin_y = gy > 0 ? gy : 1;
        f.nscan = (int)nscan;
        f.passes = passes;
        const unsigned grid = (win ? (unsigned)(f.nwin_x * f.nwin_y) : 0u) + (scan ? nscan : 0u);
#define ONL_FUSED2(KIND, ST, P)                                                                                            \
    hipLaunchKernelGGL((onl_fused_kernel<KIND, ST, P>), dim3(grid), dim3(256), 0, c->stream, f, o, lutd, lutw, D, (int)c->pitch, eta, \
                       sigma, decay_fn, c->map.p, c->S.p, c->sigma.p, c->weight.p)
#define ONL_FUSED(KIND, ST) do { if (passes == 2) ONL_FUSED2(KIND, ST, 2); else ONL_FUSED2(KIND, ST, 1); } while (0)
        if (med) {
            if (store_kind == 2) ONL_FUSED(VSOM_MEDIAN, 2); else if (store_kind == 1) ONL_FUSED(VSOM_MEDIAN, 1); else ONL_FUSED(VSOM_MEDIAN, 0);
        } else {
            if (store_kind == 2) ONL_FUSED(VSOM_STANDARD, 2); else if (store_kind == 1) ONL_FUSED(VSOM_STANDARD, 1); else ONL_FUSED(VSOM_STANDARD, 0);
        }
#undef ONL_FUSED2
#undef ONL_FUSED
    };
    auto refine = [&](const float *xs_j, int par_j, const float *xs_prev, u64 *lb_prev, bool do_refine) {
        OnlineArgs r = a;
        r.d.xa = r.d.xb = xs_j;
        r.par = par_j;
        r.pxa = r.pxb = xs_prev;
        r.do_post = xs_prev != nullptr;
        const dim3 grid((do_refine ? nref : 0u) + 1u);
        hipLaunchKernelGGL(onl_refine_kernel, grid, dim3(256), 0, c->stream, r, o, do_refine ? 1 : 0, c->hits.p, lb_prev, fB, 1);
    };
    // scores of sample 0 (no window yet): the launch works on "sample -1" of parity 1
    fused(c->Xs.p, 1, c->Xs.p, 0, false, true);
    const float *prev = nullptr;
    for (size_t j = 0; j < B; ++j) {
        const float *xs = c->Xs.p + j * c->xpitch;
        refine(xs, (int)(j & 1), prev, j ? c->lastbmu.p + (j - 1) : nullptr, true);
        const bool more = j + 1 < B;
        fused(xs, (int)(j & 1), more ? xs + c->xpitch : xs, more ? j + 1 : j, true, more);
        prev = xs;
    }
    // finish the last sample: its post step runs as the "previous sample" of a launch of the other parity
    refine(prev, (int)(B & 1), prev, c->lastbmu.p + (B - 1), false);
    hipLaunchKernelGGL(onl_sigma_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, c->stream, c->S.p, c->sigma.p, c->weight.p,
                       c->onl_dirty.p, D, (int)c->pitch, N);
    return VSOM_OK;
}

extern "C" {

int vsom_get_online_search_stats(vsom_ctx *c, uint64_t *out, int reset)
{
    CHECK_CTX_NOJOIN(c);     // (a read-back of counters: nothing to join, no reader of the staged rows)
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "null argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!c->onl_u.p)
        return VSOM_OK;
    u64 *st = reinterpret_cast<u64 *>((char *)c->onl_u.p + ONL_U_BYTES);
    VSOM_HIP_CHECK(hipMemcpyAsync(out, st, 32, hipMemcpyDeviceToHost, c->stream));
    if (reset)
        VSOM_HIP_CHECK(hipMemsetAsync(st, 0, 32, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

}   // extern "C"
