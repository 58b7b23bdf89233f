// vsom_generate.hip -- Som::autoEncoder's records (Som.cpp:568-623) for chunk rows [r0, r1): a model vector per row drawn from
// a restricted best matching distribution, and every column sampled from a logit-approximated normal around that unit's
// map / sigmaMap values (gfx950).  vsom_decode_nodes runs the second half alone for units the caller names;
// vsom_generate_masked_batch draws K units per row from the row's distribution over its VALID columns (vsom_bmd.hip's masked
// tile, bmd_row_draws_kernel) and keeps the observed columns (generate_masked_decode_kernel, below).
//
//  the draw        : vsom_bmd.hip's kernels.  VSOM_GENERATE_PER_ROW is vsom_bmd_batch's draw of every row.
//                    VSOM_GENERATE_AS_WRITTEN computes the distribution of the chunk's LAST row once (tile + row pass on that
//                    one row, which leaves its P column, its running sums at the BMD_NC-node boundaries and its mass) and
//                    then takes one draw per uniform from it (bmd_draws_kernel: the chunk search and the re-walk of
//                    bmd_sum_kernel's draw, the same device functions, so a draw is vsom_bmd_batch's on range [B-1, B)).
//  generate_decode_kernel : one thread per (row, logical column) of a slice, rows x C flattened: thread e serves row e / C,
//                    column e % C, so a wavefront covers 64 consecutive values of L and of the record -- one or more whole
//                    rows when C <= 64 -- and its 512-byte loads and stores are contiguous whatever C is.  The row's unit b
//                    (a cached 8-byte load, shared by the lanes of a row) names the map and sigmaMap rows; consecutive
//                    columns gather consecutive floats of them.  Per value, in double, one rounding per operation, nothing
//                    contracted (csrc/build.sh compiles every file with -ffp-contract=off), in the order of Som.cpp:609:
//                      q = L / (1 - L); g = log(q); z = g / 1.6; t = z * (double)s; rec = t + (double)m
//                    A unit outside [0, N) -- UINT64_MAX, a row without mass -- stores the quiet NaN 0x7FF8000000000000 in
//                    every column and gathers nothing.  No LDS, no atomics, no cross-lane traffic.
// What bounds it: 16 bytes per value through HBM (L in, the record out) plus 8 gathered bytes that mostly hit the cache
// (the draws name few distinct units), against one double log per value; and, around the kernel, the copies of L and of the
// record between the caller's memory and the device, which dominate a call.
// log is the device math library's double-precision log (-fno-fast-math: the accurate form).  No statement of its error bound
// ships with the ROCm installation this was written against; HIP's published table of device math functions gives 1 ulp for
// the double log.  The tolerance of include/vsom_hip.h therefore takes Ld = 1 AS AN ASSUMPTION, and Lh = 1 for the host's
// libm log likewise (glibc documents 1 ulp for log on x86_64).
#include "vsom_device.hpp"
#include <algorithm>
#include <cstdlib>

#define GEN_BLOCK 256
#define GEN_PIECE ((size_t)64 << 20)     // bytes of a slice's L and of its record
#define GEN_P_BYTES ((size_t)256 << 20)  // bytes of a slice's p (PER_ROW)

struct GenArgs {
    const float *map, *sigma;   // model rows, pitch ldm
    const u64 *unit;            // one per slice row
    const double *L;            // slice rows x C
    double *rec;                // slice rows x C
    int ldm, part_len, part_pitch;
    int C, N;
    size_t count;               // slice rows x C
};

// One value of the record around (m, s), Som.cpp:609, in double with one rounding per operation
__device__ __forceinline__ double generate_value(double L, float s, float m)
{
    const double om = 1.0 - L;
    const double q = L / om;
    const double g = log(q);
    const double z = g / 1.6;
    const double t = z * (double)s;
    return t + (double)m;
}

// CLR: the model row has two parts, logical column d at (d / part_len) * part_pitch + d % part_len (as similarity_kernel<false>)
template <bool CLR>
__global__ __launch_bounds__(GEN_BLOCK) void generate_decode_kernel(GenArgs a)
{
    const size_t stride = (size_t)gridDim.x * GEN_BLOCK;
    for (size_t e = (size_t)blockIdx.x * GEN_BLOCK + threadIdx.x; e < a.count; e += stride) {
        const size_t r = e / (size_t)a.C;
        const int d = (int)(e - r * (size_t)a.C);
        const double L = a.L[e];
        const u64 b = a.unit[r];
        double rec = __longlong_as_double(0x7FF8000000000000ll);
        if (b < (u64)a.N) {
            int off = d;
            if constexpr (CLR) {
                const int part = d / a.part_len;
                off = part * a.part_pitch + (d - part * a.part_len);
            }
            const size_t at = (size_t)b * a.ldm + off;
            const float m = a.map[at], s = a.sigma[at];
            rec = generate_value(L, s, m);
        }
        a.rec[e] = rec;
    }
}

// vsom_generate_masked_batch's decode (Standard / Median): K draws per slice row, one thread per (row, draw, column),
// rows x K x C flattened as above -- thread e serves draw e / C of the slice (row e / C / K) and column e % C.  unit: one per
// (row, draw).  A column the caller observed (keep != 0 and its packed validity byte set; vp: the slice's packed rows, vld
// bytes each, one: the row every sample shares) is the staged row's value, by select: L has no say there.  The others are
// generate_decode_kernel's values.  A draw without mass stores the quiet NaN in every column.
struct GenMaskedArgs {
    GenArgs g;                  // unit: slice rows x K; L, rec: slice rows x K x C; count = slice rows x K x C
    const float *x;             // the slice's staged rows, pitch ldx
    const unsigned char *vp;
    int ldx, vld, K, one, keep;
};

__global__ __launch_bounds__(GEN_BLOCK) void generate_masked_decode_kernel(GenMaskedArgs a)
{
    const size_t stride = (size_t)gridDim.x * GEN_BLOCK;
    for (size_t e = (size_t)blockIdx.x * GEN_BLOCK + threadIdx.x; e < a.g.count; e += stride) {
        const size_t rk = e / (size_t)a.g.C;
        const int d = (int)(e - rk * (size_t)a.g.C);
        const size_t r = rk / (size_t)a.K;
        const double L = a.g.L[e];
        const u64 b = a.g.unit[rk];
        double rec = __longlong_as_double(0x7FF8000000000000ll);
        if (b < (u64)a.g.N) {
            if (a.keep && a.vp[(a.one ? 0 : r * (size_t)a.vld) + d]) {
                rec = (double)a.x[r * (size_t)a.ldx + d];
            } else {
                const size_t at = (size_t)b * a.g.ldm + d;
                rec = generate_value(L, a.g.sigma[at], a.g.map[at]);
            }
        }
        a.g.rec[e] = rec;
    }
}

// Rows per slice: a slice's L and its record (K draws per row) stay within 64 MiB each, its p (one row's distribution per
// slice row, PER_ROW only) within 256 MiB; one row where one row alone needs more.  VSOM_GENERATE_SLICE_ROWS (development,
// read at every call) forces a smaller slice so that tests cross slice boundaries on small chunks.
static size_t vsom_generate_slice_rows(size_t C, size_t N, bool per_row, size_t K = 1)
{
    size_t s = std::max<size_t>(1, GEN_PIECE / (8 * C * K));
    if (per_row)
        s = std::min(s, std::max<size_t>(1, GEN_P_BYTES / (8 * N)));
    if (const char *e = std::getenv("VSOM_GENERATE_SLICE_ROWS")) {
        const long v = std::atol(e);
        if (v > 0 && (size_t)v < s)
            s = (size_t)v;
    }
    return s;
}

// L of n rows from the caller's memory, the decode, the record into the caller's memory
static int generate_decode_slice(vsom_ctx *c, const u64 *unit_dev, size_t n, size_t C, const double *l_host, double *L_dev,
                                 double *rec_dev, double *record_out)
{
    VSOM_HIP_CHECK(hipMemcpyAsync(L_dev, l_host, n * C * 8, hipMemcpyHostToDevice, c->stream));
    GenArgs a;
    a.map = c->map.p;
    a.sigma = c->sigma.p;
    a.unit = unit_dev;
    a.L = L_dev;
    a.rec = rec_dev;
    a.ldm = (int)c->pitch;
    a.part_len = (int)c->part_len;
    a.part_pitch = (int)c->part_pitch;
    a.C = (int)C;
    a.N = (int)c->N;
    a.count = n * C;
    {
        TimerScope ts(c, VSOM_T_FINISH);
        // (at most 16 workgroups per CU: more only queue behind them, the loop strides)
        const size_t blocks = std::min<size_t>((a.count + GEN_BLOCK - 1) / GEN_BLOCK, 4096);
        if (c->nparts == 1)
            hipLaunchKernelGGL(generate_decode_kernel<false>, dim3((unsigned)blocks), dim3(GEN_BLOCK), 0, c->stream, a);
        else
            hipLaunchKernelGGL(generate_decode_kernel<true>, dim3((unsigned)blocks), dim3(GEN_BLOCK), 0, c->stream, a);
        VSOM_HIP_CHECK(hipGetLastError());
    }
    VSOM_HIP_CHECK(hipMemcpyAsync(record_out, rec_dev, n * C * 8, hipMemcpyDeviceToHost, c->stream));
    return VSOM_OK;
}

int launch_generate(vsom_ctx *c, u64 min_hits, int rule, size_t r0, size_t r1, const double *u_host, const double *l_host,
                    const vsom_generate_out *out)
{
    const size_t rows = r1 - r0;
    if (rows == 0)
        return VSOM_OK;
    const size_t N = c->N, C = std::min<size_t>(c->J, c->D);
    const bool per_row = rule == VSOM_GENERATE_PER_ROW;
    const size_t slice = std::min(vsom_generate_slice_rows(C, N, per_row), rows);
    // the distribution's scratch as launch_bmd lays it out -- for a slice (PER_ROW) or for the one row B - 1 (AS_WRITTEN) --,
    // then per slice row a uniform and a unit, and the slice's L and record
    const size_t prows = per_row ? slice : 1, ppitch = vsom_bmd_pitch(prows), nch = vsom_bmd_chunks(N);
    vsom_layout lay;
    const auto p = lay.add<double>(ppitch * N), cum = lay.add<double>(nch * ppitch), vec = lay.add<double>(2 * ppitch);
    const auto draw1 = lay.add<u64>(ppitch);
    const auto us = lay.add<double>(per_row ? 0 : slice);
    const auto units = lay.add<u64>(per_row ? 0 : slice);
    const auto Lp = lay.add<double>(out->record ? slice * C : 0), recp = lay.add<double>(out->record ? slice * C : 0);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    double *P = lay.at(p), *u_dev = lay.at(vec), *norm_dev = lay.at(vec) + ppitch;

    if (!per_row) {
        // row B - 1 once: its P column, running sums and mass (the row pass stores the running sums only with draws: it
        // takes one with the uniform 0, which nobody reads)
        TimerScope ts(c, VSOM_T_BMU);
        VSOM_HIP_CHECK(hipMemsetAsync(u_dev, 0, 8, c->stream));
        if (int rc = vsom_bmd_enqueue(c, min_hits, c->B - 1, c->B, P, ppitch, lay.at(cum), u_dev, norm_dev, lay.at(draw1)))
            return rc;
    }
    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0, off = s0 - r0;
        u64 *unit_dev;
        if (per_row) {
            unit_dev = lay.at(draw1);
            VSOM_HIP_CHECK(hipMemcpyAsync(u_dev, u_host + off, n * 8, hipMemcpyHostToDevice, c->stream));
            TimerScope ts(c, VSOM_T_BMU);
            if (int rc = vsom_bmd_enqueue(c, min_hits, s0, s1, P, ppitch, lay.at(cum), u_dev, norm_dev, unit_dev))
                return rc;
        } else {
            unit_dev = lay.at(units);
            VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(us), u_host + off, n * 8, hipMemcpyHostToDevice, c->stream));
            TimerScope ts(c, VSOM_T_BMU);
            if (int rc = vsom_bmd_enqueue_draws(c, P, ppitch, 0, lay.at(cum), norm_dev, lay.at(us), n, unit_dev))
                return rc;
        }
        if (out->unit)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->unit + off, unit_dev, n * 8, hipMemcpyDeviceToHost, c->stream));
        if (out->record)
            if (int rc = generate_decode_slice(c, unit_dev, n, C, l_host + off * C, lay.at(Lp), lay.at(recp),
                                               out->record + off * C))
                return rc;
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int launch_generate_masked(vsom_ctx *c, u64 min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask, size_t K,
                           int keep_observed, const double *u_host, const double *l_host, const vsom_generate_out *out)
{
    const size_t rows = r1 - r0;
    if (rows == 0)
        return VSOM_OK;
    const size_t N = c->N, C = c->J;
    // three budgets: p, L and the record at K draws per row, the masked search's validity scratch
    const size_t slice = std::min({vsom_generate_slice_rows(C, N, true, K), vsom_masked_search_slice_rows(c), rows});
    const size_t ppitch = vsom_bmd_pitch(slice), nch = vsom_bmd_chunks(N);
    // the distribution's scratch as launch_bmd lays it out (the row pass leaves the running sums only with draws: it takes
    // one per row with the uniform 0, which nobody reads), the validity bytes, then per (row, draw) a uniform and a unit,
    // and the slice's L and record
    vsom_layout lay;
    const auto p = lay.add<double>(ppitch * N), cum = lay.add<double>(nch * ppitch), vec = lay.add<double>(2 * ppitch);
    const auto draw1 = lay.add<u64>(ppitch);
    const VsomBmdMask mask = vsom_bmd_mask_add(c, lay, valid_host, one_mask != 0, slice);
    const auto us = lay.add<double>(slice * K);
    const auto units = lay.add<u64>(slice * K);
    const auto Lp = lay.add<double>(out->record ? slice * K * C : 0), recp = lay.add<double>(out->record ? slice * K * C : 0);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    double *P = lay.at(p), *u0_dev = lay.at(vec), *norm_dev = lay.at(vec) + ppitch;
    VSOM_HIP_CHECK(hipMemsetAsync(u0_dev, 0, ppitch * 8, c->stream));
    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0, off = s0 - r0;
        VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(us), u_host + off * K, n * K * 8, hipMemcpyHostToDevice, c->stream));
        if (int rc = vsom_bmd_mask_slice_enqueue(c, lay, mask, r0, s0, s1, valid_host))
            return rc;
        {
            TimerScope ts(c, VSOM_T_BMU);
            if (int rc = vsom_bmd_enqueue(c, min_hits, s0, s1, P, ppitch, lay.at(cum), u0_dev, norm_dev, lay.at(draw1),
                                          lay.at(mask.packed), mask.one))
                return rc;
            if (int rc = vsom_bmd_enqueue_row_draws(c, P, ppitch, n, K, lay.at(cum), norm_dev, lay.at(us), lay.at(units)))
                return rc;
        }
        if (out->unit)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->unit + off * K, lay.at(units), n * K * 8, hipMemcpyDeviceToHost, c->stream));
        if (!out->record)
            continue;
        VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(Lp), l_host + off * K * C, n * K * C * 8, hipMemcpyHostToDevice, c->stream));
        GenMaskedArgs a;
        a.g.map = c->map.p;
        a.g.sigma = c->sigma.p;
        a.g.unit = lay.at(units);
        a.g.L = lay.at(Lp);
        a.g.rec = lay.at(recp);
        a.g.ldm = (int)c->pitch;
        a.g.part_len = (int)c->part_len;
        a.g.part_pitch = (int)c->part_pitch;
        a.g.C = (int)C;
        a.g.N = (int)N;
        a.g.count = n * K * C;
        a.x = c->Xs.p + s0 * c->xpitch;
        a.vp = lay.at(mask.packed);
        a.ldx = (int)c->xpitch;
        a.vld = (int)c->xpitch;
        a.K = (int)K;
        a.one = (int)mask.one;
        a.keep = keep_observed != 0;
        {
            TimerScope ts(c, VSOM_T_FINISH);
            const size_t blocks = std::min<size_t>((a.g.count + GEN_BLOCK - 1) / GEN_BLOCK, 4096);
            hipLaunchKernelGGL(generate_masked_decode_kernel, dim3((unsigned)blocks), dim3(GEN_BLOCK), 0, c->stream, a);
            VSOM_HIP_CHECK(hipGetLastError());
        }
        VSOM_HIP_CHECK(hipMemcpyAsync(out->record + off * K * C, lay.at(recp), n * K * C * 8, hipMemcpyDeviceToHost, c->stream));
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int launch_decode_nodes(vsom_ctx *c, const uint64_t *nodes_host, size_t count, const double *l_host, double *record_out)
{
    if (count == 0)
        return VSOM_OK;
    const size_t C = std::min<size_t>(c->J, c->D);
    const size_t slice = std::min(vsom_generate_slice_rows(C, c->N, false), count);
    vsom_layout lay;
    const auto units = lay.add<u64>(slice);
    const auto Lp = lay.add<double>(slice * C), recp = lay.add<double>(slice * C);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    for (size_t s0 = 0; s0 < count; s0 += slice) {
        const size_t n = std::min(count, s0 + slice) - s0;
        VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(units), nodes_host + s0, n * 8, hipMemcpyHostToDevice, c->stream));
        if (int rc = generate_decode_slice(c, lay.at(units), n, C, l_host + s0 * C, lay.at(Lp), lay.at(recp),
                                           record_out + s0 * C))
            return rc;
    }
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}
