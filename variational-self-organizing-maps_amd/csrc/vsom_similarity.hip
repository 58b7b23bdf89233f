// vsom_similarity.hip -- Som::measureSimilarity's per-record report (Som.cpp:631-714) for chunk rows [r0, r1): the search of
// the staged chunk, then one launch that scores every row against its BMU (gfx950).
//
//  similarity_kernel : one wavefront per row.  The row's lastBMU entry (wavefront-uniform) names the map and sigmaMap rows
//                      to gather; lanes stride the C = min(J, D) columns, four consecutive columns per lane and step
//                      (16-byte loads) where the model row is one part (Standard / Median), one column per lane for CLR's
//                      two-part rows.  Two steps' loads are issued before the first value is used.  Per column, in fp32
//                      with one rounding per operation: sM (the select of Som.cpp:658 as written, or a floor),
//                      delta = (x - m) / sM / k (:671), lo = m - sM k, hi = m + sM k (:675-677).  Every lane keeps its own
//                      candidates in column order; the row's results are reductions over the 64 lanes with cross-lane
//                      moves -- a packed (ordered value, ~column) key for the two maxima, the lowest column for `first`, a
//                      sum for `outside` -- and the winning value itself comes from the lane that owns the winning column.
//                      No LDS, no atomics; lane 0 stores the row's nine words.
// The memory traffic is 12 C bytes per row (three gathered rows) plus C bytes of validity and 4 C of the dense report when
// those are asked for: the kernel is bound by the latency of the dependent gather (lastBMU -> model rows), not arithmetic.
//
//  similarity_kernel<true, true> : the same wavefront for vsom_similarity_masked_batch.  The row's unit and distance come
//                      from the results of the slice's masked search (vsom_masked_search_enqueue) instead of lastBMU / sqres,
//                      the validity from the packed bytes that search read (0xFF / 0x00, xpitch per row, or the one shared
//                      row), and delta of an invalid column is the quiet NaN by select before anything is reduced: such a
//                      column can be neither dmax nor first nor amax, is not counted outside, and stores 0 in the dense
//                      report, whatever x, map and sigmaMap hold there.  Lane 0 stores a tenth word, the row's nvalid.
#include "vsom_sim_row.hpp"
#include <algorithm>
#include <cstring>

#define SIM_ROWS_PER_WG 4
#define SIM_ROW_WORDS 9     // bmu (2), dist, dmax, dmax_col, first, amax, amax_col, outside
#define SIM_MROW_WORDS 10   // ... and nvalid (vsom_similarity_masked_batch)

// (SimArgs, the column arithmetic sim_column and the wave reductions: vsom_sim_row.hpp and vsom_sim_reduce.inc, shared
//  with the ensemble's masked query kernel)

// VEC: the model row is one part and lanes take four consecutive columns per step (pitches are multiples of 32 floats and
// C <= J, D: a 16-byte load of a row's last, partial quad stays inside the padded row).  Otherwise one column per lane and
// step, logical column d of a model row at (d / part_len) * part_pitch + d % part_len.
// MASKED (with VEC): unit, distance and nvalid of row r at entry r - s0 of the slice's search results, validity row r - s0
// of the packed rows (C <= J <= xpitch: the bytes of a partial quad are padding zeros).
template <bool VEC, bool MASKED = false>
__global__ __launch_bounds__(64 * SIM_ROWS_PER_WG) void similarity_kernel(SimArgs a, int r0, int s0, int s1)
{
    constexpr int W = VEC ? 4 : 1;
    constexpr int U = 2;                        // steps whose loads are in flight together
    const int lane = threadIdx.x & 63;
    const int r = s0 + (int)blockIdx.x * SIM_ROWS_PER_WG + (int)(threadIdx.x >> 6);
    if (r >= s1)
        return;                                 // (wavefront-uniform)
    const size_t ri = MASKED ? (size_t)(r - s0) : (size_t)r;    // the row's entry of lastbmu / sqres / nvalid
    u64 b = a.lastbmu[ri];
    b = b < (u64)a.N ? b : 0;                   // (the searches store indices below N)
    const float *xr = a.x + (size_t)r * a.ldx;
    const float *mr = a.map + (size_t)b * a.ldm;
    const float *sr = a.sigma + (size_t)b * a.ldm;
    const unsigned char *vr = MASKED ? a.valid + ri * (size_t)a.vstride
                                     : (a.valid ? a.valid + (size_t)(r - r0) * a.J : nullptr);
    float *dr = a.delta ? a.delta + (size_t)(r - s0) * a.C : nullptr;
    const int C = a.C;
    const bool quad_store = VEC && (C & 3) == 0;

    SimLane l;
    sim_lane_init(l);

    for (int g0 = lane; g0 * W < C; g0 += 64 * U) {
        float xv[U][W], mv[U][W], sv[U][W];
        unsigned char vv[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int g = g0 + 64 * u;
            if (g * W < C) {
                if constexpr (VEC) {
                    const float4 x4 = *reinterpret_cast<const float4 *>(xr + 4 * g);
                    const float4 m4 = *reinterpret_cast<const float4 *>(mr + 4 * g);
                    const float4 s4 = *reinterpret_cast<const float4 *>(sr + 4 * g);
                    xv[u][0] = x4.x, xv[u][1] = x4.y, xv[u][2] = x4.z, xv[u][3] = x4.w;
                    mv[u][0] = m4.x, mv[u][1] = m4.y, mv[u][2] = m4.z, mv[u][3] = m4.w;
                    sv[u][0] = s4.x, sv[u][1] = s4.y, sv[u][2] = s4.z, sv[u][3] = s4.w;
                } else {
                    const int part = g / a.part_len;
                    const int off = part * a.part_pitch + (g - part * a.part_len);
                    xv[u][0] = xr[g];
                    mv[u][0] = mr[off];
                    sv[u][0] = sr[off];
                }
#pragma unroll
                for (int e = 0; e < W; ++e)
                    vv[u][e] = (vr && g * W + e < C) ? vr[g * W + e] : (unsigned char)1;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int g = g0 + 64 * u;
            if (g * W < C) {
                float out[W];
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const int d = g * W + e;
                    out[e] = 0.f;
                    if (d < C)
                        out[e] = sim_column<MASKED>(l, a, (uint32_t)d, xv[u][e], mv[u][e], sv[u][e], vv[u][e] != 0);
                }
                if (dr) {
                    bool stored = false;
                    if constexpr (VEC) {
                        if (quad_store) {
                            *reinterpret_cast<float4 *>(dr + 4 * g) = make_float4(out[0], out[1], out[2], out[3]);
                            stored = true;
                        }
                    }
                    if (!stored) {
#pragma unroll
                        for (int e = 0; e < W; ++e)
                            if (g * W + e < C)
                                dr[g * W + e] = out[e];
                    }
                }
            }
        }
    }

    // the row's results over the 64 lanes; the lane that owns column c is (c / W) % 64
#include "vsom_sim_reduce.inc"
    if (lane == 0) {
        const size_t i = (size_t)(r - r0), R = (size_t)a.R;
        reinterpret_cast<u64 *>(a.rows)[i] = a.lastbmu[ri];
        a.rows[2 * R + i] = __float_as_uint(a.sqres[ri]);
        a.rows[3 * R + i] = __float_as_uint(dmax);
        a.rows[4 * R + i] = dc;
        a.rows[5 * R + i] = __float_as_uint(first);
        a.rows[6 * R + i] = __float_as_uint(amax);
        a.rows[7 * R + i] = ac;
        a.rows[8 * R + i] = cnt;
        if constexpr (MASKED)
            a.rows[9 * R + i] = a.nvalid[ri];
    }
}

// rows per slice of the dense report: its device scratch stays within 64 MiB
static size_t vsom_similarity_slice_rows(size_t C)
{
    return std::max<size_t>(1, ((size_t)64 << 20) / (4 * C));
}

// what the two launchers share: the operands of the context and the call's constants
static SimArgs sim_args(const vsom_ctx *c, size_t C, size_t rows, int num_sigmas, int sigma_rule)
{
    SimArgs a{};
    a.x = c->Xs.p;
    a.map = c->map.p;
    a.sigma = c->sigma.p;
    a.ldx = (int)c->xpitch;
    a.ldm = (int)c->pitch;
    a.part_len = (int)c->part_len;
    a.part_pitch = (int)c->part_pitch;
    a.J = (int)c->J;
    a.C = (int)C;
    a.N = (int)c->N;
    a.R = (int)rows;
    a.k = (float)num_sigmas;
    a.floor_rule = sigma_rule == VSOM_SIGMA_FLOOR;
    return a;
}

int launch_similarity(vsom_ctx *c, u64 min_hits, int num_sigmas, int sigma_rule, size_t r0, size_t r1,
                      const uint8_t *valid_host, const vsom_similarity_out *out)
{
    const size_t rows = r1 - r0;
    if (rows == 0)
        return VSOM_OK;
    const size_t C = std::min<size_t>(c->J, c->D);
    const size_t slice = out->delta ? std::min(vsom_similarity_slice_rows(C), rows) : rows;
    // the per-row results of the call and their pinned host image, the validity bytes when given, a slice's dense report
    const size_t words = rows * SIM_ROW_WORDS;
    vsom_layout lay, pin;
    const auto srows = lay.add<unsigned>(words), pinned = pin.add<unsigned>(words);
    const auto valid = lay.add<unsigned char>(valid_host ? rows * c->J : 0);
    const auto delta = lay.add<float>(out->delta ? slice * C : 0);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_pinned, pin, c->stream));

    // findRestrictedBmu of the whole chunk; with min_hits = 0 every node qualifies and the search is findBmu's
    int rc = min_hits == 0 ? launch_bmu_full(c, 0, c->B) : launch_bmu_restricted(c, min_hits);
    if (rc)
        return rc;
    if (valid_host)
        VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(valid), valid_host, rows * c->J, hipMemcpyHostToDevice, c->stream));

    SimArgs a = sim_args(c, C, rows, num_sigmas, sigma_rule);
    a.lastbmu = c->lastbmu.p;
    a.sqres = c->sqres.p;
    a.nvalid = nullptr;
    a.valid = valid_host ? lay.at(valid) : nullptr;
    a.vstride = (int)c->J;
    a.delta = out->delta ? lay.at(delta) : nullptr;
    a.rows = lay.at(srows);
    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0;
        {
            TimerScope ts(c, VSOM_T_FINISH);
            const dim3 grid((unsigned)((n + SIM_ROWS_PER_WG - 1) / SIM_ROWS_PER_WG)), block(64 * SIM_ROWS_PER_WG);
            if (c->nparts == 1)
                hipLaunchKernelGGL(similarity_kernel<true>, grid, block, 0, c->stream, a, (int)r0, (int)s0, (int)s1);
            else
                hipLaunchKernelGGL(similarity_kernel<false>, grid, block, 0, c->stream, a, (int)r0, (int)s0, (int)s1);
            VSOM_HIP_CHECK(hipGetLastError());
        }
        if (out->delta)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->delta + (s0 - r0) * C, lay.at(delta), n * C * 4, hipMemcpyDeviceToHost, c->stream));
    }
    VSOM_HIP_CHECK(hipMemcpyAsync(pin.at(pinned), lay.at(srows), words * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));

    const unsigned *p = pin.at(pinned);
    void *dst[SIM_ROW_WORDS - 1] = {out->bmu, out->dist, out->dmax, out->dmax_col, out->first, out->amax, out->amax_col, out->outside};
    for (int i = 0; i < SIM_ROW_WORDS - 1; ++i) {
        const size_t at = i == 0 ? 0 : (size_t)(i + 1) * rows, len = i == 0 ? 2 * rows : rows;
        if (dst[i])
            std::memcpy(dst[i], p + at, len * 4);
    }
    return VSOM_OK;
}

// vsom_similarity_masked_batch: per slice the validity bytes up and packed once, the masked search (VSOM_T_BMU), and the
// scoring of the slice's rows from the search's own results and packed bytes (VSOM_T_FINISH).  The slice follows the masked
// search's rule with the dense report's cap on top.
int launch_similarity_masked(vsom_ctx *c, u64 min_hits, int num_sigmas, int sigma_rule, size_t r0, size_t r1,
                             const uint8_t *valid_host, int one_mask, const vsom_similarity_masked_out *out)
{
    const size_t rows = r1 - r0;
    if (rows == 0)
        return VSOM_OK;
    const size_t C = c->J;                      // (Standard / Median: D = J)
    size_t slice = std::min(vsom_masked_search_slice_rows(c), rows);
    if (out->delta)
        slice = std::min(slice, vsom_similarity_slice_rows(C));
    const size_t words = rows * SIM_MROW_WORDS;
    vsom_layout lay, pin;
    const VsomMaskedSearch ms = vsom_masked_search_add(c, lay, one_mask != 0, slice);
    const auto srows = lay.add<unsigned>(words), pinned = pin.add<unsigned>(words);
    const auto delta = lay.add<float>(out->delta ? slice * C : 0);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_pinned, pin, c->stream));

    SimArgs a = sim_args(c, C, rows, num_sigmas, sigma_rule);
    a.lastbmu = lay.at(ms.bmu);
    a.sqres = lay.at(ms.dist);
    a.nvalid = lay.at(ms.nvalid);
    a.valid = lay.at(ms.packed);
    a.vstride = ms.one ? 0 : (int)c->xpitch;
    a.delta = out->delta ? lay.at(delta) : nullptr;
    a.rows = lay.at(srows);
    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0;
        {
            TimerScope ts(c, VSOM_T_BMU);
            if (int rc = vsom_masked_slice_enqueue(c, lay, ms, min_hits, r0, s0, s1, valid_host))
                return rc;
        }
        {
            TimerScope ts(c, VSOM_T_FINISH);
            const dim3 grid((unsigned)((n + SIM_ROWS_PER_WG - 1) / SIM_ROWS_PER_WG)), block(64 * SIM_ROWS_PER_WG);
            hipLaunchKernelGGL((similarity_kernel<true, true>), grid, block, 0, c->stream, a, (int)r0, (int)s0, (int)s1);
            VSOM_HIP_CHECK(hipGetLastError());
        }
        if (out->delta)
            VSOM_HIP_CHECK(hipMemcpyAsync(out->delta + (s0 - r0) * C, lay.at(delta), n * C * 4, hipMemcpyDeviceToHost, c->stream));
    }
    VSOM_HIP_CHECK(hipMemcpyAsync(pin.at(pinned), lay.at(srows), words * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));

    const unsigned *p = pin.at(pinned);
    void *dst[SIM_MROW_WORDS - 1] = {out->bmu,  out->dist,     out->dmax,    out->dmax_col, out->first,
                                     out->amax, out->amax_col, out->outside, out->nvalid};
    for (int i = 0; i < SIM_MROW_WORDS - 1; ++i) {
        const size_t at = i == 0 ? 0 : (size_t)(i + 1) * rows, len = i == 0 ? 2 * rows : rows;
        if (dst[i])
            std::memcpy(dst[i], p + at, len * 4);
    }
    return VSOM_OK;
}
