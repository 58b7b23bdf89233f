// vsom_evaluate.hip -- Som::evaluate (Som.cpp:490-523), the validation loss of a map, for chunk rows [r0, r1): findBmu of the
// staged chunk (vsom_bmu_batch's path), one launch that scores every row against its BMU, the running mean on the host (gfx950).
//
//  evaluate_kernel : eight lanes per row, eight rows per wavefront.  A row's lastBMU entry names the model row to gather.
//                    Per logical column d < C = min(J, D), in fp32 with one rounding per operation, nothing contracted:
//                      be = log(m) * x + log(1.0f - m) * (1.0f - x) (:509), NaN / inf -> -99999.0f (:512),
//                      val = valid ? continuous[d] : 0.0f (:505), t = (be * binary[d]) * val (:514), bsum = t.dot(t) (:519).
//                    The sum takes Eigen's packet order (tests/pyref.py:dot_self), which the contract fixes, so
//                    the row is NOT reduced by a 64-lane tree: lane c of a row's eight owns element c of the two 4-wide
//                    packet accumulators and walks the columns 8k + c < a2 = C / 8 * 8 in order; lane c also squares the
//                    one column a2 + c behind them.  Then, with cross-lane moves inside the eight: p0 += p1 (lane c takes
//                    lane c + 4), the packet tail when C - a2 >= 4 (lanes 0..3 add their own column), (p0[0] + p0[2]) +
//                    (p0[1] + p0[3]), and the at most three scalar-tail columns added one by one.  Accumulators start at +0:
//                    +0 + p = p exactly for a square p, so every branch of Eigen's redux (C < 4, 4 <= C < 8, C >= 8) is this
//                    one sequence.  No LDS, no atomics; lane 0 of the eight stores the row's five words.
//                    (The row body -- ev_zero, ev_square, the column rule, the walk, the tail, the reduction -- lives in
//                    vsom_eval_row.hpp / .inc, which ensemble_evaluate_many_kernel of vsom_ensemble.hip includes too.)
//                    A column whose factor is an exact zero -- binary[d] == 0 with a finite val, or val == 0 with a finite
//                    binary[d] -- has t = +-0 whatever m and x hold (be is finite after :512), and adding its +0 changes no
//                    accumulator: such a column is skipped before anything of the row is gathered.  With the usual few
//                    binary columns the kernel reads the column arrays and the validity bytes and little else.
//  evaluate_kernel<false, true> : the same eights for vsom_evaluate_masked_batch.  The row's unit and distance come from the
//                    results of the slice's masked search instead of lastBMU / sqres, the validity from the packed bytes that
//                    search read (xpitch per row, or the one shared row), and t = valid ? (be * binary[d]) * continuous[d] : +0
//                    is a select: an invalid column adds +0 whatever its factors, x and m hold -- it is skipped like a zero
//                    factor and counts no replaced term.  Lane 0 of the eight stores a sixth word, the row's nvalid.
// What bounds it: the dependent gather lastBMU -> model row (as similarity_kernel), then for the columns that count two
// logs each; a row's eight lanes read 32 consecutive bytes per step, four steps in flight.  Memory traffic per row: J validity
// bytes when given, 8 bytes (x and m) per counting column; the two column arrays stay in cache.
// log is the device math library's single-precision logf (-fno-fast-math: the accurate form, denormals kept).  No statement
// of its error bound ships with the ROCm installation this was written against; HIP's published table of device math
// functions gives 1 ulp for logf, and the project already relies on the same library's "within an ulp" for exp in
// vsom_bmd_batch.  The tolerance of include/vsom_hip.h therefore takes L = 1 AS AN ASSUMPTION.
// Against the host loop this call replaces in the C++ mirror (libm logf, a sequential sum) the value of a data set with
// binary columns moves within that tolerance; with no binary column every t is +-0, bsum is 0 and the value is the same bits.
#include "vsom_eval_row.hpp"
#include <algorithm>
#include <cstring>

struct EvArgs {
    const float *x;             // staged rows (Xs), pitch ldx
    const float *map;           // model rows, pitch ldm
    const u64 *lastbmu;         // per chunk row; MASKED: the slice's search results, entry r - r0 for row r of slice [r0, r1)
    const float *sqres;
    const unsigned *nvalid;     // MASKED only: the slice's counts of valid columns
    const unsigned char *valid; // rows [r0, r1) x J, or null: every column valid; MASKED: the slice's packed rows, vstride
                                // bytes apart (0: the one row every sample shares)
    const float *binary, *continuous;   // [J]
    unsigned *rows;             // per-row results of [r0, r1): EV_ROW_WORDS arrays of R entries
    int ldx, ldm, part_len, part_pitch;
    int J, C, N, R, vstride;
    int out0;                   // MASKED: the slice's first row in the call's results (r0 of the slice - r0 of the call)
};

// CLR: the model row has two parts, logical column d at (d / part_len) * part_pitch + d % part_len (as similarity_kernel<false>)
// MASKED: [r0, r1) is one slice of the call; the search results and the packed validity rows are the slice's own.
template <bool CLR, bool MASKED = false>
__global__ __launch_bounds__(EV_LANES * EV_ROWS_PER_WG) void evaluate_kernel(EvArgs a, int r0, int r1)
{
    const int c = threadIdx.x & (EV_LANES - 1);
    const int row = r0 + (int)blockIdx.x * EV_ROWS_PER_WG + (int)(threadIdx.x / EV_LANES);
    const bool live = row < r1;
    const int r = live ? row : r1 - 1;              // (a dead eight repeats the last row and stores nothing)
    const size_t ri = MASKED ? (size_t)(r - r0) : (size_t)r;    // the row's entry of lastbmu / sqres / nvalid
    u64 b = a.lastbmu[ri];
    b = b < (u64)a.N ? b : 0;                       // (the searches store indices below N)
    const float *xr = a.x + (size_t)r * a.ldx;
    const float *mr = a.map + (size_t)b * a.ldm;
    const unsigned char *vr = MASKED ? a.valid + ri * (size_t)a.vstride
                                     : (a.valid ? a.valid + (size_t)(r - r0) * a.J : nullptr);
    auto model = [&](int d) -> float {
        if constexpr (CLR) {
            const int part = d / a.part_len;
            return mr[part * a.part_pitch + (d - part * a.part_len)];
        } else {
            return mr[d];
        }
    };
#include "vsom_eval_row.inc"
    if (live && c == 0) {
        const size_t i = (size_t)(r - r0) + (MASKED ? (size_t)a.out0 : 0), R = (size_t)a.R;
        reinterpret_cast<u64 *>(a.rows)[i] = a.lastbmu[ri];
        a.rows[2 * R + i] = __float_as_uint(a.sqres[ri]);
        a.rows[3 * R + i] = __float_as_uint(s);
        a.rows[4 * R + i] = nrepl;
        if constexpr (MASKED)
            a.rows[5 * R + i] = a.nvalid[ri];
    }
}

// what the two launchers share: the operands of the context and the column arrays (binary, then continuous)
static EvArgs ev_args(const vsom_ctx *c, size_t C, size_t rows, const float *cols)
{
    EvArgs a{};
    a.x = c->Xs.p;
    a.map = c->map.p;
    a.binary = cols;
    a.continuous = cols + c->J;
    a.ldx = (int)c->xpitch;
    a.ldm = (int)c->pitch;
    a.part_len = (int)c->part_len;
    a.part_pitch = (int)c->part_pitch;
    a.J = (int)c->J;
    a.C = (int)C;
    a.N = (int)c->N;
    a.R = (int)rows;
    return a;
}

int launch_evaluate(vsom_ctx *c, size_t r0, size_t r1, const float *binary_host, const float *continuous_host,
                    const uint8_t *valid_host, const vsom_evaluate_out *out)
{
    const size_t rows = r1 - r0;
    if (rows == 0) {
        if (out->error)
            *out->error = 0.0;
        return VSOM_OK;
    }
    const size_t J = c->J, C = std::min<size_t>(c->J, c->D);
    // the per-row results of the call, the validity bytes when given, the column arrays.  The pinned image holds the two
    // column arrays on their way in (behind the rows' words) and the rows' words on their way out.
    const size_t words = rows * EV_ROW_WORDS;
    vsom_layout lay, pin;
    const auto erows = lay.add<unsigned>(words), pinned = pin.add<unsigned>(words + 2 * J);
    const auto valid = lay.add<unsigned char>(valid_host ? rows * J : 0);
    const auto ecols = lay.add<float>(2 * J);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_pinned, pin, c->stream));

    int rc = launch_bmu_full(c, 0, c->B);           // findBmu of the whole chunk, as vsom_bmu_batch
    if (rc)
        return rc;
    float *cols = reinterpret_cast<float *>(pin.at(pinned) + words);
    std::memcpy(cols, binary_host, J * 4);
    std::memcpy(cols + J, continuous_host, J * 4);
    VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(ecols), cols, 2 * J * 4, hipMemcpyHostToDevice, c->stream));
    if (valid_host)
        VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(valid), valid_host, rows * J, hipMemcpyHostToDevice, c->stream));

    EvArgs a = ev_args(c, C, rows, lay.at(ecols));
    a.lastbmu = c->lastbmu.p;
    a.sqres = c->sqres.p;
    a.valid = valid_host ? lay.at(valid) : nullptr;
    a.vstride = (int)J;
    a.rows = lay.at(erows);
    {
        TimerScope ts(c, VSOM_T_FINISH);
        const dim3 grid((unsigned)((rows + EV_ROWS_PER_WG - 1) / EV_ROWS_PER_WG)), block(EV_LANES * EV_ROWS_PER_WG);
        if (c->nparts == 1)
            hipLaunchKernelGGL(evaluate_kernel<false>, grid, block, 0, c->stream, a, (int)r0, (int)r1);
        else
            hipLaunchKernelGGL(evaluate_kernel<true>, grid, block, 0, c->stream, a, (int)r0, (int)r1);
        VSOM_HIP_CHECK(hipGetLastError());
    }
    VSOM_HIP_CHECK(hipMemcpyAsync(pin.at(pinned), lay.at(erows), words * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));

    const unsigned *p = pin.at(pinned);
    if (out->bmu)
        std::memcpy(out->bmu, p, rows * 8);
    void *dst[3] = {out->dist, out->bsum, out->nrepl};
    for (int i = 0; i < 3; ++i)
        if (dst[i])
            std::memcpy(dst[i], p + (size_t)(i + 2) * rows, rows * 4);
    if (out->error)
        *out->error = ev_running_mean(reinterpret_cast<const float *>(p + 2 * rows), reinterpret_cast<const float *>(p + 3 * rows), rows);
    return VSOM_OK;
}

// vsom_evaluate_masked_batch: per slice the validity bytes up and packed once, the masked search (VSOM_T_BMU), and the scoring
// of the slice's rows from the search's own results and packed bytes (VSOM_T_FINISH); the running mean over the masked
// distances on the host.
int launch_evaluate_masked(vsom_ctx *c, u64 min_hits, size_t r0, size_t r1, const float *binary_host,
                           const float *continuous_host, const uint8_t *valid_host, int one_mask,
                           const vsom_evaluate_masked_out *out)
{
    const size_t rows = r1 - r0;
    if (rows == 0) {
        if (out->error)
            *out->error = 0.0;
        return VSOM_OK;
    }
    const size_t J = c->J, C = J;                   // (Standard / Median: D = J)
    const size_t slice = std::min(vsom_masked_search_slice_rows(c), rows);
    const size_t words = rows * EV_MROW_WORDS;
    vsom_layout lay, pin;
    const VsomMaskedSearch ms = vsom_masked_search_add(c, lay, one_mask != 0, slice);
    const auto erows = lay.add<unsigned>(words), pinned = pin.add<unsigned>(words + 2 * J);
    const auto ecols = lay.add<float>(2 * J);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_pinned, pin, c->stream));

    float *cols = reinterpret_cast<float *>(pin.at(pinned) + words);
    std::memcpy(cols, binary_host, J * 4);
    std::memcpy(cols + J, continuous_host, J * 4);
    VSOM_HIP_CHECK(hipMemcpyAsync(lay.at(ecols), cols, 2 * J * 4, hipMemcpyHostToDevice, c->stream));

    EvArgs a = ev_args(c, C, rows, lay.at(ecols));
    a.lastbmu = lay.at(ms.bmu);
    a.sqres = lay.at(ms.dist);
    a.nvalid = lay.at(ms.nvalid);
    a.valid = lay.at(ms.packed);
    a.vstride = ms.one ? 0 : (int)c->xpitch;
    a.rows = lay.at(erows);
    for (size_t s0 = r0; s0 < r1; s0 += slice) {
        const size_t s1 = std::min(r1, s0 + slice), n = s1 - s0;
        {
            TimerScope ts(c, VSOM_T_BMU);
            if (int rc = vsom_masked_slice_enqueue(c, lay, ms, min_hits, r0, s0, s1, valid_host))
                return rc;
        }
        TimerScope ts(c, VSOM_T_FINISH);
        a.out0 = (int)(s0 - r0);
        const dim3 grid((unsigned)((n + EV_ROWS_PER_WG - 1) / EV_ROWS_PER_WG)), block(EV_LANES * EV_ROWS_PER_WG);
        hipLaunchKernelGGL((evaluate_kernel<false, true>), grid, block, 0, c->stream, a, (int)s0, (int)s1);
        VSOM_HIP_CHECK(hipGetLastError());
    }
    VSOM_HIP_CHECK(hipMemcpyAsync(pin.at(pinned), lay.at(erows), words * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));

    const unsigned *p = pin.at(pinned);
    if (out->bmu)
        std::memcpy(out->bmu, p, rows * 8);
    void *dst[4] = {out->dist, out->bsum, out->nrepl, out->nvalid};
    for (int i = 0; i < 4; ++i)
        if (dst[i])
            std::memcpy(dst[i], p + (size_t)(i + 2) * rows, rows * 4);
    if (out->error)
        *out->error = ev_running_mean(reinterpret_cast<const float *>(p + 2 * rows), reinterpret_cast<const float *>(p + 3 * rows), rows);
    return VSOM_OK;
}
