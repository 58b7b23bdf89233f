// vsom_internal.hpp -- shared declarations of libvsom_hip.so (gfx950 only).
//
// Layout in HBM (see DESIGN.md "Data layout"):
//   model rows   : N x pitch fp32, pitch = nparts * part_pitch, part_pitch = roundup(part_len,32)
//                  Standard/Median: one part of D floats; CLR: [A(P) | B(P)], P = D/2.
//                  pad columns are kept at zero.
//   samples      : Bcap x xpitch fp32 (xpitch = roundup(J,32), zero padded)
//   CLR samples  : XP/YP Bcap x part_pitch (x'_p = x[i(p)], y'_p = x[j(p)], pairs i<j
//                  lexicographic, Transformation.cpp:94-101)
//   cw           : (c = w/W prefix, w) per (sample, node), pair-interleaved: one float4
//                  {c_j, w_j, c_j+1, w_j+1} at [(j>>1)][node], ceil(B/2)+8 pair rows of ldn nodes
//   Xnext[2]     : raw B x J chunks landing on the copy stream (double-buffered ingest)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/vsom_hip.h"
#include "vsom_buf.hpp"
#include "vsom_sched_round.hpp"

typedef unsigned long long u64;

// lane = node update kernels yield ceil(N/64)*ceil(D/14) wavefronts; at or below this many the
// (node, dim pair)-per-lane chain kernels are used instead (1024 SIMDs on the chip).  While every wavefront
// has a SIMD to itself the assembly kernels take ~0.12 us per sample whatever the map, the LDS-staged chain
// kernel ~2.2e-13 s per (node, dim, sample): they meet near N*D = 4e5 (tools/exp/chain_crossover.py:
// 4096 x 128: 0.99 vs 1.12 ms at B = 8192; 4096 x 64: ~2 vs 0.75 ms at B = 16384)
#define VSOM_CHAIN_MAX_WAVES 448

#define VSOM_TK 32          // K-chunk of the tile kernels; row pitches are multiples of it
#define TILE 64             // nodes (and, but for CLR, samples) of a distance tile (vsom_dist_tile.hpp; vsom_exact_plan sizes grids by it)

// spare rows behind the staged sample matrices (readable, contents unspecified: zero at allocation, stale
// samples after a larger chunk): the pipelined update kernels read ahead into them and never consume them
constexpr size_t VSOM_ROW_PAD = 32;
// bytes of vsom_ctx::onl_state (layout: vsom_online.hpp)
constexpr size_t VSOM_ONL_STATE_BYTES = 4352;

struct vsom_custom_state;

// The lane = node column-quad chain kernels of the hand-scheduled code object (gen_nt_asm.py), by arithmetic and by form:
// FULL runs the M and S chains with one column quad per wavefront (`_nt4`); the MEAN forms run the M chain alone, for
// epochs whose sigmaMap stays pending, with one quad per wavefront (`_nt4`) or two (`_nt8`).  Which one an epoch launches:
// vsom_phase2_plan.hpp.
enum VsomQuadVariant { VSOM_QV_STD, VSOM_QV_FMA, VSOM_QV_SFMA, VSOM_QV_MED, VSOM_QV_COUNT };
enum VsomQuadForm { VSOM_QF_FULL, VSOM_QF_MEAN_ONE_QUAD, VSOM_QF_MEAN_TWO_QUADS, VSOM_QF_COUNT };

struct vsom_ctx {
    int device = 0;
    uint32_t W = 0, H = 0, J = 0, D = 0, N = 0;
    int transform = 0;
    uint32_t nparts = 1, part_len = 0, part_pitch = 0, pitch = 0;
    uint32_t xpitch = 0;
    int bmu_mode = VSOM_BMU_AUTO;

    hipStream_t own_stream = nullptr, stream = nullptr;
    // side stream for work that only has to finish before the next entry point (the MSE sum)
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool aux_pending = false;

    // model state
    DevBuf<float> map, sigma, S, weight;
    DevBuf<u64> hits;

    // chunk
    size_t B = 0, Bcap = 0;
    bool chunk_loaded = false;      // a chunk (possibly of 0 rows) has been staged
    DevBuf<float> Xs, XP, YP;
    DevBuf<float> Xraw;             // staging for host uploads (B x J, unpadded)
    // double-buffered ingest: raw chunks land here on copy_stream while the current chunk trains
    DevBuf<float> Xnext[2];
    size_t Bnext = 0;
    int next_slot = 0;              // slot the next prefetch writes
    int ready_slot = -1;            // slot holding a prefetched, not yet committed chunk
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copied[2] = {nullptr, nullptr};    // H2D copy into slot finished
    hipEvent_t ev_staged[2] = {nullptr, nullptr};    // staging kernels that read slot finished
    bool staged_valid[2] = {false, false};
    DevBuf<u64> lastbmu;
    DevBuf<float> sqres;
    // The NEXT chunk staged beside the epoch of the current one (vsom_prefetch_chunk / vsom_stage_next_device -> copy
    // stream; vsom_commit_chunk adopts it).  Once a phase 2 has built its transposed chunk nothing of the epoch reads the
    // staged rows (Xs, Xc, the int8 images) any more -- `ev_rows_free` -- so the staging kernels of chunk k+1 may
    // overwrite them while the chains of chunk k run; what phase 2 still reads is double-buffered: lastBMU and the
    // compaction's column record (the *_alt set is what the ahead staging writes, commit swaps the two).
    DevBuf<u64> lastbmu_alt;
    DevBuf<int> cc_idx_alt, cc_inv_alt;
    DevBuf<unsigned> cc_meta_alt;
    hipEvent_t ev_rows_free = nullptr, ev_ahead = nullptr;
    // ev_rows_free belongs to the last enqueued work on this context.  Set only by launch_phase2 behind its last reader of
    // the staged rows; an entry point may leave it set only if it enqueues no reader of the staged rows (Xs, XP / YP, Xc,
    // the int8 images) -- the copy-stream calls, a further phase-2 range on the transposed chunk.  Every other entry point
    // clears it before it enqueues: CHECK_CTX does, and so must those that do without it (the online chunk, the phase-2
    // chain kernels, the ensemble's train calls).
    bool rows_free_valid = false;
    bool ahead_valid = false;       // a chunk is staged ahead (ahead_B rows; its compaction / int8-image state below)
    // staging kernels of a chunk staged ahead have been launched over the staged-row buffers and `stream` has neither
    // adopted them nor staged a chunk of its own since (whatever ahead_valid says: the ahead chunk may have been abandoned):
    // `stream` must wait for ev_ahead before it writes those buffers, and nobody may read the current chunk's rows
    bool ahead_rows = false;
    size_t ahead_B = 0;
    bool ahead_cc = false, ahead_xi = false;
    const float *next_dev = nullptr;   // vsom_stage_next_device: rows in HBM waiting for vsom_commit_chunk
    size_t next_dev_B = 0;
    bool next_dev_pending = false;
    PinnedBuf<float> mse;           // [1]  pinned HOST memory (device-visible): kernels store, vsom_get_mse reads after a stream wait
    // vsom_batch_schedule (vsom_tiny.hip): the schedule's neighbourhood tables followed by each epoch's table offset --
    // pinned image and device copy, one set -- and the per-epoch MSE words the kernel stores (pinned, as `mse`).  The
    // call blocks, so nothing reads them between calls.
    PinnedBuf<unsigned char> sch_host; DevBuf<unsigned char> sch_dev;
    PinnedBuf<float> sch_mse;
    DevBuf<int> pair_i, pair_j;     // CLR pair tables [P]

    // BMU tile-search scratch
    DevBuf<u64> partial;
    DevBuf<unsigned char> nan0;

    // duplicate-row representatives of the exact search (vsom_bmu.hip, bmu_dedupe_*)
    DevBuf<u64> dd_hash; DevBuf<int> dd_rep, dd_list;
    bool dedupe = true;             // VSOM_NO_DEDUPE=1 switches it off (A/B measurements)
    double dd_min_work = 2.0e10;    // exact searches of at least this many (sample, node, value) triples (vsom_set_row_dedupe)

    // MFMA shortlist scratch
    DevBuf<float> sl_G, sl_nrm; DevBuf<unsigned> sl_scal;
    DevBuf<float> sl_a2;            // CLR shortlist: per-node max A^2 (the select kernel's per-node bounds)
    DevBuf<int> sl_list;
    DevBuf<float> sl_tmin;
    PinnedBuf<unsigned> sl_fb;      // pinned host feedback: {redo samples, candidates, rows, seq}
    DevBuf<float> sl_fs, sl_fm;     // CLR shortlist: sample / node feature rows (vsom_shortlist.hip)
    // integer contraction of the shortlist (vsom_sl_i8.hip): int8 images of the chunk / the model rows
    DevBuf<signed char> sl_xi; DevBuf<float> sl_l1;
    DevBuf<signed char> sl_q; DevBuf<double> sl_qscale, sl_qcorr;
    DevBuf<int4> sl_qfast;          // per node: the constants of the uint8 kind's fp32 epilogue (sl_i8_value_fast)
    uint32_t sl_kp8 = 0;
    bool xi_valid = false;          // sl_xi / sl_l1 describe the staged chunk
    int sl_par = 0;                 // which of the two scal sets the next search uses
    int sl_skip = 0;
    unsigned sl_seq_seen = 0;       // feedback sequence number already acted on
    int sl_fail_streak = 0;         // consecutive probes that had to redo most samples exactly

    // neighbourhood
    DevBuf<float2> cw;
    DevBuf<float> lut; PinnedBuf<float> lut_host;     // lut_host: 2 x lut.cap
    hipEvent_t lut_ev[2] = {nullptr, nullptr}; bool lut_ev_valid[2] = {false, false}; int lut_slot = 0;
    double lut_sigma = -1.0; uint32_t lut_w = 0, lut_h = 0;
    DevBuf<double> lutd; double lutd_sigma = -1.0;   // online path (double)
    // the table's host image: two pinned slots used alternately (the device copy is enqueued on the stream, one-launch
    // chunks of tiny maps read the slot itself), each guarded by an event recorded behind its last reader
    PinnedBuf<double> lutd_host; double lutd_host_sigma[2] = {-1.0, -1.0};   // 2 slots of W x H
    hipEvent_t lutd_ev[2] = {nullptr, nullptr}; bool lutd_ev_valid[2] = {false, false}; int lutd_slot = 0;

    // hand-scheduled update kernel (code object loaded with hipModuleLoadData)
    void *upd_module = nullptr, *upd_clr8 = nullptr;
    void *upd_quad[VSOM_QF_COUNT][VSOM_QV_COUNT] = {};   // the lane = node quad kernels (vsom_load_asm_module names them)
    bool mean_nt4 = false;          // development builds only (VSOM_MEAN_NT4): deferred epochs launch the `_nt4` forms at every size
    int update_mode = VSOM_UPDATE_STRICT;
    bool use_chain = true;
    bool use_tiny = true;           // one-launch epoch for tiny maps (VSOM_NO_TINY=1 disables, debugging)

    // column compaction (vsom_compact.hip): columns that are zero in every row of the chunk are retired exactly
    DevBuf<unsigned> cc_flags;      // [xpitch] live flags
    DevBuf<int> cc_idx;             // [cpitch] live column list, -1 beyond the live count
    DevBuf<int> cc_inv;             // [xpitch] column -> compacted position or -1
    DevBuf<unsigned> cc_meta;       // device: {live columns, live 14-dim slices, live columns rounded up to 32, seq}
    PinnedBuf<unsigned> cc_fb;      // pinned host mirror: {live columns, seq}
    unsigned cc_seen = 0;
    int cc_skip = 0;
    long cc_min_rows = 1024;        // chunks with fewer rows are not compacted (< 0: never)
    bool cc_valid = false;          // the staged chunk has a compaction (Xc, cc_idx, cc_meta describe it)
    uint32_t cpitch = 0;            // row pitch of the compacted matrices
    DevBuf<float> Xc;               // (Bcap + VSOM_ROW_PAD) x cpitch
    DevBuf<float> Mc;               // N x cpitch: model rows on the live columns (search)
    DevBuf<float> Uc_map, Uc_S;     // N x cpitch: the chains' M and raw S on the live columns
    // the chunk transposed into column quads (vsom_xq.hip) for the lane = node, four-dims-per-wavefront chain kernels
    DevBuf<float4> Xq;              // [quads rounded up to 8][bpad]
    DevBuf<unsigned> zq;            // [quads][bpad / 32] all-zero (sample, quad) bits
    bool xq_valid = false;
    uint32_t xq_bpad = 0, xq_quads = 0;

    // Deferred sigmaMap (vsom_update.hip, "pending sigma"): a full-range phase 2 on the QUADS path whose plan says `deferred`
    // (vsom_phase2_plan.hpp) runs a MEAN form of the quad kernels and leaves sigmaMap unwritten; `sg` then records what the
    // FULL form of the same variant needs to produce that epoch's sigmaMap later (vsom_phase2_replay plans that launch).  Its inputs are the context's own buffers -- Xq / zq, cw, weight and the
    // compaction's scratch rows are written by launch_phase2 alone, which drops or materialises the record first -- except
    // the live-column record and lastBMU, which the staging and the search of the next chunk overwrite: sg_inv / sg_meta /
    // sg_bmu are owned copies.  The mean-only kernel takes the c-only form of the (c,w) array (half the bytes), so the
    // record also keeps the epoch's sigma: the materialisation runs the neighbourhood pass again in its full form.
    // Every entry point materialises it (vsom_sigma_flush_pending via vsom_join_aux) but the listed ones that never
    // read sigmaMap (vsom_capi.hip, CHECK_CTX_KEEP); the next full-range epoch, which overwrites every row, drops it.
    struct PendingSigma {
        bool on = false;
        size_t B = 0;
        uint32_t bpad = 0;
        bool compact = false;
        VsomQuadVariant variant = VSOM_QV_STD;   // the update mode and transformation in force at that epoch
        double sigma = 0.0;         // the epoch's sigma: the table of its neighbourhood pass.  (Today every call that
                                    // retabulates -- another phase 2, the tiny and custom paths -- materialises or drops the
                                    // record first, so the table in place is still this one; the record does not rely on it.)
    } sg;
    DevBuf<int> sg_inv; DevBuf<unsigned> sg_meta;
    DevBuf<u64> sg_bmu;             // [B] the epoch's lastBMU
    int sigma_mode = VSOM_SIGMA_AUTO;
    unsigned sigma_unread = 0;      // full-range epochs since the last entry point that may have read sigmaMap (AUTO)
    bool sigma_shared = false;      // a group or an ensemble reads this context's buffers directly: never deferred
    uint64_t sg_stats[3] = {0, 0, 0};   // epochs deferred, dropped, materialised

    // online path scratch
    DevBuf<float> v_dev;            // one sample, padded
    PinnedBuf<float> v_pinned;      // its pinned host staging (+ 16 floats for results)
    DevBuf<float> res_dev;          // residual
    DevBuf<u64> onl_state;          // argmin key slots + flags of the online scan (vsom_online.hpp)
    DevBuf<float> onl_f;            // [4]: dist, mse
    // image-bounded search of the online chunk loop (vsom_online_i8.hip): one byte per model value + 4 scalars per node,
    // lower bounds of the sample being searched, min-upper-bound slots, per-sample bound terms
    DevBuf<unsigned char> onl_img; DevBuf<float4> onl_nsc; DevBuf<float> onl_lb; DevBuf<unsigned> onl_u;
    DevBuf<float4> onl_xsc;
    DevBuf<unsigned char> onl_dirty;         // [N] nodes whose sigmaMap row is written at the end of the chunk

    // pinned staging of vsom_set_state's host arrays
    PinnedBuf<float> st_pinned;
    PinnedBuf<u64> out_pinned;      // [8192]: vsom_get_last_bmu of short chunks
    // scratch arenas of the chunk and distance queries (vsom_layout, vsom_buf.hpp): every call lays out what it needs and
    // the arena grows to the largest layout asked for.  The contents belong to the running call: nothing in them may be
    // expected to survive into the next entry point.
    DevBuf<unsigned char> q_scratch;
    PinnedBuf<unsigned char> q_pinned;
    // vsom_umatrix (vsom_umatrix.hip): U[N] of the last call, allocated on first use
    DevBuf<double> umatrix;
    bool um_valid = false;          // a vsom_umatrix has been enqueued on this context

    // timing
    uint32_t timing = 0;            // bit (1u << VSOM_T_*): that kernel group is timed with HIP events
    struct Ev { hipEvent_t a, b; int which; };
    std::vector<Ev> ev_live;
    std::vector<Ev> ev_pool;
    float t_ms[VSOM_T_COUNT] = {0};
    uint32_t t_cnt[VSOM_T_COUNT] = {0};

    bool in_group = false;          // a member of a vsom_group (vsom_group.hip): ensembles refuse it

    // Accumulated epoch (vsom_accum.hip): between vsom_batch_accum_begin and _end / _abort the chains of every node continue
    // in acc_M / acc_S (N x pitch) and acc_W (N) from where the previous chunk left them, acc_mse is the running MSE word
    // and `rows` counts what has been accumulated.  The buffers are the feature's own: allocated by the first begin, kept.
    struct AccumEpoch {
        bool open = false;
        double sigma = 0.0;
        int is_first = 0;
        size_t total = 0, rows = 0;
        bool masked = false;        // a masked chunk has been accumulated: the ever-dirty list below may hold columns
    } ac;
    DevBuf<float> acc_M, acc_S, acc_W, acc_mse;
    // Masked chunks of an accumulated epoch (vsom_accum_masked.hip): a column that had an invalid entry in some chunk of the
    // epoch ("ever dirty") carries M_d, S_d and its own weight sum W_d in acm_M / acm_S / acm_W ([column][node], rows of
    // N rounded up to 64), and acc_M / acc_S hold dead values there.  acm_ever / acm_fresh: per column, ever dirty / became
    // dirty in the chunk being accumulated; acm_cols: the ever-dirty columns in ascending order, acm_meta[0] their count.
    // All on the device (no host round trip), allocated by the first masked chunk and kept; begin clears ever and count.
    // acm_valid: the pinned staging of the caller's validity bytes, two halves used alternately, each guarded by an event
    // recorded behind its copy.
    DevBuf<float> acm_M, acm_S, acm_W;
    DevBuf<unsigned char> acm_ever, acm_fresh;
    DevBuf<int> acm_cols;
    DevBuf<unsigned> acm_meta;
    PinnedBuf<unsigned char> acm_valid;
    hipEvent_t acm_ev[2] = {nullptr, nullptr}; bool acm_ev_valid[2] = {false, false}; int acm_slot = 0;

    // caller-defined transformation (vsom_create_custom, vsom_custom.hip); null for the built-in ones
    vsom_custom_state *cu = nullptr;
};

// error plumbing -----------------------------------------------------------------------------
void vsom_set_error(const std::string &msg);
int vsom_fail(int code, const std::string &msg);
// (an allocation that does not fit is VSOM_ERR_NOMEM and leaves the context usable: every buffer is grown through
// vsom_buf.hpp, which drops the old buffer first and leaves a set whole or absent, and the runtime's last-error slot is
// cleared so that the next hipGetLastError() of a launch sequence does not report it again)
#define VSOM_HIP_CHECK_AS(expr, what)                                                    \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            (void)hipGetLastError();                                                     \
            return vsom_fail(_e == hipErrorOutOfMemory ? VSOM_ERR_NOMEM : VSOM_ERR_HIP,  \
                             std::string(what) + ": " + hipGetErrorString(_e));          \
        }                                                                                \
    } while (0)
#define VSOM_HIP_CHECK(expr) VSOM_HIP_CHECK_AS(expr, #expr)
// vsom_grow / vsom_grow_set: the message names the allocation
#define VSOM_ALLOC_CHECK(expr) VSOM_HIP_CHECK_AS(expr, "hipMalloc in " #expr)

// the gate of the entry points (vsom_capi.hip and the files that define entry points of their own) ------------------
#define CHECK_CTX(ctx)                                                 \
    do {                                                               \
        if (!(ctx))                                                    \
            return vsom_fail(VSOM_ERR_INVALID, "null context");        \
        hipError_t _e = hipSetDevice((ctx)->device);                   \
        if (_e != hipSuccess)                                          \
            return vsom_fail(VSOM_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(_e)); \
        if (int _rc = vsom_join_aux(ctx))                              \
            return _rc;                                                \
        (ctx)->rows_free_valid = false;   /* whatever follows may read the staged rows again */ \
    } while (0)
// The same for the entry points that provably never read sigmaMap and overwrite nothing a pending one is made from (chunk
// staging, the batch phases, the MSE and lastBMU read-backs, timing, statistics, synchronisation): a pending sigmaMap stays
// pending (vsom_internal.hpp, vsom_ctx::sg).  CHECK_CTX is the default and materialises it -- an entry point missing
// here costs time, one wrongly listed here would cost correctness.
#define CHECK_CTX_KEEP(ctx)                                            \
    do {                                                               \
        if (!(ctx))                                                    \
            return vsom_fail(VSOM_ERR_INVALID, "null context");        \
        hipError_t _e = hipSetDevice((ctx)->device);                   \
        if (_e != hipSuccess)                                          \
            return vsom_fail(VSOM_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(_e)); \
        if (int _rc = vsom_join_aux_keep(ctx))                         \
            return _rc;                                                \
        (ctx)->rows_free_valid = false;                                \
    } while (0)
// Entry points that READ the staged rows (Xs / XP / YP, the gathered rows, the int8 images): once the NEXT chunk has been
// staged ahead (vsom_prefetch_chunk / vsom_stage_next_device beside a running epoch) those buffers hold the next chunk's
// rows while B, lastBMU and the compaction record still describe the current one -- a search would silently mix the two.
// (ahead_rows, not ahead_valid: a staged-ahead chunk that was abandoned for another one has overwritten the rows all the same.)
#define CHECK_ROWS(ctx)                                                \
    do {                                                               \
        if ((ctx)->ahead_rows)                                         \
            return vsom_fail(VSOM_ERR_INVALID,                         \
                             "the next chunk is staged ahead over the current chunk's rows: vsom_commit_chunk first"); \
    } while (0)
// phase 2 runs beside the side stream's work and joins it at its end (a pending sigmaMap is its own business); the
// copy-stream calls touch neither
#define CHECK_CTX_NOJOIN(ctx)                                          \
    do {                                                               \
        if (!(ctx))                                                    \
            return vsom_fail(VSOM_ERR_INVALID, "null context");        \
        hipError_t _e = hipSetDevice((ctx)->device);                   \
        if (_e != hipSuccess)                                          \
            return vsom_fail(VSOM_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(_e)); \
    } while (0)

struct TimerScope {
    vsom_ctx *c; int which; vsom_ctx::Ev ev; bool on;
    TimerScope(vsom_ctx *ctx, int w);
    ~TimerScope();
};

// kernel launchers (each enqueues on ctx->stream and returns a vsom_status) -------------------
// the operands of the context's distance evaluations (vsom_device.hpp; defined in vsom_bmu.hip)
struct DistArgs;
DistArgs vsom_dist_args(const vsom_ctx *c);
// The node groups of a tile walk (vsom_topk.hip, vsom_masked.hip): a workgroup walks G consecutive node tiles, ng groups
// cover the ntiles node tiles.  Enough workgroups to fill the chip (2048: four rounds of two per CU) over the rtiles row
// tiles of a slice, and at most maxg groups (one result per row and group is merged afterwards).
struct VsomNodeGroups {
    size_t G, ng;
};
inline VsomNodeGroups vsom_node_groups(size_t ntiles, size_t rtiles, size_t maxg)
{
    const size_t want = std::min<size_t>({maxg, ntiles, std::max<size_t>(1, (2048 + rtiles - 1) / rtiles)});
    const size_t G = (ntiles + want - 1) / want;
    return {G, (ntiles + G - 1) / G};
}
int launch_stage_chunk(vsom_ctx *c, const float *x_dev, size_t B);
// the chunk buffers sized for B rows (vsom_capi.hip; synchronises and reallocates only when B exceeds the capacity)
int ensure_chunk_capacity(vsom_ctx *c, size_t B);
// the same kernels for the NEXT chunk on the copy stream, beside the running epoch (false: not possible now --
// the caller stages at commit time instead)
bool vsom_can_stage_ahead(const vsom_ctx *c, size_t B);
int launch_stage_chunk_ahead(vsom_ctx *c, const float *x_dev, size_t B);
int vsom_adopt_ahead(vsom_ctx *c);
// pieces of the double-buffered ingest shared with the multi-GPU group (vsom_capi.hip)
int vsom_prefetch_rows(vsom_ctx *c, const float *x_host, size_t B, size_t r0, size_t r1);
int vsom_commit_begin(vsom_ctx *c, float **raw, size_t *B);
int vsom_commit_end(vsom_ctx *c);
int launch_bmu_full(vsom_ctx *c, size_t s0, size_t s1);           // findBmu for samples [s0,s1)
int launch_bmu_local(vsom_ctx *c, size_t s0, size_t s1);          // findLocalBmu
int launch_pair_dist(vsom_ctx *c, const u64 *nodes_dev, const u64 *rows_dev, size_t count,
                     float *out_dev);
int launch_finish(vsom_ctx *c);
// make ctx->stream wait for the side stream's pending work, and materialise a pending sigmaMap: what every entry point
// does first, unless it is one of those that never read sigmaMap (vsom_join_aux_keep)
int vsom_join_aux(vsom_ctx *c);
int vsom_join_aux_keep(vsom_ctx *c); // the join alone
// pending sigmaMap (vsom_update.hip): enqueue its materialisation, if there is one; the caller may have read sigmaMap
int vsom_sigma_flush_pending(vsom_ctx *c);
void vsom_sigma_drop(vsom_ctx *c);   // the next full-range epoch overwrites every row: nothing runs
int launch_bmu_restricted(vsom_ctx *c, u64 min_hits);
int launch_row_dist(vsom_ctx *c, size_t row, float *out_dev);
// vsom_bmd.hip: findRestrictedBmd + draws for chunk rows [r0,r1) (arguments checked by vsom_bmd_batch / vsom_bmd_masked_batch);
// valid_host: null, or the validity bytes of the masked call (one_mask: J bytes for every row); synchronises
int launch_bmd(vsom_ctx *c, u64 min_hits, size_t r0, size_t r1, const double *u_host, uint64_t *draw_out, double *norm_out,
               double *prob_out, const uint8_t *valid_host = nullptr, int one_mask = 0);
// pieces of launch_bmd for callers that lay the scratch out themselves (vsom_generate.hip); they enqueue only.
// P: ppitch x N doubles, node-major, ppitch = vsom_bmd_pitch(rows of the slice); cum: vsom_bmd_chunks(N) x ppitch (written
// only with draws); u_dev, norm_dev, draw_dev: one entry per slice row, draw_dev null = no draws.  vp: the slice's packed
// validity rows (row s - s0 at vp + (s - s0) * xpitch; one: the row every sample shares), null = every column counts.
size_t vsom_bmd_pitch(size_t rows);
size_t vsom_bmd_chunks(size_t N);
int vsom_bmd_enqueue(vsom_ctx *c, u64 min_hits, size_t s0, size_t s1, double *P, size_t ppitch, double *cum,
                     const double *u_dev, double *norm_dev, u64 *draw_dev, const unsigned char *vp = nullptr, bool one = false);
// ndraws draws from the distribution of slice row `row` after a vsom_bmd_enqueue WITH draws: draw_dev[i] from u_dev[i]
int vsom_bmd_enqueue_draws(vsom_ctx *c, const double *P, size_t ppitch, size_t row, const double *cum, const double *norm_dev,
                           const double *u_dev, size_t ndraws, u64 *draw_dev);
// K draws from the distribution of each of the slice's `rows` rows after a vsom_bmd_enqueue WITH draws: draw_dev[r * K + k]
// from u_dev[r * K + k]
int vsom_bmd_enqueue_row_draws(vsom_ctx *c, const double *P, size_t ppitch, size_t rows, size_t K, const double *cum,
                               const double *norm_dev, const double *u_dev, u64 *draw_dev);
// The validity scratch of one slice of a masked distribution, added to a layout (valid_host null: nothing, on = false), and
// slice [s0, s1) of a call over rows from r0: its validity bytes up and packed (a column mask once, with the first slice).
struct VsomBmdMask {
    bool on, one;
    vsom_layout::piece<unsigned char> raw, packed;
};
VsomBmdMask vsom_bmd_mask_add(const vsom_ctx *c, vsom_layout &lay, const uint8_t *valid_host, bool one, size_t slice);
int vsom_bmd_mask_slice_enqueue(vsom_ctx *c, const vsom_layout &lay, const VsomBmdMask &m, size_t r0, size_t s0, size_t s1,
                                const uint8_t *valid_host);
// vsom_generate.hip: draws + decode of chunk rows [r0,r1) (arguments checked by vsom_generate_batch), the decode alone for
// given units (arguments checked by vsom_decode_nodes); both synchronise
int launch_generate(vsom_ctx *c, u64 min_hits, int rule, size_t r0, size_t r1, const double *u_host, const double *l_host,
                    const vsom_generate_out *out);
int launch_decode_nodes(vsom_ctx *c, const uint64_t *nodes_host, size_t count, const double *l_host, double *record_out);
// K draws per row from the row's masked distribution + decode with the observed columns kept (arguments checked by
// vsom_generate_masked_batch); synchronises
int launch_generate_masked(vsom_ctx *c, u64 min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask, size_t K,
                           int keep_observed, const double *u_host, const double *l_host, const vsom_generate_out *out);
// vsom_topk.hip: the k best matching units of chunk rows [r0,r1) (arguments checked by vsom_bmu_topk_batch); synchronises
int launch_topk(vsom_ctx *c, uint32_t k, size_t r0, size_t r1, uint64_t *idx_out, float *dist_out);
// the same over the valid columns and findRestrictedBmu's candidates, with the blended imputation (arguments checked by
// vsom_bmu_topk_masked_batch); synchronises
int launch_topk_masked(vsom_ctx *c, uint32_t k, u64 min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask,
                       const vsom_topk_masked_out *out);
// vsom_similarity.hip: search + scoring of chunk rows [r0,r1) (arguments checked by vsom_similarity_batch); synchronises
int launch_similarity(vsom_ctx *c, u64 min_hits, int num_sigmas, int sigma_rule, size_t r0, size_t r1,
                      const uint8_t *valid_host, const vsom_similarity_out *out);
// vsom_evaluate.hip: search + scoring of chunk rows [r0,r1) and the running mean (arguments checked by vsom_evaluate_batch);
// synchronises
int launch_evaluate(vsom_ctx *c, size_t r0, size_t r1, const float *binary_host, const float *continuous_host,
                    const uint8_t *valid_host, const vsom_evaluate_out *out);
// vsom_masked.hip: the search over valid columns of chunk rows [r0,r1) (arguments checked by vsom_bmu_masked_batch); synchronises
int launch_masked(vsom_ctx *c, u64 min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask,
                  const vsom_masked_out *out);
// pieces of launch_masked for callers that lay the scratch out themselves (vsom_masked_train.hip); they enqueue only.
// pack: rows x J validity bytes as given -> rows x xpitch bytes of 0xFF / 0x00.  search: chunk rows [s0,s1) over the packed
// rows vp (row s - s0 at vp + (s - s0) * xpitch; one: the row every sample shares) with the node groups of
// vsom_masked_groups(rows of the slice); part: (s1 - s0) * grp.ng keys, nan0: s1 - s0 bytes; entry s - s0 of bmu / dist /
// nvalid (device) belongs to row s.  slice_rows: the rows per slice that keep the search scratch within its bound.
void vsom_masked_pack_enqueue(vsom_ctx *c, const unsigned char *raw_dev, size_t rows, unsigned char *packed_dev);
size_t vsom_masked_search_slice_rows(const vsom_ctx *c);
VsomNodeGroups vsom_masked_groups(const vsom_ctx *c, size_t slice);
int vsom_masked_search_enqueue(vsom_ctx *c, u64 min_hits, size_t s0, size_t s1, const unsigned char *vp, bool one,
                               const VsomNodeGroups &grp, u64 *part, unsigned char *nan0, u64 *bmu, float *dist,
                               unsigned *nvalid);
// The same pieces for the callers that keep a slice's units on the device and work on them (the imputed rows of
// launch_masked, the masked scorers): the scratch of one slice of `slice` rows added to a layout -- the validity bytes as
// given and packed, the search's keys and flags, its results -- and slice [s0, s1) of a call over rows from r0: the slice's
// validity bytes up and packed (a column mask once, with the first slice), then the search.  Enqueues only.
struct VsomMaskedSearch {
    bool one;
    size_t slice;
    VsomNodeGroups grp;
    vsom_layout::piece<unsigned char> raw, packed, nan0;
    vsom_layout::piece<u64> part, bmu;
    vsom_layout::piece<float> dist;
    vsom_layout::piece<unsigned> nvalid;
};
VsomMaskedSearch vsom_masked_search_add(const vsom_ctx *c, vsom_layout &lay, bool one, size_t slice);
int vsom_masked_slice_enqueue(vsom_ctx *c, const vsom_layout &lay, const VsomMaskedSearch &ms, u64 min_hits, size_t r0,
                              size_t s0, size_t s1, const uint8_t *valid_host);
// vsom_similarity.hip / vsom_evaluate.hip: the masked search of chunk rows [r0,r1) in slices, each slice scored from its own
// results and packed validity (arguments checked by vsom_similarity_masked_batch / vsom_evaluate_masked_batch); synchronise
int launch_similarity_masked(vsom_ctx *c, u64 min_hits, int num_sigmas, int sigma_rule, size_t r0, size_t r1,
                             const uint8_t *valid_host, int one_mask, const vsom_similarity_masked_out *out);
int launch_evaluate_masked(vsom_ctx *c, u64 min_hits, size_t r0, size_t r1, const float *binary_host,
                           const float *continuous_host, const uint8_t *valid_host, int one_mask,
                           const vsom_evaluate_masked_out *out);
// vsom_masked_train.hip: the batch epoch over valid columns only (arguments checked by vsom_batch_epoch_masked); synchronises
int launch_batch_epoch_masked(vsom_ctx *c, double sigma, int is_first, const uint8_t *valid_host, int one_mask);
// vsom_accum.hip: the accumulated epoch (state and arguments checked by vsom_batch_accum_*); they enqueue only.  begin:
// the accumulators allocated and zeroed; chunk: phase 1, MSE / hits and the carried phase 2 of the loaded chunk (B > 0),
// with the sigma and is_first of c->ac; end: map, sigmaMap, weightMap and the MSE word from the accumulators
// valid_host: the chunk's validity bytes (vsom_batch_accum_chunk_masked) or null (every entry valid)
int launch_accum_begin(vsom_ctx *c);
int launch_accum_chunk(vsom_ctx *c, const uint8_t *valid_host = nullptr, int one_mask = 0);
int launch_accum_end(vsom_ctx *c);
// Pieces of launch_batch_epoch_masked shared with the accumulated epoch (vsom_accum.hip); they enqueue only.
// VsomMaskedScratch: the scratch of a masked chunk of c->B > 0 rows -- the validity bytes as given (vrows x J; one: the
// row every sample shares) and packed (vrows x xpitch), bits[column][row / 32] (J x nwords words), the chunk's dirty
// columns in ascending order (J entries) and their count, and, for the first epoch's tile walk, one search slice's
// node-group keys and flags (first; part, nan0, nvalid as for vsom_masked_search_enqueue; empty otherwise).  scratch_add: its
// members added to a layout.  How the caller's bytes reach `raw` is the caller's.  prepare: raw -> packed -> bits -> dirty
// columns.  phase1: the masked search of the whole chunk straight into lastBMU and sqres -- the tile walk in slices when
// first, findLocalBmu's walk from lastBMU otherwise.
struct VsomMaskedScratch {
    bool one, first;
    size_t vrows, nwords, slice;
    VsomNodeGroups grp;
    vsom_layout::piece<unsigned char> raw, packed, nan0;
    vsom_layout::piece<unsigned> bits, ndirty, nvalid;
    vsom_layout::piece<int> dcols;
    vsom_layout::piece<u64> part;
};
VsomMaskedScratch vsom_masked_scratch_add(const vsom_ctx *c, vsom_layout &lay, bool one, bool first);
void vsom_masked_prepare_enqueue(vsom_ctx *c, const vsom_layout &lay, const VsomMaskedScratch &ms);
int vsom_masked_phase1_enqueue(vsom_ctx *c, const vsom_layout &lay, const VsomMaskedScratch &ms);
// SomIndex(lastBMU[j]) of the chunk's rows into bxy (c->B entries), for the chains of both epoch paths
void vsom_bxy_enqueue(vsom_ctx *c, int2 *bxy);
// node rows padded to whole wavefronts: the pitch of the (c,w) rows and of the masked side state
inline size_t vsom_node_pitch(size_t N) { return (N + 63) / 64 * 64; }
// vsom_accum_masked.hip: the ever-dirty columns of an accumulated epoch (vsom_ctx::acm_*).  ensure: the side buffers and the
// pinned staging for vbytes validity bytes (may synchronise when it allocates).  stage: the caller's bytes through the
// pinned staging into raw_dev.  fold: the chunk's dirty columns into the ever-dirty list, marking the fresh ones.  chains:
// the chunk's rows into the side state of every ever-dirty column (bits null: every entry valid, no fresh column); it
// must run before the carried neighbourhood pass and chains of the chunk touch acc_W / acc_M / acc_S.  end: map and
// sigmaMap of the ever-dirty columns from the side state, after accum_end_kernel.  All but ensure enqueue only.
int vsom_accum_masked_ensure(vsom_ctx *c, size_t vbytes);
int vsom_accum_masked_reset(vsom_ctx *c);
int vsom_accum_masked_stage(vsom_ctx *c, const uint8_t *valid_host, size_t vbytes, unsigned char *raw_dev);
int vsom_accum_masked_fold(vsom_ctx *c, const int *dcols, const unsigned *ndirty);
int vsom_accum_masked_chains(vsom_ctx *c, const int2 *bxy, const unsigned *bits, size_t nwords);
int vsom_accum_masked_end(vsom_ctx *c);
int launch_raw_dist(vsom_ctx *c, const u64 *nodes_dev, const u64 *vrows_dev, size_t count, int from_map,
                    float *out_dev);
// vsom_umatrix.hip: Som::updateUMatrix of the current map / sigmaMap into ctx->umatrix; enqueues only.
// refusal: why vsom_umatrix refuses this context, or null.
const char *vsom_umatrix_refusal(const vsom_ctx *c);
int vsom_umatrix_ensure(vsom_ctx *c);
int launch_umatrix(vsom_ctx *c);
// the one-workgroup-per-map form for ensembles (maps whose model and sigma rows fit LDS): descriptors, LDS need, launch
struct VsomUmDesc {
    const float *map, *sigma;
    double *u, *out;         // the member's device buffer; its slice of the ensemble's pinned results or null
    int ldm, D, P, ppitch, W, H;
};
size_t vsom_umatrix_many_smem(const vsom_ctx *c);
int vsom_umatrix_launch_many(int clr, const VsomUmDesc *desc_dev, unsigned count, size_t smem, hipStream_t s);
// may_defer: the caller is a plain batch epoch (vsom_batch_phase2_async / _epoch_async), whose sigmaMap may stay pending
int launch_phase2(vsom_ctx *c, double sigma, size_t n0, size_t n1, bool may_defer = false);
int ensure_lut(vsom_ctx *c, double sigma);
// column compaction (vsom_compact.hip)
bool vsom_cc_applies(const vsom_ctx *c);
bool vsom_cc_considered(const vsom_ctx *c, size_t B);    // side-effect free: false = vsom_cc_begin does nothing for B rows
int vsom_cc_begin(vsom_ctx *c, size_t B, bool *on);
// live-column record + gathered rows (+ int8 images) of a chunk of B rows, on `stream`, into the given record
int vsom_cc_stage(vsom_ctx *c, size_t B, hipStream_t stream, int *idx, int *inv, unsigned *meta, bool *xi_out);
int vsom_cc_gather_map(vsom_ctx *c);
int vsom_cc_ensure_update_scratch(vsom_ctx *c);
// which rows the expansion writes from the scratch rows (bit 0: map, bit 1: sigmaMap); inv: the live-column record to use
enum VsomExpand { VSOM_EXPAND_MAP = 1, VSOM_EXPAND_SIGMA = 2, VSOM_EXPAND_BOTH = 3 };
int vsom_cc_expand(vsom_ctx *c, size_t n0, size_t nloc, VsomExpand what, const int *inv = nullptr);
// vsom_sl_i8.hip: rows onto the live columns (+ int8 images)
int launch_sl_gather_quant(vsom_ctx *c, size_t B, hipStream_t stream, const int *idx, bool *xi_out);
int vsom_xq_ensure(vsom_ctx *c);                                 // vsom_xq.hip
bool vsom_tiny_applies(const vsom_ctx *c);                        // vsom_tiny.hip
int launch_tiny_epoch(vsom_ctx *c, double sigma, int is_first);   // whole batch epoch, one workgroup

// one workgroup per map forms of the one-launch kernels (vsom_ensemble.hip).  prepare: the member's descriptor into
// `desc` and its kernel instantiation into *group, or *group = -1 when the member's single call would not take the
// one-launch kernel or its LDS need exceeds lds_limit (the member takes its ordinary path)
constexpr int VSOM_ONL_TINY_GROUPS = 12, VSOM_TINY_GROUPS = 3;
// The one-launch online chunk (vsom_online_tiny.hip), plain or over valid entries (`masked`): the same
// 12 groups, a descriptor size per flavour.  fits: the member is loaded, not custom, its single call would take the
// one-launch kernel and its LDS need (+ the static key slots) is within lds_limit -- vsom_online_masked_tiny_applies'
// conditions for the masked flavour.  prepare, for a member that fits: valid_dev = its validity bytes on the device
// (B x J, or J with one_mask), or null for the plain chunk.
bool vsom_onl_tiny_fits(const vsom_ctx *c, double sigma, bool masked, size_t lds_limit);
size_t vsom_onl_tiny_desc_bytes(bool masked);  // (descriptors are packed at exactly this size: the kernels index args[blockIdx.x])
int vsom_onl_tiny_prepare(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk, bool want_lb,
                          const unsigned char *valid_dev, int one_mask, void *desc, int *group, size_t *smem, int *lut_slot);
// before any launch of the call: the kernel's dynamic LDS limit (process-wide per device and kernel, raised only)
int vsom_onl_tiny_ready(bool masked, int group, int device, size_t lds_limit);
int vsom_onl_tiny_launch_many(bool masked, int group, const void *desc_dev, unsigned count, size_t smem, hipStream_t s);
void vsom_onl_tiny_done(vsom_ctx *c, int lut_slot);
// vsom_train_online_chunk_masked for a member of an ensemble (vsom_online.hip): every refusal but that of the membership
int vsom_online_chunk_masked_member(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk,
                                    const uint8_t *valid_host, int one_mask, uint64_t *lastbmu_out, float *mse_out);
size_t vsom_tiny_desc_bytes();       // (descriptors are packed at exactly this size: the kernels index args[blockIdx.x])
int vsom_tiny_prepare(vsom_ctx *c, double sigma, int is_first, size_t lds_limit, void *desc, int *group, size_t *smem);
int vsom_tiny_launch_many(int group, const void *desc_dev, unsigned count, size_t smem, hipStream_t s);

// whole schedules in one launch (vsom_batch_schedule, vsom_ensemble_batch_schedule; vsom_tiny.hip)
void vsom_lut_dims(const vsom_ctx *c, uint32_t *lw, uint32_t *lh);   // the shape of the context's neighbourhood table
// (the round image -- tables, table offsets, validity bytes -- is vsom_sched_round.hpp's)
const char *vsom_schedule_refusal(const vsom_ctx *c);                // why a schedule call refuses this context, or null
// the fast path applies: the single epoch would take the one-launch kernel within lds_limit, and every sigma is finite
bool vsom_tiny_schedule_applies(const vsom_ctx *c, const double *sigma, size_t epochs, size_t lds_limit);
size_t vsom_tiny_sched_desc_bytes();
// the descriptor of `epochs` epochs (first: they start the schedule) reading tables lut_dev + tab_dev[ep] and storing the
// MSE of epoch ep to mse[ep]; returns the kernel instantiation (the transform), *smem = its LDS need
int vsom_tiny_sched_fill(vsom_ctx *c, const float *lut_dev, const unsigned *tab_dev, float *mse, size_t epochs, int first,
                         int reset_bmu, void *desc, size_t *smem);
int vsom_tiny_sched_launch_many(int group, const void *desc_dev, unsigned count, size_t smem, hipStream_t s);
// the contract itself, what every context off the fast path runs: the schedule as the sequence of single epochs,
// epoch(ep) = the flavour's single-epoch call
template <typename Epoch>
int vsom_schedule_loop(vsom_ctx *c, size_t epochs, int reset_bmu, Epoch epoch)
{
    for (size_t ep = 0; ep < epochs; ++ep) {
        if (ep > 0 && reset_bmu && c->B) {
            VSOM_HIP_CHECK(hipSetDevice(c->device));
            VSOM_HIP_CHECK(hipMemsetAsync(c->lastbmu.p, 0, c->B * sizeof(uint64_t), c->stream));
        }
        if (int rc = epoch(ep))
            return rc;
    }
    return VSOM_OK;
}
// The fast path of a single context's schedule, plain or masked: rounds of at most VSOM_SCHEDULE_MAX_EPOCHS epochs, per
// round one image (vsom_sched_round.hpp) copied once and launch(...) = the flavour's descriptor and its kernel on
// c->stream; then the wait and the results.  valid_host non-null: the validity bytes are copied to the device once, before
// the rounds, and handed to every launch as valid_dev.
typedef int (*VsomSchedLaunch)(vsom_ctx *c, const unsigned char *valid_dev, int one_mask, const float *lut_dev,
                               const unsigned *tab_dev, float *mse, size_t epochs, int first, int reset_bmu);
int vsom_schedule_rounds(vsom_ctx *c, const double *sigma, size_t epochs, int reset_bmu, const uint8_t *valid_host,
                         int one_mask, float *mse_out, VsomSchedLaunch launch);
// after the wait behind the launches: sch_mse[0 .. epochs) into mse_out, the last one into the word vsom_get_mse reads
void vsom_schedule_results(vsom_ctx *c, size_t epochs, float *mse_out);

// the same over the valid entries only (vsom_batch_schedule_masked, vsom_ensemble_batch_*_masked; vsom_tiny_masked.hip,
// DESIGN.md section 4t).  A single epoch is a schedule of one epoch whose `first` is the call's is_first.
// why a masked call refuses this context whatever its chunk (custom, CLR, a non-strict update mode), or null
const char *vsom_masked_train_refusal(const vsom_ctx *c);
// the one-workgroup masked kernel applies: vsom_tiny_applies, Standard / Median, not custom, strict, LDS need <= lds_limit
bool vsom_tiny_masked_applies(const vsom_ctx *c, int one_mask, size_t lds_limit);
// ... and every sigma is finite
bool vsom_tiny_masked_schedule_applies(const vsom_ctx *c, int one_mask, const double *sigma, size_t epochs, size_t lds_limit);
size_t vsom_tiny_masked_sched_desc_bytes();
// as vsom_tiny_sched_fill; valid_dev: the validity bytes on the device (B x J, or J with one_mask)
int vsom_tiny_masked_sched_fill(vsom_ctx *c, const unsigned char *valid_dev, int one_mask, size_t lds_limit, const float *lut_dev,
                                const unsigned *tab_dev, float *mse, size_t epochs, int first, int reset_bmu, void *desc,
                                size_t *smem);
int vsom_tiny_masked_sched_launch_many(int group, const void *desc_dev, unsigned count, size_t smem, hipStream_t s);

// custom-transformation contexts (vsom_custom.hip): the entry points that accept one route here, the others refuse it
#define VSOM_CUSTOM_REFUSE(ctx, what)                                  \
    do {                                                               \
        if ((ctx) && (ctx)->cu)                                        \
            return vsom_custom_refuse(what);                           \
    } while (0)
int vsom_custom_refuse(const char *what);
void vsom_custom_destroy(vsom_ctx *c);
int vsom_custom_after_set_state(vsom_ctx *c);
int vsom_custom_upload(vsom_ctx *c, const float *x_host, size_t B, bool wait);
int vsom_custom_prefetch(vsom_ctx *c, const float *x_host, size_t B);
int vsom_custom_commit(vsom_ctx *c);
int vsom_custom_bmu_batch(vsom_ctx *c, int local, uint64_t *idx_out_host, float *dist_out_host);
// (valid_host: the vector's validity bytes for the _valid entry points, null = all valid; the column weights always apply)
int vsom_custom_find(vsom_ctx *c, const float *v_host, const uint8_t *valid_host, int local, uint64_t start, uint64_t *bmu_out,
                     float *dist_out);
int vsom_custom_dist_single(vsom_ctx *c, const float *v_host, const uint8_t *valid_host, uint64_t node, float *dist_out);
int vsom_custom_distances(vsom_ctx *c, const uint64_t *nodes_host, const uint64_t *rows_host, size_t count,
                          float *dist_out_host);
int vsom_custom_batch_epoch_async(vsom_ctx *c, double sigma, int is_first);
int vsom_custom_train_single(vsom_ctx *c, const float *v_host, const uint8_t *valid_host, double eta, double sigma,
                             uint64_t *last_bmu, int decay_fn, float *residual_out, float *dist_out, uint64_t *bmu_out);
// vsom_set_column_weights / vsom_set_chunk_validity and the four _valid calls exist on custom contexts only: the gate of
// those six entry points (a null context, then a built-in one, are VSOM_ERR_INVALID)
#define VSOM_CUSTOM_ONLY(ctx, what)                                    \
    do {                                                               \
        if (!(ctx))                                                    \
            return vsom_fail(VSOM_ERR_INVALID, "null context");        \
        if (!(ctx)->cu)                                                \
            return vsom_custom_only(what);                             \
    } while (0)
int vsom_custom_only(const char *what);
int vsom_custom_set_weights(vsom_ctx *c, const float *weights_host);
int vsom_custom_set_validity(vsom_ctx *c, const uint8_t *valid_host, int one_mask);
int vsom_custom_train_online_chunk(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk);
uint32_t vsom_custom_residual_len(const vsom_ctx *c);
