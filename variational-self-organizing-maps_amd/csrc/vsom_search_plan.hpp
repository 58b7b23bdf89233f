// vsom_search_plan.hpp -- what one findBmu over chunk rows [s0, s1) (launch_bmu_full, vsom_bmu.hip) will do, decided once and
// before it does anything.
//
// Host only, values only: vsom_search_plan and vsom_exact_plan read the context and return a plan; they launch, allocate and
// change nothing and dereference no buffer, so tests/search_plan_driver.cpp pins every rule below without a device -- every
// path computes the same bits, a threshold that moves by one tile fails nowhere else.  The launchers (vsom_bmu.hip,
// vsom_shortlist.hip, vsom_sl_i8.hip) execute a plan and decide nothing themselves.
#pragma once

#include "vsom_internal.hpp"

// tile shapes of the search kernels that the rules below size their grids and buffers by
#define SL_CMAX 2048           // sl_select_kernel: a Standard / Median sample with more candidates goes to the redo list
#define GT 128                 // sl_gemm_kernel: block tile (samples x nodes)
#define GK 32                  //   K chunk
#define RT_S 256               // sl_gemm_i8_ring*_kernel: workgroup tile, samples
#define RT_N 128               //   nodes
#define RING_BYTES 147456      //   dynamic LDS of the ring: max(3 x 40960, 2 x 73728)
#define K64_NB 16              // sl_k64_kernel: node blocks of 32 per workgroup (its 256 threads stage the constants of these 512 nodes)
#define K64_SB 2               //   sample blocks of 32 per wavefront: every model fragment feeds two MFMAs

enum SearchPath {
    VSOM_SEARCH_EXACT,     // bmu_tile_kernel over every row (launch_bmu_full_exact_masked)
    VSOM_SEARCH_SL_CLR,    // CLR: fp32 contraction over derived features, sl_select_kernel<true>
    VSOM_SEARCH_SL_FP32,   // Standard / Median rows too long for the int8 images: sl_gemm_kernel, sl_select_kernel<false>
    VSOM_SEARCH_SL_I8      // Standard / Median: the contraction in integer arithmetic (vsom_sl_i8.hip)
};
// SL_I8: what the contraction leaves for the refinement (the numbering tests/ties.py restates as ring_plan)
enum SlForm {
    VSOM_SLF_G = 0,        // the B x N matrix G and 64-node tile minima
    VSOM_SLF_K64 = 1,      // 16-node tile minima from sl_k64_kernel (at most 64 contracted columns)
    VSOM_SLF_RING = 2      // 16-node tile minima from the G-less ring kernel (big problems of at most 960 contracted columns)
};
enum SlContraction {
    VSOM_SLC_NONE,
    VSOM_SLC_FP32,         // sl_gemm_kernel
    VSOM_SLC_SMALL_TILES,  // sl_gemm_i8_kernel<2, 1> then <2, 3>: 128 x 64 tiles staged through registers, planes 1 and 3
    VSOM_SLC_RING_G,       // sl_gemm_i8_ring_kernel: 256 x 128 tiles through the LDS-DMA ring
    VSOM_SLC_RING_GLESS,   // sl_gemm_i8_ring_gless_kernel
    VSOM_SLC_K64           // sl_k64_kernel
};
enum SlRefine { VSOM_SLR_SELECT, VSOM_SLR_PICK };   // sl_select_kernel (reads G) or sl_pick_kernel<wps> (tile minima only)

struct SearchLaunch {
    unsigned gx = 0, gy = 1, block = 256;
    size_t lds = 0;        // dynamic LDS bytes
};
#define VSOM_PLAN_LAUNCH(K, l, stream, ...) \
    hipLaunchKernelGGL(K, dim3((l).gx, (l).gy), dim3((l).block), (unsigned)(l).lds, stream, __VA_ARGS__)

struct SearchPlan {
    SearchPath path = VSOM_SEARCH_EXACT;
    size_t rows = 0;
    // every shortlist path: pitch of G, tile minima per row, elements of sl_G (0: no G) and sl_tmin
    size_t ldg = 0, ntm = 0, g_elems = 0, tmin_elems = 0;
    // Standard / Median: contract over the compaction's live columns?  contracted columns; the same rounded up to 64 (SL_I8)
    bool compact = false;
    uint32_t kmax = 0, kp8 = 0;
    SlForm form = VSOM_SLF_G;
    SlContraction contraction = VSOM_SLC_NONE;
    // SL_I8: sl_prepare64_kernel / sl_quant_rows64_kernel instead of the general kernels; the G kernels get sl_qfast (the
    // fp32 two-fma epilogue of the uint8 kind needs |A| < 2^24: at most 960 contracted columns, sl_i8_value_fast)
    bool prepare64 = false, quant64 = false, qfast = false;
    // launches: sl_norm_kernel (SL_FP32) or clr_node_feat_kernel (SL_CLR); clr_sample_feat_kernel; the model images; the
    // sample images (of the whole chunk, once per staged chunk); the contraction; the refinement
    SearchLaunch norm, sample_feat, prepare, quant, contract, refine;
    SlRefine refine_kind = VSOM_SLR_SELECT;
    int wps = 0;           // PICK: wavefronts per sample, 1 / 4 / 2
    // what the refinement is given: the factors of the approximation's and the exact evaluation's share of the threshold,
    // CLR's residual term, the slack in digits of the integer contraction, the candidates (tiles for PICK) past which a sample
    // goes to the redo list
    float thr_approx = 0.f, thr_exact = 0.f, thr_e1 = 0.f, digit_slack = 0.f;
    unsigned cand_cap = 0;
    // SL_CLR: pitch of the feature rows and of their pair part, elements of sl_fs / sl_fm (the refinement's x' / y' rows are
    // refine.lds bytes)
    uint32_t Kp = 0, P32 = 0;
    size_t fs_elems = 0, fm_elems = 0;
    bool fb_xflag = false; // the redo list's feedback carries the chunk's data-kind word
    bool ring() const { return contraction == VSOM_SLC_RING_G || contraction == VSOM_SLC_RING_GLESS; }
};

struct ExactPlan {
    int ntn = 0, TS = 0, nts = 0, gy = 0;   // node tiles, samples per tile, sample tiles, grid.y
    size_t partial_elems = 0;
    bool dedupe = false;   // the three passes that leave representatives of duplicate rows only (launch_bmu_dedupe)
    bool clr = false, list = false;         // bmu_tile_kernel<clr, clr ? 2 : 4, list>
};

// the executors.  launch_bmu_full (vsom_bmu.hip) plans and hands the plan on; the redo list of a shortlist search goes through
// launch_bmu_full_exact_list with the feedback words to write (vsom_digits.hpp)
struct SlFeedback;
int launch_bmu_full_exact_list(vsom_ctx *c, size_t s0, size_t s1, const int *slist, const unsigned *scount, const SlFeedback *fb);
int launch_bmu_full_shortlist(vsom_ctx *c, size_t s0, size_t s1, const SearchPlan &p);       // vsom_shortlist.hip: SL_FP32, SL_I8
int launch_bmu_full_shortlist_clr(vsom_ctx *c, size_t s0, size_t s1, const SearchPlan &p);   //   SL_CLR
// vsom_sl_i8.hip: the int8 images and G / the tile minima of an SL_I8 plan; scal = the counter set THIS search's refinement
// and feedback read (the two sets alternate, vsom_shortlist.hip), already reset
int launch_sl_i8(vsom_ctx *c, size_t s0, size_t s1, const SearchPlan &p, unsigned *scal, unsigned *xflag);
// the dynamic LDS limit of the plan's ring kernel raised to RING_BYTES (the attribute is per DEVICE -- a group drives several
// from one process -- so it is raised on every search that takes a ring kernel, as launch_phase2 does); false: it cannot be
bool sl_i8_raise_ring_lds(SlContraction ring);

inline size_t vsom_ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// AUTO: the MFMA shortlist pays once the map is large enough to fill the matrix pipes and the vectors are long enough for the
// contraction to outweigh writing and re-reading the B x N approximation matrix (measured on 64x64 maps, B = 16384: D = 32
// exact 0.22 vs 0.36 ms, D = 64 0.34 vs 0.39, D = 128 0.61 vs 0.47).  Rows of at most 64 values (Standard / Median): the
// contraction keeps tile minima only, nothing of size B x N is written (sl_k64_kernel) -- it beats the exact kernel once
// that has ~0.1 ms of work (C4, 16384 x 4096 x 32: exact 0.21 ms).
inline bool vsom_search_auto_shortlist(const vsom_ctx &c, size_t rows)
{
    const bool short_rows = c.transform != VSOM_CLR && c.D <= 64 && c.D >= 16 && (double)rows * (double)c.N * (double)c.D >= 1.0e9;
    return c.N >= 1024 && rows >= 64 && (c.D > 64 || short_rows);
}

// Feedback of the previous shortlist search (redo samples, rows, sequence number: pinned words the device writes, possibly
// one call stale): when more than a quarter of the samples had to be redone exactly the shortlist does not pay on this map.
// A failed probe costs a fraction of the exact search it falls back to (Standard C3: 0.35 of 2.9 ms; CLR: a collapsed map is
// recognised on the device before the contraction runs, vsom_shortlist.hip) and a wrongly skipped one several times its own
// cost, and every chunk rebuilds the map from zero (Som.cpp:843,870) -- one bad map says little about the next: no pause
// after a first failure, 4 searches after a second in a row, doubling up to 32.  Returns whether this search skips the shortlist.
inline bool vsom_sl_backoff_step(int &skip, int &fail_streak, unsigned &seq_seen, unsigned redo, unsigned rows, unsigned seq)
{
    if (seq != seq_seen) {             // the verdict of a shortlist search not looked at yet
        seq_seen = seq;
        if (rows > 0 && redo * 4u > rows) {
            skip = fail_streak == 0 ? 0 : (2 << (fail_streak < 4 ? fail_streak : 4));
            ++fail_streak;
        } else {
            fail_streak = 0;
        }
    }
    if (skip <= 0)
        return false;
    --skip;
    return true;
}

// sl_quant_rows64_kernel writes the sample images of rows of 64 bytes, 16 rows per workgroup; sl_quant_rows_kernel any, one
// row per workgroup.  The compaction's gather pass (launch_sl_gather_quant) asks too.
inline bool vsom_sl_quant64(uint32_t kp8) { return kp8 == 64; }
inline unsigned vsom_sl_quant_grid(bool quant64, size_t B) { return (unsigned)(quant64 ? (B + 15) / 16 : B); }

// backoff_skips: what vsom_sl_backoff_step said (consulted only where AUTO's size rule wants the shortlist); ring_lds_ok: the
// ring kernels' dynamic LDS limit can be raised on this device (the executor plans with true, raises it if the plan asks
// for a ring kernel and plans again with false if that fails: the register-staged tiles with G)
inline SearchPlan vsom_search_plan(const vsom_ctx &c, size_t s0, size_t s1, bool backoff_skips, bool ring_lds_ok)
{
    SearchPlan p;
    if (s1 <= s0)
        return p;
    const size_t rows = p.rows = s1 - s0;
    const bool want = c.bmu_mode == VSOM_BMU_SHORTLIST ||
                      (c.bmu_mode == VSOM_BMU_AUTO && vsom_search_auto_shortlist(c, rows) && !backoff_skips);
    if (!want)
        return p;
    // CLR: the select kernel keeps the sample's x' / y' rows in LDS (2 * part_pitch floats beside 8.3 KB of static storage);
    // beyond 48 KB (part_pitch > 6144: J > 111) the exact-order kernel searches instead
    const size_t xy_bytes = (size_t)2 * c.part_pitch * sizeof(float);
    if (c.transform == VSOM_CLR && xy_bytes > 48 * 1024)
        return p;
    const double u = 5.9604644775390625e-08;   // 2^-24
    const size_t ldg = vsom_ceil_div(c.N, 128) * 128, gtiles = vsom_ceil_div(c.N, GT) * 2;
    p.refine.gx = (unsigned)rows;
    if (c.transform == VSOM_CLR) {
        p.path = VSOM_SEARCH_SL_CLR;
        p.refine.lds = xy_bytes;
        const uint32_t P = c.part_len, J = c.J;
        p.P32 = (P + 31) / 32 * 32;
        p.Kp = p.P32 + (3 * J + 31) / 32 * 32;
        p.fs_elems = c.B * (size_t)p.Kp;
        p.fm_elems = (size_t)c.N * p.Kp;
        p.norm.gx = c.N;
        p.sample_feat.gx = (unsigned)rows;
        // the bound: vsom_shortlist.hip, "CLR shortlist"
        const double g1 = ((double)GK + (double)p.Kp / GK + 3.0) * u, gf = ((double)J + 3.0) * u;
        const double ga = 3.01 * (g1 + gf) + ((double)P / 256.0 + 12.0 + 7.0) * u;   // + the final nB - 2*dot rounding
        const double g2 = ((double)P / 8.0 + 10.0) * u, e1 = 6.1 * 1.7320508075688773 * u;
        p.thr_approx = (float)(1.0001 * ga), p.thr_exact = (float)(1.0001 * g2), p.thr_e1 = (float)(1.0001 * e1);
        p.cand_cap = 128u;
    } else {
        // the contraction in exact integer arithmetic on the int8 matrix pipe: one digit per sample value for chunks of small
        // non-negative integers (MNIST pixels), three for any other data -- which of the two is a device-side fact of the
        // staged chunk that the kernels read; nothing is decided here
        const bool i8 = c.xpitch <= 4096;
        p.path = i8 ? VSOM_SEARCH_SL_I8 : VSOM_SEARCH_SL_FP32;
        // columns that are zero in every row of the chunk add exactly 0 to every <x, M>: contract over the live ones (norms,
        // bound and refinement keep the whole rows)
        p.compact = c.cc_valid;
        p.kmax = p.compact ? c.cpitch : c.xpitch;
        const double g1 = ((double)GK + (double)c.xpitch / GK + 3.0) * u, g2 = ((double)c.D / 8.0 + 10.0) * u;
        // integer contraction: |G - (|M|^2 - 2<x,M>)| <= 2 (e_s L1Mmax + l1eff_s eps_max) + 5.1u (nMmax + |x|^2) + 2^-7 eps_max
        // (vsom_sl_i8.hip; 3.1u with the fp64 epilogue, 5.1u with the two-rounding fp32 one of the uint8 kind)
        p.thr_approx = (float)(i8 ? 5.5 * u : 2.0 * g1), p.thr_exact = (float)(2.1 * g2);
        p.digit_slack = i8 ? 2.0f : 0.f;
        p.cand_cap = SL_CMAX;
        p.fb_xflag = i8;
        p.norm.gx = (unsigned)vsom_ceil_div((size_t)c.N * 16, 256);
    }
    p.contraction = VSOM_SLC_FP32;
    p.contract.gx = (unsigned)vsom_ceil_div(c.N, GT), p.contract.gy = (unsigned)vsom_ceil_div(rows, GT);
    if (p.path == VSOM_SEARCH_SL_I8) {
        p.kp8 = (p.kmax + 63) / 64 * 64;
        p.prepare64 = p.kp8 == 64 && c.part_pitch <= 64;
        p.prepare.gx = (unsigned)vsom_ceil_div(c.N, p.prepare64 ? 16 : 4);
        p.quant64 = vsom_sl_quant64(p.kp8);
        p.quant.gx = vsom_sl_quant_grid(p.quant64, c.B);
        p.qfast = p.kp8 <= 960;
        // big maps and chunks: 256 x 128 tiles through the LDS-DMA ring -- without G where the fast epilogue applies; otherwise
        // (few tiles: they would not fill the chip) 128 x 64 tiles staged through registers
        const size_t big_y = vsom_ceil_div(rows, RT_S), big_tiles = vsom_ceil_div(c.N, RT_N) * big_y;
        if (p.kp8 == 64) {
            p.form = VSOM_SLF_K64, p.contraction = VSOM_SLC_K64;
            p.contract.gx = (unsigned)vsom_ceil_div(c.N, K64_NB * 32), p.contract.gy = (unsigned)vsom_ceil_div(rows, 128 * K64_SB);
        } else if (ring_lds_ok && p.qfast && big_tiles >= 256) {
            p.form = VSOM_SLF_RING, p.contraction = VSOM_SLC_RING_GLESS;
            p.contract = {(unsigned)vsom_ceil_div(c.N, RT_N), (unsigned)big_y, 512, RING_BYTES};
        } else if (ring_lds_ok && big_tiles >= 1024) {
            p.contraction = VSOM_SLC_RING_G;
            p.contract = {(unsigned)(gtiles / 2), (unsigned)big_y, 512, RING_BYTES};
        } else {
            p.contraction = VSOM_SLC_SMALL_TILES;    // (the last of the 64-node tiles may lie past N: minima +inf)
            p.contract.gx = (unsigned)gtiles, p.contract.gy = (unsigned)vsom_ceil_div(rows, 128);
        }
    }
    const bool gless = p.form != VSOM_SLF_G;
    p.ldg = ldg;
    p.ntm = gless ? vsom_ceil_div(c.N, 32) * 2 : gtiles;
    p.g_elems = gless ? 0 : rows * ldg;
    p.tmin_elems = rows * p.ntm;
    if (gless) {
        // rows of at most 64 values: a wavefront per sample; few samples (a rank's share of a chunk): a workgroup per sample
        // (0.109 -> 0.089 ms at 512); otherwise two wavefronts
        p.refine_kind = VSOM_SLR_PICK;
        p.wps = c.D <= 64 ? 1 : rows < 4096 ? 4 : 2;
        p.refine.gx = (unsigned)(p.wps == 1 ? vsom_ceil_div(rows, 4) : p.wps == 4 ? rows : vsom_ceil_div(rows, 2));
        p.cand_cap = 64u;
    }
    return p;
}

inline ExactPlan vsom_exact_plan(const vsom_ctx &c, size_t s0, size_t s1, bool list, bool restricted)
{
    ExactPlan e;
    e.clr = c.transform == VSOM_CLR;
    e.list = list;
    e.ntn = (int)vsom_ceil_div(c.N, TILE);
    e.TS = e.clr ? 32 : TILE;
    e.nts = (int)vsom_ceil_div(s1 - s0, e.TS);
    // (a redo list is usually empty or short: ~512 workgroups -- the two per CU the kernel's registers allow -- each
    // walking on through the list's tiles; 768 for CLR measured slower: a second, half-empty round)
    e.gy = list ? std::min(e.nts, std::max(1, 512 / e.ntn)) : e.nts;
    e.partial_elems = (size_t)e.ntn * c.Bcap;
    // Representatives of the duplicate rows only -- where the search is large enough to repay three passes over the map
    // (C3's size: hash 15 + twins 5 + list 17 us): 2e10 (sample, node, value) triples = ~0.5 ms of this kernel
    // (vsom_set_row_dedupe moves the threshold; 0 = always).  With a redo list the passes look at its device-side length
    // first and leave when it is short.  Not for restricted searches: bit-identical rows may differ in their hit counts.
    const double work = (double)(s1 - s0) * (double)c.N * (double)c.D;
    e.dedupe = !restricted && c.N >= 256 && c.dedupe && c.dd_min_work >= 0 && work >= c.dd_min_work;
    // A redo list is usually empty or a handful of non-finite samples (C3: always empty), and then even three launches
    // that look at its length and leave are ~8 us of a step for nothing.  Whole-chunk redo lists are what the CLR
    // shortlist produces when it recognises a collapsed map on the device (vsom_shortlist.hip, sl_clr_degenerate): the
    // passes are enqueued behind CLR searches (8 us of a 5.4 ms step when the list is short) and, for the other
    // transformations, only when vsom_set_row_dedupe(ctx, 0) asks for them always.  (A hint from the previous search's
    // feedback words was tried: the host enqueues whole steps ahead of the device, the words are stale when it matters.)
    if (list && c.dd_min_work > 0 && !e.clr)
        e.dedupe = false;
    return e;
}
