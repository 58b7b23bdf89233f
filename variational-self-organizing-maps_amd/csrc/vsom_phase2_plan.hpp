// vsom_phase2_plan.hpp -- what one phase 2 (launch_phase2, vsom_update.hip) will do, decided once and before it does anything.
//
// Host only, values only: vsom_phase2_plan reads the context and returns a Phase2Plan; it launches, allocates and changes
// nothing, so tests/phase2_plan_driver.cpp pins every rule below without a device.  launch_phase2 executes the plan and
// decides nothing itself; vsom_batch_phase2_async (vsom_capi.hip) asks it whether the epoch reads the staged rows, and
// vsom_cc_applies (vsom_compact.hip) and vsom_small_map_chains share the small-map threshold through vsom_use_chain.
#pragma once

#include "vsom_internal.hpp"

enum Phase2Path {
    VSOM_P2_EMPTY,       // a chunk of no rows: the map becomes the zero the chains start from
    VSOM_P2_CLR,         // vsom_update_clr_rp8_gfx950: lane = node, 8 parameter pairs per wavefront
    VSOM_P2_SMALL_MAP,   // update_chain3_kernel: lane = (node, dim pair), for maps too small to fill the chip with lane = node
    VSOM_P2_QUADS        // the lane = node column-quad kernels (gen_nt_asm.py): Standard / Median
};

// what turns the chains' output into map / sigmaMap rows afterwards
enum Phase2After {
    VSOM_P2_NOTHING,                // the kernel wrote both itself, or sigmaMap stays pending and the map rows are in place
    VSOM_P2_EXPAND_MAP_AND_SIGMA,   // cc_expand_kernel from the compaction's scratch rows (vsom_compact.hip)
    VSOM_P2_EXPAND_MAP_ONLY,        // ... of a deferred epoch
    VSOM_P2_EXPAND_SIGMA_ONLY,      // ... of its materialisation (vsom_phase2_replay alone)
    VSOM_P2_FINALIZE_COLUMNS        // sigma_finalize_kernel over after_cols columns of every part, left as raw S
};

struct Phase2Plan {
    Phase2Path path = VSOM_P2_EMPTY;
    // geometry: nodes of the range, the same rounded up to 64 (the node pitch of the (c,w) array), node groups of 64, and the
    // float2 elements the (c,w) array needs
    size_t nloc = 0, ldn = 0;
    unsigned gx = 0;
    size_t cw_elems = 0;
    // launch shape of the chain kernel
    unsigned grid_x = 0, grid_y = 0, block = 0;
    // QUADS: on the compaction's live columns?  column quads; workgroups (64 nodes x 8 quads) of the launch; does sigmaMap
    // stay pending (the mean-only chains on the c-only operand array)?  is the rows-free event offered to the stage-ahead?
    bool compact = false, deferred = false, offer_rows_free = false;
    unsigned quads = 0;
    size_t chain_wgs = 0;
    VsomQuadForm form = VSOM_QF_FULL;
    // QUADS and SMALL_MAP: the arithmetic of the chains
    VsomQuadVariant variant = VSOM_QV_STD;
    int pl_log2 = 0;                // SMALL_MAP: log2 of the dim pairs per node row of a workgroup, 3..6
    unsigned nslices = 0;           // CLR: slices of 8 parameter pairs
    bool reads_staged_rows = false; // the chain kernel reads Xs / XP / YP themselves, not the transposed chunk
    Phase2After after = VSOM_P2_NOTHING;
    unsigned after_cols = 0;        // FINALIZE_COLUMNS: how many, per part
};

// lane = node kernels yield this many wavefronts over `nodes` nodes (VSOM_CHAIN_MAX_WAVES, vsom_internal.hpp)
inline size_t vsom_lane_node_waves(const vsom_ctx &c, size_t nodes) { return ((nodes + 63) / 64) * ((c.D + 13) / 14); }

// Maps whose node shard times depth is small (at most VSOM_CHAIN_MAX_WAVES wavefronts, the measured crossover against the
// lane = node kernels) take the small-map chain kernel: C4's 64x64x32 map would give the quad kernels half a wavefront per SIMD.
inline bool vsom_use_chain(const vsom_ctx &c, size_t nloc)
{
    if (!c.use_chain || c.transform == VSOM_CLR)
        return false;
    return vsom_lane_node_waves(c, nloc) <= VSOM_CHAIN_MAX_WAVES;
}

// does a full-range epoch of the quad kernels leave its sigmaMap pending?  (dense rows of a ragged depth stay eager: their last
// quad runs into the rows' padding, which sigma_finalize_kernel re-zeroes in map and sigmaMap at once)
inline bool sigma_defers(const vsom_ctx &c, bool compact)
{
    if (c.sigma_shared || c.in_group || c.sigma_mode == VSOM_SIGMA_EAGER)
        return false;
    if (!compact && c.D % 4 != 0)
        return false;
    return c.sigma_mode == VSOM_SIGMA_LAZY || c.sigma_unread >= 2;
}

// geometry every path shares
inline void vsom_phase2_geometry(Phase2Plan &p, size_t B, size_t nloc)
{
    p.nloc = nloc;
    p.ldn = (nloc + 63) / 64 * 64;
    p.gx = (unsigned)((nloc + 63) / 64);
    // pair rows: ceil(B/2) + what the kernels' staging reads ahead (one block of 16 pair-rows) + slack
    p.cw_elems = ((B + 1) / 2 + 24) * p.ldn * 2;
}

// One launch of a quad kernel of the given form over the plan's nodes: workgroup = 64 nodes x 8 column quads in every form
// (512 threads = one quad per wavefront, 256 = two), grid.x = 8 * column blocks (XCD-aware).  With the compaction the kernel
// runs on the gathered live columns -- their count is a device value it reads from the record, the grid covers cpitch.
inline void vsom_phase2_quad_launch(Phase2Plan &p, const vsom_ctx &c, bool compact, VsomQuadForm form)
{
    p.path = VSOM_P2_QUADS;
    p.compact = compact;
    p.quads = compact ? c.cpitch / 4 : (c.D + 3) / 4;
    p.chain_wgs = (size_t)p.gx * ((p.quads + 7) / 8);
    p.grid_x = 8 * ((p.quads + 7) / 8);
    p.grid_y = (p.gx + 7) / 8;
    p.form = form;
    p.block = form == VSOM_QF_MEAN_TWO_QUADS ? 256 : 512;
}

// n1 > n0 is the caller's precondition; may_defer: the caller is a plain batch epoch, whose sigmaMap may stay pending
inline Phase2Plan vsom_phase2_plan(const vsom_ctx &c, size_t n0, size_t n1, bool may_defer)
{
    Phase2Plan p;
    vsom_phase2_geometry(p, c.B, n1 - n0);
    if (c.B == 0)
        return p;
    if (c.transform == VSOM_CLR) {
        // a ragged last slice runs over the parts' zero padding (part_pitch is a multiple of 32); the kernel leaves raw S
        // in the A part and in the B part
        p.path = VSOM_P2_CLR;
        p.nslices = (c.part_len + 7) / 8;
        p.grid_x = 8 * ((p.nslices + 3) / 4);
        p.grid_y = (p.gx + 7) / 8;
        p.block = 256;
        p.reads_staged_rows = true;
        p.after = VSOM_P2_FINALIZE_COLUMNS;
        p.after_cols = 8 * p.nslices;
        return p;
    }
    // Median's FMAs are exact: one kernel for all update modes
    p.variant = c.transform == VSOM_MEDIAN ? VSOM_QV_MED
                : c.update_mode == VSOM_UPDATE_FMA ? VSOM_QV_FMA
                : c.update_mode == VSOM_UPDATE_FMA_SIGMA ? VSOM_QV_SFMA : VSOM_QV_STD;
    if (vsom_use_chain(c, p.nloc)) {
        // at least 8 dim pairs per node row (lanes past the depth idle); the kernel writes sigmaMap itself
        p.path = VSOM_P2_SMALL_MAP;
        p.pl_log2 = 3;
        while ((2u << p.pl_log2) < c.D && p.pl_log2 < 6)
            ++p.pl_log2;
        const unsigned PL = 1u << p.pl_log2, npairs = (c.D + 1) / 2;
        p.grid_x = (unsigned)((p.nloc + (256 / PL) - 1) / (256 / PL));
        p.grid_y = (npairs + PL - 1) / PL;
        p.block = 256;
        p.reads_staged_rows = true;
        return p;
    }
    const bool compact = c.cc_valid;
    vsom_phase2_quad_launch(p, c, compact, VSOM_QF_FULL);
    // Nothing behind the transposition reads the staged rows of this chunk any more, so the next chunk's staging kernels may
    // overwrite them beside the chains -- where that pays: kernels running beside the chain kernel take slots and clock from
    // it, and measured (tools/exp/ab_stage.py, interleaved A/B, strict, B = 4096 x 784) the step gains 2.7 % / 2.3 % on 48x48 /
    // 64x64 maps (the chain launch leaves slots idle: 1.3 rounds of the 1024 resident workgroups), nothing at 80x80 / 96x96
    // and LOSES 1 % at 112x112 / 128x128 (six full rounds: 0.05 ms of staging kernels cost the chains 0.09 ms).  So the event
    // is offered only when the chain launch is at most two rounds.
    p.offer_rows_free = p.chain_wgs <= 2048;
    const bool full = n0 == 0 && n1 == c.N;
    p.deferred = may_defer && full && sigma_defers(c, compact);
    if (p.deferred) {
        // Two column quads per wavefront (gen_nt_asm.py, K2) where the launch is more than two thirds of a round of 1024
        // workgroups; below, the one-quad form: a small launch leaves SIMDs short of wavefronts, and the two-quad form has
        // half as many, each twice as long.  Measured (B = 4096 x 784 sparse, 21 column blocks, launch time one-quad ->
        // two-quad, profiles/mean_nt8_small_launches.txt): 525 workgroups 0.310 -> 0.344 ms, 672 0.340 -> 0.343 (the step
        // 0.488 -> 0.503), 756 0.590 -> 0.405, 1008 0.592 -> 0.491, 5376 (C3) 2.28 -> 1.86.
        const bool two = !c.mean_nt4 && 3 * p.chain_wgs > 2 * 1024;
        vsom_phase2_quad_launch(p, c, compact, two ? VSOM_QF_MEAN_TWO_QUADS : VSOM_QF_MEAN_ONE_QUAD);
    }
    // compaction: cc_expand_kernel writes the dense scratch rows back; otherwise a last quad of a ragged depth ran into the
    // rows' zero padding and sigma_finalize_kernel re-zeroes it (a deferred dense epoch has no ragged quad and no sigmaMap yet)
    if (compact) {
        p.after = p.deferred ? VSOM_P2_EXPAND_MAP_ONLY : VSOM_P2_EXPAND_MAP_AND_SIGMA;
    } else if (!p.deferred) {
        p.after = VSOM_P2_FINALIZE_COLUMNS;
        p.after_cols = 4 * p.quads;
    }
    return p;
}

// The materialisation of a pending sigmaMap (sigma_materialise, vsom_update.hip) as a plan: the full kernel of the epoch's
// variant over the whole map, on the columns that epoch ran on, for a chunk of B rows; its raw S becomes sigmaMap as in an
// eager epoch, its M goes where the mean-only kernel put the same values.
inline Phase2Plan vsom_phase2_replay(const vsom_ctx &c, size_t B, VsomQuadVariant variant, bool compact)
{
    Phase2Plan p;
    vsom_phase2_geometry(p, B, c.N);
    vsom_phase2_quad_launch(p, c, compact, VSOM_QF_FULL);
    p.variant = variant;
    p.after = compact ? VSOM_P2_EXPAND_SIGMA_ONLY : VSOM_P2_FINALIZE_COLUMNS;
    p.after_cols = compact ? 0 : 4 * p.quads;
    return p;
}
