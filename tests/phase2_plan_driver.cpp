// Host-only driver for csrc/vsom_phase2_plan.hpp (tests/test_phase2_plan.py): contexts filled by hand, buffers left null,
// and what vsom_phase2_plan decides for each compared with literals worked out from the rules by hand -- never with a
// second call of the code under test.  No device is touched.
#include "vsom_phase2_plan.hpp"

#include <cstdio>

static long g_errors = 0;
static const char *g_case = "";

#define EXPECT(cond)                                                                    \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("%s:%d: [%s] expected %s\n", __FILE__, __LINE__, g_case, #cond); \
            ++g_errors;                                                                 \
        }                                                                               \
    } while (0)

static uint32_t up32(uint32_t v) { return (v + 31) / 32 * 32; }

// a W x H map of depth J (CLR: J inputs, J(J-1)/2 parameter pairs in each of two parts) holding a chunk of B rows;
// LAZY, no compaction
static void shape(vsom_ctx &c, uint32_t W, uint32_t H, uint32_t J, size_t B, int transform = VSOM_STANDARD)
{
    c.W = W, c.H = H, c.N = W * H, c.J = J, c.transform = transform;
    c.nparts = transform == VSOM_CLR ? 2 : 1;
    c.part_len = transform == VSOM_CLR ? J * (J - 1) / 2 : J;
    c.D = c.nparts * c.part_len;
    c.part_pitch = up32(c.part_len);
    c.pitch = c.nparts * c.part_pitch;
    c.xpitch = up32(J);
    c.B = B;
    c.chunk_loaded = true;
    c.sigma_mode = VSOM_SIGMA_LAZY;
}

static Phase2Plan whole(const vsom_ctx &c, bool may_defer = true) { return vsom_phase2_plan(c, 0, c.N, may_defer); }

int main()
{
    {
        g_case = "128x128 x 784, B = 4096";
        vsom_ctx c;
        shape(c, 128, 128, 784, 4096);
        Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.nloc == 16384 && p.ldn == 16384 && p.gx == 256);
        EXPECT(!p.compact && p.quads == 196 && p.chain_wgs == 6400 && !p.offer_rows_free);
        EXPECT(p.deferred && p.form == VSOM_QF_MEAN_TWO_QUADS && p.variant == VSOM_QV_STD);
        EXPECT(p.grid_x == 200 && p.grid_y == 32 && p.block == 256);
        EXPECT(p.after == VSOM_P2_NOTHING && !p.reads_staged_rows);
        EXPECT(p.cw_elems == 67895296);

        g_case = "same, range [0, 8192)";
        p = vsom_phase2_plan(c, 0, 8192, true);
        EXPECT(p.path == VSOM_P2_QUADS && !p.deferred && p.form == VSOM_QF_FULL && p.block == 512);
        EXPECT(p.nloc == 8192 && p.ldn == 8192 && p.gx == 128 && p.grid_x == 200 && p.grid_y == 16 && p.chain_wgs == 3200);
        EXPECT(p.after == VSOM_P2_FINALIZE_COLUMNS && p.after_cols == 784);

        g_case = "same, compacted to a pitch of 800";
        c.cc_valid = true, c.cpitch = 800;
        p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.compact && p.quads == 200 && p.chain_wgs == 6400);
        EXPECT(p.grid_x == 200 && p.grid_y == 32 && p.deferred && p.form == VSOM_QF_MEAN_TWO_QUADS && p.block == 256);
        EXPECT(p.after == VSOM_P2_EXPAND_MAP_ONLY);
        g_case = "same, compacted, range [0, 8192)";
        p = vsom_phase2_plan(c, 0, 8192, true);
        EXPECT(!p.deferred && p.form == VSOM_QF_FULL && p.block == 512 && p.grid_x == 200 && p.grid_y == 16);
        EXPECT(p.after == VSOM_P2_EXPAND_MAP_AND_SIGMA && p.chain_wgs == 3200);
        g_case = "same, compacted, range [8192, 16384)";
        p = vsom_phase2_plan(c, 8192, 16384, true);
        EXPECT(!p.deferred && p.after == VSOM_P2_EXPAND_MAP_AND_SIGMA);
        c.cc_valid = false;

        g_case = "same, AUTO";
        c.sigma_mode = VSOM_SIGMA_AUTO;
        c.sigma_unread = 1;
        p = whole(c);
        EXPECT(!p.deferred && p.form == VSOM_QF_FULL && p.block == 512 && p.after == VSOM_P2_FINALIZE_COLUMNS);
        c.sigma_unread = 2;
        EXPECT(whole(c).deferred);
        EXPECT(!whole(c, false).deferred && whole(c, false).form == VSOM_QF_FULL);
    }
    {
        g_case = "64x64 x 32, Median, B = 16384";
        vsom_ctx c;
        shape(c, 64, 64, 32, 16384, VSOM_MEDIAN);
        const Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_SMALL_MAP && p.pl_log2 == 4 && p.grid_x == 256 && p.grid_y == 1 && p.block == 256);
        EXPECT(p.reads_staged_rows && !p.deferred && p.after == VSOM_P2_NOTHING && p.variant == VSOM_QV_MED);
        EXPECT(p.nloc == 4096 && p.ldn == 4096 && p.gx == 64 && p.cw_elems == (size_t)(8192 + 24) * 4096 * 2);
    }
    {
        g_case = "4096 x 98";
        vsom_ctx c;
        shape(c, 64, 64, 98, 4096);
        Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_SMALL_MAP && p.pl_log2 == 6 && p.grid_x == 1024 && p.grid_y == 1 && p.reads_staged_rows);
        EXPECT(!p.deferred && p.variant == VSOM_QV_STD);
        g_case = "4096 x 98, use_chain off";
        c.use_chain = false;
        p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && !p.reads_staged_rows && p.quads == 25);
    }
    {
        g_case = "4096 x 99";
        vsom_ctx c;
        shape(c, 64, 64, 99, 4096);
        Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.quads == 25 && p.chain_wgs == 256 && p.offer_rows_free && !p.reads_staged_rows);
        EXPECT(!p.deferred && p.form == VSOM_QF_FULL && p.block == 512 && p.grid_x == 32 && p.grid_y == 8);
        EXPECT(p.after == VSOM_P2_FINALIZE_COLUMNS && p.after_cols == 100);
        g_case = "4096 x 100";
        shape(c, 64, 64, 100, 4096);
        p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.quads == 25 && p.chain_wgs == 256 && p.offer_rows_free);
        EXPECT(p.deferred && p.form == VSOM_QF_MEAN_ONE_QUAD && p.block == 512 && p.grid_x == 32 && p.grid_y == 8);
        EXPECT(p.after == VSOM_P2_NOTHING);
    }
    {
        g_case = "41x39 x 784";
        vsom_ctx c;
        shape(c, 41, 39, 784, 4096);
        const Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.nloc == 1599 && p.ldn == 1600 && p.gx == 25 && p.chain_wgs == 625);
        EXPECT(p.deferred && p.form == VSOM_QF_MEAN_ONE_QUAD && p.block == 512 && p.grid_x == 200 && p.grid_y == 4);
    }
    {
        g_case = "1984 x 704";
        vsom_ctx c;
        shape(c, 62, 32, 704, 4096);
        const Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.chain_wgs == 682 && p.deferred && p.form == VSOM_QF_MEAN_ONE_QUAD && p.block == 512);
    }
    {
        g_case = "43712 x 32";
        vsom_ctx c;
        shape(c, 683, 64, 32, 4096);
        Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.chain_wgs == 683 && p.deferred && p.form == VSOM_QF_MEAN_TWO_QUADS && p.block == 256);
        EXPECT(p.grid_x == 8 && p.grid_y == 86);
        g_case = "43712 x 32, mean_nt4";
        c.mean_nt4 = true;
        p = whole(c);
        EXPECT(p.deferred && p.form == VSOM_QF_MEAN_ONE_QUAD && p.block == 512 && p.grid_x == 8 && p.grid_y == 86);
    }
    {
        g_case = "5184 x 784";
        vsom_ctx c;
        shape(c, 72, 72, 784, 4096);
        Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.chain_wgs == 2025 && p.offer_rows_free);
        g_case = "5248 x 784";
        shape(c, 82, 64, 784, 4096);
        p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.chain_wgs == 2050 && !p.offer_rows_free);
        g_case = "131072 x 32 and 131136 x 32: exactly two rounds, and one workgroup more";
        shape(c, 2048, 64, 32, 4096);
        p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.chain_wgs == 2048 && p.offer_rows_free && p.grid_x == 8 && p.grid_y == 256);
        shape(c, 2049, 64, 32, 4096);
        p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.chain_wgs == 2049 && !p.offer_rows_free && p.grid_y == 257);
    }
    {
        g_case = "45x45 x 794, dense";
        vsom_ctx c;
        shape(c, 45, 45, 794, 4096);
        Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && !p.deferred && p.form == VSOM_QF_FULL && p.block == 512);
        EXPECT(p.after == VSOM_P2_FINALIZE_COLUMNS && p.after_cols == 796);
        g_case = "45x45 x 794, compacted to a pitch of 800";
        c.cc_valid = true, c.cpitch = 800;
        p = whole(c);
        EXPECT(p.deferred && p.chain_wgs == 800 && p.form == VSOM_QF_MEAN_TWO_QUADS && p.block == 256);
        EXPECT(p.after == VSOM_P2_EXPAND_MAP_ONLY);
    }
    {
        g_case = "80x80 x 784, compacted to a pitch of 800";
        vsom_ctx c;
        shape(c, 80, 80, 784, 4096);
        c.cc_valid = true, c.cpitch = 800;
        Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_QUADS && p.chain_wgs == 2500 && p.deferred && p.after == VSOM_P2_EXPAND_MAP_ONLY);
        g_case = "same, sigma_shared";
        c.sigma_shared = true;
        p = whole(c);
        EXPECT(!p.deferred && p.form == VSOM_QF_FULL && p.block == 512 && p.after == VSOM_P2_EXPAND_MAP_AND_SIGMA);
        c.sigma_shared = false;
        g_case = "same, in_group";
        c.in_group = true;
        p = whole(c);
        EXPECT(!p.deferred && p.form == VSOM_QF_FULL && p.after == VSOM_P2_EXPAND_MAP_AND_SIGMA);
        c.in_group = false;
        g_case = "same, EAGER";
        c.sigma_mode = VSOM_SIGMA_EAGER;
        p = whole(c);
        EXPECT(!p.deferred && p.form == VSOM_QF_FULL && p.after == VSOM_P2_EXPAND_MAP_AND_SIGMA);
        c.sigma_mode = VSOM_SIGMA_LAZY;
        EXPECT(whole(c).deferred);

        g_case = "the kernel's variant";
        c.update_mode = VSOM_UPDATE_FMA;
        EXPECT(whole(c).variant == VSOM_QV_FMA);
        c.update_mode = VSOM_UPDATE_FMA_SIGMA;
        EXPECT(whole(c).variant == VSOM_QV_SFMA);
        c.update_mode = VSOM_UPDATE_STRICT;
        EXPECT(whole(c).variant == VSOM_QV_STD);
        c.transform = VSOM_MEDIAN;
        for (int mode : {VSOM_UPDATE_STRICT, VSOM_UPDATE_FMA, VSOM_UPDATE_FMA_SIGMA}) {
            c.update_mode = mode;
            EXPECT(whole(c).variant == VSOM_QV_MED && whole(c).path == VSOM_P2_QUADS);
        }

        // the materialisation of that epoch's sigmaMap: the full kernel over the same columns, sigmaMap rows alone expanded
        g_case = "replay, compacted";
        p = vsom_phase2_replay(c, 4096, VSOM_QV_MED, true);
        EXPECT(p.path == VSOM_P2_QUADS && p.form == VSOM_QF_FULL && p.variant == VSOM_QV_MED && p.block == 512 && p.compact);
        EXPECT(p.nloc == 6400 && p.ldn == 6400 && p.quads == 200 && p.grid_x == 200 && p.grid_y == 13 && !p.deferred);
        EXPECT(p.after == VSOM_P2_EXPAND_SIGMA_ONLY);
        g_case = "replay, dense";
        p = vsom_phase2_replay(c, 4096, VSOM_QV_SFMA, false);
        EXPECT(p.form == VSOM_QF_FULL && p.variant == VSOM_QV_SFMA && p.block == 512 && !p.compact && p.quads == 196);
        EXPECT(p.grid_x == 200 && p.grid_y == 13 && p.after == VSOM_P2_FINALIZE_COLUMNS && p.after_cols == 784);
    }
    {
        g_case = "32x32 CLR, J = 64, B = 8192";
        vsom_ctx c;
        shape(c, 32, 32, 64, 8192, VSOM_CLR);
        Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_CLR && p.nslices == 252 && p.grid_x == 504 && p.grid_y == 2 && p.block == 256);
        EXPECT(p.after == VSOM_P2_FINALIZE_COLUMNS && p.after_cols == 2016 && p.reads_staged_rows && !p.deferred);
        EXPECT(p.nloc == 1024 && p.ldn == 1024 && p.gx == 16 && p.cw_elems == (size_t)(4096 + 24) * 1024 * 2);
        g_case = "CLR, use_chain off, AUTO with two unread epochs";
        c.use_chain = false, c.sigma_mode = VSOM_SIGMA_AUTO, c.sigma_unread = 5;
        p = whole(c);
        EXPECT(p.path == VSOM_P2_CLR && !p.deferred && p.reads_staged_rows);
    }
    {
        g_case = "empty chunks";
        vsom_ctx c;
        shape(c, 128, 128, 784, 0);
        Phase2Plan p = whole(c);
        EXPECT(p.path == VSOM_P2_EMPTY && !p.deferred && !p.reads_staged_rows && p.after == VSOM_P2_NOTHING && !p.offer_rows_free);
        shape(c, 64, 64, 32, 0, VSOM_MEDIAN);
        p = whole(c);
        EXPECT(p.path == VSOM_P2_EMPTY && !p.deferred && !p.reads_staged_rows && p.after == VSOM_P2_NOTHING);
        shape(c, 32, 32, 64, 0, VSOM_CLR);
        p = vsom_phase2_plan(c, 0, 512, true);
        EXPECT(p.path == VSOM_P2_EMPTY && !p.deferred && !p.reads_staged_rows && p.after == VSOM_P2_NOTHING);
    }
    {
        // the predicate vsom_small_map_chains and vsom_cc_applies answer through: 64 x 7 = 448 wavefronts against 64 x 8
        g_case = "vsom_use_chain";
        vsom_ctx c;
        shape(c, 64, 64, 98, 4096);
        EXPECT(vsom_use_chain(c, 4096) && !vsom_use_chain(c, 4097) && vsom_lane_node_waves(c, 4096) == 448);
        shape(c, 64, 64, 99, 4096);
        EXPECT(!vsom_use_chain(c, 4096) && vsom_use_chain(c, 3584) && vsom_lane_node_waves(c, 4096) == 512);
        shape(c, 32, 32, 8, 4096, VSOM_CLR);
        EXPECT(!vsom_use_chain(c, 1024));
    }
    if (g_errors) {
        std::printf("%ld failure(s)\n", g_errors);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
