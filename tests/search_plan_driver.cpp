// Host-only driver for csrc/vsom_search_plan.hpp (tests/test_search_plan.py): contexts filled by hand, buffers left null,
// and what vsom_search_plan, vsom_exact_plan and vsom_sl_backoff_step decide for each compared with literals worked out
// from the rules by hand -- never with a second call of the code under test.  No device is touched.
#include "vsom_search_plan.hpp"

#include <cmath>
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
// AUTO, no compaction
static void shape(vsom_ctx &c, uint32_t W, uint32_t H, uint32_t J, size_t B, int transform = VSOM_STANDARD)
{
    c.W = W, c.H = H, c.N = W * H, c.J = J, c.transform = transform;
    c.nparts = transform == VSOM_CLR ? 2 : 1;
    c.part_len = transform == VSOM_CLR ? J * (J - 1) / 2 : J;
    c.D = c.nparts * c.part_len;
    c.part_pitch = up32(c.part_len);
    c.pitch = c.nparts * c.part_pitch;
    c.xpitch = up32(J);
    c.B = c.Bcap = B;
    c.chunk_loaded = true;
}

// the first `rows` rows of the chunk; no back-off, the ring kernels' LDS available
static SearchPlan rows_of(const vsom_ctx &c, size_t rows, bool skips = false, bool ring_lds_ok = true)
{
    return vsom_search_plan(c, 0, rows, skips, ring_lds_ok);
}

// a threshold factor in units of u = 2^-24 (a float rounded from a double product: compared to a few float ulps)
static bool units(float got, double want_u) { return std::fabs((double)got - want_u * 0x1p-24) <= 1e-6 * want_u * 0x1p-24; }

static bool launch(const SearchLaunch &l, unsigned gx, unsigned gy, unsigned block, size_t lds = 0)
{
    return l.gx == gx && l.gy == gy && l.block == block && l.lds == lds;
}

// how many searches in a row skip the shortlist once the feedback words read (redo, rows, seq)
static int skipped(int &skip, int &streak, unsigned &seen, unsigned redo, unsigned rows, unsigned seq)
{
    int n = 0;
    while (n < 1000 && vsom_sl_backoff_step(skip, streak, seen, redo, rows, seq))
        ++n;
    return n;
}

int main()
{
    {
        g_case = "AUTO: nodes 1023 / 1024";
        vsom_ctx c;
        shape(c, 33, 31, 784, 4096);
        EXPECT(rows_of(c, 4096).path == VSOM_SEARCH_EXACT && rows_of(c, 4096).rows == 4096);
        EXPECT(rows_of(c, 4096).contraction == VSOM_SLC_NONE && rows_of(c, 4096).g_elems == 0 && rows_of(c, 4096).tmin_elems == 0);
        shape(c, 32, 32, 784, 4096);
        EXPECT(rows_of(c, 4096).path == VSOM_SEARCH_SL_I8);
        g_case = "AUTO: rows 63 / 64";
        EXPECT(rows_of(c, 63).path == VSOM_SEARCH_EXACT);
        EXPECT(rows_of(c, 64).path == VSOM_SEARCH_SL_I8);
        EXPECT(vsom_search_plan(c, 100, 163, false, true).path == VSOM_SEARCH_EXACT);
        EXPECT(vsom_search_plan(c, 100, 164, false, true).path == VSOM_SEARCH_SL_I8);
        g_case = "no rows";
        EXPECT(vsom_search_plan(c, 7, 7, false, true).path == VSOM_SEARCH_EXACT && vsom_search_plan(c, 7, 7, false, true).rows == 0);
        g_case = "AUTO: depth 64 / 65 with 64 x 1024 x D triples";
        shape(c, 32, 32, 64, 4096);
        EXPECT(rows_of(c, 64).path == VSOM_SEARCH_EXACT);
        shape(c, 32, 32, 65, 4096);
        EXPECT(rows_of(c, 64).path == VSOM_SEARCH_SL_I8);
        g_case = "AUTO: depth 15 / 16 with over 1e9 triples";
        shape(c, 64, 64, 15, 16384);
        EXPECT(rows_of(c, 16384).path == VSOM_SEARCH_EXACT);
        shape(c, 64, 64, 16, 16384);
        EXPECT(rows_of(c, 16384).path == VSOM_SEARCH_SL_I8);
        g_case = "AUTO: 64x64x32, 7629 / 7630 rows";      // 7629 * 4096 * 32 = 999 948 288, 7630: 1 000 079 360
        shape(c, 64, 64, 32, 16384);
        EXPECT(rows_of(c, 7629).path == VSOM_SEARCH_EXACT);
        EXPECT(rows_of(c, 7630).path == VSOM_SEARCH_SL_I8 && rows_of(c, 7630).wps == 1 && rows_of(c, 7630).refine.gx == 1908);
        g_case = "AUTO: the back-off skips";
        EXPECT(rows_of(c, 7630, true).path == VSOM_SEARCH_EXACT);
        g_case = "modes EXACT and SHORTLIST";
        c.bmu_mode = VSOM_BMU_EXACT;
        EXPECT(rows_of(c, 16384).path == VSOM_SEARCH_EXACT);
        c.bmu_mode = VSOM_BMU_SHORTLIST;
        EXPECT(rows_of(c, 7629).path == VSOM_SEARCH_SL_I8 && rows_of(c, 1).path == VSOM_SEARCH_SL_I8);
        EXPECT(rows_of(c, 7629, true).path == VSOM_SEARCH_SL_I8);
        shape(c, 33, 31, 784, 4096);
        EXPECT(rows_of(c, 63).path == VSOM_SEARCH_SL_I8);
        g_case = "AUTO: CLR is never short rows";         // J = 6: 15 pairs, D = 30; 16384 * 4096 * 30 = 2.0e9 triples
        c.bmu_mode = VSOM_BMU_AUTO;
        shape(c, 64, 64, 6, 16384, VSOM_CLR);
        EXPECT(c.D == 30 && rows_of(c, 16384).path == VSOM_SEARCH_EXACT);
        shape(c, 64, 64, 6, 16384, VSOM_MEDIAN);
        c.D = c.part_len = 30;
        EXPECT(rows_of(c, 16384).path == VSOM_SEARCH_SL_I8);
    }
    {
        g_case = "flagship: 128x128 x 784, 4096 rows, dense";
        vsom_ctx c;
        shape(c, 128, 128, 784, 4096);
        SearchPlan p = rows_of(c, 4096);
        EXPECT(p.path == VSOM_SEARCH_SL_I8 && p.rows == 4096 && !p.compact && p.kmax == 800 && p.kp8 == 832);
        EXPECT(p.form == VSOM_SLF_RING && p.contraction == VSOM_SLC_RING_GLESS && p.ring());
        EXPECT(!p.prepare64 && !p.quant64 && p.qfast);
        EXPECT(p.ldg == 16384 && p.ntm == 1024 && p.g_elems == 0 && p.tmin_elems == 4194304);
        EXPECT(launch(p.prepare, 4096, 1, 256) && launch(p.quant, 4096, 1, 256) && launch(p.contract, 128, 16, 512, 147456));
        EXPECT(p.refine_kind == VSOM_SLR_PICK && p.wps == 2 && launch(p.refine, 2048, 1, 256));
        EXPECT(units(p.thr_approx, 5.5) && units(p.thr_exact, 226.8) && p.thr_e1 == 0.f && p.digit_slack == 2.0f && p.cand_cap == 64);
        EXPECT(p.fb_xflag);
        g_case = "flagship, samples [4096, 8191): a workgroup per sample below 4096 rows";
        c.B = c.Bcap = 8192;
        p = vsom_search_plan(c, 4096, 8191, false, true);
        EXPECT(p.form == VSOM_SLF_RING && p.wps == 4 && launch(p.refine, 4095, 1, 256) && launch(p.contract, 128, 16, 512, 147456));
        EXPECT(launch(p.quant, 8192, 1, 256) && p.tmin_elems == 4095 * 1024);
        c.B = c.Bcap = 4096;
        g_case = "flagship, compacted to a pitch of 800";
        c.cc_valid = true, c.cpitch = 800;
        p = rows_of(c, 4096);
        EXPECT(p.path == VSOM_SEARCH_SL_I8 && p.compact && p.kmax == 800 && p.kp8 == 832 && p.form == VSOM_SLF_RING);
        EXPECT(p.ntm == 1024 && p.g_elems == 0 && launch(p.contract, 128, 16, 512, 147456) && p.wps == 2 && launch(p.refine, 2048, 1, 256));
        g_case = "flagship, compacted to a pitch of 704";
        c.cpitch = 704;
        p = rows_of(c, 4096);
        EXPECT(p.compact && p.kmax == 704 && p.kp8 == 704 && p.form == VSOM_SLF_RING && p.qfast && !p.quant64 && !p.prepare64);
        EXPECT(units(p.thr_exact, 226.8));                // the bound keeps the whole rows
        g_case = "flagship, compacted to a pitch of 64: k64 over rows of 784 values";
        c.cpitch = 64;
        p = rows_of(c, 4096);
        EXPECT(p.kmax == 64 && p.kp8 == 64 && p.form == VSOM_SLF_K64 && p.contraction == VSOM_SLC_K64 && p.quant64 && !p.prepare64);
        EXPECT(launch(p.prepare, 4096, 1, 256) && launch(p.quant, 256, 1, 256) && launch(p.contract, 32, 16, 256));
        EXPECT(p.refine_kind == VSOM_SLR_PICK && p.wps == 2 && launch(p.refine, 2048, 1, 256));
        EXPECT(rows_of(c, 4095).wps == 4);
        c.cc_valid = false;

        g_case = "flagship, no ring LDS";
        p = rows_of(c, 4096, false, false);
        EXPECT(p.path == VSOM_SEARCH_SL_I8 && p.form == VSOM_SLF_G && p.contraction == VSOM_SLC_SMALL_TILES && !p.ring() && p.qfast);
        EXPECT(p.ntm == 256 && p.g_elems == (size_t)4096 * 16384 && p.tmin_elems == 1048576 && launch(p.contract, 256, 32, 256));
        EXPECT(p.refine_kind == VSOM_SLR_SELECT && launch(p.refine, 4096, 1, 256) && p.cand_cap == 2048);

        g_case = "G-less ring from 256 big tiles: 256 / 257 rows";
        p = rows_of(c, 256);
        EXPECT(p.form == VSOM_SLF_G && p.contraction == VSOM_SLC_SMALL_TILES && launch(p.contract, 256, 2, 256));
        EXPECT(p.g_elems == (size_t)256 * 16384 && p.ntm == 256 && p.refine_kind == VSOM_SLR_SELECT && launch(p.refine, 256, 1, 256));
        p = rows_of(c, 257);
        EXPECT(p.form == VSOM_SLF_RING && p.contraction == VSOM_SLC_RING_GLESS && launch(p.contract, 128, 2, 512, 147456));
        EXPECT(p.g_elems == 0 && p.ntm == 1024 && p.wps == 4 && launch(p.refine, 257, 1, 256));

        g_case = "kp8 960 / 1024";
        shape(c, 128, 128, 960, 4096);
        p = rows_of(c, 4096);
        EXPECT(p.kp8 == 960 && p.qfast && p.form == VSOM_SLF_RING && p.contraction == VSOM_SLC_RING_GLESS);
        shape(c, 128, 128, 992, 4096);
        p = rows_of(c, 4096);
        EXPECT(p.kmax == 992 && p.kp8 == 1024 && !p.qfast && p.form == VSOM_SLF_G && p.contraction == VSOM_SLC_RING_G);
        EXPECT(launch(p.contract, 128, 16, 512, 147456) && p.refine_kind == VSOM_SLR_SELECT && p.g_elems == (size_t)4096 * 16384);

        g_case = "G ring from 1024 big tiles: J = 1024, 1792 / 2048 rows";
        shape(c, 128, 128, 1024, 4096);
        p = rows_of(c, 1792);
        EXPECT(p.kp8 == 1024 && p.form == VSOM_SLF_G && p.contraction == VSOM_SLC_SMALL_TILES && !p.qfast && launch(p.contract, 256, 14, 256));
        p = rows_of(c, 2048);
        EXPECT(p.form == VSOM_SLF_G && p.contraction == VSOM_SLC_RING_G && !p.qfast && launch(p.contract, 128, 8, 512, 147456));
        EXPECT(p.ntm == 256 && p.ldg == 16384 && p.refine_kind == VSOM_SLR_SELECT && launch(p.refine, 2048, 1, 256));
        p = rows_of(c, 2048, false, false);
        EXPECT(p.form == VSOM_SLF_G && p.contraction == VSOM_SLC_SMALL_TILES && launch(p.contract, 256, 16, 256));
    }
    {
        g_case = "k64: 32, 64 and 65 values";
        vsom_ctx c;
        shape(c, 64, 64, 32, 16384);
        SearchPlan p = rows_of(c, 16384);
        EXPECT(p.path == VSOM_SEARCH_SL_I8 && p.kmax == 32 && p.kp8 == 64 && p.form == VSOM_SLF_K64 && p.contraction == VSOM_SLC_K64);
        EXPECT(p.prepare64 && p.quant64 && p.qfast && !p.ring());
        EXPECT(launch(p.prepare, 256, 1, 256) && launch(p.quant, 1024, 1, 256) && launch(p.contract, 8, 64, 256));
        EXPECT(p.refine_kind == VSOM_SLR_PICK && p.wps == 1 && launch(p.refine, 4096, 1, 256) && p.cand_cap == 64);
        EXPECT(p.ntm == 256 && p.g_elems == 0 && p.tmin_elems == 4194304 && p.ldg == 4096);
        EXPECT(units(p.thr_approx, 5.5) && units(p.thr_exact, 29.4) && p.digit_slack == 2.0f && p.fb_xflag);
        shape(c, 64, 64, 64, 16384);
        p = rows_of(c, 16384);
        EXPECT(p.kp8 == 64 && p.form == VSOM_SLF_K64 && p.prepare64 && p.wps == 1);
        shape(c, 64, 64, 65, 16384);
        p = rows_of(c, 16384);
        EXPECT(p.kmax == 96 && p.kp8 == 128 && p.form == VSOM_SLF_RING && !p.prepare64 && !p.quant64 && p.wps == 2);
        EXPECT(launch(p.prepare, 1024, 1, 256) && launch(p.quant, 16384, 1, 256) && launch(p.contract, 32, 64, 512, 147456));
        shape(c, 32, 32, 65, 4096);
        p = rows_of(c, 64);
        EXPECT(p.kp8 == 128 && p.form == VSOM_SLF_G && p.contraction == VSOM_SLC_SMALL_TILES && launch(p.contract, 16, 1, 256));
    }
    {
        g_case = "40x36 x 784, 200 rows";
        vsom_ctx c;
        shape(c, 40, 36, 784, 200);
        const SearchPlan p = rows_of(c, 200);
        EXPECT(p.path == VSOM_SEARCH_SL_I8 && p.kp8 == 832 && p.form == VSOM_SLF_G && p.contraction == VSOM_SLC_SMALL_TILES && p.qfast);
        EXPECT(p.ldg == 1536 && p.ntm == 24 && p.g_elems == 307200 && p.tmin_elems == 4800);
        EXPECT(!p.prepare64 && launch(p.prepare, 360, 1, 256) && !p.quant64 && launch(p.quant, 200, 1, 256));
        EXPECT(launch(p.contract, 24, 2, 256));
        EXPECT(p.refine_kind == VSOM_SLR_SELECT && launch(p.refine, 200, 1, 256) && p.cand_cap == 2048);
        EXPECT(units(p.thr_approx, 5.5) && units(p.thr_exact, 226.8) && p.digit_slack == 2.0f && p.fb_xflag);

        // the shapes whose form tests/test_gpu_ties.py states (PLAN, through ties.ring_plan): 0, 2, 1, 1
        g_case = "the forms of the tie cases";
        c.bmu_mode = VSOM_BMU_SHORTLIST;
        EXPECT(rows_of(c, 200).form == VSOM_SLF_G && VSOM_SLF_G == 0);
        shape(c, 128, 128, 784, 2048);
        EXPECT(rows_of(c, 2048).form == VSOM_SLF_RING && VSOM_SLF_RING == 2);
        shape(c, 64, 64, 32, 400);
        EXPECT(rows_of(c, 400).form == VSOM_SLF_K64 && VSOM_SLF_K64 == 1);
        shape(c, 40, 36, 24, 200);
        EXPECT(rows_of(c, 200).form == VSOM_SLF_K64);
    }
    {
        g_case = "xpitch 4096 / 4128: integer / fp32 contraction";
        vsom_ctx c;
        shape(c, 32, 32, 4096, 128);
        SearchPlan p = rows_of(c, 128);
        EXPECT(p.path == VSOM_SEARCH_SL_I8 && p.kp8 == 4096 && !p.qfast && p.form == VSOM_SLF_G && p.contraction == VSOM_SLC_SMALL_TILES);
        EXPECT(p.refine_kind == VSOM_SLR_SELECT && units(p.thr_approx, 5.5) && units(p.thr_exact, 1096.2) && p.digit_slack == 2.0f);
        EXPECT(p.fb_xflag && launch(p.contract, 16, 1, 256));
        shape(c, 32, 32, 4097, 128);
        p = rows_of(c, 128);
        EXPECT(p.path == VSOM_SEARCH_SL_FP32 && p.kmax == 4128 && p.kp8 == 0 && p.form == VSOM_SLF_G && p.contraction == VSOM_SLC_FP32);
        EXPECT(!p.compact && !p.ring() && !p.fb_xflag && p.digit_slack == 0.f && p.cand_cap == 2048);
        EXPECT(units(p.thr_approx, 328.0) && units(p.thr_exact, 1096.4625));      // 2 g1 = 2 (32 + 4128 / 32 + 3) u
        EXPECT(launch(p.norm, 64, 1, 256) && launch(p.contract, 8, 1, 256) && launch(p.refine, 128, 1, 256));
        EXPECT(p.refine_kind == VSOM_SLR_SELECT && p.ldg == 1024 && p.ntm == 16 && p.g_elems == 131072 && p.tmin_elems == 2048);
        c.cc_valid = true, c.cpitch = 2048;
        p = rows_of(c, 128);
        EXPECT(p.path == VSOM_SEARCH_SL_FP32 && p.compact && p.kmax == 2048 && units(p.thr_approx, 328.0));
    }
    {
        g_case = "CLR 34x34, J = 10, 120 rows";
        vsom_ctx c;
        shape(c, 34, 34, 10, 120, VSOM_CLR);
        SearchPlan p = rows_of(c, 120);
        EXPECT(c.D == 90 && c.part_pitch == 64 && p.path == VSOM_SEARCH_SL_CLR && p.P32 == 64 && p.Kp == 96);
        EXPECT(p.ldg == 1280 && p.ntm == 20 && p.g_elems == 153600 && p.tmin_elems == 2400 && p.fs_elems == 11520 && p.fm_elems == 110976);
        EXPECT(launch(p.norm, 1156, 1, 256) && launch(p.sample_feat, 120, 1, 256) && launch(p.contract, 10, 1, 256));
        EXPECT(p.contraction == VSOM_SLC_FP32 && p.refine_kind == VSOM_SLR_SELECT && launch(p.refine, 120, 1, 256, 512));
        // ga = 3.01 (38 + 13) u + (45 / 256 + 19) u, g2 = (45 / 8 + 10) u, e1 = 6.1 sqrt(3) u, each times 1.0001
        EXPECT(units(p.thr_approx, 172.703049828125) && units(p.thr_exact, 15.6265625) && units(p.thr_e1, 10.56656647716277));
        EXPECT(p.cand_cap == 128 && p.digit_slack == 0.f && !p.fb_xflag && !p.compact && p.kp8 == 0);
        g_case = "CLR: x' / y' rows of 48 KB stay, one pitch step more goes exact";
        shape(c, 34, 34, 111, 120, VSOM_CLR);             // 6105 pairs
        EXPECT(c.part_pitch == 6112 && rows_of(c, 120).path == VSOM_SEARCH_SL_CLR);
        c.part_pitch = 6144, c.pitch = 12288;             // 2 * 6144 * 4 = 49152 = 48 * 1024
        p = rows_of(c, 120);
        EXPECT(p.path == VSOM_SEARCH_SL_CLR && p.refine.lds == 49152);
        c.part_pitch = 6176, c.pitch = 12352;
        p = rows_of(c, 120);
        EXPECT(p.path == VSOM_SEARCH_EXACT && p.contraction == VSOM_SLC_NONE && p.g_elems == 0);
        c.bmu_mode = VSOM_BMU_SHORTLIST;
        EXPECT(rows_of(c, 120).path == VSOM_SEARCH_EXACT);
        shape(c, 34, 34, 112, 120, VSOM_CLR);             // 6216 pairs
        EXPECT(c.part_pitch == 6240 && rows_of(c, 120).path == VSOM_SEARCH_EXACT);
    }
    {
        g_case = "exact plan: 128x128 x 784, 1557 / 1558 rows";     // x 16384 x 784: 19 999 752 192 / 20 012 597 248 triples
        vsom_ctx c;
        shape(c, 128, 128, 784, 4096);
        ExactPlan e = vsom_exact_plan(c, 0, 1557, false, false);
        EXPECT(!e.dedupe && e.ntn == 256 && e.TS == 64 && e.nts == 25 && e.gy == 25 && e.partial_elems == 1048576 && !e.clr && !e.list);
        e = vsom_exact_plan(c, 0, 1558, false, false);
        EXPECT(e.dedupe && e.nts == 25 && e.gy == 25);
        EXPECT(vsom_exact_plan(c, 2000, 3558, false, false).dedupe && !vsom_exact_plan(c, 2000, 3557, false, false).dedupe);
        g_case = "exact plan: restricted, switched off";
        EXPECT(!vsom_exact_plan(c, 0, 4096, false, true).dedupe);
        c.dedupe = false;
        EXPECT(!vsom_exact_plan(c, 0, 4096, false, false).dedupe);
        c.dedupe = true, c.dd_min_work = -1.0;
        EXPECT(!vsom_exact_plan(c, 0, 4096, false, false).dedupe);
        c.dd_min_work = 0.0;
        EXPECT(vsom_exact_plan(c, 0, 1, false, false).dedupe && !vsom_exact_plan(c, 0, 1, false, true).dedupe);
        g_case = "exact plan: with a redo list";
        e = vsom_exact_plan(c, 0, 4096, true, false);     // threshold 0: always
        EXPECT(e.dedupe && e.list && e.nts == 64 && e.gy == 2);
        c.dd_min_work = 2.0e10;
        e = vsom_exact_plan(c, 0, 4096, true, false);
        EXPECT(!e.dedupe && e.list && e.gy == 2);
        EXPECT(vsom_exact_plan(c, 0, 4096, false, false).dedupe && vsom_exact_plan(c, 0, 4096, false, false).gy == 64);
        EXPECT(vsom_exact_plan(c, 0, 64, true, false).gy == 1);
        g_case = "exact plan: 255 / 256 nodes";
        c.dd_min_work = 0.0;
        shape(c, 15, 17, 784, 4096);
        e = vsom_exact_plan(c, 0, 4096, false, false);
        EXPECT(!e.dedupe && e.ntn == 4 && e.partial_elems == 16384);
        shape(c, 16, 16, 784, 4096);
        EXPECT(vsom_exact_plan(c, 0, 4096, false, false).dedupe);
        g_case = "exact plan: grid of a list search";
        shape(c, 40, 36, 784, 200);
        e = vsom_exact_plan(c, 0, 200, true, false);      // 23 node tiles: up to 22 workgroups each
        EXPECT(e.ntn == 23 && e.nts == 4 && e.gy == 4);
        c.B = c.Bcap = 4096;
        e = vsom_exact_plan(c, 0, 4096, true, false);
        EXPECT(e.nts == 64 && e.gy == 22 && e.partial_elems == 23 * 4096);
        shape(c, 1024, 64, 784, 4096);
        e = vsom_exact_plan(c, 0, 4096, true, false);
        EXPECT(e.ntn == 1024 && e.gy == 1);
        g_case = "exact plan: CLR";
        shape(c, 34, 34, 10, 120, VSOM_CLR);
        c.dd_min_work = 1.0;
        e = vsom_exact_plan(c, 0, 120, true, false);
        EXPECT(e.clr && e.list && e.TS == 32 && e.nts == 4 && e.ntn == 19 && e.gy == 4 && e.dedupe);
        c.dd_min_work = 2.0e10;
        EXPECT(!vsom_exact_plan(c, 0, 120, true, false).dedupe);      // 120 x 1156 x 90 triples
        c.transform = VSOM_STANDARD, c.dd_min_work = 1.0;
        e = vsom_exact_plan(c, 0, 120, true, false);
        EXPECT(!e.clr && e.TS == 64 && e.nts == 2 && !e.dedupe);
        EXPECT(vsom_exact_plan(c, 0, 120, false, false).dedupe);
    }
    {
        g_case = "back-off";
        int skip = 0, streak = 0;
        unsigned seen = 0;
        EXPECT(skipped(skip, streak, seen, 0, 100, 1) == 0 && streak == 0 && seen == 1);
        EXPECT(skipped(skip, streak, seen, 25, 100, 2) == 0 && streak == 0);      // a quarter redone is no failure
        EXPECT(skipped(skip, streak, seen, 26, 100, 3) == 0 && streak == 1);      // the first failure skips nothing
        EXPECT(skipped(skip, streak, seen, 99, 100, 3) == 0 && streak == 1);      // a sequence number is acted on once
        EXPECT(skipped(skip, streak, seen, 26, 100, 4) == 4 && streak == 2 && skip == 0);
        EXPECT(skipped(skip, streak, seen, 26, 100, 4) == 0 && streak == 2);
        EXPECT(skipped(skip, streak, seen, 100, 100, 5) == 8 && streak == 3);
        EXPECT(skipped(skip, streak, seen, 100, 100, 6) == 16 && streak == 4);
        EXPECT(skipped(skip, streak, seen, 100, 100, 7) == 32 && streak == 5);
        EXPECT(skipped(skip, streak, seen, 100, 100, 8) == 32 && streak == 6);
        EXPECT(skipped(skip, streak, seen, 100, 100, 9) == 32 && streak == 7);
        EXPECT(skipped(skip, streak, seen, 5, 0, 10) == 0 && streak == 0);         // no rows: no failure, and the streak ends
        EXPECT(skipped(skip, streak, seen, 100, 100, 11) == 0 && streak == 1);
        EXPECT(skipped(skip, streak, seen, 100, 100, 12) == 4 && streak == 2);
        EXPECT(skipped(skip, streak, seen, 1, 100, 13) == 0 && streak == 0);       // a success resets the streak
        EXPECT(skipped(skip, streak, seen, 100, 100, 14) == 0 && streak == 1);
        // the searches skipped count the one that saw the failure; a success seen meanwhile does not end the pause
        EXPECT(vsom_sl_backoff_step(skip, streak, seen, 100, 100, 15) && skip == 3 && streak == 2);
        EXPECT(vsom_sl_backoff_step(skip, streak, seen, 0, 100, 16) && skip == 2 && streak == 0);
        EXPECT(skipped(skip, streak, seen, 0, 100, 16) == 2);
        g_case = "the quant kernel of the gather pass";
        EXPECT(vsom_sl_quant64(64) && !vsom_sl_quant64(128) && vsom_sl_quant_grid(true, 4097) == 257 && vsom_sl_quant_grid(false, 4097) == 4097);
    }
    if (g_errors) {
        std::printf("%ld failure(s)\n", g_errors);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
