// sched_round_driver.cpp -- the round image of a resident schedule (csrc/vsom_sched_round.hpp) on the host, without a
// device or the library: tests/test_sched_round.py compiles this file (with the sanitizers where the toolchain has them)
// and runs it.  The library's vsom_neighbourhood_weight is the header's one outside reference; the stand-in below encodes
// its arguments, so a table value names the (dx, dy, sigma) it was asked for and where it landed.
#include "vsom_sched_round.hpp"
#include <cstdio>
#include <cstdlib>

extern "C" double vsom_neighbourhood_weight(size_t cx, size_t cy, size_t bx, size_t by, double sigma)
{
    if (bx || by)
        return -1.0;             // (the tables are tabulated around the origin)
    return sigma * 1000.0 + (double)cy * 10.0 + (double)cx + 0.25;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static VsomSchedMember member(uint32_t lw, uint32_t lh, const double *sigma, size_t epochs, const uint8_t *valid = nullptr,
                              size_t vbytes = 0)
{
    return VsomSchedMember{lw, lh, sigma, epochs, valid, vbytes};
}

// the planned round written into an image of exactly bytes() (the sanitizer sees a write past it)
static std::vector<unsigned char> image(const VsomSchedRound &r, const std::vector<VsomSchedMember> &m)
{
    std::vector<unsigned char> img(r.bytes());
    r.write(img.data(), m.data());
    return img;
}

static unsigned offset_word(const VsomSchedRound &r, const std::vector<unsigned char> &img, size_t i)
{
    unsigned v;
    std::memcpy(&v, img.data() + r.table_bytes() + i * sizeof(unsigned), sizeof(v));
    return v;
}

static float table_value(const std::vector<unsigned char> &img, size_t i)
{
    float v;
    std::memcpy(&v, img.data() + i * sizeof(float), sizeof(v));
    return v;
}

int main()
{
    VsomSchedRound r;
    // one member, three epochs, two equal sigmas: two tables, offsets [0, wh, 0]
    {
        const double s[3] = {2.0, 1.5, 2.0};
        std::vector<VsomSchedMember> m = {member(4, 3, s, 3)};
        CHECK(r.plan(m.data(), m.size()));
        CHECK(r.tabs.at.size() == 2 && r.tabs.floats == 24);
        CHECK(r.table_bytes() == 96 && r.offset_bytes() == 12 && r.valid_bytes() == 0 && r.bytes() == 108);
        CHECK(r.tab_at[0] == 0 && r.v_at[0] == 0);
        const auto img = image(r, m);
        CHECK(offset_word(r, img, 0) == 0 && offset_word(r, img, 1) == 12 && offset_word(r, img, 2) == 0);
    }
    // two members of equal shape sharing a sigma: one table; their offsets in member order
    {
        const double a[2] = {2.0, 3.0}, b[1] = {3.0};
        std::vector<VsomSchedMember> m = {member(5, 5, a, 2), member(5, 5, b, 1)};
        CHECK(r.plan(m.data(), m.size()));
        CHECK(r.tabs.at.size() == 2 && r.tabs.floats == 50);
        CHECK(r.tab_at[0] == 0 && r.tab_at[1] == 2 && r.tab.size() == 3);
        const auto img = image(r, m);
        CHECK(offset_word(r, img, 0) == 0 && offset_word(r, img, 1) == 25 && offset_word(r, img, 2) == 25);
    }
    // two members whose shapes differ with equal sigma: two tables, at the offsets of first appearance
    {
        const double s[1] = {2.0};
        std::vector<VsomSchedMember> m = {member(5, 4, s, 1), member(4, 5, s, 1)};
        CHECK(r.plan(m.data(), m.size()));
        CHECK(r.tabs.at.size() == 2 && r.tabs.floats == 40);
        const auto img = image(r, m);
        CHECK(offset_word(r, img, 0) == 0 && offset_word(r, img, 1) == 20);
    }
    // 0.0 and -0.0: distinct bit patterns, two tables
    {
        const double s[3] = {0.0, -0.0, 0.0};
        std::vector<VsomSchedMember> m = {member(2, 2, s, 3)};
        CHECK(r.plan(m.data(), m.size()));
        CHECK(r.tabs.at.size() == 2 && r.tabs.floats == 8);
        const auto img = image(r, m);
        CHECK(offset_word(r, img, 0) == 0 && offset_word(r, img, 1) == 4 && offset_word(r, img, 2) == 0);
    }
    // a member with no epochs left in the round (though it has validity bytes): no offsets, no validity bytes; the offsets
    // of the members after it are those of the round without it
    {
        const double a[2] = {2.0, 2.5}, b[2] = {2.5, 4.0};
        const uint8_t va[3] = {1, 0, 1}, ve[5] = {9, 9, 9, 9, 9}, vb[2] = {0, 1};
        std::vector<VsomSchedMember> with = {member(3, 3, a, 2, va, 3), member(7, 7, a, 0, ve, 5), member(3, 3, b, 2, vb, 2)};
        std::vector<VsomSchedMember> without = {with[0], with[2]};
        VsomSchedRound q;
        CHECK(r.plan(with.data(), with.size()) && q.plan(without.data(), without.size()));
        CHECK(r.tab == q.tab && r.tabs.floats == q.tabs.floats && r.tabs.floats == 27);
        CHECK(r.tab_at[0] == 0 && r.tab_at[2] == 2 && q.tab_at[1] == 2);
        CHECK(r.v_at[0] == 0 && r.v_at[2] == 3 && r.valid_bytes() == 5 && q.valid_bytes() == 5);
        CHECK(image(r, with) == image(q, without));
    }
    // validity offsets for the mix B x J, J (one row) and none; the bytes land behind the offsets, packed
    {
        const double s[1] = {2.0};
        uint8_t full[12], row[4];
        for (int i = 0; i < 12; ++i)
            full[i] = (uint8_t)(i + 1);
        for (int i = 0; i < 4; ++i)
            row[i] = (uint8_t)(0x80 + i);
        std::vector<VsomSchedMember> m = {member(2, 2, s, 1, full, 12), member(2, 2, s, 1, row, 4), member(2, 2, s, 1),
                                          member(2, 2, s, 1, row, 4)};
        CHECK(r.plan(m.data(), m.size()));
        CHECK(r.v_at[0] == 0 && r.v_at[1] == 12 && r.v_at[2] == 16 && r.v_at[3] == 16 && r.valid_bytes() == 20);
        CHECK(r.table_bytes() == 16 && r.offset_bytes() == 16 && r.bytes() == 52);
        const auto img = image(r, m);
        const unsigned char *v = img.data() + r.table_bytes() + r.offset_bytes();
        CHECK(std::memcmp(v, full, 12) == 0 && std::memcmp(v + 12, row, 4) == 0 && std::memcmp(v + 16, row, 4) == 0);
    }
    // the tables of one round exceed 2^32 values: refused by the size computation alone (nothing is tabulated or allocated)
    {
        const double s[2] = {2.0, 3.0};
        std::vector<VsomSchedMember> m = {member(65536, 32768, s, 2)};
        CHECK(!r.plan(m.data(), m.size()));
        CHECK(r.tabs.floats == (size_t)1 << 32);
        std::vector<VsomSchedMember> fits = {member(65536, 32768, s, 1), member(65535, 32768, s + 1, 1)};
        CHECK(r.plan(fits.data(), fits.size()));
        CHECK(r.tabs.floats == 0xFFFF8000ull && r.tab[1] == 0x80000000u);
    }
    // the table values: (float)vsom_neighbourhood_weight(dx, dy, 0, 0, sigma), row by row, for one 3 x 2 table
    {
        const double s[1] = {1.75};
        std::vector<VsomSchedMember> m = {member(3, 2, s, 1)};
        CHECK(r.plan(m.data(), m.size()));
        const auto img = image(r, m);
        for (uint32_t dy = 0; dy < 2; ++dy)
            for (uint32_t dx = 0; dx < 3; ++dx)
                CHECK(table_value(img, dy * 3 + dx) == (float)vsom_neighbourhood_weight(dx, dy, 0, 0, 1.75));
        CHECK(table_value(img, 5) == 1762.25f);
    }
    std::printf("ok\n");
    return 0;
}
