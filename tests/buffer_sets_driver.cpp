// Host-only driver for csrc/vsom_buf.hpp (tests/test_buffer_sets.py): the allocate / free seam is replaced by host
// memory that fails on the k-th allocation, and every outcome of a set is checked -- no device is touched.
#include "vsom_buf.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

static std::set<void *> g_live;        // allocations not yet freed
static long g_calls = 0, g_fail_at = -1, g_errors = 0;

static hipError_t fake_alloc(void **p, size_t bytes, bool)
{
    if (g_calls++ == g_fail_at) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    std::memset(*p, 0xAB, bytes);
    g_live.insert(*p);
    return hipSuccess;
}

static hipError_t fake_release(void *p, bool)
{
    if (!g_live.erase(p)) {
        std::printf("freed a pointer that is not live (double free or foreign)\n");
        ++g_errors;
    }
    std::free(p);
    return hipSuccess;
}

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("%s:%d: expected %s (k = %ld)\n", __FILE__, __LINE__, #cond, g_fail_at); \
            ++g_errors;                                                       \
        }                                                                     \
    } while (0)

struct Set {
    DevBuf<unsigned long long> a;
    DevBuf<float> b;
    PinnedBuf<unsigned> c;
    DevBuf<int4> d;
    PinnedBuf<double> e;
    hipError_t grow(size_t n, unsigned flags = 0)
    {
        return vsom_grow_set(nullptr, flags, {vsom_member(a, n), vsom_member(b, 2 * n), vsom_member(c, 16, VSOM_BUF_ZERO),
                                              vsom_member(d, n + 1), vsom_member(e, 3 * n, VSOM_BUF_ZERO)});
    }
    bool empty() const
    {
        return !a.p && !b.p && !c.p && !d.p && !e.p && !a.cap && !b.cap && !c.cap && !d.cap && !e.cap;
    }
};

int main()
{
    vsom_mem = {fake_alloc, fake_release};
    const int members = 5;

    // a fresh set whose k-th allocation fails: NOMEM, every member null with capacity 0, nothing leaked
    for (long k = 0; k < members; ++k) {
        g_calls = 0, g_fail_at = k;
        {
            Set s;
            EXPECT(s.grow(100) == hipErrorOutOfMemory);
            EXPECT(s.empty());
            EXPECT(g_live.empty());
            g_fail_at = -1;            // the retry succeeds and the guard sees the set as absent until then
            EXPECT(s.grow(100) == hipSuccess);
            EXPECT(!s.empty() && s.a.cap == 100 && s.b.cap == 200 && s.c.cap == 16 && s.d.cap == 101 && s.e.cap == 300);
            EXPECT(g_live.size() == (size_t)members);
        }
        EXPECT(g_live.empty());        // the owners freed the set exactly once
    }

    // growing an allocated set whose k-th allocation fails: the old members are freed first, the set ends empty
    for (long k = 0; k < members; ++k) {
        g_calls = 0, g_fail_at = -1;
        {
            Set s;
            EXPECT(s.grow(10) == hipSuccess);
            g_calls = 0, g_fail_at = k;
            EXPECT(s.grow(1000) == hipErrorOutOfMemory);
            EXPECT(s.empty());
            EXPECT(g_live.empty());
        }
        EXPECT(g_live.empty());
    }

    // a set that fits allocates nothing; a forced rebuild reallocates at the given sizes; zero fills are done
    g_calls = 0, g_fail_at = -1;
    {
        Set s;
        EXPECT(s.grow(50) == hipSuccess);
        for (size_t i = 0; i < 16; ++i)
            EXPECT(s.c.p[i] == 0u);
        for (size_t i = 0; i < 150; ++i)
            EXPECT(s.e.p[i] == 0.0);
        const long calls = g_calls;
        EXPECT(s.grow(20) == hipSuccess && g_calls == calls && s.a.cap == 50);
        EXPECT(s.grow(20, VSOM_BUF_REBUILD) == hipSuccess && g_calls == calls + members && s.a.cap == 20);
        EXPECT(g_live.size() == (size_t)members);
    }
    EXPECT(g_live.empty());

    // one buffer: grow-only, the old buffer is freed before the new one is allocated, a failure leaves it empty
    {
        DevBuf<float> x;
        g_calls = 0, g_fail_at = -1;
        EXPECT(vsom_grow(x, 8, nullptr) == hipSuccess && x.cap == 8 && g_live.size() == 1);
        EXPECT(vsom_grow(x, 4, nullptr) == hipSuccess && x.cap == 8 && g_calls == 1);
        EXPECT(vsom_grow(x, 64, nullptr) == hipSuccess && x.cap == 64 && g_live.size() == 1);
        g_fail_at = g_calls;
        EXPECT(vsom_grow(x, 128, nullptr) == hipErrorOutOfMemory && !x.p && x.cap == 0 && g_live.empty());
        g_fail_at = -1;
        EXPECT(vsom_grow(x, 0, nullptr) == hipSuccess && !x.p);
        // moves hand the buffer over without a second free
        EXPECT(vsom_grow(x, 16, nullptr) == hipSuccess);
        DevBuf<float> y(std::move(x));
        EXPECT(!x.p && x.cap == 0 && y.p && y.cap == 16);
        DevBuf<float> z;
        z = std::move(y);
        EXPECT(!y.p && z.p && g_live.size() == 1);
    }
    EXPECT(g_live.empty());

    if (g_errors) {
        std::printf("%ld failure(s)\n", g_errors);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
