// Host-only driver for csrc/vsom_buf.hpp (tests/test_buffer_sets.py): the allocate / free seam is replaced by host
// memory that fails on the k-th allocation, and every outcome of a set is checked -- no device is touched.
#include "vsom_buf.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

static std::set<void *> g_live;        // allocations not yet freed
static long g_calls = 0, g_fail_at = -1, g_errors = 0;
static long g_releases = 0, g_pinned_allocs = 0, g_pinned_releases = 0;

static hipError_t fake_alloc(void **p, size_t bytes, bool pinned)
{
    g_pinned_allocs += pinned;
    if (g_calls++ == g_fail_at) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    std::memset(*p, 0xAB, bytes);
    g_live.insert(*p);
    return hipSuccess;
}

static hipError_t fake_release(void *p, bool pinned)
{
    ++g_releases;
    g_pinned_releases += pinned;
    if (!g_live.erase(p)) {
        std::printf("freed a pointer that is not live (double free or foreign)\n");
        ++g_errors;
    }
    std::free(p);
    return hipSuccess;
}

// The arena grows with VSOM_BUF_SYNC.  The program's own definition takes the place of the runtime's, so that no device is
// needed, and counts the calls: a synchronise comes before every drop of an allocated arena.
static long g_syncs = 0;
extern "C" hipError_t hipStreamSynchronize(hipStream_t)
{
    ++g_syncs;
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

    // the scratch arena: a layout of mixed types and counts carves at multiples of 256 bytes, in request order, without
    // overlap; a zero count takes no bytes; no pointer before the arena is there
    g_calls = 0, g_fail_at = -1;
    {
        DevBuf<unsigned char> arena;
        vsom_layout lay;
        const auto a = lay.add<unsigned long long>(3);
        const auto b = lay.add<unsigned char>(5);
        const auto z = lay.add<double>(0);
        const auto f = lay.add<float>(7);
        EXPECT(a.off == 0 && b.off == 256 && z.off == 512 && f.off == 512 && lay.bytes == 768);
        EXPECT(a.off + 3 * 8 <= b.off && b.off + 5 <= z.off && f.off + 7 * 4 <= lay.bytes);
        EXPECT(!lay.at(a) && !lay.at(f));
        EXPECT(vsom_arena_ensure(arena, lay, nullptr) == hipSuccess && arena.p && arena.cap == 4096 && g_calls == 1);
        EXPECT((unsigned char *)lay.at(a) == arena.p && lay.at(b) == arena.p + 256 && (unsigned char *)lay.at(f) == arena.p + 512);
        EXPECT((unsigned char *)lay.at(z) == arena.p + 512);
        for (int i = 0; i < 3; ++i)        // (every carved element is writable: the sanitizer build checks the bounds)
            lay.at(a)[i] = 1;
        for (int i = 0; i < 7; ++i)
            lay.at(f)[i] = 1.f;
        std::memset(lay.at(b), 1, 5);

        // grow-only: a smaller layout after a larger one allocates nothing and is bound to the same arena
        vsom_layout big;
        (void)big.add<float>(5000);
        const auto tail = big.add<unsigned char>(1);
        EXPECT(tail.off == 20224 && big.bytes == 20480);
        g_releases = 0;
        EXPECT(vsom_arena_ensure(arena, big, nullptr) == hipSuccess && arena.cap == 20480);
        EXPECT(g_calls == 2 && g_releases == 1 && g_live.size() == 1);   // exactly one buffer released, one allocated
        EXPECT(g_syncs == 1);                                            // (behind a synchronise; none on first use)
        unsigned char *held = arena.p;
        vsom_layout small;
        const auto s0 = small.add<unsigned>(9);
        EXPECT(vsom_arena_ensure(arena, small, nullptr) == hipSuccess && g_calls == 2 && g_releases == 1);
        EXPECT(arena.p == held && arena.cap == 20480 && (unsigned char *)small.at(s0) == held);
        vsom_layout none;                   // an empty layout asks for nothing
        EXPECT(vsom_arena_ensure(arena, none, nullptr) == hipSuccess && g_calls == 2 && arena.p == held);

        // a failing allocator: the error, the arena absent, no pointer; the next, smaller request succeeds
        vsom_layout huge;
        const auto h = huge.add<double>(1 << 20);
        g_fail_at = g_calls;
        EXPECT(vsom_arena_ensure(arena, huge, nullptr) == hipErrorOutOfMemory);
        EXPECT(!arena.p && arena.cap == 0 && !huge.at(h) && g_live.empty());
        g_fail_at = -1;
        EXPECT(vsom_arena_ensure(arena, lay, nullptr) == hipSuccess && arena.p && arena.cap == 4096);
        EXPECT((unsigned char *)lay.at(f) == arena.p + 512 && g_live.size() == 1);
    }
    EXPECT(g_live.empty());

    // the pinned arena passes pinned = true to both allocator functions, the device arena to neither
    {
        g_pinned_allocs = g_pinned_releases = g_releases = 0;
        g_calls = 0;
        PinnedBuf<unsigned char> pinned;
        DevBuf<unsigned char> dev;
        vsom_layout one, two;
        (void)one.add<unsigned>(10);
        (void)two.add<unsigned>(2000);
        EXPECT(vsom_arena_ensure(dev, one, nullptr) == hipSuccess && vsom_arena_ensure(dev, two, nullptr) == hipSuccess);
        EXPECT(g_calls == 2 && g_releases == 1 && g_pinned_allocs == 0 && g_pinned_releases == 0);
        EXPECT(vsom_arena_ensure(pinned, one, nullptr) == hipSuccess && vsom_arena_ensure(pinned, two, nullptr) == hipSuccess);
        EXPECT(g_calls == 4 && g_releases == 2 && g_pinned_allocs == 2 && g_pinned_releases == 1);
    }
    EXPECT(g_live.empty() && g_pinned_releases == 2);

    if (g_errors) {
        std::printf("%ld failure(s)\n", g_errors);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
