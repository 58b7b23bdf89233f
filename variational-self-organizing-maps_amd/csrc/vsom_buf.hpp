// vsom_buf.hpp -- owners of the device and pinned host buffers of a context.
//
// DevBuf<T> / PinnedBuf<T>: a typed pointer and its capacity in elements, freed by the destructor (move-only).  Kernels
// and launches take the raw pointer, `buf.p`.
//
// vsom_grow_set(stream, flags, {vsom_member(buf, count[, VSOM_BUF_ZERO]), ...}) sizes buffers that exist together.  When
// every member already holds its count (and VSOM_BUF_REBUILD is not set) it does nothing.  Otherwise it drops every
// member first (after synchronising `stream` when VSOM_BUF_SYNC is set and a member is allocated), so that what fits
// now still fits after the rebuild, then allocates all members into locals and publishes them only once every
// allocation (and zero fill, on `stream` -- never hipMemset, which runs on the null stream) has succeeded.  On failure
// it frees what it allocated and every member is left null with capacity 0: a set is either whole or absent.  A count
// of 0 leaves that member null.  The result is a hipError_t for VSOM_HIP_CHECK (out of memory -> VSOM_ERR_NOMEM).
// vsom_grow(buf, count, stream, flags) is the set of one.
//
// vsom_layout / vsom_arena_ensure: the scratch of one call, carved out of one grow-only byte arena (device or pinned).
// The call collects its pieces first, h = lay.add<T>(count), each at a multiple of 256 bytes as hipMalloc would place it
// (a count of 0 takes no bytes); vsom_arena_ensure(arena, lay, stream) then grows the arena to the layout's total rounded
// up to 4 KiB (VSOM_BUF_SYNC; on failure the arena is absent) and binds the layout to it.  lay.at(h), the piece's typed
// pointer, is null until that has succeeded.  An arena's contents belong to the running call.
//
// The allocate / free functions are reached through `vsom_mem`, so a host-only test can substitute failing ones.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>
#include <initializer_list>

struct vsom_mem_fns {
    hipError_t (*alloc)(void **p, size_t bytes, bool pinned);
    hipError_t (*release)(void *p, bool pinned);
};

inline hipError_t vsom_hip_alloc(void **p, size_t bytes, bool pinned)
{
    return pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
}

inline hipError_t vsom_hip_release(void *p, bool pinned) { return pinned ? hipHostFree(p) : hipFree(p); }

inline vsom_mem_fns vsom_mem = {vsom_hip_alloc, vsom_hip_release};

template <typename T, bool Pinned>
struct vsom_buf {
    T *p = nullptr;
    size_t cap = 0;     // elements

    vsom_buf() = default;
    vsom_buf(const vsom_buf &) = delete;
    vsom_buf &operator=(const vsom_buf &) = delete;
    vsom_buf(vsom_buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    vsom_buf &operator=(vsom_buf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~vsom_buf() { reset(); }

    void reset()
    {
        if (p)
            (void)vsom_mem.release(p, Pinned);
        p = nullptr;
        cap = 0;
    }
};

template <typename T> using DevBuf = vsom_buf<T, false>;
template <typename T> using PinnedBuf = vsom_buf<T, true>;

enum : unsigned {
    VSOM_BUF_SYNC = 1,      // synchronise the stream before an allocated buffer is freed
    VSOM_BUF_ZERO = 2,      // zero-fill after allocation (device: on the stream; pinned: on the host)
    VSOM_BUF_REBUILD = 4,   // reallocate even if every member fits (a shape key changed)
};

// one member of a set, type-erased
struct vsom_buf_member {
    void **p;
    size_t *cap;
    size_t count, bytes;
    bool pinned, zero;
};

template <typename T, bool Pinned>
vsom_buf_member vsom_member(vsom_buf<T, Pinned> &b, size_t count, unsigned flags = 0)
{
    return {reinterpret_cast<void **>(&b.p), &b.cap, count, count * sizeof(T), Pinned, (flags & VSOM_BUF_ZERO) != 0};
}

inline hipError_t vsom_grow_set(hipStream_t stream, unsigned flags, std::initializer_list<vsom_buf_member> set)
{
    constexpr size_t kMax = 16;
    if (set.size() > kMax)
        return hipErrorInvalidValue;
    bool fits = !(flags & VSOM_BUF_REBUILD), any = false;
    for (const vsom_buf_member &m : set) {
        fits = fits && *m.cap >= m.count;
        any = any || *m.p;
    }
    if (fits)
        return hipSuccess;
    if (any && (flags & VSOM_BUF_SYNC)) {
        hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess)
            return e;
    }
    for (const vsom_buf_member &m : set) {
        if (*m.p)
            (void)vsom_mem.release(*m.p, m.pinned);
        *m.p = nullptr;
        *m.cap = 0;
    }
    void *got[kMax] = {};
    hipError_t e = hipSuccess;
    size_t i = 0;
    for (const vsom_buf_member &m : set) {
        if (m.count) {
            if ((e = vsom_mem.alloc(&got[i], m.bytes, m.pinned)) != hipSuccess) {
                got[i] = nullptr;
                break;
            }
            if (m.zero) {
                if (m.pinned)
                    memset(got[i], 0, m.bytes);
                else if ((e = hipMemsetAsync(got[i], 0, m.bytes, stream)) != hipSuccess)
                    break;
            }
        }
        ++i;
    }
    i = 0;
    for (const vsom_buf_member &m : set) {
        if (e != hipSuccess) {
            if (got[i])
                (void)vsom_mem.release(got[i], m.pinned);
        } else {
            *m.p = got[i];
            *m.cap = m.count;
        }
        ++i;
    }
    return e;
}

template <typename T, bool Pinned>
hipError_t vsom_grow(vsom_buf<T, Pinned> &b, size_t count, hipStream_t stream, unsigned flags = 0)
{
    return vsom_grow_set(stream, flags & ~VSOM_BUF_ZERO, {vsom_member(b, count, flags)});
}

struct vsom_layout {
    template <typename T> struct piece { size_t off; };
    size_t bytes = 0;
    unsigned char *base = nullptr;      // the arena this layout is bound to (vsom_arena_ensure)
    template <typename T> piece<T> add(size_t count)
    {
        const piece<T> h{bytes};
        bytes += (count * sizeof(T) + 255) / 256 * 256;
        return h;
    }
    template <typename T> T *at(piece<T> h) const { return base ? reinterpret_cast<T *>(base + h.off) : nullptr; }
};

template <bool Pinned>
hipError_t vsom_arena_ensure(vsom_buf<unsigned char, Pinned> &arena, vsom_layout &lay, hipStream_t stream)
{
    const hipError_t e = vsom_grow(arena, (lay.bytes + 4095) / 4096 * 4096, stream, VSOM_BUF_SYNC);
    lay.base = arena.p;     // (null after a failure)
    return e;
}
