// vsom_ensemble.hip -- many small maps trained by one call (include/vsom_hip.h).
//
// The one-launch kernels of tiny maps (online_tiny_chunk_kernel, tiny_batch_epoch_kernel) are one workgroup on one CU
// and keep every piece of a map's state in LDS and registers.  Their *_many forms run one map per workgroup from a
// descriptor array: the members that would take the one-launch kernel alone are grouped by kernel instantiation, and
// each group is one launch of dim3(members in the group).  Every other member is trained in the same call by its own
// single-context entry point, so any mix of contexts gives the results of the single calls made one by one.
//
// The descriptor array lives in two slots (pinned host image + device copy), used alternately: a slot is rewritten only
// after the event recorded behind its last launch has completed -- the scheme of the pinned neighbourhood-table slots.
#include "vsom_internal.hpp"
#include <algorithm>
#include <cstring>

struct vsom_ensemble {
    int device = 0;
    std::vector<vsom_ctx *> m;
    size_t lds_limit = 0;                    // hipDeviceAttributeMaxSharedMemoryPerBlock of the device
    hipStream_t own_stream = nullptr;        // launch stream when the members' streams differ
    std::vector<hipEvent_t> ev_in;           // behind each distinct member stream's pending work
    struct Slot {
        PinnedBuf<unsigned char> host;       // descriptors staged here, copied to dev
        DevBuf<unsigned char> dev;
        hipEvent_t ev = nullptr;
        bool valid = false;
    } slot[2];
    int next = 0;
    // per call scratch
    std::vector<unsigned char> desc;         // one descriptor per member, packed at the kind's own descriptor size
    std::vector<int> grp, lslot;
    std::vector<size_t> smem;
};

static int ens_fail(size_t k, const char *what)
{
    return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: member " + std::to_string(k) + ": " + what);
}

int vsom_ensemble_create(vsom_ensemble **out, vsom_ctx *const *members, size_t count)
{
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "null output");
    *out = nullptr;
    if (!members || count == 0)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: no members");
    for (size_t k = 0; k < count; ++k) {
        if (!members[k])
            return ens_fail(k, "null context");
        if (members[k]->in_group)
            return ens_fail(k, "a member of a vsom_group");
        if (members[k]->device != members[0]->device)
            return ens_fail(k, "on another device than member 0");
    }
    std::vector<vsom_ctx *> sorted(members, members + count);
    std::sort(sorted.begin(), sorted.end());
    for (size_t k = 1; k < count; ++k)
        if (sorted[k] == sorted[k - 1]) {
            for (size_t i = 0; i < count; ++i)
                if (members[i] == sorted[k])
                    for (size_t j = i + 1; j < count; ++j)
                        if (members[j] == sorted[k])
                            return ens_fail(j, "the same context as an earlier member");
        }
    VSOM_HIP_CHECK(hipSetDevice(members[0]->device));
    int lds = 0;
    VSOM_HIP_CHECK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, members[0]->device));
    vsom_ensemble *e = new vsom_ensemble;
    e->device = members[0]->device;
    e->m.assign(members, members + count);
    e->lds_limit = (size_t)lds;
    *out = e;
    return VSOM_OK;
}

void vsom_ensemble_destroy(vsom_ensemble *e)
{
    if (!e)
        return;
    (void)hipSetDevice(e->device);
    if (e->own_stream)
        (void)hipStreamSynchronize(e->own_stream);
    for (auto &s : e->slot) {
        if (s.valid)
            (void)hipEventSynchronize(s.ev);
        if (s.ev)
            (void)hipEventDestroy(s.ev);
    }
    for (hipEvent_t ev : e->ev_in)
        (void)hipEventDestroy(ev);
    if (e->own_stream)
        (void)hipStreamDestroy(e->own_stream);
    delete e;
}

size_t vsom_ensemble_size(const vsom_ensemble *e) { return e ? e->m.size() : 0; }

// what every train call does for each member first: the bookkeeping of CHECK_CTX (join the side stream; whatever follows
// reads the staged rows, so a later stage-ahead must not take them)
static int join_members(vsom_ensemble *e)
{
    for (vsom_ctx *c : e->m) {
        if (int rc = vsom_join_aux(c))
            return rc;
        c->rows_free_valid = false;
    }
    return VSOM_OK;
}

// the launches of the members whose e->grp[k] >= 0: ready(group) for every group first (nothing is launched unless all
// of them can be), descriptors -- `stride` bytes each, the size the kernel indexes its array by -- into a free slot, the
// launch stream joined to every such member's stream, one launch(group, desc_dev, count, smem) per group.
// *ls_out: the launch stream (null: no launch).  The caller waits for it before it returns, on every path: that wait
// orders whatever is enqueued on a member's stream afterwards behind the launches (so no event joins the member streams
// back), and it is what releases the members' table slots.
template <typename Ready, typename Launch>
static int launch_groups(vsom_ensemble *e, int ngroups, size_t stride, Ready ready, Launch launch, hipStream_t *ls_out)
{
    *ls_out = nullptr;
    const size_t n = e->m.size();
    std::vector<unsigned> cnt(ngroups, 0);
    std::vector<size_t> gsmem(ngroups, 0);
    hipStream_t shared = nullptr;
    bool first = true, same = true;
    for (size_t k = 0; k < n; ++k) {
        const int g = e->grp[k];
        if (g < 0)
            continue;
        ++cnt[g];
        gsmem[g] = std::max(gsmem[g], e->smem[k]);
        if (first)
            shared = e->m[k]->stream;
        else if (e->m[k]->stream != shared)
            same = false;
        first = false;
    }
    if (first)
        return VSOM_OK;                      // no member takes the one-launch kernel
    for (int g = 0; g < ngroups; ++g)
        if (cnt[g])
            if (int rc = ready(g))
                return rc;
    std::vector<size_t> off(ngroups + 1, 0);
    for (int g = 0; g < ngroups; ++g)
        off[g + 1] = off[g] + cnt[g];
    const size_t bytes = off[ngroups] * stride;

    // a free slot: its last launch has completed
    auto &s = e->slot[e->next];
    if (!s.ev)
        VSOM_HIP_CHECK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    if (s.valid)
        VSOM_HIP_CHECK(hipEventSynchronize(s.ev));
    s.valid = false;
    if (bytes > s.host.cap) {
        const size_t cap = std::max(bytes, (size_t)64 * stride);
        VSOM_ALLOC_CHECK(vsom_grow_set(nullptr, VSOM_BUF_REBUILD, {vsom_member(s.host, cap), vsom_member(s.dev, cap)}));
    }
    std::vector<size_t> at(off.begin(), off.end() - 1);
    for (size_t k = 0; k < n; ++k)
        if (e->grp[k] >= 0)
            std::memcpy(s.host.p + (at[e->grp[k]]++) * stride, e->desc.data() + k * stride, stride);

    // the launch stream: the members' one stream, or the ensemble's own behind every member stream's pending work
    hipStream_t ls = shared;
    std::vector<hipStream_t> streams;
    if (!same) {
        if (!e->own_stream)
            VSOM_HIP_CHECK(hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
        ls = e->own_stream;
        for (size_t k = 0; k < n; ++k)
            if (e->grp[k] >= 0)
                streams.push_back(e->m[k]->stream);
        std::sort(streams.begin(), streams.end());
        streams.erase(std::unique(streams.begin(), streams.end()), streams.end());
        while (e->ev_in.size() < streams.size()) {
            hipEvent_t ev = nullptr;
            VSOM_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            e->ev_in.push_back(ev);
        }
        for (size_t i = 0; i < streams.size(); ++i) {
            VSOM_HIP_CHECK(hipEventRecord(e->ev_in[i], streams[i]));
            VSOM_HIP_CHECK(hipStreamWaitEvent(ls, e->ev_in[i], 0));
        }
    }
    *ls_out = ls;
    VSOM_HIP_CHECK(hipMemcpyAsync(s.dev.p, s.host.p, bytes, hipMemcpyHostToDevice, ls));
    for (int g = 0; g < ngroups; ++g)
        if (cnt[g])
            if (int rc = launch(g, s.dev.p + off[g] * stride, cnt[g], gsmem[g], ls))
                return rc;
    VSOM_HIP_CHECK(hipEventRecord(s.ev, ls));
    s.valid = true;
    e->next ^= 1;
    return VSOM_OK;
}

int vsom_ensemble_train_online_chunk_fetch(vsom_ensemble *e, const double *eta, const double *sigma, const int *decay_fn,
                                           int first_chunk, uint64_t *const *lastbmu_out, float *mse_out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (!eta || !sigma || !decay_fn)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null parameter array");
    const size_t n = e->m.size();
    // refusals first: nothing is enqueued for any member unless every member can train
    for (size_t k = 0; k < n; ++k) {
        const vsom_ctx *c = e->m[k];
        if (decay_fn[k] != VSOM_EXPONENTIAL && decay_fn[k] != VSOM_INVERSE_PROPORTIONAL)
            return ens_fail(k, "online training needs Exponential or InverseProportional");
        if (!c->chunk_loaded)
            return ens_fail(k, "no chunk loaded");
        if (c->ahead_rows)
            return ens_fail(k, "the next chunk is staged ahead over the current chunk's rows: vsom_commit_chunk first");
    }
    VSOM_HIP_CHECK(hipSetDevice(e->device));
    if (int rc = join_members(e))
        return rc;
    const size_t stride = vsom_onl_tiny_desc_bytes();
    e->desc.resize(n * stride);
    e->grp.assign(n, -1);
    e->lslot.assign(n, 0);
    e->smem.assign(n, 0);
    for (size_t k = 0; k < n; ++k) {
        vsom_ctx *c = e->m[k];
        if (c->cu)
            continue;                        // custom transformation: its own path
        const bool want_lb = lastbmu_out && lastbmu_out[k];
        if (int rc = vsom_onl_tiny_prepare(c, eta[k], sigma[k], decay_fn[k], first_chunk, want_lb, e->lds_limit,
                                           e->desc.data() + k * stride, &e->grp[k], &e->smem[k], &e->lslot[k]))
            return rc;
    }
    hipStream_t ls = nullptr;
    int rc = launch_groups(
        e, VSOM_ONL_TINY_GROUPS, stride, [&](int g) { return vsom_onl_tiny_ready(g, e->device, e->lds_limit); },
        [&](int g, const void *d, unsigned cnt, size_t smem, hipStream_t s) {
            return vsom_onl_tiny_launch_many(g, d, cnt, smem, s);
        },
        &ls);
    // the other members through their ordinary path, while the launches run
    for (size_t k = 0; k < n && !rc; ++k)
        if (e->grp[k] < 0)
            rc = vsom_train_online_chunk_fetch(e->m[k], eta[k], sigma[k], decay_fn[k], first_chunk,
                                               lastbmu_out ? lastbmu_out[k] : nullptr, mse_out ? mse_out + k : nullptr);
    // (also on an error: a launched member's table slot is released only once its reader has completed)
    if (ls)
        VSOM_HIP_CHECK(hipStreamSynchronize(ls));
    for (size_t k = 0; k < n; ++k)
        if (e->grp[k] >= 0 && ls)
            vsom_onl_tiny_done(e->m[k], e->lslot[k]);
    if (rc)
        return rc;
    // results of the launched members: the kernels stored them into each member's pinned words
    for (size_t k = 0; k < n; ++k) {
        if (e->grp[k] < 0)
            continue;
        vsom_ctx *c = e->m[k];
        if (lastbmu_out && lastbmu_out[k])
            std::memcpy(lastbmu_out[k], c->out_pinned.p, c->B * sizeof(uint64_t));
        if (mse_out)
            mse_out[k] = *static_cast<volatile float *>(c->mse.p);
    }
    return VSOM_OK;
}

int vsom_ensemble_batch_epoch(vsom_ensemble *e, const double *sigma, int is_first, float *mse_out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (!sigma)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null parameter array");
    const size_t n = e->m.size();
    for (size_t k = 0; k < n; ++k) {
        const vsom_ctx *c = e->m[k];
        if (!c->chunk_loaded)
            return ens_fail(k, "no chunk loaded");
        if (c->ahead_rows)
            return ens_fail(k, "the next chunk is staged ahead over the current chunk's rows: vsom_commit_chunk first");
    }
    VSOM_HIP_CHECK(hipSetDevice(e->device));
    if (int rc = join_members(e))
        return rc;
    const size_t stride = vsom_tiny_desc_bytes();
    e->desc.resize(n * stride);
    e->grp.assign(n, -1);
    e->smem.assign(n, 0);
    for (size_t k = 0; k < n; ++k) {
        vsom_ctx *c = e->m[k];
        if (c->cu)
            continue;
        // (no attribute is raised for the batch kernels: they may ask for the default 64 KiB at most)
        if (int rc = vsom_tiny_prepare(c, sigma[k], is_first, std::min(e->lds_limit, (size_t)64 << 10),
                                       e->desc.data() + k * stride, &e->grp[k], &e->smem[k]))
            return rc;
    }
    hipStream_t ls = nullptr;
    int rc = launch_groups(
        e, VSOM_TINY_GROUPS, stride, [](int) { return VSOM_OK; },
        [&](int g, const void *d, unsigned cnt, size_t smem, hipStream_t s) { return vsom_tiny_launch_many(g, d, cnt, smem, s); },
        &ls);
    for (size_t k = 0; k < n && !rc; ++k)
        if (e->grp[k] < 0)
            rc = vsom_batch_epoch(e->m[k], sigma[k], is_first, mse_out ? mse_out + k : nullptr);
    if (ls)
        VSOM_HIP_CHECK(hipStreamSynchronize(ls));
    if (rc)
        return rc;
    for (size_t k = 0; k < n; ++k)
        if (e->grp[k] >= 0 && mse_out)
            mse_out[k] = *static_cast<volatile float *>(e->m[k]->mse.p);
    return VSOM_OK;
}
