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
//
// The calls around training are batched the same way.  vsom_ensemble_upload_chunks copies the union of the members' row
// ranges with one H2D copy into the ensemble's raw buffer and stages every plain member's rows with one launch of
// stage_rows_many_kernel (one workgroup per (member, 16 rows)); members whose chunk gets the column compaction, CLR members
// and those with no rows are staged by their single-context path from that device copy, custom members by their own
// upload.  vsom_ensemble_bmu_batch scores every tiny member with one launch of ensemble_bmu_many_kernel<kind> per kind
// (one workgroup per (member, 64 rows)): the exact search of the one-launch batch epoch's phase 1, whose results the
// kernel also stores into one pinned buffer for all members; every other member runs vsom_bmu_batch in the same call.
// vsom_ensemble_bmu_masked_batch and vsom_ensemble_similarity_masked_batch are the same shape over the valid columns only
// (DESIGN.md section 4v): one launch of ensemble_masked_many_kernel<kind, score> per kind, the search of that kernel on the
// masked distance followed in the same workgroup by a per-row epilogue (nvalid, the imputed row, the similarity words).
// vsom_ensemble_bmu_topk_batch and vsom_ensemble_bmu_topk_masked_batch keep, in the same workgroup
// shape, each row's k smallest keys as a sorted list in LDS: one launch of ensemble_topk_many_kernel<kind, masked> per kind.
// vsom_ensemble_evaluate_batch and vsom_ensemble_evaluate_masked_batch run the search and, in the same
// workgroup, evaluate_kernel's row scoring against the unit's row in LDS: ensemble_evaluate_many_kernel<kind, masked>.
#include "vsom_masked_dist.hpp"
#include "vsom_sim_row.hpp"
#include "vsom_eval_row.hpp"
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
        // what the launch reads besides the descriptors -- a schedule round's image (vsom_sched_round.hpp), the online
        // chunk's validity bytes -- copied once on the launch stream; reused under the same event as the descriptors
        PinnedBuf<unsigned char> img_host;
        DevBuf<unsigned char> img_dev;
        hipEvent_t ev = nullptr;
        bool valid = false;
    } slot[2];
    int next = 0;
    // per call scratch
    std::vector<unsigned char> desc;         // one descriptor per member, packed at the kind's own descriptor size
    std::vector<int> grp;
    std::vector<size_t> smem;
    std::vector<unsigned> ext;               // the grid's other dimension: 16-row blocks (staging), 64-row tiles (scoring)
    // upload: the members' rows as one copy of the host range (grow-only); ev_raw is recorded behind the call's last
    // reader of it (the staging launch, and -- joined back into the launch stream -- the ordinary stagings)
    DevBuf<float> raw;
    hipEvent_t ev_raw = nullptr, ev_stage = nullptr;
    bool raw_valid = false;
    // scoring: idx / dist of every launched member, stored by the kernel (pinned host memory, grow-only)
    PinnedBuf<u64> sc_idx;
    PinnedBuf<float> sc_dist;
    // U-matrices of the launched members, stored by the kernel (pinned host memory, grow-only)
    PinnedBuf<double> um_out;
    // the masked queries: the per-row words of every launched member (arrays of B entries, vsom_similarity.hip's order) and
    // the dense rows (fill / delta, B x J) of those that asked for them, stored by the kernel (pinned, grow-only; one set
    // for both calls)
    PinnedBuf<unsigned> mq_rows;
    PinnedBuf<float> mq_dense;
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
    for (size_t k = 0; k < count; ++k)
        if (int rc = vsom_sigma_flush_pending(members[k]))
            return rc;
    vsom_ensemble *e = new vsom_ensemble;
    e->device = members[0]->device;
    e->m.assign(members, members + count);
    e->lds_limit = (size_t)lds;
    // The ensemble's calls read the members' sigmaMap rows directly, so from here on (nothing above is left to fail) a
    // member's epochs keep sigmaMap current.  The flag outlives the ensemble: vsom_ensemble_destroy may run after its
    // members are gone and cannot touch them (include/vsom_hip.h, vsom_set_sigma_mode, says so).
    for (vsom_ctx *c : e->m)
        c->sigma_shared = true;
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
    if (e->raw_valid)
        (void)hipEventSynchronize(e->ev_raw);
    for (hipEvent_t ev : {e->ev_raw, e->ev_stage})
        if (ev)
            (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->ev_in)
        (void)hipEventDestroy(ev);
    if (e->own_stream)
        (void)hipStreamDestroy(e->own_stream);
    delete e;
}

size_t vsom_ensemble_size(const vsom_ensemble *e) { return e ? e->m.size() : 0; }

// why a call that reads the staged rows refuses a member, or null
static const char *ens_rows_refusal(const vsom_ctx *c)
{
    if (!c->chunk_loaded)
        return "no chunk loaded";
    if (c->ahead_rows)
        return "the next chunk is staged ahead over the current chunk's rows: vsom_commit_chunk first";
    return nullptr;
}

// what every call does first for each member (`only`: for those with only[k] != 0): the bookkeeping of CHECK_CTX -- join
// the side stream and, where the call reads the staged rows, keep a later stage-ahead from taking them
static int join_members(vsom_ensemble *e, const size_t *only, bool reads_rows)
{
    for (size_t k = 0; k < e->m.size(); ++k) {
        if (only && !only[k])
            continue;
        if (int rc = vsom_join_aux(e->m[k]))
            return rc;
        if (reads_rows)
            e->m[k]->rows_free_valid = false;
    }
    return VSOM_OK;
}

// the per-member inputs of ens_launch, cleared: no member is launched
static void ens_scratch(vsom_ensemble *e, size_t stride)
{
    const size_t n = e->m.size();
    e->desc.resize(n * stride);
    e->grp.assign(n, -1);
    e->smem.assign(n, 0);
    e->ext.assign(n, 0);
}

// whose streams the launch stream runs behind: the members of the call's launches, or every member but the custom ones
// (an event record per distinct stream: the smaller set where it is enough); ENS_JOINED: the caller has joined already
enum EnsSet { ENS_LAUNCHED, ENS_PLAIN, ENS_JOINED };

// What one call enqueues for the ensemble, and the one way out of that call.  Declared before the call's first enqueue:
// whichever return leaves the scope -- a failed HIP call or allocation, a member's rc -- waits for the launch stream
// first (end() on the ordinary way and reports the wait's status; the destructor on every other, where the status that
// is returned is the first failure's).  That wait orders whatever is enqueued on a member's stream afterwards behind the
// launches (so no event joins the member streams back), and it is what releases the members' table slots.
struct EnsCall {
    vsom_ensemble *e;
    hipStream_t ls = nullptr;                // the launch stream (null: nothing joined or launched yet)
    std::vector<hipStream_t> streams;        // the distinct streams of the last join
    std::vector<std::pair<vsom_ctx *, int>> held;   // online training: the launched members' table slots, released by wait()
    bool open = true;
    explicit EnsCall(vsom_ensemble *ens) : e(ens) {}
    EnsCall(const EnsCall &) = delete;
    ~EnsCall()
    {
        if (open)
            (void)wait(true);
    }
    // the launch stream: the set's one stream (the fast form: no events), or the ensemble's own behind the pending work
    // of every stream of the set.  May be repeated: new work on the member streams is joined in.
    int join(EnsSet set)
    {
        streams.clear();
        for (size_t k = 0; k < e->m.size(); ++k)
            if ((set == ENS_LAUNCHED ? e->grp[k] >= 0 : !e->m[k]->cu) &&
                (streams.empty() || streams.back() != e->m[k]->stream))
                streams.push_back(e->m[k]->stream);
        if (streams.size() > 1) {            // (one stream, or runs of a few, need no sort)
            std::sort(streams.begin(), streams.end());
            streams.erase(std::unique(streams.begin(), streams.end()), streams.end());
        }
        if (streams.size() <= 1) {
            if (!streams.empty())
                ls = streams[0];
            return VSOM_OK;
        }
        if (!e->own_stream)
            VSOM_HIP_CHECK(hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
        ls = e->own_stream;
        while (e->ev_in.size() < streams.size()) {
            hipEvent_t ev = nullptr;
            VSOM_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            e->ev_in.push_back(ev);
        }
        for (size_t i = 0; i < streams.size(); ++i) {
            VSOM_HIP_CHECK(hipEventRecord(e->ev_in[i], streams[i]));
            VSOM_HIP_CHECK(hipStreamWaitEvent(ls, e->ev_in[i], 0));
        }
        return VSOM_OK;
    }
    // the host wait that ends the call.  failed: something may be left on the joined member streams as well (an upload's
    // ordinary stagings read e->raw there), so they are drained too and e->raw has no reader that ev_raw does not cover.
    hipError_t wait(bool failed)
    {
        open = false;
        hipError_t err = hipSuccess;
        auto sync = [&err](hipStream_t s) {
            const hipError_t x = s ? hipStreamSynchronize(s) : hipSuccess;
            if (err == hipSuccess)
                err = x;
        };
        if (failed)
            for (hipStream_t s : streams)
                sync(s);
        sync(ls);
        // (also on an error: a launched member's table slot is released only once its reader has completed)
        for (size_t i = 0; i < held.size() && ls; ++i)
            vsom_onl_tiny_done(held[i].first, held[i].second);
        return err;
    }
    int end(int rc)
    {
        const hipError_t err = wait(rc != VSOM_OK);
        if (rc)
            return rc;                       // (the first failure is the one reported)
        VSOM_HIP_CHECK_AS(err, "hipStreamSynchronize(ls)");
        return VSOM_OK;
    }
    void detach() { open = false; }          // (the asynchronous upload: its success returns without a host wait)
};

// The launches of the members whose e->grp[k] >= 0, from the per-member inputs the caller has filled: e->grp (the group),
// e->desc (`stride` bytes each, the size the kernel indexes its array by), e->smem (the LDS need) and e->ext (the extent
// on the grid's other dimension, where the kernel has one).  ready(group) for every group first (nothing is launched
// unless all of them can be), the launch stream joined to the streams of `set`, the descriptors sorted by group into a
// free slot and sent, then launch(group, desc_dev, count, smem, ext, ls) per group with the group's largest smem and
// ext -- in slices of at most `cap` members, the bound of the grid dimension the members sit on.
constexpr unsigned ENS_NO_CAP = ~0u;         // members on grid.x
static int ens_always_ready(int) { return VSOM_OK; }

template <typename Ready, typename Launch>
static int ens_launch(EnsCall &call, EnsSet set, int ngroups, size_t stride, unsigned cap, Ready ready, Launch launch)
{
    vsom_ensemble *e = call.e;
    const size_t n = e->m.size();
    std::vector<size_t> off(ngroups + 1, 0), gsmem(ngroups, 0);
    std::vector<unsigned> gext(ngroups, 0);
    for (size_t k = 0; k < n; ++k) {
        const int g = e->grp[k];
        if (g < 0)
            continue;
        ++off[g + 1];
        gsmem[g] = std::max(gsmem[g], e->smem[k]);
        gext[g] = std::max(gext[g], e->ext[k]);
    }
    for (int g = 0; g < ngroups; ++g) {
        if (off[g + 1])
            if (int rc = ready(g))
                return rc;
        off[g + 1] += off[g];
    }
    if (off[ngroups] == 0)
        return VSOM_OK;                      // no member is launched
    if (set != ENS_JOINED)
        if (int rc = call.join(set))
            return rc;
    hipStream_t ls = call.ls;

    // a free slot: its last launch has completed
    auto &s = e->slot[e->next];
    if (!s.ev)
        VSOM_HIP_CHECK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    if (s.valid)
        VSOM_HIP_CHECK(hipEventSynchronize(s.ev));
    s.valid = false;
    const size_t bytes = off[ngroups] * stride;
    if (bytes > s.host.cap) {
        const size_t grown = std::max(bytes, (size_t)64 * stride);
        VSOM_ALLOC_CHECK(vsom_grow_set(nullptr, VSOM_BUF_REBUILD, {vsom_member(s.host, grown), vsom_member(s.dev, grown)}));
    }
    std::vector<size_t> at(off.begin(), off.end() - 1);
    for (size_t k = 0; k < n; ++k)
        if (e->grp[k] >= 0)
            std::memcpy(s.host.p + (at[e->grp[k]]++) * stride, e->desc.data() + k * stride, stride);
    VSOM_HIP_CHECK(hipMemcpyAsync(s.dev.p, s.host.p, bytes, hipMemcpyHostToDevice, ls));
    for (int g = 0; g < ngroups; ++g)
        for (size_t i = off[g]; i < off[g + 1]; i += cap) {
            const unsigned cnt = (unsigned)std::min(off[g + 1] - i, (size_t)cap);
            if (int rc = launch(g, s.dev.p + i * stride, cnt, gsmem[g], gext[g], ls))
                return rc;
        }
    VSOM_HIP_CHECK(hipEventRecord(s.ev, ls));
    s.valid = true;
    e->next ^= 1;
    return VSOM_OK;
}

// The online chunk of every member, plain or with validity (DESIGN.md sections 4c, 4u); valid_host null: no member has
// validity bytes.  Up to two ens_launch passes on one launch stream, each with its own descriptor slot: the plain members
// that take online_tiny_chunk_many_kernel, then the masked members that take online_tiny_masked_chunk_many_kernel, whose
// validity bytes form one pinned image in the second pass's slot, copied once.  Every other member runs its single call
// while the launches run.  The callers have made their argument checks.
static int ens_online_chunk(vsom_ensemble *e, const double *eta, const double *sigma, const int *decay_fn, int first_chunk,
                            const uint8_t *const *valid_host, const int *one_mask, uint64_t *const *lastbmu_out,
                            float *mse_out)
{
    const size_t n = e->m.size();
    VSOM_HIP_CHECK(hipSetDevice(e->device));
    EnsCall call(e);
    if (int rc = join_members(e, nullptr, true))
        return rc;
    // who is launched: 1 = a plain member on the one-launch chunk (prepared here), 2 = a masked one
    const size_t pstride = vsom_onl_tiny_desc_bytes(false), mstride = vsom_onl_tiny_desc_bytes(true);
    std::vector<int> how(n, 0);
    std::vector<size_t> v_at(n, 0), vbytes(n, 0);
    size_t vtotal = 0;
    bool any_plain = false, any_masked = false;
    ens_scratch(e, pstride);
    for (size_t k = 0; k < n; ++k) {
        vsom_ctx *c = e->m[k];
        const bool masked = valid_host && valid_host[k];
        if (!vsom_onl_tiny_fits(c, sigma[k], masked, e->lds_limit))
            continue;                        // (a custom transformation among them): its own path
        if (!masked) {
            int lslot = 0;
            if (int rc = vsom_onl_tiny_prepare(c, eta[k], sigma[k], decay_fn[k], first_chunk, lastbmu_out && lastbmu_out[k],
                                               nullptr, 0, e->desc.data() + k * pstride, &e->grp[k], &e->smem[k], &lslot))
                return rc;
            how[k] = 1;
            any_plain = true;
            call.held.emplace_back(c, lslot);
        } else {
            how[k] = 2;
            any_masked = true;
            vbytes[k] = ((one_mask && one_mask[k]) ? 1 : c->B) * (size_t)c->J;
            v_at[k] = vtotal;
            vtotal += (vbytes[k] + 15) / 16 * 16;
        }
    }
    int rc = VSOM_OK;
    if (any_plain || any_masked) {
        // one launch stream behind every launched member's stream, for both passes
        std::vector<int> pgrp;
        if (any_masked) {
            pgrp = e->grp;
            for (size_t k = 0; k < n; ++k)
                if (how[k] == 2)
                    e->grp[k] = 0;
        }
        if (int jrc = call.join(ENS_LAUNCHED))
            return jrc;
        if (any_masked)
            e->grp = pgrp;
    }
    if (any_plain)
        rc = ens_launch(
            call, ENS_JOINED, VSOM_ONL_TINY_GROUPS, pstride, ENS_NO_CAP,
            [&](int g) { return vsom_onl_tiny_ready(false, g, e->device, e->lds_limit); },
            [](int g, const void *d, unsigned cnt, size_t smem, unsigned, hipStream_t s) {
                return vsom_onl_tiny_launch_many(false, g, d, cnt, smem, s);
            });
    if (any_masked && !rc) {
        // the slot ens_launch is about to take: its last launch has completed, so its image may be rewritten
        auto &s = e->slot[e->next];
        if (s.valid)
            VSOM_HIP_CHECK(hipEventSynchronize(s.ev));
        VSOM_ALLOC_CHECK(vsom_grow_set(nullptr, 0, {vsom_member(s.img_host, vtotal), vsom_member(s.img_dev, vtotal)}));
        for (size_t k = 0; k < n; ++k)
            if (how[k] == 2)
                std::memcpy(s.img_host.p + v_at[k], valid_host[k], vbytes[k]);
        VSOM_HIP_CHECK(hipMemcpyAsync(s.img_dev.p, s.img_host.p, vtotal, hipMemcpyHostToDevice, call.ls));
        ens_scratch(e, mstride);
        for (size_t k = 0; k < n && !rc; ++k) {
            if (how[k] != 2)
                continue;
            vsom_ctx *c = e->m[k];
            int lslot = 0;
            rc = vsom_onl_tiny_prepare(c, eta[k], sigma[k], decay_fn[k], first_chunk, lastbmu_out && lastbmu_out[k],
                                       s.img_dev.p + v_at[k], one_mask ? one_mask[k] : 0, e->desc.data() + k * mstride,
                                       &e->grp[k], &e->smem[k], &lslot);
            if (!rc)
                call.held.emplace_back(c, lslot);
        }
        if (!rc)
            rc = ens_launch(
                call, ENS_JOINED, VSOM_ONL_TINY_GROUPS, mstride, ENS_NO_CAP,
                [&](int g) { return vsom_onl_tiny_ready(true, g, e->device, e->lds_limit); },
                [](int g, const void *d, unsigned cnt, size_t smem, unsigned, hipStream_t st) {
                    return vsom_onl_tiny_launch_many(true, g, d, cnt, smem, st);
                });
    }
    // the other members through their single calls, while the launches run
    for (size_t k = 0; k < n && !rc; ++k) {
        if (how[k])
            continue;
        uint64_t *lb = lastbmu_out ? lastbmu_out[k] : nullptr;
        float *mse = mse_out ? mse_out + k : nullptr;
        rc = valid_host && valid_host[k]
                 ? vsom_online_chunk_masked_member(e->m[k], eta[k], sigma[k], decay_fn[k], first_chunk, valid_host[k],
                                                   one_mask ? one_mask[k] : 0, lb, mse)
                 : vsom_train_online_chunk_fetch(e->m[k], eta[k], sigma[k], decay_fn[k], first_chunk, lb, mse);
    }
    if ((rc = call.end(rc)))
        return rc;
    // results of the launched members: the kernels stored them into each member's pinned words
    for (size_t k = 0; k < n; ++k) {
        if (!how[k])
            continue;
        vsom_ctx *c = e->m[k];
        if (lastbmu_out && lastbmu_out[k])
            std::memcpy(lastbmu_out[k], c->out_pinned.p, c->B * sizeof(uint64_t));
        if (mse_out)
            mse_out[k] = *static_cast<volatile float *>(c->mse.p);
    }
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
        if (const char *why = ens_rows_refusal(c))
            return ens_fail(k, why);
    }
    return ens_online_chunk(e, eta, sigma, decay_fn, first_chunk, nullptr, nullptr, lastbmu_out, mse_out);
}

int vsom_ensemble_train_online_chunk_masked(vsom_ensemble *e, const double *eta, const double *sigma, const int *decay_fn,
                                            int first_chunk, const uint8_t *const *valid_host, const int *one_mask,
                                            uint64_t *const *lastbmu_out, float *mse_out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (!eta || !sigma || !decay_fn)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null parameter array");
    if (!valid_host)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null valid_host array");
    const size_t n = e->m.size();
    // refusals first: nothing is enqueued for any member unless every member can train
    for (size_t k = 0; k < n; ++k) {
        const vsom_ctx *c = e->m[k];
        if (decay_fn[k] != VSOM_EXPONENTIAL && decay_fn[k] != VSOM_INVERSE_PROPORTIONAL)
            return ens_fail(k, "online training needs Exponential or InverseProportional");
        if (valid_host[k] && c->cu)
            return ens_fail(k, "vsom_train_online_chunk_masked: custom contexts are not supported");
        if (valid_host[k] && c->transform == VSOM_CLR)
            return ens_fail(k, "vsom_train_online_chunk_masked: CLR contexts are not supported (residual and step run over column pairs)");
        if (const char *why = ens_rows_refusal(c))
            return ens_fail(k, why);
    }
    return ens_online_chunk(e, eta, sigma, decay_fn, first_chunk, valid_host, one_mask, lastbmu_out, mse_out);
}

int vsom_ensemble_batch_epoch(vsom_ensemble *e, const double *sigma, int is_first, float *mse_out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (!sigma)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null parameter array");
    const size_t n = e->m.size();
    for (size_t k = 0; k < n; ++k)
        if (const char *why = ens_rows_refusal(e->m[k]))
            return ens_fail(k, why);
    VSOM_HIP_CHECK(hipSetDevice(e->device));
    EnsCall call(e);
    if (int rc = join_members(e, nullptr, true))
        return rc;
    const size_t stride = vsom_tiny_desc_bytes();
    ens_scratch(e, stride);
    for (size_t k = 0; k < n; ++k) {
        vsom_ctx *c = e->m[k];
        if (c->cu)
            continue;
        // (no attribute is raised for the batch kernels: they may ask for the default 64 KiB at most)
        if (int rc = vsom_tiny_prepare(c, sigma[k], is_first, std::min(e->lds_limit, (size_t)64 << 10),
                                       e->desc.data() + k * stride, &e->grp[k], &e->smem[k]))
            return rc;
    }
    int rc = ens_launch(call, ENS_LAUNCHED, VSOM_TINY_GROUPS, stride, ENS_NO_CAP, ens_always_ready,
                        [](int g, const void *d, unsigned cnt, size_t smem, unsigned, hipStream_t s) {
                            return vsom_tiny_launch_many(g, d, cnt, smem, s);
                        });
    for (size_t k = 0; k < n && !rc; ++k)
        if (e->grp[k] < 0)
            rc = vsom_batch_epoch(e->m[k], sigma[k], is_first, mse_out ? mse_out + k : nullptr);
    if ((rc = call.end(rc)))
        return rc;
    for (size_t k = 0; k < n; ++k)
        if (e->grp[k] >= 0 && mse_out)
            mse_out[k] = *static_cast<volatile float *>(e->m[k]->mse.p);
    return VSOM_OK;
}

// The schedule calls (DESIGN.md sections 4m, 4t), one routine over the flavour of the launched members: plain
// (vsom_ensemble_batch_schedule: the members on the fast path of vsom_batch_schedule) or masked (the masked train calls:
// the members with validity bytes on the fast path of vsom_batch_schedule_masked; an epoch is a schedule of one epoch whose
// `first` is the call's is_first).  They go as rounds of at most VSOM_SCHEDULE_MAX_EPOCHS epochs, one launch per kind and
// round, each workgroup looping its own count; the round's image (vsom_sched_round.hpp: tables, every member's table
// offsets, the masked members' validity bytes) is pinned in the round's descriptor slot and copied once on the launch
// stream, so a round is ordered behind the one two before it by the slot's event and nothing else waits between rounds.
// Every other member -- off the fast path, or a plain one in a masked call (valid_host[k] null) -- runs single(k), its
// single-context call, in the same call.  `what`: the entry point, for the refusal's text.
template <typename Single>
static int ens_schedule_train(vsom_ensemble *e, bool masked, const char *what, const double *const *sigma,
                              const size_t *epochs, int first, int reset_bmu, const uint8_t *const *valid_host,
                              const int *one_mask, float *const *mse_out, Single single)
{
    const size_t n = e->m.size();
    VSOM_HIP_CHECK(hipSetDevice(e->device));
    EnsCall call(e);
    if (int rc = join_members(e, epochs, true))   // (a member without epochs is not touched)
        return rc;
    // who is launched
    const size_t lds_cap = std::min(e->lds_limit, (size_t)64 << 10);   // (no attribute is raised for the batch kernels)
    std::vector<int> kind(n, -1);
    std::vector<VsomSchedMember> mem(n);
    size_t longest = 0;
    bool any = false;
    for (size_t k = 0; k < n; ++k) {
        vsom_ctx *c = e->m[k];
        const int one = masked && one_mask ? one_mask[k] : 0;
        mem[k] = VsomSchedMember{0, 0, nullptr, 0, nullptr, 0};
        if (!epochs[k])
            continue;
        if (masked ? !valid_host[k] || !vsom_tiny_masked_schedule_applies(c, one, sigma[k], epochs[k], lds_cap)
                   : !vsom_tiny_schedule_applies(c, sigma[k], epochs[k], lds_cap))
            continue;
        kind[k] = c->transform;
        vsom_lut_dims(c, &mem[k].lw, &mem[k].lh);
        if (masked) {
            mem[k].valid = valid_host[k];
            mem[k].vbytes = (one ? 1 : c->B) * (size_t)c->J;
        }
        longest = std::max(longest, epochs[k]);
        any = true;
    }
    int rc = VSOM_OK;
    if (any) {
        for (size_t k = 0; k < n; ++k)
            if (kind[k] >= 0)
                VSOM_ALLOC_CHECK(vsom_grow(e->m[k]->sch_mse, epochs[k], e->m[k]->stream, VSOM_BUF_SYNC));
        const size_t stride = masked ? vsom_tiny_masked_sched_desc_bytes() : vsom_tiny_sched_desc_bytes();
        VsomSchedRound round;
        for (size_t e0 = 0; e0 < longest && !rc; e0 += VSOM_SCHEDULE_MAX_EPOCHS) {
            for (size_t k = 0; k < n; ++k)
                if (kind[k] >= 0) {
                    mem[k].sigma = sigma[k] + std::min(e0, epochs[k]);
                    mem[k].epochs = epochs[k] > e0 ? std::min(epochs[k] - e0, (size_t)VSOM_SCHEDULE_MAX_EPOCHS) : 0;
                }
            if (!round.plan(mem.data(), n)) {
                rc = vsom_fail(VSOM_ERR_INVALID, std::string(what) + ": the tables of one round exceed 2^32 values");
                break;
            }
            // (a member whose schedule has ended stays in the launches with no epochs: every round then has the same
            //  launch stream, and the rounds stay ordered)
            ens_scratch(e, stride);
            for (size_t k = 0; k < n; ++k)
                e->grp[k] = kind[k];
            if (int jrc = call.join(ENS_LAUNCHED))
                return jrc;
            // the slot ens_launch is about to take: its last launch has completed, so its image may be rewritten
            auto &s = e->slot[e->next];
            if (s.valid)
                VSOM_HIP_CHECK(hipEventSynchronize(s.ev));
            const size_t bytes = round.bytes();
            VSOM_ALLOC_CHECK(vsom_grow_set(nullptr, 0, {vsom_member(s.img_host, bytes), vsom_member(s.img_dev, bytes)}));
            round.write(s.img_host.p, mem.data());
            VSOM_HIP_CHECK(hipMemcpyAsync(s.img_dev.p, s.img_host.p, bytes, hipMemcpyHostToDevice, call.ls));
            const float *lut_dev = reinterpret_cast<const float *>(s.img_dev.p);
            const unsigned *tab_dev = reinterpret_cast<const unsigned *>(s.img_dev.p + round.table_bytes());
            const unsigned char *v_dev = s.img_dev.p + round.table_bytes() + round.offset_bytes();
            for (size_t k = 0; k < n; ++k) {
                if (kind[k] < 0)
                    continue;
                vsom_ctx *c = e->m[k];
                const size_t cnt = mem[k].epochs;
                const unsigned *tab_k = tab_dev + (cnt ? round.tab_at[k] : 0);
                float *mse_k = c->sch_mse.p + (cnt ? e0 : 0);
                void *desc = e->desc.data() + k * stride;
                if (masked)
                    vsom_tiny_masked_sched_fill(c, v_dev + (cnt ? round.v_at[k] : 0), one_mask ? one_mask[k] : 0, lds_cap,
                                                lut_dev, tab_k, mse_k, cnt, e0 == 0 && first, reset_bmu, desc, &e->smem[k]);
                else
                    vsom_tiny_sched_fill(c, lut_dev, tab_k, mse_k, cnt, e0 == 0 && first, reset_bmu, desc, &e->smem[k]);
            }
            rc = ens_launch(call, ENS_JOINED, VSOM_TINY_GROUPS, stride, ENS_NO_CAP, ens_always_ready,
                            [masked](int g, const void *d, unsigned cnt, size_t smem, unsigned, hipStream_t st) {
                                return masked ? vsom_tiny_masked_sched_launch_many(g, d, cnt, smem, st)
                                              : vsom_tiny_sched_launch_many(g, d, cnt, smem, st);
                            });
        }
    }
    // the other members through their single calls, while the launches run
    for (size_t k = 0; k < n && !rc; ++k)
        if (kind[k] < 0 && epochs[k])
            rc = single(k);
    if ((rc = call.end(rc)))
        return rc;
    for (size_t k = 0; k < n; ++k)
        if (kind[k] >= 0)
            vsom_schedule_results(e->m[k], epochs[k], mse_out[k]);
    return VSOM_OK;
}

int vsom_ensemble_batch_schedule(vsom_ensemble *e, const double *const *sigma, const size_t *epochs, int reset_bmu,
                                 float *const *mse_out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (!epochs)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null epochs array");
    const size_t n = e->m.size();
    for (size_t k = 0; k < n; ++k) {
        if (!epochs[k])
            continue;                        // not touched
        if (!sigma || !mse_out || !sigma[k] || !mse_out[k])
            return ens_fail(k, "null sigma or mse_out with epochs > 0");
        if (const char *why = vsom_schedule_refusal(e->m[k]))
            return ens_fail(k, why);
    }
    // the members off the fast path through the sequence of single epochs
    return ens_schedule_train(e, false, "vsom_ensemble_batch_schedule", sigma, epochs, 1, reset_bmu, nullptr, nullptr, mse_out,
                              [&](size_t k) {
                                  return vsom_schedule_loop(e->m[k], epochs[k], reset_bmu, [&](size_t ep) {
                                      return vsom_batch_epoch(e->m[k], sigma[k][ep], ep == 0, &mse_out[k][ep]);
                                  });
                              });
}

// what both masked forms refuse for member k (its chunk, and for a masked member its kind), or null
static const char *ens_masked_refusal(const vsom_ctx *c, const uint8_t *valid)
{
    if (const char *why = vsom_schedule_refusal(c))
        return why;
    return valid ? vsom_masked_train_refusal(c) : nullptr;
}

int vsom_ensemble_batch_epoch_masked(vsom_ensemble *e, const double *sigma, int is_first, const uint8_t *const *valid_host,
                                     const int *one_mask, float *mse_out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (!sigma)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null parameter array");
    if (!valid_host)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null valid_host array");
    const size_t n = e->m.size();
    for (size_t k = 0; k < n; ++k)
        if (const char *why = ens_masked_refusal(e->m[k], valid_host[k]))
            return ens_fail(k, why);
    // every member a schedule of one epoch; the MSEs land in a local array (mse_out may be null)
    std::vector<const double *> sig(n);
    std::vector<size_t> epochs(n, 1);
    std::vector<float> mse(n, 0.f);
    std::vector<float *> msep(n);
    for (size_t k = 0; k < n; ++k) {
        sig[k] = sigma + k;
        msep[k] = &mse[k];
    }
    const int rc = ens_schedule_train(e, true, "vsom_ensemble", sig.data(), epochs.data(), is_first ? 1 : 0, 0, valid_host,
                                      one_mask, msep.data(), [&](size_t k) {
                                          return valid_host[k] ? vsom_batch_epoch_masked(e->m[k], sigma[k], is_first, valid_host[k],
                                                                                         one_mask ? one_mask[k] : 0, msep[k])
                                                               : vsom_batch_epoch(e->m[k], sigma[k], is_first, msep[k]);
                                      });
    if (rc)
        return rc;
    if (mse_out)
        std::copy(mse.begin(), mse.end(), mse_out);
    return VSOM_OK;
}

int vsom_ensemble_batch_schedule_masked(vsom_ensemble *e, const double *const *sigma, const size_t *epochs, int reset_bmu,
                                        const uint8_t *const *valid_host, const int *one_mask, float *const *mse_out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (!epochs)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null epochs array");
    if (!valid_host)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null valid_host array");
    const size_t n = e->m.size();
    for (size_t k = 0; k < n; ++k) {
        if (!epochs[k])
            continue;                        // not touched
        if (!sigma || !mse_out || !sigma[k] || !mse_out[k])
            return ens_fail(k, "null sigma or mse_out with epochs > 0");
        if (const char *why = ens_masked_refusal(e->m[k], valid_host[k]))
            return ens_fail(k, why);
    }
    return ens_schedule_train(e, true, "vsom_ensemble", sigma, epochs, 1, reset_bmu, valid_host, one_mask, mse_out, [&](size_t k) {
        return valid_host[k] ? vsom_batch_schedule_masked(e->m[k], sigma[k], epochs[k], reset_bmu, valid_host[k],
                                                          one_mask ? one_mask[k] : 0, mse_out[k])
                             : vsom_batch_schedule(e->m[k], sigma[k], epochs[k], reset_bmu, mse_out[k]);
    });
}

// ================================================================================================================
// upload and scoring
// ================================================================================================================
// one member's rows for stage_rows_many_kernel: stage_rows_kernel's arguments without the compaction flags (members whose
// chunk gets the compaction take the single-context staging)
struct EnsStageDesc {
    const float *x;          // B x J raw rows in the ensemble's copy
    float *xs;
    u64 *lastbmu;
    unsigned *xflag;         // the integer shortlist's data-kind word, or null
    int J, B, xpitch, pad;
};

// stage_rows_kernel's work for every member in one launch: workgroup (x, y) = rows [16x, 16x + 16) of member y
__global__ __launch_bounds__(256) void stage_rows_many_kernel(const EnsStageDesc *__restrict__ descs)
{
    const EnsStageDesc a = descs[blockIdx.y];
    const int r0 = blockIdx.x * 16;
    if (r0 >= a.B)
        return;                                          // (workgroup-uniform: the grid covers the longest chunk)
    const int r1 = r0 + 16 < a.B ? r0 + 16 : a.B;
    if (threadIdx.x < 16 && r0 + (int)threadIdx.x < a.B)
        a.lastbmu[r0 + threadIdx.x] = 0;                 // DataSet.cpp:136-137
    if (a.xflag && blockIdx.x == 0 && threadIdx.x < 33)
        a.xflag[32 * threadIdx.x] = 0u;                  // the word and its 32 write slots (vsom_sl_i8.hip)
    for (int d = threadIdx.x; d < a.xpitch; d += 256) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            v[i] = (d < a.J && r0 + i < r1) ? a.x[(size_t)(r0 + i) * a.J + d] : 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (r0 + i < r1)
                a.xs[(size_t)(r0 + i) * a.xpitch + d] = v[i];
    }
}

constexpr int ENS_SCORE_ROWS = 64;   // rows per workgroup of ensemble_bmu_many_kernel

struct EnsScoreDesc {
    DistArgs d;
    u64 *lastbmu;
    float *sqres;
    u64 *out_idx;            // the member's slice of the ensemble's pinned result buffers
    float *out_dist;
    int B, N;
};

// Som::findBmu (Som.cpp:291-309) for rows [64x, 64x + 64) of member y: the is_first phase 1 of the one-launch batch epoch
// (vsom_tiny_batch_body.inc) -- every (row, node) distance by an 8-lane group in Eigen's order (vsom_group_dist), the
// argmin as an LDS atomicMin on the (distance, index) key (strict <, lowest index, NaN never wins), a NaN at node 0 pins
// the BMU to 0 with sqres = NaN -- on the model rows copied into LDS first (N * part_len <= 4096: at most 32 KB for CLR).
template <int KIND>
__global__ __launch_bounds__(256) void ensemble_bmu_many_kernel(const EnsScoreDesc *__restrict__ descs)
{
    constexpr bool CLR = KIND == VSOM_CLR;
    const EnsScoreDesc a = descs[blockIdx.y];
    const int s0 = blockIdx.x * ENS_SCORE_ROWS;
    if (s0 >= a.B)
        return;                                          // (workgroup-uniform)
    const int T = a.B - s0 < ENS_SCORE_ROWS ? a.B - s0 : ENS_SCORE_ROWS, N = a.N, L = a.d.L;
    extern __shared__ __attribute__((aligned(16))) unsigned char ens_smem[];
    u64 *keys = reinterpret_cast<u64 *>(ens_smem);               // [64]
    int *nan0 = reinterpret_cast<int *>(keys + ENS_SCORE_ROWS);   // [64]
    float *ml = reinterpret_cast<float *>(nan0 + ENS_SCORE_ROWS); // N rows of L values (CLR: A part, then B part)
    const int tid = threadIdx.x;
    const int rl = CLR ? 2 * L : L;
    for (int i = tid; i < N * rl; i += 256) {
        const int n = i / rl, e = i - n * rl;
        ml[i] = e < L ? a.d.ma[(size_t)n * a.d.ldm + e] : a.d.mb[(size_t)n * a.d.ldm + e - L];
    }
    for (int s = tid; s < T; s += 256) {
        keys[s] = ~0ull;
        nan0[s] = 0;
    }
    __syncthreads();
    const float *ma = ml, *mb = CLR ? ml + L : ml;
    const int grp = tid >> 3, k = tid & 7;
    for (int p = grp; p < T * N; p += 32) {
        const int s = p / N, n = p - s * N;
        const size_t row = (size_t)(s0 + s) * a.d.ldx;
        const float dd = vsom_group_dist<CLR>(a.d.xa + row, a.d.xb + row, ma + (size_t)n * rl, mb + (size_t)n * rl, L, k);
        if (k == 0) {
            if (n == 0 && dd != dd)
                nan0[s] = 1;
            atomicMin(&keys[s], vsom_key(dd, (uint32_t)n));
        }
    }
    __syncthreads();
    for (int s = tid; s < T; s += 256) {
        const u64 key = keys[s];
        const u64 idx = nan0[s] ? 0ull : (key & 0xFFFFFFFFull);
        const float sq = nan0[s] ? __uint_as_float(0x7FC00000u) : __uint_as_float((uint32_t)(key >> 32));
        a.lastbmu[s0 + s] = idx;
        a.sqres[s0 + s] = sq;
        a.out_idx[s0 + s] = idx;
        a.out_dist[s0 + s] = sq;
    }
}

// grid.y is at most 65535: more members are launched in slices
constexpr unsigned ENS_MAX_Y = 65535;

int vsom_ensemble_upload_chunks(vsom_ensemble *e, const float *x_host, size_t n_floats, const size_t *offset,
                                const size_t *B, int wait)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (!offset || !B)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null array");
    const size_t n = e->m.size();
    for (size_t k = 0; k < n; ++k) {
        if (B[k] > 0x7FFFFFFFull)
            return ens_fail(k, "chunk too large");
        if (B[k] > 0 && !x_host)
            return ens_fail(k, "x_host is null");
        const size_t len = B[k] * e->m[k]->J;   // (< 2^31 * 2^32: no overflow)
        if (offset[k] > n_floats || len > n_floats - offset[k])
            return ens_fail(k, "rows beyond n_floats");
    }
    VSOM_HIP_CHECK(hipSetDevice(e->device));
    EnsCall call(e);
    if (int rc = join_members(e, nullptr, true))
        return rc;
    // host bookkeeping first (a capacity that grows synchronises the member and reallocates); which members the one
    // launch stages (grp 0), and the extent of the rows on the device
    ens_scratch(e, sizeof(EnsStageDesc));
    size_t lo = SIZE_MAX, hi = 0;
    for (size_t k = 0; k < n; ++k) {
        vsom_ctx *c = e->m[k];
        if (c->cu)
            continue;
        if (int rc = ensure_chunk_capacity(c, B[k]))
            return rc;
        if (B[k] == 0)
            continue;
        lo = std::min(lo, offset[k]);
        hi = std::max(hi, offset[k] + B[k] * c->J);
        if (c->transform != VSOM_CLR && !vsom_cc_considered(c, B[k]))
            e->grp[k] = 0;
    }
    if (hi > lo) {
        if (hi - lo > e->raw.cap) {
            if (e->raw_valid)                    // an earlier call's staging may still read the old buffer
                VSOM_HIP_CHECK(hipEventSynchronize(e->ev_raw));
            e->raw_valid = false;
            VSOM_ALLOC_CHECK(vsom_grow(e->raw, hi - lo, nullptr));
        }
        if (!e->ev_raw)
            VSOM_HIP_CHECK(hipEventCreateWithFlags(&e->ev_raw, hipEventDisableTiming));
        if (!e->ev_stage)
            VSOM_HIP_CHECK(hipEventCreateWithFlags(&e->ev_stage, hipEventDisableTiming));
        // (joined here, not by ens_launch: the copy goes first, and it is made whether or not a member is launched)
        if (int rc = call.join(ENS_PLAIN))
            return rc;
        hipStream_t ls = call.ls;
        if (e->raw_valid)                        // (behind the previous call's readers, whichever stream it used)
            VSOM_HIP_CHECK(hipStreamWaitEvent(ls, e->ev_raw, 0));
        VSOM_HIP_CHECK(hipMemcpyAsync(e->raw.p, x_host + lo, (hi - lo) * sizeof(float), hipMemcpyHostToDevice, ls));
        // the one launch: launch_stage_chunk's bookkeeping for each of its members, then the descriptors
        for (size_t k = 0; k < n; ++k) {
            if (e->grp[k] != 0)
                continue;
            vsom_ctx *c = e->m[k];
            c->B = B[k];
            c->chunk_loaded = true;
            c->cc_valid = false;
            c->xq_valid = false;
            c->xi_valid = false;
            c->rows_free_valid = false;
            if (c->ahead_rows) {                 // stagings of a chunk staged ahead may still write these buffers
                VSOM_HIP_CHECK(hipStreamWaitEvent(ls, c->ev_ahead, 0));
                c->ahead_rows = false;
            }
            c->ahead_valid = false;
            const EnsStageDesc d = {e->raw.p + (offset[k] - lo), c->Xs.p, c->lastbmu.p,
                                    c->sl_scal.p ? c->sl_scal.p + 8192 : nullptr, (int)c->J, (int)B[k], (int)c->xpitch, 0};
            std::memcpy(e->desc.data() + k * sizeof(d), &d, sizeof(d));
            e->ext[k] = (unsigned)((B[k] + 15) / 16);
        }
        if (int rc = ens_launch(call, ENS_JOINED, 1, sizeof(EnsStageDesc), ENS_MAX_Y, ens_always_ready,
                                [](int, const void *d, unsigned cnt, size_t, unsigned blocks, hipStream_t s) -> int {
                                    hipLaunchKernelGGL(stage_rows_many_kernel, dim3(blocks, cnt), dim3(256), 0, s,
                                                       static_cast<const EnsStageDesc *>(d));
                                    VSOM_HIP_CHECK(hipGetLastError());
                                    return VSOM_OK;
                                }))
            return rc;
        // every member stream behind the copy and the staging: later work on a member, and the ordinary stagings below
        VSOM_HIP_CHECK(hipEventRecord(e->ev_stage, ls));
        for (hipStream_t s : call.streams)
            if (s != ls)
                VSOM_HIP_CHECK(hipStreamWaitEvent(s, e->ev_stage, 0));
    }
    // the other members: their single-context staging from the device copy (no rows: nothing is read), custom members
    // from the host range
    for (size_t k = 0; k < n; ++k) {
        if (e->grp[k] == 0)
            continue;
        vsom_ctx *c = e->m[k];
        int rc = c->cu ? vsom_custom_upload(c, B[k] ? x_host + offset[k] : nullptr, B[k], wait != 0)
                       : vsom_set_chunk_device(c, B[k] ? e->raw.p + (offset[k] - lo) : nullptr, B[k]);
        if (rc)
            return rc;
    }
    if (call.ls) {
        // the raw buffer's last readers, joined back into the launch stream: the next call (or a growth) waits for ev_raw
        // before it overwrites the buffer
        if (int rc = call.join(ENS_PLAIN))
            return rc;
        VSOM_HIP_CHECK(hipEventRecord(e->ev_raw, call.ls));
        e->raw_valid = true;
        if (wait)                                // x_host may be reused by the caller
            VSOM_HIP_CHECK(hipEventSynchronize(e->ev_raw));
    }
    call.detach();                               // (wait = 0 returns without a host wait; ev_raw covers what is in flight)
    return VSOM_OK;
}

int vsom_ensemble_bmu_batch(vsom_ensemble *e, uint64_t *const *idx_out, float *const *dist_out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    const size_t n = e->m.size();
    for (size_t k = 0; k < n; ++k)
        if (const char *why = ens_rows_refusal(e->m[k]))
            return ens_fail(k, why);
    VSOM_HIP_CHECK(hipSetDevice(e->device));
    EnsCall call(e);
    if (int rc = join_members(e, nullptr, true))
        return rc;
    // tiny members (the one-launch kernels' bound on the map) with rows: one launch per kind
    const size_t lds_cap = std::min(e->lds_limit, (size_t)64 << 10);
    ens_scratch(e, sizeof(EnsScoreDesc));
    std::vector<size_t> at(n, 0);                // the member's place in the pinned result buffers
    size_t total = 0;
    for (size_t k = 0; k < n; ++k) {
        const vsom_ctx *c = e->m[k];
        const size_t L = c->part_len, rl = c->transform == VSOM_CLR ? 2 * L : L;
        const size_t smem = ENS_SCORE_ROWS * (sizeof(u64) + sizeof(int)) + (size_t)c->N * rl * sizeof(float);
        if (c->cu || c->B == 0 || (size_t)c->N * L > 4096 || smem > lds_cap)
            continue;
        e->grp[k] = c->transform;
        e->smem[k] = smem;
        e->ext[k] = (unsigned)((c->B + ENS_SCORE_ROWS - 1) / ENS_SCORE_ROWS);
        at[k] = total;
        total += c->B;
    }
    int rc = VSOM_OK;
    if (total) {
        if (total > e->sc_idx.cap)             // (no kernel of an earlier call is running: every call ends in a wait)
            VSOM_ALLOC_CHECK(vsom_grow_set(nullptr, 0, {vsom_member(e->sc_idx, total), vsom_member(e->sc_dist, total)}));
        for (size_t k = 0; k < n; ++k) {
            if (e->grp[k] < 0)
                continue;
            vsom_ctx *c = e->m[k];
            const bool clr = c->transform == VSOM_CLR;
            EnsScoreDesc a;
            a.d.xa = clr ? c->XP.p : c->Xs.p;
            a.d.xb = clr ? c->YP.p : c->Xs.p;
            a.d.ldx = (int)(clr ? c->part_pitch : c->xpitch);
            a.d.ma = c->map.p;
            a.d.mb = clr ? c->map.p + c->part_pitch : c->map.p;
            a.d.ldm = (int)c->pitch;
            a.d.L = (int)c->part_len;
            a.lastbmu = c->lastbmu.p;
            a.sqres = c->sqres.p;
            a.out_idx = e->sc_idx.p + at[k];
            a.out_dist = e->sc_dist.p + at[k];
            a.B = (int)c->B;
            a.N = (int)c->N;
            std::memcpy(e->desc.data() + k * sizeof(a), &a, sizeof(a));
        }
        // by VSOM_CLR - kind: named in the order they always were, which is the order the compiler emits them in (the
        // device object stays what it was, byte for byte)
        static void (*const kernel[])(const EnsScoreDesc *) = {ensemble_bmu_many_kernel<VSOM_CLR>,
                                                               ensemble_bmu_many_kernel<VSOM_MEDIAN>,
                                                               ensemble_bmu_many_kernel<VSOM_STANDARD>};
        rc = ens_launch(call, ENS_PLAIN, 3, sizeof(EnsScoreDesc), ENS_MAX_Y, ens_always_ready,
                        [](int kind, const void *d, unsigned cnt, size_t smem, unsigned tiles, hipStream_t s) -> int {
                            hipLaunchKernelGGL(kernel[VSOM_CLR - kind], dim3(tiles, cnt), dim3(256), smem, s,
                                               static_cast<const EnsScoreDesc *>(d));
                            VSOM_HIP_CHECK_AS(hipGetLastError(), "ensemble_bmu_many_kernel");
                            return VSOM_OK;
                        });
    }
    // the other members through vsom_bmu_batch, while the launches run
    for (size_t k = 0; k < n && !rc; ++k)
        if (e->grp[k] < 0 && e->m[k]->B > 0)
            rc = vsom_bmu_batch(e->m[k], idx_out ? idx_out[k] : nullptr, dist_out ? dist_out[k] : nullptr);
    if ((rc = call.end(rc)))
        return rc;
    for (size_t k = 0; k < n; ++k) {
        if (e->grp[k] < 0)
            continue;
        const size_t b = e->m[k]->B;
        if (idx_out && idx_out[k])
            std::memcpy(idx_out[k], e->sc_idx.p + at[k], b * sizeof(uint64_t));
        if (dist_out && dist_out[k])
            std::memcpy(dist_out[k], e->sc_dist.p + at[k], b * sizeof(float));
    }
    return VSOM_OK;
}

// ================================================================================================================
// the masked queries: search over the valid columns, imputation, similarity
// ================================================================================================================
struct EnsMaskedDesc {
    const float *x;              // the member's staged rows (Xs), pitch ldx
    const float *map, *sigma;    // model rows, pitch ldm (sigma: SCORE only)
    const u64 *hits;
    u64 min_hits;
    const unsigned char *valid;  // the member's validity bytes in the call's image, vstride bytes per row (0: one row for all)
    unsigned *rows;              // the member's per-row words in the pinned results: arrays of B entries -- bmu (2 words),
                                 // dist, then nvalid (search) or dmax, dmax_col, first, amax, amax_col, outside, nvalid (SCORE)
    unsigned *dense;             // B x J words in the pinned results -- fill (search) or delta (SCORE) -- or null
    int ldx, ldm, vstride, B, N, J;
    float k;                     // SCORE: (float)num_sigmas, and the sigma rule
    int floor_rule;
};

constexpr int ENS_MQ_WORDS = 4, ENS_MQ_SCORE_WORDS = 10;   // per row: the search's words, the similarity's

// vsom_bmu_masked_batch (SCORE: vsom_similarity_masked_batch) for rows [64x, 64x + 64) of member y.  The search is
// ensemble_bmu_many_kernel's on the masked distance: the model rows in LDS (N * J <= 4096 values), every (row, node)
// distance by an 8-lane group (masked_group_dist: the residual +0 at an invalid column, the exact search's order), nodes
// n > 0 with bmuHits[n] < min_hits left out (node 0 seeds whatever its hits), the argmin as an LDS atomicMin on the
// (distance, index) key (strict <, lowest index, NaN never wins), a NaN at node 0 pins the unit to 0 with distance NaN.
// Then, behind one barrier, one wavefront per row (16 rows each): the count of valid columns, the imputed row (the bits
// of x where valid, of the unit's LDS row where not) when asked for, and under SCORE the row body of similarity_kernel
// (vsom_sim_row.hpp, vsom_sim_reduce.inc: one column per lane and step) on x, the unit's LDS row and its sigmaMap row.
// Validity bytes are read as given (non-zero = valid); Standard / Median only.  KIND is only a launch-group label, as in
// ensemble_bmu_many_kernel (one launch per kind): the body never reads it, so the two instantiations of a SCORE are the
// same machine code.
template <int KIND, bool SCORE>
__global__ __launch_bounds__(256) void ensemble_masked_many_kernel(const EnsMaskedDesc *__restrict__ descs)
{
    static_assert(KIND == VSOM_STANDARD || KIND == VSOM_MEDIAN, "the masked residual does not run over CLR's column pairs");
    const EnsMaskedDesc a = descs[blockIdx.y];
    const int s0 = blockIdx.x * ENS_SCORE_ROWS;
    if (s0 >= a.B)
        return;                                          // (workgroup-uniform)
    const int T = a.B - s0 < ENS_SCORE_ROWS ? a.B - s0 : ENS_SCORE_ROWS, N = a.N, L = a.J;
    extern __shared__ __attribute__((aligned(16))) unsigned char ens_mq_smem[];
    u64 *keys = reinterpret_cast<u64 *>(ens_mq_smem);            // [64]
    int *nan0 = reinterpret_cast<int *>(keys + ENS_SCORE_ROWS);   // [64]
    float *ml = reinterpret_cast<float *>(nan0 + ENS_SCORE_ROWS); // N rows of L values
    const int tid = threadIdx.x;
    for (int i = tid; i < N * L; i += 256) {
        const int n = i / L, e = i - n * L;
        ml[i] = a.map[(size_t)n * a.ldm + e];
    }
    for (int s = tid; s < T; s += 256) {
        keys[s] = ~0ull;
        nan0[s] = 0;
    }
    __syncthreads();
    const int grp = tid >> 3, k = tid & 7;
    for (int p = grp; p < T * N; p += 32) {
        const int s = p / N, n = p - s * N;
        // findRestrictedBmu (Som.cpp:316-322): node 0 seeds unconditionally, the others need the hits (group-uniform)
        if (n > 0 && a.min_hits && a.hits[n] < a.min_hits)
            continue;
        const float dd = masked_group_dist(a.x + (size_t)(s0 + s) * a.ldx, a.valid + (size_t)(s0 + s) * a.vstride,
                                           ml + (size_t)n * L, L, k);
        if (k == 0) {
            if (n == 0 && dd != dd)
                nan0[s] = 1;
            atomicMin(&keys[s], vsom_key(dd, (uint32_t)n));
        }
    }
    __syncthreads();
    // the rows' epilogue: wavefront w takes rows w, w + 4, ...
    const int lane = tid & 63;
    const size_t R = (size_t)a.B;
    SimArgs sa{};                                        // (sim_column reads k and floor_rule)
    sa.k = a.k;
    sa.floor_rule = a.floor_rule;
    for (int s = tid >> 6; s < T; s += 4) {
        const u64 key = keys[s];
        const u64 idx = nan0[s] ? 0ull : (key & 0xFFFFFFFFull);
        const float sq = nan0[s] ? __uint_as_float(0x7FC00000u) : __uint_as_float((uint32_t)(key >> 32));
        const size_t i = (size_t)(s0 + s);
        const unsigned *xr = reinterpret_cast<const unsigned *>(a.x) + i * a.ldx;
        const unsigned *mr = reinterpret_cast<const unsigned *>(ml) + (size_t)idx * L;
        const float *sr = a.sigma + (size_t)idx * a.ldm;
        const unsigned char *vr = a.valid + i * (size_t)a.vstride;
        unsigned *dr = a.dense ? a.dense + i * L : nullptr;
        unsigned nv = 0;
        SimLane l;
        sim_lane_init(l);
        for (int d = lane; d < L; d += 64) {
            const bool valid = vr[d] != 0;
            const unsigned xb = xr[d], mb = mr[d];
            nv += valid ? 1u : 0u;
            if constexpr (SCORE) {
                const float out = sim_column<true>(l, sa, (uint32_t)d, __uint_as_float(xb), __uint_as_float(mb), sr[d], valid);
                if (dr)
                    dr[d] = __float_as_uint(out);
            } else if (dr) {
                dr[d] = valid ? xb : mb;
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
            nv += __shfl_xor(nv, m);
        if constexpr (SCORE) {
            constexpr int W = 1;                         // one column per lane and step
#include "vsom_sim_reduce.inc"
            if (lane == 0) {
                a.rows[3 * R + i] = __float_as_uint(dmax);
                a.rows[4 * R + i] = dc;
                a.rows[5 * R + i] = __float_as_uint(first);
                a.rows[6 * R + i] = __float_as_uint(amax);
                a.rows[7 * R + i] = ac;
                a.rows[8 * R + i] = cnt;
            }
        }
        if (lane == 0) {
            reinterpret_cast<u64 *>(a.rows)[i] = idx;
            a.rows[2 * R + i] = __float_as_uint(sq);
            a.rows[(SCORE ? 9 : 3) * R + i] = nv;
        }
    }
}

// what both masked queries refuse for member k with a validity, or null
static const char *ens_masked_query_refusal(const vsom_ctx *c, const char *what, std::string &buf)
{
    if (c->cu) {
        buf = std::string(what) + ": custom contexts are not supported";
        return buf.c_str();
    }
    if (c->transform == VSOM_CLR) {
        buf = std::string(what) + ": CLR contexts are not supported (the residual runs over column pairs)";
        return buf.c_str();
    }
    return ens_rows_refusal(c);
}

// a launched member's row words from the pinned results into the caller's arrays (null: not wanted): array 0 is bmu, two
// words per row, every later one a word per row, in the order the kernel stores them
static void ens_mq_copy_out(const unsigned *p, size_t b, std::initializer_list<void *> dst)
{
    size_t i = 0;
    for (void *d : dst) {
        if (d)
            std::memcpy(d, p + (i == 0 ? 0 : (i + 1) * b), (i == 0 ? 2 * b : b) * 4);
        ++i;
    }
}

// what both entry points check: the arrays every form takes, and -- last, behind the call's own arguments -- every member
// with a validity (`what`: the single call, for the refusal's text).  Nothing is enqueued for any member unless every
// member with a validity can be searched.
static int ens_masked_query_arrays(const vsom_ensemble *e, const uint8_t *const *valid_host, const void *out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (!valid_host)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null valid_host array");
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null out array");
    return VSOM_OK;
}

static int ens_masked_query_members(const vsom_ensemble *e, const char *what, const uint8_t *const *valid_host)
{
    std::string buf;
    for (size_t k = 0; k < e->m.size(); ++k)
        if (valid_host[k])
            if (const char *why = ens_masked_query_refusal(e->m[k], what, buf))
                return ens_fail(k, why);
    return VSOM_OK;
}

// Both masked queries (the callers have made their argument checks): bout (the search, vsom_bmu_masked_batch per member) or
// sout (the similarity, vsom_similarity_masked_batch per member) is non-null.  The members with a validity and rows whose
// map fits the kernel's LDS rows go as one launch per kind, their validity bytes as one pinned image in the launch's
// descriptor slot, copied once; every other member with a validity runs its single call while the launches run.
static int ens_masked_query(vsom_ensemble *e, const uint64_t *min_hits, const int *num_sigmas, int sigma_rule,
                            const uint8_t *const *valid_host, const int *one_mask, const vsom_masked_out *bout,
                            const vsom_similarity_masked_out *sout)
{
    const bool score = sout != nullptr;
    const size_t n = e->m.size();
    VSOM_HIP_CHECK(hipSetDevice(e->device));
    EnsCall call(e);
    std::vector<size_t> asked(n);
    for (size_t k = 0; k < n; ++k)
        asked[k] = valid_host[k] != nullptr;             // (a member without a validity is not touched)
    if (int rc = join_members(e, asked.data(), true))    // (a pending sigmaMap is materialised here)
        return rc;
    const size_t lds_cap = std::min(e->lds_limit, (size_t)64 << 10);
    const size_t words = score ? ENS_MQ_SCORE_WORDS : ENS_MQ_WORDS;
    ens_scratch(e, sizeof(EnsMaskedDesc));
    std::vector<size_t> v_at(n, 0), vbytes(n, 0), w_at(n, 0), d_at(n, 0);
    std::vector<float *> dense(n, nullptr);              // the caller's fill / delta
    size_t vtotal = 0, wtotal = 0, dtotal = 0;
    for (size_t k = 0; k < n; ++k) {
        const vsom_ctx *c = e->m[k];
        if (!asked[k] || c->B == 0)
            continue;
        dense[k] = score ? sout[k].delta : bout[k].fill;
        const size_t smem = ENS_SCORE_ROWS * (sizeof(u64) + sizeof(int)) + (size_t)c->N * c->J * sizeof(float);
        if ((size_t)c->N * c->part_len > 4096 || smem > lds_cap)
            continue;
        e->grp[k] = c->transform;
        e->smem[k] = smem;
        e->ext[k] = (unsigned)((c->B + ENS_SCORE_ROWS - 1) / ENS_SCORE_ROWS);
        vbytes[k] = ((one_mask && one_mask[k]) ? 1 : c->B) * (size_t)c->J;
        v_at[k] = vtotal;
        vtotal += (vbytes[k] + 15) / 16 * 16;
        w_at[k] = wtotal;
        wtotal += (c->B * words + 3) / 4 * 4;            // (16-byte steps: the 8-byte units lead each member's words)
        if (dense[k]) {
            d_at[k] = dtotal;
            dtotal += c->B * (size_t)c->J;
        }
    }
    int rc = VSOM_OK;
    if (wtotal) {
        if (int jrc = call.join(ENS_LAUNCHED))
            return jrc;
        // the slot ens_launch is about to take: its last launch has completed, so its image may be rewritten
        auto &s = e->slot[e->next];
        if (s.valid)
            VSOM_HIP_CHECK(hipEventSynchronize(s.ev));
        VSOM_ALLOC_CHECK(vsom_grow_set(nullptr, 0, {vsom_member(s.img_host, vtotal), vsom_member(s.img_dev, vtotal)}));
        // (no kernel of an earlier call is running: every call ends in a wait)
        VSOM_ALLOC_CHECK(vsom_grow_set(nullptr, 0, {vsom_member(e->mq_rows, wtotal), vsom_member(e->mq_dense, std::max<size_t>(dtotal, 1))}));
        for (size_t k = 0; k < n; ++k)
            if (e->grp[k] >= 0)
                std::memcpy(s.img_host.p + v_at[k], valid_host[k], vbytes[k]);
        VSOM_HIP_CHECK(hipMemcpyAsync(s.img_dev.p, s.img_host.p, vtotal, hipMemcpyHostToDevice, call.ls));
        for (size_t k = 0; k < n; ++k) {
            if (e->grp[k] < 0)
                continue;
            const vsom_ctx *c = e->m[k];
            EnsMaskedDesc a;
            a.x = c->Xs.p;
            a.map = c->map.p;
            a.sigma = c->sigma.p;
            a.hits = c->hits.p;
            a.min_hits = min_hits ? min_hits[k] : 0;
            a.valid = s.img_dev.p + v_at[k];
            a.rows = e->mq_rows.p + w_at[k];
            a.dense = dense[k] ? reinterpret_cast<unsigned *>(e->mq_dense.p + d_at[k]) : nullptr;
            a.ldx = (int)c->xpitch;
            a.ldm = (int)c->pitch;
            a.vstride = (one_mask && one_mask[k]) ? 0 : (int)c->J;
            a.B = (int)c->B;
            a.N = (int)c->N;
            a.J = (int)c->J;
            a.k = score ? (float)num_sigmas[k] : 0.f;
            a.floor_rule = sigma_rule == VSOM_SIGMA_FLOOR;
            std::memcpy(e->desc.data() + k * sizeof(a), &a, sizeof(a));
        }
        static void (*const kernel[2][2])(const EnsMaskedDesc *) = {
            {ensemble_masked_many_kernel<VSOM_STANDARD, false>, ensemble_masked_many_kernel<VSOM_MEDIAN, false>},
            {ensemble_masked_many_kernel<VSOM_STANDARD, true>, ensemble_masked_many_kernel<VSOM_MEDIAN, true>}};
        rc = ens_launch(call, ENS_JOINED, 2, sizeof(EnsMaskedDesc), ENS_MAX_Y, ens_always_ready,
                        [score](int kind, const void *d, unsigned cnt, size_t smem, unsigned tiles, hipStream_t st) -> int {
                            hipLaunchKernelGGL(kernel[score][kind], dim3(tiles, cnt), dim3(256), smem, st,
                                               static_cast<const EnsMaskedDesc *>(d));
                            VSOM_HIP_CHECK_AS(hipGetLastError(), "ensemble_masked_many_kernel");
                            return VSOM_OK;
                        });
    }
    // the other members through their single calls, while the launches run
    for (size_t k = 0; k < n && !rc; ++k) {
        vsom_ctx *c = e->m[k];
        if (!asked[k] || c->B == 0 || e->grp[k] >= 0)
            continue;
        const int one = one_mask ? one_mask[k] : 0;
        const u64 mh = min_hits ? min_hits[k] : 0;
        rc = score ? launch_similarity_masked(c, mh, num_sigmas[k], sigma_rule, 0, c->B, valid_host[k], one, &sout[k])
                   : launch_masked(c, mh, 0, c->B, valid_host[k], one, &bout[k]);
    }
    if ((rc = call.end(rc)))
        return rc;
    // results of the launched members: the kernel stored them into the pinned buffers
    for (size_t k = 0; k < n; ++k) {
        if (e->grp[k] < 0)
            continue;
        const size_t b = e->m[k]->B;
        const unsigned *p = e->mq_rows.p + w_at[k];
        if (score) {
            const vsom_similarity_masked_out &o = sout[k];
            ens_mq_copy_out(p, b, {o.bmu, o.dist, o.dmax, o.dmax_col, o.first, o.amax, o.amax_col, o.outside, o.nvalid});
        } else {
            const vsom_masked_out &o = bout[k];
            ens_mq_copy_out(p, b, {o.bmu, o.dist, o.nvalid});
        }
        if (dense[k])
            std::memcpy(dense[k], e->mq_dense.p + d_at[k], b * (size_t)e->m[k]->J * sizeof(float));
    }
    return VSOM_OK;
}

int vsom_ensemble_bmu_masked_batch(vsom_ensemble *e, const uint64_t *min_hits, const uint8_t *const *valid_host,
                                   const int *one_mask, const vsom_masked_out *out)
{
    if (int rc = ens_masked_query_arrays(e, valid_host, out))
        return rc;
    if (int rc = ens_masked_query_members(e, "vsom_bmu_masked_batch", valid_host))
        return rc;
    return ens_masked_query(e, min_hits, nullptr, VSOM_SIGMA_FLOOR, valid_host, one_mask, out, nullptr);
}

int vsom_ensemble_similarity_masked_batch(vsom_ensemble *e, const uint64_t *min_hits, const int *num_sigmas, int sigma_rule,
                                          const uint8_t *const *valid_host, const int *one_mask,
                                          const vsom_similarity_masked_out *out)
{
    if (int rc = ens_masked_query_arrays(e, valid_host, out))
        return rc;
    if (!num_sigmas)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null num_sigmas array");
    if (sigma_rule != VSOM_SIGMA_AS_WRITTEN && sigma_rule != VSOM_SIGMA_FLOOR)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: unknown sigma_rule");
    if (int rc = ens_masked_query_members(e, "vsom_similarity_masked_batch", valid_host))
        return rc;
    return ens_masked_query(e, min_hits, num_sigmas, sigma_rule, valid_host, one_mask, nullptr, out);
}

// ================================================================================================================
// the k best matching units of every row of every member, plain and over the valid columns
// ================================================================================================================
struct EnsTopkDesc {
    DistArgs d;                  // plain: ensemble_bmu_many_kernel's operands; masked: xa = the staged rows (Xs), ma = the map
    const u64 *hits;             // masked: the candidates are node 0 and the nodes with hits >= min_hits
    u64 min_hits;
    const unsigned char *valid;  // masked: the member's validity bytes in the call's image, vstride bytes per row (0: one row)
    unsigned *out;               // the member's words in the pinned results: idx (B x k, two words each), dist (B x k),
                                 // count (B), nvalid (B)
    int vstride, B, N, k;
};

// words of one member in the pinned results (a multiple of 4: the 8-byte indices lead each member's words)
static size_t ens_topk_words(size_t B, size_t k) { return (B * (3 * k + 2) + 3) / 4 * 4; }

// the row stride of the LDS lists in keys: odd, so that the lists of the eight rows whose groups share a wavefront start
// on eight different bank pairs (the groups' lanes 0 insert at the same time, at about the same place of their lists)
__host__ __device__ constexpr int ens_topk_stride(int k) { return k | 1; }

// vsom_bmu_topk_batch (MASKED: vsom_bmu_topk_masked_batch without blend) for rows [64x, 64x + 64) of member y.  The model
// rows in LDS as in ensemble_bmu_many_kernel; the 32 eight-lane groups each own rows g and g + 32 of the tile and walk
// that row's nodes in index order: every (row, node) distance by vsom_group_dist<CLR> (MASKED: masked_group_dist, nodes
// n > 0 with bmuHits[n] < min_hits left out), and lane 0 of the group keeps the row's sorted list of its k smallest keys
// vsom_key(d, n) in LDS -- a key that beats the list's last (or finds the list short) is inserted by shifting.  One lane
// owns a list from start to end, keys are unique and arrive in index order: no atomics, no second pass, one result.  The
// node-0 rule (Som.cpp:291-309): a NaN d_0 is recorded and kept out of the list, which then holds k - 1 keys; the
// epilogue puts node 0 with 0x7FC00000 in front.  The epilogue, behind one barrier, is one wavefront per row (16 rows
// each): lane j stores entry j (idx, dist; UINT64_MAX / 0x7FC00000 behind the row's last real entry) and, MASKED, the
// wavefront counts the row's valid columns as ensemble_masked_many_kernel does and stores count and nvalid.
// LDS: 64 lists of (k | 1) keys, 64 counts, 64 flags, the model rows -- independent of N but for the model rows.
template <int KIND, bool MASKED>
__global__ __launch_bounds__(256) void ensemble_topk_many_kernel(const EnsTopkDesc *__restrict__ descs)
{
    constexpr bool CLR = KIND == VSOM_CLR;
    static_assert(!(CLR && MASKED), "the masked residual does not run over CLR's column pairs");
    const EnsTopkDesc a = descs[blockIdx.y];
    const int s0 = blockIdx.x * ENS_SCORE_ROWS;
    if (s0 >= a.B)
        return;                                          // (workgroup-uniform)
    const int T = a.B - s0 < ENS_SCORE_ROWS ? a.B - s0 : ENS_SCORE_ROWS, N = a.N, L = a.d.L, K = a.k;
    const int LS = ens_topk_stride(K);
    extern __shared__ __attribute__((aligned(16))) unsigned char ens_tk_smem[];
    u64 *lists = reinterpret_cast<u64 *>(ens_tk_smem);            // [64][LS]
    int *cnts = reinterpret_cast<int *>(lists + ENS_SCORE_ROWS * LS);   // [64] keys in the row's list
    int *nan0 = cnts + ENS_SCORE_ROWS;                            // [64]
    float *ml = reinterpret_cast<float *>(nan0 + ENS_SCORE_ROWS); // N rows of L values (CLR: A part, then B part)
    const int tid = threadIdx.x;
    const int rl = CLR ? 2 * L : L;
    for (int i = tid; i < N * rl; i += 256) {
        const int n = i / rl, e = i - n * rl;
        ml[i] = e < L ? a.d.ma[(size_t)n * a.d.ldm + e] : a.d.mb[(size_t)n * a.d.ldm + e - L];
    }
    __syncthreads();
    const float *ma = ml, *mb = CLR ? ml + L : ml;
    const int grp = tid >> 3, k = tid & 7;
    for (int s = grp; s < T; s += 32) {                  // (group-uniform)
        u64 *list = lists + s * LS;
        const size_t row = (size_t)(s0 + s) * a.d.ldx;
        // lane 0's record of the list: its length, its capacity (k, or k - 1 behind a NaN node 0), its last key once full
        int cnt = 0, cap = K, first_nan = 0;
        u64 last = 0;
        for (int n = 0; n < N; ++n) {
            float dd;
            if constexpr (MASKED) {
                // findRestrictedBmu (Som.cpp:316-322): node 0 seeds unconditionally, the others need the hits
                if (n > 0 && a.min_hits && a.hits[n] < a.min_hits)
                    continue;
                dd = masked_group_dist(a.d.xa + row, a.valid + (size_t)(s0 + s) * a.vstride, ml + (size_t)n * L, L, k);
            } else {
                dd = vsom_group_dist<CLR>(a.d.xa + row, a.d.xb + row, ma + (size_t)n * rl, mb + (size_t)n * rl, L, k);
            }
            if (k != 0)
                continue;
            if (n == 0 && dd != dd) {
                first_nan = 1;
                cap = K - 1;
                continue;
            }
            const u64 key = vsom_key(dd, (uint32_t)n);
            int j;                                       // the place that opens: behind a short list, or its last key's
            if (cnt < cap)
                j = cnt++;
            else if (cap > 0 && key < last)
                j = cap - 1;
            else
                continue;
            for (; j > 0; --j) {
                const u64 prev = list[j - 1];
                if (prev < key)
                    break;
                list[j] = prev;
            }
            list[j] = key;
            if (cnt == cap)
                last = list[cap - 1];
        }
        if (k == 0) {
            cnts[s] = cnt;
            nan0[s] = first_nan;
        }
    }
    __syncthreads();
    // the rows' epilogue: wavefront w takes rows w, w + 4, ...; lane j stores entry j
    const int lane = tid & 63;
    const size_t R = (size_t)a.B;
    u64 *oidx = reinterpret_cast<u64 *>(a.out);
    unsigned *odist = a.out + 2 * R * K, *ocount = odist + R * K, *onvalid = ocount + R;
    for (int s = tid >> 6; s < T; s += 4) {
        const size_t i = (size_t)(s0 + s);
        const int pinned = nan0[s], cnt = cnts[s];
        if (lane < K) {
            u64 idx = ~0ull;
            unsigned bits = 0x7FC00000u;
            const int e = lane - pinned;
            if (e < 0) {
                idx = 0ull;                              // node 0 with the quiet NaN
            } else if (e < cnt) {
                const u64 key = lists[s * LS + e];
                idx = key & 0xFFFFFFFFull;
                const unsigned b = (unsigned)(key >> 32);
                bits = b == 0xFFFFFFFFu ? 0x7FC00000u : b;
            }
            oidx[i * K + lane] = idx;
            odist[i * K + lane] = bits;
        }
        if constexpr (MASKED) {
            const unsigned char *vr = a.valid + i * (size_t)a.vstride;
            unsigned nv = 0;
            for (int d = lane; d < L; d += 64)
                nv += vr[d] != 0 ? 1u : 0u;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1)
                nv += __shfl_xor(nv, m);
            if (lane == 0) {
                ocount[i] = (unsigned)(pinned + cnt);
                onvalid[i] = nv;
            }
        }
    }
}

// the LDS need of a member in ensemble_topk_many_kernel
static size_t ens_topk_smem(const vsom_ctx *c, uint32_t k)
{
    const size_t rl = c->transform == VSOM_CLR ? 2 * c->part_len : c->part_len;
    return ENS_SCORE_ROWS * ((size_t)ens_topk_stride((int)k) * sizeof(u64) + 2 * sizeof(int)) + (size_t)c->N * rl * sizeof(float);
}

// the fast-path rule (include/vsom_hip.h): would this member with this k run in ensemble_topk_many_kernel?
static bool ens_topk_fast(const vsom_ensemble *e, const vsom_ctx *c, uint32_t k, bool masked)
{
    if (c->cu || (masked && c->transform == VSOM_CLR) || !c->chunk_loaded || c->B == 0)
        return false;
    if (k == 0 || k > 64 || k > c->N || (size_t)c->N * c->part_len > 4096)
        return false;
    return ens_topk_smem(c, k) <= std::min(e->lds_limit, (size_t)64 << 10);   // (no attribute is raised)
}

int vsom_ensemble_topk_applies(const vsom_ensemble *e, size_t member, uint32_t k, int masked)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (member >= e->m.size())
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: member index out of range");
    return ens_topk_fast(e, e->m[member], k, masked != 0) ? 1 : 0;
}

// Both top-k calls (the callers have made their argument checks); valid_host null: the plain call, whose covered members
// are those with an idx.  The covered members on the fast path go as one launch per kind, the masked ones' validity bytes
// as one pinned image in the launch's descriptor slot, copied once; every other covered member with rows runs its single
// call while the launches run.
static int ens_topk(vsom_ensemble *e, const uint32_t *k, const uint64_t *min_hits, const uint8_t *const *valid_host,
                    const int *one_mask, const vsom_ensemble_topk_out *out)
{
    const bool masked = valid_host != nullptr;
    const size_t n = e->m.size();
    VSOM_HIP_CHECK(hipSetDevice(e->device));
    EnsCall call(e);
    std::vector<size_t> asked(n);
    for (size_t m = 0; m < n; ++m)
        asked[m] = masked ? valid_host[m] != nullptr : out[m].idx != nullptr;   // (a skipped member is not touched)
    if (int rc = join_members(e, asked.data(), true))
        return rc;
    ens_scratch(e, sizeof(EnsTopkDesc));
    std::vector<size_t> v_at(n, 0), vbytes(n, 0), w_at(n, 0);
    size_t vtotal = 0, wtotal = 0;
    for (size_t m = 0; m < n; ++m) {
        const vsom_ctx *c = e->m[m];
        if (!asked[m] || !ens_topk_fast(e, c, k[m], masked))
            continue;
        e->grp[m] = c->transform;
        e->smem[m] = ens_topk_smem(c, k[m]);
        e->ext[m] = (unsigned)((c->B + ENS_SCORE_ROWS - 1) / ENS_SCORE_ROWS);
        if (masked) {
            vbytes[m] = ((one_mask && one_mask[m]) ? 1 : c->B) * (size_t)c->J;
            v_at[m] = vtotal;
            vtotal += (vbytes[m] + 15) / 16 * 16;
        }
        w_at[m] = wtotal;
        wtotal += ens_topk_words(c->B, k[m]);
    }
    int rc = VSOM_OK;
    if (wtotal) {
        if (int jrc = call.join(ENS_LAUNCHED))
            return jrc;
        // the slot ens_launch is about to take: its last launch has completed, so its image may be rewritten
        auto &s = e->slot[e->next];
        if (s.valid)
            VSOM_HIP_CHECK(hipEventSynchronize(s.ev));
        if (masked)
            VSOM_ALLOC_CHECK(vsom_grow_set(nullptr, 0, {vsom_member(s.img_host, vtotal), vsom_member(s.img_dev, vtotal)}));
        // (no kernel of an earlier call is running: every call ends in a wait)
        VSOM_ALLOC_CHECK(vsom_grow(e->mq_rows, wtotal, nullptr));
        if (masked) {
            for (size_t m = 0; m < n; ++m)
                if (e->grp[m] >= 0)
                    std::memcpy(s.img_host.p + v_at[m], valid_host[m], vbytes[m]);
            VSOM_HIP_CHECK(hipMemcpyAsync(s.img_dev.p, s.img_host.p, vtotal, hipMemcpyHostToDevice, call.ls));
        }
        for (size_t m = 0; m < n; ++m) {
            if (e->grp[m] < 0)
                continue;
            const vsom_ctx *c = e->m[m];
            const bool clr = c->transform == VSOM_CLR;
            EnsTopkDesc a;
            a.d.xa = clr ? c->XP.p : c->Xs.p;
            a.d.xb = clr ? c->YP.p : c->Xs.p;
            a.d.ldx = (int)(clr ? c->part_pitch : c->xpitch);
            a.d.ma = c->map.p;
            a.d.mb = clr ? c->map.p + c->part_pitch : c->map.p;
            a.d.ldm = (int)c->pitch;
            a.d.L = (int)c->part_len;
            a.hits = c->hits.p;
            a.min_hits = masked && min_hits ? min_hits[m] : 0;
            a.valid = masked ? s.img_dev.p + v_at[m] : nullptr;
            a.out = e->mq_rows.p + w_at[m];
            a.vstride = (one_mask && one_mask[m]) ? 0 : (int)c->J;
            a.B = (int)c->B;
            a.N = (int)c->N;
            a.k = (int)k[m];
            std::memcpy(e->desc.data() + m * sizeof(a), &a, sizeof(a));
        }
        static void (*const kernel[2][3])(const EnsTopkDesc *) = {
            {ensemble_topk_many_kernel<VSOM_STANDARD, false>, ensemble_topk_many_kernel<VSOM_MEDIAN, false>,
             ensemble_topk_many_kernel<VSOM_CLR, false>},
            {ensemble_topk_many_kernel<VSOM_STANDARD, true>, ensemble_topk_many_kernel<VSOM_MEDIAN, true>, nullptr}};
        rc = ens_launch(call, ENS_JOINED, 3, sizeof(EnsTopkDesc), ENS_MAX_Y, ens_always_ready,
                        [masked](int kind, const void *d, unsigned cnt, size_t smem, unsigned tiles, hipStream_t st) -> int {
                            hipLaunchKernelGGL(kernel[masked][kind], dim3(tiles, cnt), dim3(256), smem, st,
                                               static_cast<const EnsTopkDesc *>(d));
                            VSOM_HIP_CHECK_AS(hipGetLastError(), "ensemble_topk_many_kernel");
                            return VSOM_OK;
                        });
    }
    // the other members through their single calls, while the launches run
    for (size_t m = 0; m < n && !rc; ++m) {
        vsom_ctx *c = e->m[m];
        if (!asked[m] || c->B == 0 || e->grp[m] >= 0)
            continue;
        if (masked) {
            const vsom_topk_masked_out o = {out[m].idx, out[m].dist, out[m].count, out[m].nvalid, nullptr};
            rc = launch_topk_masked(c, k[m], min_hits ? min_hits[m] : 0, 0, c->B, valid_host[m], one_mask ? one_mask[m] : 0, &o);
        } else {
            rc = launch_topk(c, k[m], 0, c->B, out[m].idx, out[m].dist);
        }
    }
    if ((rc = call.end(rc)))
        return rc;
    // results of the launched members: the kernel stored them into the pinned buffer
    for (size_t m = 0; m < n; ++m) {
        if (e->grp[m] < 0)
            continue;
        const size_t b = e->m[m]->B, bk = b * k[m];
        const unsigned *p = e->mq_rows.p + w_at[m];
        std::memcpy(out[m].idx, p, bk * sizeof(uint64_t));
        if (out[m].dist)
            std::memcpy(out[m].dist, p + 2 * bk, bk * sizeof(float));
        if (masked && out[m].count)
            std::memcpy(out[m].count, p + 3 * bk, b * sizeof(uint32_t));
        if (masked && out[m].nvalid)
            std::memcpy(out[m].nvalid, p + 3 * bk + b, b * sizeof(uint32_t));
    }
    return VSOM_OK;
}

// what both top-k calls check for a covered member, behind the call's own arrays: the member, then its k
static int ens_topk_member(const vsom_ensemble *e, size_t m, const char *what, bool masked, uint32_t k, std::string &buf)
{
    const vsom_ctx *c = e->m[m];
    if (masked) {
        if (const char *why = ens_masked_query_refusal(c, what, buf))
            return ens_fail(m, why);
    } else {
        if (c->cu) {
            buf = std::string(what) + ": custom contexts are not supported";
            return ens_fail(m, buf.c_str());
        }
        if (const char *why = ens_rows_refusal(c))
            return ens_fail(m, why);
    }
    if (k == 0 || k > 64 || k > c->N)
        return ens_fail(m, "k must be in [1, min(64, N)]");
    return VSOM_OK;
}

int vsom_ensemble_bmu_topk_batch(vsom_ensemble *e, const uint32_t *k, const vsom_ensemble_topk_out *out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (!k)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null k array");
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null out array");
    std::string buf;
    for (size_t m = 0; m < e->m.size(); ++m)
        if (out[m].idx)
            if (int rc = ens_topk_member(e, m, "vsom_bmu_topk_batch", false, k[m], buf))
                return rc;
    return ens_topk(e, k, nullptr, nullptr, nullptr, out);
}

int vsom_ensemble_bmu_topk_masked_batch(vsom_ensemble *e, const uint32_t *k, const uint64_t *min_hits,
                                        const uint8_t *const *valid_host, const int *one_mask,
                                        const vsom_ensemble_topk_out *out)
{
    if (int rc = ens_masked_query_arrays(e, valid_host, out))
        return rc;
    if (!k)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null k array");
    std::string buf;
    for (size_t m = 0; m < e->m.size(); ++m) {
        if (!valid_host[m])
            continue;
        if (int rc = ens_topk_member(e, m, "vsom_bmu_topk_masked_batch", true, k[m], buf))
            return rc;
        if (!out[m].idx)
            return ens_fail(m, "out->idx is null");
    }
    return ens_topk(e, k, min_hits, valid_host, one_mask, out);
}

// ================================================================================================================
// the validation loss of every member, plain and over the valid columns
// ================================================================================================================
struct EnsEvalDesc {
    DistArgs d;                  // plain: ensemble_bmu_many_kernel's operands; masked: xa = the staged rows (Xs), ma = the map
    const float *x;              // the staged rows the scoring reads (Xs), pitch ldxs
    const u64 *hits;             // masked: the candidates are node 0 and the nodes with hits >= min_hits
    u64 min_hits;
    const unsigned char *valid;  // the member's validity bytes in the call's image, vstride bytes per row (masked, 0: one row
                                 // for all); plain: null when every column is valid
    const float *binary, *continuous;   // [J] in the call's image
    u64 *lastbmu;                // plain: the member's lastBMU / sqres, stored as ensemble_bmu_many_kernel stores them
    float *sqres;
    unsigned *rows;              // the member's per-row words in the pinned results: arrays of B entries -- bmu (2 words),
                                 // dist, bsum, nrepl, and nvalid (masked)
    int ldxs, vstride, B, N, C;
};

// vsom_evaluate_batch (MASKED: vsom_evaluate_masked_batch) for rows [64x, 64x + 64) of member y.
// Phase 1 is the sibling's search: ensemble_bmu_many_kernel's (MASKED: ensemble_masked_many_kernel's) -- the model rows in
// LDS, every (row, node) distance by an 8-lane group, the argmin as an LDS atomicMin on the (distance, index) key, a NaN at
// node 0 pins the unit to 0 with distance NaN.
// Phase 2, behind one barrier, is evaluate_kernel's row scoring in its geometry: eight lanes per row, so the 256 threads
// take 32 rows per pass and two passes cover the tile.  The row body is the one evaluate_kernel runs (vsom_eval_row.inc: the
// same operations in the same order on the same logf, hence the same bits), on x and the unit's row IN LDS -- the layout of
// phase 1 keeps a CLR row's two parts side by side, so logical column d is element d of the row and nothing is gathered from
// global memory behind the search's result.  Lane 0 of the eight stores the row's words; the plain form also stores the
// member's lastBMU / sqres.  No LDS beyond the search's, no atomics in phase 2.  The two passes are one rolled loop: the
// row body's registers are live once.  Residency in workgroups per CU, bound by the registers, is the sibling search's: the
// plain forms reach it unasked (8 as ensemble_bmu_many_kernel, CLR 5); the masked form is held to
// ensemble_masked_many_kernel's 7 by the second launch bound (it would take 74 registers, two past the step; nothing spills).
template <int KIND, bool MASKED>
__global__ __launch_bounds__(256, MASKED ? 7 : 1) void ensemble_evaluate_many_kernel(const EnsEvalDesc *__restrict__ descs)
{
    constexpr bool CLR = KIND == VSOM_CLR;
    static_assert(!(CLR && MASKED), "the masked residual does not run over CLR's column pairs");
    const EnsEvalDesc a = descs[blockIdx.y];
    const int s0 = blockIdx.x * ENS_SCORE_ROWS;
    if (s0 >= a.B)
        return;                                          // (workgroup-uniform)
    const int T = a.B - s0 < ENS_SCORE_ROWS ? a.B - s0 : ENS_SCORE_ROWS, N = a.N, L = a.d.L;
    extern __shared__ __attribute__((aligned(16))) unsigned char ens_ev_smem[];
    u64 *keys = reinterpret_cast<u64 *>(ens_ev_smem);             // [64]
    int *nan0 = reinterpret_cast<int *>(keys + ENS_SCORE_ROWS);   // [64]
    float *ml = reinterpret_cast<float *>(nan0 + ENS_SCORE_ROWS); // N rows of L values (CLR: A part, then B part)
    const int tid = threadIdx.x;
    const int rl = CLR ? 2 * L : L;
    for (int i = tid; i < N * rl; i += 256) {
        const int n = i / rl, e = i - n * rl;
        ml[i] = e < L ? a.d.ma[(size_t)n * a.d.ldm + e] : a.d.mb[(size_t)n * a.d.ldm + e - L];
    }
    for (int s = tid; s < T; s += 256) {
        keys[s] = ~0ull;
        nan0[s] = 0;
    }
    __syncthreads();
    {
        const float *ma = ml, *mb = CLR ? ml + L : ml;
        const int grp = tid >> 3, k = tid & 7;
        for (int p = grp; p < T * N; p += 32) {
            const int s = p / N, n = p - s * N;
            const size_t row = (size_t)(s0 + s) * a.d.ldx;
            float dd;
            if constexpr (MASKED) {
                // findRestrictedBmu (Som.cpp:316-322): node 0 seeds unconditionally, the others need the hits (group-uniform)
                if (n > 0 && a.min_hits && a.hits[n] < a.min_hits)
                    continue;
                dd = masked_group_dist(a.d.xa + row, a.valid + (size_t)(s0 + s) * a.vstride, ml + (size_t)n * L, L, k);
            } else {
                dd = vsom_group_dist<CLR>(a.d.xa + row, a.d.xb + row, ma + (size_t)n * rl, mb + (size_t)n * rl, L, k);
            }
            if (k == 0) {
                if (n == 0 && dd != dd)
                    nan0[s] = 1;
                atomicMin(&keys[s], vsom_key(dd, (uint32_t)n));
            }
        }
    }
    __syncthreads();
    // the rows' scoring: eight tid >> 3 takes rows tid >> 3 and 32 + (tid >> 3)
    const int c = tid & (EV_LANES - 1);
    const size_t R = (size_t)a.B;
#pragma unroll 1
    for (int h = 0; h < T; h += EV_ROWS_PER_WG) {        // (workgroup-uniform)
        const int sl = h + (tid >> 3);
        const bool live = sl < T;
        const int sr = live ? sl : T - 1;                // (a dead eight repeats the last row and stores nothing)
        const u64 key = keys[sr];
        const u64 idx = nan0[sr] ? 0ull : (key & 0xFFFFFFFFull);
        const float sq = nan0[sr] ? __uint_as_float(0x7FC00000u) : __uint_as_float((uint32_t)(key >> 32));
        const size_t i = (size_t)(s0 + sr);
        const float *xr = a.x + i * a.ldxs;
        const float *mr = ml + (size_t)idx * rl;
        const unsigned char *vr = (MASKED || a.valid) ? a.valid + i * (size_t)a.vstride : nullptr;
        auto model = [&](int d) -> float { return mr[d]; };
#include "vsom_eval_row.inc"
        unsigned nv = 0;
        if constexpr (MASKED) {
            for (int d = c; d < L; d += EV_LANES)
                nv += vr[d] != 0 ? 1u : 0u;
#pragma unroll
            for (int m = 4; m >= 1; m >>= 1)
                nv += __shfl_xor(nv, m);
        }
        if (live && c == 0) {
            if constexpr (!MASKED) {
                a.lastbmu[i] = idx;
                a.sqres[i] = sq;
            }
            reinterpret_cast<u64 *>(a.rows)[i] = idx;
            a.rows[2 * R + i] = __float_as_uint(sq);
            a.rows[3 * R + i] = __float_as_uint(s);
            a.rows[4 * R + i] = nrepl;
            if constexpr (MASKED)
                a.rows[5 * R + i] = nv;
        }
    }
}

// the LDS need of a member in ensemble_evaluate_many_kernel: that of the sibling search
static size_t ens_eval_smem(const vsom_ctx *c)
{
    const size_t rl = c->transform == VSOM_CLR ? 2 * c->part_len : c->part_len;
    return ENS_SCORE_ROWS * (sizeof(u64) + sizeof(int)) + (size_t)c->N * rl * sizeof(float);
}

// the fast-path rule (include/vsom_hip.h): would this member run in ensemble_evaluate_many_kernel?  The members that
// vsom_ensemble_bmu_batch (masked: vsom_ensemble_bmu_masked_batch) searches in its one launch, with rows.
static bool ens_eval_fast(const vsom_ensemble *e, const vsom_ctx *c, bool masked)
{
    if (c->cu || (masked && c->transform == VSOM_CLR) || !c->chunk_loaded || c->B == 0)
        return false;
    if ((size_t)c->N * c->part_len > 4096)
        return false;
    return ens_eval_smem(c) <= std::min(e->lds_limit, (size_t)64 << 10);      // (no attribute is raised)
}

int vsom_ensemble_evaluate_applies(const vsom_ensemble *e, size_t member, int masked)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (member >= e->m.size())
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: member index out of range");
    return ens_eval_fast(e, e->m[member], masked != 0) ? 1 : 0;
}

// Both evaluate calls (the callers have made their argument checks): pout (vsom_evaluate_batch per member, covered: a
// binary_host[k]) or mout (vsom_evaluate_masked_batch per member, covered: a valid_host[k]) is non-null.  The covered members
// on the fast path go as one launch per kind; their column arrays and validity bytes form one pinned image in the launch's
// descriptor slot, copied once.  Every other covered member with rows runs its single call while the launches run.
static int ens_evaluate(vsom_ensemble *e, const uint64_t *min_hits, const float *const *binary_host,
                        const float *const *continuous_host, const uint8_t *const *valid_host, const int *one_mask,
                        const vsom_evaluate_out *pout, const vsom_evaluate_masked_out *mout)
{
    const bool masked = mout != nullptr;
    const size_t n = e->m.size();
    VSOM_HIP_CHECK(hipSetDevice(e->device));
    EnsCall call(e);
    std::vector<size_t> asked(n);
    for (size_t k = 0; k < n; ++k)
        asked[k] = masked ? valid_host[k] != nullptr : binary_host[k] != nullptr;   // (a skipped member is not touched)
    if (int rc = join_members(e, asked.data(), true))
        return rc;
    const size_t words = masked ? EV_MROW_WORDS : EV_ROW_WORDS;
    ens_scratch(e, sizeof(EnsEvalDesc));
    std::vector<size_t> c_at(n, 0), v_at(n, 0), vbytes(n, 0), w_at(n, 0);
    std::vector<const uint8_t *> vh(n, nullptr);         // the member's validity bytes, or null (plain: every column valid)
    size_t itotal = 0, wtotal = 0;
    for (size_t k = 0; k < n; ++k) {
        const vsom_ctx *c = e->m[k];
        if (!asked[k])
            continue;
        vh[k] = valid_host ? valid_host[k] : nullptr;
        if (!ens_eval_fast(e, c, masked))
            continue;
        e->grp[k] = c->transform;
        e->smem[k] = ens_eval_smem(c);
        e->ext[k] = (unsigned)((c->B + ENS_SCORE_ROWS - 1) / ENS_SCORE_ROWS);
        c_at[k] = itotal;
        itotal += (2 * c->J * sizeof(float) + 15) / 16 * 16;
        if (vh[k]) {
            vbytes[k] = ((masked && one_mask && one_mask[k]) ? 1 : c->B) * (size_t)c->J;
            v_at[k] = itotal;
            itotal += (vbytes[k] + 15) / 16 * 16;
        }
        w_at[k] = wtotal;
        wtotal += (c->B * words + 3) / 4 * 4;            // (16-byte steps: the 8-byte units lead each member's words)
    }
    int rc = VSOM_OK;
    if (wtotal) {
        if (int jrc = call.join(ENS_LAUNCHED))
            return jrc;
        // the slot ens_launch is about to take: its last launch has completed, so its image may be rewritten
        auto &s = e->slot[e->next];
        if (s.valid)
            VSOM_HIP_CHECK(hipEventSynchronize(s.ev));
        VSOM_ALLOC_CHECK(vsom_grow_set(nullptr, 0, {vsom_member(s.img_host, std::max<size_t>(itotal, 1)),
                                                    vsom_member(s.img_dev, std::max<size_t>(itotal, 1))}));
        // (no kernel of an earlier call is running: every call ends in a wait)
        VSOM_ALLOC_CHECK(vsom_grow(e->mq_rows, wtotal, nullptr));
        for (size_t k = 0; k < n; ++k) {
            if (e->grp[k] < 0)
                continue;
            const size_t J = e->m[k]->J;
            float *cols = reinterpret_cast<float *>(s.img_host.p + c_at[k]);
            std::memcpy(cols, binary_host[k], J * sizeof(float));
            std::memcpy(cols + J, continuous_host[k], J * sizeof(float));
            if (vh[k])
                std::memcpy(s.img_host.p + v_at[k], vh[k], vbytes[k]);
        }
        if (itotal)
            VSOM_HIP_CHECK(hipMemcpyAsync(s.img_dev.p, s.img_host.p, itotal, hipMemcpyHostToDevice, call.ls));
        for (size_t k = 0; k < n; ++k) {
            if (e->grp[k] < 0)
                continue;
            const vsom_ctx *c = e->m[k];
            const bool clr = c->transform == VSOM_CLR;
            EnsEvalDesc a;
            a.d.xa = clr ? c->XP.p : c->Xs.p;
            a.d.xb = clr ? c->YP.p : c->Xs.p;
            a.d.ldx = (int)(clr ? c->part_pitch : c->xpitch);
            a.d.ma = c->map.p;
            a.d.mb = clr ? c->map.p + c->part_pitch : c->map.p;
            a.d.ldm = (int)c->pitch;
            a.d.L = (int)c->part_len;
            a.x = c->Xs.p;
            a.hits = c->hits.p;
            a.min_hits = masked && min_hits ? min_hits[k] : 0;
            a.valid = vh[k] ? s.img_dev.p + v_at[k] : nullptr;
            a.binary = reinterpret_cast<const float *>(s.img_dev.p + c_at[k]);
            a.continuous = a.binary + c->J;
            a.lastbmu = c->lastbmu.p;
            a.sqres = c->sqres.p;
            a.rows = e->mq_rows.p + w_at[k];
            a.ldxs = (int)c->xpitch;
            a.vstride = (masked && one_mask && one_mask[k]) ? 0 : (int)c->J;
            a.B = (int)c->B;
            a.N = (int)c->N;
            a.C = (int)std::min<size_t>(c->J, c->D);
            std::memcpy(e->desc.data() + k * sizeof(a), &a, sizeof(a));
        }
        static void (*const kernel[2][3])(const EnsEvalDesc *) = {
            {ensemble_evaluate_many_kernel<VSOM_STANDARD, false>, ensemble_evaluate_many_kernel<VSOM_MEDIAN, false>,
             ensemble_evaluate_many_kernel<VSOM_CLR, false>},
            {ensemble_evaluate_many_kernel<VSOM_STANDARD, true>, ensemble_evaluate_many_kernel<VSOM_MEDIAN, true>, nullptr}};
        rc = ens_launch(call, ENS_JOINED, 3, sizeof(EnsEvalDesc), ENS_MAX_Y, ens_always_ready,
                        [masked](int kind, const void *d, unsigned cnt, size_t smem, unsigned tiles, hipStream_t st) -> int {
                            hipLaunchKernelGGL(kernel[masked][kind], dim3(tiles, cnt), dim3(256), smem, st,
                                               static_cast<const EnsEvalDesc *>(d));
                            VSOM_HIP_CHECK_AS(hipGetLastError(), "ensemble_evaluate_many_kernel");
                            return VSOM_OK;
                        });
    }
    // the other members through their single calls, while the launches run (no rows: *error = 0 and nothing else)
    for (size_t k = 0; k < n && !rc; ++k) {
        vsom_ctx *c = e->m[k];
        if (!asked[k] || e->grp[k] >= 0)
            continue;
        rc = masked ? launch_evaluate_masked(c, min_hits ? min_hits[k] : 0, 0, c->B, binary_host[k], continuous_host[k],
                                             valid_host[k], one_mask ? one_mask[k] : 0, &mout[k])
                    : launch_evaluate(c, 0, c->B, binary_host[k], continuous_host[k], vh[k], &pout[k]);
    }
    if ((rc = call.end(rc)))
        return rc;
    // results of the launched members: the kernel stored them into the pinned buffer
    for (size_t k = 0; k < n; ++k) {
        if (e->grp[k] < 0)
            continue;
        const size_t b = e->m[k]->B;
        const unsigned *p = e->mq_rows.p + w_at[k];
        double *error;
        if (masked) {
            const vsom_evaluate_masked_out &o = mout[k];
            ens_mq_copy_out(p, b, {o.bmu, o.dist, o.bsum, o.nrepl, o.nvalid});
            error = o.error;
        } else {
            const vsom_evaluate_out &o = pout[k];
            ens_mq_copy_out(p, b, {o.bmu, o.dist, o.bsum, o.nrepl});
            error = o.error;
        }
        if (error)
            *error = ev_running_mean(reinterpret_cast<const float *>(p + 2 * b), reinterpret_cast<const float *>(p + 3 * b), b);
    }
    return VSOM_OK;
}

// what both evaluate calls check for a covered member: its column arrays, its kind, its chunk
static int ens_evaluate_member(const vsom_ensemble *e, size_t k, bool masked, const float *binary, const float *continuous,
                               std::string &buf)
{
    const vsom_ctx *c = e->m[k];
    if (!binary || !continuous)
        return ens_fail(k, "binary_host or continuous_host is null");
    if (masked) {
        if (const char *why = ens_masked_query_refusal(c, "vsom_evaluate_masked_batch", buf))
            return ens_fail(k, why);
        return VSOM_OK;
    }
    if (c->cu)
        return ens_fail(k, "vsom_evaluate_batch: custom contexts are not supported");
    if (const char *why = ens_rows_refusal(c))
        return ens_fail(k, why);
    return VSOM_OK;
}

int vsom_ensemble_evaluate_batch(vsom_ensemble *e, const float *const *binary_host, const float *const *continuous_host,
                                 const uint8_t *const *valid_host, const vsom_evaluate_out *out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    if (!binary_host || !continuous_host)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null binary_host or continuous_host array");
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null out array");
    std::string buf;
    for (size_t k = 0; k < e->m.size(); ++k)
        if (binary_host[k])
            if (int rc = ens_evaluate_member(e, k, false, binary_host[k], continuous_host[k], buf))
                return rc;
    return ens_evaluate(e, nullptr, binary_host, continuous_host, valid_host, nullptr, out, nullptr);
}

int vsom_ensemble_evaluate_masked_batch(vsom_ensemble *e, const uint64_t *min_hits, const float *const *binary_host,
                                        const float *const *continuous_host, const uint8_t *const *valid_host,
                                        const int *one_mask, const vsom_evaluate_masked_out *out)
{
    if (int rc = ens_masked_query_arrays(e, valid_host, out))
        return rc;
    if (!binary_host || !continuous_host)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_ensemble: null binary_host or continuous_host array");
    std::string buf;
    for (size_t k = 0; k < e->m.size(); ++k)
        if (valid_host[k])
            if (int rc = ens_evaluate_member(e, k, true, binary_host[k], continuous_host[k], buf))
                return rc;
    return ens_evaluate(e, min_hits, binary_host, continuous_host, valid_host, one_mask, nullptr, out);
}

// Som::updateUMatrix of every member (vsom_umatrix.hip): members whose model and sigma rows fit LDS in one launch per kind
// (plain / CLR), one workgroup per member, the results stored into each member's own buffer and into one pinned buffer
// for all of them; every other member through vsom_umatrix.  Nothing here reads staged rows: rows_free_valid stays.
int vsom_ensemble_umatrix(vsom_ensemble *e, double *const *u_out)
{
    if (!e)
        return vsom_fail(VSOM_ERR_INVALID, "null ensemble");
    const size_t n = e->m.size();
    for (size_t k = 0; k < n; ++k)
        if (const char *why = vsom_umatrix_refusal(e->m[k]))
            return ens_fail(k, why);
    VSOM_HIP_CHECK(hipSetDevice(e->device));
    EnsCall call(e);
    if (int rc = join_members(e, nullptr, false))
        return rc;
    const size_t lds_cap = std::min(e->lds_limit, (size_t)64 << 10);
    ens_scratch(e, sizeof(VsomUmDesc));
    std::vector<size_t> at(n, 0);                // the member's place in the pinned result buffer
    size_t total = 0;
    for (size_t k = 0; k < n; ++k) {
        vsom_ctx *c = e->m[k];
        if ((size_t)c->N * c->part_len > 4096 || vsom_umatrix_many_smem(c) > lds_cap)
            continue;
        if (int rc = vsom_umatrix_ensure(c))
            return rc;
        e->grp[k] = c->transform == VSOM_CLR ? 1 : 0;
        e->smem[k] = vsom_umatrix_many_smem(c);
        if (u_out && u_out[k]) {
            at[k] = total;
            total += c->N;
        }
    }
    if (total > e->um_out.cap)                 // (no kernel of an earlier call is running: every call ends in a wait)
        VSOM_ALLOC_CHECK(vsom_grow(e->um_out, total, nullptr));
    for (size_t k = 0; k < n; ++k) {
        if (e->grp[k] < 0)
            continue;
        vsom_ctx *c = e->m[k];
        const VsomUmDesc d = {c->map.p, c->sigma.p, c->umatrix.p, (u_out && u_out[k]) ? e->um_out.p + at[k] : nullptr,
                              (int)c->pitch, (int)c->D, (int)c->part_len, (int)c->part_pitch, (int)c->W, (int)c->H};
        std::memcpy(e->desc.data() + k * sizeof(d), &d, sizeof(d));
    }
    int rc = ens_launch(call, ENS_PLAIN, 2, sizeof(VsomUmDesc), ENS_NO_CAP, ens_always_ready,
                        [e](int clr, const void *d, unsigned cnt, size_t smem, unsigned, hipStream_t s) {
                            if (int rc = vsom_umatrix_launch_many(clr, static_cast<const VsomUmDesc *>(d), cnt, smem, s))
                                return rc;
                            for (size_t k = 0; k < e->m.size(); ++k)
                                if (e->grp[k] == clr)
                                    e->m[k]->um_valid = true;
                            return (int)VSOM_OK;
                        });
    // the other members: every launch enqueued first, then the copies (or the wait)
    for (size_t k = 0; k < n && !rc; ++k)
        if (e->grp[k] < 0)
            rc = vsom_umatrix(e->m[k], nullptr);
    for (size_t k = 0; k < n && !rc; ++k)
        if (e->grp[k] < 0) {
            if (u_out && u_out[k])
                rc = vsom_get_umatrix(e->m[k], u_out[k]);
            else
                rc = vsom_synchronize(e->m[k]);
        }
    if ((rc = call.end(rc)))
        return rc;
    for (size_t k = 0; k < n; ++k)
        if (e->grp[k] >= 0 && u_out && u_out[k])
            std::memcpy(u_out[k], e->um_out.p + at[k], (size_t)e->m[k]->N * sizeof(double));
    return VSOM_OK;
}
