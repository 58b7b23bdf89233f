// vsom_capi.hip -- the extern "C" entry points declared in include/vsom_hip.h.
#include "vsom_internal.hpp"
#include "vsom_phase2_plan.hpp"

#include <cstring>
#include <cstdlib>
#include <cmath>
#include <new>

static thread_local std::string g_last_error;

void vsom_set_error(const std::string &msg) { g_last_error = msg; }
int vsom_fail(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

TimerScope::TimerScope(vsom_ctx *ctx, int w) : c(ctx), which(w), on((ctx->timing >> w) & 1u)
{
    if (!on)
        return;
    if (!c->ev_pool.empty()) {
        ev = c->ev_pool.back();
        c->ev_pool.pop_back();
    } else {
        if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) {
            on = false;
            return;
        }
    }
    ev.which = which;
    (void)hipEventRecord(ev.a, c->stream);
}
TimerScope::~TimerScope()
{
    if (!on)
        return;
    (void)hipEventRecord(ev.b, c->stream);
    c->ev_live.push_back(ev);
}

static inline uint32_t roundup(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

// ---- pieces of the double-buffered ingest shared with the multi-GPU group (vsom_group.hip) -------------
// Rows [r0,r1) of a B-row host chunk -> the same rows of the context's NEXT raw device buffer, on the
// copy stream (a group copies each device's shard only and all-gathers the rest over xGMI).
int vsom_prefetch_rows(vsom_ctx *c, const float *x_host, size_t B, size_t r0, size_t r1)
{
    CHECK_CTX_NOJOIN(c);
    if (B > 0 && !x_host)
        return vsom_fail(VSOM_ERR_INVALID, "x_host is null");
    if (B > 0x7FFFFFFFull)
        return vsom_fail(VSOM_ERR_INVALID, "chunk too large");
    if (r0 > r1 || r1 > B)
        return vsom_fail(VSOM_ERR_INVALID, "row range out of bounds");
    const int k = c->next_slot;
    const size_t need = B * c->J;
    // the staging kernels of the chunk committed from this slot two prefetches ago must be done
    if (c->staged_valid[k])
        VSOM_HIP_CHECK(hipStreamWaitEvent(c->copy_stream, c->ev_staged[k], 0));
    if (need > c->Xnext[k].cap) {
        if (c->staged_valid[k])
            VSOM_HIP_CHECK(hipEventSynchronize(c->ev_staged[k]));
        VSOM_ALLOC_CHECK(vsom_grow(c->Xnext[k], need, c->copy_stream, VSOM_BUF_SYNC));
    }
    if (r1 > r0)
        VSOM_HIP_CHECK(hipMemcpyAsync(c->Xnext[k].p + r0 * c->J, x_host + r0 * c->J, (r1 - r0) * c->J * 4,
                                      hipMemcpyHostToDevice, c->copy_stream));
    VSOM_HIP_CHECK(hipEventRecord(c->ev_copied[k], c->copy_stream));
    c->Bnext = B;
    c->ready_slot = k;
    c->next_slot = k ^ 1;
    return VSOM_OK;
}

// first half of vsom_commit_chunk: the compute stream waits for the copy; *raw = the B x J rows
int vsom_commit_begin(vsom_ctx *c, float **raw, size_t *B)
{
    CHECK_CTX_KEEP(c);
    if (c->ready_slot < 0)
        return vsom_fail(VSOM_ERR_INVALID, "no prefetched chunk to commit");
    const int k = c->ready_slot;
    VSOM_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_copied[k], 0));
    *raw = c->Xnext[k].p;
    *B = c->Bnext;
    return VSOM_OK;
}

// second half: stage the rows (lastBMU := 0) and mark the slot reusable once staging has read it
int vsom_commit_end(vsom_ctx *c)
{
    CHECK_CTX_KEEP(c);
    if (c->ready_slot < 0)
        return vsom_fail(VSOM_ERR_INVALID, "no prefetched chunk to commit");
    const int k = c->ready_slot;
    c->ready_slot = -1;
    if (c->ahead_valid)           // staged beside the previous epoch (vsom_prefetch_chunk): nothing left to launch
        return vsom_adopt_ahead(c);
    int rc = vsom_set_chunk_device(c, c->Xnext[k].p, c->Bnext);
    if (rc)
        return rc;
    VSOM_HIP_CHECK(hipEventRecord(c->ev_staged[k], c->stream));
    c->staged_valid[k] = true;
    return VSOM_OK;
}

int ensure_chunk_capacity(vsom_ctx *c, size_t B)
{
    if (B <= c->Bcap)
        return VSOM_OK;
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->copy_stream));
    c->ahead_valid = false;       // (a chunk staged ahead into the old buffers is staged anew at its commit)
    c->partial.reset();
    c->Bcap = 0;
    // no chunk is staged from here on: should an allocation below fail, later entry points report
    // "no chunk loaded" instead of launching kernels on null buffers
    c->B = 0;
    c->chunk_loaded = false;
    size_t cap = (B + 63) / 64 * 64;
    // the fills below go to the context's stream: hipMemset would run on the null stream, which a
    // non-blocking stream does not wait for -- the fill could then land on top of the rows the staging
    // kernel writes next (seen as a few zero sample rows in one search of ~600 random cases)
    // the assembly update kernel reads up to 2 sample rows past the chunk and touches rows up to
    // PF_ROWS + 3 past it (gen_update_asm.py, load_cw)
    // XP / YP (CLR) like Xs: the pipelined update kernels read one sample pair past the chunk
    const size_t pp_rows = c->transform == VSOM_CLR ? (cap + VSOM_ROW_PAD) * c->part_pitch : 0;
    VSOM_ALLOC_CHECK(vsom_grow_set(c->stream, VSOM_BUF_REBUILD,
                                 {vsom_member(c->Xs, (cap + VSOM_ROW_PAD) * c->xpitch, VSOM_BUF_ZERO),
                                  vsom_member(c->XP, pp_rows, VSOM_BUF_ZERO), vsom_member(c->YP, pp_rows, VSOM_BUF_ZERO),
                                  vsom_member(c->lastbmu, cap, VSOM_BUF_ZERO), vsom_member(c->lastbmu_alt, cap, VSOM_BUF_ZERO),
                                  vsom_member(c->sqres, cap, VSOM_BUF_ZERO), vsom_member(c->nan0, cap, VSOM_BUF_ZERO)}));
    c->Bcap = cap;
    return VSOM_OK;
}

extern "C" {

const char *vsom_last_error(void) { return g_last_error.c_str(); }

int vsom_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

// streams, events and modules; the buffers are the owners' (vsom_buf.hpp): they go with `delete c`, on c->device
static int free_all(vsom_ctx *c)
{
    vsom_custom_destroy(c);
    for (int i = 0; i < 2; ++i) {
        if (c->lut_ev[i])
            (void)hipEventDestroy(c->lut_ev[i]);
        if (c->lutd_ev[i])
            (void)hipEventDestroy(c->lutd_ev[i]);
        if (c->acm_ev[i])
            (void)hipEventDestroy(c->acm_ev[i]);
    }
    for (auto &e : c->ev_live) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    for (auto &e : c->ev_pool) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    if (c->upd_module)
        (void)hipModuleUnload((hipModule_t)c->upd_module);
    if (c->aux_stream) {
        (void)hipStreamSynchronize(c->aux_stream);
        (void)hipStreamDestroy(c->aux_stream);
    }
    if (c->copy_stream) {
        (void)hipStreamSynchronize(c->copy_stream);
        (void)hipStreamDestroy(c->copy_stream);
    }
    for (int i = 0; i < 2; ++i) {
        if (c->ev_copied[i])
            (void)hipEventDestroy(c->ev_copied[i]);
        if (c->ev_staged[i])
            (void)hipEventDestroy(c->ev_staged[i]);
    }
    if (c->ev_rows_free)
        (void)hipEventDestroy(c->ev_rows_free);
    if (c->ev_ahead)
        (void)hipEventDestroy(c->ev_ahead);
    if (c->ev_fork)
        (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join)
        (void)hipEventDestroy(c->ev_join);
    if (c->own_stream)
        (void)hipStreamDestroy(c->own_stream);
    return 0;
}

int vsom_create(vsom_ctx **out, int device, uint32_t width, uint32_t height, uint32_t in_len,
                int transform)
{
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (width == 0 || height == 0 || in_len == 0)
        return vsom_fail(VSOM_ERR_INVALID, "width, height and in_len must be > 0");
    if (transform < VSOM_STANDARD || transform > VSOM_CLR)
        return vsom_fail(VSOM_ERR_INVALID, "unknown transformation kind");
    if (transform == VSOM_CLR && in_len < 2)
        return vsom_fail(VSOM_ERR_INVALID, "CombinatorialLinearRegression needs in_len >= 2");
    if ((uint64_t)width * height > 0x7FFFFFFFull)
        return vsom_fail(VSOM_ERR_INVALID, "map too large");
    int sigma_mode = VSOM_SIGMA_AUTO;
    if (const char *e = std::getenv("VSOM_SIGMA_MODE")) {  // initial vsom_set_sigma_mode: auto / eager / lazy, nothing else
        const std::string v(e);
        if (v == "eager")
            sigma_mode = VSOM_SIGMA_EAGER;
        else if (v == "lazy")
            sigma_mode = VSOM_SIGMA_LAZY;
        else if (v != "auto")
            return vsom_fail(VSOM_ERR_INVALID, "VSOM_SIGMA_MODE is '" + v + "': auto, eager or lazy");
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return vsom_fail(VSOM_ERR_HIP, "no HIP device available (libvsom_hip has no CPU fallback)");
    if (device < 0 || device >= ndev)
        return vsom_fail(VSOM_ERR_INVALID, "device index out of range");
    VSOM_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    VSOM_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return vsom_fail(VSOM_ERR_UNSUPPORTED,
                         std::string("libvsom_hip is built for gfx950 only, device is ") + prop.gcnArchName);

    vsom_ctx *c = new (std::nothrow) vsom_ctx();
    if (!c)
        return vsom_fail(VSOM_ERR_NOMEM, "out of host memory");
    c->device = device;
    c->W = width;
    c->H = height;
    c->J = in_len;
    c->N = width * height;
    c->transform = transform;
    // Transformation::Length (Transformation.cpp:31-35, 69-73, 162-165)
    c->D = transform == VSOM_CLR ? in_len * (in_len - 1u) : in_len;
    c->nparts = transform == VSOM_CLR ? 2 : 1;
    c->part_len = c->D / c->nparts;
    c->part_pitch = roundup(c->part_len, VSOM_TK);
    c->pitch = c->nparts * c->part_pitch;
    c->xpitch = roundup(c->J, VSOM_TK);
    if (const char *e = std::getenv("VSOM_NO_TINY"))
        c->use_tiny = !(e[0] == '1');
    if (const char *e = std::getenv("VSOM_COMPACT_MIN_ROWS"))     // development: initial vsom_set_column_compaction
        c->cc_min_rows = std::atol(e);
    if (const char *e = std::getenv("VSOM_NO_DEDUPE"))
        c->dedupe = !(e[0] == '1');     // A/B measurements of the duplicate-row pass of the exact search
    c->sigma_mode = sigma_mode;
    if (const char *e = std::getenv("VSOM_NO_CHAIN"))
        c->use_chain = !(e[0] == '1');  // debugging aid: lane = node update kernel on small maps too

    int rc = VSOM_OK;
    do {
        // the copy stream also runs the staging kernels of a chunk staged AHEAD, beside the chains of the current one
        // (vsom_prefetch_chunk): lowest priority, so that the dispatcher hands them the slots the chain kernel leaves
        // free at its ragged end instead of taking turns with it (at equal priority the chains of a 128x128 map lost
        // 0.09 ms to 0.05 ms of staging kernels: tools/exp/ab_stage.py)
        int prio_low = 0, prio_high = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
        if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
            hipStreamCreateWithPriority(&c->copy_stream, hipStreamNonBlocking, prio_low) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_copied[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_copied[1], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_staged[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_staged[1], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_rows_free, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_ahead, hipEventDisableTiming) != hipSuccess) {
            rc = vsom_fail(VSOM_ERR_HIP, "hipStreamCreate failed");
            break;
        }
        c->stream = c->own_stream;
        const size_t nd = (size_t)c->N * c->pitch;
        // (mse: pinned host memory the kernels write through; vsom_get_mse reads it after a stream wait)
        if (vsom_grow_set(c->stream, 0, {vsom_member(c->map, nd, VSOM_BUF_ZERO), vsom_member(c->sigma, nd, VSOM_BUF_ZERO),
                                         vsom_member(c->S, nd, VSOM_BUF_ZERO), vsom_member(c->weight, c->N, VSOM_BUF_ZERO),
                                         vsom_member(c->hits, c->N, VSOM_BUF_ZERO), vsom_member(c->mse, 4, VSOM_BUF_ZERO),
                                         vsom_member(c->onl_state, VSOM_ONL_STATE_BYTES / sizeof(u64)),
                                         vsom_member(c->onl_f, 16)}) != hipSuccess) {
            (void)hipGetLastError();
            rc = vsom_fail(VSOM_ERR_NOMEM, "hipMalloc of model state failed");
            break;
        }
        if (transform == VSOM_CLR) {
            // pair tables, i<j lexicographic (Transformation.cpp:94-101; tests/test1.cpp:18-43)
            std::vector<int> pi(c->part_len), pj(c->part_len);
            size_t p = 0;
            for (uint32_t i = 0; i < in_len; ++i)
                for (uint32_t j = i + 1; j < in_len; ++j) {
                    pi[p] = (int)i;
                    pj[p] = (int)j;
                    ++p;
                }
            if (vsom_grow_set(c->stream, 0, {vsom_member(c->pair_i, p), vsom_member(c->pair_j, p)}) != hipSuccess) {
                (void)hipGetLastError();
                rc = vsom_fail(VSOM_ERR_NOMEM, "hipMalloc of pair tables failed");
                break;
            }
            (void)hipMemcpy(c->pair_i.p, pi.data(), p * 4, hipMemcpyHostToDevice);
            (void)hipMemcpy(c->pair_j.p, pj.data(), p * 4, hipMemcpyHostToDevice);
        }
        if (hipStreamSynchronize(c->stream) != hipSuccess) {
            rc = vsom_fail(VSOM_ERR_HIP, "initialisation failed");
            break;
        }
    } while (0);
    if (rc != VSOM_OK) {
        std::string keep = g_last_error;
        free_all(c);
        delete c;
        g_last_error = keep;
        return rc;
    }
    *out = c;
    return VSOM_OK;
}

void vsom_destroy(vsom_ctx *c)
{
    if (!c)
        return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->aux_stream)
        (void)hipStreamSynchronize(c->aux_stream);
    free_all(c);
    delete c;
}

int vsom_set_stream(vsom_ctx *c, void *hip_stream)
{
    CHECK_CTX(c);
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return VSOM_OK;
}

int vsom_synchronize(vsom_ctx *c)
{
    CHECK_CTX_KEEP(c);
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_set_bmu_mode(vsom_ctx *c, int mode)
{
    if (!c || mode < VSOM_BMU_AUTO || mode > VSOM_BMU_SHORTLIST)
        return vsom_fail(VSOM_ERR_INVALID, "bad bmu mode");
    c->bmu_mode = mode;
    return VSOM_OK;
}

int vsom_get_shortlist_stats(vsom_ctx *c, uint32_t *out)
{
    CHECK_CTX_KEEP(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_get_shortlist_stats");
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "null output");
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 4; ++i)
        out[i] = c->sl_fb.p ? ((volatile unsigned *)c->sl_fb.p)[i] : 0u;
    return VSOM_OK;
}

int vsom_set_column_compaction(vsom_ctx *c, long min_rows)
{
    if (!c)
        return vsom_fail(VSOM_ERR_INVALID, "null context");
    VSOM_CUSTOM_REFUSE(c, "column compaction");
    c->cc_min_rows = min_rows;
    c->cc_skip = 0;
    return VSOM_OK;
}

int vsom_set_row_dedupe(vsom_ctx *c, double min_work)
{
    if (!c)
        return vsom_fail(VSOM_ERR_INVALID, "null context");
    VSOM_CUSTOM_REFUSE(c, "row dedupe");
    c->dd_min_work = min_work;
    return VSOM_OK;
}

int vsom_set_sigma_mode(vsom_ctx *c, int mode)
{
    if (!c || mode < VSOM_SIGMA_AUTO || mode > VSOM_SIGMA_LAZY)
        return vsom_fail(VSOM_ERR_INVALID, "bad sigma mode");
    c->sigma_mode = mode;        // (a sigmaMap already pending stays pending: every reader materialises it in any mode)
    return VSOM_OK;
}

int vsom_sigma_flush(vsom_ctx *c)
{
    CHECK_CTX(c);                // (materialises)
    return VSOM_OK;
}

int vsom_sigma_stats(vsom_ctx *c, uint64_t *out)
{
    if (!c || !out)
        return vsom_fail(VSOM_ERR_INVALID, "null context or output");
    for (int i = 0; i < 3; ++i)
        out[i] = c->sg_stats[i];
    out[3] = c->sg.on ? 1 : 0;
    return VSOM_OK;
}

int vsom_set_update_mode(vsom_ctx *c, int mode)
{
    if (!c || (mode != VSOM_UPDATE_STRICT && mode != VSOM_UPDATE_FMA && mode != VSOM_UPDATE_FMA_SIGMA))
        return vsom_fail(VSOM_ERR_INVALID, "bad update mode");
    if (mode != VSOM_UPDATE_STRICT)
        VSOM_CUSTOM_REFUSE(c, "a contracted update mode");
    c->update_mode = mode;
    return VSOM_OK;
}

uint32_t vsom_depth(const vsom_ctx *c) { return c ? c->D : 0; }
uint32_t vsom_nodes(const vsom_ctx *c) { return c ? c->N : 0; }
uint32_t vsom_residual_len(const vsom_ctx *c) { return c ? (c->cu ? vsom_custom_residual_len(c) : c->part_len) : 0; }
size_t vsom_chunk_size(const vsom_ctx *c) { return c ? c->B : 0; }

// (caller arrays may be only 4-byte aligned: the words are loaded with memcpy, not through a uint64_t pointer)
static bool all_zero_bits(const void *p, size_t bytes)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    size_t i = 0;
    for (; i + 64 <= bytes; i += 64) {
        uint64_t w[8];
        std::memcpy(w, b + i, 64);
        if (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7])
            return false;
    }
    for (; i < bytes; ++i)
        if (b[i])
            return false;
    return true;
}

// host [N][D] <-> device [N][pitch] (each part separately for CLR).  Host -> device: an all-zero array (what
// Som::randomInitialize hands over for sigmaMap / SMap, Som.cpp:977-997) is a device fill; anything else travels through a
// pinned staging buffer -- a strided copy out of pageable memory took 5 ms per 4 MB array (tests/perf/ref_harness.py).
static int copy_rows(vsom_ctx *c, float *dev, const float *host_in, float *host_out)
{
    const size_t bytes = (size_t)c->N * c->D * 4;
    if (host_in && all_zero_bits(host_in, bytes)) {
        VSOM_HIP_CHECK(hipMemsetAsync(dev, 0, (size_t)c->N * c->pitch * 4, c->stream));   // (pad columns are zero anyway)
        return VSOM_OK;
    }
    if (host_in && bytes <= ((size_t)256 << 20)) {
        const size_t n = (size_t)c->N * c->D;
        if (n > c->st_pinned.cap) {
            VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
            if (vsom_grow(c->st_pinned, n, c->stream) != hipSuccess)
                (void)hipGetLastError();
        }
        if (c->st_pinned.cap >= n) {
            VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));       // the previous array's copy out of the buffer
            std::memcpy(c->st_pinned.p, host_in, bytes);
            host_in = c->st_pinned.p;
        }
    }
    for (uint32_t part = 0; part < c->nparts; ++part) {
        float *d = dev + (size_t)part * c->part_pitch;
        if (host_in) {
            const float *h = host_in + (size_t)part * c->part_len;
            VSOM_HIP_CHECK(hipMemcpy2DAsync(d, (size_t)c->pitch * 4, h, (size_t)c->D * 4,
                                            (size_t)c->part_len * 4, c->N, hipMemcpyHostToDevice,
                                            c->stream));
        } else {
            float *h = host_out + (size_t)part * c->part_len;
            VSOM_HIP_CHECK(hipMemcpy2DAsync(h, (size_t)c->D * 4, d, (size_t)c->pitch * 4,
                                            (size_t)c->part_len * 4, c->N, hipMemcpyDeviceToHost,
                                            c->stream));
        }
    }
    return VSOM_OK;
}

int vsom_set_state(vsom_ctx *c, const float *map, const float *sigma, const float *S,
                   const float *weight, const uint64_t *bmu_hits)
{
    CHECK_CTX(c);
    int rc;
    if (map && (rc = copy_rows(c, c->map.p, map, nullptr)))
        return rc;
    if (sigma && (rc = copy_rows(c, c->sigma.p, sigma, nullptr)))
        return rc;
    if (S && (rc = copy_rows(c, c->S.p, S, nullptr)))
        return rc;
    if (weight) {
        if (all_zero_bits(weight, (size_t)c->N * 4))
            VSOM_HIP_CHECK(hipMemsetAsync(c->weight.p, 0, (size_t)c->N * 4, c->stream));
        else
            VSOM_HIP_CHECK(hipMemcpyAsync(c->weight.p, weight, (size_t)c->N * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (bmu_hits) {
        if (all_zero_bits(bmu_hits, (size_t)c->N * 8))
            VSOM_HIP_CHECK(hipMemsetAsync(c->hits.p, 0, (size_t)c->N * 8, c->stream));
        else
            VSOM_HIP_CHECK(hipMemcpyAsync(c->hits.p, bmu_hits, (size_t)c->N * 8, hipMemcpyHostToDevice, c->stream));
    }
    if (c->cu && sigma)
        return vsom_custom_after_set_state(c);     // (synchronises)
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_get_state(vsom_ctx *c, float *map, float *sigma, float *S, float *weight, uint64_t *bmu_hits)
{
    CHECK_CTX(c);
    int rc;
    if (map && (rc = copy_rows(c, c->map.p, nullptr, map)))
        return rc;
    if (sigma && (rc = copy_rows(c, c->sigma.p, nullptr, sigma)))
        return rc;
    if (S && (rc = copy_rows(c, c->S.p, nullptr, S)))
        return rc;
    if (weight)
        VSOM_HIP_CHECK(hipMemcpyAsync(weight, c->weight.p, (size_t)c->N * 4, hipMemcpyDeviceToHost, c->stream));
    if (bmu_hits)
        VSOM_HIP_CHECK(hipMemcpyAsync(bmu_hits, c->hits.p, (size_t)c->N * 8, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_set_chunk_device(vsom_ctx *c, const float *x_dev, size_t B)
{
    CHECK_CTX_KEEP(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_set_chunk_device");
    if (B > 0 && !x_dev)
        return vsom_fail(VSOM_ERR_INVALID, "x_dev is null");
    if (B > 0x7FFFFFFFull)
        return vsom_fail(VSOM_ERR_INVALID, "chunk too large");
    int rc = ensure_chunk_capacity(c, B);
    if (rc)
        return rc;
    c->B = B;
    c->chunk_loaded = true;
    return launch_stage_chunk(c, x_dev, B);
}

static int upload_chunk_impl(vsom_ctx *c, const float *x_host, size_t B, bool wait)
{
    CHECK_CTX_KEEP(c);
    if (c->cu)
        return vsom_custom_upload(c, x_host, B, wait);
    if (B > 0 && !x_host)
        return vsom_fail(VSOM_ERR_INVALID, "x_host is null");
    size_t need = B * c->J;
    VSOM_ALLOC_CHECK(vsom_grow(c->Xraw, need, c->stream, VSOM_BUF_SYNC));
    if (need)
        VSOM_HIP_CHECK(hipMemcpyAsync(c->Xraw.p, x_host, need * 4, hipMemcpyHostToDevice, c->stream));
    int rc = vsom_set_chunk_device(c, c->Xraw.p, B);
    if (rc)
        return rc;
    if (wait)
        VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));   // x_host may be reused by the caller
    return VSOM_OK;
}

int vsom_upload_chunk(vsom_ctx *c, const float *x_host, size_t B) { return upload_chunk_impl(c, x_host, B, true); }

// the hooks' value_weight on a custom context: the loader's column weights (they belong to the context) and the loaded
// chunk's validity (it belongs to the chunk: every call that makes a new chunk current resets it)
int vsom_set_column_weights(vsom_ctx *c, const float *weights_host)
{
    VSOM_CUSTOM_ONLY(c, "vsom_set_column_weights");
    CHECK_CTX_KEEP(c);
    return vsom_custom_set_weights(c, weights_host);
}

int vsom_set_chunk_validity(vsom_ctx *c, const uint8_t *valid_host, int one_mask)
{
    VSOM_CUSTOM_ONLY(c, "vsom_set_chunk_validity");
    CHECK_CTX_KEEP(c);
    return vsom_custom_set_validity(c, valid_host, one_mask);
}

// copy and staging enqueued on the context's stream, no wait: x_host (pinned: vsom_host_alloc) stays the caller's to keep
// unchanged until a call that synchronises the context has returned
int vsom_upload_chunk_async(vsom_ctx *c, const float *x_host, size_t B) { return upload_chunk_impl(c, x_host, B, false); }

int vsom_host_alloc(void **out, size_t bytes)
{
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "null output");
    *out = nullptr;
    if (bytes == 0)
        return VSOM_OK;
    if (vsom_mem.alloc(out, bytes, true) != hipSuccess) {
        (void)hipGetLastError();
        return vsom_fail(VSOM_ERR_NOMEM, "hipHostMalloc failed");
    }
    return VSOM_OK;
}

int vsom_host_free(void *p)
{
    if (p)
        VSOM_HIP_CHECK(vsom_mem.release(p, true));
    return VSOM_OK;
}

// what follows the copy of a prefetched chunk (or a chunk that already lives in HBM): its staging kernels on the copy
// stream, beside the epoch of the current chunk -- when that is possible now (vsom_can_stage_ahead), else at commit
static int stage_ahead_if_possible(vsom_ctx *c, const float *x_dev, size_t B)
{
    c->ahead_valid = false;       // (an abandoned ahead staging may still be running: ahead_rows stays set)
    if (!vsom_can_stage_ahead(c, B))
        return VSOM_OK;
    return launch_stage_chunk_ahead(c, x_dev, B);
}

int vsom_prefetch_chunk(vsom_ctx *c, const float *x_host, size_t B)
{
    if (c && c->cu) {
        CHECK_CTX_KEEP(c);
        return vsom_custom_prefetch(c, x_host, B);
    }
    int rc = vsom_prefetch_rows(c, x_host, B, 0, B);
    if (rc)
        return rc;
    c->next_dev_pending = false;
    const int k = c->ready_slot;
    if ((rc = stage_ahead_if_possible(c, c->Xnext[k].p, B)))
        return rc;
    if (c->ahead_valid) {         // the slot's raw rows have been read once the ahead staging is through
        VSOM_HIP_CHECK(hipEventRecord(c->ev_staged[k], c->copy_stream));
        c->staged_valid[k] = true;
    }
    return VSOM_OK;
}

int vsom_stage_next_device(vsom_ctx *c, const float *x_dev, size_t B)
{
    CHECK_CTX_NOJOIN(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_stage_next_device");
    if (B > 0 && !x_dev)
        return vsom_fail(VSOM_ERR_INVALID, "x_dev is null");
    if (B > 0x7FFFFFFFull)
        return vsom_fail(VSOM_ERR_INVALID, "chunk too large");
    c->ready_slot = -1;           // replaces a prefetched chunk that was never committed
    c->next_dev = x_dev;
    c->next_dev_B = B;
    c->next_dev_pending = true;
    return stage_ahead_if_possible(c, x_dev, B);
}

int vsom_prefetch_wait(vsom_ctx *c)
{
    CHECK_CTX_NOJOIN(c);
    if (c->cu)
        return VSOM_OK;             // (the prefetch took a host copy)
    VSOM_HIP_CHECK(hipStreamSynchronize(c->copy_stream));
    return VSOM_OK;
}

int vsom_commit_chunk(vsom_ctx *c)
{
    if (c && c->cu) {
        CHECK_CTX_KEEP(c);
        return vsom_custom_commit(c);
    }
    if (c && c->next_dev_pending) {       // vsom_stage_next_device: adopt what was staged ahead, or stage it now
        CHECK_CTX_KEEP(c);
        c->next_dev_pending = false;
        if (c->ahead_valid)
            return vsom_adopt_ahead(c);
        return vsom_set_chunk_device(c, c->next_dev, c->next_dev_B);
    }
    float *raw = nullptr;
    size_t B = 0;
    int rc = vsom_commit_begin(c, &raw, &B);
    if (rc)
        return rc;
    return vsom_commit_end(c);
}

__global__ void copy_u64_kernel(u64 *dst, const u64 *src, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        dst[i] = src[i];
}

int vsom_get_last_bmu(vsom_ctx *c, uint64_t *out_host)
{
    CHECK_CTX_KEEP(c);
    if (c->B && !out_host)
        return vsom_fail(VSOM_ERR_INVALID, "null output");
    // short chunks (the reference's own scenarios train 20 rows an epoch): one small kernel stores the indices into pinned
    // host memory -- a device-to-host copy into the caller's pageable buffer was 18 us beyond the wait for the chunk
    if (c->B && c->B <= 8192) {
        VSOM_ALLOC_CHECK(vsom_grow(c->out_pinned, 8192, c->stream));
        hipLaunchKernelGGL(copy_u64_kernel, dim3((unsigned)((c->B + 255) / 256)), dim3(256), 0, c->stream,
                           c->out_pinned.p, c->lastbmu.p, (int)c->B);
        VSOM_HIP_CHECK(hipGetLastError());
        VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
        std::memcpy(out_host, c->out_pinned.p, c->B * 8);
        return VSOM_OK;
    }
    if (c->B)
        VSOM_HIP_CHECK(hipMemcpyAsync(out_host, c->lastbmu.p, c->B * 8, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_set_last_bmu(vsom_ctx *c, const uint64_t *in_host)
{
    CHECK_CTX_KEEP(c);
    if (c->B && !in_host)
        return vsom_fail(VSOM_ERR_INVALID, "null input");
    for (size_t i = 0; i < c->B; ++i)
        if (in_host[i] >= c->N)
            return vsom_fail(VSOM_ERR_INVALID, "lastBMU index out of range");
    if (c->B)
        VSOM_HIP_CHECK(hipMemcpyAsync(c->lastbmu.p, in_host, c->B * 8, hipMemcpyHostToDevice, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_get_sqres(vsom_ctx *c, float *out_host)
{
    CHECK_CTX_KEEP(c);
    if (c->B && !out_host)
        return vsom_fail(VSOM_ERR_INVALID, "null output");
    if (c->B)
        VSOM_HIP_CHECK(hipMemcpyAsync(out_host, c->sqres.p, c->B * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

static int copy_search_results(vsom_ctx *c, uint64_t *idx, float *dist)
{
    if (idx && c->B)
        VSOM_HIP_CHECK(hipMemcpyAsync(idx, c->lastbmu.p, c->B * 8, hipMemcpyDeviceToHost, c->stream));
    if (dist && c->B)
        VSOM_HIP_CHECK(hipMemcpyAsync(dist, c->sqres.p, c->B * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_bmu_batch(vsom_ctx *c, uint64_t *idx_out_host, float *dist_out_host)
{
    CHECK_CTX(c);
    if (c->cu)
        return vsom_custom_bmu_batch(c, 0, idx_out_host, dist_out_host);
    CHECK_ROWS(c);
    int rc = launch_bmu_full(c, 0, c->B);
    if (rc)
        return rc;
    return copy_search_results(c, idx_out_host, dist_out_host);
}

int vsom_bmu_local_batch(vsom_ctx *c, uint64_t *idx_out_host, float *dist_out_host)
{
    CHECK_CTX(c);
    if (c->cu)
        return vsom_custom_bmu_batch(c, 1, idx_out_host, dist_out_host);
    CHECK_ROWS(c);
    int rc = launch_bmu_local(c, 0, c->B);
    if (rc)
        return rc;
    return copy_search_results(c, idx_out_host, dist_out_host);
}

// The checked pair lists of vsom_distances (from_map < 0) / vsom_distances_raw in, their distances out.  The scratch is the
// context's arena: a device allocation and free per call cost more than the queries' kernels (tests/perf/ref_harness.py).
static int pair_query(vsom_ctx *c, const uint64_t *nodes_host, const uint64_t *rows_host, size_t count, int from_map,
                      float *dist_out_host)
{
    vsom_layout lay;
    const auto hn = lay.add<u64>(count), hr = lay.add<u64>(count);
    const auto hd = lay.add<float>(count);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    u64 *dn = lay.at(hn), *dr = lay.at(hr);
    float *dd = lay.at(hd);
    VSOM_HIP_CHECK(hipMemcpyAsync(dn, nodes_host, count * 8, hipMemcpyHostToDevice, c->stream));
    VSOM_HIP_CHECK(hipMemcpyAsync(dr, rows_host, count * 8, hipMemcpyHostToDevice, c->stream));
    if (int rc = from_map < 0 ? launch_pair_dist(c, dn, dr, count, dd) : launch_raw_dist(c, dn, dr, count, from_map, dd))
        return rc;
    VSOM_HIP_CHECK(hipMemcpyAsync(dist_out_host, dd, count * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_distances(vsom_ctx *c, const uint64_t *nodes_host, const uint64_t *rows_host, size_t count,
                   float *dist_out_host)
{
    CHECK_CTX(c);
    if (c->cu)
        return vsom_custom_distances(c, nodes_host, rows_host, count, dist_out_host);
    CHECK_ROWS(c);
    if (count == 0)
        return VSOM_OK;
    if (!nodes_host || !rows_host || !dist_out_host)
        return vsom_fail(VSOM_ERR_INVALID, "null argument");
    if (count > 0x0FFFFFFFull)
        return vsom_fail(VSOM_ERR_INVALID, "too many pairs");
    for (size_t i = 0; i < count; ++i)
        if (nodes_host[i] >= c->N || rows_host[i] >= c->B)
            return vsom_fail(VSOM_ERR_INVALID, "pair index out of range");
    return pair_query(c, nodes_host, rows_host, count, -1, dist_out_host);
}

int vsom_bmu_restricted_batch(vsom_ctx *c, uint64_t min_hits, uint64_t *idx_out_host, float *dist_out_host)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_bmu_restricted_batch");
    CHECK_ROWS(c);
    if (c->B == 0)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    int rc = launch_bmu_restricted(c, min_hits);
    if (rc)
        return rc;
    return copy_search_results(c, idx_out_host, dist_out_host);
}

int vsom_bmd_batch(vsom_ctx *c, uint64_t min_hits, size_t r0, size_t r1, const double *u_host, uint64_t *draw_out,
                   double *norm_out, double *prob_out)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_bmd_batch");
    CHECK_ROWS(c);
    if (c->B == 0)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    if (r0 > r1 || r1 > c->B)
        return vsom_fail(VSOM_ERR_INVALID, "row range out of bounds");
    if (draw_out && !u_host)
        return vsom_fail(VSOM_ERR_INVALID, "draws need one uniform per row");
    for (size_t i = 0; u_host && i < r1 - r0; ++i)
        if (!(u_host[i] >= 0.0 && u_host[i] < 1.0))
            return vsom_fail(VSOM_ERR_INVALID, "uniform " + std::to_string(i) + " is not in [0,1)");
    return launch_bmd(c, min_hits, r0, r1, u_host, draw_out, norm_out, prob_out);
}

int vsom_bmu_topk_batch(vsom_ctx *c, uint32_t k, size_t r0, size_t r1, uint64_t *idx_out, float *dist_out)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_bmu_topk_batch");
    CHECK_ROWS(c);
    if (c->B == 0)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    if (r0 > r1 || r1 > c->B)
        return vsom_fail(VSOM_ERR_INVALID, "row range out of bounds");
    if (k == 0 || k > 64 || k > c->N)
        return vsom_fail(VSOM_ERR_INVALID, "k must be in [1, min(64, N)]");
    if (!idx_out)
        return vsom_fail(VSOM_ERR_INVALID, "idx_out is null");
    return launch_topk(c, k, r0, r1, idx_out, dist_out);
}

int vsom_similarity_batch(vsom_ctx *c, uint64_t min_hits, int num_sigmas, int sigma_rule, size_t r0, size_t r1,
                          const uint8_t *valid_host, vsom_similarity_out *out)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_similarity_batch");
    CHECK_ROWS(c);
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "out is null");
    if (c->B == 0)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    if (r0 > r1 || r1 > c->B)
        return vsom_fail(VSOM_ERR_INVALID, "row range out of bounds");
    if (sigma_rule != VSOM_SIGMA_AS_WRITTEN && sigma_rule != VSOM_SIGMA_FLOOR)
        return vsom_fail(VSOM_ERR_INVALID, "unknown sigma_rule");
    return launch_similarity(c, min_hits, num_sigmas, sigma_rule, r0, r1, valid_host, out);
}

int vsom_evaluate_batch(vsom_ctx *c, size_t r0, size_t r1, const float *binary_host, const float *continuous_host,
                        const uint8_t *valid_host, vsom_evaluate_out *out)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_evaluate_batch");
    CHECK_ROWS(c);
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "out is null");
    if (!binary_host || !continuous_host)
        return vsom_fail(VSOM_ERR_INVALID, "binary_host or continuous_host is null");
    if (c->B == 0)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    if (r0 > r1 || r1 > c->B)
        return vsom_fail(VSOM_ERR_INVALID, "row range out of bounds");
    return launch_evaluate(c, r0, r1, binary_host, continuous_host, valid_host, out);
}

int vsom_generate_batch(vsom_ctx *c, uint64_t min_hits, int rule, size_t r0, size_t r1, const double *u_host,
                        const double *l_host, vsom_generate_out *out)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_generate_batch");
    CHECK_ROWS(c);
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "out is null");
    if (!u_host || !l_host)
        return vsom_fail(VSOM_ERR_INVALID, "u_host or l_host is null");
    if (rule != VSOM_GENERATE_AS_WRITTEN && rule != VSOM_GENERATE_PER_ROW)
        return vsom_fail(VSOM_ERR_INVALID, "unknown rule");
    if (c->J == 0 || c->D == 0)
        return vsom_fail(VSOM_ERR_INVALID, "the records have no columns");
    if (c->B == 0)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    if (r0 > r1 || r1 > c->B)
        return vsom_fail(VSOM_ERR_INVALID, "row range out of bounds");
    for (size_t i = 0; i < r1 - r0; ++i)
        if (!(u_host[i] >= 0.0 && u_host[i] < 1.0))
            return vsom_fail(VSOM_ERR_INVALID, "uniform " + std::to_string(i) + " is not in [0,1)");
    return launch_generate(c, min_hits, rule, r0, r1, u_host, l_host, out);
}

// Reads the model state only: a chunk staged ahead does not matter.
int vsom_decode_nodes(vsom_ctx *c, const uint64_t *nodes_host, size_t count, const double *l_host, double *record_out)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_decode_nodes");
    if (!l_host || !record_out)
        return vsom_fail(VSOM_ERR_INVALID, "l_host or record_out is null");
    if (count > 0 && !nodes_host)
        return vsom_fail(VSOM_ERR_INVALID, "nodes_host is null");
    if (c->J == 0 || c->D == 0)
        return vsom_fail(VSOM_ERR_INVALID, "the records have no columns");
    for (size_t i = 0; i < count; ++i)
        if (nodes_host[i] >= c->N)
            return vsom_fail(VSOM_ERR_INVALID, "node " + std::to_string(i) + " is out of range");
    return launch_decode_nodes(c, nodes_host, count, l_host, record_out);
}

int vsom_bmu_masked_batch(vsom_ctx *c, uint64_t min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask,
                          vsom_masked_out *out)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_bmu_masked_batch");
    if (c->transform == VSOM_CLR)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_bmu_masked_batch: CLR contexts are not supported (the residual runs over column pairs)");
    CHECK_ROWS(c);
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "out is null");
    if (!valid_host)
        return vsom_fail(VSOM_ERR_INVALID, "valid_host is null");
    if (c->B == 0)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    if (r0 > r1 || r1 > c->B)
        return vsom_fail(VSOM_ERR_INVALID, "row range out of bounds");
    return launch_masked(c, min_hits, r0, r1, valid_host, one_mask, out);
}

// the gate the masked chunk queries share behind CHECK_CTX (`what`: the entry point's name; has_out: the call takes an
// `out` structure, which must not be null)
static int vsom_masked_score_gate(vsom_ctx *c, const char *what, size_t r0, size_t r1, const void *valid_host, const void *out,
                                  bool has_out = true)
{
    VSOM_CUSTOM_REFUSE(c, what);
    if (c->transform == VSOM_CLR)
        return vsom_fail(VSOM_ERR_INVALID, std::string(what) + ": CLR contexts are not supported (the residual runs over column pairs)");
    CHECK_ROWS(c);
    if (has_out && !out)
        return vsom_fail(VSOM_ERR_INVALID, "out is null");
    if (!valid_host)
        return vsom_fail(VSOM_ERR_INVALID, "valid_host is null");
    if (c->B == 0)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    if (r0 > r1 || r1 > c->B)
        return vsom_fail(VSOM_ERR_INVALID, "row range out of bounds");
    return VSOM_OK;
}

int vsom_similarity_masked_batch(vsom_ctx *c, uint64_t min_hits, int num_sigmas, int sigma_rule, size_t r0, size_t r1,
                                 const uint8_t *valid_host, int one_mask, vsom_similarity_masked_out *out)
{
    CHECK_CTX(c);                // (reads sigmaMap: a pending one is materialised)
    if (int rc = vsom_masked_score_gate(c, "vsom_similarity_masked_batch", r0, r1, valid_host, out))
        return rc;
    if (sigma_rule != VSOM_SIGMA_AS_WRITTEN && sigma_rule != VSOM_SIGMA_FLOOR)
        return vsom_fail(VSOM_ERR_INVALID, "unknown sigma_rule");
    return launch_similarity_masked(c, min_hits, num_sigmas, sigma_rule, r0, r1, valid_host, one_mask, out);
}

int vsom_evaluate_masked_batch(vsom_ctx *c, uint64_t min_hits, size_t r0, size_t r1, const float *binary_host,
                               const float *continuous_host, const uint8_t *valid_host, int one_mask,
                               vsom_evaluate_masked_out *out)
{
    CHECK_CTX(c);                // (reads the map only; the safe default all the same, as vsom_evaluate_batch)
    if (int rc = vsom_masked_score_gate(c, "vsom_evaluate_masked_batch", r0, r1, valid_host, out))
        return rc;
    if (!binary_host || !continuous_host)
        return vsom_fail(VSOM_ERR_INVALID, "binary_host or continuous_host is null");
    return launch_evaluate_masked(c, min_hits, r0, r1, binary_host, continuous_host, valid_host, one_mask, out);
}

// the same gate for the masked distribution and its records, and per_row uniforms per row, each in [0,1)
static int vsom_masked_draw_gate(vsom_ctx *c, const char *what, size_t r0, size_t r1, const void *valid_host, const void *out,
                                 bool has_out, const double *u_host, size_t per_row)
{
    if (int rc = vsom_masked_score_gate(c, what, r0, r1, valid_host, out, has_out))
        return rc;
    for (size_t i = 0; u_host && i < (r1 - r0) * per_row; ++i)
        if (!(u_host[i] >= 0.0 && u_host[i] < 1.0))
            return vsom_fail(VSOM_ERR_INVALID, "uniform " + std::to_string(i) + " is not in [0,1)");
    return VSOM_OK;
}

int vsom_bmd_masked_batch(vsom_ctx *c, uint64_t min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask,
                          const double *u_host, uint64_t *draw_out, double *norm_out, double *prob_out)
{
    CHECK_CTX(c);
    if (draw_out && !u_host)
        return vsom_fail(VSOM_ERR_INVALID, "draws need one uniform per row");
    if (int rc = vsom_masked_draw_gate(c, "vsom_bmd_masked_batch", r0, r1, valid_host, nullptr, false, u_host, 1))
        return rc;
    return launch_bmd(c, min_hits, r0, r1, u_host, draw_out, norm_out, prob_out, valid_host, one_mask);
}

int vsom_generate_masked_batch(vsom_ctx *c, uint64_t min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask,
                               uint32_t draws, int keep_observed, const double *u_host, const double *l_host,
                               vsom_generate_out *out)
{
    CHECK_CTX(c);                // (reads sigmaMap: a pending one is materialised)
    if (!u_host || !l_host)
        return vsom_fail(VSOM_ERR_INVALID, "u_host or l_host is null");
    if (draws == 0 || draws > 65535)
        return vsom_fail(VSOM_ERR_INVALID, "draws must be in [1, 65535]");
    if (int rc = vsom_masked_draw_gate(c, "vsom_generate_masked_batch", r0, r1, valid_host, out, true, u_host, draws))
        return rc;
    return launch_generate_masked(c, min_hits, r0, r1, valid_host, one_mask, draws, keep_observed, u_host, l_host, out);
}

// Reads the map only: a pending sigmaMap stays pending.
int vsom_bmu_topk_masked_batch(vsom_ctx *c, uint32_t k, uint64_t min_hits, size_t r0, size_t r1, const uint8_t *valid_host,
                               int one_mask, vsom_topk_masked_out *out)
{
    CHECK_CTX_KEEP(c);
    if (int rc = vsom_masked_score_gate(c, "vsom_bmu_topk_masked_batch", r0, r1, valid_host, out))
        return rc;
    if (!out->idx)
        return vsom_fail(VSOM_ERR_INVALID, "out->idx is null");
    if (k == 0 || k > 64 || k > c->N)
        return vsom_fail(VSOM_ERR_INVALID, "k must be in [1, min(64, N)]");
    return launch_topk_masked(c, k, min_hits, r0, r1, valid_host, one_mask, out);
}

int vsom_distances_row(vsom_ctx *c, size_t row, float *dist_out_host)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_distances_row");
    CHECK_ROWS(c);
    if (row >= c->B || !dist_out_host)
        return vsom_fail(VSOM_ERR_INVALID, "row out of range or null output");
    vsom_layout lay;
    const auto hd = lay.add<float>(c->N);
    VSOM_ALLOC_CHECK(vsom_arena_ensure(c->q_scratch, lay, c->stream));
    float *dd = lay.at(hd);
    if (int rc = launch_row_dist(c, row, dd))
        return rc;
    VSOM_HIP_CHECK(hipMemcpyAsync(dist_out_host, dd, (size_t)c->N * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_distances_raw(vsom_ctx *c, const uint64_t *nodes_host, const uint64_t *vrows_host, size_t count,
                       int from_map, float *dist_out_host)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_distances_raw");
    if (!from_map)
        CHECK_ROWS(c);
    if (count == 0)
        return VSOM_OK;
    if (!nodes_host || !vrows_host || !dist_out_host)
        return vsom_fail(VSOM_ERR_INVALID, "null argument");
    for (size_t i = 0; i < count; ++i)
        if (nodes_host[i] >= c->N || vrows_host[i] >= (from_map ? (uint64_t)c->N : (uint64_t)c->B))
            return vsom_fail(VSOM_ERR_INVALID, "pair index out of range");
    return pair_query(c, nodes_host, vrows_host, count, from_map != 0, dist_out_host);
}

// Som::updateUMatrix (vsom_umatrix.hip).  No reader of the staged rows is enqueued, so rows_free_valid stays as it is and
// a chunk staged ahead does not matter.
int vsom_umatrix(vsom_ctx *c, double *u_out_host)
{
    CHECK_CTX_NOJOIN(c);
    if (const char *why = vsom_umatrix_refusal(c))
        return vsom_fail(VSOM_ERR_INVALID, why);
    int rc = vsom_join_aux(c);
    if (rc)
        return rc;
    if ((rc = launch_umatrix(c)))
        return rc;
    if (!u_out_host)
        return VSOM_OK;
    VSOM_HIP_CHECK(hipMemcpyAsync(u_out_host, c->umatrix.p, (size_t)c->N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_get_umatrix(vsom_ctx *c, double *u_out_host)
{
    CHECK_CTX_NOJOIN(c);
    if (!u_out_host)
        return vsom_fail(VSOM_ERR_INVALID, "null output");
    if (!c->um_valid)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_get_umatrix: no vsom_umatrix has run on this context");
    VSOM_HIP_CHECK(hipMemcpyAsync(u_out_host, c->umatrix.p, (size_t)c->N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_batch_phase1_async(vsom_ctx *c, size_t s0, size_t s1, int is_first)
{
    CHECK_CTX_KEEP(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_batch_phase1_async");
    CHECK_ROWS(c);
    if (s0 > s1 || s1 > c->B)
        return vsom_fail(VSOM_ERR_INVALID, "sample range out of bounds");
    return is_first ? launch_bmu_full(c, s0, s1) : launch_bmu_local(c, s0, s1);
}

int vsom_batch_finish_async(vsom_ctx *c)
{
    CHECK_CTX_KEEP(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_batch_finish_async");
    if (!c->chunk_loaded)   // an EMPTY chunk is legal: the reference's epoch then zeroes the map
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    return launch_finish(c);
}

int vsom_batch_phase2_async(vsom_ctx *c, double sigma, size_t n0, size_t n1)
{
    CHECK_CTX_NOJOIN(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_batch_phase2_async");
    // (a further node range of the same epoch works on the transposed chunk it already has -- unless its plan takes a
    // path that reads the staged rows themselves: a range small enough for the small-map chain kernel)
    if (!c->xq_valid || (n1 > n0 && vsom_phase2_plan(*c, n0, n1, true).reads_staged_rows))
        CHECK_ROWS(c);
    if (n0 > n1 || n1 > c->N)
        return vsom_fail(VSOM_ERR_INVALID, "node range out of bounds");
    if (!c->chunk_loaded)   // an EMPTY chunk is legal: the reference's epoch then zeroes the map
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    return launch_phase2(c, sigma, n0, n1, true);
}

int vsom_batch_epoch_async(vsom_ctx *c, double sigma, int is_first)
{
    CHECK_CTX_KEEP(c);
    if (c->cu)
        return vsom_custom_batch_epoch_async(c, sigma, is_first);
    CHECK_ROWS(c);
    if (!c->chunk_loaded)   // an EMPTY chunk is legal: the reference's epoch then zeroes the map
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    if (vsom_tiny_applies(c)) {
        vsom_sigma_drop(c);                             // (every sigmaMap row is rewritten)
        return launch_tiny_epoch(c, sigma, is_first);   // tiny map: the whole epoch in one launch
    }
    int rc = vsom_batch_phase1_async(c, 0, c->B, is_first);
    if (rc)
        return rc;
    if ((rc = launch_finish(c)))
        return rc;
    return launch_phase2(c, sigma, 0, c->N, true);
}

int vsom_get_mse(vsom_ctx *c, float *mse_out)
{
    CHECK_CTX_KEEP(c);
    if (!mse_out)
        return vsom_fail(VSOM_ERR_INVALID, "null output");
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    *mse_out = *static_cast<volatile float *>(c->mse.p);     // pinned host memory: the kernels' store lands here (22 -> 2 us a call)
    return VSOM_OK;
}

int vsom_batch_epoch(vsom_ctx *c, double sigma, int is_first, float *mse_out)
{
    int rc = vsom_batch_epoch_async(c, sigma, is_first);
    if (rc)
        return rc;
    if (mse_out)
        return vsom_get_mse(c, mse_out);
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_batch_epoch_masked(vsom_ctx *c, double sigma, int is_first, const uint8_t *valid_host, int one_mask, float *mse_out)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_batch_epoch_masked");
    if (c->transform == VSOM_CLR)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_epoch_masked: CLR contexts are not supported (residual and step run over column pairs)");
    CHECK_ROWS(c);
    if (!valid_host)
        return vsom_fail(VSOM_ERR_INVALID, "valid_host is null");
    if (!mse_out)
        return vsom_fail(VSOM_ERR_INVALID, "mse_out is null");
    if (!c->chunk_loaded)   // an EMPTY chunk is legal, as for vsom_batch_epoch
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    if (c->update_mode != VSOM_UPDATE_STRICT)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_epoch_masked: the masked chains exist in the strict update mode only");
    if (int rc = launch_batch_epoch_masked(c, sigma, is_first, valid_host, one_mask))
        return rc;
    return vsom_get_mse(c, mse_out);
}

// ---- the accumulated epoch (vsom_accum.hip): ordinary entry points, a pending sigmaMap is materialised by the first ----

int vsom_batch_accum_begin(vsom_ctx *c, double sigma, int is_first, size_t total_rows)
{
    CHECK_CTX(c);
    VSOM_CUSTOM_REFUSE(c, "vsom_batch_accum_begin");
    if (c->transform == VSOM_CLR)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_accum_begin: CLR contexts are not supported (the chains run over column pairs)");
    if (c->update_mode != VSOM_UPDATE_STRICT)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_accum_begin: the carried chains exist in the strict update mode only");
    if (c->in_group || c->sigma_shared)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_accum_begin: the context has joined a group or an ensemble");
    if (c->ac.open)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_accum_begin: an accumulated epoch is already open");
    if (total_rows > 0x7FFFFFFFull)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_accum_begin: total_rows too large");
    if (int rc = launch_accum_begin(c))
        return rc;
    c->ac.open = true;
    c->ac.sigma = sigma;
    c->ac.is_first = is_first;
    c->ac.total = total_rows;
    c->ac.rows = 0;
    return VSOM_OK;
}

// valid_host null: the plain call
static int accum_chunk(vsom_ctx *c, const char *name, const uint8_t *valid_host, int one_mask)
{
    const std::string who(name);
    if (!c->ac.open)
        return vsom_fail(VSOM_ERR_INVALID, who + ": no accumulated epoch is open");
    CHECK_ROWS(c);
    if (!c->chunk_loaded)   // an EMPTY chunk is legal and changes nothing
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    if (c->ac.rows + c->B > c->ac.total)
        return vsom_fail(VSOM_ERR_INVALID, who + ": the chunk's " + std::to_string(c->B) + " rows exceed total_rows (" +
                                               std::to_string(c->ac.rows) + " of " + std::to_string(c->ac.total) + " accumulated)");
    if (c->B == 0)
        return VSOM_OK;
    if (int rc = launch_accum_chunk(c, valid_host, one_mask))
        return rc;
    c->ac.rows += c->B;
    return VSOM_OK;
}

int vsom_batch_accum_chunk(vsom_ctx *c)
{
    CHECK_CTX(c);
    return accum_chunk(c, "vsom_batch_accum_chunk", nullptr, 0);
}

int vsom_batch_accum_chunk_masked(vsom_ctx *c, const uint8_t *valid_host, int one_mask)
{
    CHECK_CTX(c);
    if (!valid_host)
        return vsom_fail(VSOM_ERR_INVALID, "valid_host is null");
    return accum_chunk(c, "vsom_batch_accum_chunk_masked", valid_host, one_mask);
}

int vsom_batch_accum_end(vsom_ctx *c, float *mse_out)
{
    CHECK_CTX(c);
    if (!c->ac.open)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_accum_end: no accumulated epoch is open");
    if (c->ac.rows != c->ac.total)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_accum_end: " + std::to_string(c->ac.rows) + " of total_rows = " +
                                               std::to_string(c->ac.total) + " rows accumulated (the epoch stays open)");
    if (int rc = launch_accum_end(c))
        return rc;
    c->ac.open = false;
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (mse_out)
        *mse_out = *static_cast<volatile float *>(c->mse.p);
    return VSOM_OK;
}

int vsom_batch_accum_abort(vsom_ctx *c)
{
    CHECK_CTX(c);
    if (!c->ac.open)
        return vsom_fail(VSOM_ERR_INVALID, "vsom_batch_accum_abort: no accumulated epoch is open");
    c->ac.open = false;     // (chunks still running write the accumulators only)
    return VSOM_OK;
}

void *vsom_device_ptr(vsom_ctx *c, int which)
{
    if (!c)
        return nullptr;
    switch (which) {
    case VSOM_BUF_MAP: return c->map.p;
    case VSOM_BUF_SIGMA:
        // the caller is about to read it: current as of this call; a pointer kept across later epochs is current again
        // after vsom_sigma_flush (include/vsom_hip.h)
        if (hipSetDevice(c->device) != hipSuccess || vsom_sigma_flush_pending(c) != VSOM_OK)
            return nullptr;
        return c->sigma.p;
    case VSOM_BUF_S: return c->S.p;
    case VSOM_BUF_WEIGHT: return c->weight.p;
    case VSOM_BUF_HITS: return c->hits.p;
    case VSOM_BUF_LASTBMU: return c->lastbmu.p;
    case VSOM_BUF_SQRES: return c->sqres.p;
    case VSOM_BUF_CHUNK: return c->Xs.p;
    case VSOM_BUF_UMATRIX: return c->um_valid ? c->umatrix.p : nullptr;
    default: return nullptr;
    }
}

uint32_t vsom_pitch(const vsom_ctx *c) { return c ? c->pitch : 0; }
uint32_t vsom_chunk_pitch(const vsom_ctx *c) { return c ? c->xpitch : 0; }

int vsom_enable_timing(vsom_ctx *c, int on)
{
    if (!c)
        return vsom_fail(VSOM_ERR_INVALID, "null context");
    c->timing = on ? ~0u : 0u;
    return VSOM_OK;
}

int vsom_enable_timing_of(vsom_ctx *c, uint32_t group_mask)
{
    if (!c)
        return vsom_fail(VSOM_ERR_INVALID, "null context");
    c->timing = group_mask;
    return VSOM_OK;
}

int vsom_get_timing(vsom_ctx *c, float *ms_out, uint32_t *count_out, int reset)
{
    CHECK_CTX_KEEP(c);
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (auto &e : c->ev_live) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            c->t_ms[e.which] += ms;
            c->t_cnt[e.which] += 1;
        }
        c->ev_pool.push_back(e);
    }
    c->ev_live.clear();
    for (int i = 0; i < VSOM_T_COUNT; ++i) {
        if (ms_out)
            ms_out[i] = c->t_ms[i];
        if (count_out)
            count_out[i] = c->t_cnt[i];
        if (reset) {
            c->t_ms[i] = 0.f;
            c->t_cnt[i] = 0;
        }
    }
    return VSOM_OK;
}

}   // extern "C"
