// vsom_custom.hip -- contexts of a caller-defined Transformation (vsom_create_custom): the caller's Comparer / Stepper
// arrive as device source, are compiled with hipRTC together with the generic kernels of vsom_custom_kernels.inc and
// run from the module loaded into the context.  The arithmetic is host/src/vsom_custom.cpp's, operation for operation.
//
// A custom context is an ordinary vsom_ctx (state, chunk rows, lastBMU, the pinned MSE word, the stream) whose
// model rows are unpadded (pitch = D) and whose chunk rows are unpadded (xpitch = J); `cu` holds the rest.  The
// entry points that accept a custom context route here from vsom_capi.hip / vsom_online.hip / vsom_single.hip; all others refuse it.
#include "vsom_internal.hpp"

#include <hip/hiprtc.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace {

const char *const kKernelText =
#include "vsom_custom_kernels.inc"
    ;

// (hipRTC compiles without the HIP headers: the few types the contract names are declared here)
const char *const kPrelude =
    "typedef unsigned int uint32_t;\n"
    "typedef unsigned long long uint64_t;\n"
    "#line 1 \"hook_source\"\n";

// hook source + generic kernels -> gfx950 code object; false with the hipRTC log in *log on failure
bool compile_hooks(const char *hook_source, std::vector<char> &code, std::string &log)
{
    const std::string src = std::string(kPrelude) + hook_source + "\n#line 1 \"vsom_custom_kernels\"\n" + kKernelText;
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "vsom_custom.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        log = "hiprtcCreateProgram failed";
        return false;
    }
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                          "-fhip-fp32-correctly-rounded-divide-sqrt"};
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)(sizeof(opts) / sizeof(opts[0])), opts);
    size_t n = 0;
    if (hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) {
        std::vector<char> buf(n + 1, 0);
        if (hiprtcGetProgramLog(prog, buf.data()) == HIPRTC_SUCCESS) {
            buf[n] = 0;
            log.assign(buf.data());
        }
    }
    bool ok = rc == HIPRTC_SUCCESS;
    if (ok) {
        size_t sz = 0;
        ok = hiprtcGetCodeSize(prog, &sz) == HIPRTC_SUCCESS && sz > 0;
        if (ok) {
            code.resize(sz);
            ok = hiprtcGetCode(prog, code.data()) == HIPRTC_SUCCESS;
        }
    }
    if (!ok && log.empty())
        log = hiprtcGetErrorString(rc);
    (void)hiprtcDestroyProgram(&prog);
    return ok;
}

int check_shape(uint32_t depth, uint32_t residual_len, const char *hook_source)
{
    if (!hook_source || !*hook_source)
        return vsom_fail(VSOM_ERR_INVALID, "hook_source is empty");
    if (depth == 0 || residual_len == 0)
        return vsom_fail(VSOM_ERR_INVALID, "depth and residual_len must be > 0");
    if (depth > VSOM_CUSTOM_MAX_DEPTH)
        return vsom_fail(VSOM_ERR_INVALID, "depth " + std::to_string(depth) + " exceeds VSOM_CUSTOM_MAX_DEPTH (" +
                                               std::to_string(VSOM_CUSTOM_MAX_DEPTH) + "): the phase-2 model does not fit in LDS");
    return VSOM_OK;
}

}   // namespace

struct vsom_custom_state {
    uint32_t R = 0;
    hipModule_t mod = nullptr;
    hipFunction_t k_floor = nullptr, k_expand = nullptr, k_full = nullptr, k_local = nullptr, k_pair = nullptr,
                  k_resid = nullptr, k_finish = nullptr, k_phase2 = nullptr, k_onl_update = nullptr, k_onl_post = nullptr;
    DevBuf<float> sigf;           // [N][D] select(sigma < 1e-5, 1e-5, sigma): the dispersion the distance passes
    DevBuf<float> ones;           // [J] the value weights while neither validity nor column weights are set: all 1
    // value_weight (vsom_set_chunk_validity, vsom_set_column_weights): expanded once per setter call by vc_expand_validity,
    // read by every launch.  mask: 0 = the chunk is all valid, 1 = one [J] mask for every row, 2 = [B][J].
    int mask = 0;
    bool weighted = false;
    DevBuf<unsigned char> vbytes; // the current chunk's validity bytes as given ([J] or [B][J]; kept for a change of the weights)
    DevBuf<float> wts;            // [J] the column weights
    DevBuf<float> cvalid, cvw;    // [J] or [B][J]: valid as 0 / 1, valid * weights
    DevBuf<unsigned char> vec_bytes; DevBuf<float> vec_valid, vec_vw;   // [J] the same for one host vector (the _valid calls)
    DevBuf<float> vec;            // [J] one host vector (find / dist / train_single)
    DevBuf<float> resid;          // [R] train_single's residual
    DevBuf<u64> slot;             // [2] one BMU index
    DevBuf<float> fout;           // [2] one distance
    DevBuf<u64> pairs; DevBuf<float> pair_out;    // [2][count] node / row pairs, [count] distances
    DevBuf<double> lutd; double lutd_sigma = -1.0;   // [H][W] calculateNeighbourhoodWeight(dx, dy, 0, 0, sigma)
    std::vector<float> next; size_t next_B = 0; bool next_pending = false;   // vsom_prefetch_chunk's rows until the commit
};

namespace {

// the value_weight rows of a launch: row s is p + s * stride (stride 0: one [J] vector for every row)
struct VwRef {
    const float *p;
    u64 stride;
};

int launch(vsom_ctx *c, hipFunction_t f, unsigned grid, unsigned block, unsigned lds, std::vector<void *> args)
{
    if (grid == 0)
        return VSOM_OK;
    VSOM_HIP_CHECK(hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, lds, c->stream, args.data(), nullptr));
    return VSOM_OK;
}

int refresh_sigf(vsom_ctx *c)
{
    vsom_custom_state *u = c->cu;
    u64 n = (u64)c->N * c->D;
    const float *sg = c->sigma.p;
    return launch(c, u->k_floor, (unsigned)((n + 255) / 256), 256, 0, {&sg, &u->sigf.p, &n});
}

// valid .* weights of the chunk rows (Som.cpp:134, :905): `ones` while nothing is set -- the launches of an untouched
// context -- and the weights themselves while every entry is valid (1.0f * w is w)
VwRef chunk_vw(const vsom_ctx *c)
{
    const vsom_custom_state *u = c->cu;
    if (!u->mask)
        return {u->weighted ? u->wts.p : u->ones.p, 0};
    return {u->cvw.p, u->mask == 2 ? (u64)c->J : 0};
}

// valid alone (the batch residual and phase 2, Som.cpp:780,:803,:861,:867)
VwRef chunk_valid(const vsom_ctx *c)
{
    const vsom_custom_state *u = c->cu;
    if (!u->mask)
        return {u->ones.p, 0};
    return {u->cvalid.p, u->mask == 2 ? (u64)c->J : 0};
}

int expand_validity(vsom_ctx *c, const unsigned char *bytes, float *valid, float *vw, u64 rows)
{
    vsom_custom_state *u = c->cu;
    const float *w = u->weighted ? u->wts.p : nullptr;
    u64 n = rows * c->J;
    uint32_t J = c->J;
    return launch(c, u->k_expand, (unsigned)((n + 255) / 256), 256, 0, {&bytes, &w, &valid, &vw, &n, &J});
}

// cvalid / cvw of the current chunk from vbytes and wts, after either changed (nothing to do while the chunk is all valid).
// A failed allocation leaves the chunk all valid: the set is absent then.
int refresh_chunk_vw(vsom_ctx *c)
{
    vsom_custom_state *u = c->cu;
    if (!u->mask)
        return VSOM_OK;
    const size_t rows = u->mask == 2 ? c->B : 1, cap = (u->mask == 2 ? c->Bcap : 1) * (size_t)c->J;
    if (vsom_grow_set(c->stream, VSOM_BUF_SYNC, {vsom_member(u->cvalid, cap), vsom_member(u->cvw, cap)}) != hipSuccess) {
        (void)hipGetLastError();
        u->mask = 0;
        return vsom_fail(VSOM_ERR_NOMEM, "hipMalloc of the chunk's value weights failed");
    }
    return expand_validity(c, u->vbytes.p, u->cvalid.p, u->cvw.p, rows);
}

// the one value_weight vector of a host vector: valid_host (null: all valid) .* the column weights
int vector_vw(vsom_ctx *c, const uint8_t *valid_host, VwRef *out)
{
    vsom_custom_state *u = c->cu;
    if (!valid_host) {
        *out = {u->weighted ? u->wts.p : u->ones.p, 0};
        return VSOM_OK;
    }
    VSOM_HIP_CHECK(hipMemcpyAsync(u->vec_bytes.p, valid_host, c->J, hipMemcpyHostToDevice, c->stream));
    *out = {u->vec_vw.p, 0};
    return expand_validity(c, u->vec_bytes.p, u->vec_valid.p, u->vec_vw.p, 1);
}

int ensure_chunk(vsom_ctx *c, size_t B)
{
    if (B <= c->Bcap)
        return VSOM_OK;
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->Bcap = 0;
    c->B = 0;
    c->chunk_loaded = false;
    const size_t cap = (B + 63) / 64 * 64;
    VSOM_ALLOC_CHECK(vsom_grow_set(c->stream, VSOM_BUF_REBUILD, {vsom_member(c->Xs, cap * c->J), vsom_member(c->lastbmu, cap),
                                                               vsom_member(c->sqres, cap)}));
    c->Bcap = cap;
    return VSOM_OK;
}

int stage_vec(vsom_ctx *c, const float *v_host)
{
    if (!v_host)
        return vsom_fail(VSOM_ERR_INVALID, "null vector");
    VSOM_HIP_CHECK(hipMemcpyAsync(c->cu->vec.p, v_host, (size_t)c->J * 4, hipMemcpyHostToDevice, c->stream));
    return VSOM_OK;
}

// full search of `rows` sample rows starting at X
int search_full(vsom_ctx *c, const float *X, VwRef vw, unsigned rows, u64 *bmu, float *dist)
{
    vsom_custom_state *u = c->cu;
    u64 xs = c->J;
    uint32_t N = c->N, J = c->J, D = c->D, R = u->R;
    return launch(c, u->k_full, rows, 256, 0,
                  {&X, &xs, &c->map.p, &u->sigf.p, &vw.p, &vw.stride, &N, &J, &D, &R, &bmu, &dist});
}

int search_local(vsom_ctx *c, const float *X, VwRef vw, uint32_t rows, const u64 *start, u64 *bmu, float *dist)
{
    vsom_custom_state *u = c->cu;
    u64 xs = c->J;
    uint32_t W = c->W, H = c->H, J = c->J, D = c->D, R = u->R;
    return launch(c, u->k_local, (rows + 63) / 64, 64, 0,
                  {&X, &xs, &c->map.p, &u->sigf.p, &vw.p, &vw.stride, &W, &H, &J, &D, &R, &start, &bmu, &dist, &rows});
}

int ensure_lutd(vsom_ctx *c, double sigma)
{
    vsom_custom_state *u = c->cu;
    if (u->lutd_sigma == sigma)
        return VSOM_OK;
    std::vector<double> host((size_t)c->W * c->H);
    for (uint32_t dy = 0; dy < c->H; ++dy)
        for (uint32_t dx = 0; dx < c->W; ++dx)
            host[(size_t)dy * c->W + dx] = vsom_neighbourhood_weight(dx, dy, 0, 0, sigma);
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));    // its previous contents may still be read
    VSOM_HIP_CHECK(hipMemcpy(u->lutd.p, host.data(), host.size() * 8, hipMemcpyHostToDevice));
    u->lutd_sigma = sigma;
    return VSOM_OK;
}

// one trainSingle step of the sample at device address x (hostTrainSingle): search, window update, residual / distance;
// bmu is the sample's lastBMU slot (in / out); every hook call takes row `row` of vw (Som.cpp:891,:905-946)
int online_step(vsom_ctx *c, const float *x, VwRef vw, u64 row, double eta, double sigma, int decay_fn, u64 *bmu, float *resid,
                float *dist, u64 *hits, float *mse, uint32_t B)
{
    vsom_custom_state *u = c->cu;
    const VwRef mine{vw.p + row * vw.stride, 0};
    int rc = sigma > 1.0 ? search_full(c, x, mine, 1, bmu, u->fout.p) : search_local(c, x, mine, 1, bmu, bmu, u->fout.p);
    if (rc)
        return rc;
    // a box of nx x ny workgroups covers the window: x1 - x0 <= floor(5 sigma) + 1
    const double ext = std::floor(5.0 * sigma) + 2.0;
    uint32_t nx = ext >= c->W ? c->W : (uint32_t)ext, ny = ext >= c->H ? c->H : (uint32_t)ext;
    uint32_t W = c->W, H = c->H, J = c->J, D = c->D, R = u->R;
    if ((rc = launch(c, u->k_onl_update, nx * ny, 256, 2 * D * 4,
                     {&x, &c->map.p, &c->S.p, &c->sigma.p, &u->sigf.p, &c->weight.p, &bmu, &u->lutd.p, &W, &H, &vw.p, &vw.stride,
                      &row, &J, &D, &eta, &sigma, &decay_fn, &nx})))
        return rc;
    return launch(c, u->k_onl_post, 1, 64, 0,
                  {&x, &c->map.p, &c->sigma.p, &u->sigf.p, &vw.p, &vw.stride, &row, &J, &D, &R, &bmu, &resid, &dist, &hits, &mse,
                   &B});
}

void free_custom(vsom_custom_state *u)
{
    if (u->mod)
        (void)hipModuleUnload(u->mod);
    delete u;
}

}   // namespace

void vsom_custom_destroy(vsom_ctx *c)
{
    if (c->cu)
        free_custom(c->cu);
    c->cu = nullptr;
}

uint32_t vsom_custom_residual_len(const vsom_ctx *c) { return c->cu->R; }

int vsom_custom_refuse(const char *what)
{
    return vsom_fail(VSOM_ERR_INVALID, std::string(what) + " is not available on a custom-transformation context");
}

int vsom_custom_only(const char *what)
{
    return vsom_fail(VSOM_ERR_INVALID, std::string(what) + " needs a custom-transformation context: the built-in Comparer / "
                                       "Stepper ignore valueWeight; for missing values on a built-in context use the masked "
                                       "calls (vsom_bmu_masked_batch, vsom_batch_epoch_masked, vsom_train_online_chunk_masked)");
}

int vsom_custom_after_set_state(vsom_ctx *c)
{
    int rc = refresh_sigf(c);
    if (rc)
        return rc;
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_custom_upload(vsom_ctx *c, const float *x_host, size_t B, bool wait)
{
    if (B > 0 && !x_host)
        return vsom_fail(VSOM_ERR_INVALID, "x_host is null");
    if (B > 0x7FFFFFFFull)
        return vsom_fail(VSOM_ERR_INVALID, "chunk too large");
    int rc = ensure_chunk(c, B);
    if (rc)
        return rc;
    if (B) {
        VSOM_HIP_CHECK(hipMemcpyAsync(c->Xs.p, x_host, B * c->J * 4, hipMemcpyHostToDevice, c->stream));
        VSOM_HIP_CHECK(hipMemsetAsync(c->lastbmu.p, 0, B * 8, c->stream));     // DataSet.cpp:136-137
        VSOM_HIP_CHECK(hipMemsetAsync(c->sqres.p, 0, B * 4, c->stream));
    }
    c->B = B;
    c->chunk_loaded = true;
    c->cu->mask = 0;                // a new chunk is all valid; the column weights stay
    if (wait)
        VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

// Som.cpp's valueWeight on the device: the column weights of the context (DataSet::getWeights) ...
int vsom_custom_set_weights(vsom_ctx *c, const float *weights_host)
{
    vsom_custom_state *u = c->cu;
    u->weighted = weights_host != nullptr;
    if (weights_host)
        VSOM_HIP_CHECK(hipMemcpyAsync(u->wts.p, weights_host, (size_t)c->J * 4, hipMemcpyHostToDevice, c->stream));
    if (int rc = refresh_chunk_vw(c))
        return rc;
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));    // weights_host is the caller's again
    return VSOM_OK;
}

// ... and the validity of the loaded chunk (DataSet::getValidity); the bytes go up from the caller's memory as they are
int vsom_custom_set_validity(vsom_ctx *c, const uint8_t *valid_host, int one_mask)
{
    vsom_custom_state *u = c->cu;
    if (!c->chunk_loaded)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    CHECK_ROWS(c);
    const size_t n = (one_mask ? 1 : c->B) * (size_t)c->J;
    const int mask = !valid_host || n == 0 ? 0 : one_mask ? 1 : 2;
    if (mask) {
        u->mask = 0;                // (until the bytes are up: a failure below leaves the chunk all valid)
        VSOM_ALLOC_CHECK(vsom_grow(u->vbytes, (one_mask ? 1 : c->Bcap) * (size_t)c->J, c->stream, VSOM_BUF_SYNC));
        VSOM_HIP_CHECK(hipMemcpyAsync(u->vbytes.p, valid_host, n, hipMemcpyHostToDevice, c->stream));
    }
    u->mask = mask;
    if (int rc = refresh_chunk_vw(c))
        return rc;
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));    // valid_host is the caller's again
    return VSOM_OK;
}

// double-buffered ingest on a custom context: the prefetch keeps a host copy of the rows, the commit uploads it
int vsom_custom_prefetch(vsom_ctx *c, const float *x_host, size_t B)
{
    if (B > 0 && !x_host)
        return vsom_fail(VSOM_ERR_INVALID, "x_host is null");
    vsom_custom_state *u = c->cu;
    u->next.assign(x_host, x_host + B * c->J);
    u->next_B = B;
    u->next_pending = true;
    return VSOM_OK;
}

int vsom_custom_commit(vsom_ctx *c)
{
    vsom_custom_state *u = c->cu;
    if (!u->next_pending)
        return vsom_fail(VSOM_ERR_INVALID, "no prefetched chunk to commit");
    u->next_pending = false;
    return vsom_custom_upload(c, u->next.data(), u->next_B, true);
}

static int copy_results(vsom_ctx *c, uint64_t *idx, float *dist)
{
    if (idx && c->B)
        VSOM_HIP_CHECK(hipMemcpyAsync(idx, c->lastbmu.p, c->B * 8, hipMemcpyDeviceToHost, c->stream));
    if (dist && c->B)
        VSOM_HIP_CHECK(hipMemcpyAsync(dist, c->sqres.p, c->B * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_custom_bmu_batch(vsom_ctx *c, int local, uint64_t *idx_out_host, float *dist_out_host)
{
    const VwRef vw = chunk_vw(c);
    int rc = local ? search_local(c, c->Xs.p, vw, (uint32_t)c->B, c->lastbmu.p, c->lastbmu.p, c->sqres.p)
                   : search_full(c, c->Xs.p, vw, (unsigned)c->B, c->lastbmu.p, c->sqres.p);
    if (rc)
        return rc;
    return copy_results(c, idx_out_host, dist_out_host);
}

int vsom_custom_find(vsom_ctx *c, const float *v_host, const uint8_t *valid_host, int local, uint64_t start, uint64_t *bmu_out,
                     float *dist_out)
{
    vsom_custom_state *u = c->cu;
    if (local && start >= c->N)
        return vsom_fail(VSOM_ERR_INVALID, "lastBMU out of range");
    VwRef vw;
    int rc = stage_vec(c, v_host);
    if (rc || (rc = vector_vw(c, valid_host, &vw)))
        return rc;
    u64 s = start;
    VSOM_HIP_CHECK(hipMemcpyAsync(u->slot.p, &s, 8, hipMemcpyHostToDevice, c->stream));
    rc = local ? search_local(c, u->vec.p, vw, 1, u->slot.p, u->slot.p, u->fout.p)
               : search_full(c, u->vec.p, vw, 1, u->slot.p, u->fout.p);
    if (rc)
        return rc;
    float d = 0.f;
    VSOM_HIP_CHECK(hipMemcpyAsync(&s, u->slot.p, 8, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipMemcpyAsync(&d, u->fout.p, 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (bmu_out)
        *bmu_out = s;
    if (dist_out)
        *dist_out = d;
    return VSOM_OK;
}

static int pair_dist(vsom_ctx *c, const float *X, VwRef vw, const uint64_t *nodes_host, const uint64_t *rows_host, size_t count,
                     float *out_host)
{
    vsom_custom_state *u = c->cu;
    VSOM_ALLOC_CHECK(vsom_grow_set(c->stream, VSOM_BUF_SYNC, {vsom_member(u->pairs, 2 * count), vsom_member(u->pair_out, count)}));
    u64 *dn = u->pairs.p, *dr = u->pairs.p + count;
    VSOM_HIP_CHECK(hipMemcpyAsync(dn, nodes_host, count * 8, hipMemcpyHostToDevice, c->stream));
    VSOM_HIP_CHECK(hipMemcpyAsync(dr, rows_host, count * 8, hipMemcpyHostToDevice, c->stream));
    u64 xs = c->J, cnt = count;
    uint32_t J = c->J, D = c->D, R = u->R;
    int rc = launch(c, u->k_pair, (unsigned)((count + 63) / 64), 64, 0,
                    {&X, &xs, &c->map.p, &u->sigf.p, &vw.p, &vw.stride, &J, &D, &R, &dn, &dr, &cnt, &u->pair_out.p});
    if (rc)
        return rc;
    VSOM_HIP_CHECK(hipMemcpyAsync(out_host, u->pair_out.p, count * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VSOM_OK;
}

int vsom_custom_dist_single(vsom_ctx *c, const float *v_host, const uint8_t *valid_host, uint64_t node, float *dist_out)
{
    if (node >= c->N || !dist_out)
        return vsom_fail(VSOM_ERR_INVALID, "node out of range or null output");
    VwRef vw;
    int rc = stage_vec(c, v_host);
    if (rc || (rc = vector_vw(c, valid_host, &vw)))
        return rc;
    const uint64_t row = 0;
    return pair_dist(c, c->cu->vec.p, vw, &node, &row, 1, dist_out);
}

int vsom_custom_distances(vsom_ctx *c, const uint64_t *nodes_host, const uint64_t *rows_host, size_t count,
                          float *dist_out_host)
{
    if (count == 0)
        return VSOM_OK;
    if (!nodes_host || !rows_host || !dist_out_host)
        return vsom_fail(VSOM_ERR_INVALID, "null argument");
    if (count > 0x0FFFFFFFull)
        return vsom_fail(VSOM_ERR_INVALID, "too many pairs");
    for (size_t i = 0; i < count; ++i)
        if (nodes_host[i] >= c->N || rows_host[i] >= c->B)
            return vsom_fail(VSOM_ERR_INVALID, "pair index out of range");
    return pair_dist(c, c->Xs.p, chunk_vw(c), nodes_host, rows_host, count, dist_out_host);
}

// Som::trainBatchSomEpoch (hostBatchEpoch): phase 1 search + residual, bmuHits / MSE, phase 2 per node
int vsom_custom_batch_epoch_async(vsom_ctx *c, double sigma, int is_first)
{
    if (!c->chunk_loaded)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    vsom_custom_state *u = c->cu;
    uint32_t B = (uint32_t)c->B, W = c->W, H = c->H, J = c->J, D = c->D, R = u->R;
    VwRef vw = chunk_vw(c), valid = chunk_valid(c);    // search: valid .* weights; residual and phase 2: valid alone
    int rc = is_first ? search_full(c, c->Xs.p, vw, B, c->lastbmu.p, c->sqres.p)
                      : search_local(c, c->Xs.p, vw, B, c->lastbmu.p, c->lastbmu.p, c->sqres.p);
    if (rc)
        return rc;
    u64 xs = c->J;
    if ((rc = launch(c, u->k_resid, (B + 63) / 64, 64, 0,
                     {&c->Xs.p, &xs, &c->map.p, &c->S.p, &valid.p, &valid.stride, &J, &D, &R, &c->lastbmu.p, &c->sqres.p, &B})))
        return rc;
    float *mse = c->mse.p;
    if ((rc = launch(c, u->k_finish, 1, 64, 0, {&c->lastbmu.p, &c->sqres.p, &B, &c->hits.p, &mse})))
        return rc;
    if ((rc = ensure_lut(c, sigma)))
        return rc;
    uint32_t lutw = c->lut_w;
    return launch(c, u->k_phase2, c->N, 256, 3 * D * 4,
                  {&c->Xs.p, &xs, &c->map.p, &c->sigma.p, &u->sigf.p, &c->weight.p, &c->lastbmu.p, &c->lut.p, &lutw, &W, &H, &B,
                   &valid.p, &valid.stride, &J, &D});
}

// Som::trainSingle (hostTrainSingle) on one host vector
int vsom_custom_train_single(vsom_ctx *c, const float *v_host, const uint8_t *valid_host, double eta, double sigma,
                             uint64_t *last_bmu, int decay_fn, float *residual_out, float *dist_out, uint64_t *bmu_out)
{
    vsom_custom_state *u = c->cu;
    if (!v_host || !last_bmu)
        return vsom_fail(VSOM_ERR_INVALID, "null argument");
    if (decay_fn != VSOM_EXPONENTIAL && decay_fn != VSOM_INVERSE_PROPORTIONAL)
        return vsom_fail(VSOM_ERR_INVALID, "online training needs Exponential or InverseProportional");
    if (*last_bmu >= c->N)
        return vsom_fail(VSOM_ERR_INVALID, "lastBMU out of range");
    VwRef vw;
    int rc = stage_vec(c, v_host);
    if (rc || (rc = vector_vw(c, valid_host, &vw)) || (rc = ensure_lutd(c, sigma)))
        return rc;
    u64 s = *last_bmu;
    VSOM_HIP_CHECK(hipMemcpyAsync(u->slot.p, &s, 8, hipMemcpyHostToDevice, c->stream));
    if ((rc = online_step(c, u->vec.p, vw, 0, eta, sigma, decay_fn, u->slot.p, u->resid.p, u->fout.p + 1, nullptr, nullptr, 1)))
        return rc;
    float d = 0.f;
    VSOM_HIP_CHECK(hipMemcpyAsync(&s, u->slot.p, 8, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipMemcpyAsync(&d, u->fout.p + 1, 4, hipMemcpyDeviceToHost, c->stream));
    if (residual_out)
        VSOM_HIP_CHECK(hipMemcpyAsync(residual_out, u->resid.p, (size_t)u->R * 4, hipMemcpyDeviceToHost, c->stream));
    VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    *last_bmu = s;
    if (bmu_out)
        *bmu_out = s;
    if (dist_out)
        *dist_out = d;
    return VSOM_OK;
}

// the inner loop of Som::trainBasicSom over the staged chunk: one launch sequence per sample, in sample order
int vsom_custom_train_online_chunk(vsom_ctx *c, double eta, double sigma, int decay_fn, int first_chunk)
{
    vsom_custom_state *u = c->cu;
    if (decay_fn != VSOM_EXPONENTIAL && decay_fn != VSOM_INVERSE_PROPORTIONAL)
        return vsom_fail(VSOM_ERR_INVALID, "online training needs Exponential or InverseProportional");
    if (!c->chunk_loaded)
        return vsom_fail(VSOM_ERR_INVALID, "no chunk loaded");
    int rc = ensure_lutd(c, sigma);
    if (rc)
        return rc;
    if (first_chunk) {
        VSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
        *static_cast<volatile float *>(c->mse.p) = 0.f;
    }
    const uint32_t B = (uint32_t)c->B;
    const VwRef vw = chunk_vw(c);
    for (uint32_t s = 0; s < B; ++s)
        if ((rc = online_step(c, c->Xs.p + (size_t)s * c->J, vw, s, eta, sigma, decay_fn, c->lastbmu.p + s, nullptr, u->fout.p + 1,
                              c->hits.p, c->mse.p, B)))
            return rc;
    return VSOM_OK;
}

extern "C" {

int vsom_custom_compile_check(const char *hook_source, uint32_t depth, uint32_t residual_len)
{
    int rc = check_shape(depth, residual_len, hook_source);
    if (rc)
        return rc;
    std::vector<char> code;
    std::string log;
    if (!compile_hooks(hook_source, code, log))
        return vsom_fail(VSOM_ERR_INVALID, "hook source does not compile:\n" + log);
    return VSOM_OK;
}

int vsom_create_custom(vsom_ctx **out, int device, uint32_t width, uint32_t height, uint32_t in_len, uint32_t depth,
                       uint32_t residual_len, const char *hook_source)
{
    if (!out)
        return vsom_fail(VSOM_ERR_INVALID, "out is null");
    *out = nullptr;
    int rc = check_shape(depth, residual_len, hook_source);
    if (rc)
        return rc;
    std::vector<char> code;
    std::string log;
    if (!compile_hooks(hook_source, code, log))
        return vsom_fail(VSOM_ERR_INVALID, "hook source does not compile:\n" + log);
    vsom_ctx *c = nullptr;
    // the context of the built-in Standard transformation carries the state, the stream and the bookkeeping; its
    // rows are then re-laid out unpadded
    if ((rc = vsom_create(&c, device, width, height, in_len, VSOM_STANDARD)))
        return rc;
    auto fail = [&](int code_, const std::string &msg) {
        std::string keep = msg;
        vsom_destroy(c);
        return vsom_fail(code_, keep);
    };
    vsom_custom_state *u = new (std::nothrow) vsom_custom_state();
    if (!u)
        return fail(VSOM_ERR_NOMEM, "out of host memory");
    c->cu = u;
    c->transform = -1;
    u->R = residual_len;
    c->D = depth;
    c->nparts = 1;
    c->part_len = depth;
    c->part_pitch = depth;
    c->pitch = depth;
    c->xpitch = in_len;
    const size_t nd = (size_t)c->N * depth;
    // the model state at this depth replaces the built-in one (zero-filled on the stream: the first use is on it)
    if (vsom_grow_set(c->stream, VSOM_BUF_SYNC | VSOM_BUF_REBUILD,
                      {vsom_member(c->map, nd, VSOM_BUF_ZERO), vsom_member(c->sigma, nd, VSOM_BUF_ZERO),
                       vsom_member(c->S, nd, VSOM_BUF_ZERO), vsom_member(u->sigf, nd), vsom_member(u->ones, in_len),
                       vsom_member(u->vec, in_len), vsom_member(u->resid, residual_len), vsom_member(u->slot, 2),
                       vsom_member(u->fout, 2), vsom_member(u->lutd, (size_t)width * height), vsom_member(u->wts, in_len),
                       vsom_member(u->vec_bytes, in_len), vsom_member(u->vec_valid, in_len),
                       vsom_member(u->vec_vw, in_len)}) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VSOM_ERR_NOMEM, "hipMalloc of the custom context's state failed");
    }
    const std::vector<float> ones(in_len, 1.f);
    if (hipMemcpy(u->ones.p, ones.data(), (size_t)in_len * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(VSOM_ERR_HIP, "initialisation of the custom context failed");
    if (hipModuleLoadData(&u->mod, code.data()) != hipSuccess) {
        (void)hipGetLastError();
        u->mod = nullptr;
        return fail(VSOM_ERR_HIP, "hipModuleLoadData of the hook module failed");
    }
    struct { hipFunction_t *f; const char *name; } fns[] = {
        {&u->k_floor, "vc_floor_sigma"}, {&u->k_expand, "vc_expand_validity"}, {&u->k_full, "vc_search_full"},
        {&u->k_local, "vc_search_local"}, {&u->k_pair, "vc_pair_dist"}, {&u->k_resid, "vc_batch_residual"}, {&u->k_finish, "vc_batch_finish"},
        {&u->k_phase2, "vc_batch_phase2"}, {&u->k_onl_update, "vc_online_update"}, {&u->k_onl_post, "vc_online_post"}};
    for (auto &f : fns)
        if (hipModuleGetFunction(f.f, u->mod, f.name) != hipSuccess) {
            (void)hipGetLastError();
            return fail(VSOM_ERR_HIP, std::string("hook module lacks ") + f.name);
        }
    if ((rc = vsom_custom_after_set_state(c))) {
        std::string keep = vsom_last_error();
        return fail(rc, keep);
    }
    *out = c;
    return VSOM_OK;
}

}   // extern "C"
