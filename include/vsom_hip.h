/*
 * vsom_hip.h -- C ABI of libvsom_hip.so: the MI355X (gfx950) implementation of the VSOM
 * training hot path (BMU search + Gaussian-neighbourhood mean / sigma^2 update).
 *
 * The reference (PereUbu7/Variational-Self-Organizing-Maps) has no FFI layer: callers link
 * libsom and use `class Som` (include/SOM.hpp:39-189).  This header is the boundary a
 * maintainer binds instead of src/Som.cpp's CPU loops; every entry point names the reference
 * member function it replaces.  Host-side `Som` / `Transformation` mirrors that call these
 * entry points live in variational-self-organizing-maps_amd/host/ (C++) and
 * variational-self-organizing-maps_amd/som.py (ctypes).  INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++ or torch types.
 *  - every function returns 0 on success, a negative vsom_status otherwise; the message is
 *    available from vsom_last_error() (thread-local).  Nothing throws across the ABI.
 *  - model state is row-major N x D fp32 (N = width*height, node index = y*width + x,
 *    D = Transformation::Length(J)); samples are row-major B x J fp32.
 *  - "host" pointers are ordinary host memory, copied synchronously; "dev" pointers are
 *    device memory on the context's GPU.
 *  - all work is enqueued on the context's HIP stream (vsom_set_stream adopts an external
 *    one, e.g. torch's current stream); entry points that return values to the host
 *    synchronise that stream, the *_async ones do not.
 *  - there is no CPU fallback: if no gfx950 device / code object is usable, vsom_create fails.
 */
#ifndef VSOM_HIP_H
#define VSOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vsom_ctx vsom_ctx;

typedef enum vsom_status {
    VSOM_OK = 0,
    VSOM_ERR_INVALID = -1, /* bad argument / state (e.g. no chunk loaded)          */
    VSOM_ERR_HIP = -2,     /* HIP runtime error, text in vsom_last_error()         */
    VSOM_ERR_NOMEM = -3,
    VSOM_ERR_UNSUPPORTED = -4
} vsom_status;

/* Transformation factories: src/Transformation.cpp:3-39 / 41-77 / 79-167 */
typedef enum vsom_transform {
    VSOM_STANDARD = 0,
    VSOM_MEDIAN = 1,
    VSOM_CLR = 2
} vsom_transform;

/* Som::WeigthDecayFunction: include/SOM.hpp:70-75 */
typedef enum vsom_decay {
    VSOM_EXPONENTIAL = 0,
    VSOM_INVERSE_PROPORTIONAL = 1,
    VSOM_BATCHMAP = 2
} vsom_decay;

/* BMU search strategy of the full search (results are identical) */
typedef enum vsom_bmu_mode {
    VSOM_BMU_AUTO = 0,      /* MFMA shortlist + exact-order refinement when applicable */
    VSOM_BMU_EXACT = 1,     /* brute-force exact-order VALU kernel                     */
    VSOM_BMU_SHORTLIST = 2  /* force the MFMA shortlist path                           */
} vsom_bmu_mode;

/* arithmetic of the phase-2 chain kernel */
typedef enum vsom_update_mode {
    VSOM_UPDATE_STRICT = 0, /* one rounding per fp32 operation: bit-identical to the reference's SSE2
                               build (default)                                                    */
    VSOM_UPDATE_FMA = 1,    /* contracted Standard chains: M = fma(c,d,M), S = fma(w*d,d,S) (1/3 fewer VALU
                               ops).  After ONE epoch from a given map, map / sigmaMap differ from the reference by
                               rounding only: |err| <= 1e-5 * max(|ref|, scale of the chain's operands) (measured
                               1e-7; pure element-wise <= 4e-7 on the MNIST workloads), BMU indices, bmuHits, MSE
                               and weightMap bit-exact.  NOT a schedule-level guarantee: the next search runs on
                               the perturbed map, near-ties flip, and a multi-epoch trainBatchSom leaves the
                               reference's trajectory within the first epochs (measured: profiles/
                               r3_fma_schedule.jsonl -- C3, 2 chunks: 5 of 8192 BMUs differ in epoch 0, 24 % by
                               epoch 9).  Use for single passes / throughput studies only.                  */
    VSOM_UPDATE_FMA_SIGMA = 2 /* only the variance accumulation (Som.cpp:867) contracted: t = c*d, M = M + t (Som.cpp:864)
                               as the reference rounds them, S = fma(w*d, d, S) (1/6 fewer VALU ops).  map is BIT-IDENTICAL, and so
                               are lastBMU, bmuHits, MSE and weightMap of every later epoch of a schedule -- no
                               training step reads sigmaMap (Transformation.cpp:7-8,45-46,82: the built-in
                               Comparers ignore the dispersion); sigmaMap is a sum of non-negative terms.
                               What can be PROVEN for it: both accumulations of B non-negative terms carry a
                               relative error <= (B+1)*2^-24 against the exact sum, so S differs by at most
                               2(B+1)*2^-24 and sigmaMap = sqrt(S/W) by (B+1)*2^-24 relative = 2.4e-4 at B = 4096
                               (if every rounding pointed the same way; ~sqrt(B)*2^-24 = 4e-6 when they do not).
                               What is MEASURED and asserted: within 1e-5 relative, element by element, over 10-14-
                               epoch schedules up to 128x128x784 with chunks of 4096 (worst 9.1e-7;
                               tests/test_gpu_fma_schedule.py).  The 1e-5 figure is therefore empirical.
                               Median and CLR have ONE arithmetic, bit-identical to the reference, in every mode:
                               the Median chains' fused operations are exact, and the CLR recurrence amplifies
                               rounding differences beyond the tolerance.                                    */
} vsom_update_mode;

/* when a batch epoch writes sigmaMap (vsom_set_sigma_mode) */
typedef enum vsom_sigma_mode {
    VSOM_SIGMA_AUTO = 0,    /* default: an epoch leaves its sigmaMap pending when the two epochs before it ended without
                               anybody reading theirs; a new context, and every context after a read, is eager again */
    VSOM_SIGMA_EAGER = 1,   /* every epoch writes sigmaMap, as the reference does */
    VSOM_SIGMA_LAZY = 2     /* every epoch that can leaves it pending (tests) */
} vsom_sigma_mode;

/* selectors for vsom_device_ptr / vsom_get_timing */
typedef enum vsom_buffer {
    VSOM_BUF_MAP = 0,      /* float   [N][D]                                    */
    VSOM_BUF_SIGMA = 1,    /* float   [N][D]                                    */
    VSOM_BUF_S = 2,        /* float   [N][D]                                    */
    VSOM_BUF_WEIGHT = 3,   /* float   [N]                                       */
    VSOM_BUF_HITS = 4,     /* uint64  [N]                                       */
    VSOM_BUF_LASTBMU = 5,  /* uint64  [chunk capacity]                          */
    VSOM_BUF_SQRES = 6,    /* float   [chunk capacity]  ||Comparer(x,M[bmu])||^2 */
    VSOM_BUF_CHUNK = 7,    /* float   [B][J] staged samples                     */
    VSOM_BUF_UMATRIX = 8   /* double  [N] of the last vsom_umatrix (NULL before the first) */
} vsom_buffer;

typedef enum vsom_timer {
    VSOM_T_STAGE = 0,      /* chunk re-layout kernels                           */
    VSOM_T_BMU = 1,        /* full / local BMU search kernels                   */
    VSOM_T_FINISH = 2,     /* bmuHits + MSE; the scoring kernels of vsom_similarity_batch / vsom_evaluate_batch and their masked forms, vsom_generate_batch's decode */
    VSOM_T_CW = 3,         /* neighbourhood weight chain (w, w/W) kernel        */
    VSOM_T_UPDATE = 4,     /* mean / sigma^2 chain kernel                       */
    VSOM_T_ONLINE = 5,     /* online (trainSingle) kernels                      */
    VSOM_T_SIGMA = 6,      /* sigmaMap = sqrt(S/W) pass after the assembly chain kernel */
    VSOM_T_COUNT = 7
} vsom_timer;

const char *vsom_last_error(void);
/* number of visible HIP devices (0 when none / no driver) */
int vsom_device_count(void);

/* ---- lifetime -------------------------------------------------------------------------
 * Som::Som(width,height,depth,Transformation) + Som::Construct (SOM.hpp:83-87,
 * Som.cpp:11-48): all state zero.  in_len = J (sample length); D = Length(J).          */
int vsom_create(vsom_ctx **out, int device, uint32_t width, uint32_t height,
                uint32_t in_len, int transform);
void vsom_destroy(vsom_ctx *ctx);

/* ---- caller-defined Transformation (reference include/Transformation.hpp:10-41; tests/test1.cpp builds one) -------
 * The caller's Comparer / Stepper arrive as HIP device source that defines two pure functions, each evaluated per
 * output element with read access to whole rows (J = sample length, D = model depth, R = residual length):
 *   __device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
 *                                 const float *value_weight, uint32_t J, uint32_t D);     element r < R of Comparer
 *   __device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
 *                              uint32_t J, uint32_t D);                                   element d < D of Stepper
 * x has J values, model and dispersion D, value_weight J: what Som.cpp builds at that call from the chunk's validity
 * (0.0f / 1.0f) and the column weights, see "value_weight" below; all 1 while neither has been set.  The source
 * is compiled with hipRTC for gfx950 (-O3 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt) together with
 * generic search / batch / online kernels that evaluate the hooks exactly where Som.cpp calls Comparer / Stepper, with
 * the fp32 operation order of the host path for custom hooks (host/src/vsom_custom.cpp): a device hook that computes
 * what a host hook computes gives the same bits.  Hooks must be pure (the reference's second Stepper call of an update
 * is taken to return the first one's values).
 * vsom_create_custom: a compile error is VSOM_ERR_INVALID with the hipRTC log in vsom_last_error(); depth must be
 * <= VSOM_CUSTOM_MAX_DEPTH (the batch update keeps a node's model, step and spread in LDS: 3 x D floats).
 * On a custom context these work: vsom_set_state / vsom_get_state, vsom_upload_chunk(_async), vsom_get_last_bmu /
 * vsom_set_last_bmu, vsom_get_sqres, vsom_bmu_batch, vsom_bmu_local_batch, vsom_find_bmu, vsom_find_local_bmu,
 * vsom_dist_single, vsom_distances, vsom_batch_epoch(_async), vsom_get_mse, vsom_train_single,
 * vsom_train_online_chunk(_acc, _fetch), vsom_residual_len (= R), vsom_prefetch_chunk / vsom_prefetch_wait /
 * vsom_commit_chunk (the prefetch takes a host copy of the rows; the commit uploads it), vsom_set_column_weights,
 * vsom_set_chunk_validity and the four _valid calls (below) and the plumbing (stream,
 * depth, nodes, pointers, timing).  Everything else -- device-resident chunks, the split batch phases, restricted and raw
 * distances, compaction, dedupe, shortlist statistics, non-strict update modes -- returns VSOM_ERR_INVALID and leaves
 * the context usable.  Custom contexts cannot join a group.  vsom_custom_compile_check compiles a hook source the
 * same way without opening a device. */
#define VSOM_CUSTOM_MAX_DEPTH 5120
int vsom_create_custom(vsom_ctx **out, int device, uint32_t width, uint32_t height, uint32_t in_len,
                       uint32_t depth, uint32_t residual_len, const char *hook_source);
int vsom_custom_compile_check(const char *hook_source, uint32_t depth, uint32_t residual_len);
/* ---- value_weight: missing fields and column weights of a custom context -------------------------------------------------
 * The reference lets missing fields and column weights matter through the valueWeight argument of Comparer / Stepper
 * alone (the built-in transformations drop it, Transformation.cpp:7-12,45-50), and Som builds it from the data set at
 * every call.  A custom context does the same from two settings, with valid as 0.0f / 1.0f and vw = valid * weights,
 * one fp32 product per element:
 *   vsom_bmu_batch, vsom_bmu_local_batch, vsom_distances    search / distance of a row with the row's vw   Som.cpp:134
 *   vsom_batch_epoch(_async)                                search with vw; the residual against SMap[bmu] and the
 *                                                           phase-2 Stepper with valid alone    :774,:780,:797,:803,:861,:867
 *   vsom_train_online_chunk(_acc, _fetch)                   row s: search, window Steppers, residual and BMU distance, all
 *                                                           with the vw of row s                              :891,:905-946
 *   the four _valid calls                                   one vw from valid_host (NULL = all valid) and the column
 *                                                           weights, where trainSingle / findBmu / findLocalBmu /
 *                                                           euclidianWeightedDist use totalWeight             :889-946
 * vsom_find_bmu, vsom_find_local_bmu, vsom_dist_single and vsom_train_single on a custom context keep an all-valid
 * vector and still apply the column weights, as findBmu(v) with a default `valid` would.
 * vsom_set_column_weights: the weights belong to the context, as getWeights() belongs to the loader, and hold until set
 * again (NULL = all 1).  Values pass through as given: a zero, a negative value or a NaN is the caller's business.
 * vsom_set_chunk_validity: the validity belongs to the loaded chunk -- one_mask == 0: B x J bytes row-major, != 0: J bytes
 * for every row; non-zero = valid; NULL = all valid.  Every call that makes a new chunk current (vsom_upload_chunk(_async),
 * vsom_commit_chunk, vsom_ensemble_upload_chunks for a custom member) resets it to all valid; it survives everything
 * else (epochs, vsom_set_last_bmu, vsom_set_state).  Both setters expand their input once, on the context's stream, into
 * the fp32 arrays the kernels read ([B][J] for a per-row mask, else [J]) and return when the caller's memory has been
 * read.  While neither is set every launch is the one of a context that never called them: same kernels, grid and bits.
 * Refused (VSOM_ERR_INVALID, nothing enqueued, the context stays usable): a null context; a built-in context for any
 * of the six (its hooks ignore valueWeight: use the masked calls, vsom_bmu_masked_batch, vsom_batch_epoch_masked,
 * vsom_train_online_chunk_masked ...); vsom_set_chunk_validity with no chunk loaded.  (It also checks for a chunk staged
 * ahead over the current rows, as the masked calls do; a custom context never stages ahead today -- its prefetch keeps
 * a host copy until the commit -- so that refusal cannot occur yet.)
 * Out of scope: validity for the consumers that refuse custom contexts (restricted, top-k, BMD, similarity, evaluate,
 * generate, U-matrix), groups, checkpoints of custom maps. */
int vsom_set_column_weights(vsom_ctx *ctx, const float *weights_host /*[J]; NULL = all 1*/);
int vsom_set_chunk_validity(vsom_ctx *ctx, const uint8_t *valid_host, int one_mask);
int vsom_find_bmu_valid(vsom_ctx *ctx, const float *v_host, const uint8_t *valid_host /*[J]*/, uint64_t *bmu_out,
                        float *dist_out);
int vsom_find_local_bmu_valid(vsom_ctx *ctx, const float *v_host, const uint8_t *valid_host, uint64_t last_bmu,
                              uint64_t *bmu_out, float *dist_out);
int vsom_dist_single_valid(vsom_ctx *ctx, const float *v_host, const uint8_t *valid_host, uint64_t node, float *dist_out);
int vsom_train_single_valid(vsom_ctx *ctx, const float *v_host, const uint8_t *valid_host, double eta, double sigma,
                            uint64_t *last_bmu, int decay_fn, float *residual_out, float *dist_out, uint64_t *bmu_out);
/* adopt an external hipStream_t (NULL = back to the context's own stream) */
int vsom_set_stream(vsom_ctx *ctx, void *hip_stream);
int vsom_synchronize(vsom_ctx *ctx);
int vsom_set_bmu_mode(vsom_ctx *ctx, int mode);
int vsom_set_update_mode(vsom_ctx *ctx, int mode);
/* [MI355X build; the reference computes sigmaMap in every epoch, Som.cpp:867-873, and reads it in none: the next epoch
 * rebuilds every row from zero and the built-in Comparers ignore the dispersion]
 * Pending sigmaMap.  A whole-map batch epoch (vsom_batch_epoch(_async), vsom_batch_phase2_async over [0, N)) of a Standard
 * or Median context on the lane = node chain kernels may run the mean chains alone -- half the arithmetic -- and keep what
 * the full kernel needs to produce that epoch's sigmaMap later.  The next whole-map epoch drops the record (it overwrites
 * every row); every other entry point materialises it first, on the context's stream: the full chain kernel of that
 * epoch, bit-identical to what the eager epoch would have written.  So results never depend on the mode; only where
 * the time goes does.  The calls that leave it pending, and no others:
 *   chunk staging     vsom_upload_chunk(_async), vsom_set_chunk_device, vsom_prefetch_chunk, vsom_prefetch_wait,
 *                     vsom_stage_next_device, vsom_commit_chunk
 *   batch epochs      vsom_batch_phase1_async, vsom_batch_finish_async, vsom_batch_phase2_async (a partial node range
 *                     materialises), vsom_batch_epoch_async, vsom_batch_epoch
 *   read-backs        vsom_get_mse, vsom_get_last_bmu, vsom_set_last_bmu, vsom_get_sqres, vsom_get_umatrix,
 *                     vsom_get_shortlist_stats, vsom_get_online_search_stats, vsom_get_timing, vsom_sigma_stats
 *   plumbing          vsom_synchronize, vsom_set_bmu_mode, vsom_set_update_mode, vsom_set_sigma_mode,
 *                     vsom_set_column_compaction, vsom_set_row_dedupe, vsom_enable_timing(_of), vsom_depth, vsom_nodes,
 *                     vsom_residual_len, vsom_chunk_size, vsom_pitch, vsom_chunk_pitch, vsom_small_map_chains,
 *                     vsom_device_ptr of every buffer but VSOM_BUF_SIGMA
 * (vsom_set_stream materialises.  So do the four vsom_batch_accum_* calls: the first of them materialises a pending record,
 * vsom_batch_accum_end writes its sigmaMap eagerly, none of them defers or counts towards VSOM_SIGMA_AUTO's rule.)
 * Partial node ranges, CLR, small maps (vsom_small_map_chains), group members, the masked
 * and custom epochs are always eager, and so is a context from the moment it joins an ensemble -- also after that
 * ensemble is destroyed.
 * The environment variable VSOM_SIGMA_MODE (auto / eager / lazy) sets the initial mode at vsom_create; any other value
 * makes vsom_create fail with VSOM_ERR_INVALID.
 * vsom_sigma_flush enqueues the materialisation (a no-op when nothing is pending) and counts as a read.
 * A call that is refused (VSOM_ERR_INVALID) changes no result; if it is not on the list above it may already have
 * materialised a pending sigmaMap and counted as a read (its arguments and the staged rows are checked behind the entry
 * check that materialises).
 * vsom_sigma_stats: out[0..3] = epochs deferred, records dropped, records materialised, 1 if one is pending now. */
int vsom_set_sigma_mode(vsom_ctx *ctx, int mode);
int vsom_sigma_flush(vsom_ctx *ctx);
int vsom_sigma_stats(vsom_ctx *ctx, uint64_t *out /*[4]*/);
/* [MI355X build; no counterpart in the reference, whose phase 2 walks every column: Som.cpp:840-875]
 * Exact retirement of the sample columns that are zero in every row of a chunk (csrc/vsom_compact.hip: their
 * chains stay 0 -- or NaN for a node whose first weight is 0/0 -- and they add nothing to the search's
 * contraction; MNIST has ~120 such columns per 4096-image chunk).  Results are bit-identical with it on or off.
 * Chunks of at least min_rows rows use it (default 1024: below that the passes cost more than they save);
 * min_rows < 0 switches it off. */
int vsom_set_column_compaction(vsom_ctx *ctx, long min_rows);
/* [MI355X build] The exact search (small problems, the shortlist's redo list, VSOM_BMU_EXACT) evaluates ONE representative
 * per class of bit-identical model rows (csrc/vsom_bmu.hip: equal rows give equal distances and the reference's strict `<`
 * keeps the lowest index, Som.cpp:293-304) -- batch training on degenerate chunks leaves such maps (an empty chunk: one
 * class).  Results are bit-identical with it on or off.  Searches of at least min_work (sample, node, value) triples use
 * it (default 2e10; behind a shortlist search -- its redo list -- only for the CLR comparer, whose collapsed maps put whole
 * chunks on that list); 0: always; < 0: never. */
int vsom_set_row_dedupe(vsom_ctx *ctx, double min_work);
/* diagnostics of the last MFMA-shortlist search (synchronises): out[0] = samples that had to be
 * redone by the exact-order kernel, out[1] = shortlisted candidates in total, out[2] = samples
 * searched, out[3] = number of shortlist searches so far */
int vsom_get_shortlist_stats(vsom_ctx *ctx, uint32_t *out /*[4]*/);
uint32_t vsom_depth(const vsom_ctx *ctx);   /* D */
uint32_t vsom_nodes(const vsom_ctx *ctx);   /* N */

/* ---- state (Som::map / sigmaMap / SMap / weightMap / bmuHits, SOM.hpp:56-61) -----------
 * NULL pointers are skipped.  Replaces getNeuron/getSigmaNeuron/getWeigthMap/getBmuHits
 * (Som.cpp:164-212) and the element writes of randomInitialize/load (Som.cpp:977-997).    */
int vsom_set_state(vsom_ctx *ctx, const float *map, const float *sigma, const float *S,
                   const float *weight, const uint64_t *bmu_hits);
int vsom_get_state(vsom_ctx *ctx, float *map, float *sigma, float *S, float *weight,
                   uint64_t *bmu_hits);

/* ---- chunk (DataSet::loadNextDataFromStream, DataSet.cpp:118-160) ----------------------
 * Stages B samples and zeroes lastBMU (DataSet.cpp:136-137).                              */
int vsom_upload_chunk(vsom_ctx *ctx, const float *x_host, size_t B);
/* same without the final wait: copy and staging kernels are enqueued on the context's stream and the call returns; x_host
 * must be pinned (vsom_host_alloc; from pageable memory the copy degrades to a blocking one) and stay unchanged until a
 * call that synchronises the context (vsom_get_mse, vsom_get_last_bmu, vsom_train_online_chunk_fetch ...) has returned.
 * For the first chunk of an epoch, when nothing runs that a prefetch on the copy stream could overlap with. */
int vsom_upload_chunk_async(vsom_ctx *ctx, const float *x_host, size_t B);
/* same, samples already resident in HBM (no PCIe copy) */
int vsom_set_chunk_device(vsom_ctx *ctx, const float *x_dev, size_t B);
/* Double-buffered ingest: the reference reloads every chunk from its loader each
 * epoch (Som.cpp:737, DataSet.cpp:118-160), so the host->device copy of chunk i+1 should run while
 * chunk i trains.  vsom_prefetch_chunk copies B x J floats into the context's NEXT raw device buffer
 * on a copy stream and returns at once when x_host is pinned (vsom_host_alloc); the current chunk is
 * untouched.  vsom_commit_chunk makes the prefetched chunk current: the compute stream waits for the
 * copy, stages it and zeroes lastBMU -- the same state vsom_upload_chunk of the same data leaves.
 * vsom_prefetch_wait blocks until the copy has left x_host (then the host buffer may be rewritten). */
int vsom_host_alloc(void **out, size_t bytes);   /* pinned host memory */
int vsom_host_free(void *p);
int vsom_prefetch_chunk(vsom_ctx *ctx, const float *x_host, size_t B);
/* Staging ahead (round 5): when the call directly follows an asynchronous batch epoch on the current chunk
 * (vsom_batch_epoch_async / vsom_batch_phase2_async, Standard / Median on a map large enough for the lane = node
 * chain kernels but small enough that their launch leaves workgroup slots idle -- at most two rounds of the chip's
 * resident workgroups, e.g. 64x64x784; bigger launches lose more to the company than the overlap saves), the
 * prefetched chunk's staging kernels are enqueued too -- on the copy stream, after the point of the
 * epoch from which nothing reads the current chunk's sample rows any more -- so that they run BESIDE the epoch's
 * chains and vsom_commit_chunk launches nothing.  Between such a prefetch and its commit the current chunk's
 * sample rows are gone: lastBMU, the MSE and the model state of the current chunk stay readable, a search or a
 * distance call on it does not (commit first), nor does a further vsom_batch_phase2_async range small enough for the
 * small-map chain kernel (vsom_small_map_chains), which reads the rows themselves.  In every other situation the staging
 * happens at commit, as before. */
int vsom_prefetch_wait(vsom_ctx *ctx);
int vsom_commit_chunk(vsom_ctx *ctx);
/* the same for a next chunk that ALREADY lives in HBM (x_dev must stay valid until vsom_commit_chunk has been called):
 * staged beside the running epoch when that is possible now, else at vsom_commit_chunk */
int vsom_stage_next_device(vsom_ctx *ctx, const float *x_dev, size_t B);
/* DataSet::getLastBMU (DataSet.cpp:60-69) */
int vsom_get_last_bmu(vsom_ctx *ctx, uint64_t *out_host);
int vsom_set_last_bmu(vsom_ctx *ctx, const uint64_t *in_host);
int vsom_get_sqres(vsom_ctx *ctx, float *out_host);

/* ---- search ----------------------------------------------------------------------------
 * Som::findBmu for every sample of the chunk (Som.cpp:291-309, distance :124-141);
 * writes lastBMU / sqres on the device; optional host copies.                             */
int vsom_bmu_batch(vsom_ctx *ctx, uint64_t *idx_out_host, float *dist_out_host);
/* Som::findBmu(v) for one host vector (Som.cpp:283-309; the perf harness calls it 1000 times,
 * tests/performance/perf_tests.cpp:181-199): one copy, one scan launch, 32 bytes back.  Does not
 * touch the staged chunk.  dist_out = euclidianWeightedDist(bmu, v) (NaN when node 0 is NaN). */
int vsom_find_bmu(vsom_ctx *ctx, const float *v_host, uint64_t *bmu_out, float *dist_out);
/* Som::euclidianWeightedDist(pos, v, ...) (Som.cpp:124-141) and Som::findLocalBmu(v, ..., lastBMU, ...)
 * (Som.cpp:335-454) for ONE host vector (the perf harness calls them a million times each,
 * tests/performance/perf_tests.cpp:200-222, 269-295): one copy, one single-wavefront launch, 16 bytes back,
 * one synchronisation, no allocation.  Neither touches the staged chunk. */
int vsom_dist_single(vsom_ctx *ctx, const float *v_host, uint64_t node, float *dist_out);
int vsom_find_local_bmu(vsom_ctx *ctx, const float *v_host, uint64_t last_bmu, uint64_t *bmu_out, float *dist_out);
/* Som::findRestrictedBmu(v, ..., minBmuHits, ...) (Som.cpp:313-332: node 0 seeds the search whatever its hits) and the
 * distances Som::findRestrictedBmd walks (Som.cpp:457-487: dist_out_host[N] = euclidianWeightedDist(i, v)) for ONE host
 * vector, the same way: one copy, one scan launch, one synchronisation; the staged chunk is not touched. */
int vsom_find_restricted_bmu(vsom_ctx *ctx, const float *v_host, uint64_t min_hits, uint64_t *bmu_out, float *dist_out);
int vsom_distances_single(vsom_ctx *ctx, const float *v_host, float *dist_out_host);
/* Som::findLocalBmu from the current lastBMU of every sample (Som.cpp:335-454) */
int vsom_bmu_local_batch(vsom_ctx *ctx, uint64_t *idx_out_host, float *dist_out_host);
/* Som::euclidianWeightedDist(pos, v, ...) for `count` (node, sample-row) pairs of the chunk */
int vsom_distances(vsom_ctx *ctx, const uint64_t *nodes_host, const uint64_t *rows_host,
                   size_t count, float *dist_out_host);

/* ---- consumers of the search outside the training loop (SURVEY 8f "next" rows) --------------
 * Som::findRestrictedBmu (Som.cpp:313-332) for every sample of the chunk: argmin over node 0 and
 * the nodes with bmuHits >= min_hits.  Overwrites the chunk's lastBMU / sqres like vsom_bmu_batch. */
int vsom_bmu_restricted_batch(vsom_ctx *ctx, uint64_t min_hits, uint64_t *idx_out_host,
                              float *dist_out_host);
/* Som::euclidianWeightedDist of EVERY node for chunk row `row` (input of findRestrictedBmd,
 * Som.cpp:457-487); dist_out_host[N]. */
int vsom_distances_row(vsom_ctx *ctx, size_t row, float *dist_out_host);
/* Som::findRestrictedBmd (Som.cpp:457-487) for chunk rows [r0, r1), and optionally one draw per row.
 * Read-only: lastBMU, sqres, bmuHits and the map are not touched.
 * norm_out[r1-r0]      C of each row (may be NULL)
 * prob_out[(r1-r0)*N]  row-major p_i / C, what findRestrictedBmd returns for that row (may be NULL)
 * u_host[r1-r0]        one uniform in [0,1) per row; required iff draw_out != NULL
 * draw_out[r1-r0]      drawn node per row, UINT64_MAX when the row has no mass (may be NULL)
 * p_i = bmuHits[i] >= min_hits ? exp(-(double)d_i * d_i / 2) : 0 with d_i the fp32 distance of vsom_distances_row
 * (node 0 is not exempt), C = ((0 + p_0) + p_1) + ... in node order, in double.  The draw is the smallest i whose
 * running sum exceeds u * C -- the largest i with p_i > 0 when rounding leaves none; no draw when C is 0 or not
 * finite.  exp runs on the device (within an ulp of libm's).  Refuses (VSOM_ERR_INVALID, nothing enqueued) custom
 * contexts, no chunk, a bad row range, draws without uniforms, a uniform that is NaN or outside [0,1), a chunk staged
 * ahead.  Device scratch: p of at most max(1, 256 MiB / (8 N)) rows at a time. */
int vsom_bmd_batch(vsom_ctx *ctx, uint64_t min_hits, size_t r0, size_t r1, const double *u_host,
                   uint64_t *draw_out, double *norm_out, double *prob_out);
/* The k best matching units of chunk rows [r0, r1): the runner-up for the topographic error, k-nearest-node queries.
 * idx_out[(r1-r0)*k]   row-major, required
 * dist_out[(r1-r0)*k]  d of each idx_out entry, bit for bit (may be NULL)
 * d_i is the fp32 distance of vsom_distances_row; nodes are ordered by the key (d_i, i) with NaN after +inf, so ties go
 * to the lower index.  Every node is a candidate (bit-identical model rows each appear, in index order).  Entry 0 is
 * findBmu's BMU, the node vsom_bmu_batch returns (Som.cpp:291-309): node 0 with a NaN distance when d_0 is NaN; entries
 * 1..k-1 are the other nodes in ascending key order (when d_0 is not NaN the row is the k smallest keys).  A NaN distance
 * is stored as the quiet NaN 0x7FC00000, as vsom_bmu_batch's sqres.  Read-only: the map, sigma, bmuHits, lastBMU and
 * sqres are not touched.  Refuses (VSOM_ERR_INVALID, nothing enqueued) custom contexts, no chunk, a bad row range,
 * k = 0, k > 64, k > N, a null idx_out, a chunk staged ahead; an empty range returns VSOM_OK.  Device scratch: at most
 * 64 node groups of k keys for a slice of at most 64 MiB / (512 k) rows at a time. */
int vsom_bmu_topk_batch(vsom_ctx *ctx, uint32_t k, size_t r0, size_t r1, uint64_t *idx_out, float *dist_out);
/* Som::measureSimilarity's per-record report (Som.cpp:631-714) for chunk rows [r0, r1): every row is searched and then
 * scored against its best matching unit, column by column, in units of that unit's sigma -- one call, one stream wait.
 * Search: b = Som::findRestrictedBmu(x_r, min_hits) for EVERY row of the chunk, exactly as vsom_bmu_restricted_batch (node 0
 * seeds the search whatever its hits); it overwrites the chunk's lastBMU / sqres for the whole chunk like that call.  With
 * min_hits = 0 every node qualifies, the search is findBmu's and takes vsom_bmu_batch's path (the shortlist included; every
 * vsom_set_bmu_mode gives the same indices).
 * Per column d < C = min(J, D), in fp32 with one rounding per operation and nothing contracted: m = map[b][d],
 * s = sigmaMap[b][d], k = (float)num_sigmas,
 *   sM    = s > 1e-5f ? 1e-5f : s   VSOM_SIGMA_AS_WRITTEN: the select of Som.cpp:658 as the reference wrote it, a cap (NaN stays)
 *           s > 1e-5f ? s : 1e-5f   VSOM_SIGMA_FLOOR: the evident intent, a floor (a NaN sigma becomes 1e-5f)
 *   delta = (x - m) / sM / k (:671),  lo = m - sM * k,  hi = m + sM * k (:675-677);
 * column d of row r is valid iff valid_host == NULL or valid_host[(r - r0) * J + d] != 0.
 * Outputs (host pointers, each may be NULL; entry r - r0 belongs to row r; lowest column on ties; columns d < C only):
 *   bmu, dist          b and the stored sqres of the row, as the search calls return them (a NaN distance is 0x7FC00000)
 *   dmax, dmax_col     the largest delta (signed) over the columns whose delta is not NaN; -inf, UINT32_MAX when none
 *   first              delta of the lowest column with delta > -99999999.f; NaN (0x7FC00000) when none
 *   amax, amax_col     the largest |delta| over the VALID columns whose delta is finite: the row's anomaly score and the
 *                      column that causes it; 0, UINT32_MAX when none
 *   outside            the number of valid columns with x < lo || x > hi (a NaN compares false, as in :702)
 *   delta              dense report, delta[(r - r0) * C + d], NaN and +-inf replaced by 0 (:693)
 * first and dmax carry the reference's running maximum (:684-690 compares the signed delta and stores its fabs): start at
 * the first row whose `first` is not NaN with maxValue = |first|; for that row and every later one, dmax > maxValue makes
 * maxValue = dmax and that row the reported one; measureSimilarity returns outside[reported row] == 0.
 * Read-only apart from lastBMU / sqres: map, sigmaMap, S, weightMap, bmuHits and the chunk are untouched.  Refuses
 * (VSOM_ERR_INVALID, nothing enqueued, the context stays usable): a null context or out, custom contexts, no chunk, a chunk
 * staged ahead, r0 > r1 or r1 > B, an unknown sigma_rule.  An empty range returns VSOM_OK and enqueues nothing (no search).
 * Device scratch: 36 bytes per row, the validity bytes when given, and for the dense report a slice of at most
 * max(1, 64 MiB / (4 C)) rows at a time; without delta nothing of size rows x C is allocated.  delta and valid_host travel
 * straight from / to the caller's memory, the per-row results through pinned memory of the context. */
typedef enum vsom_sigma_rule {
    VSOM_SIGMA_AS_WRITTEN = 0,
    VSOM_SIGMA_FLOOR = 1
} vsom_sigma_rule;
typedef struct vsom_similarity_out {
    uint64_t *bmu;
    float *dist;
    float *dmax;
    uint32_t *dmax_col;
    float *first;
    float *amax;
    uint32_t *amax_col;
    uint32_t *outside;
    float *delta;
} vsom_similarity_out;
int vsom_similarity_batch(vsom_ctx *ctx, uint64_t min_hits, int num_sigmas, int sigma_rule, size_t r0, size_t r1,
                          const uint8_t *valid_host, vsom_similarity_out *out);
/* The best matching unit of chunk rows [r0, r1) over their VALID columns only -- partial-vector search, the SOM's way
 * of handling missing data -- and the record imputed from it.  Every other search treats every value as present, as the
 * reference's built-in Comparers do (Transformation.cpp:7-8,45-46 drop valueWeight); this one computes what
 * Som::euclidianWeightedDist documents ("Considers only dimensions where valid is true", Som.cpp:112-141, the form of the
 * commented-out :139) -- the evident intent next to "as written", as VSOM_SIGMA_FLOOR is.  Standard and Median (D = J).
 * Mask: valid_host is (r1-r0) x J bytes, row-major, when one_mask == 0, and J bytes applied to every row (a column mask:
 * "which unit matches these columns, and what do its others say?") when one_mask != 0; a non-zero byte means valid.
 * Distance of row x to node m: r_d = valid[d] ? (m_d - x_d) : +0.0f -- a select, not a multiply: a NaN or inf stored at
 * an invalid position of x or m has no effect -- and d = r.dot(r) over all J positions in the Eigen packet order of the
 * unmasked distance (8 class accumulators, the same reduction tree).  With an all-valid mask every (bmu, dist) is
 * bit-identical to vsom_bmu_restricted_batch with the same min_hits (min_hits = 0: to vsom_bmu_batch, every mode).
 * Argmin: Som::findRestrictedBmu (Som.cpp:313-332): node 0 seeds the search whatever its hits, then strict `<` over the
 * nodes with bmuHits >= min_hits, so the lowest index wins ties; NaN never wins and a NaN d_0 keeps node 0.  A NaN
 * distance is stored as 0x7FC00000.  A row without a valid column has every distance +0: node 0, distance 0, nvalid 0.
 * Outputs (host pointers, each may be NULL; entry r - r0 belongs to row r):
 *   bmu, dist   the unit and the masked distance of the row to it, bit for bit
 *   nvalid      the number of valid columns of the row
 *   fill        [(r1-r0) * J] row-major: the bits of x at valid positions, of map[bmu][d] at invalid ones
 * Read-only: lastBMU, sqres, the map, sigmaMap, S, weightMap, bmuHits and the chunk are untouched.  One call makes one
 * stream wait; validity bytes and results travel from / to the caller's memory.  Refuses (VSOM_ERR_INVALID, nothing
 * enqueued, the context stays usable): a null context, out or valid_host, custom and CLR contexts (the CLR residual runs
 * over column pairs), no chunk, a chunk staged ahead, r0 > r1 or r1 > B.  An empty range returns VSOM_OK and enqueues
 * nothing.  Device scratch: the rows are searched in slices whose scratch stays within 64 MiB (one row where a single
 * row needs more): per row of a slice J + roundup(J, 32) validity bytes, at most 64 keys of 8 bytes, 17 bytes of results
 * and, with fill, 4 J bytes. */
typedef struct vsom_masked_out {
    uint64_t *bmu;
    float *dist;
    uint32_t *nvalid;
    float *fill;
} vsom_masked_out;
int vsom_bmu_masked_batch(vsom_ctx *ctx, uint64_t min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask,
                          vsom_masked_out *out);
/* Som::evaluate (Som.cpp:490-523), the validation loss of a map, for chunk rows [r0, r1): every row is searched, scored
 * against its best matching unit, and the running mean of :519 is taken -- one call, one stream wait, nothing of size
 * N x D moves.
 * Search: b = Som::findBmu(x_r) for EVERY row of the chunk, exactly as vsom_bmu_batch (the same path, the shortlist
 * included; every vsom_set_bmu_mode gives the same indices); it overwrites the chunk's lastBMU / sqres like that call.  The
 * built-in comparers ignore `valid`, so the distance is unmasked ("as written").
 * Per column d < C = min(J, D), in fp32 with one rounding per operation, nothing contracted, no fast-math log:
 * m = map[b][d], x = x_r[d],
 *   be   = log(m) * x + log(1.0f - m) * (1.0f - x)              (:509; the reference's never-filled `ones` taken as ones)
 *   be   = (isnan(be) || isinf(be)) ? -99999.0f : be            (:512)
 *   val  = valid ? continuous_host[d] : 0.0f                    (:505; column d of row r is valid iff valid_host == NULL
 *                                                                or valid_host[(r - r0) * J + d] != 0)
 *   t    = (be * binary_host[d]) * val                          (:514, in that order)
 *   bsum = t.dot(t) over d = 0..C-1 in Eigen's packet order (two 4-wide accumulators over the multiples of 8,
 *          p0 += p1, the packet tail, (p0[0] + p0[2]) + (p0[1] + p0[3]), the scalar tail) -- the order of every other
 *          r.dot(r) of this library.
 * Outputs (host pointers, each may be NULL; entry r - r0 belongs to row r):
 *   bmu, dist   b and euclidianWeightedDist(b, x_r): what vsom_bmu_batch returns, bit for bit (a NaN distance is 0x7FC00000)
 *   bsum        binaryError.dot(binaryError) of the row, before the sqrt of :519
 *   nrepl       the number of columns d < C whose term was replaced by -99999 and whose factor is non-zero
 *               (binary_host[d] != 0 and val != 0)
 *   error[1]    error += 1.0 / (i + 1.0) * ((double)dist + sqrt((double)bsum) - error) in row order, i counted from 0 at r0,
 *               evaluated on the host from the returned dist / bsum
 * Accuracy: only log can differ from a CPU restatement.  For x in [0,1] and m in (0,1) both products of be have the same
 * sign, nothing cancels, and with L the device log's error bound in ulps bsum lies within (C + 2 L + 4) * 2^-24 relative of
 * the float64 value computed from the fp32 operands (1.0f - m and 1.0f - x formed in fp32 first); the sqrt halves it.
 * L = 1 is taken (csrc/vsom_evaluate.hip names the source and labels the assumption).  A zero factor, a replaced term,
 * the search outputs and the running mean of the returned values carry no tolerance.  With binary_host all 0 every t
 * is +-0, bsum is 0 and error is the running mean of vsom_bmu_batch's distances.
 * Read-only apart from lastBMU / sqres: map, sigmaMap, S, weightMap, bmuHits and the chunk are untouched.  Refuses
 * (VSOM_ERR_INVALID, nothing enqueued, the context stays usable): a null context, out, binary_host or continuous_host,
 * custom contexts, no chunk, a chunk staged ahead, r0 > r1 or r1 > B.  An empty range returns VSOM_OK, enqueues nothing
 * (no search) and writes *error = 0.  Device scratch: 20 bytes per row, the validity bytes when given, 8 J bytes of column
 * arrays; one grow-only set.  valid_host travels straight from the caller's memory, the column arrays and the per-row
 * results through pinned memory of the context; the scoring launch is timed under VSOM_T_FINISH. */
typedef struct vsom_evaluate_out {
    uint64_t *bmu;
    float *dist;
    float *bsum;
    uint32_t *nrepl;
    double *error;
} vsom_evaluate_out;
int vsom_evaluate_batch(vsom_ctx *ctx, size_t r0, size_t r1, const float *binary_host, const float *continuous_host,
                        const uint8_t *valid_host, vsom_evaluate_out *out);
/* vsom_similarity_batch and vsom_evaluate_batch for records with missing fields: the search runs over the VALID columns of
 * every row, as vsom_bmu_masked_batch, and the row is scored against that unit in its valid columns only -- one call, one
 * stream wait, nothing of size N x D moves.  (The valid_host of the two unmasked calls only gates which columns count AFTER
 * a search that took a missing field for a measured zero.)  Standard and Median (D = J, C = J).
 * Mask: as vsom_bmu_masked_batch -- valid_host is (r1-r0) x J bytes, row-major (entry (r - r0) * J + d belongs to chunk row r),
 * when one_mask == 0, and J bytes applied to every row when one_mask != 0; a non-zero byte means valid; required.
 * Search: for rows [r0, r1) ONLY, the search of vsom_bmu_masked_batch(min_hits, mask) word for word: r_d = valid ?
 * (m_d - x_d) : +0.0f as a select on the bits, the Eigen packet order of the exact tile, findRestrictedBmu's argmin (node 0
 * seeds, strict `<` over the nodes with bmuHits >= min_hits, NaN never wins, a NaN d_0 keeps node 0 and stores 0x7FC00000).
 * bmu, dist and nvalid are bit-identical to that call's outputs for the same arguments; a row without a valid column gets
 * node 0, distance +0, nvalid 0.
 * vsom_similarity_masked_batch scores as vsom_similarity_batch does (the same fp32 operations, both sigma rules) with one
 * addition: at an invalid column delta is the quiet NaN, by select, before anything is reduced.  So dmax / dmax_col and
 * first range over the valid columns only, amax / amax_col and outside are as there (they always ranged over the valid
 * columns), and the dense delta stores 0 at an invalid column.  A row without a valid column reports dmax = -inf,
 * dmax_col = UINT32_MAX, first = NaN (0x7FC00000), amax = 0, amax_col = UINT32_MAX, outside = 0 and a zero delta row.  first
 * and dmax feed the same running maximum as those of vsom_similarity_batch.
 * vsom_evaluate_masked_batch scores as vsom_evaluate_batch does, except
 *   t = valid ? (be * binary_host[d]) * continuous_host[d] : +0.0f
 * -- a select, not the multiplication by a zero val: an inf product at an invalid column cannot become NaN.  nrepl counts
 * valid columns only; error is the running mean of (double)dist + sqrt((double)bsum) in row order from r0, on the host, with
 * the masked dist; an empty range writes *error = 0.  The accuracy statement of vsom_evaluate_batch holds for bsum.
 * Outputs: the fields of vsom_similarity_out / vsom_evaluate_out, and nvalid, the number of valid columns of the row (host
 * pointers, each may be NULL; entry r - r0 belongs to row r).
 *  - With an all-valid mask every output of vsom_similarity_masked_batch is bit-identical to vsom_similarity_batch(min_hits,
 *    ..., valid_host = NULL), with nvalid = J; every output of vsom_evaluate_masked_batch(min_hits = 0) to
 *    vsom_evaluate_batch(valid_host = NULL) in every vsom_set_bmu_mode, bsum included (the same kernel arithmetic).
 *  - What a row of the chunk holds at an invalid position (NaN, +-inf, 1e30, values outside [0,1]) reaches no output, nor
 *    does what the unit's map / sigmaMap rows hold there.
 *  - Read-only: lastBMU and sqres (unlike the unmasked scorers: only [r0, r1) is searched, into scratch), map, sigmaMap, S,
 *    weightMap, bmuHits and the chunk are untouched.
 *  - A pending sigmaMap is materialised by both calls.
 * Refuses (VSOM_ERR_INVALID, nothing enqueued, the context stays usable): a null context, out or valid_host, a null
 * binary_host or continuous_host (evaluate), custom and CLR contexts (the CLR residual runs over column pairs), no chunk, a
 * chunk staged ahead, r0 > r1 or r1 > B, an unknown sigma_rule.  An empty range returns VSOM_OK and enqueues nothing.
 * Device scratch: the rows are searched and scored in slices that follow vsom_bmu_masked_batch's rule (64 MiB; with the dense
 * delta at most max(1, 64 MiB / (4 J)) rows, 4 J bytes each); per row of a slice J + roundup(J, 32) validity bytes, at most
 * 64 keys of 8 bytes and 17 bytes of search results; per row of the call 40 (similarity) or 24 (evaluate) bytes of results,
 * which return through pinned memory of the context; evaluate: 8 J bytes of column arrays.  A slice's validity bytes go up
 * once and are packed once; the packed bytes serve the search and the scoring.  The search is timed under VSOM_T_BMU, the
 * scoring under VSOM_T_FINISH. */
typedef struct vsom_similarity_masked_out {
    uint64_t *bmu;
    float *dist;
    float *dmax;
    uint32_t *dmax_col;
    float *first;
    float *amax;
    uint32_t *amax_col;
    uint32_t *outside;
    float *delta;
    uint32_t *nvalid;
} vsom_similarity_masked_out;
typedef struct vsom_evaluate_masked_out {
    uint64_t *bmu;
    float *dist;
    float *bsum;
    uint32_t *nrepl;
    double *error;
    uint32_t *nvalid;
} vsom_evaluate_masked_out;
int vsom_similarity_masked_batch(vsom_ctx *ctx, uint64_t min_hits, int num_sigmas, int sigma_rule, size_t r0, size_t r1,
                                 const uint8_t *valid_host, int one_mask, vsom_similarity_masked_out *out);
int vsom_evaluate_masked_batch(vsom_ctx *ctx, uint64_t min_hits, size_t r0, size_t r1, const float *binary_host,
                               const float *continuous_host, const uint8_t *valid_host, int one_mask,
                               vsom_evaluate_masked_out *out);
/* Som::autoEncoder's records (Som.cpp:568-623) for chunk rows [r0, r1): a model vector per row drawn from a restricted best
 * matching distribution (Som::findRestrictedBmd, vsom_bmd_batch), and every column of the record sampled from a
 * logit-approximated normal around that unit's map / sigmaMap values -- one call, one stream wait, nothing of size N x D moves.
 * rule (vsom_generate_rule):
 *   VSOM_GENERATE_AS_WRITTEN  the reference calls variationalAutoEncoder(data) afresh for every row, and that walks the whole
 *                             data set and returns the draw of its LAST row (:532-565): every row's unit is an independent
 *                             draw, with the row's own uniform, from the distribution of chunk row B - 1 (whatever r0, r1)
 *   VSOM_GENERATE_PER_ROW     row r's unit is drawn from row r's own distribution, the evident intent (:584-589)
 * The draw is vsom_bmd_batch's, word for word: p_i = bmuHits[i] >= min_hits ? exp(-(double)d_i * d_i / 2) : 0,
 * C = ((0 + p_0) + p_1) + ... in node order in double, the unit is the smallest i whose running sum exceeds u * C, the
 * largest i with p_i > 0 when rounding leaves none, UINT64_MAX when C is 0 or not finite.  PER_ROW returns the bits
 * vsom_bmd_batch returns for the same rows and uniforms; AS_WRITTEN those of vsom_bmd_batch on [B - 1, B) with each uniform.
 *   u_host[r1-r0]        one uniform in [0,1) per row, required
 *   l_host[(r1-r0)*C]    row-major, C = min(J, D): the reference's L of :608, one per value.  Not validated; the arithmetic
 *                        is IEEE: L = 0 gives -inf, L = 1 gives +inf, L outside [0,1] gives NaN
 * Decode, per row with unit b and logical column d < C (the column vsom_get_state returns), m = map[b][d], s = sigmaMap[b][d],
 * in double with one rounding per operation, nothing contracted, in the order of :609:
 *   q = L / (1 - L);  g = log(q);  z = g / 1.6;  t = z * (double)s;  rec = t + (double)m
 * A row without mass has unit = UINT64_MAX and the quiet NaN 0x7FF8000000000000 in every column of its record.
 * Outputs (host pointers, each may be NULL; entry r - r0 belongs to row r): unit[r1-r0], record[(r1-r0)*C] row-major.
 * Accuracy: only log can differ from a CPU restatement (q is one IEEE division on both sides).  With Ld, Lh the error
 * bounds in ulps of the device's and of the host's double log, and ulp(x) <= 2^-52 |x|: the two g differ by at most
 * (Ld + Lh) 2^-52 |g|; the division by 1.6 rounds once on each side (2 * 2^-53), the product with s likewise, so the two t
 * differ by at most (Ld + Lh + 2) 2^-52 |z s|; the final sum rounds once on each side, 2^-53 (|rec_dev| + |rec_ref|).  To
 * first order in 2^-52:
 *   |rec_dev - rec_ref| <= (Ld + Lh + 2) * 2^-52 * |z * s| + 2^-52 * |rec_ref|
 * Ld = Lh = 1 are taken AS ASSUMPTIONS (csrc/vsom_generate.hip names the sources).  No tolerance: unit; L = 0.5 (q = 1,
 * g = +0, rec = m); s = 0 with a finite g (rec = m); NaN and inf propagation; the row without mass.
 * Read-only: map, sigmaMap, S, weightMap, bmuHits, lastBMU, sqres and the chunk are untouched.  Refuses (VSOM_ERR_INVALID,
 * nothing enqueued, the context stays usable): a null context, out, u_host or l_host, custom contexts, C = 0, an unknown
 * rule, no chunk, a chunk staged ahead, r0 > r1 or r1 > B, a uniform that is NaN or outside [0,1).  An empty range returns
 * VSOM_OK and enqueues nothing.  Device scratch, in the query arena: the distribution of a slice (PER_ROW: at most 256 MiB
 * of p) or of row B - 1 (AS_WRITTEN: 8 N doubles), and a slice's L and record, at most 64 MiB each; VSOM_GENERATE_SLICE_ROWS
 * (read at every call) caps the rows of a slice.  l_host and record travel straight from and to the caller's memory, u_host
 * and unit as vsom_bmd_batch moves them.  The draw launches are timed under VSOM_T_BMU, the decode under VSOM_T_FINISH. */
typedef enum vsom_generate_rule {
    VSOM_GENERATE_AS_WRITTEN = 0, /* every row's unit is drawn from the BMD of the chunk's LAST row (row B-1) */
    VSOM_GENERATE_PER_ROW = 1     /* row r's unit is drawn from row r's own BMD: the evident intent (Som.cpp:584-589) */
} vsom_generate_rule;
typedef struct vsom_generate_out { uint64_t *unit; double *record; } vsom_generate_out;
int vsom_generate_batch(vsom_ctx *ctx, uint64_t min_hits, int rule, size_t r0, size_t r1,
                        const double *u_host, const double *l_host, vsom_generate_out *out);
/* The decode of vsom_generate_batch for `count` units the caller names: record_out[i*C + d] from nodes_host[i] and
 * l_host[i*C + d], the same kernel, the same arithmetic and accuracy.  Needs no chunk and makes no search; read-only.
 * Refuses (VSOM_ERR_INVALID, nothing enqueued): a null context, l_host or record_out, a null nodes_host with count > 0,
 * custom contexts, C = 0, a node >= N.  count = 0 returns VSOM_OK and enqueues nothing. */
int vsom_decode_nodes(vsom_ctx *ctx, const uint64_t *nodes_host, size_t count, const double *l_host, double *record_out);
/* vsom_bmd_batch and vsom_generate_batch for records with missing fields: the distribution over the units is taken over the
 * VALID columns of every row, and the records sampled from it keep what was observed -- the sampled (multiple) imputation next
 * to the point imputation of vsom_bmu_masked_batch's fill.  (The unmasked calls take a missing field for a measured zero: the
 * mass moves towards units near 0 there, and one wild placeholder, d > ~38.6, leaves the row without mass.)  Standard and
 * Median (D = J).  One call, one stream wait, nothing of size N x D moves.
 * Mask: as vsom_bmu_masked_batch -- valid_host is (r1-r0) x J bytes, row-major (entry (r - r0) * J + d belongs to chunk row r),
 * when one_mask == 0, and J bytes applied to every row when one_mask != 0; a non-zero byte means valid; required.
 *
 * vsom_bmd_masked_batch is vsom_bmd_batch, word for word, on the masked distance of vsom_bmu_masked_batch: r_d = valid ?
 * (m_d - x_d) : +0.0f as a select on the bits, d_i = r.dot(r) in the Eigen packet order of the exact tile;
 * p_i = bmuHits[i] >= min_hits ? exp(-(double)d_i * d_i / 2) : 0 (node 0 is not exempt), C = ((0 + p_0) + p_1) + ... in node
 * order, in double; the draw is the smallest i whose running sum exceeds u * C, the largest i with p_i > 0 when rounding
 * leaves none, UINT64_MAX when C is 0 or not finite; prob is p_i / C.
 *   u_host[r1-r0], draw_out[r1-r0], norm_out[r1-r0], prob_out[(r1-r0)*N]   as vsom_bmd_batch's (each output may be NULL;
 *                                                                          u_host is required iff draw_out != NULL)
 *  - With an all-valid mask norm, prob and draw are bit-identical to vsom_bmd_batch's (the same operations on the same
 *    operands: derived, not measured).
 *  - What a row of the chunk or a model row holds at an invalid position (NaN, +-inf, 1e30) reaches no output.
 *  - A row without a valid column has d_i = +0 for every node: p_i = 1 on the nodes with enough hits, norm is their count,
 *    prob exactly 1 / count, and the draw is the floor(u * count)-th of them (counted from 0).
 *
 * vsom_generate_masked_batch produces draws = K >= 1 records per row:
 *   u_host[(r1-r0)*K]      uniforms in [0,1), entry (r - r0) * K + k belongs to draw k of row r, required
 *   l_host[(r1-r0)*K*J]    the L of vsom_generate_batch, entry ((r - r0) * K + k) * J + d, required; not validated
 *   out->unit[(r1-r0)*K], out->record[(r1-r0)*K*J]   row-major, the draw index inside the row index (each may be NULL)
 * Unit k of row r is what vsom_bmd_masked_batch draws for row r with the uniform u[(r - r0) * K + k] (the same device
 * functions on the same distribution: the same bits); only the row's own distribution is used (no "as written" last-row rule).
 * Column d of that record: with keep_observed != 0 and the column valid for row r it is (double)x[r][d], the staged value
 * -- a select: L there has no effect, a NaN included --; otherwise vsom_generate_batch's decode around the unit, operation for
 * operation (q = L / (1 - L); g = log(q); z = g / 1.6; t = z * (double)s; rec = t + (double)m), with that call's accuracy
 * statement.  A draw without mass has unit UINT64_MAX and the quiet NaN 0x7FF8000000000000 in EVERY column of its record, the
 * observed ones included.  With keep_observed = 0, draws = 1 and an all-valid mask unit and record are bit-identical to
 * vsom_generate_batch(VSOM_GENERATE_PER_ROW).
 *
 * Read-only: map, sigmaMap, S, weightMap, bmuHits, lastBMU, sqres and the chunk are untouched; vsom_generate_masked_batch
 * reads sigmaMap, so a pending one is materialised.  Both refuse (VSOM_ERR_INVALID, nothing enqueued, the context stays
 * usable): a null context or valid_host, custom and CLR contexts (the CLR residual runs over column pairs), no chunk, a chunk
 * staged ahead, r0 > r1 or r1 > B, a uniform that is NaN or outside [0,1); vsom_bmd_masked_batch: draw_out without u_host;
 * vsom_generate_masked_batch: a null out, u_host or l_host, draws = 0, draws > 65535.  An empty range returns VSOM_OK and
 * enqueues nothing.  Device scratch, in the query arena: the rows are taken in slices that respect three budgets (one row
 * where a single row needs more) -- the node-major p of a slice within 256 MiB (8 N bytes per row), vsom_bmu_masked_batch's
 * 64 MiB rule for the validity bytes (J + roundup(J, 32) per row; one row of each with one_mask, uploaded and packed once), and
 * for generate the slice's L and record within 64 MiB each (8 K J bytes per row) plus 16 K bytes of uniforms and units per
 * row.  VSOM_MASKED_SLICE_ROWS and (generate) VSOM_GENERATE_SLICE_ROWS, read at every call, cap the rows of a slice.  The tile,
 * the row pass and the draws are timed under VSOM_T_BMU, the decode under VSOM_T_FINISH. */
int vsom_bmd_masked_batch(vsom_ctx *ctx, uint64_t min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask,
                          const double *u_host, uint64_t *draw_out, double *norm_out, double *prob_out);
int vsom_generate_masked_batch(vsom_ctx *ctx, uint64_t min_hits, size_t r0, size_t r1, const uint8_t *valid_host, int one_mask,
                               uint32_t draws, int keep_observed, const double *u_host, const double *l_host,
                               vsom_generate_out *out);
/* The k best matching units of chunk rows [r0, r1) over their VALID columns only -- vsom_bmu_topk_batch for records with
 * missing fields: the runner-up for the topographic error of a map trained on such records, and an imputation blended
 * from k units.  Standard and Median (D = J).  One call, one stream wait.
 * Mask: exactly vsom_bmu_masked_batch's -- valid_host is (r1-r0) x J bytes, row-major, when one_mask == 0, and J bytes
 * applied to every row when one_mask != 0; a non-zero byte means valid; required.
 * Distance: r_d = valid ? (m_d - x_d) : +0.0f as a select on the bits, d_i = r.dot(r) in the Eigen packet order of the exact
 * tile: what a row or a model row holds at an invalid position (NaN, +-inf, 1e30) reaches no idx, dist, count or nvalid.
 * Candidates: node 0 always (it seeds Som::findRestrictedBmu whatever its hits) and every node with bmuHits >= min_hits;
 * bit-identical model rows each appear, in index order.
 * Order: the key (d_i, i) with NaN after +inf, so ties go to the lower index, and vsom_bmu_topk_batch's node-0 rule: when
 * d_0 is NaN, node 0 is entry 0 and the others follow in key order.  Entry 0 is therefore, bit for bit, the (bmu, dist) of
 * vsom_bmu_masked_batch for the same min_hits and mask.  A NaN distance is stored as 0x7FC00000.  With an all-valid mask
 * and min_hits = 0, idx and dist are bit-identical to vsom_bmu_topk_batch's.
 * Padding: a row with fewer than k candidates has count < k, and idx = UINT64_MAX, dist = 0x7FC00000 from entry count on
 * (k itself is only checked against N).  A row without a valid column has every distance +0: its list is the first count
 * candidates in index order and nvalid is 0.
 * Outputs (host pointers; entry r - r0 belongs to row r):
 *   idx[(r1-r0)*k]     row-major, required
 *   dist[(r1-r0)*k]    d of each idx entry, bit for bit (may be NULL)
 *   count[r1-r0]       real entries of the row: min(k, candidates) (may be NULL)
 *   nvalid[r1-r0]      valid columns of the row, as vsom_bmu_masked_batch (may be NULL)
 *   blend[(r1-r0)*J]   the record imputed from the k units, weighted as the BMD weights units (may be NULL).  In double,
 *                      one rounding per operation, nothing contracted: for the real entries j in list order
 *                      a_j = (double)d_j * (double)d_j; t = the a of the first entry whose distance is not NaN; the row has
 *                      mass iff that entry exists and its distance is finite; q_j = exp(-(a_j - t) / 2) for a finite d_j and
 *                      0 for a NaN or +inf one; terms with q_j == 0 are skipped, not multiplied;
 *                      Q = ((0 + q_0) + q_1) + ..., num_d = ((0 + q_0 * (double)m[0][d]) + q_1 * (double)m[1][d]) + ...
 *                      A valid column is (double)x of the staged row, by select (a NaN stays, the model does not matter);
 *                      an invalid one is num_d / Q, and the quiet NaN 0x7FF8000000000000 where the row has no mass.  exp
 *                      runs on the device (within an ulp of libm's), as vsom_bmd_batch's.  blend reads map only.
 * Read-only: map, sigmaMap, S, weightMap, bmuHits, lastBMU, sqres and the chunk are untouched; a pending sigmaMap stays
 * pending.  Refuses (VSOM_ERR_INVALID, nothing enqueued, the context stays usable): a null context, out, out->idx or
 * valid_host, custom and CLR contexts (the CLR residual runs over column pairs), no chunk, a chunk staged ahead, r0 > r1
 * or r1 > B, k = 0, k > 64, k > N.  An empty range returns VSOM_OK and enqueues nothing.  Device scratch, in the query
 * arena: the rows are taken in slices of at most the smallest of vsom_bmu_topk_batch's 64 MiB / (512 k) rows,
 * vsom_bmu_masked_batch's 64 MiB rule for the validity bytes (VSOM_MASKED_SLICE_ROWS, read at every call, caps it) and,
 * with blend, 64 MiB / (8 J) rows -- one row where a single row needs more.  Tile and merge are timed under VSOM_T_BMU,
 * the blend under VSOM_T_FINISH. */
typedef struct vsom_topk_masked_out {
    uint64_t *idx;
    float *dist;
    uint32_t *count;
    uint32_t *nvalid;
    double *blend;
} vsom_topk_masked_out;
int vsom_bmu_topk_masked_batch(vsom_ctx *ctx, uint32_t k, uint64_t min_hits, size_t r0, size_t r1,
                               const uint8_t *valid_host, int one_mask, vsom_topk_masked_out *out);
/* Som::euclidianWeightedDistRaw(pos, v, ones, ones) (Som.cpp:143-157) for `count` pairs; v is
 * chunk row vrows[i] (from_map = 0) or model vector vrows[i] (from_map = 1, the U-matrix case). */
int vsom_distances_raw(vsom_ctx *ctx, const uint64_t *nodes_host, const uint64_t *vrows_host,
                       size_t count, int from_map, float *dist_out_host);
/* Som::updateUMatrix (Som.cpp:999-1111) of the context's current map and sigmaMap, on the context's stream: one stencil
 * launch, nothing uploaded.  U[n] = the mean of euclidianWeightedDistRaw(n, map[m]) (the fp32 distance of
 * vsom_distances_raw with from_map = 1) over the 3 / 5 / 8 in-grid neighbours m of node n, diagonals weighted 0.3,
 * combined in double in the reference's order of additions.
 * u_out_host[N] doubles; NULL: only enqueue (no wait) -- the result stays in the context's device buffer
 * (VSOM_BUF_UMATRIX) and vsom_get_umatrix returns it later (the precedent is vsom_train_online_chunk / vsom_get_mse).
 * vsom_get_umatrix synchronises and returns the matrix of the state at the time of the last vsom_umatrix call (stream
 * order), not of later state.  Read-only: map, sigma, S, weight, bmuHits, lastBMU, sqres and the chunk are untouched; no
 * chunk is needed, and a chunk staged ahead does not matter.  Refuses (VSOM_ERR_INVALID, nothing enqueued, the context
 * stays usable): a null context, custom contexts, width < 2 or height < 2 (the reference indexes outside the map there),
 * vsom_get_umatrix before any vsom_umatrix on that context, a null u_out_host of vsom_get_umatrix. */
int vsom_umatrix(vsom_ctx *ctx, double *u_out_host);
int vsom_get_umatrix(vsom_ctx *ctx, double *u_out_host);

/* ---- batch epoch: Som::trainBatchSomEpoch (Som.cpp:756-879) ----------------------------
 * phase 1 (:762-806) over samples [s0,s1): BMU (findBmu when is_first else findLocalBmu)
 *   + per-sample ||residual||^2;  finish: bmuHits += 1, fp32 MSE in sample order;
 * phase 2 (:809-876) over nodes [n0,n1): new map, sigmaMap, weightMap rows.
 * vsom_batch_epoch = phase1(0,B) + finish + phase2(0,N); mse_out may be NULL.
 * The split entry points exist for node/sample sharding across GPUs (multi-GPU).*/
int vsom_batch_phase1_async(vsom_ctx *ctx, size_t s0, size_t s1, int is_first);
int vsom_batch_finish_async(vsom_ctx *ctx);
int vsom_batch_phase2_async(vsom_ctx *ctx, double sigma, size_t n0, size_t n1);
int vsom_batch_epoch_async(vsom_ctx *ctx, double sigma, int is_first);
int vsom_batch_epoch(vsom_ctx *ctx, double sigma, int is_first, float *mse_out);
/* Som::trainBatchSomEpoch over the VALID entries of the chunk only: the loaders store a missing field as 0.0f with
 * valid = 0 and the built-in Steppers drop valueWeight (Transformation.cpp:11-12,49-50), so vsom_batch_epoch takes every
 * missing field as a measured zero.  This call is the evident intent beside "as written", as vsom_bmu_masked_batch is for
 * the search.  Blocking, on the context's stream; Standard and Median (D = J), strict update mode only.
 * valid_host: B x J bytes row-major, or J bytes applied to every row when one_mask != 0; a non-zero byte means valid.  The
 * bytes travel with the call, nothing is kept between calls.  For the chunk's rows x_0 .. x_{B-1} in load order:
 *   phase 1 (:762-806) on the distance of vsom_bmu_masked_batch (r_d = valid[d] ? m_d - x_d : +0.0f, r.dot(r) over all J
 *     positions in the exact search's order): is_first != 0 the argmin of findBmu over all nodes (vsom_bmu_masked_batch
 *     with min_hits = 0), else findLocalBmu's walk (Som.cpp:335-454) from lastBMU[r], every distance the masked one.
 *     lastBMU[r] = the unit, sqres[r] = its masked distance; bmuHits and the MSE come from the unchanged finish step.
 *   phase 2 (:809-876) column by column: for node i and column d the rows are walked in load order and every row that
 *     is invalid at d is skipped; for a valid row w = (float)h(i, lastBMU[j], sigma), W_d += w, delta = Stepper(x_jd, M_d),
 *     M_d = M_d + (w / W_d) * delta, S_d = S_d + (w * delta) * delta -- the float operations of the unmasked chain, unfused,
 *     the division correctly rounded; map[i][d] = M_d, sigmaMap[i][d] = sqrt(S_d / W_d).  Column d of the result is column
 *     d of the unmasked phase 2 run over the rows valid at d with those rows' units.  What x holds at an invalid position
 *     (NaN, inf, anything) has no effect; a column without a valid row gives map = +0, sigmaMap = NaN (sqrt(0/0), literally);
 *     weightMap[i] is the sum of w over all B rows, as in vsom_batch_epoch; S is untouched.
 * With an all-valid mask (per row or one_mask) map, sigmaMap, weightMap, bmuHits, lastBMU, sqres and the MSE are
 * bit-identical to vsom_batch_epoch on the same state, chunk and lastBMU.  An empty chunk behaves as in vsom_batch_epoch.
 * Refuses (VSOM_ERR_INVALID, nothing enqueued, the state untouched, the context stays usable): a null context, valid_host
 * or mse_out, custom and CLR contexts, no chunk, a chunk staged ahead, an update mode other than VSOM_UPDATE_STRICT.
 * Timed under VSOM_T_STAGE (validity packing), VSOM_T_BMU, VSOM_T_FINISH, VSOM_T_CW, VSOM_T_UPDATE (the masked chains too)
 * and VSOM_T_SIGMA.  Device scratch: B (J + roundup(J, 32)) validity bytes (one row of each with one_mask), J ceil(B/32)
 * words of (column, row) bits, 8 B bytes of BMU coordinates, 4 J bytes of column list and the search's slice scratch. */
int vsom_batch_epoch_masked(vsom_ctx *ctx, double sigma, int is_first, const uint8_t *valid_host, int one_mask,
                            float *mse_out);
/* [MI355X build; Som::trainBatchSom restarts every node's chain with every chunk (Som.cpp:843,870), so after a pass over a
 * data set that loads in K chunks the map is the batch map of the LAST chunk alone]
 * A batch epoch over ALL rows of a data set that loads in several chunks.  Call order:
 *     vsom_batch_accum_begin(ctx, sigma, is_first, total_rows)
 *     for every chunk k = 0 .. K-1 of B_k rows, sum B_k = total_rows:
 *         load it (any staging call), optionally vsom_set_last_bmu (a load zeroes lastBMU), vsom_batch_accum_chunk(ctx)
 *     vsom_batch_accum_end(ctx, &mse)
 * The result equals, bit for bit, vsom_batch_epoch on the state at begin with the concatenated rows as ONE chunk and the
 * concatenated lastBMU: per node the reference's chain is a sequential walk over the rows in load order that carries W, M_d
 * and S_d; the walk is cut at the chunk borders and the three values are carried in buffers of the context.
 *   begin   opens the epoch; the accumulators (2 N pitch + N floats, allocated once and kept) start at zero.  map, sigmaMap,
 *           weightMap and S are untouched until end.
 *   chunk   enqueues and does not block, like vsom_batch_epoch_async.  Phase 1 as vsom_batch_phase1_async(0, B, is_first)
 *           against map, which still holds the epoch-start values: lastBMU and sqres of the chunk as phase 1 leaves them,
 *           bmuHits incremented per row; the MSE word continues in sample order, mse = mse + sqres[s] / (float)total_rows.
 *           Phase 2 for every node i and the chunk's rows j in load order: w = (float)h(i, lastBMU[j], sigma),
 *           accW = accW + w, c = w / accW (correctly rounded, 0/0 -> NaN), and for every column d
 *           delta = Stepper(x_jd, accM_d), accM_d = accM_d + c * delta, accS_d = accS_d + (w * delta) * delta -- the float
 *           operations of the epoch's chain, unfused.  Standard and Median (D = J).  A chunk of 0 rows changes nothing.  The
 *           chains read the staged rows: a vsom_prefetch_chunk behind it copies beside it and stages at vsom_commit_chunk.
 *   end     blocks.  map = accM, sigmaMap = sqrt(accS / accW), weightMap = accW, pad columns as every epoch leaves them; S
 *           is untouched; vsom_device_ptr values stay the same.  mse_out (may be NULL) and vsom_get_mse afterwards: the
 *           running MSE.  With total_rows = 0 the state is that of vsom_batch_epoch on an empty chunk (map +0, sigmaMap NaN,
 *           weightMap 0).  Closes the epoch.
 *   abort   closes the epoch: map, sigmaMap, weightMap and S are what they were at begin.  bmuHits, lastBMU, sqres and the
 *           MSE word keep what the chunk calls did to them.
 * Between begin and end the staging calls (upload, _async, set_chunk_device, prefetch, commit, set / get_last_bmu, get_sqres)
 * and read-only queries are legal; the queries see the epoch-start map.  A call that rewrites the model state in between
 * (vsom_set_state, any other training call) is not refused, but the epoch is then no epoch of the reference: each chunk
 * searches the map current at its call and end overwrites the state.  The accumulators are not reachable by other calls.
 * Refuses (VSOM_ERR_INVALID, nothing enqueued, the state untouched, the context stays usable): every call a null context;
 * begin while an epoch is open, custom and CLR contexts, an update mode other than VSOM_UPDATE_STRICT, a context that has
 * joined a group or an ensemble; chunk, end and abort when no epoch is open; chunk when no chunk is loaded, with a chunk
 * staged ahead over the current rows, or when the rows so far plus B exceed total_rows; end while the rows accumulated
 * differ from total_rows (the epoch stays open: add the missing chunk or abort).
 * Timed under VSOM_T_BMU (phase 1), VSOM_T_FINISH (MSE and hits), VSOM_T_CW (carried neighbourhood pass), VSOM_T_UPDATE
 * (carried chains) and VSOM_T_SIGMA (end).  Device scratch per chunk: 8 B roundup(N, 64) bytes of (c, w) and 8 B bytes of
 * BMU coordinates in the query arena.  Out of scope: CLR and custom contexts, the contracted update modes, groups and
 * ensembles, a deferred sigmaMap. */
int vsom_batch_accum_begin(vsom_ctx *ctx, double sigma, int is_first, size_t total_rows);
int vsom_batch_accum_chunk(vsom_ctx *ctx);
int vsom_batch_accum_end(vsom_ctx *ctx, float *mse_out);
int vsom_batch_accum_abort(vsom_ctx *ctx);
/* The chunk call of an accumulated epoch over the VALID entries of the chunk only: legal wherever
 * vsom_batch_accum_chunk is, in any mix with it, refused for the same reasons and for a null valid_host.  valid_host and
 * one_mask as in vsom_batch_epoch_masked: B x J bytes, nonzero = valid, or with one_mask one row of J bytes applied to every
 * row of the chunk.  It is not read after the call returns (it is copied into pinned memory of the context); the call
 * enqueues and does not wait for the stream.
 * begin, K chunk calls (masked or plain; a plain chunk counts as all valid) and end leave, bit for bit (NaN == NaN), what
 * vsom_batch_epoch_masked leaves on the state at begin with the concatenated rows as ONE chunk, the concatenated validity
 * and the concatenated lastBMU: map, sigmaMap, weightMap, bmuHits, every chunk's lastBMU and sqres, the MSE.
 *   Phase 1 as in vsom_batch_epoch_masked (the masked tile walk when is_first, the masked local walk from lastBMU otherwise)
 *   against map, which keeps its epoch-start values; hits and the running MSE as for vsom_batch_accum_chunk.
 *   Phase 2: for node i and column d the rows are walked in load order across all chunks; a row invalid at d is skipped, a
 *   valid one does  w = (float)h(i, lastBMU[j], sigma), W_d = W_d + w, delta = Stepper(x, M_d), M_d = M_d + (w / W_d) * delta,
 *   S_d = S_d + (w * delta) * delta  (unfused, a correctly rounded division).  A column that had an invalid entry in some
 *   chunk of the epoch carries M_d, S_d and W_d in side buffers of the context (3 J roundup(N, 64) floats, allocated by the
 *   first masked chunk and kept); every other column is the unmasked epoch's.  What x holds at an invalid position (NaN,
 *   inf) has no effect on any output.
 *   end: map = M_d, sigmaMap = sqrt(S_d / W_d), weightMap = the sum of w over ALL rows; a column without a valid row in the
 *   whole epoch is +0 / NaN.  abort restores as it does for plain chunks.
 * A plain vsom_batch_accum_chunk in an epoch that has had a masked chunk also walks the columns that were dirty so far, with
 * every entry valid; in an epoch without a masked chunk its launches and results are unchanged.
 * Timed under VSOM_T_STAGE (validity staging, bits, dirty columns), VSOM_T_BMU, VSOM_T_FINISH, VSOM_T_CW, VSOM_T_UPDATE (the
 * masked chains too) and VSOM_T_SIGMA.  Device scratch per masked chunk in the query arena: that of vsom_batch_accum_chunk
 * and of vsom_batch_epoch_masked; pinned: 2 B J validity bytes (two halves used alternately). */
int vsom_batch_accum_chunk_masked(vsom_ctx *ctx, const uint8_t *valid_host, int one_mask);
/* MSE of the last finish / online chunk (synchronises) */
int vsom_get_mse(vsom_ctx *ctx, float *mse_out);
/* A whole batch schedule on the chunk currently loaded, in one call.  The result is, bit for bit,
 * that of
 *     for ep in 0 .. epochs-1:
 *         if ep > 0 and reset_bmu: lastBMU := 0            (the reference's per-epoch reload, DataSet.cpp:136-137)
 *         batch_epoch(ctx, sigma[ep], ep == 0, &mse_out[ep])
 * so epoch 0 runs findBmu and the later ones findLocalBmu from lastBMU; reset_bmu = 1 is trainBatchSom on a one-chunk data
 * set, reset_bmu = 0 carries every row's BMU into the next epoch's walk.  The caller supplies every sigma (the stop rule
 * sigma < 1 of Som.cpp:729-730 belongs to the mirrors); sigma <= 1 is legal (the 1/0 table).  Map, sigmaMap, weightMap,
 * bmuHits (accumulated over all epochs), lastBMU, sqres, the MSE word and the context's bookkeeping end as after the last
 * call of that sequence; S is untouched; the neighbourhood table cached by the single-epoch calls is left alone.
 * Where the single epoch takes the one-launch kernel of a tiny map (not custom, not VSOM_NO_TINY=1) and every sigma is
 * finite, one launch runs up to VSOM_SCHEDULE_MAX_EPOCHS epochs (longer schedules: successive launches, each with the
 * tables of its own epochs); every other
 * context runs the sequence above inside the library.  epochs = 0: nothing is done (VSOM_OK).  The call blocks.
 * Refuses (VSOM_ERR_INVALID, nothing enqueued, state untouched): a null context; with epochs > 0 a null sigma or mse_out,
 * no chunk loaded, the next chunk staged ahead over the current chunk's rows (custom contexts included). */
#define VSOM_SCHEDULE_MAX_EPOCHS 1024
int vsom_batch_schedule(vsom_ctx *ctx, const double *sigma, size_t epochs, int reset_bmu, float *mse_out /*[epochs]*/);
/* vsom_batch_schedule over the VALID entries of the chunk only: bit for bit the loop above with
 *     vsom_batch_epoch_masked(ctx, sigma[ep], ep == 0, valid_host, one_mask, &mse_out[ep])
 * in place of batch_epoch -- map, sigmaMap, weightMap, bmuHits, lastBMU, sqres, every MSE, the MSE word and the context's
 * bookkeeping; S is untouched.  The same validity (valid_host / one_mask as in vsom_batch_epoch_masked) applies to every
 * epoch; it is copied to the device once per call and not read after the call returns.  Where
 * vsom_masked_tiny_applies(ctx, one_mask) holds and every sigma is finite, one launch of the one-workgroup masked kernel
 * runs up to VSOM_SCHEDULE_MAX_EPOCHS epochs (longer schedules: successive launches); every other context runs the loop
 * inside the library.  epochs = 0: nothing is done (VSOM_OK).  The call blocks.  Refuses (VSOM_ERR_INVALID, nothing
 * enqueued, state untouched, the context stays usable) what vsom_batch_schedule refuses, a null valid_host, and what
 * vsom_batch_epoch_masked refuses: custom and CLR contexts, an update mode other than VSOM_UPDATE_STRICT. */
int vsom_batch_schedule_masked(vsom_ctx *ctx, const double *sigma, size_t epochs, int reset_bmu, const uint8_t *valid_host,
                               int one_mask, float *mse_out /*[epochs]*/);
/* 1: a masked schedule on the loaded chunk would take the one-workgroup masked kernel (finite sigmas given) -- the chunk
 * and map are within the one-launch bounds of vsom_batch_epoch (not VSOM_NO_TINY=1), the context is Standard or Median,
 * not custom, in the strict update mode, and the kernel's LDS need (per-row arrays, the rows when B J <= 10240, the
 * neighbourhood table, J ceil(B/32) validity words -- J with one_mask) is within 64 KiB.  0 otherwise. */
int vsom_masked_tiny_applies(const vsom_ctx *ctx, int one_mask);

/* ---- online path -----------------------------------------------------------------------
 * Som::trainSingle (Som.cpp:885-947) on one host vector; residual_out has
 * vsom_residual_len() floats (may be NULL).  *last_bmu in/out.                            */
uint32_t vsom_residual_len(const vsom_ctx *ctx);
int vsom_train_single(vsom_ctx *ctx, const float *v_host, double eta, double sigma,
                      uint64_t *last_bmu, int decay_fn, float *residual_out,
                      float *dist_out, uint64_t *bmu_out);
/* inner loop of Som::trainBasicSom over the staged chunk (Som.cpp:1159-1171): B sequential
 * trainSingle steps + addBmu (:1189-1192) + MSE, without leaving the device.  With mse_out =
 * NULL the call only enqueues (asynchronous); vsom_get_mse then returns the chunk's MSE.     */
int vsom_train_online_chunk(vsom_ctx *ctx, double eta, double sigma, int decay_fn,
                            float *mse_out);
/* The same with the epoch's MSE accumulator carried over: the reference keeps ONE running float over
 * all chunks of an epoch (declared before the chunk loop, Som.cpp:1153; every sample adds its
 * squaredNorm/epochSize, :1167).  first_chunk != 0 starts it at 0, otherwise it continues from the
 * previous chunk; mse_out / vsom_get_mse give the running value after this chunk.
 * vsom_train_online_chunk = first_chunk 1. */
int vsom_train_online_chunk_acc(vsom_ctx *ctx, double eta, double sigma, int decay_fn, int first_chunk,
                                float *mse_out);
/* The same as ONE synchronising call that also hands back what Som::trainBasicSom reads after the sample loop of an
 * epoch's last chunk: the chunk's lastBMU (trainSingle writes data.getLastBMU(s) as it goes, Som.cpp:895,1163) and the
 * running MSE (:1167,1175).  lastbmu_out: B values (NULL: not wanted); mse_out: the running value after this chunk
 * (NULL: not wanted).  Equivalent to vsom_train_online_chunk_acc(..., NULL) + vsom_get_last_bmu + vsom_get_mse; on
 * maps small enough for the one-launch chunk kernel the results come back through pinned memory the kernel itself
 * stores into -- one launch and one stream wait per chunk (the reference's own 10 x 10 x 9 scenario). */
int vsom_train_online_chunk_fetch(vsom_ctx *ctx, double eta, double sigma, int decay_fn, int first_chunk,
                                  uint64_t *lastbmu_out, float *mse_out);
/* vsom_train_online_chunk_fetch over the VALID entries of the rows only: blocking, one stream wait,
 * on the context's stream.  valid_host and one_mask as in vsom_batch_epoch_masked: B x J bytes row-major, nonzero = valid, or
 * with one_mask one row of J bytes applied to every row.  The bytes travel with the call; nothing is kept between calls.
 * Standard and Median only (D = J).  For the staged rows x_0 .. x_{B-1} in load order, each with its validity row v_j, B
 * sequential steps, each on the state the previous one left:
 *   Search: the distance of vsom_bmu_masked_batch, r_d = v_j[d] ? m_d - x_d : +0, r.dot(r) over all J positions in the Eigen
 *   packet order of the unmasked distance.  sigma > 1: findBmu's argmin over all nodes, strict < from node 0 (the lowest
 *   index wins a tie, a NaN d_0 keeps node 0); sigma <= 1: findLocalBmu's walk from lastBMU[j] (Som.cpp:335-454) with every
 *   distance the masked one.  lastBMU[j] = bmu.
 *   Window (Som.cpp:899-944): for every window node n, weightMap[n] and the scalars of the step (scM, tw, twf) are exactly
 *   the unmasked step's -- the node's weight counts the sample whatever its columns.  A valid column d gets the unmasked
 *   step's float operations on map, SMap and sigmaMap (unfused); at an invalid column none of the three is written: the
 *   bits there, NaN included, stay as they were.
 *   Post (:946, :1165-1167): dist = the masked distance of x_j to the updated BMU row, mse = mse + dist / (float)B,
 *   bmuHits[bmu] += 1.  first_chunk starts or continues the running MSE as in vsom_train_online_chunk_acc.
 * Guarantees:
 *   With an all-valid mask (per row or one_mask) map, SMap, sigmaMap, weightMap, bmuHits, lastBMU and the MSE are
 *   bit-identical to vsom_train_online_chunk_fetch on the same state and chunk.
 *   What x holds at an invalid position (NaN, inf, anything) has no effect on any output.
 *   A row without a valid column has every distance +0: its BMU is node 0 (sigma > 1) or lastBMU[j] (sigma <= 1), its
 *   distance 0, and only weightMap and bmuHits move.
 *   Known bias, not solved here: weightMap is per node, so InverseProportional's step h / weightMap[n] and the denominator
 *   of sigmaMap count samples that were invalid at column d (per-column online weights would be a new N x D state array).
 * Refuses (VSOM_ERR_INVALID, nothing enqueued, state untouched, the context stays usable): a null context or valid_host;
 * custom and CLR contexts; a decay_fn other than the two online ones; no chunk loaded; a chunk staged ahead over the
 * current rows; a context that has joined a group or an ensemble.  A pending sigmaMap is materialised first, as for the
 * unmasked chunk calls.  Two loops give these results, bit for bit the same.  A tiny map, where
 * vsom_online_masked_tiny_applies holds, takes the one-launch chunk of one workgroup (csrc/vsom_online_tiny.hip,
 * DESIGN.md section 4u): one H2D copy of the validity bytes and one launch per call, lastBMU and the MSE back through
 * pinned memory as in vsom_train_online_chunk_fetch.  Every other chunk takes the per-sample loop on the exact scan, for
 * every vsom_set_bmu_mode; the image-bounded search is never used, and vsom_get_online_search_stats counts the samples of
 * neither loop.
 * Timed under VSOM_T_STAGE (validity staging) and VSOM_T_ONLINE (the kernels).  Device scratch in the query arena:
 * B (J + chunk pitch) validity bytes, or one row of each with one_mask (the one-launch chunk: B J, or J); VSOM_ERR_NOMEM
 * leaves the state untouched. */
int vsom_train_online_chunk_masked(vsom_ctx *ctx, double eta, double sigma, int decay_fn, int first_chunk,
                                   const uint8_t *valid_host, int one_mask,
                                   uint64_t *lastbmu_out /*[B], may be NULL*/, float *mse_out /*may be NULL*/);
/* 1: vsom_train_online_chunk_masked(ctx, ., sigma, ., ., ., one_mask, ., .) would take the one-launch chunk.  That is: a
 * chunk is loaded; the kind is Standard or Median and not custom; N <= 1024, N D <= 4096, D <= 512, B <= 4096; sigma is no
 * NaN; the search mode is VSOM_BMU_AUTO (EXACT and SHORTLIST name the per-sample loop); VSOM_NO_TINY=1 was not set when the
 * context was created; and the kernel's LDS need -- the unmasked one-launch chunk's plus a block of 2048 validity bytes --
 * is within the 96 KiB its launch sets.  0 otherwise, a null context included.  No side effects. */
int vsom_online_masked_tiny_applies(const vsom_ctx *ctx, double sigma, int one_mask);
/* diagnostics of the chunk loop's image-bounded search (csrc/vsom_online_i8.hip; synchronises): out[0] = samples searched
 * through the image since the last reset, out[1] = nodes evaluated exactly for them (the candidates that survived the
 * bound), out[2] = refinement workgroups that had a candidate, out[3] = 0.  All zero while the exact scan is in use. */
int vsom_get_online_search_stats(vsom_ctx *ctx, uint64_t *out /*[4]*/, int reset);

/* ---- ensembles: many small maps uploaded, trained and scored by one call each ---------------
 * An ensemble is a set of existing contexts on one device; its calls give every member its rows
 * (vsom_ensemble_upload_chunks), train every member, each with its own parameters, or score every member's chunk
 * (vsom_ensemble_bmu_batch), and have the same effect, bit for bit, as the single-context call made on every member in turn (map, S, sigmaMap,
 * weightMap, bmuHits, lastBMU, the MSE, the running MSE across chunks).  Members whose single call takes the one-launch
 * kernel of a tiny map (online: the chunk kernel; batch: the epoch kernel) and whose LDS need fits the device run as one
 * launch per kernel instantiation, one workgroup per member; every other member (larger maps, CLR online, custom
 * contexts, VSOM_NO_TINY=1, non-AUTO search modes, sigma = NaN) is trained in the same call through its ordinary path.
 * Members stay ordinary contexts: upload their chunks, set and read their state and checkpoint them as usual between
 * ensemble calls.  Each member's work stays ordered on that member's stream.  Give all members ONE stream
 * (vsom_set_stream) for the fast form; members on different streams are joined with events (the same results).
 * Every call waits for its launches before it returns.  The one-launch members are not timed: vsom_get_timing of such a
 * member does not count ensemble calls (members on their ordinary path are timed as in their single call).
 * create refuses (VSOM_ERR_INVALID): no members, a null or repeated member, members on different devices, members of a
 * vsom_group.  A train call refuses (VSOM_ERR_INVALID, naming the member index, before anything is enqueued for any
 * member): a member without a chunk, a member whose next chunk is staged ahead over its rows (vsom_commit_chunk first),
 * and an online decay_fn other than Exponential / InverseProportional.  A refused call changes nothing.
 * Lifetime: a member must not be destroyed while an ensemble holds it; destroy the ensemble first.
 * Arrays are indexed by member (the order given to create).  online: lastbmu_out (NULL: none wanted) holds a pointer per
 * member, each NULL or room for that member's B values; mse_out (NULL: not wanted) gets each member's running MSE. */
typedef struct vsom_ensemble vsom_ensemble;
int vsom_ensemble_create(vsom_ensemble **out, vsom_ctx *const *members, size_t count);
void vsom_ensemble_destroy(vsom_ensemble *e);
size_t vsom_ensemble_size(const vsom_ensemble *e);
int vsom_ensemble_train_online_chunk_fetch(vsom_ensemble *e, const double *eta, const double *sigma, const int *decay_fn,
                                           int first_chunk, uint64_t *const *lastbmu_out, float *mse_out);
/* vsom_ensemble_train_online_chunk_fetch for members whose rows have missing fields.  valid_host[k]
 * is member k's validity (B_k x J_k bytes, or J_k bytes when one_mask[k] != 0; one_mask NULL: all 0) or NULL for a PLAIN
 * member, which is trained exactly as vsom_ensemble_train_online_chunk_fetch trains it (any kind of context).  Per masked
 * member the results are those of vsom_train_online_chunk_masked on a context that is no member, bit for bit.  Masked
 * members for which vsom_online_masked_tiny_applies holds and whose LDS need fits the device's limit run as one launch per
 * kernel instantiation, one workgroup per member; their validity bytes are gathered into one pinned image and copied to
 * the device once per call.  Every other masked member runs the single call's loop inside this call.  valid_host is not
 * read after the call returns.  Refuses (VSOM_ERR_INVALID, naming the member, before anything is enqueued for any member):
 * what vsom_ensemble_train_online_chunk_fetch refuses, a null valid_host array, and for a masked member a custom or CLR
 * context. */
int vsom_ensemble_train_online_chunk_masked(vsom_ensemble *e, const double *eta, const double *sigma, const int *decay_fn,
                                            int first_chunk, const uint8_t *const *valid_host /*[K]*/,
                                            const int *one_mask /*[K], NULL: all 0*/, uint64_t *const *lastbmu_out,
                                            float *mse_out);
int vsom_ensemble_batch_epoch(vsom_ensemble *e, const double *sigma, int is_first, float *mse_out);
/* vsom_batch_schedule for every member, each with its own schedule: sigma[k] / mse_out[k] hold epochs[k] values.  Per
 * member the result of vsom_batch_schedule(member k, sigma[k], epochs[k], reset_bmu, mse_out[k]).  Members on the fast
 * path of that call run as one launch per kind, one workgroup per member looping its own epochs; members whose schedules
 * name the same sigma on the same table shape share one table.  Every other member runs its sequence in the same call;
 * a member with epochs[k] = 0 is not touched.  Refuses (VSOM_ERR_INVALID, naming the member, before anything is enqueued
 * for any member): a null ensemble; a null epochs array; for a member with epochs[k] > 0 a null sigma, mse_out, sigma[k]
 * or mse_out[k], no chunk loaded, the next chunk staged ahead over its rows. */
int vsom_ensemble_batch_schedule(vsom_ensemble *e, const double *const *sigma /*[K][epochs[k]]*/, const size_t *epochs /*[K]*/,
                                 int reset_bmu, float *const *mse_out /*[K][epochs[k]]*/);
/* The two calls above for members whose rows have missing fields.  valid_host[k] is member k's
 * validity (B_k x J_k bytes, or J_k bytes when one_mask[k] != 0; one_mask NULL: all 0) or NULL for a PLAIN member.  Per
 * member, bit for bit: vsom_batch_epoch_masked / vsom_batch_schedule_masked with valid_host[k], one_mask[k] for a masked
 * member, vsom_batch_epoch / vsom_batch_schedule for a plain one (any kind of context).  Masked members for which
 * vsom_masked_tiny_applies holds (and, in the schedule form, whose sigmas are finite) run as one launch per kind, one
 * workgroup per member; their validity bytes are gathered into one pinned image and copied to the device once per launch.
 * Every other member runs its single call in the same call.  valid_host is not read after the call returns.  mse_out of
 * the epoch form may be NULL; a member with epochs[k] = 0 is not touched.  Refuses (VSOM_ERR_INVALID, naming the member,
 * before anything is enqueued for any member): what the unmasked forms refuse, a null valid_host array, and for a masked
 * member a custom or CLR context or an update mode other than VSOM_UPDATE_STRICT. */
int vsom_ensemble_batch_epoch_masked(vsom_ensemble *e, const double *sigma, int is_first,
                                     const uint8_t *const *valid_host /*[K]*/, const int *one_mask /*[K], NULL: all 0*/,
                                     float *mse_out);
int vsom_ensemble_batch_schedule_masked(vsom_ensemble *e, const double *const *sigma, const size_t *epochs, int reset_bmu,
                                        const uint8_t *const *valid_host, const int *one_mask, float *const *mse_out);
/* Every member's chunk from ONE host buffer.  Member k gets B[k] rows of its own row length J_k (the length
 * vsom_upload_chunk reads for that member), contiguous at x_host + offset[k] (offsets in floats).  Several members may
 * name the same rows (equal offsets: a sweep over one data set).  n_floats = the extent of x_host.  Afterwards every call
 * on every member gives, bit for bit, what it gives after vsom_upload_chunk(member, x_host + offset[k], B[k]) (wait = 1)
 * or vsom_upload_chunk_async (wait = 0).  The union of the members' ranges, gaps between them included, is copied to the
 * device once; the plain members' rows are staged by one launch, the others (a chunk that gets the column compaction,
 * CLR, no rows) by their single-context staging from that copy, custom members by their own upload.
 * wait = 1: returns when x_host may be reused.  wait = 0: x_host must be pinned (vsom_host_alloc) and stay unchanged
 * until a call that synchronises the members has returned (the contract of vsom_upload_chunk_async); work enqueued on a
 * member's stream afterwards runs behind the staging.  Refuses (VSOM_ERR_INVALID, naming the member, before anything is
 * enqueued): a null array, a null x_host with some B[k] > 0, offset[k] + B[k] * J_k > n_floats, B[k] > 0x7FFFFFFF.
 * Every member state the single upload accepts is accepted (a chunk staged ahead, a prefetched chunk not committed). */
int vsom_ensemble_upload_chunks(vsom_ensemble *e, const float *x_host, size_t n_floats, const size_t *offset,
                                const size_t *B, int wait);
/* Som::findBmu for every row of every member's staged chunk: per member exactly what vsom_bmu_batch returns and leaves
 * on the device (lastBMU, sqres: a later vsom_get_last_bmu, vsom_get_sqres or batch epoch with is_first = 0 sees the
 * same values).  Members whose map has N * part_len <= 4096 (part_len: D, or D / 2 for CLR) are searched by one launch
 * per kind, whatever their chunk size and search settings; larger maps and custom members run vsom_bmu_batch in the same
 * call.  idx_out / dist_out: NULL, or one pointer per member (NULL or room for that member's B values).  Refuses like
 * the train calls: a member without a chunk, a member whose next chunk is staged ahead over its rows. */
int vsom_ensemble_bmu_batch(vsom_ensemble *e, uint64_t *const *idx_out, float *const *dist_out);
/* The two queries of a map trained on records with missing fields, for every member in one call:
 * which unit matches a row's observed columns and what does it say about the others (vsom_bmu_masked_batch: bmu, dist,
 * nvalid, fill), and how far is the row from that unit in units of its sigma and which column is to blame
 * (vsom_similarity_masked_batch: the similarity words, nvalid, the dense delta).  valid_host[k] is member k's validity
 * (B_k x J_k bytes, row-major, or J_k bytes when one_mask[k] != 0; one_mask NULL: all 0; a non-zero byte means valid) or
 * NULL: that member is SKIPPED -- nothing is enqueued for it and out[k] is neither read nor written.  min_hits NULL: all 0;
 * num_sigmas holds one value per member, sigma_rule applies to all.  out[k] holds host pointers, each may be NULL.
 * Per member with a validity every output is, bit for bit, that of
 *   vsom_bmu_masked_batch(member k, min_hits[k], 0, B_k, valid_host[k], one_mask[k], &out[k])
 *   vsom_similarity_masked_batch(member k, min_hits[k], num_sigmas[k], sigma_rule, 0, B_k, valid_host[k], one_mask[k], &out[k])
 * made on a context that is no member -- the arithmetic, the argmin rule and the edge cases stated at those calls hold
 * word for word: node 0 seeds the search whatever its hits, strict `<` over the nodes with bmuHits >= min_hits, NaN never
 * wins, a NaN d_0 pins node 0 and stores 0x7FC00000, a row without a valid column reports node 0, distance +0, nvalid 0 and
 * the similarity defaults given there; what x, map and sigmaMap hold at an invalid position reaches no output but `fill`,
 * which copies the map by definition.  A member with B_k = 0 writes nothing.
 * Members with a validity, B_k > 0, N * D <= 4096 and an LDS need (768 bytes + 4 N D) within the device's limit run as one
 * launch per kind (Standard, Median), one workgroup per (member, 64 rows), whatever their search settings: the search of
 * vsom_ensemble_bmu_batch on the masked distance and, in the same workgroup, the per-row epilogue (nvalid, fill, the
 * similarity words by the code vsom_similarity_masked_batch runs).  Their validity bytes are gathered into one pinned
 * image and copied to the device once per call, and their results return through pinned buffers of the ensemble (grow-only,
 * one set for both calls; B_k x J_k floats of fill / delta only for the members that ask for them).  Every other member
 * with a validity runs its single call inside this call, while the launches are in flight.  Each call ends in one wait
 * for the launches; valid_host is not read after the call returns.
 * Read-only: every member's lastBMU, sqres, map, sigmaMap, S, weightMap, bmuHits and chunk are untouched.  A member has
 * no pending sigmaMap to materialise: vsom_ensemble_create materialises one and a member's epochs are eager from then on
 * (vsom_set_sigma_mode), so sigmaMap is current when these calls read it; the entry gate that would materialise one is
 * the single calls' all the same.
 * Refuses (VSOM_ERR_INVALID, naming the member, before anything is enqueued for any member; a refused call changes nothing):
 * a null ensemble, valid_host array or out array; similarity: a null num_sigmas, an unknown sigma_rule; for a member with
 * a validity: a custom or CLR context, no chunk, the next chunk staged ahead over its rows. */
int vsom_ensemble_bmu_masked_batch(vsom_ensemble *e, const uint64_t *min_hits /*[K], NULL: all 0*/,
                                   const uint8_t *const *valid_host /*[K]*/, const int *one_mask /*[K], NULL: all 0*/,
                                   const vsom_masked_out *out /*[K]*/);
int vsom_ensemble_similarity_masked_batch(vsom_ensemble *e, const uint64_t *min_hits, const int *num_sigmas /*[K]*/,
                                          int sigma_rule, const uint8_t *const *valid_host, const int *one_mask,
                                          const vsom_similarity_masked_out *out /*[K]*/);
/* The k best matching units of every row of every member in one call, over all columns (vsom_bmu_topk_batch per member) or
 * over the valid columns only (vsom_bmu_topk_masked_batch per member): the runner-up that the topographic error of every
 * map of a sweep needs.  k holds one value per member; out[m] holds member m's host pointers
 * (idx[B_m * k_m] row-major, required for a covered member; dist[B_m * k_m], count[B_m], nvalid[B_m] may be NULL; the
 * plain call ignores count and nvalid).  blend is out of scope for the ensemble calls -- the struct has no such field:
 * vsom_bmu_topk_masked_batch on the member gives it.
 * Plain call: covers every member with out[m].idx != NULL; a member with a NULL idx is SKIPPED -- nothing is enqueued for
 * it and out[m] is not written.  Standard, Median and CLR members are taken, as in vsom_ensemble_bmu_batch.  Per covered
 * member idx and dist are, bit for bit, those of
 *   vsom_bmu_topk_batch(member m, k[m], 0, B_m, idx, dist)
 * made on a context that is no member, and what is stated at that call holds word for word: nodes ordered by the key
 * (d_i, i) with NaN after +inf, every node a candidate, entry 0 findBmu's BMU -- node 0 with 0x7FC00000 when d_0 is NaN,
 * the others behind it in key order -- and a NaN distance stored as 0x7FC00000.
 * Masked call: covers every member with valid_host[m] != NULL (B_m x J_m bytes, row-major, or J_m bytes when
 * one_mask[m] != 0; one_mask NULL: all 0; a non-zero byte means valid); NULL: SKIPPED, as in
 * vsom_ensemble_bmu_masked_batch.  min_hits NULL: all 0.  Per covered member idx, dist, count and nvalid are, bit for
 * bit, those of
 *   vsom_bmu_topk_masked_batch(member m, k[m], min_hits[m], 0, B_m, valid_host[m], one_mask[m], ...)
 * and that call's contract holds unchanged: the candidates are node 0 and the nodes with bmuHits >= min_hits; a row with
 * fewer than k candidates has count < k and idx = UINT64_MAX, dist = 0x7FC00000 from entry count on; a row without a
 * valid column gets that call's list (the first count candidates in index order, every distance +0, nvalid 0); what x
 * and the map hold at an invalid position reaches no output.
 * Both: a member with B_m = 0 writes nothing.  Read-only: every member's lastBMU, sqres, map, sigmaMap, S, weightMap,
 * bmuHits and chunk are untouched.  valid_host is not read after the call returns.  Each call ends in one wait.
 * The fast path: a covered member that is not custom, with B_m > 0, k <= N, N * part_len <= 4096 (part_len: D, or D / 2
 * for CLR) and an LDS need of 512 + 512 (k | 1) + 4 N D bytes within min(the device's limit per workgroup, 64 KiB) runs
 * in one launch per kind of ensemble_topk_many_kernel, one workgroup per (member, 64 rows): the model rows in LDS, every
 * (row, node) distance by the 8-lane routine of vsom_ensemble_bmu_batch (masked: of vsom_ensemble_bmu_masked_batch),
 * each row's k smallest keys kept as a sorted list in LDS.  vsom_ensemble_topk_applies reports it.  The validity bytes of
 * those members travel as one pinned image, copied once per call, and their results return through the pinned buffers
 * of the masked queries.  Every other covered member runs its single call inside the same call, while the launches are
 * in flight.
 * Refuses (VSOM_ERR_INVALID, naming the member, before anything is enqueued for any member; a refused call changes
 * nothing): a null ensemble, k array or out array; masked: a null valid_host array; for a covered member: a null idx
 * (masked call), k = 0, k > 64, k > N, a custom context, no chunk, the next chunk staged ahead over its rows; masked: a
 * CLR context (the residual runs over column pairs). */
typedef struct vsom_ensemble_topk_out {   /* host pointers of ONE member; idx required, the others may be NULL */
    uint64_t *idx;      /* [B_k * k_k] row-major */
    float    *dist;     /* [B_k * k_k] */
    uint32_t *count;    /* [B_k]  masked call only; the plain call ignores it */
    uint32_t *nvalid;   /* [B_k]  masked call only; the plain call ignores it */
} vsom_ensemble_topk_out;
int vsom_ensemble_bmu_topk_batch(vsom_ensemble *e, const uint32_t *k /*[K]*/, const vsom_ensemble_topk_out *out /*[K]*/);
int vsom_ensemble_bmu_topk_masked_batch(vsom_ensemble *e, const uint32_t *k /*[K]*/,
                                        const uint64_t *min_hits /*[K], NULL: all 0*/,
                                        const uint8_t *const *valid_host /*[K]*/, const int *one_mask /*[K], NULL: all 0*/,
                                        const vsom_ensemble_topk_out *out /*[K]*/);
/* 1 when member `member` with that k would run in ensemble_topk_many_kernel (the fast path above, on its loaded chunk),
 * 0 when it would run its single call inside the ensemble call (or be refused); VSOM_ERR_INVALID for a null ensemble or
 * a member index out of range.  masked != 0: the masked call, which takes no CLR member. */
int vsom_ensemble_topk_applies(const vsom_ensemble *e, size_t member, uint32_t k, int masked);
/* Som::evaluate (Som.cpp:490-523), the validation loss, of every member on its own chunk in one call, over all columns
 * (vsom_evaluate_batch per member) or over the valid columns only (vsom_evaluate_masked_batch per member): the number a
 * sweep is ranked by.  binary_host[k] / continuous_host[k] hold member k's J_k column factors;
 * out[k] holds member k's host pointers, each of which may be NULL.
 * Plain call: covers every member with binary_host[k] != NULL -- every field of vsom_evaluate_out is optional, so the
 * column array is what names a covered member; a member with a NULL binary_host[k] is SKIPPED: nothing is enqueued for it
 * and out[k] is neither read nor written.  valid_host: NULL (every column of every member valid), or one entry per member:
 * NULL or B_k x J_k bytes.  Standard, Median and CLR members are taken.  Per covered member every output is, bit for bit,
 * that of
 *   vsom_evaluate_batch(member k, 0, B_k, binary_host[k], continuous_host[k], valid_host ? valid_host[k] : NULL, &out[k])
 * made on a context that is no member.  The call IS vsom_ensemble_bmu_batch's search for the covered members, as
 * vsom_evaluate_batch is vsom_bmu_batch: their lastBMU / sqres are left as that call leaves them.
 * Masked call: covers every member with valid_host[k] != NULL (B_k x J_k bytes, row-major, or J_k bytes when
 * one_mask[k] != 0; one_mask NULL: all 0; a non-zero byte means valid); NULL: SKIPPED, as in
 * vsom_ensemble_bmu_masked_batch.  min_hits NULL: all 0.  Per covered member every output is, bit for bit, that of
 *   vsom_evaluate_masked_batch(member k, min_hits[k], 0, B_k, binary_host[k], continuous_host[k], valid_host[k],
 *                              one_mask[k], &out[k])
 * Read-only: every member's lastBMU, sqres, map, sigmaMap, S, weightMap, bmuHits and chunk are untouched.
 * Both: what is stated at the two single calls holds word for word -- the search, the node-0 rule, the NaN rules, the
 * select at invalid columns, the -99999 replacement, bsum's packet order, the accuracy statement for log; bsum is the
 * same bits as the single call's because both kernels run one row body on the same logf.  *error is the running mean in
 * row order, evaluated on the host.  A member with B_k = 0 writes *error = 0 and nothing else.  The host arrays are not
 * read after the call returns.  Each call ends in one wait.
 * The fast path: the covered members with B_k > 0 that vsom_ensemble_bmu_batch (masked: vsom_ensemble_bmu_masked_batch)
 * searches in its one launch -- not custom, N * part_len <= 4096 (part_len: D, or D / 2 for CLR; masked: Standard / Median,
 * N * D <= 4096) and an LDS need of 768 + 4 N D bytes within min(the device's limit per workgroup, 64 KiB) -- run in one
 * launch per kind of ensemble_evaluate_many_kernel, one workgroup per (member, 64 rows): that search, and behind one
 * barrier the row scoring of vsom_evaluate_batch's kernel, eight lanes per row, against the unit's row in LDS.
 * vsom_ensemble_evaluate_applies reports it.  The column arrays (2 J_k floats) and the validity bytes of those members
 * travel as one pinned image, copied once per call; their results (5 words per row, masked 6) return through the pinned
 * buffers of the masked queries.  Every other covered member runs its single call inside the same call, while the
 * launches are in flight.
 * Refuses (VSOM_ERR_INVALID, naming the member, before anything is enqueued for any member; a refused call changes
 * nothing): a null ensemble, binary_host, continuous_host or out array; masked: a null valid_host array; for a covered
 * member: a null continuous_host[k] (masked: or binary_host[k]), a custom context, no chunk, the next chunk staged ahead
 * over its rows; masked: a CLR context (the residual runs over column pairs). */
int vsom_ensemble_evaluate_batch(vsom_ensemble *e, const float *const *binary_host /*[K][J_k]*/,
                                 const float *const *continuous_host /*[K][J_k]*/,
                                 const uint8_t *const *valid_host /*NULL, or [K]: NULL or B_k x J_k bytes*/,
                                 const vsom_evaluate_out *out /*[K]*/);
int vsom_ensemble_evaluate_masked_batch(vsom_ensemble *e, const uint64_t *min_hits /*[K], NULL: all 0*/,
                                        const float *const *binary_host, const float *const *continuous_host,
                                        const uint8_t *const *valid_host /*[K]*/, const int *one_mask /*[K], NULL: all 0*/,
                                        const vsom_evaluate_masked_out *out /*[K]*/);
/* 1 when member `member` would run in ensemble_evaluate_many_kernel (the fast path above, on its loaded chunk), 0 when it
 * would run its single call inside the ensemble call (or be refused); VSOM_ERR_INVALID for a null ensemble or a member
 * index out of range.  masked != 0: the masked call, which takes no CLR member. */
int vsom_ensemble_evaluate_applies(const vsom_ensemble *e, size_t member, int masked);
/* Som::updateUMatrix of every member: per member exactly what vsom_umatrix gives (also in the member's VSOM_BUF_UMATRIX
 * buffer: a later vsom_get_umatrix of the member returns it).  u_out: NULL, or one pointer per member (NULL entries
 * skipped, else room for that member's N doubles).  Members whose map has N * part_len <= 4096 are computed by one launch
 * per kind (plain / CLR), one workgroup per member; every other member runs vsom_umatrix in the same call.  The call waits
 * before it returns.  Refuses (VSOM_ERR_INVALID): a null ensemble, or naming the first member that vsom_umatrix would
 * refuse (a custom context, width < 2 or height < 2) -- before anything is enqueued for any member. */
int vsom_ensemble_umatrix(vsom_ensemble *e, double *const *u_out);

/* ---- multi-GPU batch epoch, one process, the GPUs of one node ------------------------
 * Som::trainBatchSomEpoch's two loops shard differently: phase 1 (Som.cpp:764-782 / 786-805) is
 * independent per SAMPLE, phase 2 (Som.cpp:809-876) is independent per NODE but sequential in samples
 * (the variance accumulator uses the prefix mean).  A group holds one context per device, each with
 * the whole map and the whole chunk; an epoch runs phase 1 on the device's samples, all-gathers
 * lastBMU / ||residual||^2, forms bmuHits and the MSE on every device, runs phase 2 on the device's
 * nodes and all-gathers the new map rows (sigmaMap / weightMap rows follow on a second stream behind the
 * next search).  Every device ends with the bit-identical state of the single-GPU epoch.
 * Transport: RCCL over xGMI (librccl is bound at run time; ncclCommInitAll over the devices);
 * VSOM_GROUP_TRANSPORT=peer, or a device list that repeats a device (rehearsal of the N > 1 flow on a
 * one-GPU box, which RCCL refuses), uses ordered peer copies instead.
 * devices = NULL means devices 0 .. ndev-1; ndev = 0 means every visible device.
 * vsom_group_ctx(g, r) exposes a member for the single-context calls (searches, getters): call
 * vsom_group_synchronize first, and write state only through vsom_group_set_state.               */
typedef struct vsom_group vsom_group;
int vsom_group_create(vsom_group **out, int ndev, const int *devices, uint32_t width, uint32_t height,
                      uint32_t in_len, int transform);
void vsom_group_destroy(vsom_group *g);
int vsom_group_size(const vsom_group *g);
vsom_ctx *vsom_group_ctx(vsom_group *g, int rank);
const char *vsom_group_transport(const vsom_group *g);   /* "rccl" or "peer" */
int vsom_group_synchronize(vsom_group *g);
int vsom_group_set_state(vsom_group *g, const float *map, const float *sigma, const float *S,
                         const float *weight, const uint64_t *bmu_hits);
int vsom_group_get_state(vsom_group *g, float *map, float *sigma, float *S, float *weight,
                         uint64_t *bmu_hits);
int vsom_group_set_update_mode(vsom_group *g, int mode);
int vsom_group_set_bmu_mode(vsom_group *g, int mode);
/* DataSet::loadNextDataFromStream for the group: every device copies ITS 1/n of the rows from the host
 * and the rest arrives by all-gather; upload = prefetch + commit + wait (same contract as the
 * single-context calls above) */
int vsom_group_upload_chunk(vsom_group *g, const float *x_host, size_t B);
int vsom_group_prefetch_chunk(vsom_group *g, const float *x_host, size_t B);
int vsom_group_prefetch_wait(vsom_group *g);
int vsom_group_commit_chunk(vsom_group *g);
/* DataSet::loadNextDataFromStream (DataSet.cpp:118-160) for a chunk already resident in HBM: rows_dev[r] = member r's own rows [B*r/n, B*(r+1)/n) on ITS
 * device; all-gather of the rows, staging, lastBMU := 0 -- asynchronous on the members' streams */
int vsom_group_set_chunk_device(vsom_group *g, const void *const *rows_dev /*[n]*/, size_t B);
int vsom_group_set_last_bmu(vsom_group *g, const uint64_t *in_host);
int vsom_group_get_last_bmu(vsom_group *g, uint64_t *out_host);
/* Som::trainBatchSomEpoch (Som.cpp:756-879) over the group */
int vsom_group_batch_epoch_async(vsom_group *g, double sigma, int is_first);
int vsom_group_batch_epoch(vsom_group *g, double sigma, int is_first, float *mse_out);
int vsom_group_get_mse(vsom_group *g, float *mse_out);

/* ---- static helper: Som::calculateNeighbourhoodWeight (Som.cpp:949-975) ---------------- */
double vsom_neighbourhood_weight(size_t cx, size_t cy, size_t bx, size_t by, double sigma);

/* ---- interop / measurement -------------------------------------------------------------*/
/* raw device pointer of a context buffer (for RCCL / torch.distributed collectives).  VSOM_BUF_SIGMA materialises a
 * pending sigmaMap, so the rows are current for work enqueued behind this call; a pointer KEPT across later whole-map
 * epochs is current again only after vsom_sigma_flush (or any call that materialises). */
void *vsom_device_ptr(vsom_ctx *ctx, int which);
size_t vsom_chunk_size(const vsom_ctx *ctx);
/* row pitch in floats of the MAP/SIGMA/S device buffers (>= D; CLR: [A | pad | B | pad]) and
 * of the staged CHUNK buffer */
uint32_t vsom_pitch(const vsom_ctx *ctx);
uint32_t vsom_chunk_pitch(const vsom_ctx *ctx);
/* 1 when phase 2 over a shard of `nodes` nodes takes the small-map chain kernel (lane = (node, dim pair),
   update_chain3_kernel) instead of the lane = node kernels -- for reports that name the dominant kernel */
int vsom_small_map_chains(const vsom_ctx *ctx, size_t nodes);
/* per-kernel-group HIP-event timing on the context stream */
int vsom_enable_timing(vsom_ctx *ctx, int on);
/* the same for the groups whose bit (1u << VSOM_T_*) is set only: every timed group puts two event records between
 * kernels that otherwise run back to back (~5 us of idle device each on this chip), so a measurement of a whole step
 * times the one group it needs */
int vsom_enable_timing_of(vsom_ctx *ctx, uint32_t group_mask);
/* accumulated milliseconds and launch counts since the last reset (synchronises) */
int vsom_get_timing(vsom_ctx *ctx, float *ms_out /*[VSOM_T_COUNT]*/,
                    uint32_t *count_out /*[VSOM_T_COUNT]*/, int reset);

#ifdef __cplusplus
}
#endif
#endif
