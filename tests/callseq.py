"""Seeded random walks over the single-context C ABI (include/vsom_hip.h), checked against the CPU oracle.

Imported by tests/test_gpu_call_sequences.py (the real library) and tests/test_call_sequences_model.py (fake contexts
backed by a second oracle, some of them wrong on purpose).  A walk is a list of ops -- plain tuples (name, params) that
print as Python literals -- whose first entry names the configuration and the seed; `replay(ops)` reruns a printed list.

The model is an oracle.pyoracle.OracleSom plus a record of what the header promises about the rest of the context: the
current chunk and its lastBMU, the pending (prefetched / device-staged) chunk, the last MSE and the online running
accumulator.  Every accepted call must return the model's values bit for bit (NaN == NaN); a call that reads the staged
rows while a chunk is pending may instead be refused (VSOM_ERR_INVALID naming the commit), which changes nothing.

Two profiles.  "ingest" is the walk over the chunk pipeline (uploads, prefetches, commits, epochs whole and split, online
chunks, searches).  "sigma" walks the pending sigmaMap (include/vsom_hip.h, vsom_set_sigma_mode): it sets a sigma mode,
adds the flush, the column compaction, whole-map phase-2 ranges, empty chunks, the masked epoch, partial vsom_set_state
calls, the sigmaMap readers and the arena queries, and holds by construction the runs in which a record stays pending
across a stage-ahead and its commit, a lastBMU write, a reallocating upload, an empty chunk, an online chunk enqueued
without a wait and a weight-only state write.  The model (SigmaRecord) restates the header's contract -- which calls leave
a record pending, when AUTO defers, what vsom_sigma_stats counts -- and the walk compares all four numbers of
vsom_sigma_stats after every accepted call; a refused call may have materialised the record or not, nothing else.  The
oracle state never depends on the mode.  The real backend drives a second context fixed at VSOM_SIGMA_EAGER through the
same calls: what the readers, the arena queries and the masked epoch return must equal that twin's output bit for bit
(doubles on 64 bits), and the twin's own state is compared with the oracle at the end.  The masked epoch's model is
tests/masked_train_ref.py (its phase 1 and phase 2) applied to the model's oracle state.

A third profile, "accum", walks the accumulated batch epoch (include/vsom_hip.h, vsom_batch_accum_begin / _chunk /
_chunk_masked / _end / _abort; DESIGN.md sections 4n, 4o): the one protocol of the C ABI whose state lives across calls
that do not block.  It keeps every op of the sigma profile, under a sigma mode, and adds the five calls, the two masked
scoring calls as row-window queries and an update-mode switch.  Epochs are generated whole (generate_accum); each walk holds,
between ("run", id) / ("run_end", id) markers the backends never see, these runs:
  1  no wait: begin(first), three masked chunks, each behind a load that does not synchronise and never the same rows
     twice in a row, end -- the third reuses the first pinned validity half; this epoch has a row without a valid column
     and a column without a valid row
  2  no wait: plain chunks of growing size, the configuration's largest last, one top-8 query between two of them -- the
     chunk buffers and the query arena grow behind enqueued work
  3  plain, masked, plain in a non-first epoch, vsom_set_last_bmu between each load and its chunk call
  4  abort behind two chunks or more, one masked; get_state; a plain epoch on the same context (the ever-dirty list is gone)
  5  epoch_async, prefetch, begin, a chunk call, commit, a chunk call, abort: where stages_ahead(cfg) the prefetch is
     staged ahead and the first chunk call MUST be refused, naming the commit (elsewhere it takes the old chunk)
  6  every refusal the header lists, each followed by a comparison of the whole state; the empty epoch; an empty chunk
  7  an epoch that leaves its sigmaMap pending (where the configuration defers), then begin
  8  vsom_set_state(map) and a single step at another sigma between two chunks; ended with end
  9  the masked scoring calls, the masked search, the BMD and a reader between two chunks
In runs 1-4 and 6-9 a call is refused only where the header says it must be; every refusal of one of the five calls,
run 5's included, is followed at once by a comparison of the whole state, lastBMU and the MSE word.  The model (Model._accum_*) keeps the epoch's
rows, validity and lastBMU and restates begin / chunk / end / abort from the oracle: phase 1 per chunk on the model's
current map (batch_phase1_range, or masked_train_ref.phase1), the running MSE in sample order over total_rows, phase 2 at end
over the concatenation -- the clean columns from one batch_phase2_range, every column that had an invalid entry from
masked_train_ref.phase2.  Masks are engineered (materialize): at most 16 dirty columns per epoch -- column 0, column J - 1,
columns 31 and 32, one column invalid in every masked chunk, and columns that turn dirty only in the epoch's second or
third masked chunk -- except in run 1, whose row without a valid column makes every column dirty.  The rows loaded for a
masked chunk call are made for that call (poisoned_rows; the load op carries the call's parameters): NaN / +-inf under
every invalid entry of its mask -- the border columns, the column invalid throughout, the columns that have just turned
dirty, the empty row -- and nowhere else.  The real backend drives a second context through the same calls, fed from
pageable memory, fixed at VSOM_SIGMA_EAGER and synchronised after every call: what the twin-compared calls return must equal
that sequential twin's output bit for bit.  Between two calls of a walk the twin makes its call and waits, and the model
runs its own (a Python masked search takes a second), so the first context's stream is as good as idle at every call:
call by call the walk tests the state logic, not the ordering.  The no-wait runs 1 and 2 are therefore issued back to back
on the first context (run_walk, back_to_back), with nothing between two calls but the calls' own host work, and only then
replayed on the twin and the model, each return held against them: there the third masked chunk does meet a busy stream,
and the buffers and the arena do grow behind enqueued work.  (Not on clr12 / custom12, where begin is refused, and not on
the CPU fake, which is sequential by nature.)

A fourth profile, "ensemble" (generate_ensemble, run_ensemble_walk, EnsGpuBackend, at the end of this file), walks the nine
vsom_ensemble_* calls with the single-context calls on their members between them -- among these vsom_batch_schedule,
vsom_batch_schedule_masked and vsom_train_online_chunk_masked, which enter the walks here.  Its members (ENS_MEMBERS, beside
CONFIGS) have row counts at the borders of the path predicates, restated as batch_tiny / masked_batch_tiny / online_tiny;
two ensemble configurations (ENS_CONFIGS) put them on one stream and on a stream each.  EnsModel keeps one Model per member:
an accepted ensemble call is the single call on every member in index order, every output compares bit for bit, a refused
call must name the member the header says and is followed by a comparison of the whole state of every member.  Masks are
accum_mask's, the rows of a masked member poisoned under every invalid entry; members without validity (valid_host[k] = NULL)
are in every masked call.  The real backend keeps a twin of every member that never joins and makes the single calls one by
one, synchronised after each: what an ensemble call returns must equal the twins' returns and the model's.  Where the header
gives a member another answer than a context that never joined (vsom_train_online_chunk_masked, vsom_batch_accum_begin), the
model says so: the member must refuse.  The walk's first no-wait run goes to the ensemble back to back before twins and model
see it; the pinned rows of a wait = 0 upload are overwritten once a call that synchronises every member has returned.

A fifth profile, "ensemble_query" (generate_ensemble_query, the last section of this file), walks the four ensemble calls
that return results through state shared across calls -- vsom_ensemble_bmu_masked_batch, _similarity_masked_batch,
_bmu_topk_batch, _bmu_topk_masked_batch, with vsom_ensemble_topk_applies -- between the ensemble profile's calls, and adds
the single-context vsom_similarity_masked_batch, vsom_bmu_topk_batch, vsom_bmu_topk_masked_batch, vsom_bmd_masked_batch and
vsom_generate_masked_batch on members.  Its members and configurations stand beside the ensemble profile's (ENSQ_MEMBERS,
ENSQ_CONFIGS), its path predicates beside batch_tiny (masked_query_fast, topk_fast).  run_ensemble_walk serves it: a query
changes nothing, so the model has nothing to apply; EnsModel.query computes what every covered member must return from the
member's oracle state and the plain references (masked_score_ref, topk_masked_ref), every row of the small members and a
seeded sample of the large ones; the real backend gives every output array a canary and a guard and holds every row to the
member's twin.  ensq_conditions asserts that a walk was not vacuous.
"""
import copy
import ctypes as C

import numpy as np

import gen
import masked_train_ref
import online_masked_ref
import schedule_ref
from oracle import pyoracle as po

VSOM_ERR_INVALID = -1
VSOM_ERR_UNSUPPORTED = -4
EXPONENTIAL, INVERSE_PROPORTIONAL = 0, 1
BMU_AUTO, BMU_EXACT, BMU_SHORTLIST = 0, 1, 2
SIGMA_AUTO, SIGMA_EAGER, SIGMA_LAZY = 0, 1, 2
SIGMA_MODES = {"auto": SIGMA_AUTO, "eager": SIGMA_EAGER, "lazy": SIGMA_LAZY}
NTHREADS = 16
VSOM_CHAIN_MAX_WAVES = 448           # csrc/vsom_internal.hpp

# configuration: map, transformation, chunks (size, kind); kinds: "u8" uint8-valued, "f" the same / 255, "dense" blobs,
# "clr" correlated columns
CONFIGS = {
    # (accum_chunks: further chunks of the accum profile alone, two of them short enough for the model's masked full
    # search, so that the masked chunks of run 1 follow each other with different rows)
    "std48": dict(W=48, H=48, J=196, tr=po.STANDARD, custom=False,
                  chunks=[(1100, "u8"), (1280, "f"), (77, "u8"), (1500, "dense"), (4500, "u8"), (1024, "f")],
                  accum_chunks=[(33, "u8"), (23, "f")]),
    # (sigma_weights: the sigma profile's draws alone.  Median's online scan and its masked search -- Python, a row of the
    # 300-row shortest chunk at a time -- are the model's dearest ops: drawn less often there)
    "med48": dict(W=48, H=48, J=196, tr=po.MEDIAN, custom=False,
                  chunks=[(1100, "u8"), (300, "dense"), (1536, "f"), (4500, "u8"), (1024, "u8")],
                  sigma_weights={"online": 1, "single": 1, "epoch_masked": 0.5}, accum_chunks=[(33, "dense"), (23, "u8")]),
    "std12": dict(W=12, H=12, J=24, tr=po.STANDARD, custom=False,
                  chunks=[(300, "dense"), (128, "dense"), (77, "dense"), (1500, "dense")]),
    "clr12": dict(W=12, H=12, J=6, tr=po.CLR, custom=False,
                  chunks=[(300, "clr"), (128, "clr"), (77, "clr"), (700, "clr")]),
    "custom12": dict(W=12, H=12, J=24, tr=po.STANDARD, custom=True,
                     chunks=[(200, "dense"), (64, "dense"), (301, "dense")]),
    # 100 node groups x 7 column blocks = 700 workgroups: a deferred whole-map launch takes the two-quad mean-only chains
    # (two_quad_launch below).  The online scan and the single step cost N x D per sample on the oracle: drawn less often.
    "std80": dict(W=80, H=80, J=196, tr=po.STANDARD, custom=False,
                  chunks=[(320, "u8"), (77, "u8"), (512, "f"), (200, "dense")], weights={"online": 2, "single": 1},
                  accum_chunks=[(40, "u8"), (12, "dense"), (11, "u8")]),
}

# ---- the ensemble profile: members (never a parametrisation of the other profiles) and ensemble configurations ----
# Every row count stands at a border of a path predicate (batch_tiny, online_tiny below).  A2 has A's shape and chunks, so
# chunk_data gives it A's rows: vsom_ensemble_upload_chunks names them by equal offsets.
ENS_MEMBERS = {
    "A": dict(W=10, H=10, J=9, tr=po.STANDARD, custom=False,
              chunks=[(20, "dense"), (160, "dense"), (170, "dense"), (257, "dense")]),
    "A2": dict(W=10, H=10, J=9, tr=po.STANDARD, custom=False, map_seed=100,
               chunks=[(20, "dense"), (160, "dense"), (170, "dense"), (257, "dense")]),
    # (B * N <= 16384 alone would end B's one-launch batch epochs at 151 rows; N * D * B <= 262144 ends them at 121)
    "B": dict(W=12, H=9, J=20, tr=po.MEDIAN, custom=False,
              chunks=[(37, "dense"), (151, "dense"), (152, "dense"), (121, "dense"), (122, "dense")]),
    "C": dict(W=12, H=12, J=6, tr=po.CLR, custom=False, chunks=[(77, "clr"), (128, "clr")]),
    "D": dict(W=4, H=2, J=512, tr=po.MEDIAN, custom=False, chunks=[(3, "dense"), (64, "dense")]),
    # (1100 rows with an all-zero column: the chunk gets the column compaction, so vsom_ensemble_upload_chunks stages it by
    # the single-context path from the raw copy)
    "E": dict(W=40, H=36, J=24, tr=po.STANDARD, custom=False, zero_col=(2, 5),
              chunks=[(77, "dense"), (300, "dense"), (1100, "dense")]),
    "F": dict(CONFIGS["custom12"], chunks=[(64, "dense"), (200, "dense")]),
    "G": dict(CONFIGS["std48"], chunks=[(77, "u8"), (300, "f")], lazy=True),      # created under VSOM_SIGMA_LAZY
}
ENS_CONFIGS = {
    "ens_shared": dict(members=["A", "A2", "B", "C", "D", "E"], one_stream=True),       # the header's fast form
    "ens_own": dict(members=["A", "B", "C", "E", "F", "G"], one_stream=False),          # joined through own_stream
}


# ---- the ensemble_query profile: two more members and two configurations of their own (generate_ensemble_query) ----
ENSQ_MEMBERS = {
    # (the many-member query kernels take one workgroup per (member, 64 rows): every row count is at a tile border;
    # exact_rows: chunk_data gives these members the rows they name, a chunk of one row included)
    "Q": dict(W=10, H=10, J=9, tr=po.STANDARD, custom=False, map_seed=200, exact_rows=True,
              chunks=[(1, "dense"), (63, "dense"), (64, "dense"), (65, "dense"), (128, "dense"), (129, "dense")]),
    # (N * D = 4104: the first size beyond the fast path's N * D <= 4096, beside D's 4096)
    "D2": dict(W=4, H=2, J=513, tr=po.MEDIAN, custom=False, exact_rows=True, chunks=[(3, "dense"), (64, "dense")]),
}
ENSQ_CONFIGS = {
    "ensq_shared": dict(members=["A", "A2", "B", "C", "D", "D2", "Q", "E"], one_stream=True),
    "ensq_own": dict(members=["A", "B", "C", "D", "D2", "Q", "F", "G"], one_stream=False),
}


def config(name):
    """a configuration of the single-context profiles, or an ensemble member"""
    if name in CONFIGS:
        return CONFIGS[name]
    return ENS_MEMBERS[name] if name in ENS_MEMBERS else ENSQ_MEMBERS[name]


def ens_config(name):
    """an ensemble configuration of the ensemble or the ensemble_query profile"""
    return ENS_CONFIGS[name] if name in ENS_CONFIGS else ENSQ_CONFIGS[name]


# ops that read the staged rows of the current chunk: the ones a pending chunk staged ahead may refuse
READS_ROWS = {"bmu", "bmu_local", "bmu_restricted", "distances", "distances_row", "p1", "p2", "epoch", "epoch_async",
              "online", "epoch_masked", "similarity", "generate", "evaluate", "topk", "bmd", "bmu_masked",
              "distances_raw"}       # (distances_raw: against chunk rows, not from_map)
OBSERVE = {"get_state", "get_last_bmu", "get_sqres", "get_mse"}
# what a custom context refuses (include/vsom_hip.h, vsom_create_custom)
CUSTOM_REFUSED = {"stage", "p1", "finish", "p2", "bmu_restricted", "distances_row", "epoch_masked", "similarity",
                  "generate", "decode_nodes", "distances_raw", "umatrix", "evaluate", "topk", "bmd", "bmu_masked",
                  "compaction"}
# what a CLR context refuses (vsom_bmu_masked_batch, vsom_batch_epoch_masked: Standard / Median only)
CLR_REFUSED = {"bmu_masked", "epoch_masked"}
# the calls that leave a pending sigmaMap pending, "and no others" (include/vsom_hip.h, vsom_set_sigma_mode); a whole-map
# epoch drops it, a partial phase-2 range materialises it
SIGMA_KEEP = {"upload", "upload_empty", "prefetch", "stage", "commit", "p1", "finish", "p2", "epoch", "epoch_async",
              "get_mse", "get_last_bmu", "set_last_bmu", "get_sqres", "bmu_mode", "sigma_mode", "compaction"}
READERS = ("similarity", "generate", "decode_nodes", "distances_raw", "umatrix", "evaluate")
ARENA = ("topk", "bmd", "bmu_masked")
# what the real backend checks against its EAGER twin, bit for bit
TWIN_COMPARED = set(READERS) | set(ARENA) | {"epoch_masked"}
# ---- the accum profile ----
ACCUM_OPS = ("accum_begin", "accum_chunk", "accum_chunk_masked", "accum_end", "accum_abort")
MASKED_SCORES = ("similarity_masked", "evaluate_masked")
READS_ROWS |= {"accum_chunk", "accum_chunk_masked"} | set(MASKED_SCORES)
CUSTOM_REFUSED |= set(MASKED_SCORES)
CLR_REFUSED |= set(MASKED_SCORES)
ACCUM_TWIN_COMPARED = TWIN_COMPARED | set(MASKED_SCORES)
# vsom_set_update_mode touches neither the stream nor the pending record
ACCUM_KEEP = {"update_mode"}
ACCUM_DRAWS = 12                     # random draws of an accum walk, around its runs (about 120 ops)
UPDATE_STRICT, UPDATE_FMA = 0, 1
MASK_ROWS = 300                      # masked chunks on chunks of at most this many rows (at scale 1): the model's masked
#                                      search is pure Python, a row at a time
MASK_DISTANCES = 80000               # ... at about 9 us a distance
MAX_DIRTY = 16                       # dirty columns of an epoch (but for run 1's row without a valid column)
RUNS = tuple(range(1, 10))
NO_WAIT_RUNS = (1, 2)
# what may stand inside a no-wait run: none of these waits for the stream (an upload only with asynchronous=True, a
# prefetch only from pinned memory); run 2's top-k query, its subject, is the one exception
NO_WAIT_OPS = {"upload", "prefetch", "stage", "commit", "accum_begin", "accum_chunk", "accum_chunk_masked"}


def chunk_list(cfg, profile="ingest"):
    """the configuration's chunks (size, kind) as the profile sees them"""
    return cfg["chunks"] + (cfg.get("accum_chunks", []) if profile == "accum" else [])


def chunk_data(cfg_name, seed, scale=1, profile="ingest"):
    cfg = config(cfg_name)
    out = []
    for i, (b, kind) in enumerate(chunk_list(cfg, profile)):
        b = b if cfg.get("exact_rows") else max(8, b // scale)
        s = 1000 * seed + 17 * i + 3
        if kind == "u8":
            x = gen.mnist_like(b, seed=s, dim=cfg["J"])
        elif kind == "f":
            x = (gen.mnist_like(b, seed=s, dim=cfg["J"]) / np.float32(255)).astype(np.float32)
        elif kind == "clr":
            x = gen.correlated(b, cfg["J"], seed=s)
        else:
            x = gen.blobs(b, cfg["J"], 5, s, s + 1, sigma=0.4)
        if cfg.get("zero_col", (None,))[0] == i:      # (ensemble member E: a column the compaction drops)
            x = np.array(x, np.float32)
            x[:, cfg["zero_col"][1]] = 0
        out.append(np.ascontiguousarray(x, np.float32))
    return out


def maskable(cfg, first=False):
    """The chunks a masked chunk call may run on: at most MASK_ROWS rows at scale 1, and at most MASK_DISTANCES masked
    distances of the model's -- rows x nodes in an epoch that searches the whole map (is_first), an eighth of that or less
    for the local walk from lastBMU.  (Only run 1 puts masked chunks into a first epoch: generate_accum.)"""
    cap = (1 if first else 8) * MASK_DISTANCES // (cfg["W"] * cfg["H"])
    return [i for i, (b, _) in enumerate(chunk_list(cfg, "accum")) if b <= min(cap, MASK_ROWS)]


def accepts_accum(cfg):
    """whether vsom_batch_accum_begin opens an epoch on this configuration (Standard / Median, no custom hooks)"""
    return not cfg["custom"] and cfg["tr"] != po.CLR


def border_columns(J):
    """the columns every masked chunk has invalid entries in: the first, the last, one each side of the 32-column word
    border of the (column, row) bits (where the map is that deep)"""
    return sorted({0, J - 1} | ({31, 32} if J > 33 else set()))


def poisoned_rows(X, seed, k, form, full):
    """X with NaN / +inf / -inf under every invalid entry of accum_mask(seed, k, form, full, X): what the masked chunk call
    with these parameters is given.  None of it may reach an output."""
    valid = np.broadcast_to(accum_mask(seed, k, form, full, X) != 0, X.shape)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    rs = np.random.RandomState([seed, k, 1])
    return np.where(valid, X, bad[rs.randint(3, size=X.shape)]).astype(np.float32)


def accum_mask(seed, k, form, full, X):
    """The validity bytes of the k-th masked chunk (from 0) of the epoch whose draws `seed` names, for the rows X: uint8
    [B, J] (form "rows") or [J] ("one_mask").  The epoch's dirty columns are the border columns, one column invalid in every
    masked chunk (with masked chunks only: no valid row in the whole epoch) and columns that turn dirty in the epoch's
    second or third masked chunk, MAX_DIRTY at the most; `full` adds a row without a valid column, which makes every
    column dirty.  Whatever is not finite in X is invalid."""
    B, J = X.shape
    rs = np.random.RandomState(seed)
    base = border_columns(J)
    others = [int(d) for d in rs.permutation(J) if d not in base]
    dead, late = others[0], others[1:MAX_DIRTY - len(base)]
    active = base + [d for i, d in enumerate(late) if 1 + i % 2 <= k]
    rk = np.random.RandomState([seed, k])
    if form == "one_mask":
        valid = np.ones(J, np.uint8)
        valid[base] = 0
        valid[dead] = 0
        for d in active[len(base):]:
            valid[d] = rk.rand() < 0.5
        return valid & np.isfinite(X).all(axis=0)
    valid = np.ones((B, J), np.uint8)
    valid[:, dead] = 0
    if B:
        for d in active:
            bad = rk.rand(B) < 0.3
            bad[rk.randint(B)] = True
            valid[bad, d] = 0
        if full:
            valid[rk.randint(B), :] = 0
    return valid & np.isfinite(X)


def chain_max_nodes(cfg):
    """The largest phase-2 node range that takes the small-map chain kernel, which reads the staged rows themselves
    (csrc/vsom_phase2_plan.hpp, vsom_use_chain: ceil(n / 64) * ceil(D / 14) <= VSOM_CHAIN_MAX_WAVES); a larger range takes
    the lane = node kernels, which record the rows-are-free event a later prefetch may stage ahead behind.  None where
    nothing is staged ahead (CLR, custom contexts)."""
    if cfg["custom"] or cfg["tr"] == po.CLR:
        return None
    D = po.length(cfg["tr"], cfg["J"])
    return 64 * (VSOM_CHAIN_MAX_WAVES // ((D + 13) // 14))


def stages_ahead(cfg):
    """whether a whole-map phase 2 takes the lane = node kernels, so that a prefetch right behind it stages ahead"""
    c = chain_max_nodes(cfg)
    return c is not None and cfg["W"] * cfg["H"] > c


def defers(cfg):
    """whether a whole-map epoch of this configuration may leave its sigmaMap pending: Standard / Median on the lane = node
    kernels, at a depth that is a multiple of 4 (so that it does not matter whether the column compaction applied)"""
    return stages_ahead(cfg) and po.length(cfg["tr"], cfg["J"]) % 4 == 0


def two_quad_launch(cfg):
    """mirror of the launch rule of the mean-only chains (csrc/vsom_phase2_plan.hpp, vsom_phase2_plan): workgroups = node groups of
    64 x blocks of 8 column quads; the two-quad kernels where 3 * workgroups > 2 * 1024.  (With the compaction the quads
    come from the compacted pitch, which is fixed per context: the depth rounded up to 32 columns.)"""
    D = po.length(cfg["tr"], cfg["J"])
    wgs = ((cfg["W"] * cfg["H"] + 63) // 64) * (((D + 3) // 4 + 7) // 8)
    return wgs, 3 * wgs > 2 * 1024


def initial_map(cfg_name, seed):
    cfg = config(cfg_name)
    D = po.length(cfg["tr"], cfg["J"])
    m = gen.random_map(cfg["W"] * cfg["H"], D, seed=seed)
    if cfg["J"] >= 100:                  # in the range of the uint8-valued chunks
        m = (m * np.float32(100) + np.float32(100)).astype(np.float32)
    if cfg["tr"] == po.CLR:
        m = (m * np.float32(0.2)).astype(np.float32)
    return m


# ---- generator ---------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, cfg_name, seed, scale, profile="ingest", mode="lazy"):
        self.cfg = CONFIGS[cfg_name]
        self.profile = profile
        self.walk_mode = self.mode = mode  # sigma profile: the mode the required runs need, the mode in force
        self.last_sigma = None
        self.rs = np.random.RandomState(seed)
        self.sizes = [max(8, b // scale) for b, _ in chunk_list(self.cfg, profile)]
        self.N = self.cfg["W"] * self.cfg["H"]
        self.B = self.sizes[0]
        self.pending = None                # index of the pending chunk
        self.chain = False                 # an online chunk may continue the running MSE (first_chunk = 0)
        self.ops = []

    def r(self, n):
        return int(self.rs.randint(n))

    def sigma(self):
        return float(self.rs.choice([0.7, 1.0, 2.5, 6.0, 12.0]))

    def emit(self, name, **p):
        self.ops.append((name, p))
        if name == "upload":
            self.B = self.sizes[p["chunk"]]
        elif name == "upload_empty":
            self.B = 0
        elif name == "sigma_mode":
            self.mode = p["mode"]
        elif name == "stage" and self.cfg["custom"] and self.profile == "accum":
            pass                           # (refused: a custom context takes no chunk in HBM; nothing becomes pending)
        elif name in ("prefetch", "stage"):
            self.pending = p["chunk"]
        elif name == "commit" and self.pending is not None:
            self.B = self.sizes[self.pending]
            self.pending = None
        if name == "online":
            self.chain = self.pending is None       # (with a chunk pending the call may be refused)
        elif name in ("single", "epoch", "epoch_async", "p1", "finish", "p2", "epoch_masked") or name in ACCUM_OPS:
            self.chain = False
        if "sigma" in p and name != "online":
            self.last_sigma = p["sigma"]

    def next_chunk(self):
        return self.r(len(self.sizes))

    def give(self, chunk=None):
        """a prefetch from pinned or pageable memory, or a chunk handed over in HBM"""
        src = ["pinned", "pageable", "device"][self.r(3)]
        chunk = self.next_chunk() if chunk is None else chunk
        if src == "device":
            self.emit("stage", chunk=chunk)
        else:
            self.emit("prefetch", chunk=chunk, src=src)

    def online(self, mode=None):
        mode = mode or ["null", "mse", "fetch"][self.r(3)]
        first = True if not self.chain else bool(self.r(2))
        self.emit("online", eta=float(self.rs.choice([0.05, 0.2])), sigma=self.sigma(),
                  decay=self.r(2), first=first, mode=mode)

    def split(self, interleave=False, end_with_commit=False, whole=False):
        """phase 1 over a random partition of the rows, finish, phase 2 over a random partition of the nodes (whole: over
        exactly [0, N), which the header counts as a whole-map epoch)"""
        if interleave and stages_ahead(self.cfg):
            self.emit("upload", chunk=0, asynchronous=False)     # (not the short chunk staged ahead below)
        first = bool(self.r(2))
        cuts = sorted(set([0, self.B] + [self.r(self.B + 1) for _ in range(self.r(3))]))
        ranges = list(zip(cuts[:-1], cuts[1:]))
        self.rs.shuffle(ranges)
        for s0, s1 in ranges:
            self.emit("p1", s0=int(s0), s1=int(s1), first=first)
        self.emit("finish")
        sg = self.sigma()
        if whole:
            self.emit("p2", sigma=sg, n0=0, n1=self.N)
        elif interleave and stages_ahead(self.cfg):
            # a range large enough for the lane = node kernels, a short next chunk staged ahead behind it, then ranges
            # small enough for the chain kernel, which must not read the rows that staging overwrote
            c = chain_max_nodes(self.cfg)
            # (on a map of more than 2 c nodes the first range is longer, so that what is left fits the chain kernel)
            big = max(c + 1, self.N - c) + self.r(min(64, self.N - c - 1))
            sg = 12.0                       # (a wide neighbourhood: every node of the chain ranges feels every sample)
            cuts = sorted(set([big, self.N] + [big + self.r(self.N - big) for _ in range(self.r(3))]))
            rest = list(zip(cuts[:-1], cuts[1:]))
            self.rs.shuffle(rest)
            self.emit("p2", sigma=sg, n0=0, n1=int(big))
            self.give(chunk=int(np.argmin(self.sizes)))
            for n0, n1 in rest:
                self.emit("p2", sigma=sg, n0=int(n0), n1=int(n1))
        else:
            cuts = sorted(set([0, self.N, 1 + self.r(self.N - 1)] + [self.r(self.N + 1) for _ in range(self.r(3))]))
            ranges = list(zip(cuts[:-1], cuts[1:]))
            self.rs.shuffle(ranges)
            for k, (n0, n1) in enumerate(ranges):
                self.emit("p2", sigma=sg, n0=int(n0), n1=int(n1))
                if interleave and k == 0:
                    self.give()
        if end_with_commit:
            self.emit("commit")

    def random_op(self):
        cfg = self.cfg
        choices = ["upload", "give", "commit", "epoch_async", "epoch", "split", "online", "single", "bmu", "bmu_local",
                   "bmu_restricted", "distances", "distances_row", "set_last_bmu", "get_last_bmu", "get_sqres",
                   "get_mse", "bmu_mode", "set_state", "get_state"]
        w = np.array([3, 4, 4, 4, 3, 2, 5, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1], np.float64)
        sigma_ops = self.profile in ("sigma", "accum")       # (the accum profile keeps every op of the sigma profile)
        if sigma_ops:
            w[choices.index("epoch_async")], w[choices.index("epoch")] = 6, 5
            w[choices.index("online")] = 2         # (the oracle's serial scan: the ingest profile's subject, not this one's)
            more = ["sigma_mode", "sigma_flush", "compaction", "whole_p2", "upload_empty", "epoch_masked", "topk", "bmd",
                    "bmu_masked"] + list(READERS)
            choices = choices + more
            w = np.concatenate([w, [2, 1, 1, 3, 1, 1, 1, 1, 1] + [1] * len(READERS)])
        if self.profile == "accum":
            choices = choices + ["accum_epoch", "accum_stray"] + list(MASKED_SCORES)
            w = np.concatenate([w, [3, 1, 1, 1]])
        for k, v in cfg.get("weights", {}).items():
            w[choices.index(k)] = v
        if sigma_ops:
            for k, v in cfg.get("sigma_weights", {}).items():
                w[choices.index(k)] = v
        if self.profile == "accum":
            for k, v in cfg.get("accum_weights", {}).items():
                w[choices.index(k)] = v
        if cfg["custom"]:
            w[choices.index("bmu_mode")] = 0
            if "compaction" in choices:
                w[choices.index("compaction")] = 0     # (refused: the custom path has no compaction)
        what = choices[int(self.rs.choice(len(choices), p=w / w.sum()))]
        if what == "upload":
            self.emit("upload", chunk=self.next_chunk(), asynchronous=bool(self.r(2)))
        elif what == "give":
            self.give()
        elif what == "commit":
            self.emit("commit")
        elif what in ("epoch_async", "epoch"):
            self.emit(what, sigma=self.sigma(), first=bool(self.r(2)))
        elif what == "split":
            if self.pending is None:       # (a refusal inside phase 1 would leave a half-searched chunk to the finish)
                self.split()
        elif what == "online":
            if self.profile == "ingest" or self.B <= 512:      # (Median's scan of 1024 rows: 5 s on the oracle)
                self.online()
        elif what == "single":
            self.emit("single", seed=self.r(1 << 30), eta=0.1, sigma=self.sigma(), decay=self.r(2),
                      last=self.r(self.N))
        elif what == "bmu_restricted":
            if self.B <= 1100:
                self.emit(what, min_hits=int(self.rs.choice([0, 1, 3])))
        elif what == "distances":
            self.emit(what, seed=self.r(1 << 30), count=1 + self.r(300))
        elif what == "distances_row":
            self.emit(what, row=self.r(self.B))
        elif what == "set_last_bmu":
            self.emit(what, seed=self.r(1 << 30))
        elif what == "bmu_mode":
            self.emit(what, mode=self.r(3))
        elif what == "set_state":
            parts = ["map", "msw", "all"] + (["map_only", "weight_only"] if sigma_ops else [])
            self.emit(what, seed=self.r(1 << 30), parts=parts[self.r(len(parts))])
        elif what == "sigma_mode":
            self.emit(what, mode=["auto", "eager", "lazy"][self.r(3)])
        elif what == "compaction":
            self.emit(what, min_rows=int(self.rs.choice([1, -1, 1024])))
        elif what == "whole_p2":
            if self.pending is None:
                self.split(whole=True)
        elif what == "upload_empty":
            self.empty_chunk_epoch()
            self.emit("upload", chunk=self.next_chunk(), asynchronous=False)
        elif what == "epoch_masked":
            self.masked_epoch()
        elif what in READERS or what in ARENA or what in MASKED_SCORES:
            self.query(what)
        elif what == "accum_epoch":
            self.random_epoch()
        elif what == "accum_stray":
            self.emit(["accum_chunk", "accum_end", "accum_abort"][self.r(3)])      # (no epoch is open: refused)
        else:
            self.emit(what)

    # ---- the accum profile: epochs are generated whole, so that total_rows is known at the begin ----
    def load(self, chunk, nowait=False, poisoned=False):
        """make `chunk` the current chunk; nowait: by calls that do not wait for the stream (an asynchronous upload from
        pinned memory, a prefetch from pinned memory or a chunk handed over in HBM, and the commit)"""
        p = dict(chunk=int(chunk))
        if poisoned and accepts_accum(self.cfg):       # (elsewhere the call is refused and the rows reach the other ops)
            p["poisoned"] = poisoned
        how = self.r(3 if nowait else 5)
        if how == 2 and self.cfg["custom"]:    # (a custom context refuses the hand-over in HBM)
            how = 1
        if how == 0:
            self.emit("upload", asynchronous=True, **p)
        elif how == 1:
            self.emit("prefetch", src="pinned", **p)
            self.emit("commit")
        elif how == 2:
            self.emit("stage", **p)
            self.emit("commit")
        elif how == 3:
            self.emit("prefetch", src="pageable", **p)
            self.emit("commit")
        else:
            self.emit("upload", asynchronous=False, **p)

    def accum_epoch(self, plan, first, nowait=False, finish="end", set_lb=False, full=False, between=None, sigma=None):
        """begin, one load and one chunk call per entry of plan -- (chunk, "plain" / "rows" / "one_mask") --, between[i]()
        behind chunk call i, then end / abort.  The masked chunks of an epoch share its seed and count up k (accum_mask);
        their rows are the poisoned ones."""
        seed = self.r(1 << 30)
        self.emit("accum_begin", sigma=self.sigma() if sigma is None else sigma, first=bool(first),
                  total=int(sum(self.sizes[c] for c, _ in plan)))
        k = 0
        for i, (chunk, kind) in enumerate(plan):
            p = None
            if kind != "plain":
                p = dict(seed=seed, form=kind, k=k)
                if full and kind == "rows" and not any(kd == "rows" for _, kd in plan[:i]):
                    p["full"] = True
            self.load(chunk, nowait, poisoned=p)
            if set_lb:
                self.emit("set_last_bmu", seed=self.r(1 << 30))
            if kind == "plain":
                self.emit("accum_chunk")
            else:
                self.emit("accum_chunk_masked", **p)
                k += 1
            if between and i in between:
                between[i]()
        if finish:
            self.emit("accum_" + finish)

    def first_for(self, plan):
        """is_first of an epoch with this plan: drawn, but 0 where it has a masked chunk (the model's full masked search
        is its dearest op: run 1 alone pays for it)"""
        return bool(self.r(2)) and all(kind == "plain" for _, kind in plan)

    def masked_kind(self):
        return ["rows", "one_mask"][self.r(2)]

    def any_maskable(self, first=False):
        m = maskable(self.cfg, first)
        return m[self.r(len(m))]

    def clean_chunk(self):
        """(a poisoned chunk must not stay current: the other ops would read its NaN)"""
        self.emit("upload", chunk=self.small(), asynchronous=False)

    def random_epoch(self):
        if self.pending is not None:
            self.emit("commit")
        plan = []
        for _ in range(1 + self.r(3)):
            if self.r(10) < 3:
                plan.append((self.any_maskable(), self.masked_kind()))
            else:
                plan.append((self.small(), "plain"))
        first = self.first_for(plan)
        self.accum_epoch(plan, first, set_lb=not first and bool(self.r(2)), finish="end" if self.r(4) else "abort")
        self.clean_chunk()

    def accum_run(self, run):
        cfg = self.cfg
        if self.pending is not None:
            self.emit("commit")
        if self.mode != self.walk_mode:
            self.emit("sigma_mode", mode=self.walk_mode)
        self.emit("upload", chunk=self.small(), asynchronous=False)
        self.emit("run", id=run)
        order = [int(i) for i in np.argsort(self.sizes, kind="stable")]
        if run == 1:
            short = [int(c) for c in self.rs.permutation(maskable(cfg, True))]      # no chunk twice in a row
            kinds = ["rows", self.masked_kind(), self.masked_kind()]
            self.rs.shuffle(kinds)
            plan = [(short[i % len(short)], kinds[i]) for i in range(3)]
            self.accum_epoch(plan, True, nowait=True, full=True)
        elif run == 2:
            a, b = sorted(self.rs.choice(len(order) - 1, 2, replace=False))
            plan = [(order[a], "plain"), (order[b], "plain"), (order[-1], "plain")]

            def topk():
                n = min(64, self.B)
                r0 = self.r(self.B - n + 1)
                self.emit("topk", k=8, r0=r0, r1=r0 + n)
            self.accum_epoch(plan, True, nowait=True, between={1: topk})
        elif run == 3:
            plan = [(self.small(), "plain"), (self.any_maskable(), self.masked_kind()), (self.small(), "plain")]
            self.accum_epoch(plan, False, set_lb=True)
        elif run == 4:
            plan = [(self.small(), "plain") for _ in range(2 + self.r(2))]
            plan[self.r(len(plan))] = (self.any_maskable(), self.masked_kind())
            self.accum_epoch(plan, False, finish="abort")
            self.emit("get_state")
            self.accum_epoch([(self.small(), "plain") for _ in range(1 + self.r(2))], bool(self.r(2)))
        elif run == 5:
            short = order[0]
            total = self.B + self.sizes[short]
            self.emit("epoch_async", sigma=self.sigma(), first=bool(self.r(2)))
            self.emit("prefetch", chunk=short, src=["pinned", "pageable"][self.r(2)])
            self.emit("accum_begin", sigma=self.sigma(), first=True, total=total)
            self.emit("accum_chunk")           # refused where the prefetch was staged ahead; else it takes the old chunk
            self.emit("commit")
            self.emit("accum_chunk")
            self.emit("accum_abort")           # (rows are missing where the first chunk call was refused)
        elif run == 6:
            for name in ("accum_chunk", "accum_end", "accum_abort"):
                self.emit(name)                # no epoch is open
            self.emit("accum_chunk_masked", seed=0, form="rows", k=0, null=True)
            if not cfg["custom"]:              # (a custom context refuses the contracted modes themselves)
                self.emit("update_mode", mode=UPDATE_FMA)
                self.emit("accum_begin", sigma=self.sigma(), first=True, total=self.B)
                self.emit("update_mode", mode=UPDATE_STRICT)
            self.emit("accum_begin", sigma=self.sigma(), first=True, total=0)       # the empty epoch
            self.emit("accum_end")
            self.emit("get_state")
            self.emit("set_state", seed=self.r(1 << 30), parts="msw")
            c1, c2, big = self.small(), order[0], order[-1]
            self.emit("accum_begin", sigma=self.sigma(), first=True, total=self.sizes[c1] + self.sizes[c2])
            self.emit("accum_begin", sigma=self.sigma(), first=True, total=7)       # an epoch is open
            self.load(c1)
            self.emit("accum_chunk")
            self.emit("accum_chunk_masked", seed=0, form="rows", k=0, null=True)
            self.emit("upload_empty")
            self.emit("accum_chunk")           # an empty chunk: accepted, changes nothing
            self.load(big)
            self.emit("accum_chunk")           # more rows than are missing
            self.emit("accum_end")             # rows are missing: refused, the epoch stays open
            self.load(c2)
            self.emit("accum_chunk")
            self.emit("accum_end")
        elif run == 7:
            self.pending_epoch(("epoch_async",))
            plan = [(self.small(), "plain") for _ in range(1 + self.r(2))]
            self.accum_epoch(plan, bool(self.r(2)))
        elif run == 8:
            sg = self.sigma()
            other = self.sigma()
            while other == sg:
                other = self.sigma()

            def rewrite():
                self.emit("set_state", seed=self.r(1 << 30), parts="map")
                self.emit("single", seed=self.r(1 << 30), eta=0.1, sigma=other, decay=self.r(2), last=self.r(self.N))
            plan = [(self.small(), "plain"), (self.any_maskable(), self.masked_kind()) if self.r(2) else (self.small(), "plain")]
            self.accum_epoch(plan, self.first_for(plan), between={0: rewrite}, sigma=sg)
        elif run == 9:
            def queries():
                for what in MASKED_SCORES + ("bmu_masked", "bmd", READERS[self.r(len(READERS))]):
                    self.query(what)
            plan = [(self.small(), "plain"), (self.any_maskable(), self.masked_kind()) if self.r(2) else (self.small(), "plain")]
            self.accum_epoch(plan, self.first_for(plan), between={0: queries})
        self.emit("run_end", id=run)
        self.clean_chunk()
        self.emit("get_state")

    # ---- the sigma profile ----
    def window(self):
        """a row window of at most 64 rows"""
        n = 1 + self.r(min(64, self.B))
        r0 = self.r(self.B - n + 1)
        return dict(r0=r0, r1=r0 + n)

    def query(self, what):
        seed = self.r(1 << 30)
        if what == "similarity":
            # (the model's restricted search is a Python loop over the chunk's rows, as for bmu_restricted)
            self.emit(what, min_hits=self.r(2) if self.B <= 1100 else 0, rule=self.r(2), **self.window())
        elif what in ("generate", "bmd", "bmu_masked"):
            self.emit(what, min_hits=self.r(2), rule=self.r(2), seed=seed, **self.window())
        elif what == "evaluate":
            self.emit(what, seed=seed, **self.window())
        elif what == "similarity_masked":
            self.emit(what, min_hits=self.r(2), rule=self.r(2), seed=seed, form=self.masked_kind(), **self.window())
        elif what == "evaluate_masked":
            self.emit(what, min_hits=self.r(2), seed=seed, form=self.masked_kind(), **self.window())
        elif what == "topk":
            self.emit(what, k=1 + self.r(8), **self.window())
        elif what == "decode_nodes":
            self.emit(what, count=1 + self.r(64), seed=seed)
        elif what == "distances_raw":
            self.emit(what, count=1 + self.r(64), seed=seed, from_map=bool(self.r(2)))
        else:
            self.emit(what)

    def reader(self):
        self.query(READERS[self.r(len(READERS))])

    def small(self):
        """one of the shorter chunks (never the largest)"""
        order = np.argsort(self.sizes, kind="stable")
        return int(order[self.r(max(1, len(order) // 2))])

    def masked_epoch(self):
        # the masked search of the model is pure Python, a row at a time: on the shortest chunk
        if self.pending is not None:
            self.emit("commit")
        self.emit("upload", chunk=int(np.argmin(self.sizes)), asynchronous=False)
        self.emit("epoch_masked", sigma=self.sigma(), first=bool(self.r(2)), seed=self.r(1 << 30))

    def empty_chunk_epoch(self):
        if self.pending is not None:
            self.emit("commit")
        self.emit("upload_empty")
        self.emit(["epoch", "epoch_async"][self.r(2)], sigma=self.sigma(), first=bool(self.r(2)))

    def whole_epoch(self, kinds=("epoch_async", "epoch", "p2")):
        kind = kinds[self.r(len(kinds))]
        if kind == "p2" and not self.cfg["custom"]:        # (a custom context refuses the split phases)
            self.split(whole=True)
        else:
            self.emit("epoch" if kind == "epoch" else "epoch_async", sigma=self.sigma(), first=bool(self.r(2)))

    def pending_epoch(self, kinds=("epoch_async", "epoch", "p2")):
        """a whole-map epoch that leaves its sigmaMap pending where the configuration defers: in the walk's mode -- under
        AUTO behind two whole-map epochs with nothing between them"""
        if self.mode != self.walk_mode:
            self.emit("sigma_mode", mode=self.walk_mode)
        if self.walk_mode == "auto":
            self.whole_epoch(("epoch_async",))
            self.whole_epoch(("epoch_async",))
        self.whole_epoch(kinds)

    def sigma_run(self, run):
        if self.pending is not None:
            self.emit("commit")
        short = int(np.argmin(self.sizes))
        self.emit("upload", chunk=short if run == 4 else self.small(), asynchronous=False)
        if run == 0:
            # (an asynchronous epoch or a whole-map range: what a prefetch right behind it stages ahead of)
            self.pending_epoch(("epoch_async", "p2"))
            self.give(chunk=short)
            self.emit("commit")
            self.reader()
        elif run == 1:
            self.pending_epoch()
            self.emit("set_last_bmu", seed=self.r(1 << 30))
            sg = self.sigma()
            while sg == self.last_sigma:
                sg = self.sigma()
            n0 = 1 + self.r(self.N - 1)
            self.emit("p2", sigma=sg, n0=n0, n1=n0 + 1 + self.r(self.N - n0))
        elif run == 2:
            self.pending_epoch()
            self.emit("upload", chunk=int(np.argmax(self.sizes)), asynchronous=bool(self.r(2)))
            self.emit("sigma_flush")
        elif run == 3:
            self.pending_epoch()
            self.empty_chunk_epoch()
            self.emit("get_state")
            self.emit("upload", chunk=self.small(), asynchronous=False)
        elif run == 4:
            self.pending_epoch()
            self.online(mode="null")
        elif run == 5:
            self.pending_epoch()
            self.emit("set_state", seed=self.r(1 << 30), parts="weight_only")
        else:
            if self.mode != self.walk_mode:
                self.emit("sigma_mode", mode=self.walk_mode)
            for _ in range(3):
                self.whole_epoch()
                keep = self.r(4)
                if keep == 0:
                    self.emit("get_mse")
                elif keep == 1:
                    self.emit("get_last_bmu")
                elif keep == 2:
                    self.emit("upload", chunk=self.small(), asynchronous=bool(self.r(2)))
                else:
                    self.give(chunk=self.small())
                    self.emit("commit")
            self.reader()
        self.emit("get_state")


def generate_sigma(cfg_name, seed, n_ops, scale, mode):
    """The sigma profile.  By construction the walk holds each of these runs, with no materialising call before its end
    (E: a whole-map epoch that leaves its sigmaMap pending where the configuration defers -- under AUTO the third of three):
    E -> prefetch / stage_next_device (staged ahead where the configuration stages ahead) -> commit -> reader;
    E -> set_last_bmu -> partial phase-2 range at another sigma;
    E -> upload of the largest chunk -> sigma_flush;
    E -> upload_empty -> epoch -> get_state;
    E -> online chunk (mse NULL) -> get_state;
    E -> weight-only set_state -> get_state;
    three whole-map epochs with a call that keeps the record behind each (get_mse, get_last_bmu, an upload, a prefetch and
    its commit) -> reader."""
    assert mode in ("lazy", "auto"), mode
    g = _Gen(cfg_name, seed, scale, "sigma", mode)
    g.ops.append(("config", {"name": cfg_name, "seed": seed, "scale": scale, "profile": "sigma", "mode": mode}))
    g.emit("sigma_mode", mode=mode)
    g.emit("set_state", seed=seed, parts="init")
    g.emit("upload", chunk=0, asynchronous=False)
    slots = sorted(g.rs.choice(np.arange(3, n_ops - 4), 7, replace=False))
    runs = list(g.rs.permutation(7))
    k = 3
    while k < n_ops:
        if slots and k >= slots[0]:
            slots.pop(0)
            g.sigma_run(runs.pop(0))
            k += 2
            continue
        g.random_op()
        k += 1
    g.emit("get_state")
    return g.ops


def generate_accum(cfg_name, seed, n_ops, scale, mode):
    """The accum profile: n_ops random draws (the sigma profile's ops, whole accumulated epochs, stray accum calls, the
    masked scoring calls) around the nine runs of the module docstring, each between its markers.  The walk opens with the
    one refusal that needs a context without a chunk."""
    assert mode in ("lazy", "auto"), mode
    g = _Gen(cfg_name, seed, scale, "accum", mode)
    g.ops.append(("config", {"name": cfg_name, "seed": seed, "scale": scale, "profile": "accum", "mode": mode}))
    g.emit("sigma_mode", mode=mode)
    g.emit("set_state", seed=seed, parts="init")
    g.emit("run", id=6)
    g.emit("accum_begin", sigma=g.sigma(), first=True, total=g.sizes[0])
    g.emit("accum_chunk")                  # no chunk loaded
    g.emit("accum_abort")
    g.emit("run_end", id=6)
    g.emit("upload", chunk=0, asynchronous=False)
    slots = sorted(g.rs.choice(np.arange(1, n_ops), len(RUNS), replace=False))
    runs = [int(r) for r in g.rs.permutation(RUNS)]
    for k in range(n_ops):
        if slots and k >= slots[0]:
            slots.pop(0)
            g.accum_run(runs.pop(0))
        g.random_op()
    g.emit("get_state")
    return g.ops


def generate(cfg_name, seed, n_ops=40, scale=1, profile="ingest", mode="lazy"):
    """A walk of about n_ops ops.  profile="sigma": generate_sigma, in `mode` ("lazy" / "auto").  profile="accum":
    generate_accum, with n_ops random draws around its runs.  profile="ingest": by
    construction it holds each of these runs with no synchronising call inside:
    async epoch -> online chunk (mse NULL) -> prefetch / stage_next_device -> commit;
    phase-2 range -> prefetch -> phase-2 range(s) -> commit (where a prefetch stages ahead: a lane = node range, a short
    chunk staged behind it, chain-kernel ranges);
    async epoch -> prefetch -> prefetch (an abandoned stage-ahead) -> search -> commit."""
    if profile == "sigma":
        return generate_sigma(cfg_name, seed, n_ops, scale, mode)
    if profile == "accum":
        return generate_accum(cfg_name, seed, n_ops, scale, mode)
    assert profile == "ingest", profile
    g = _Gen(cfg_name, seed, scale)
    g.ops.append(("config", {"name": cfg_name, "seed": seed, "scale": scale}))
    g.emit("set_state", seed=seed, parts="init")
    g.emit("upload", chunk=0, asynchronous=False)
    slots = sorted(g.rs.choice(np.arange(2, n_ops - 8), 3, replace=False))
    runs = list(g.rs.permutation(3))
    k = 2
    while k < n_ops:
        if slots and k >= slots[0]:
            slots.pop(0)
            run = runs.pop(0)
            if g.pending is not None:
                g.emit("commit")
            if run == 0:
                # a long online chunk (the per-sample scan over the first chunk's rows) and a short next chunk that fits
                # the staged-row buffers: staged ahead, its staging would land inside the online chunk
                g.emit("upload", chunk=0, asynchronous=False)
                if not g.cfg["custom"]:
                    g.emit("bmu_mode", mode=BMU_EXACT)
                g.emit("epoch_async", sigma=g.sigma(), first=bool(g.r(2)))
                g.online(mode="null")
                g.give(chunk=int(np.argmin(g.sizes)))
                g.emit("commit")
            elif run == 1:
                g.split(interleave=True, end_with_commit=True)
            else:
                g.emit("epoch_async", sigma=g.sigma(), first=bool(g.r(2)))
                g.give()
                g.give()
                search = ["bmu", "bmu_local", "distances_row"][g.r(3)]
                if search == "distances_row":
                    g.emit(search, row=g.r(g.B))
                else:
                    g.emit(search)
                g.emit("commit")
            g.emit("get_state")     # (after the run: before a later epoch rewrites what the run left)
            k += 4
            continue
        g.random_op()
        k += 1
    g.emit("get_state")
    return g.ops


# ---- the model ---------------------------------------------------------------------------------------------------------
class Refused(Exception):
    pass


def _rand_state(cfg_name, seed, parts, N, D):
    rs = np.random.RandomState(seed)
    if parts == "hits0":                   # (the ensemble_query profile: only node 0 is a candidate under min_hits >= 1)
        return {"hits": np.zeros(N, np.uint64)}
    if parts == "weight_only":
        return {"weight": (rs.rand(N) * 10 + 0.5).astype(np.float32)}
    st = {"map": initial_map(cfg_name, seed)}      # ("map", "map_only": the map alone)
    if parts in ("msw", "all"):
        st["sigma"] = (rs.rand(N, D) * 0.5).astype(np.float32)
        st["S"] = (rs.rand(N, D) * 2).astype(np.float32)
        st["weight"] = (rs.rand(N) * 10).astype(np.float32)
        if parts == "msw":
            st["sigma"][...] = 0
            st["S"][...] = 0
    if parts == "all":
        st["hits"] = rs.randint(0, 5, size=N).astype(np.uint64)
    return st


def materialize(op, model):
    """the concrete arguments of an op in the model's current state (the same for every backend)"""
    name, p = op
    cfg = model.cfg
    N, B = model.N, model.B
    if name in ("upload", "prefetch", "stage"):
        return {"X": model.rows(p)}
    if name == "accum_chunk_masked":
        if p.get("null"):
            return {"valid": None}
        X = model.X if model.X is not None else np.zeros((0, cfg["J"]), np.float32)
        return {"valid": np.ascontiguousarray(accum_mask(p["seed"], p["k"], p["form"], p.get("full", False), X), np.uint8)}
    if name in ("schedule_masked", "online_masked"):
        return {"valid": ens_mask(p, model.X)}
    if name in MASKED_SCORES:
        rs = np.random.RandomState(p["seed"])
        Xw = model.X[p["r0"]:p["r1"]]
        if p["form"] == "one_mask":
            valid = (rs.rand(cfg["J"]) < 0.8) & np.isfinite(Xw).all(axis=0)
        else:
            valid = (rs.rand(*Xw.shape) < 0.8) & np.isfinite(Xw)
        binary = (rs.rand(cfg["J"]) < 0.3).astype(np.float32)
        return {"valid": valid.astype(np.uint8), "binary": binary, "continuous": (1 - binary).astype(np.float32)}
    if name in ("topk_masked", "bmd_masked", "generate_masked"):       # (the ensemble_query profile's member ops)
        rs = np.random.RandomState(p["seed"])
        n, J, draws = p["r1"] - p["r0"], cfg["J"], p.get("draws", 1)
        valid = (rs.rand(J) < 0.7) if p["form"] == "one_mask" else (rs.rand(n, J) < 0.8)
        return {"valid": valid.astype(np.uint8), "u": rs.rand(n) if name == "bmd_masked" else rs.rand(n, draws),
                "l": 0.05 + 0.9 * rs.rand(n, draws, J)}
    if name == "single":
        rs = np.random.RandomState(p["seed"])
        X = model.chunks[rs.randint(len(model.chunks))]
        return {"v": np.ascontiguousarray(X[rs.randint(X.shape[0])])}
    if name == "distances":
        rs = np.random.RandomState(p["seed"])
        return {"nodes": rs.randint(0, N, size=p["count"]).astype(np.uint64),
                "rows": rs.randint(0, max(B, 1), size=p["count"]).astype(np.uint64)}
    if name == "set_last_bmu":
        return {"idx": np.random.RandomState(p["seed"]).randint(0, N, size=B).astype(np.uint64)}
    if name == "set_state":
        return _rand_state(model.cfg_name, p["seed"], p["parts"], N, po.length(cfg["tr"], cfg["J"]))
    J = cfg["J"]
    cols = min(J, po.length(cfg["tr"], J))
    rs = np.random.RandomState(p.get("seed", 0))
    n = p.get("r1", 0) - p.get("r0", 0)
    if name == "upload_empty":
        return {"X": np.zeros((0, J), np.float32)}
    if name == "epoch_masked":
        return {"valid": (rs.rand(B, J) < 0.8).astype(np.uint8)}
    if name == "bmu_masked":
        return {"valid": (rs.rand(n, J) < 0.8).astype(np.uint8)}
    if name == "generate":
        return {"u": rs.rand(n), "l": 0.05 + 0.9 * rs.rand(n, cols)}
    if name == "bmd":
        return {"u": rs.rand(n)}
    if name == "decode_nodes":
        return {"nodes": rs.randint(0, N, size=p["count"]).astype(np.uint64), "l": 0.05 + 0.9 * rs.rand(p["count"], cols)}
    if name == "distances_raw":
        return {"nodes": rs.randint(0, N, size=p["count"]).astype(np.uint64),
                "vrows": rs.randint(0, N if p["from_map"] else max(B, 1), size=p["count"]).astype(np.uint64)}
    if name == "evaluate":
        binary = (rs.rand(J) < 0.3).astype(np.float32)
        return {"binary": binary, "continuous": (1 - binary).astype(np.float32)}
    return {}


class SigmaRecord:
    """The pending sigmaMap as include/vsom_hip.h states it (vsom_sigma_mode, vsom_set_sigma_mode): the mode, the whole-map
    epochs since the last call that may have read sigmaMap, whether a record is pending, and vsom_sigma_stats' counters.
    Two points the header leaves open are pinned to what csrc/vsom_capi.hip and launch_phase2 do: a partial phase-2 range
    materialises without counting as a read (the header lists it among the calls that never read sigmaMap), and a refused
    call that is not on the keep list counts as a read (the header: it "may").  The vsom_batch_accum_* calls are ordinary
    entry points here, as the header says of them: none is on the keep list, so the first materialises a pending record
    (and resets AUTO's count, like every such call); none is a whole-map epoch, so none defers, drops or counts towards
    AUTO's rule; vsom_batch_accum_end writes sigmaMap eagerly (Model._accum_end)."""

    def __init__(self, cfg):
        self.can_defer = defers(cfg) and not cfg["custom"] and cfg["tr"] != po.CLR
        self.mode = SIGMA_AUTO
        self.unread = 0
        self.pending = False
        self.deferred = self.dropped = self.materialised = 0

    def stats(self):
        return (self.deferred, self.dropped, self.materialised, int(self.pending))

    def read(self):
        """an entry point that is not on the header's list: materialises, and counts as a read"""
        self.unread = 0
        if self.pending:
            self.pending = False
            self.materialised += 1

    def accepted(self, op, B, N):
        name, p = op
        if name == "sigma_mode":
            self.mode = SIGMA_MODES[p["mode"]]
        whole = name in ("epoch", "epoch_async") or (name == "p2" and p["n0"] == 0 and p["n1"] == N)
        if whole:
            if self.pending:                 # the epoch overwrites every row
                self.pending = False
                self.dropped += 1
            if self.can_defer and B > 0 and (self.mode == SIGMA_LAZY or (self.mode == SIGMA_AUTO and self.unread >= 2)):
                self.pending = True
                self.deferred += 1
            self.unread += 1
        elif name == "p2":
            if self.pending and p["n1"] > p["n0"]:     # a partial range materialises (and is no read)
                self.pending = False
                self.materialised += 1
        elif name not in SIGMA_KEEP and name not in ACCUM_KEEP:
            self.read()

    def refused(self, op, got):
        """A refused call may have materialised the record before it was refused, or not: the header does not say.  Returns
        whether `got` (vsom_sigma_stats after the call) is one of the two, and adopts it.  Whether such a call counted as a
        read the counters cannot show when nothing was pending: the model takes it as one, as the library's entry check
        does (include/vsom_hip.h allows both); were that to change, the AUTO walks would report a deferral one epoch off."""
        before = self.stats()
        if op[0] not in SIGMA_KEEP and op[0] not in ACCUM_KEEP:
            self.unread = 0
        if tuple(got) == before:
            return True
        if self.pending and tuple(got) == (before[0], before[1], before[2] + 1, 0):
            self.pending = False
            self.materialised += 1
            return True
        return False


class Model:
    """what the header says the context holds after each call"""

    def __init__(self, cfg_name, seed, scale=1, profile="ingest"):
        cfg = config(cfg_name)
        self.cfg_name, self.cfg, self.profile = cfg_name, cfg, profile
        self.som = po.OracleSom(cfg["W"], cfg["H"], cfg["J"], cfg["tr"])
        self.N = cfg["W"] * cfg["H"]
        self.chunks = chunk_data(cfg_name, seed, scale, profile)
        self.poisoned = {}                     # rows(): the poisoned copies made so far
        self.acc = None                        # the open accumulated epoch (_accum_begin)
        self.update_mode = UPDATE_STRICT
        self.X = None
        self.lb = np.zeros(0, np.uint64)
        self.sq = np.zeros(0, np.float32)      # the oracle's per-sample residuals of the last phase 1 (the finish sums them)
        self.sqres = None                      # what vsom_get_sqres returns, when a search has defined it
        self.pending = None
        self.mse = None                        # last MSE (None: nothing has written one yet)
        self.run = None                        # online running accumulator after the last online chunk
        self.sig = SigmaRecord(cfg)

    @property
    def B(self):
        return 0 if self.X is None else self.X.shape[0]

    def close(self):
        self.som.close()

    def rows(self, p):
        """the rows a load op names: the chunk, or (p["poisoned"]: the masked chunk call they are loaded for) that chunk
        with NaN / +-inf under every invalid entry of that call's mask"""
        if "poisoned" not in p:
            return self.chunks[p["chunk"]]
        q = p["poisoned"]
        key = (p["chunk"], q["seed"], q["k"], q["form"], q.get("full", False))
        if key not in self.poisoned:
            self.poisoned[key] = poisoned_rows(self.chunks[p["chunk"]], *key[1:])
        return self.poisoned[key]

    def _load(self, X):
        self.X = X
        self.lb = np.zeros(X.shape[0], np.uint64)
        self.sq = np.zeros(X.shape[0], np.float32)
        self.sqres = None

    def _dist(self, nodes, rows):
        return np.array([self.som.dist(int(n), self.X[int(r)]) for n, r in zip(nodes, rows)], np.float32)

    def refusal_allowed(self, name, p=None):
        if name == "distances_raw" and p["from_map"]:
            return False
        return name in READS_ROWS and self.pending is not None

    def _search_chunk(self, min_hits):
        """what vsom_similarity_batch / vsom_evaluate_batch leave behind: they search the WHOLE chunk, as vsom_bmu_batch
        (min_hits 0) or vsom_bmu_restricted_batch does, and score the rows of the window"""
        if min_hits:
            self.lb[:] = [self.som.find_restricted_bmu(x, min_hits) for x in self.X]
        else:
            self.som.batch_phase1_range(self.X, 0, self.B, self.lb, self.sq, True, nthreads=NTHREADS)
        self.sqres = self._dist(self.lb, np.arange(self.B))

    def _epoch_masked(self, p, valid):
        """tests/masked_train_ref.py (MaskedOracle.epoch) on this model's state"""
        s, cfg = self.som, self.cfg
        valid = valid != 0
        lb, sq = masked_train_ref.phase1(cfg["tr"], cfg["W"], cfg["H"], s.map, self.X, valid, self.lb, p["first"])
        mse = s.batch_phase1_finish(lb, sq) if self.B else np.float32(0)
        newmap, newsig, weight = masked_train_ref.phase2(cfg["tr"], cfg["W"], cfg["H"], self.X, valid, lb, p["sigma"])
        s.set_state(map=newmap, sigma=newsig, weight=weight)
        self.lb[...] = lb
        self.sqres = None
        return mse

    # ---- the accumulated epoch (include/vsom_hip.h, vsom_batch_accum_begin / vsom_batch_accum_chunk_masked) ----
    def accum_refusal(self, op, staged=False):
        """None where the header accepts the call, else words of the refusal it must get, in the order csrc/vsom_capi.hip
        checks; staged: the backend has the next chunk staged ahead over the current rows (the model cannot know)"""
        name, p = op
        acc = self.acc
        if name == "accum_begin":
            if self.cfg["custom"]:
                return "vsom_batch_accum_begin is not available on a custom-transformation context"
            if self.cfg["tr"] == po.CLR:
                return "CLR"
            if self.update_mode != UPDATE_STRICT:
                return "strict update mode"
            return "already open" if acc is not None else None
        if name == "accum_chunk_masked" and p.get("null"):
            return "valid_host is null"
        if acc is None:
            return "no accumulated epoch is open"
        if name in ("accum_chunk", "accum_chunk_masked"):
            if staged:
                return "vsom_commit_chunk first"
            if self.X is None:
                return "no chunk loaded"
            if acc["rows"] + self.B > acc["total"]:
                return "exceed total_rows"
        elif name == "accum_end" and acc["rows"] != acc["total"]:
            return "rows accumulated"
        return None

    def _accum_chunk(self, valid):
        """phase 1 of the current chunk against the current map, hits, the running MSE over total_rows; the chunk's rows,
        validity (None: a plain chunk, all valid) and lastBMU join the epoch's record"""
        acc, s, cfg, B = self.acc, self.som, self.cfg, self.B
        if B == 0:
            return
        if valid is None:
            v = np.ones(self.X.shape, bool)
            s.batch_phase1_range(self.X, 0, B, self.lb, self.sq, acc["first"], nthreads=NTHREADS)
        else:
            v = np.broadcast_to(np.asarray(valid) != 0, self.X.shape).copy()
            lb, sq = masked_train_ref.phase1(cfg["tr"], cfg["W"], cfg["H"], s.map, self.X, v, self.lb, acc["first"])
            self.lb[...] = lb
            self.sq[...] = sq
        s.batch_phase1_finish(self.lb, self.sq)        # bmuHits (its MSE is the chunk's own, not the epoch's)
        run, div = acc["run"], np.float32(acc.get("divisor", acc["total"]))
        with np.errstate(all="ignore"):
            for q in self.sq:
                run = np.float32(run + np.float32(q / div))
        acc["run"] = self.mse = run
        self.sqres = self.sq.copy()
        acc["parts"].append((self.X, v, self.lb.copy()))
        acc["rows"] += B

    def accum_phase2(self, acc):
        """(map, sigmaMap, weightMap) of vsom_batch_accum_end: the oracle's phase 2 over the concatenated rows; every column
        that had an invalid entry from the per-column restatement (tests/masked_train_ref.py, phase2).  What the rows hold
        at an invalid position is replaced by 0 first: it may reach no output."""
        cfg, J = self.cfg, self.cfg["J"]
        parts = acc["parts"]
        X = np.concatenate([x for x, _, _ in parts]) if parts else np.zeros((0, J), np.float32)
        valid = np.concatenate([v for _, v, _ in parts]) if parts else np.zeros((0, J), bool)
        lb = np.ascontiguousarray(np.concatenate([b for _, _, b in parts]) if parts else np.zeros(0), np.uint64)
        X = np.ascontiguousarray(np.where(valid, X, np.float32(0)), np.float32)
        t = po.OracleSom(cfg["W"], cfg["H"], J, cfg["tr"])
        t.batch_phase2_range(X, lb, acc["sigma"], 0, self.N, nthreads=NTHREADS)
        newmap, newsig, weight = t.map.copy(), t.sigma.copy(), t.weight.copy()
        t.close()
        dirty = np.flatnonzero(~valid.all(axis=0))
        if dirty.size:
            m, sg, _ = masked_train_ref.phase2(cfg["tr"], cfg["W"], cfg["H"], X[:, dirty], valid[:, dirty], lb, acc["sigma"])
            newmap[:, dirty] = m
            newsig[:, dirty] = sg
        return newmap, newsig, weight

    def _accum(self, op, a):
        name, p = op
        if name == "accum_begin":
            # (phase 2 never reads the map and abort writes nothing: the state at begin need not be kept)
            self.acc = dict(sigma=p["sigma"], first=p["first"], total=p["total"], rows=0, run=np.float32(0), parts=[])
        elif name == "accum_chunk":
            self._accum_chunk(None)
        elif name == "accum_chunk_masked":
            self._accum_chunk(a["valid"])
        elif name == "accum_end":
            newmap, newsig, weight = self.accum_phase2(self.acc)
            self.som.set_state(map=newmap, sigma=newsig, weight=weight)       # S is untouched
            self.mse = self.acc["run"]
            self.acc = None
            return {"mse": self.mse}
        else:                                  # abort: the model state stays; hits, lastBMU, sqres, the MSE word too
            self.acc = None
        return {}

    def apply(self, op, a):
        """the op's effect; returns the outputs the call must give"""
        name, p = op
        s = self.som
        if name in ACCUM_OPS:
            return self._accum(op, a)
        if name == "update_mode":
            self.update_mode = p["mode"]
        elif name in ("upload", "upload_empty"):
            self._load(a["X"])
        elif name == "epoch_masked":
            self.mse = self._epoch_masked(p, a["valid"])
            return {"mse": self.mse}
        elif name == "similarity":
            self._search_chunk(p["min_hits"])
        elif name == "evaluate":
            self._search_chunk(0)
        elif name in ("prefetch", "stage"):
            self.pending = a["X"]
        elif name == "commit":
            if self.pending is None:
                raise Refused("nothing pending")
            self._load(self.pending)
            self.pending = None
        elif name in ("epoch", "epoch_async"):
            self.mse = s.batch_epoch(self.X, self.lb, p["sigma"], p["first"], nthreads=NTHREADS)
            self.sqres = None
            return {"mse": self.mse} if name == "epoch" else {}
        elif name == "p1":
            s.batch_phase1_range(self.X, p["s0"], p["s1"], self.lb, self.sq, p["first"], nthreads=NTHREADS)
            self.sqres = None
        elif name == "finish":
            self.mse = s.batch_phase1_finish(self.lb, self.sq)
        elif name == "p2":
            s.batch_phase2_range(self.X, self.lb, p["sigma"], p["n0"], p["n1"], nthreads=NTHREADS)
        elif name == "online":
            start = 0.0 if p["first"] else self.run
            self.run = s.train_online_chunk(self.X, self.lb, p["eta"], p["sigma"], p["decay"], mse_start=start)
            self.mse = self.run
            self.sqres = None
            if p["mode"] == "mse":
                return {"mse": self.run}
            if p["mode"] == "fetch":
                return {"mse": self.run, "lb": self.lb.copy()}
        elif name == "single":
            bmu, res, dist, lb = s.train_single(a["v"], p["eta"], p["sigma"], p["last"], p["decay"])
            return {"bmu": bmu, "res": res, "dist": dist, "last": lb}
        elif name in ("bmu", "bmu_local"):
            s.batch_phase1_range(self.X, 0, self.B, self.lb, self.sq, name == "bmu", nthreads=NTHREADS)
            self.sqres = self._dist(self.lb, np.arange(self.B))
            return {"idx": self.lb.copy(), "dist": self.sqres.copy()}
        elif name == "bmu_restricted":
            self.lb[:] = [s.find_restricted_bmu(x, p["min_hits"]) for x in self.X]
            self.sqres = self._dist(self.lb, np.arange(self.B))
            return {"idx": self.lb.copy(), "dist": self.sqres.copy()}
        elif name == "distances":
            return {"d": self._dist(a["nodes"], a["rows"])}
        elif name == "distances_row":
            return {"d": self._dist(np.arange(self.N), np.full(self.N, p["row"]))}
        elif name == "set_last_bmu":
            self.lb[:] = a["idx"]
        elif name == "get_last_bmu":
            return {"lb": self.lb.copy()}
        elif name == "get_sqres":
            return {"sq": None if self.sqres is None else self.sqres.copy()}
        elif name == "get_mse":
            return {"mse": self.mse}
        elif name == "set_state":
            s.set_state(**a)
        elif name == "get_state":
            return self.state()
        # ---- single-context ops that enter with the ensemble profile ----
        elif name == "schedule":
            return {"mses": self._schedule(p["sigmas"], p["reset"], None)}
        elif name == "schedule_masked":
            return {"mses": self._schedule(p["sigmas"], p["reset"], a["valid"])}
        elif name == "online_masked":
            return self._online_masked(p, a["valid"])
        elif name == "um":
            self.um = s.update_umatrix()
            return {"u": self.um.copy()}
        elif name == "get_umatrix":
            return {"u": None if getattr(self, "um", None) is None else self.um.copy()}
        return {}

    def _schedule(self, sigmas, reset, valid):
        """vsom_batch_schedule as tests/schedule_ref.py, oracle_loop, states it (valid None), vsom_batch_schedule_masked as
        the same loop over _epoch_masked; a None in sigmas stands for NaN (an op list prints as Python literals)"""
        sigmas = [float("nan") if v is None else v for v in sigmas]
        if not sigmas:
            return np.zeros(0, np.float32)     # "nothing is done"
        if valid is None:
            mses, lb = schedule_ref.oracle_loop(self.som, self.X, sigmas, reset)
            self.lb[...] = lb
        else:
            valid = np.broadcast_to(np.asarray(valid) != 0, self.X.shape).copy()
            mses = np.zeros(len(sigmas), np.float32)
            for ep, sg in enumerate(sigmas):
                if ep > 0 and reset:
                    self.lb[:] = 0
                mses[ep] = self._epoch_masked({"first": ep == 0, "sigma": sg}, valid)
        self.mse = mses[-1]
        self.sqres = None
        return mses

    def _online_masked(self, p, valid):
        """tests/online_masked_ref.py, OnlineMasked.train_chunk, on this model's state"""
        s, cfg = self.som, self.cfg
        r = online_masked_ref.OnlineMasked(cfg["W"], cfg["H"], cfg["J"], cfg["tr"])
        r.set_state(map=s.map, sigma=s.sigma, S=s.S, weight=s.weight, hits=s.hits)
        start = 0.0 if p["first"] else self.run
        self.run = r.train_chunk(self.X, valid, self.lb, p["eta"], p["sigma"], p["decay"], mse_start=start)
        s.set_state(map=r.map, sigma=r.sigma, S=r.S, weight=r.weight, hits=r.hits)
        self.mse = self.run
        self.sqres = None
        return {"mse": self.run, "lb": self.lb.copy()}

    def state(self):
        s = self.som
        return {"map": s.map.copy(), "sigma": s.sigma.copy(), "S": s.S.copy(), "weight": s.weight.copy(),
                "hits": s.hits.copy()}


# ---- comparison --------------------------------------------------------------------------------------------------------
def first_difference(got, exp):
    """None when got equals exp bit for bit (floats: NaN == NaN), else a description of the first differing element"""
    if exp is None:
        return None                        # (nothing defined to compare with)
    g, e = np.asarray(got), np.asarray(exp)
    if g.shape != e.shape:
        return f"shape {g.shape} != {e.shape}"
    if e.dtype.kind == "f":
        g32, e32 = g.astype(np.float32), e.astype(np.float32)
        same = (g32.view(np.uint32) == e32.view(np.uint32)) | (np.isnan(g32) & np.isnan(e32))
    else:
        same = g == e
    if same.all():
        return None
    at = np.unravel_index(int(np.argmin(same.reshape(-1))), same.shape) if same.ndim else ()
    return f"element {tuple(int(i) for i in at)}: got {g[at]!r}, expected {e[at]!r} ({int((~same).sum())} differ)"


def first_difference_exact(got, exp):
    """the same on the values' own width (doubles on 64 bits); None values must be None on both sides"""
    if got is None or exp is None:
        return None if got is exp else f"got {type(got).__name__}, expected {type(exp).__name__}"
    g, e = np.asarray(got), np.asarray(exp)
    if g.shape != e.shape or g.dtype != e.dtype:
        return f"shape / type {g.shape} {g.dtype} != {e.shape} {e.dtype}"
    same = g == e
    if e.dtype.kind == "f":
        same = same & (np.signbit(g) == np.signbit(e)) | (np.isnan(g) & np.isnan(e))
    if np.all(same):
        return None
    same = np.atleast_1d(same)
    at = np.unravel_index(int(np.argmin(same.reshape(-1))), same.shape)
    return (f"element {tuple(int(i) for i in at)}: got {np.atleast_1d(g)[at]!r}, expected {np.atleast_1d(e)[at]!r} "
            f"({int((~same).sum())} differ)")


class WalkFailure(AssertionError):
    pass


def run_walk(ops, make_backend):
    """Run `ops` on the backend make_backend(cfg_name, model) returns and on the model; raises WalkFailure with the seed,
    the ops up to the failing one and the first differing element.  Returns counts of what happened."""
    name0, cfg = ops[0]
    assert name0 == "config", ops[0]
    sigma = cfg.get("profile", "ingest") in ("sigma", "accum")
    model = Model(cfg["name"], cfg["seed"], cfg.get("scale", 1), cfg.get("profile", "ingest"))
    model.ops = ops                        # (the real backend makes its pinned and device copies of the rows up front)
    be = make_backend(cfg["name"], model)
    stats = {"ops": 0, "refused": 0}
    if model.profile == "accum":
        stats["accum"] = {"chunks": 0, "masked": 0, "ends": 0, "aborts": 0, "staged": 0}
    run = None                             # the run of generate_accum the walk is in
    done = [ops[0]]

    def fail(msg):
        raise WalkFailure(f"call-sequence walk {cfg['name']} seed {cfg['seed']}: {msg}\n"
                          f"replay(ops) with ops = {done!r}")

    def check_outputs(what, got, exp):
        for k, e in exp.items():
            d = first_difference(got.get(k), e)
            if d:
                fail(f"{what}: output {k!r} differs from the oracle at {d}")

    def check_all(what, observe=None):
        got = (observe or be.observe)()
        exp = model.state()
        exp.update(lb=model.lb, mse=model.mse)
        check_outputs(f"{what} (full state)", got, exp)

    def check_sigma(op, out, refused):
        """vsom_sigma_stats after the call against the header's contract (SigmaRecord)"""
        if not sigma:
            return
        got = tuple(int(v) for v in out["sigma_stats"])
        stats["sigma"] = got
        if refused:
            before = model.sig.stats()
            if not model.sig.refused(op, got):
                fail(f"{op[0]} was refused and left vsom_sigma_stats = {got}: neither unchanged from {before} nor one more "
                     f"record materialised and none pending")
        elif got != model.sig.stats():
            fail(f"{op[0]}: vsom_sigma_stats = {got}, the header's contract gives {model.sig.stats()} "
                 f"(deferred, dropped, materialised, pending)")

    def check(op, a, rc, msg, out):
        """one call's return against the model; the model then makes the call"""
        name, p = op
        stats["ops"] += 1
        if out.get("twin_diff"):
            fail(f"{name}: {out['twin_diff']}")
        if model.cfg["custom"] and name in CUSTOM_REFUSED:
            if rc != VSOM_ERR_INVALID:
                fail(f"{name} on a custom context returned {rc}, not VSOM_ERR_INVALID")
            return check_sigma(op, out, True)
        if model.cfg["tr"] == po.CLR and name in CLR_REFUSED:
            if rc != VSOM_ERR_INVALID:
                fail(f"{name} on a CLR context returned {rc}, not VSOM_ERR_INVALID")
            return check_sigma(op, out, True)
        if model.cfg["tr"] == po.CLR and name == "distances_raw" and not p["from_map"]:
            # (Som::euclidianWeightedDistRaw against a sample needs depth == sample length: csrc/vsom_bmu.hip)
            if rc != VSOM_ERR_UNSUPPORTED:
                fail(f"{name} against chunk rows on a CLR context returned {rc}, not VSOM_ERR_UNSUPPORTED")
            return check_sigma(op, out, True)
        if name == "commit" and model.pending is None:
            if rc != VSOM_ERR_INVALID:
                fail(f"commit with nothing pending returned {rc}")
            return check_sigma(op, out, True)
        staged = rc == VSOM_ERR_INVALID and "commit" in msg and model.refusal_allowed(name, p)
        if name in ACCUM_OPS:
            why = model.accum_refusal(op)
            # (a chunk staged ahead is checked before the chunk and its rows)
            if why is not None and not (staged and why in ("no chunk loaded", "exceed total_rows")):
                if rc != VSOM_ERR_INVALID or why not in msg:
                    fail(f"{name} returned {rc} {msg!r}: the header refuses it ({why})")
                check_sigma(op, out, True)
                check_all(f"{name} refused ({why})")      # a refused call leaves everything as it was
                model.sig.read()                          # (vsom_get_state)
                return
            # run 5: where a prefetch right behind an asynchronous epoch stages ahead, the first chunk call of the epoch
            # opened behind it must be refused for the chunk staged ahead
            if run == 5 and stages_ahead(model.cfg) and name == "accum_chunk" and model.pending is not None and \
                    not (staged and "vsom_commit_chunk first" in msg):
                fail(f"{name} behind epoch_async, prefetch, begin returned {rc} {msg!r}: the next chunk is staged ahead over "
                     f"the current rows, the header refuses it (vsom_commit_chunk first)")
        if rc != 0:
            if staged:
                if run is not None and run != 5:
                    fail(f"{name} was refused inside run {run}, whose calls the header accepts: {msg}")
                stats["refused"] += 1
                check_sigma(op, out, True)
                if name in ACCUM_OPS:                     # as after every refusal of these calls
                    stats["accum"]["staged"] += 1
                    check_all(f"{name} refused (a chunk staged ahead)")
                    model.sig.read()
                return
            fail(f"{name} failed: {rc} {msg}")
        model.sig.accepted(op, model.B, model.N)
        exp = model.apply(op, a)
        check_outputs(name, out, exp)
        check_sigma(op, out, False)
        if name in ("accum_chunk", "accum_chunk_masked") and model.B:
            stats["accum"]["chunks"] += 1
            stats["accum"]["masked"] += name == "accum_chunk_masked"
        elif name in ("accum_end", "accum_abort"):
            stats["accum"][name[6:] + "s"] += 1
        # (the full state is read through vsom_get_state, which materialises: in the sigma profile only where the
        # op itself has just done so)
        if name in OBSERVE and (not sigma or name == "get_state"):
            check_all(name)

    def back_to_back(batch):
        """A no-wait run on a backend that can separate its first context from the twin (call_first / call_twin): every
        call of the run goes to the first context before the twin or the model sees one of them, so nothing but the
        calls' own host work stands between them.  The arguments come from a shadow of the model that follows the loads
        alone (a mask depends on the chunk's rows, not on the model's state); then the twin and the model replay the run,
        each call's return held against them."""
        shadow = copy.copy(model)
        made = []
        for op in batch:
            a = materialize(op, shadow)
            made.append((op, a) + tuple(be.call_first(op, a)))
            if made[-1][2] == 0 and op[0] in ("upload", "prefetch", "stage", "commit"):
                shadow.apply(op, a)
        for op, a, rc, msg, out in made:
            done.append(op)
            be.call_twin(op, a, rc, msg, out)
            check(op, a, rc, msg, out)

    try:
        todo = list(ops[1:])
        while todo:
            op = todo.pop(0)
            name, p = op
            if name in ("run", "run_end"):     # markers of generate_accum: no call
                done.append(op)
                run = p["id"] if name == "run" else None
                # (not where begin is refused: the whole-state comparison behind a refusal must follow its call at once)
                if run in NO_WAIT_RUNS and hasattr(be, "call_first") and accepts_accum(model.cfg):
                    n = [o[0] for o in todo].index("run_end")
                    back_to_back(todo[:n])
                    del todo[:n]
                continue
            done.append(op)
            a = materialize(op, model)
            rc, msg, out = be.call(op, a)
            check(op, a, rc, msg, out)
        check_all("end of walk")
        if sigma and hasattr(be, "observe_twin"):
            check_all("end of walk, the EAGER twin", be.observe_twin)     # (accum profile: EAGER and sequential)
    finally:
        be.close()
        model.close()
    return stats


# ---- the real library --------------------------------------------------------------------------------------------------
class GpuBackend:
    """the C ABI of libvsom_hip.so, called directly (the Python wrapper synchronises where the walk must not)"""

    def __init__(self, cfg_name, model):
        import vsom_amd
        from vsom_amd import capi
        import custom_hooks
        self.capi = capi
        self.L = capi.lib()
        cfg = config(cfg_name)
        if cfg["custom"]:
            depth, rlen = custom_hooks.shape("standard", cfg["J"])
            make = lambda: capi.Context(cfg["W"], cfg["H"], cfg["J"], capi.CUSTOM, source=custom_hooks.STANDARD,
                                        depth=depth, residual_len=rlen)
        else:
            make = lambda: vsom_amd.Context(cfg["W"], cfg["H"], cfg["J"], cfg["tr"])
        self.make = make                   # (the ensemble profile makes each member's twin with it)
        self.ctx = make()
        # sigma profile: a second context fixed at VSOM_SIGMA_EAGER that receives every call of the walk
        # accum profile: that twin is also the sequential one -- fed from pageable memory, synchronised after every call
        self.sigma = model.profile in ("sigma", "accum")
        self.accum = model.profile == "accum"
        self.custom = cfg["custom"]
        self.twin = None
        if self.sigma:
            self.twin = make()
            self.twin.set_sigma_mode(SIGMA_EAGER)
        self.N, self.D = self.ctx.n_nodes, self.ctx.depth
        # pinned and device copies of every chunk, made up front: an allocation inside the walk (hipHostMalloc,
        # hipMalloc + hipMemcpy) would synchronise the device and hide the asynchrony the walk is about
        self.hip = C.CDLL("libamdhip64.so")
        self.pinned, self.dev = [], []
        self.pinned_poisoned, self.dev_poisoned = {}, {}
        for X in model.chunks:
            pb, ptr = self._copies(X)
            self.pinned.append(pb)
            self.dev.append(ptr)
        for name, p in getattr(model, "ops", ()):      # the poisoned rows of every masked chunk call of the walk
            if "poisoned" in p and self._key(p) not in self.pinned_poisoned:
                self.pinned_poisoned[self._key(p)], self.dev_poisoned[self._key(p)] = self._copies(model.rows(p))

    @staticmethod
    def _key(p):
        return (p["chunk"],) + tuple(sorted(p["poisoned"].items()))

    def _copies(self, X):
        pb = self.capi.PinnedBuffer(X.shape)
        pb.array[...] = X
        ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(ptr), C.c_size_t(max(X.nbytes, 4))) == 0
        assert self.hip.hipMemcpy(ptr, X.ctypes.data_as(C.c_void_p), C.c_size_t(X.nbytes), C.c_int(1)) == 0
        return pb, ptr

    def close(self):
        self.ctx.close()
        if self.twin is not None:
            self.twin.close()
        for pb in self.pinned + list(self.pinned_poisoned.values()):
            pb.free()
        for p in self.dev + list(self.dev_poisoned.values()):
            self.hip.hipFree(p)

    def call(self, op, a):
        rc, msg, out = self.call_first(op, a)
        self.call_twin(op, a, rc, msg, out)
        return rc, msg, out

    def call_first(self, op, a):
        """the call on the first context alone (and vsom_sigma_stats, which reads host counters)"""
        rc, msg, out = self._call(self.ctx, op, a)
        if self.sigma:
            out["sigma_stats"] = tuple(self.ctx.sigma_stats()[k] for k in ("deferred", "dropped", "materialised", "pending"))
        return rc, msg, out

    def call_twin(self, op, a, rc, msg, out):
        """the same call on the twin, compared with what the first context returned (out["twin_diff"])"""
        name = op[0]
        # The sequential twin never has a chunk staged ahead (vsom_synchronize ends the window in which a prefetch stages
        # ahead), so a call the first context refuses for one is not made on the twin: it changes nothing on either.
        if self.accum and rc == VSOM_ERR_INVALID and name in READS_ROWS and "vsom_commit_chunk first" in msg:
            return
        if self.sigma:
            trc, _, tout = self._call(self.twin, op, a, twin=self.accum)
            if name == "sigma_mode":                   # (the twin stays eager)
                self.twin.set_sigma_mode(SIGMA_EAGER)
            if trc != rc:
                out["twin_diff"] = f"returned {rc}, the EAGER twin {trc}"
            elif rc == 0 and name in (ACCUM_TWIN_COMPARED if self.accum else TWIN_COMPARED):
                for k in tout:
                    d = first_difference_exact(out.get(k), tout[k])
                    if d:
                        out["twin_diff"] = f"output {k!r} differs from the EAGER twin's at {d}"
                        break

    def _wrapped(self, fn, *args, **kw):
        """a call through the Python wrapper: (rc, what it returned as a dict)"""
        try:
            res = fn(*args, **kw)
        except self.capi.VsomError as e:
            return int(str(e).split("error ", 1)[1].split(":", 1)[0]), {}
        if isinstance(res, tuple):
            res = {f"r{i}": v for i, v in enumerate(res)}
        elif not isinstance(res, dict):
            res = {"r0": res}
        return 0, res

    def _call(self, ctx, op, a, twin=False):
        """the call on ctx; twin: as the sequential twin makes it -- rows from pageable memory only (a blocking upload, a
        prefetch from pageable memory, also for a chunk the walk hands over in HBM), vsom_synchronize behind the call"""
        rc, msg, out = self._call1(ctx, op, a, twin)
        if twin:
            self.capi.check(self.L.vsom_synchronize(ctx._h))
        return rc, msg, out

    def _call1(self, ctx, op, a, twin):
        L, h, capi = self.L, ctx._h, self.capi
        f, u = capi._f, capi._u
        name, p = op
        out = {}
        B = int(L.vsom_chunk_size(h))
        if name in ("similarity", "generate", "evaluate", "topk", "bmd", "bmu_masked", "topk_masked", "bmd_masked",
                    "generate_masked") or name in MASKED_SCORES:
            w = dict(r0=p["r0"], r1=p["r1"])
        if "poisoned" in p:                    # (one entry, under the chunk's index)
            pinned = {p["chunk"]: self.pinned_poisoned[self._key(p)]}
            dev = {p["chunk"]: self.dev_poisoned[self._key(p)]}
        else:
            pinned, dev = self.pinned, self.dev
        # the five calls of the accumulated epoch go to the C ABI as they are: the wrapper copies and converts
        if name == "accum_begin":
            rc = L.vsom_batch_accum_begin(h, p["sigma"], int(p["first"]), p["total"])
        elif name == "accum_chunk":
            rc = L.vsom_batch_accum_chunk(h)
        elif name == "accum_chunk_masked":
            if a["valid"] is None:
                rc = L.vsom_batch_accum_chunk_masked(h, None, 0)
            else:
                vb = a["valid"].copy()
                rc = L.vsom_batch_accum_chunk_masked(h, vb.ctypes.data_as(C.POINTER(C.c_uint8)), int(vb.ndim == 1))
                vb[...] = 0                    # "not read after the call returns": the chunk is still in flight
        elif name == "accum_end":
            m = C.c_float()
            rc = L.vsom_batch_accum_end(h, C.byref(m))
            out["mse"] = np.float32(m.value)
        elif name == "accum_abort":
            rc = L.vsom_batch_accum_abort(h)
        # the single-context ops of the ensemble profile
        elif name in ("schedule", "schedule_masked"):
            sg = np.array([np.nan if v is None else v for v in p["sigmas"]], np.float64)
            mses = np.zeros(sg.size, np.float32)
            dp = sg.ctypes.data_as(C.POINTER(C.c_double))
            if name == "schedule":
                rc = L.vsom_batch_schedule(h, dp, sg.size, int(p["reset"]), f(mses))
            else:
                vb = np.ascontiguousarray(a["valid"], np.uint8).copy()
                rc = L.vsom_batch_schedule_masked(h, dp, sg.size, int(p["reset"]), vb.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  int(vb.ndim == 1), f(mses))
                vb[...] = 0
            out["mses"] = mses
        elif name == "online_masked":
            vb = np.ascontiguousarray(a["valid"], np.uint8).copy()
            lb, m = np.zeros(B, np.uint64), C.c_float()
            rc = L.vsom_train_online_chunk_masked(h, p["eta"], p["sigma"], p["decay"], int(p["first"]),
                                                  vb.ctypes.data_as(C.POINTER(C.c_uint8)), int(vb.ndim == 1), u(lb), C.byref(m))
            vb[...] = 0
            out.update(lb=lb, mse=np.float32(m.value))
        elif name in ("um", "get_umatrix"):
            um = np.zeros(self.N, np.float64)
            rc = getattr(L, "vsom_umatrix" if name == "um" else "vsom_get_umatrix")(h, um.ctypes.data_as(C.POINTER(C.c_double)))
            out["u"] = um
        elif name == "update_mode":
            rc = L.vsom_set_update_mode(h, p["mode"])
        elif name == "similarity_masked":
            rc, out = self._wrapped(ctx.similarity_masked, a["valid"], p["min_hits"], 2, p["rule"], delta=True, **w)
        elif name == "evaluate_masked":
            rc, out = self._wrapped(ctx.evaluate_masked, a["valid"], a["binary"], a["continuous"], p["min_hits"], **w)
        elif name == "sigma_mode":
            rc = L.vsom_set_sigma_mode(h, SIGMA_MODES[p["mode"]])
        elif name == "sigma_flush":
            rc = L.vsom_sigma_flush(h)
        elif name == "compaction":
            rc = L.vsom_set_column_compaction(h, C.c_long(p["min_rows"]))
        elif name == "upload_empty":
            rc = L.vsom_upload_chunk(h, f(a["X"]), 0)
        elif name == "epoch_masked":
            rc, out = self._wrapped(ctx.batch_epoch_masked, p["sigma"], p["first"], a["valid"])
            out = {"mse": out.get("r0")}
        elif name == "similarity":
            rc, out = self._wrapped(ctx.similarity, p["min_hits"], 2, p["rule"], delta=True, **w)
        elif name == "generate":
            rc, out = self._wrapped(ctx.generate, p["min_hits"], a["u"], a["l"], p["rule"], **w)
        elif name == "decode_nodes":
            rc, out = self._wrapped(ctx.decode_nodes, a["nodes"], a["l"])
        elif name == "distances_raw":
            rc, out = self._wrapped(ctx.distances_raw, a["nodes"], a["vrows"], p["from_map"])
        elif name == "umatrix":
            rc, out = self._wrapped(ctx.umatrix)
        elif name == "evaluate":
            rc, out = self._wrapped(ctx.evaluate, a["binary"], a["continuous"], **w)
        elif name == "topk":
            rc, out = self._wrapped(ctx.bmu_topk, p["k"], **w)
        elif name == "bmd":
            rc, out = self._wrapped(ctx.restricted_bmd, p["min_hits"], u=a["u"], **w)
        elif name == "bmu_masked":
            rc, out = self._wrapped(ctx.bmu_masked, a["valid"], min_hits=p["min_hits"], fill=True, **w)
        elif name == "topk_masked":
            rc, out = self._wrapped(ctx.bmu_topk_masked, p["k"], a["valid"], min_hits=p["min_hits"], blend=p["blend"], **w)
        elif name == "bmd_masked":
            rc, out = self._wrapped(ctx.restricted_bmd_masked, a["valid"], p["min_hits"], u=a["u"], probs=True, **w)
        elif name == "generate_masked":
            rc, out = self._wrapped(ctx.generate_masked, a["valid"], p["min_hits"], a["u"], a["l"], draws=p["draws"], **w)
        elif name == "upload":
            X = a["X"]
            if p["asynchronous"] and not twin:
                X = pinned[p["chunk"]].array
                rc = L.vsom_upload_chunk_async(h, f(X), X.shape[0])
            else:
                rc = L.vsom_upload_chunk(h, f(X), X.shape[0])
        elif name == "prefetch":
            X = a["X"] if p["src"] == "pageable" or twin else pinned[p["chunk"]].array
            rc = L.vsom_prefetch_chunk(h, f(X), X.shape[0])
        elif name == "stage" and twin and not self.custom:        # (a custom context refuses the hand-over: the twin too)
            rc = L.vsom_prefetch_chunk(h, f(a["X"]), a["X"].shape[0])
        elif name == "stage":
            rc = L.vsom_stage_next_device(h, C.c_void_p(dev[p["chunk"]].value), a["X"].shape[0])
        elif name == "commit":
            rc = L.vsom_commit_chunk(h)
        elif name == "epoch_async":
            rc = L.vsom_batch_epoch_async(h, p["sigma"], int(p["first"]))
        elif name == "epoch":
            m = C.c_float()
            rc = L.vsom_batch_epoch(h, p["sigma"], int(p["first"]), C.byref(m))
            out["mse"] = np.float32(m.value)
        elif name == "p1":
            rc = L.vsom_batch_phase1_async(h, p["s0"], p["s1"], int(p["first"]))
        elif name == "finish":
            rc = L.vsom_batch_finish_async(h)
        elif name == "p2":
            rc = L.vsom_batch_phase2_async(h, p["sigma"], p["n0"], p["n1"])
        elif name == "online":
            m = C.c_float()
            if p["mode"] == "fetch":
                lb = np.zeros(B, np.uint64)
                rc = L.vsom_train_online_chunk_fetch(h, p["eta"], p["sigma"], p["decay"], int(p["first"]), u(lb),
                                                     C.byref(m))
                out["lb"] = lb
            else:
                rc = L.vsom_train_online_chunk_acc(h, p["eta"], p["sigma"], p["decay"], int(p["first"]),
                                                   C.byref(m) if p["mode"] == "mse" else None)
            out["mse"] = np.float32(m.value)
        elif name == "single":
            res = np.empty(int(L.vsom_residual_len(h)), np.float32)
            lb, bmu, dist = C.c_uint64(p["last"]), C.c_uint64(), C.c_float()
            rc = L.vsom_train_single(h, f(a["v"]), p["eta"], p["sigma"], C.byref(lb), p["decay"], f(res),
                                     C.byref(dist), C.byref(bmu))
            out.update(bmu=int(bmu.value), res=res, dist=np.float32(dist.value), last=int(lb.value))
        elif name in ("bmu", "bmu_local", "bmu_restricted"):
            idx, dist = np.empty(B, np.uint64), np.empty(B, np.float32)
            if name == "bmu":
                rc = L.vsom_bmu_batch(h, u(idx), f(dist))
            elif name == "bmu_local":
                rc = L.vsom_bmu_local_batch(h, u(idx), f(dist))
            else:
                rc = L.vsom_bmu_restricted_batch(h, p["min_hits"], u(idx), f(dist))
            out.update(idx=idx, dist=dist)
        elif name == "distances":
            d = np.empty(a["nodes"].size, np.float32)
            rc = L.vsom_distances(h, u(a["nodes"]), u(a["rows"]), a["nodes"].size, f(d))
            out["d"] = d
        elif name == "distances_row":
            d = np.empty(self.N, np.float32)
            rc = L.vsom_distances_row(h, p["row"], f(d))
            out["d"] = d
        elif name == "set_last_bmu":
            rc = L.vsom_set_last_bmu(h, u(a["idx"]))
        elif name == "get_last_bmu":
            lb = np.empty(B, np.uint64)
            rc = L.vsom_get_last_bmu(h, u(lb))
            out["lb"] = lb
        elif name == "get_sqres":
            sq = np.empty(B, np.float32)
            rc = L.vsom_get_sqres(h, f(sq))
            out["sq"] = sq
        elif name == "get_mse":
            m = C.c_float()
            rc = L.vsom_get_mse(h, C.byref(m))
            out["mse"] = np.float32(m.value)
        elif name == "bmu_mode":
            rc = L.vsom_set_bmu_mode(h, p["mode"])
        elif name == "set_state":
            g = lambda k: a.get(k)
            rc = L.vsom_set_state(h, f(g("map")), f(g("sigma")), f(g("S")), f(g("weight")), u(g("hits")))
        elif name == "get_state":
            out = self._state(ctx)
            rc = 0 if out is not None else -1
        else:
            raise ValueError(name)
        msg = "" if rc == 0 else L.vsom_last_error().decode(errors="replace")
        return rc, msg, out

    def _state(self, ctx=None):
        h = (ctx or self.ctx)._h
        N, D = self.N, self.D
        st = {"map": np.empty((N, D), np.float32), "sigma": np.empty((N, D), np.float32),
              "S": np.empty((N, D), np.float32), "weight": np.empty(N, np.float32), "hits": np.empty(N, np.uint64)}
        f, u = self.capi._f, self.capi._u
        self.capi.check(self.L.vsom_get_state(h, f(st["map"]), f(st["sigma"]), f(st["S"]), f(st["weight"]),
                                              u(st["hits"])))
        return st

    def observe_twin(self):
        return self.observe(self.twin)

    def observe(self, ctx=None):
        ctx = ctx or self.ctx
        st = self._state(ctx)
        lb = np.empty(int(self.L.vsom_chunk_size(ctx._h)), np.uint64)
        self.capi.check(self.L.vsom_get_last_bmu(ctx._h, self.capi._u(lb)))
        m = C.c_float()
        self.capi.check(self.L.vsom_get_mse(ctx._h, C.byref(m)))
        st.update(lb=lb, mse=np.float32(m.value))
        return st


def replay(ops):
    """rerun a printed op list against the real library"""
    if ops[0][1].get("profile") in ("ensemble", "ensemble_query"):
        return run_ensemble_walk(ops, EnsGpuBackend)
    return run_walk(ops, GpuBackend)


# ---- the ensemble profile ----------------------------------------------------------------------------------------------
# The nine calls of include/vsom_hip.h, "ensembles", walked with the single-context calls on their members between them.
# An op is ("ens_*", params) for an ensemble call -- params["e"] names the ensemble, per-member values are lists in the
# order given to create --, ("m", {"k": member, "op": (name, params)}) for a single-context call on one member (Model.apply
# and GpuBackend._call1 serve it), ("ens_create", {"e", "order"}), ("ens_destroy", {"e"}) or ("sigma_stats", {"k", "expect"}).
# The model (EnsModel) keeps one Model per member: an accepted ensemble call is the single call on every member in index
# order, a refused one names the member the header says and changes nothing.  generate_ensemble's docstring lists the runs.
ENS_CALLS = ("ens_upload", "ens_online", "ens_online_masked", "ens_epoch", "ens_epoch_masked", "ens_schedule",
             "ens_schedule_masked", "ens_bmu", "ens_umatrix")
ENS_TRAIN = ENS_CALLS[1:7]
ENS_NEW_OPS = set(ENS_CALLS) | {"ens_create", "ens_destroy", "m", "sigma_stats", "schedule", "schedule_masked",
                                "online_masked", "um", "get_umatrix"}
ENS_MASKABLE = ("A", "A2", "B", "D")     # the members the masked calls name (the model's masked searches are pure Python)
ENS_DRAWS = 10                           # random draws of an ensemble walk, around its runs
ENS_RUNS = tuple(range(1, 10))
ENS_REFUSALS = ("null", "no_chunk", "decay", "masked_clr", "non_strict", "offset", "member_online_masked",
                "member_accum_begin")                              # run 5, every configuration
ENS_REFUSALS_OWN = ("masked_custom", "umatrix_custom")             # ... those that need the custom member F


def batch_tiny(cfg, B):
    """vsom_tiny_applies (csrc/vsom_tiny.hip:52): the batch epoch of this chunk takes the one-launch kernel --
    0 < B <= 256, N * part_len <= 4096 (part_len: D, or D / 2 for CLR), B * N <= 16384, N * part_len * B <= 262144; never
    a custom context."""
    N, D = cfg["W"] * cfg["H"], po.length(cfg["tr"], cfg["J"])
    chains = N * (D // 2 if cfg["tr"] == po.CLR else D)
    return not cfg["custom"] and 0 < B <= 256 and chains <= 4096 and B * N <= 16384 and chains * B <= 262144


def masked_batch_tiny(cfg, B, strict=True):
    """vsom_masked_tiny_applies (csrc/vsom_tiny_masked.hip:114, vsom_tiny_masked_applies): batch_tiny on a Standard / Median
    context in the strict update mode.  (Its LDS bound, 64 KiB, holds for every member of ENS_MEMBERS: at most 256 rows of
    24 bytes, a table of at most 23 x 23 floats, J * ceil(B / 32) words, and the rows only when B * J <= 10240.)"""
    return batch_tiny(cfg, B) and cfg["tr"] != po.CLR and strict


def online_tiny(cfg, B, sigma, mode=BMU_AUTO):
    """vsom_online_masked_tiny_applies as include/vsom_hip.h:933 states it (vsom_onl_tiny_fits, csrc/vsom_online_tiny.hip), which is
    the unmasked one-launch chunk's rule too: Standard / Median, not custom, N <= 1024, N * D <= 4096, D <= 512,
    B <= 4096, sigma no NaN, the search mode VSOM_BMU_AUTO.  (The LDS need of every member here is within 96 KiB.)"""
    N, D = cfg["W"] * cfg["H"], po.length(cfg["tr"], cfg["J"])
    return cfg["tr"] != po.CLR and not cfg["custom"] and N <= 1024 and N * D <= 4096 and D <= 512 and 0 < B <= 4096 and \
        sigma == sigma and mode == BMU_AUTO


def ens_mask(spec, X):
    """the validity bytes a masked call gives a member whose rows are X: accum_mask's engineered mask with every late
    column active -- the border columns, one column valid in no row, spec["full"]: one row without a valid column"""
    return np.ascontiguousarray(accum_mask(spec["seed"], 2, spec["form"], spec.get("full", False), X), np.uint8)


def ens_poisoned(spec, X):
    """X with NaN / +-inf under every invalid entry of ens_mask(spec, X), and nowhere else"""
    return poisoned_rows(X, spec["seed"], 2, spec["form"], spec.get("full", False))


def _nan(v):
    return float("nan") if v is None else v


class _EnsGen:
    def __init__(self, cfg_name, seed):
        self.ec = ens_config(cfg_name)
        self.all = list(self.ec["members"])
        self.rs = np.random.RandomState(seed)
        self.sizes = {n: [b for b, _ in config(n)["chunks"]] for n in self.all}
        self.B = {n: None for n in self.all}
        self.chain = {n: False for n in self.all}
        self.ens = {}
        self.uid = 0
        self.ops = []

    def r(self, n):
        return int(self.rs.randint(n))

    def sigma(self):
        return float(self.rs.choice([0.7, 1.0, 2.5, 6.0]))

    def emit(self, name, **p):
        self.ops.append((name, p))

    def m(self, k, name, **p):
        self.ops.append(("m", {"k": k, "op": (name, p)}))
        if name == "upload":
            self.B[k] = self.sizes[k][p["chunk"]]
        if name == "online":
            self.chain[k] = True
        elif name in ("epoch", "epoch_async", "schedule", "schedule_masked", "online_masked") or name in ACCUM_OPS:
            self.chain[k] = False

    # ---- ensemble calls ----
    def small(self, n):
        """a chunk of member n for a random draw: never E's 1100 rows nor G's 300 (the model's dearest: once per walk)"""
        return self.r(2 if n == "E" else (1 if n == "G" else len(self.sizes[n])))

    def upload(self, e=0, pick=None, wait=1, poison=None, share=None, bad=None):
        """vsom_ensemble_upload_chunks: pick[n] the chunk of member n (else drawn), poison[n] the masked call its rows are
        made for, share = (n, rows): A2 names the first `rows` rows of A's range (equal offsets)"""
        rows = {}
        for n in self.ens[e]:
            rows[n] = {"chunk": int((pick or {}).get(n, self.small(n)))}
        if share and "A" in rows and "A2" in rows:
            rows["A2"] = {"share": "A", "n": int(min(share, self.sizes["A"][rows["A"]["chunk"]]))}
        p = dict(e=e, uid=self.uid, wait=int(wait), rows=rows)
        self.uid += 1
        if poison:
            p["poison"] = {n: s for n, s in poison.items() if n in rows}
        if bad:
            p["bad"] = bad
        self.emit("ens_upload", **p)
        if not bad:
            for n, s in rows.items():
                self.B[n] = s["n"] if "share" in s else self.sizes[n][s["chunk"]]

    def specs(self, e, names=None, full=None):
        """a mask per masked member: both forms, `full` gets the row without a valid column; the others stay plain
        (valid_host[k] = NULL)"""
        names = [n for n in self.ens[e] if n in (names or ENS_MASKABLE)]
        out = {}
        for i, n in enumerate(names):
            out[n] = {"seed": self.r(1 << 30), "form": ["rows", "one_mask"][(i + self.r(2)) % 2 if i else 0]}
            if n == full:
                out[n]["form"] = "rows"
                out[n]["full"] = True
        return out

    def per(self, e, f):
        return [f() for _ in self.ens[e]]

    def train(self, kind, e=0, masks=None, first=True, sigmas=None, reset=None, bad=None, must_refuse=None):
        K = len(self.ens[e])
        p = dict(e=e)
        if kind in ("ens_epoch", "ens_epoch_masked"):
            p.update(sigma=self.per(e, self.sigma), first=bool(first))
        elif kind in ("ens_schedule", "ens_schedule_masked"):
            p.update(sigmas=sigmas if sigmas is not None else [[self.sigma() for _ in range(1 + self.r(2))] for _ in range(K)],
                     reset=bool(self.r(2) if reset is None else reset))
        else:
            p.update(eta=self.per(e, lambda: float(self.rs.choice([0.05, 0.2]))), sigma=self.per(e, self.sigma),
                     decay=self.per(e, lambda: self.r(2)), first=bool(first))
        if kind.endswith("_masked"):
            p["masks"] = masks if masks is not None else {}
        if kind == "ens_online_masked":
            # (the model's masked chunk is pure Python: on more than 40 rows the local walk, sigma <= 1, not the full scan)
            # (and D's 512 columns on 3 rows only)
            p["masks"] = {n: s for n, s in p["masks"].items() if n != "D" or (self.B[n] or 0) <= 40}
            for k, n in enumerate(self.ens[e]):
                if n in p["masks"]:          # (the full scan, sigma > 1, with a window of a few nodes)
                    p["sigma"][k] = [0.7, 1.0 if (self.B[n] or 0) > 40 else 1.5][self.r(2)]
        if bad:
            p["bad"] = bad
        if must_refuse:
            p["must_refuse"] = must_refuse
        self.emit(kind, **p)
        if bad or must_refuse:
            return
        for n in self.ens[e]:
            if kind in ("ens_schedule", "ens_schedule_masked") and not p["sigmas"][self.ens[e].index(n)]:
                continue
            self.chain[n] = kind in ("ens_online", "ens_online_masked")

    def can_chain(self, e):
        return all(self.chain[n] for n in self.ens[e])

    def masked_block(self, kinds, e=0, pick=None, names=None, full=None, first=True, wait=1):
        """rows poisoned for the masked members' masks, the masked calls, clean rows again"""
        masks = self.specs(e, names, full)
        self.upload(e, pick, wait=wait, poison=masks)
        for kind in kinds:
            self.train(kind, e, masks=masks, first=first)
        return masks

    # ---- random draws ----
    def member_op(self):
        n = self.all[self.r(len(self.all))]
        cfg = config(n)
        plain = not cfg["custom"] and cfg["tr"] != po.CLR
        what = ["upload", "prefetch", "set_state", "get_state", "set_last_bmu", "get_last_bmu", "get_sqres", "get_mse",
                "epoch", "online", "bmu", "bmu_masked", "um", "bmu_mode", "schedule", "schedule_masked"][self.r(16)]
        if what == "upload":
            self.m(n, "upload", chunk=self.small(n), asynchronous=bool(self.r(2)))
        elif what == "prefetch":
            c = self.small(n)
            self.m(n, "prefetch", chunk=c, src=["pinned", "pageable"][self.r(2)])
            self.m(n, "commit")
            self.B[n] = self.sizes[n][c]
        elif what == "set_state":
            self.m(n, "set_state", seed=self.r(1 << 30), parts=["map_only", "weight_only", "msw"][self.r(3)])
        elif what == "epoch":
            self.m(n, "epoch", sigma=self.sigma(), first=bool(self.r(2)))
        elif what == "online":
            first = True if not self.chain[n] else bool(self.r(2))
            self.m(n, "online", eta=0.1, sigma=self.sigma(), decay=self.r(2), first=first, mode=["mse", "fetch", "null"][self.r(3)])
        elif what == "set_last_bmu":
            self.m(n, "set_last_bmu", seed=self.r(1 << 30))
        elif what == "bmu_masked":
            if plain and n in ENS_MASKABLE:
                k = 1 + self.r(min(32, self.B[n]))
                r0 = self.r(self.B[n] - k + 1)
                self.m(n, "bmu_masked", min_hits=self.r(2), rule=self.r(2), seed=self.r(1 << 30), r0=r0, r1=r0 + k)
        elif what == "um":
            if not cfg["custom"]:
                self.m(n, "um")
                self.m(n, "get_umatrix")
        elif what == "bmu_mode":
            if not cfg["custom"]:
                self.m(n, "bmu_mode", mode=self.r(3))
                self.m(n, "online", eta=0.1, sigma=2.5, decay=0, first=True, mode="mse")
                self.m(n, "bmu_mode", mode=BMU_AUTO)
        elif what == "schedule":
            if n not in ("E", "G"):
                self.m(n, "schedule", sigmas=[self.sigma() for _ in range(self.r(3))], reset=bool(self.r(2)))
        elif what == "schedule_masked":
            if n in ENS_MASKABLE:
                self.m(n, "schedule_masked", sigmas=[self.sigma()], reset=True, seed=self.r(1 << 30),
                       form=["rows", "one_mask"][self.r(2)])
        else:
            self.m(n, what)

    def random_op(self, e=0):
        what = ["epoch", "schedule", "online", "bmu", "umatrix", "upload", "masked", "member", "member", "member"][self.r(10)]
        if what == "epoch":
            self.train("ens_epoch", e, first=bool(self.r(2)))
        elif what == "schedule":
            self.train("ens_schedule", e)
        elif what == "online":
            self.train("ens_online", e, first=True if not self.can_chain(e) else bool(self.r(2)))
        elif what == "bmu":
            self.emit("ens_bmu", e=e)
        elif what == "umatrix":
            if "F" not in self.ens[e]:
                self.emit("ens_umatrix", e=e)
                n = self.ens[e][self.r(len(self.ens[e]))]
                self.m(n, "get_umatrix")
        elif what == "upload":
            self.upload(e, wait=self.r(2), share=[None, 20, 160][self.r(3)])
        elif what == "masked":
            kind = ["ens_epoch_masked", "ens_schedule_masked", "ens_online_masked"][self.r(3)]
            two = [n for n in self.ens[e] if n in ENS_MASKABLE]
            self.rs.shuffle(two)
            self.masked_block([kind], e, names=two[:2], pick={n: 0 for n in two}, first=True)
            self.upload(e)
        else:
            self.member_op()

    # ---- the runs ----
    def run(self, run):
        own = not self.ec["one_stream"]
        e = 0
        self.upload(e, wait=1)               # (every run starts from clean rows)
        self.emit("run", id=run)
        if run == 1:
            pick = {"A": 1, "A2": 0, "B": 1, "C": 0, "D": 1, "E": 0, "F": 0, "G": 0}
            masks = self.specs(e, full="A")
            self.upload(e, pick, wait=0, poison=masks)
            self.train("ens_epoch_masked", e, masks=masks, first=True)
            self.emit("ens_bmu", e=e)
            if not own:
                self.emit("ens_umatrix", e=e)
            self.train("ens_schedule_masked", e, masks=masks,       # (one masked epoch of the model on the long chunks)
                       sigmas=[[self.sigma()] * (1 if n in ("A", "B") else 2) for n in self.ens[e]])
            self.train("ens_online_masked", e, masks=masks, first=True)
            big = {"A": 3, "A2": 3, "B": 2, "C": 1, "D": 1, "E": 2, "F": 1, "G": 1}
            self.upload(e, big, wait=0)      # more floats than the first: the raw buffer grows behind the stagings
            self.train("ens_epoch", e, first=True)
        elif run == 2:
            self.train("ens_online", e, first=True)
            x, y = "A", "B"
            self.m(x, "upload", chunk=self.r(2), asynchronous=False)
            self.m(y, "upload", chunk=0, asynchronous=bool(self.r(2)))
            self.m(x, "online", eta=0.1, sigma=self.sigma(), decay=self.r(2), first=False, mode="mse")
            self.train("ens_online_masked", e, masks=self.specs(e, names=(x, y, "D")), first=False)
            for n in self.ens[e]:
                self.m(n, "get_mse")
        elif run == 3:
            steps = [{"A": 1, "B": 1}, {"A": 2, "B": 2}, {"A": 1, "B": 3}]
            for i, pick in enumerate([{"A": 1, "B": 3}, {"A": 2, "B": 4}, {"A": 1, "B": 3}]):
                pick = dict(pick, A2=0, D=1, E=0, G=0)
                masks = self.specs(e, names=("A", "B"))
                self.upload(e, pick, poison=masks)
                self.train("ens_epoch_masked", e, masks=masks, first=i == 0)
                if i < 2:
                    self.train("ens_schedule_masked", e, masks=masks, reset=False,
                               sigmas=[[self.sigma()] if n != "E" or i else [2.5, None] for n in self.ens[e]])
                    if i == 0:               # (a plain member's NaN sigma: its map is NaN now)
                        self.m("E", "get_state")
                        self.m("E", "set_state", seed=self.r(1 << 30), parts="all")
                self.train("ens_online_masked", e, masks=masks, first=True)
            for i, pick in enumerate(steps):
                self.upload(e, dict(pick, E=0, G=0), share=[160, None, 20][i])
                self.train("ens_epoch", e, first=i == 0)
                idle = self.ens[e][self.r(len(self.ens[e]))]
                sig = [[self.sigma() for _ in range(1 + self.r(2))] if n != idle else [] for n in self.ens[e]]
                if i == 1 and idle != "A":
                    sig[self.ens[e].index("A")] = [2.5, None]
                self.train("ens_schedule", e, sigmas=sig, reset=bool(i % 2))
                for what in ("get_last_bmu", "get_sqres", "get_mse"):    # epochs[k] = 0: not touched
                    self.m(idle, what)
                if i == 1 and idle != "A":
                    self.m("A", "get_state")
                    self.m("A", "set_state", seed=self.r(1 << 30), parts="all")
                self.train("ens_online", e, first=True)
            self.m("A", "bmu_mode", mode=BMU_EXACT)
            self.train("ens_online", e, first=False)
            self.train("ens_online_masked", e, masks=self.specs(e, names=("A", "B")), first=True)
            self.m("A", "bmu_mode", mode=BMU_AUTO)
            self.train("ens_online", e, first=True)
        elif run == 4:
            k = "G" if own else "E"
            ahead = k if stages_ahead(ENS_MEMBERS[k]) else None
            self.m(k, "upload", chunk=0, asynchronous=False)
            self.m(k, "epoch_async", sigma=self.sigma(), first=True)
            self.m(k, "prefetch", chunk=0, src="pinned")
            if ahead:                        # every row-reading call MUST be refused, naming the member
                for kind in ENS_TRAIN:
                    self.train(kind, e, masks={}, must_refuse=ahead)
                self.emit("ens_bmu", e=e, must_refuse=ahead)
            else:                            # (nothing is staged ahead: the calls take the old chunk)
                self.emit("ens_bmu", e=e)
            self.upload(e, {k: 0})           # accepted, as the header says
            self.m(k, "commit")
            self.train("ens_epoch", e, first=True)
            self.emit("ens_bmu", e=e)
        elif run == 5:
            K = len(self.ens[e])
            self.train("ens_epoch", e, bad="null")
            self.train("ens_online_masked", e, bad="null_valid")
            self.train("ens_schedule", e, bad="null_epochs")
            self.train("ens_schedule", e, bad="null_sigma", sigmas=[[1.0]] * K)
            self.upload(e, bad="null")
            self.upload(e, bad="offset")
            self.train("ens_online", e, bad="decay")
            c = {"C": {"seed": 5, "form": "rows"}}
            self.train("ens_epoch_masked", e, masks=c)
            self.train("ens_schedule_masked", e, masks=dict(c, A={"seed": 6, "form": "one_mask"}))
            self.train("ens_online_masked", e, masks=c)
            if own:
                f = {"F": {"seed": 5, "form": "rows"}}
                self.train("ens_epoch_masked", e, masks=f)
                self.train("ens_online_masked", e, masks=f)
                self.emit("ens_umatrix", e=e)
            a = {"A": {"seed": 7, "form": "rows"}}
            self.m("A", "update_mode", mode=UPDATE_FMA)
            self.train("ens_epoch_masked", e, masks=a)
            self.train("ens_schedule_masked", e, masks=a)
            self.m("A", "update_mode", mode=UPDATE_STRICT)
            self.m("B", "online_masked", eta=0.1, sigma=2.5, decay=0, first=True, seed=3, form="rows")
            self.m("A", "accum_begin", sigma=2.5, first=True, total=self.B["A"])
        elif run == 6:
            self.m("A", "set_state", seed=self.r(1 << 30), parts="map_only")
            self.m("B", "set_state", seed=self.r(1 << 30), parts="weight_only")
            self.m("E", "set_last_bmu", seed=self.r(1 << 30))
            self.m("A", "set_last_bmu", seed=self.r(1 << 30))
            self.train("ens_epoch", e, first=False)
            self.m("B", "set_last_bmu", seed=self.r(1 << 30))
            self.train("ens_schedule_masked", e, masks=self.specs(e, names=("B",)), reset=False,
                       sigmas=[[self.sigma(), self.sigma()] for _ in self.ens[e]])
            self.m("B", "get_last_bmu")
        elif run == 7:
            old = list(self.ens[0])
            self.emit("ens_destroy", e=0)
            del self.ens[0]
            for n in old[:3]:
                self.m(n, "epoch", sigma=self.sigma(), first=True)
            if own:                          # a former member stays eager: the deferred count does not move
                self.m("G", "epoch_async", sigma=self.sigma(), first=True)
                self.emit("sigma_stats", k="G", expect=[1, 0, 1, 0])
            sub = [n for n in old if n != ("F" if own else "C")]
            sub = [sub[i] for i in self.rs.permutation(len(sub))]
            self.emit("ens_create", e=0, order=sub)
            self.ens[0] = sub
            self.emit("ens_umatrix", e=0)
            self.m(sub[0], "get_umatrix")
            self.ens[1] = [sub[2], sub[0], old[-1] if old[-1] not in (sub[0], sub[2]) else sub[1]]
            self.emit("ens_create", e=1, order=self.ens[1])
            for _ in range(2):
                self.train("ens_epoch", 0, first=bool(self.r(2)))
                self.train("ens_online", 1, first=True)
                self.emit("ens_bmu", e=0)
                self.train("ens_schedule", 1)
            self.upload(1)
            self.train("ens_epoch", 1, first=True)
            self.emit("ens_destroy", e=1)
            del self.ens[1]
            self.train("ens_epoch", 0, first=False)
            self.emit("ens_umatrix", e=0)
            self.m(sub[1], "get_umatrix")
        self.emit("run_end", id=run)
        self.m(self.all[self.r(len(self.all))], "get_state")


def generate_ensemble(cfg_name, seed, n_ops=ENS_DRAWS):
    """The ensemble profile: n_ops random draws (ensemble calls, masked blocks, single-context calls on members) around
    these runs, each between ("run", id) / ("run_end", id) markers.  Runs 8, 9 and the refusal for a member without a chunk
    open the walk (they need contexts that have not joined yet); runs 1-6 follow in a drawn order, run 7 ends the walk.
      1  back to back: upload_chunks(wait = 0) of poisoned rows from pinned memory, batch_epoch_masked, bmu_batch, umatrix
         (ens_shared), batch_schedule_masked, train_online_chunk_masked; a second, larger upload_chunks(wait = 0) -- the raw
         buffer grows behind the stagings --, batch_epoch.  Six descriptor sizes through two slots.
      2  the running MSE: ensemble online (first_chunk = 1), new rows for A and B by their own uploads, a single online chunk
         with first = 0 on A, the ensemble masked online with first_chunk = 0; every member's vsom_get_mse
      3  path borders between two calls of each kind: A 160 -> 170 -> 160 rows, B 121 -> 122 -> 121 (masked calls) and
         151 -> 152 -> 121 (plain calls); A's search mode EXACT, then AUTO; one schedule with a NaN sigma; a member with
         epochs[k] = 0, whose lastBMU, sqres and MSE word are read
      4  the stage-ahead: an asynchronous epoch and a prefetch on G (ens_own; E on ens_shared, where nothing stages ahead);
         where stages_ahead holds every row-reading ensemble call MUST be refused naming the member; upload_chunks is
         accepted; after the commit the calls are accepted
      5  every refusal the header lists, and vsom_train_online_chunk_masked / vsom_batch_accum_begin on a member
      6  vsom_set_state(map) on A, (weight) on B, vsom_set_last_bmu on A and E, batch_epoch(is_first = 0); vsom_set_last_bmu
         on B, batch_schedule_masked(reset_bmu = 0)
      7  destroy, single epochs on the former members, create over a permuted subset (ens_own without F: umatrix is now
         accepted), a second ensemble over an overlapping subset, calls alternating between the two
      8  G (ens_own): a whole-map epoch under VSOM_SIGMA_LAZY leaves its sigmaMap pending before the first create, which
         must materialise it; vsom_sigma_stats' deferred count never moves again
      9  an accumulated epoch opened on A before it joins: begin, chunk, create, an ensemble batch_epoch, chunk, end"""
    g = _EnsGen(cfg_name, seed)
    g.ops.append(("config", {"name": cfg_name, "seed": seed, "profile": "ensemble"}))
    own = "G" in g.all
    for n in g.all:
        g.m(n, "set_state", seed=seed + ENS_MEMBERS[n].get("map_seed", 0), parts="init")
    if own:
        g.emit("run", id=8)
        g.m("G", "sigma_mode", mode="lazy")
        g.m("G", "upload", chunk=0, asynchronous=False)
        g.m("G", "epoch", sigma=g.sigma(), first=True)
        g.emit("sigma_stats", k="G", expect=[1, 0, 0, 1])
    for n in g.all:
        if n not in ("C", "G"):
            g.m(n, "upload", chunk=0, asynchronous=False)
    # (no member yet: the masked online chunk is accepted, on the member's context and on its twin)
    g.m("B", "online_masked", eta=0.1, sigma=1.5, decay=1, first=True, seed=g.r(1 << 30), form="rows")
    g.emit("run", id=9)
    g.m("A", "accum_begin", sigma=g.sigma(), first=True, total=2 * g.sizes["A"][0])
    g.m("A", "accum_chunk")
    g.emit("ens_create", e=0, order=list(g.all))
    g.ens[0] = list(g.all)
    if own:
        g.emit("sigma_stats", k="G", expect=[1, 0, 1, 0])
        g.m("G", "get_state")
        g.emit("run_end", id=8)
    g.train("ens_epoch", 0)                  # C has no chunk: refused
    g.emit("ens_bmu", e=0)
    g.upload(0, {n: 0 for n in g.all})
    g.train("ens_epoch", 0, first=True)
    g.m("A", "accum_chunk")
    g.m("A", "accum_end")
    g.emit("run_end", id=9)
    g.m("A", "get_state")
    slots = sorted(g.rs.choice(np.arange(0, n_ops), 6, replace=False)) if n_ops >= 6 else [0] * 6
    runs = [int(r) for r in g.rs.permutation(6) + 1]
    for k in range(n_ops):
        while slots and k >= slots[0]:
            slots.pop(0)
            g.run(runs.pop(0))
        g.random_op()
    while runs:
        g.run(runs.pop(0))
    g.run(7)
    if own:
        g.m("G", "epoch", sigma=g.sigma(), first=True)
        g.emit("sigma_stats", k="G", expect=[1, 0, 1, 0])
    for n in g.all:
        g.m(n, "get_state")
    return g.ops


class EnsModel:
    """one Model per member, the ensembles' member orders, and who has ever joined one"""

    def __init__(self, cfg_name, seed):
        self.cfg_name = cfg_name
        self.names = list(ens_config(cfg_name)["members"])
        self.m = {n: Model(n, seed, 1, "ensemble") for n in self.names}
        for mod in self.m.values():
            mod.bmu_mode = BMU_AUTO
            mod.um = None
        self.ens = {}
        self.joined = set()

    def close(self):
        for mod in self.m.values():
            mod.close()

    def layout(self, p):
        """vsom_ensemble_upload_chunks' arguments: each member's rows, the host buffer (a gap of 3 floats between two
        ranges), offsets and row counts in member order"""
        order = self.ens[p["e"]]
        X, off, parts, at = {}, {}, [], 0
        for n in order:
            s = p["rows"][n]
            if "share" in s:
                continue
            x = self.m[n].chunks[s["chunk"]]
            if "head" in s:                  # (the ensemble_query profile: the chunk's first rows, none of them: B = 0)
                x = x[:s["head"]]
            if n in p.get("poison", {}):
                x = ens_poisoned(p["poison"][n], x)
            X[n], off[n] = x, at
            parts.append(x.reshape(-1))
            parts.append(np.full(3, -7.0, np.float32))
            at += x.size + 3
        for n in order:
            s = p["rows"][n]
            if "share" in s:
                X[n], off[n] = X[s["share"]][:s["n"]], off[s["share"]]
        buf = np.ascontiguousarray(np.concatenate(parts), np.float32)
        n_floats = buf.size - (4 if p.get("bad") == "offset" else 0)
        return {"X": X, "buf": buf, "n_floats": n_floats, "off": [off[n] for n in order],
                "B": [X[n].shape[0] for n in order]}

    def materialize(self, op):
        name, p = op
        if name == "m":
            return materialize(p["op"], self.m[p["k"]])
        if name == "ens_upload":
            return self.layout(p)
        if "masks" in p:
            return {"valid": {n: (ens_mask(p["masks"][n], self.m[n].X) if n in p["masks"] and self.m[n].X is not None
                                  else (np.ones(1, np.uint8) if n in p["masks"] else None)) for n in self.ens[p["e"]]}}
        return {}

    def path(self, op, n, k):
        """whether member n (index k) of an accepted train call takes its one-launch kernel, by the restated predicates"""
        name, p = op
        mod = self.m[n]
        cfg, B = mod.cfg, mod.B
        masked = n in p.get("masks", {})
        if name in ("ens_topk", "ens_topk_masked"):
            return topk_fast(cfg, B, p["k"][k], name == "ens_topk_masked")
        if name in ("ens_epoch", "ens_epoch_masked"):
            return masked_batch_tiny(cfg, B, mod.update_mode == UPDATE_STRICT) if masked else batch_tiny(cfg, B)
        if name in ("ens_schedule", "ens_schedule_masked"):
            sg = [_nan(v) for v in p["sigmas"][k]]
            if not sg or not all(np.isfinite(sg)):
                return False
            return masked_batch_tiny(cfg, B, mod.update_mode == UPDATE_STRICT) if masked else batch_tiny(cfg, B)
        return online_tiny(cfg, B, p["sigma"][k], mod.bmu_mode)

    def ens_refusal(self, op, a):
        """None where the header accepts the ensemble call, else (member index or None, words of the message, the entry of
        run 5's list), in the order csrc/vsom_ensemble.hip checks; a chunk staged ahead is the backend's to know"""
        name, p = op
        bad = p.get("bad")
        order = self.ens[p["e"]]
        if bad in ("null", "null_epochs", "null_valid"):
            return None, {"null": "null", "null_epochs": "null epochs array", "null_valid": "null valid_host array"}[bad], "null"
        for k, n in enumerate(order):
            mod = self.m[n]
            cfg = mod.cfg
            masked = n in p.get("masks", {})
            if name == "ens_upload":
                if a["off"][k] + a["B"][k] * cfg["J"] > a["n_floats"]:
                    return k, "rows beyond n_floats", "offset"
                continue
            if name == "ens_umatrix":
                if cfg["custom"]:
                    return k, "custom-transformation context", "umatrix_custom"
                continue
            if name in ("ens_schedule", "ens_schedule_masked"):
                if not p["sigmas"][k]:
                    continue                 # not touched
                if bad == "null_sigma" and k == len(order) - 1:
                    return k, "null sigma or mse_out", "null"
            if name in ("ens_online", "ens_online_masked"):
                if bad == "decay" and k == 1:
                    return k, "Exponential or InverseProportional", "decay"
                if masked and cfg["custom"]:
                    return k, "custom contexts are not supported", "masked_custom"
                if masked and cfg["tr"] == po.CLR:
                    return k, "CLR contexts are not supported", "masked_clr"
            if mod.X is None:
                return k, "no chunk loaded", "no_chunk"
            if name in ("ens_epoch_masked", "ens_schedule_masked") and masked:
                if cfg["custom"]:
                    return k, "custom context", "masked_custom"
                if cfg["tr"] == po.CLR:
                    return k, "CLR contexts are not supported", "masked_clr"
                if mod.update_mode != UPDATE_STRICT:
                    return k, "strict update mode", "non_strict"
        return None

    def member_refusal(self, n, op):
        """what a single-context call on member n must be refused for: (rc, words, label) or None"""
        name, p = op
        mod = self.m[n]
        cfg = mod.cfg
        if cfg["custom"] and (name in CUSTOM_REFUSED or name in ("schedule_masked", "online_masked", "um", "update_mode")):
            return VSOM_ERR_INVALID, "", None
        if cfg["tr"] == po.CLR and (name in CLR_REFUSED or name in ("schedule_masked", "online_masked")):
            return VSOM_ERR_INVALID, "CLR", None
        if name == "online_masked" and n in self.joined:
            return VSOM_ERR_INVALID, "joined a group or an ensemble", "member_online_masked"
        if name in ACCUM_OPS:
            why = mod.accum_refusal(op)
            if name == "accum_begin" and n in self.joined and why in (None, "already open"):
                return VSOM_ERR_INVALID, "joined a group or an ensemble", "member_accum_begin"
            if why is not None:
                return VSOM_ERR_INVALID, why, None
        return None

    def apply_member(self, n, op, a):
        mod = self.m[n]
        if op[0] == "bmu_mode":
            mod.bmu_mode = op[1]["mode"]
        if op[0] in MEMBER_QUERIES and mod.profile == "ensemble":    # read-only: the window's rows from the plain references
            return member_query(mod, op, a)
        return mod.apply(op, a)

    # ---- the four query calls of the ensemble_query profile (read-only: apply() has nothing to do for them) ----
    def ensq_refusal(self, op):
        """None where the header accepts the query call, else (member index or None, words of the message, the entry of
        ENSQ_REFUSALS), in the order csrc/vsom_ensemble.hip checks: the call's arrays, then member by member the context,
        its chunk, its k, its idx pointer.  A chunk staged ahead is the backend's to know (must_refuse)."""
        name, p = op
        bad = p.get("bad")
        order = self.ens[p["e"]]
        masked = name != "ens_topk"
        arrays = (["null_valid", "null_out"] if masked else ["null_k", "null_out"]) + \
            {"ens_similarity_masked": ["null_num_sigmas", "bad_rule"], "ens_topk_masked": ["null_k"]}.get(name, [])
        words = {"null_valid": "null valid_host array", "null_out": "null out array", "null_k": "null k array",
                 "null_num_sigmas": "null num_sigmas array", "bad_rule": "unknown sigma_rule"}
        if bad in arrays:
            return None, words[bad], bad
        cov = covered(op, order)
        for k, n in enumerate(order):
            if n not in cov:
                continue
            mod = self.m[n]
            if mod.cfg["custom"]:
                return k, "custom contexts are not supported", "custom"
            if masked and mod.cfg["tr"] == po.CLR:
                return k, "CLR contexts are not supported", "clr"
            if mod.X is None:
                return k, "no chunk loaded", "no_chunk"
            if "k" in p and not 1 <= p["k"][k] <= min(64, mod.N):
                return k, "k must be in [1, min(64, N)]", f"k{p['k'][k]}"
            if bad == "null_idx" and n == p["null_idx"]:
                return k, "out->idx is null", "null_idx"
        return None

    def query_fast(self, op, n, k):
        """whether member n (index k) of an accepted query call runs in the many-member kernel, by the restated predicates"""
        if op[0] in ("ens_topk", "ens_topk_masked"):
            return self.path(op, n, k)
        return masked_query_fast(self.m[n].cfg, self.m[n].B)

    def query(self, op, a, hits=None, sigma=None):
        """{member: (rows, {output: expected values of those rows})} of an accepted query call, every covered member with
        rows; hits / sigma: {member: array} taken for the member's own (the CPU fake's mutants)"""
        name, p = op
        order = self.ens[p["e"]]
        res = {}
        for n in covered(op, order):
            mod, k = self.m[n], order.index(n)
            if mod.B == 0:
                continue
            valid = a.get("valid", {}).get(n)
            rows = model_rows(mod, valid, p, k)
            res[n] = (rows, query_member(mod, name, p, k, valid, rows, (hits or {}).get(n), (sigma or {}).get(n)))
        return res

    def apply(self, op, a):
        """an accepted ensemble call: the single call on every member in index order; outputs keyed "<member>.<name>" """
        name, p = op
        out = {}
        if name == "ens_create":
            self.ens[p["e"]] = list(p["order"])
            self.joined |= set(p["order"])
            return out
        if name == "ens_destroy":
            del self.ens[p["e"]]
            return out
        for k, n in enumerate(self.ens[p["e"]]):
            mod = self.m[n]
            valid = a.get("valid", {}).get(n)
            if name == "ens_upload":
                single, arg = ("upload", {}), {"X": a["X"][n]}
            elif name in ("ens_epoch", "ens_epoch_masked"):
                q = {"sigma": p["sigma"][k], "first": p["first"]}
                single, arg = ("epoch", q) if valid is None else ("epoch_masked", q), {"valid": valid}
                if valid is not None:
                    arg = {"valid": np.broadcast_to(valid, mod.X.shape).copy()}
            elif name in ("ens_schedule", "ens_schedule_masked"):
                q = {"sigmas": p["sigmas"][k], "reset": p["reset"]}
                single, arg = ("schedule", q) if valid is None else ("schedule_masked", q), {"valid": valid}
                if not q["sigmas"]:
                    continue                 # "a member with epochs[k] = 0 is not touched"
            elif name in ("ens_online", "ens_online_masked"):
                q = {"eta": p["eta"][k], "sigma": p["sigma"][k], "decay": p["decay"][k], "first": p["first"], "mode": "fetch"}
                single, arg = ("online", q) if valid is None else ("online_masked", q), {"valid": valid}
            elif name == "ens_bmu":
                single, arg = ("bmu", {}), {}
            else:
                single, arg = ("um", {}), {}
            for key, v in mod.apply(single, arg).items():
                out[f"{n}.{key}"] = v
        return out


def ens_conditions(cfg_name, stats, gpu=False):
    """what a walk of the ensemble profile must have met, from run_ensemble_walk's counts, so that it cannot pass vacuously"""
    own = not ENS_CONFIGS[cfg_name]["one_stream"]
    assert stats["ops"] >= 100, stats
    assert all(stats["accepted"][c] >= 2 for c in ENS_CALLS), stats["accepted"]
    # in each kind of train call: one call at least with two launched members and one on its ordinary path
    assert all(stats["mixed"][c] >= 1 for c in ENS_TRAIN), stats["mixed"]
    for label in ENS_REFUSALS + (ENS_REFUSALS_OWN if own else ()):
        assert stats["refusals"].get(label, 0) >= 1, (label, stats["refusals"])
    # run 4: G's chunk is staged ahead (ens_own): the six train calls and bmu_batch were refused, naming it
    assert stats["staged"] == (7 if own else 0), stats
    if gpu:
        assert stats["nowait"] >= 2 and stats["applies"] >= 10, stats


class Within:
    """An expected array of a member op whose arithmetic is not restated bit for bit (the device's double exp and log): `ref`
    and a bound per element -- 0: the element bit for bit (NaN equal to NaN), inf: not compared (a draw within
    bmd_masked_ref.NEAR of a cumulative boundary, and what hangs on it), else |got - ref| <= bound."""

    def __init__(self, ref, bound):
        self.ref = np.asarray(ref)
        self.bound = np.broadcast_to(np.asarray(bound, np.float64), self.ref.shape)

    def difference(self, got):
        if got is None:
            return "got nothing"
        g, e, b = np.asarray(got), self.ref, self.bound
        if g.shape != e.shape or g.dtype != e.dtype:
            return f"shape / type {g.shape} {g.dtype} != {e.shape} {e.dtype}"
        exact = b == 0
        if e.dtype.kind == "f":
            with np.errstate(all="ignore"):
                exact = exact | ~np.isfinite(e)          # (an infinite or NaN reference value: the same value)
                near = (np.abs(g - e) <= b) | (g == e)   # (a NaN bound -- a NaN in the row's units -- asks for the same value)
            same = np.where(exact, (g == e) & (np.signbit(g) == np.signbit(e)) | (np.isnan(g) & np.isnan(e)), near)
        else:
            same = g == e
        same = same | np.isinf(b)
        if same.all():
            return None
        at = np.unravel_index(int(np.argmin(same.reshape(-1))), same.shape)
        return (f"element {tuple(int(i) for i in at)}: got {g[at]!r}, expected {e[at]!r} within {b[at]!r} "
                f"({int((~same).sum())} differ)")


def plain(out):
    """a model's outputs as a library would return them: the reference values of the bounded ones"""
    return {k: (v.ref.copy() if isinstance(v, Within) else v) for k, v in out.items()}


def ens_difference(got, exp):
    """first_difference on the values' own width: the U-matrix is a double"""
    if isinstance(exp, Within):
        return exp.difference(got)
    if exp is not None and np.asarray(exp).dtype == np.float64 and np.asarray(exp).ndim:
        return first_difference_exact(np.asarray(got, np.float64), np.asarray(exp))
    return first_difference(got, exp)


def run_ensemble_walk(ops, make_backend):
    """run_walk for the ensemble profile: the backend make_backend(cfg_name, model) holds the members (the real one: also a
    twin of each that never joins) and the ensembles.  Returns counts: accepted calls per ensemble call, per kind of train
    call the calls with at least two launched members and one on its ordinary path, the refusals of run 5 by entry, the
    stage-ahead refusals, the wait = 0 uploads followed by a call with no host wait between."""
    name0, cfg = ops[0]
    assert name0 == "config" and cfg["profile"] in ("ensemble", "ensemble_query"), ops[0]
    em = EnsModel(cfg["name"], cfg["seed"])
    em.ops = ops
    be = make_backend(cfg["name"], em)
    stats = {"ops": 0, "accepted": {c: 0 for c in ENS_CALLS}, "mixed": {c: 0 for c in ENS_TRAIN}, "refusals": {},
             "staged": 0, "nowait": 0, "applies": 0, "q": ensq_stats()}
    done = [ops[0]]

    def fail(msg):
        raise WalkFailure(f"call-sequence walk {cfg['name']} seed {cfg['seed']}: {msg}\n"
                          f"replay(ops) with ops = {done!r}")

    def check_outputs(what, got, exp):
        for k, e in exp.items():
            d = ens_difference(got.get(k), e)
            if d:
                fail(f"{what}: output {k!r} differs from the oracle at {d}")

    def check_all(what, observe=None):
        for n in em.names:
            mod = em.m[n]
            exp = mod.state()
            exp.update(lb=mod.lb, mse=mod.mse)
            check_outputs(f"{what} (full state of member {n})", (observe or be.observe)(n), exp)

    def refusal(what, rc, msg, k, words, label):
        if rc != VSOM_ERR_INVALID or words not in msg or (k is not None and f"member {k}:" not in msg):
            fail(f"{what} returned {rc} {msg!r}: the header refuses it ({words}" +
                 (f", naming member {k})" if k is not None else ")"))
        if label:
            stats["refusals"][label] = stats["refusals"].get(label, 0) + 1
        check_all(f"{what} refused ({words})")       # a refused call changes nothing in any member

    def check(op, a, rc, msg, out):
        name, p = op
        stats["ops"] += 1
        if out.get("twin_diff"):
            fail(f"{name}: {out['twin_diff']}")
        if name in ENSQ_CALLS:
            return check_query(op, a, rc, msg, out)
        if name == "sigma_stats":
            if rc != 0 or [int(v) for v in out["stats"]] != list(p["expect"]):
                fail(f"vsom_sigma_stats of member {p['k']} = {out.get('stats')}, the header's contract gives {p['expect']} "
                     f"(deferred, dropped, materialised, pending)")
            return
        if name == "m":
            n, inner = p["k"], p["op"]
            why = em.member_refusal(n, inner)
            if why is not None:
                if rc != why[0] or why[1] not in msg:
                    fail(f"{inner[0]} on member {n} returned {rc} {msg!r}: the header refuses it ({why[1]})")
                if why[2]:
                    refusal(f"{inner[0]} on member {n}", rc, msg, None, why[1], why[2])
                return
            if rc != 0:
                fail(f"{inner[0]} on member {n} failed: {rc} {msg}")
            check_outputs(f"{inner[0]} on member {n}", out, em.apply_member(n, inner, a))
            if inner[0] == "get_state":
                check_all("get_state")
            return
        if name in ("ens_create", "ens_destroy"):
            if rc != 0:
                fail(f"{name} failed: {rc} {msg}")
            em.apply(op, a)
            return
        why = em.ens_refusal(op, a)
        if why is not None:
            return refusal(name, rc, msg, *why)
        if "must_refuse" in p:
            k = em.ens[p["e"]].index(p["must_refuse"])
            stats["staged"] += 1
            return refusal(f"{name} behind epoch_async, prefetch on member {k}", rc, msg, k, "vsom_commit_chunk first", None)
        if rc != 0:
            fail(f"{name} failed: {rc} {msg}")
        for n, v in out.pop("applies", {}).items():       # the library's own predicate for every masked member
            k = em.ens[p["e"]].index(n)
            stats["applies"] += 1
            if bool(v) != em.path(op, n, k):
                fail(f"{name}: member {k} ({n}, {em.m[n].B} rows): the library's *_tiny_applies says {v}, the restated "
                     f"predicate {em.path(op, n, k)}")
        if name in ENS_TRAIN:
            order = em.ens[p["e"]]
            touched = [k for k in range(len(order)) if "sigmas" not in p or p["sigmas"][k]]
            fast = sum(em.path(op, order[k], k) for k in touched)
            stats["mixed"][name] += fast >= 2 and len(touched) - fast >= 1
        stats["accepted"][name] += 1
        check_outputs(name, out, em.apply(op, a))

    def check_query(op, a, rc, msg, out):
        """one of the four query calls of the ensemble_query profile: the library's fast-path predicate, the refusal the
        header lists, the arrays that must stay as they were, every covered member's outputs against the model"""
        name, p = op
        q = stats["q"]
        order = em.ens[p["e"]]
        cov = covered(op, order)
        for n, v in out.pop("applies", {}).items():
            k = order.index(n)
            q["applies"] += 1
            if int(v) != int(em.path(op, n, k)):
                fail(f"{name}: member {k} ({n}, {em.m[n].B} rows, k = {p['k'][k]}): vsom_ensemble_topk_applies says {v}, the "
                     f"restated predicate topk_fast {em.path(op, n, k)}")
        rows_of = {n: em.m[n].B for n in order}
        why = em.ensq_refusal(op)
        if why is None and "must_refuse" in p:
            why = (order.index(p["must_refuse"]), "vsom_commit_chunk first", "staged")
        if why is not None:
            wrote = sorted(k for k in out if "." in k)
            if wrote:
                fail(f"{name} returned {rc} and wrote {wrote}: the header refuses it ({why[1]}), and a refused call writes nothing")
            return refusal(name, rc, msg, why[0], why[1], "q_" + why[2])
        if rc != 0:
            fail(f"{name} failed: {rc} {msg}")
        for key in sorted(out):
            n = key.split(".")[0]
            if "." in key and (n not in cov or rows_of[n] == 0):
                fail(f"{name}: output {key!r} of member {order.index(n)} was written (element 0: "
                     f"{np.asarray(out[key]).reshape(-1)[:1].tolist()}): the member is "
                     f"{'skipped' if n not in cov else 'without rows'} and its arrays must keep what they held")
        fast = [n for n in cov if rows_of[n] and em.query_fast(op, n, order.index(n))]
        slow = [n for n in cov if rows_of[n] and n not in fast]
        q["accepted"][name] += 1
        q["mixed"][name] += len(fast) >= 2 and len(slow) >= 1 and len(cov) < len(order)
        q["b0"] += sum(rows_of[n] == 0 for n in cov)
        q["ahead_skipped"] += bool(p.get("ahead_skipped"))
        for label in p.get("labels", ()):
            q["met"][label] = q["met"].get(label, 0) + 1
        for n, (rows, exp) in em.query(op, a).items():
            q["covered_rows"][n] = q["covered_rows"].get(n, 0) + rows_of[n]
            q["model_rows"][n] = q["model_rows"].get(n, 0) + len(rows)
            if "count" in exp:
                q["padded"] += int((exp["count"] < p["k"][order.index(n)]).sum())
            q["novalid"] += int((exp["nvalid"] == 0).sum()) if "nvalid" in exp else 0
            for key, e in exp.items():
                got = out.get(f"{n}.{key}")
                if got is None:
                    continue                   # (a NULL output pointer)
                got = np.asarray(got)
                if got.shape[:1] != (rows_of[n],):
                    fail(f"{name}: output {n}.{key} returned {got.shape} values for {rows_of[n]} rows")
                d = query_difference(got[rows], e, key)
                if d:
                    fail(f"{name}: output {n}.{key} (member {order.index(n)}, rows {rows[:8].tolist()}...) differs from "
                         f"the model at {d}")

    def back_to_back(batch):
        """run 1 on a backend that can separate the ensemble from the twins (call_first / call_twin): every call goes to
        the ensemble before a twin or the model sees one; the arguments come from a shadow that follows the uploads alone"""
        shadow = copy.copy(em)
        shadow.m = {n: copy.copy(mod) for n, mod in em.m.items()}
        made = []
        for op in batch:
            a = shadow.materialize(op)
            made.append((op, a) + tuple(be.call_first(op, a)))
            if made[-1][2] == 0 and op[0] == "ens_upload":
                for n in shadow.ens[op[1]["e"]]:
                    shadow.m[n].X = a["X"][n]
            if len(made) > 1 and made[-2][0][0] == "ens_upload" and made[-2][0][1]["wait"] == 0 and made[-1][2] == 0:
                stats["nowait"] += 1
        for op, a, rc, msg, out in made:
            done.append(op)
            be.call_twin(op, a, rc, msg, out)
            check(op, a, rc, msg, out)

    try:
        todo = list(ops[1:])
        while todo:
            op = todo.pop(0)
            done.append(op)
            if op[0] in ("run", "run_end"):
                if op == ("run", {"id": 1}) and hasattr(be, "call_first"):
                    n = [o[0] for o in todo].index("run_end")
                    back_to_back(todo[:n])
                    del todo[:n]
                continue
            a = em.materialize(op)
            rc, msg, out = be.call(op, a)
            check(op, a, rc, msg, out)
        check_all("end of walk")
        if hasattr(be, "observe_twin"):
            check_all("end of walk, the twins", be.observe_twin)
    finally:
        be.close()
        em.close()
    return stats


class EnsGpuBackend:
    """The members of an ensemble configuration and one twin of each that never joins, on the C ABI.  A member is a
    GpuBackend (its context, pinned and device copies of its chunks); its twin comes from the same constructor, gets the
    same settings, and makes every call as a single call, fed from pageable memory and synchronised after each.  What an
    ensemble call returns must equal, bit for bit, what the twins' single calls return in member order."""

    def __init__(self, cfg_name, em):
        self.em = em
        ec = ens_config(cfg_name)
        self.gb = {n: GpuBackend(n, em.m[n]) for n in em.names}
        self.capi, self.L, self.hip = self.gb[em.names[0]].capi, self.gb[em.names[0]].L, self.gb[em.names[0]].hip
        self.twin = {n: self.gb[n].make() for n in em.names}
        self.streams = []
        self.queries = cfg_name in ENSQ_CONFIGS    # the ensemble_query profile: every twin is fixed at VSOM_SIGMA_EAGER
        for i, n in enumerate(em.names):
            if config(n).get("lazy"):             # (the twin too: it never joins, and may go on deferring)
                self.gb[n].ctx.set_sigma_mode(SIGMA_LAZY)
                self.twin[n].set_sigma_mode(SIGMA_EAGER if self.queries else SIGMA_LAZY)
            if not ec["one_stream"] or i == 0:
                s = C.c_void_p()
                assert self.hip.hipStreamCreate(C.byref(s)) == 0
                self.streams.append(s)
            self.capi.check(self.L.vsom_set_stream(self.gb[n].ctx._h, self.streams[-1]))
        self.ens = {}
        # the pinned buffer of every wait = 0 upload, made and filled up front (an allocation inside the walk would
        # synchronise the device); junk goes in once a synchronising call on the members has returned
        self.pinned, self.in_flight = {}, []
        shadow = copy.copy(em)
        shadow.ens = {}
        for name, p in em.ops[1:]:
            if name == "ens_create":
                shadow.ens[p["e"]] = list(p["order"])
            elif name == "ens_destroy":
                del shadow.ens[p["e"]]
            elif name == "ens_upload" and p["wait"] == 0:
                lay = shadow.layout(p)
                pb = self.capi.PinnedBuffer((lay["buf"].size,))
                pb.array[...] = lay["buf"]
                self.pinned[p["uid"]] = pb

    def close(self):
        for n, gb in self.gb.items():
            self.L.vsom_synchronize(gb.ctx._h)
        for e in list(self.ens.values()):
            self.L.vsom_ensemble_destroy(e)
        for n, gb in self.gb.items():
            self.twin[n].close()
            gb.close()
        for pb in self.pinned.values():
            pb.free()
        for s in self.streams:
            self.hip.hipStreamDestroy(s)

    def call(self, op, a):
        rc, msg, out = self.call_first(op, a)
        self.call_twin(op, a, rc, msg, out)
        return rc, msg, out

    def _err(self, rc):
        return "" if rc == 0 else self.L.vsom_last_error().decode(errors="replace")

    # ---- the members and the ensembles ----
    def call_first(self, op, a):
        name, p = op
        L = self.L
        if name == "m":
            gb = self.gb[p["k"]]
            return gb._call(gb.ctx, p["op"], a)
        if name == "sigma_stats":
            st = self.gb[p["k"]].ctx.sigma_stats()
            return 0, "", {"stats": tuple(st[k] for k in ("deferred", "dropped", "materialised", "pending"))}
        if name == "ens_create":
            K = len(p["order"])
            arr = (C.c_void_p * K)(*[self.gb[n].ctx._h.value for n in p["order"]])
            h = C.c_void_p()
            rc = L.vsom_ensemble_create(C.byref(h), arr, K)
            if rc == 0:
                self.ens[p["e"]] = h
            return rc, self._err(rc), {}
        if name == "ens_destroy":
            L.vsom_ensemble_destroy(self.ens.pop(p["e"]))
            return 0, "", {}
        if name in ENSQ_CALLS:
            # (a query that skips a member has not synchronised it: the pinned rows of a wait = 0 upload stay as they are
            # until a call that covers every member has returned, below)
            rc, out = self._query(self.ens[p["e"]], self.em.ens[p["e"]], op, a)
            return rc, self._err(rc), out
        rc, out = self._ensemble(self.ens[p["e"]], self.em.ens[p["e"]], op, a)
        msg = self._err(rc)
        if rc == 0 and name in ENS_TRAIN + ("ens_bmu",) and self.in_flight and \
                not any("sigmas" in p and not s for s in p.get("sigmas", [])):
            # every member's stream has been waited for: the pinned rows of earlier wait = 0 uploads may change
            for pb in self.in_flight:
                pb.array[...] = np.float32(np.nan)
            self.in_flight = []
        return rc, msg, out

    def _ensemble(self, eh, order, op, a):
        name, p = op
        L, K = self.L, len(order)
        f, u = self.capi._f, self.capi._u
        dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        bad = p.get("bad")
        B = [int(L.vsom_chunk_size(self.gb[n].ctx._h)) for n in order]
        out, keep = {}, []
        if "masks" in p and bad != "null_valid":
            valid = [a["valid"][n] for n in order]
            keep = [None if v is None else v.copy() for v in valid]
            vptr = (u8p * K)(*[u8p() if v is None else v.ctypes.data_as(u8p) for v in keep])
            ones = (C.c_int * K)(*[0 if v is None else int(v.ndim == 1) for v in keep])
            masked = [n for n, v in zip(order, valid) if v is not None]
        if name == "ens_upload":
            buf = self.pinned[p["uid"]].array if p["wait"] == 0 else a["buf"]
            off, bs = (C.c_size_t * K)(*a["off"]), (C.c_size_t * K)(*a["B"])
            rc = L.vsom_ensemble_upload_chunks(eh, f(buf), a["n_floats"], None if bad == "null" else off, bs, p["wait"])
            if rc == 0 and p["wait"] == 0:
                self.in_flight.append(self.pinned[p["uid"]])
        elif name in ("ens_epoch", "ens_epoch_masked"):
            sig, mse = (C.c_double * K)(*p["sigma"]), np.zeros(K, np.float32)
            if name == "ens_epoch":
                rc = L.vsom_ensemble_batch_epoch(eh, None if bad == "null" else sig, int(p["first"]), f(mse))
            else:
                if bad != "null_valid":
                    out["applies"] = {n: L.vsom_masked_tiny_applies(self.gb[n].ctx._h, int(a["valid"][n].ndim == 1))
                                      for n in masked if self.em.m[n].X is not None}
                rc = L.vsom_ensemble_batch_epoch_masked(eh, sig, int(p["first"]), vptr, ones, f(mse))
            out.update({f"{n}.mse": mse[k] for k, n in enumerate(order)})
        elif name in ("ens_schedule", "ens_schedule_masked"):
            sgs = [np.array([_nan(v) for v in s], np.float64) for s in p["sigmas"]]
            mses = [np.zeros(s.size, np.float32) for s in sgs]
            sig = (dp * K)(*[s.ctypes.data_as(dp) for s in sgs])
            if bad == "null_sigma":
                sig[K - 1] = dp()
            mo = (C.POINTER(C.c_float) * K)(*[f(m) for m in mses])
            cnt = (C.c_size_t * K)(*[s.size for s in sgs])
            if name == "ens_schedule":
                rc = L.vsom_ensemble_batch_schedule(eh, sig, None if bad == "null_epochs" else cnt, int(p["reset"]), mo)
            else:
                out["applies"] = {n: L.vsom_masked_tiny_applies(self.gb[n].ctx._h, int(a["valid"][n].ndim == 1))
                                  for k, n in enumerate(order) if n in masked and self.em.m[n].X is not None and
                                  sgs[k].size and np.isfinite(sgs[k]).all()}
                rc = L.vsom_ensemble_batch_schedule_masked(eh, sig, cnt, int(p["reset"]), vptr, ones, mo)
            out.update({f"{n}.mses": mses[k] for k, n in enumerate(order) if sgs[k].size})
        elif name in ("ens_online", "ens_online_masked"):
            decay = list(p["decay"])
            if bad == "decay":
                decay[1] = 7
            eta, sig, dec = (C.c_double * K)(*p["eta"]), (C.c_double * K)(*p["sigma"]), (C.c_int * K)(*decay)
            lbs = [np.zeros(b, np.uint64) for b in B]
            lp = (C.POINTER(C.c_uint64) * K)(*[u(x) for x in lbs])
            mse = np.zeros(K, np.float32)
            if name == "ens_online":
                rc = L.vsom_ensemble_train_online_chunk_fetch(eh, eta, sig, dec, int(p["first"]), lp, f(mse))
            elif bad == "null_valid":
                rc = L.vsom_ensemble_train_online_chunk_masked(eh, eta, sig, dec, int(p["first"]), None, None, lp, f(mse))
            else:
                out["applies"] = {n: L.vsom_online_masked_tiny_applies(self.gb[n].ctx._h, p["sigma"][order.index(n)],
                                                                       int(a["valid"][n].ndim == 1))
                                  for n in masked if self.em.m[n].X is not None}
                rc = L.vsom_ensemble_train_online_chunk_masked(eh, eta, sig, dec, int(p["first"]), vptr, ones, lp, f(mse))
            for k, n in enumerate(order):
                out[f"{n}.mse"], out[f"{n}.lb"] = mse[k], lbs[k]
        elif name == "ens_bmu":
            idx, dist = [np.zeros(b, np.uint64) for b in B], [np.zeros(b, np.float32) for b in B]
            rc = L.vsom_ensemble_bmu_batch(eh, (C.POINTER(C.c_uint64) * K)(*[u(x) for x in idx]),
                                           (C.POINTER(C.c_float) * K)(*[f(x) for x in dist]))
            for k, n in enumerate(order):
                out[f"{n}.idx"], out[f"{n}.dist"] = idx[k], dist[k]
        else:
            um = [np.zeros(self.gb[n].N, np.float64) for n in order]
            rc = L.vsom_ensemble_umatrix(eh, (dp * K)(*[x.ctypes.data_as(dp) for x in um]))
            out.update({f"{n}.u": um[k] for k, n in enumerate(order)})
        for v in keep:                         # "valid_host is not read after the call returns"
            if v is not None:
                v[...] = 0
        return rc, out

    # ---- the four query calls: the C ABI directly, every array behind a canary ----
    QUERY_ARRAYS = {
        "ens_bmu_masked": (("bmu", np.uint64, "B"), ("dist", np.float32, "B"), ("nvalid", np.uint32, "B"),
                           ("fill", np.float32, "BJ")),
        "ens_similarity_masked": (("bmu", np.uint64, "B"), ("dist", np.float32, "B"), ("dmax", np.float32, "B"),
                                  ("dmax_col", np.uint32, "B"), ("first", np.float32, "B"), ("amax", np.float32, "B"),
                                  ("amax_col", np.uint32, "B"), ("outside", np.uint32, "B"), ("delta", np.float32, "BJ"),
                                  ("nvalid", np.uint32, "B")),
        "ens_topk": (("idx", np.uint64, "Bk"), ("dist", np.float32, "Bk"), ("count", np.uint32, "B"),
                     ("nvalid", np.uint32, "B")),
    }
    GUARD = 8                                  # elements behind every array that must keep the canary too

    def _query(self, eh, order, op, a):
        """One query call.  Every output array of every member -- covered, skipped, asked for or not -- is filled with the
        byte 0xA5 first and has GUARD elements more than its size.  After the call: an array the call was given for a
        covered member with rows must be overwritten (no element of an index / count array still the canary) and is
        returned as "<member>.<output>"; every other array, every array of a refused call and every guard must still hold
        the canary -- one that does not is returned like an output, and the walk reports the write."""
        name, p = op
        L, K, bad = self.L, len(order), p.get("bad")
        u8p = C.POINTER(C.c_uint8)
        masked = name != "ens_topk"
        cov = covered(op, order)
        B = [int(L.vsom_chunk_size(self.gb[n].ctx._h)) for n in order]
        out = {}
        ks = p.get("k", [1] * K)
        if "k" in p and bad != "null_k":       # the library's own predicate for every covered member, and an index past the end
            out["applies"] = {n: L.vsom_ensemble_topk_applies(eh, order.index(n), ks[order.index(n)], int(masked)) for n in cov}
            if L.vsom_ensemble_topk_applies(eh, K, 1, int(masked)) != VSOM_ERR_INVALID:
                out["twin_diff"] = f"vsom_ensemble_topk_applies accepted the member index {K} of {K} members"
        spec = self.QUERY_ARRAYS["ens_topk" if "k" in p else name]
        struct = {"ens_bmu_masked": self.capi.MaskedOut, "ens_similarity_masked": self.capi.SimilarityMaskedOut}.get(
            name, self.capi.EnsembleTopkOut)
        outs = (struct * K)()
        arrays = {}
        for k, n in enumerate(order):
            J = config(n)["J"]
            for key, dtype, shape in spec:
                count = B[k] * {"B": 1, "BJ": J, "Bk": ks[k]}[shape]
                arr = np.empty(count + self.GUARD, dtype)
                arr.view(np.uint8)[...] = 0xA5
                asked = p[key][k] if key in p and isinstance(p[key], list) and key != "k" else True
                if key in ("count", "nvalid") and name == "ens_topk":
                    asked = True               # (the plain call ignores them: they must stay as they are)
                if key == "idx" and ((not masked and n not in cov) or (bad == "null_idx" and n == p["null_idx"])):
                    asked = False              # (the plain call: a NULL idx is what skips a member)
                if asked:
                    setattr(outs[k], key, arr.ctypes.data_as(dict(struct._fields_)[key]))
                arrays[n, key] = (arr, count, asked, shape)
        keep = [a["valid"][n].copy() if masked and a["valid"].get(n) is not None else None for n in order]
        vptr = (u8p * K)(*[u8p() if v is None else v.ctypes.data_as(u8p) for v in keep])
        ones = (C.c_int * K)(*[0 if v is None else int(v.ndim == 1) for v in keep])
        mh = (C.c_uint64 * K)(*p.get("min_hits", [0] * K))
        kp = (C.c_uint32 * K)(*ks)
        vp = None if bad == "null_valid" else vptr
        op_ = None if bad == "null_out" else outs
        if name == "ens_bmu_masked":
            rc = L.vsom_ensemble_bmu_masked_batch(eh, mh, vp, ones, op_)
        elif name == "ens_similarity_masked":
            ns = (C.c_int * K)(*p["num_sigmas"])
            rc = L.vsom_ensemble_similarity_masked_batch(eh, mh, None if bad == "null_num_sigmas" else ns,
                                                         7 if bad == "bad_rule" else p["rule"], vp, ones, op_)
        elif name == "ens_topk":
            rc = L.vsom_ensemble_bmu_topk_batch(eh, None if bad == "null_k" else kp, op_)
        else:
            rc = L.vsom_ensemble_bmu_topk_masked_batch(eh, None if bad == "null_k" else kp, mh, vp, ones, op_)
        for v in keep:                         # "valid_host is not read after the call returns"
            if v is not None:
                v[...] = 0
        for (n, key), (arr, count, asked, shape) in arrays.items():
            k = order.index(n)
            body, guard = arr[:count], arr[count:]
            clean = lambda x: bool((x.view(np.uint8) == 0xA5).all())
            if not clean(guard):
                out["twin_diff"] = f"the {self.GUARD} elements behind output {key!r} of member {k} ({n}) were written"
            written = rc == 0 and asked and n in cov and B[k] > 0 and not (name == "ens_topk" and key in ("count", "nvalid"))
            if not written:
                if not clean(body):
                    out[f"{n}.{key}"] = body.copy()
                continue
            if body.dtype.kind == "u" and (body.view(np.uint8).reshape(count, -1) == 0xA5).all(axis=1).any():
                out["twin_diff"] = f"output {key!r} of member {k} ({n}) still holds the canary: not every element was written"
            cols = {"B": (), "BJ": (config(n)["J"],), "Bk": (ks[k],)}[shape]
            out[f"{n}.{key}"] = body.reshape((B[k],) + cols).copy()
        return rc, out

    def _query_twins(self, order, op, a, out):
        """every covered member's share as the single call over [0, B) on its twin, from pageable memory; every row compared
        on the words (NaN payloads and signs included)"""
        name, p = op
        for n in covered(op, order):
            k, t = order.index(n), self.twin[n]
            if int(self.L.vsom_chunk_size(t._h)) == 0:
                continue                       # (the single calls refuse a chunk without rows)
            valid = a.get("valid", {}).get(n)
            if name == "ens_bmu_masked":
                tout = t.bmu_masked(valid, min_hits=p["min_hits"][k], fill=p["fill"][k])
            elif name == "ens_similarity_masked":
                tout = t.similarity_masked(valid, p["min_hits"][k], p["num_sigmas"][k], p["rule"], delta=p["delta"][k])
            elif name == "ens_topk":
                tout = dict(zip(("idx", "dist"), t.bmu_topk(p["k"][k], dist=p["dist"][k])))
            else:
                tout = t.bmu_topk_masked(p["k"][k], valid, min_hits=p["min_hits"][k], dist=p["dist"][k])
            self.capi.check(self.L.vsom_synchronize(t._h))
            for key, v in tout.items():
                got = out.get(f"{n}.{key}")
                if v is None or got is None:
                    continue
                d = first_difference_exact(words(got), words(v))
                if d:
                    out["twin_diff"] = f"output {key!r} of member {k} ({n}) differs from its twin's single call at {d}"
                    return

    # ---- the twins ----
    def call_twin(self, op, a, rc, msg, out):
        name, p = op
        if rc != 0 and name != "m":
            return                             # (a refused ensemble call: nothing to replay)
        if name in ("ens_create", "ens_destroy", "sigma_stats"):
            return
        if name == "m":
            n, inner = p["k"], p["op"]
            gb, t = self.gb[n], self.twin[n]
            joined = n in self.em.joined
            if inner[0] == "online_masked" and joined and not self.em.m[n].cfg["custom"] and self.em.m[n].cfg["tr"] != po.CLR:
                return                         # the member must refuse it; the twin would accept and train
            trc, _, tout = gb._call(t, inner, a, twin=True)
            if inner[0] == "sigma_mode" and self.queries:
                t.set_sigma_mode(SIGMA_EAGER)
            if inner[0] == "accum_begin" and joined and rc != 0 and trc == 0:
                # the header gives the twin, which never joined, another answer: it accepts -- and is put back
                self.capi.check(self.L.vsom_batch_accum_abort(t._h))
                return
            if trc != rc:
                out["twin_diff"] = f"{inner[0]} on member {n} returned {rc}, its twin {trc}"
                return
            if rc == 0 and inner[0] != "get_state":      # (the same single call on both: on the words where it is a query)
                self._diff(out, tout, f"member {n}'s twin", on_words=inner[0] in MEMBER_QUERIES or inner[0] == "bmu_masked")
            return
        order = self.em.ens[p["e"]]
        if name in ENSQ_CALLS:
            return self._query_twins(order, op, a, out)
        tout = {}
        for k, n in enumerate(order):
            for key, v in self._single(self.twin[n], n, k, op, a).items():
                tout[f"{n}.{key}"] = v
            self.capi.check(self.L.vsom_synchronize(self.twin[n]._h))
        self._diff(out, tout, "the twins' single calls")

    def _diff(self, out, tout, who, on_words=False):
        for key, v in tout.items():
            g, v = np.asarray(out.get(key)), np.asarray(v)
            if on_words and g.dtype == v.dtype and v.dtype.kind == "f":
                g, v = words(g), words(v)      # (NaN payloads too: a record that is NaN throughout, a padded list)
            d = first_difference_exact(g, v)
            if d:
                out["twin_diff"] = f"output {key!r} differs from {who} at {d}"
                return

    def _single(self, t, n, k, op, a):
        """member k's share of an accepted ensemble call as the single call on its twin"""
        name, p = op
        L, h = self.L, t._h
        f, u = self.capi._f, self.capi._u
        dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        valid = a.get("valid", {}).get(n)
        vb = None if valid is None else valid.copy()
        vp, one = (None, 0) if vb is None else (vb.ctypes.data_as(u8p), int(vb.ndim == 1))
        m = C.c_float()
        out = {}
        if name == "ens_upload":
            X = np.ascontiguousarray(a["X"][n], np.float32)
            rc = L.vsom_upload_chunk(h, f(X), X.shape[0])
        elif name in ("ens_epoch", "ens_epoch_masked"):
            if vb is None:
                rc = L.vsom_batch_epoch(h, p["sigma"][k], int(p["first"]), C.byref(m))
            else:
                rc = L.vsom_batch_epoch_masked(h, p["sigma"][k], int(p["first"]), vp, one, C.byref(m))
            out["mse"] = np.float32(m.value)
        elif name in ("ens_schedule", "ens_schedule_masked"):
            sg = np.array([_nan(v) for v in p["sigmas"][k]], np.float64)
            if not sg.size:
                return out
            mses = np.zeros(sg.size, np.float32)
            if vb is None:
                rc = L.vsom_batch_schedule(h, sg.ctypes.data_as(dp), sg.size, int(p["reset"]), f(mses))
            else:
                rc = L.vsom_batch_schedule_masked(h, sg.ctypes.data_as(dp), sg.size, int(p["reset"]), vp, one, f(mses))
            out["mses"] = mses
        elif name in ("ens_online", "ens_online_masked"):
            lb = np.zeros(int(L.vsom_chunk_size(h)), np.uint64)
            args = (h, p["eta"][k], p["sigma"][k], p["decay"][k], int(p["first"]))
            if vb is None:
                rc = L.vsom_train_online_chunk_fetch(*args, u(lb), C.byref(m))
            else:
                rc = L.vsom_train_online_chunk_masked(*args, vp, one, u(lb), C.byref(m))
            out.update(mse=np.float32(m.value), lb=lb)
        elif name == "ens_bmu":
            B = int(L.vsom_chunk_size(h))
            idx, dist = np.zeros(B, np.uint64), np.zeros(B, np.float32)
            rc = L.vsom_bmu_batch(h, u(idx), f(dist))
            out.update(idx=idx, dist=dist)
        else:
            um = np.zeros(self.gb[n].N, np.float64)
            rc = L.vsom_umatrix(h, um.ctypes.data_as(dp))
            out["u"] = um
        self.capi.check(rc)
        return out

    def observe(self, n):
        return self.gb[n].observe(self.gb[n].ctx)

    def observe_twin(self, n):
        return self.gb[n].observe(self.twin[n])


# ---- the ensemble_query profile ----------------------------------------------------------------------------------------
# The four query calls of include/vsom_hip.h, "ensembles" -- vsom_ensemble_bmu_masked_batch, _similarity_masked_batch,
# _bmu_topk_batch, _bmu_topk_masked_batch (with vsom_ensemble_topk_applies) -- walked with the ensemble profile's calls
# between them.  Ops: ("ens_bmu_masked", {e, masks, min_hits[], fill[]}), ("ens_similarity_masked", {e, masks, min_hits[],
# num_sigmas[], rule, delta[]}), ("ens_topk", {e, cover[], k[], dist[]}), ("ens_topk_masked", {e, masks, k[], min_hits[],
# dist[], count[], nvalid[]}); masks names the covered members (ens_mask specs), every other member is skipped; the boolean
# lists say which optional output pointers are non-NULL.  generate_ensemble_query's docstring lists the runs.
ENSQ_CALLS = ("ens_bmu_masked", "ens_similarity_masked", "ens_topk", "ens_topk_masked")
ENSQ_MASKED = ("ens_bmu_masked", "ens_similarity_masked", "ens_topk_masked")
ENSQ_NEW_OPS = set(ENSQ_CALLS) | {"similarity_masked", "topk_masked", "bmd_masked", "generate_masked"}
ENSQ_MASKABLE = ("A", "A2", "B", "D", "D2", "Q")      # the model checks every row of these (B * N <= ENSQ_ALL_ROWS)
ENSQ_DRAWS = 6                       # random draws of an ensemble_query walk, around its runs
ENSQ_RUNS = tuple(range(1, 9))
ENSQ_K = (1, 2, 8, 64)
ENSQ_ALL_ROWS = 32768                # B * N up to which the model checks every row of a covered member
ENSQ_SAMPLE = 8                      # ... beyond it: this many rows (row 0, the last, the row without a valid column)
ENSQ_REFUSALS = ("null_valid", "null_out", "null_k", "null_num_sigmas", "bad_rule", "clr", "no_chunk", "k0", "k65", "k9",
                 "null_idx")                                       # run 6, every configuration
ENSQ_REFUSALS_OWN = ("custom",)                                    # ... the one that needs the custom member F
QNAN32 = np.uint32(0x7FC00000)


def masked_query_fast(cfg, B):
    """include/vsom_hip.h, vsom_ensemble_bmu_masked_batch: the member runs in ensemble_masked_many_kernel -- Standard /
    Median, not custom, B > 0, N * D <= 4096.  (The LDS term 768 + 4 N D is at most 17152 bytes there: it never binds.)"""
    N, D = cfg["W"] * cfg["H"], po.length(cfg["tr"], cfg["J"])
    return not cfg["custom"] and cfg["tr"] != po.CLR and B > 0 and N * D <= 4096


def topk_fast(cfg, B, k, masked):
    """vsom_ensemble_topk_applies as include/vsom_hip.h states it: not custom, B > 0, 1 <= k <= min(64, N),
    N * part_len <= 4096 (part_len: D, or D / 2 for CLR), no CLR member in the masked call.  (The LDS term
    512 + 512 (k | 1) + 4 N D is at most 512 + 512 * 65 + 4 * 2 * 4096 = 66560 bytes only for a CLR map at k = 64 with
    N * part_len = 4096; for the members here it is at most 50176: it never binds.)"""
    N, D = cfg["W"] * cfg["H"], po.length(cfg["tr"], cfg["J"])
    part = D // 2 if cfg["tr"] == po.CLR else D
    return not cfg["custom"] and B > 0 and 1 <= k <= min(64, N) and N * part <= 4096 and \
        not (masked and cfg["tr"] == po.CLR)


def covered(op, order):
    """the members a query call covers, in member order"""
    name, p = op
    if name == "ens_topk":
        return [n for n, c in zip(order, p["cover"]) if c]
    return [n for n in order if n in p["masks"]]


def ensq_stats():
    return {"accepted": {c: 0 for c in ENSQ_CALLS}, "mixed": {c: 0 for c in ENSQ_CALLS}, "applies": 0, "padded": 0,
            "novalid": 0, "b0": 0, "ahead_skipped": 0, "met": {}, "covered_rows": {}, "model_rows": {}}


# -- the model's distances: pure Python (about 12 us a distance), cached by content, so that the calls of one block and the
# CPU fake (tests/test_call_sequences_model.py), which states the same function of ITS state, share them
_DIST_CACHE = {}


def _digest(*arrays):
    import hashlib
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.shape, a.dtype)).encode())
        h.update(a.tobytes())
    return h.digest()


def _cached(key, make):
    if key not in _DIST_CACHE:
        if len(_DIST_CACHE) > 256:
            _DIST_CACHE.clear()
        _DIST_CACHE[key] = make()
    return _DIST_CACHE[key]


def masked_distances(mod, X, V):
    """masked_score_ref.masked_dists of the rows X under the validity V to every node of the member's map: rows x N"""
    import masked_score_ref as msr
    M = mod.som.map
    def make():
        with np.errstate(all="ignore"):
            return np.array([msr.masked_dists(mod.cfg["tr"], x, M, v) for x, v in zip(X, V)], np.float32).reshape(len(X), mod.N)
    return _cached(("masked", mod.cfg["tr"], _digest(M, X, V)), make)


def plain_distances(mod, rows):
    """the oracle's own distance (Model._dist) of the chunk's rows `rows` to every node: rows x N"""
    def make():
        with np.errstate(all="ignore"):
            return np.array([mod._dist(np.arange(mod.N), np.full(mod.N, r)) for r in rows], np.float32).reshape(len(rows), mod.N)
    return _cached(("plain", mod.cfg["tr"], mod.cfg["J"], _digest(mod.som.map, mod.X[rows])), make)


def model_rows(mod, valid, p, k):
    """The rows of a covered member the model checks: all of them where B * N <= ENSQ_ALL_ROWS; on the larger members a
    seeded sample of ENSQ_SAMPLE rows with row 0, the last row and the row without a valid column, if the mask has one"""
    B = mod.B
    if B * mod.N <= ENSQ_ALL_ROWS:
        return np.arange(B)
    rows = {0, B - 1}
    if valid is not None and np.ndim(valid) == 2:
        rows |= set(np.flatnonzero(~(np.asarray(valid) != 0).any(axis=1))[:1].tolist())
    rs = np.random.RandomState([B, k, mod.N])
    for r in rs.permutation(B):
        if len(rows) >= ENSQ_SAMPLE:
            break
        rows.add(int(r))
    return np.array(sorted(rows))


def _searched(d, hits, min_hits):
    """masked_score_ref.argmin_rule per row of distances; a NaN distance is 0x7FC00000"""
    import masked_score_ref as msr
    with np.errstate(all="ignore"):
        got = [msr.argmin_rule(row, hits, min_hits) for row in d]
    bmu = np.array([b for b, _ in got], np.uint64)
    dist = np.array([v for _, v in got], np.float32)
    dist[np.isnan(dist)] = QNAN32.view(np.float32)
    return bmu, dist


def query_member(mod, name, p, k, valid, rows, hits=None, sigma=None):
    """what one covered member's share of a query call returns for the chunk's rows `rows`, from the plain references:
    masked_score_ref (masked_dists, argmin_rule, similarity), topk_masked_ref (lists, nvalid, keys' order over the
    oracle's own distances for the plain call); fill is x at valid columns and the unit's map row elsewhere"""
    import masked_score_ref as msr
    import topk_masked_ref as tmr
    s = mod.som
    hits = s.hits if hits is None else hits
    if name == "ens_topk":
        idx, dist, _ = tmr.lists(plain_distances(mod, rows), hits, 0, p["k"][k])
        return {"idx": idx, "dist": dist}
    X = mod.X[rows]
    V = np.broadcast_to(np.asarray(valid) != 0, mod.X.shape)[rows]
    d = masked_distances(mod, X, V)
    nvalid = V.sum(axis=1).astype(np.uint32)
    mh = p["min_hits"][k]
    if name == "ens_topk_masked":
        idx, dist, count = tmr.lists(d, hits, mh, p["k"][k])
        return {"idx": idx, "dist": dist, "count": count, "nvalid": nvalid}
    bmu, dist = _searched(d, hits, mh)
    b = bmu.astype(np.int64)
    if name == "ens_bmu_masked":
        return {"bmu": bmu, "dist": dist, "nvalid": nvalid, "fill": np.where(V, X, s.map[b]).astype(np.float32)}
    with np.errstate(all="ignore"):
        out = msr.similarity(X, s.map[b], (s.sigma if sigma is None else sigma)[b], p["num_sigmas"][k], p["rule"] == 1, V)
    out.update(bmu=bmu, dist=dist, nvalid=nvalid)
    return out


MEMBER_QUERIES = ("topk", "topk_masked", "similarity_masked", "bmd_masked", "generate_masked")
BMD_RTOL = 1e-15                     # norm and prob against the float64 restatement: tests/test_gpu_bmd_masked.py's RTOL


def member_query(mod, op, a):
    """The single-context queries this profile draws on a member, for its rows [r0, r1), from the plain references:
    topk_masked_ref (lists, nvalid, blend within blend_bound), masked_score_ref.similarity, bmd_masked_ref (distribution,
    draws, records within generate_ref.bound).  What depends on the device's exp or log is a Within; a draw within
    bmd_masked_ref.NEAR of a cumulative boundary is not compared, nor is the record around it."""
    import bmd_masked_ref as bmr
    import generate_ref as gr
    import masked_score_ref as msr
    import topk_masked_ref as tmr
    name, p = op
    s = mod.som
    rows = np.arange(p["r0"], p["r1"])
    if name == "topk":
        idx, dist, _ = tmr.lists(plain_distances(mod, rows), s.hits, 0, p["k"])
        return {"r0": idx, "r1": dist}
    X = mod.X[rows]
    V = np.broadcast_to(a["valid"] != 0, X.shape)
    d = masked_distances(mod, X, V)
    nvalid = V.sum(axis=1).astype(np.uint32)
    if name == "topk_masked":
        idx, dist, count = tmr.lists(d, s.hits, p["min_hits"], p["k"])
        out = {"idx": idx, "dist": dist, "count": count, "nvalid": nvalid}
        if p["blend"]:
            want, mass = tmr.blend(X, V, s.map, idx, dist, count)
            bound = np.where(V | ~mass[:, None], 0.0, tmr.blend_bound(s.map, idx, count, p["k"]))
            out["blend"] = Within(want, bound)
        return out
    if name == "similarity_masked":
        bmu, dist = _searched(d, s.hits, p["min_hits"])
        b = bmu.astype(np.int64)
        with np.errstate(all="ignore"):      # (GpuBackend._call1: two sigmas, with delta)
            out = msr.similarity(X, s.map[b], s.sigma[b], 2, p["rule"] == 1, V)
        out.update(bmu=bmu, dist=dist, nvalid=nvalid)
        return out
    P, norm, prob = bmr.distribution(d, s.hits, p["min_hits"])
    unit, near = bmr.draws(P, a["u"])
    clear = near > bmr.NEAR
    if name == "bmd_masked":
        with np.errstate(all="ignore"):
            return {"norm": Within(norm, BMD_RTOL * np.abs(norm)), "prob": Within(prob, BMD_RTOL * np.abs(prob)),
                    "draw": Within(unit, np.where(clear, 0.0, np.inf))}
    rec, zs, kept = bmr.records(s.map, s.sigma, unit, a["l"], X, V, True)
    with np.errstate(all="ignore"):
        bound = np.where(kept, 0.0, gr.bound(rec, zs))
    return {"unit": Within(unit, np.where(clear, 0.0, np.inf)),
            "record": Within(rec, np.where(clear[:, :, None], bound, np.inf))}


def words(a):
    """an array as its words: floats as unsigned integers of their width, so that NaN payloads and signs compare"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


# outputs whose NaN is computed, not defined: the similarity words, and fill, which copies the map at invalid columns -- a
# NaN there was computed by an earlier epoch (x is finite wherever it is valid), on the host with the host's payload
ARITHMETIC_NAN = ("dmax", "first", "amax", "delta", "fill")


def query_difference(got, exp, key=None):
    """A query output against the model, on the words: every bit, NaN payloads included -- the header fixes every NaN these
    calls store by definition (0x7FC00000 for a NaN distance and for the padding of a short list, UINT64_MAX for its
    units).  Only the outputs of ARITHMETIC_NAN, where a NaN is the result of the CPU's own arithmetic (a NaN in the map or
    the sigmaMap), compare as values with NaN equal to NaN; every other bit of them, the sign of a zero included, counts."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return f"a shape / type: returned {got.shape} {got.dtype} values, expected {exp.shape} {exp.dtype}"
    if key in ARITHMETIC_NAN:
        return first_difference_exact(got, exp)
    d = first_difference_exact(words(got), words(exp))
    if d and exp.dtype.kind == "f":
        at = np.unravel_index(int(np.argmax(words(got).reshape(-1) != words(exp).reshape(-1))), exp.shape)
        d += f"; as values: got {got[at]!r}, expected {exp[at]!r}"
    return d


class _EnsqGen(_EnsGen):
    """the ensemble profile's generator and the four query calls"""

    def slow(self):
        return "G" if "G" in self.all else "E"

    def kfor(self, n, k=None):
        """a k of ENSQ_K for member n: k = N = 8 on D and D2 instead of 8 and 64"""
        k = ENSQ_K[self.r(len(ENSQ_K))] if k is None else k
        N = config(n)["W"] * config(n)["H"]
        return min(k, N) if k in ENSQ_K else k       # (a refusal's k -- 0, 65, 9 -- stays as it is)

    def train(self, kind, e=0, masks=None, **kw):
        if kind == "ens_online_masked" and masks:      # (D2's 513 columns as D's 512: on 3 rows only)
            masks = {n: s for n, s in masks.items() if n != "D2" or (self.B[n] or 0) <= 40}
        return super().train(kind, e, masks=masks, **kw)

    def q(self, kind, e=0, cover=(), masks=None, k=None, min_hits=None, flags=None, full=None, **tags):
        """One query call.  cover: the covered members' names (every other member is skipped); masks: specs to reuse (the
        rows are poisoned for them), a covered member without one gets a fresh spec; k / min_hits: one value, a dict per
        member, or drawn; flags[output]: True / False / a set of member names with a non-NULL pointer, else drawn"""
        order = self.ens[e]
        cover = [n for n in order if n in cover]
        K = len(order)
        p = dict(e=e)

        def per(v, draw):
            return [int(v[n]) if isinstance(v, dict) and n in v else (draw(n) if v is None or isinstance(v, dict) else int(v))
                    for n in order]

        def flag(key):
            v = (flags or {}).get(key)
            if v is None:
                return [bool(self.r(2)) for _ in range(K)]
            return [v] * K if isinstance(v, bool) else [n in v for n in order]

        if kind == "ens_topk":
            p["cover"] = [n in cover for n in order]
        else:
            new = [n for n in cover if n not in (masks or {})]
            fresh = self.specs(e, names=new, full=full) if new else {}
            p["masks"] = {n: dict((masks or {}).get(n) or fresh[n]) for n in cover}
        if kind in ("ens_topk", "ens_topk_masked"):
            p["k"] = per(k, lambda n: self.kfor(n))
            p["k"] = [self.kfor(n, v) for n, v in zip(order, p["k"])]
        if kind != "ens_topk":
            p["min_hits"] = per(min_hits, lambda n: self.r(3))
        if kind == "ens_bmu_masked":
            p["fill"] = flag("fill")
        elif kind == "ens_similarity_masked":
            p.update(num_sigmas=[1 + self.r(3) for _ in range(K)], rule=self.r(2), delta=flag("delta"))
        elif kind == "ens_topk":
            p["dist"] = flag("dist")
        else:
            p.update(dist=flag("dist"), count=flag("count"), nvalid=flag("nvalid"))
        p.update(tags)
        self.emit(kind, **p)

    def four(self, e=0, cover=(), masks=None, **kw):
        """the four calls over one cover, the three masked ones under the same masks (the model's distances are shared)"""
        names = [n for n in self.ens[e] if n in cover and n not in (masks or {}) and n != "C"]
        masks = dict(masks or {}, **(self.specs(e, names=names) if names else {}))
        for kind in ENSQ_CALLS:
            self.q(kind, e, cover=[n for n in cover if n != "C" or kind == "ens_topk"], masks=masks, **kw)

    def maskable(self, e=0):
        return [n for n in self.ens[e] if n in ENSQ_MASKABLE]

    def some(self, e=0, slow=None):
        """a cover for a drawn query: two or more of the small members but not all of them, the slow member in half"""
        names = self.maskable(e)
        self.rs.shuffle(names)
        names = names[:max(2, 1 + self.r(len(names) - 1))] if len(names) > 2 else names
        if (self.r(2) if slow is None else slow) and self.slow() in self.ens[e]:
            names = names + [self.slow()]
        return names

    def member_query(self):
        """a single-context query on a small member: the ones this profile adds beside bmu_masked"""
        n = self.maskable()[self.r(len(self.maskable()))]
        B = self.B[n] or 0
        if B == 0:
            return
        k = 1 + self.r(min(32, B))
        r0 = self.r(B - k + 1)
        w = dict(r0=r0, r1=r0 + k, seed=self.r(1 << 30))
        N = config(n)["W"] * config(n)["H"]
        form = ["rows", "one_mask"][self.r(2)]
        what = ["similarity_masked", "topk", "topk_masked", "bmd_masked", "generate_masked"][self.r(5)]
        if what == "similarity_masked":
            self.m(n, what, min_hits=self.r(2), rule=self.r(2), form=form, **w)
        elif what == "topk":
            self.ops.append(("m", {"k": n, "op": (what, dict(k=min(N, ENSQ_K[self.r(4)]), r0=w["r0"], r1=w["r1"]))}))
        elif what == "topk_masked":
            self.ops.append(("m", {"k": n, "op": (what, dict(k=min(N, ENSQ_K[self.r(4)]), min_hits=self.r(3),
                                                           blend=bool(self.r(2)), form=form, **w))}))
        elif what == "bmd_masked":
            self.m(n, what, min_hits=self.r(2), form=form, **w)
        else:
            self.m(n, what, min_hits=self.r(2), draws=[1, 3][self.r(2)], form=form, **w)

    def random_op(self, e=0):
        what = self.r(10)
        if what < 4:
            self.q(ENSQ_CALLS[what], e, cover=self.some(e) + (["C"] if what == 2 and "C" in self.ens[e] and self.r(2) else []))
        elif what == 4:
            self.member_query()
        else:
            super().random_op(e)

    # ---- the runs ----
    def qrun(self, run):
        own = not self.ec["one_stream"]
        e, S = 0, self.slow()
        small = self.maskable(e)
        # (every run starts from clean rows; short chunks: the model's masked distance is pure Python)
        self.upload(e, {"A": 0, "A2": 0, "B": 0, "Q": 1}, wait=1)
        self.emit("run", id=run)
        if run == 1:
            pick = {"A": 0, "A2": 0, "B": 0, "C": 0, "D": 1, "D2": 1, "Q": 3, "E": 0, "F": 0, "G": 0}
            tm = self.specs(e, names=[n for n in small if n != "D2"], full="A")
            skip = [n for n in small if n not in ("A", "Q")]
            cov = lambda i: [n for n in small if n != skip[i % len(skip)]] + [S]
            self.upload(e, pick, wait=0, poison=tm)
            self.train("ens_epoch_masked", e, masks=tm, first=True)
            self.q("ens_bmu_masked", e, cover=cov(0), masks=tm, flags={"fill": True})
            self.train("ens_schedule_masked", e, masks=tm, sigmas=[[self.sigma()] for _ in self.ens[e]])
            self.q("ens_topk_masked", e, cover=cov(1), masks=tm)
            self.train("ens_online_masked", e, masks=tm, first=True)
            self.q("ens_similarity_masked", e, cover=cov(2), masks=tm, flags={"delta": True})
            big = {"A": 3, "A2": 3, "B": 2, "C": 1, "D": 1, "D2": 1, "Q": 5, "E": 2, "F": 1, "G": 1}
            self.upload(e, big, wait=0)      # more floats than the first: the raw buffer grows behind the stagings
            self.q("ens_topk", e, cover=[n for n in self.ens[e] if n not in ("F", skip[0])])
            self.train("ens_epoch", e, first=True)         # covers every member: the pinned rows may change behind it
        elif run == 2:
            self.upload(e, {"A": 0, "A2": 0, "B": 0, "D": 1, "D2": 1, "Q": 3, "E": 0, "G": 0})
            tm = self.specs(e, names=small + [S], full="Q")
            wide = [n for n in self.ens[e] if n != "F"]
            self.q("ens_similarity_masked", e, cover=small + [S], masks=tm, flags={"delta": True})
            self.q("ens_topk", e, cover=wide[:-1] if S == wide[-1] and not own else wide[1:], k=64, flags={"dist": True})
            self.q("ens_bmu_masked", e, cover=["A", "Q"], masks=tm, flags={"fill": False})
            self.q("ens_topk", e, cover=wide[1:], k=1)
            self.q("ens_topk_masked", e, cover=small[1:] + [S], masks=tm, k={"A": 2, "B": 8, "Q": 64, "D": 8, "D2": 1, S: 2},
                   flags={"dist": set(small[1:-1]), "count": set(small[2:]) | {S}, "nvalid": set(small[1:3]) | {S}})
            self.q("ens_bmu_masked", e, cover=small[:-1] + [S], masks=tm, flags={"fill": {"B"}})
        elif run == 3:
            self.upload(e, {"A": 0, "A2": 0, "B": 0, "D": 0, "D2": 0, "Q": 1, "E": 0, "G": 0})
            self.m("A", "set_last_bmu", seed=self.r(1 << 30))
            self.m("Q", "set_last_bmu", seed=self.r(1 << 30))
            tm = self.specs(e, names=small + [S])
            self.four(e, cover=[n for n in self.ens[e] if n in tm or n == "C"], masks=tm)
            for n in self.ens[e]:
                for what in ("get_last_bmu", "get_sqres", "get_mse"):
                    self.m(n, what)
            self.train("ens_epoch", e, first=False)
            self.m("B", "set_state", seed=self.r(1 << 30), parts="hits0")
            self.m("A", "set_state", seed=self.r(1 << 30), parts="all")
            for again in range(2):
                self.q("ens_bmu_masked", e, cover=small[:-1], masks=tm, min_hits=1)
                self.q("ens_similarity_masked", e, cover=small[1:] + [S], masks=tm, min_hits=2, flags={"delta": True})
                self.q("ens_topk_masked", e, cover=small, masks=tm, min_hits={"A": 2, "B": 1, "Q": 2}, k={"A": 8, "B": 8, "Q": 2},
                       flags={"dist": True, "count": True, "nvalid": True})
                if not again:
                    self.train("ens_online", e, first=True)
        elif run == 4:
            for i, c in enumerate((1, 2, 3, 5, 0)):          # Q at 63, 64, 65, 129 rows and at 1
                self.upload(e, {"Q": c, "D": i % 2, "D2": i % 2, "A": 0, "A2": 0, "B": 0, "E": 0, "G": 0})
                if i == 1:
                    self.m("A", "bmu_mode", mode=BMU_EXACT)
                    self.m("A", "update_mode", mode=UPDATE_FMA)
                self.four(e, cover=["A", "D", "D2", "Q"] + ([S] if i in (1, 4) else []) + (["B"] if i == 2 else []))
                if i == 1:
                    self.m("A", "update_mode", mode=UPDATE_STRICT)
                    self.m("A", "bmu_mode", mode=BMU_AUTO)
            if "E" in self.ens[e]:           # a NaN sigma: E's map is NaN when the queries read it
                self.train("ens_schedule", e, sigmas=[[2.5, None] if n == "E" else [] for n in self.ens[e]], reset=False)
                self.four(e, cover=["A", "Q", "E"], labels=["nan_map"])
                self.m("E", "get_state")
                self.m("E", "set_state", seed=self.r(1 << 30), parts="all")
        elif run == 5:
            ahead = S if stages_ahead(config(S)) else None
            self.m(S, "upload", chunk=0, asynchronous=False)
            self.m(S, "epoch_async", sigma=self.sigma(), first=True)
            self.m(S, "prefetch", chunk=0, src="pinned")
            tm = self.specs(e, names=["A", "Q", S])
            for kind in ENSQ_CALLS:          # covered: MUST be refused where the chunk is staged ahead, naming the member
                self.q(kind, e, cover=["A", "Q", S], masks=tm, **({"must_refuse": ahead} if ahead else {}))
            for kind in ENSQ_CALLS:          # skipped: accepted
                self.q(kind, e, cover=["A", "Q"], masks=tm, **({"ahead_skipped": ahead} if ahead else {}))
            self.m(S, "commit")
            for kind in ENSQ_CALLS:
                self.q(kind, e, cover=["A", "Q", S], masks=tm)
        elif run == 6:
            tm = self.specs(e, names=["A", "D", "Q"])
            for kind in ENSQ_MASKED:
                self.q(kind, e, cover=["A", "D", "Q"], masks=tm, bad="null_valid")
            for kind in ENSQ_CALLS:
                self.q(kind, e, cover=["A", "D", "Q"], masks=tm, bad="null_out")
            for kind in ("ens_topk", "ens_topk_masked"):
                self.q(kind, e, cover=["A", "D", "Q"], masks=tm, bad="null_k")
            self.q("ens_similarity_masked", e, cover=["A", "Q"], masks=tm, bad="null_num_sigmas")
            self.q("ens_similarity_masked", e, cover=["A", "Q"], masks=tm, bad="bad_rule")
            if own:
                for kind in ENSQ_CALLS:
                    self.q(kind, e, cover=["A", "Q", "F"], masks=tm)
            for kind in ENSQ_MASKED:
                self.q(kind, e, cover=["A", "C", "Q"], masks=tm)
            self.q("ens_topk", e, cover=["A", "C", "Q"], labels=["topk_clr"])       # accepted
            for kind in ("ens_topk", "ens_topk_masked"):
                self.q(kind, e, cover=["A", "D", "Q"], masks=tm, k={"A": 0, "D": 8, "Q": 2})
                self.q(kind, e, cover=["A", "D", "Q"], masks=tm, k={"A": 65, "D": 8, "Q": 2})
                self.q(kind, e, cover=["A", "D", "Q"], masks=tm, k={"A": 2, "D": 9, "Q": 2})
                self.q(kind, e, cover=["A", "Q"], masks=tm, k={"A": 2, "D": 9, "Q": 2}, labels=["k_of_a_skipped_member"])
            self.q("ens_topk_masked", e, cover=["A", "D", "Q"], masks=tm, bad="null_idx", null_idx="D")
        elif run == 7:
            old = list(self.ens[0])
            self.emit("ens_destroy", e=0)
            del self.ens[0]
            self.ens[0] = old                # (member_query draws among the former members)
            for _ in range(6):
                self.member_query()
            del self.ens[0]
            sub = [n for n in old if n != ("F" if own else "C")]
            sub = [sub[i] for i in self.rs.permutation(len(sub))]
            self.emit("ens_create", e=0, order=sub)
            self.ens[0] = sub
            self.ens[1] = [n for n in reversed(sub) if n in ENSQ_MASKABLE][:3]
            self.emit("ens_create", e=1, order=self.ens[1])
            for i in range(4):
                self.q(ENSQ_CALLS[i], 0, cover=self.some(0, slow=i % 2))
                self.q(ENSQ_CALLS[(i + 1) % 4], 1, cover=self.ens[1][:2] if i % 2 else self.ens[1])
            empty = self.ens[1][1]
            self.upload(1, {"A": 0, "A2": 0, "B": 0, "Q": 2})
            self.ops[-1][1]["rows"][empty] = {"chunk": 0, "head": 0}      # B = 0: that member writes nothing
            self.B[empty] = 0
            self.four(1, cover=self.ens[1], labels=["b0"])
            self.four(0, cover=[n for n in self.maskable(0)[:3]] + [empty])
            self.upload(1)
            self.emit("ens_destroy", e=1)
            del self.ens[1]
            self.four(0, cover=self.some(0, slow=1))
            self.emit("ens_destroy", e=0)
            del self.ens[0]
        self.emit("run_end", id=run)
        self.m(self.all[self.r(len(self.all))], "get_state")


def generate_ensemble_query(cfg_name, seed, n_ops=ENSQ_DRAWS):
    """The ensemble_query profile: n_ops random draws -- the four query calls and single-context queries on members mixed
    into the ensemble profile's draws (training calls, masked blocks, uploads, member ops) -- around these runs, each
    between ("run", id) / ("run_end", id) markers.  Run 8 and the refusals of run 6 that need a member without a chunk open
    the walk; runs 1-6 follow in a drawn order, run 7 ends the walk.
      1  back to back, no wait: upload_chunks(wait = 0) of rows poisoned for the masks from pinned memory, batch_epoch_masked,
         bmu_masked (fill), batch_schedule_masked, bmu_topk_masked, train_online_chunk_masked, similarity_masked (delta) --
         six images of different sizes through the two descriptor slots, training tables and query images in turn --; a
         second, larger upload_chunks(wait = 0) of clean rows and bmu_topk at once behind it; a batch epoch, which covers
         every member, ends the run.  Every query covers the slow member (E / G) and skips one
      2  the result buffers shrink and change their layout, on one set of rows: similarity_masked with delta for every small
         member, bmu_topk with k = 64 where N allows, bmu_masked without fill over two members, bmu_topk with k = 1,
         bmu_topk_masked with mixed k and dist / count / nvalid each NULL for some member, bmu_masked with fill for one
      3  read-only, and the live state: vsom_set_last_bmu on A and Q, the four queries, every member's lastBMU / sqres / MSE,
         batch_epoch(is_first = 0); bmuHits all zero on B and mixed on A, the masked queries with min_hits 1 and 2, an
         ensemble online chunk, the same queries again
      4  path borders: Q at 63, 64, 65, 129 and 1 rows between two calls of each kind, D and D2 in the same calls; A's search
         mode EXACT and its update mode non-strict around one block; E (ensq_shared) queried with a NaN map
      5  the stage-ahead: an asynchronous epoch and a prefetch on G (ensq_own; E on ensq_shared, where nothing stages ahead):
         the four calls covering it MUST be refused naming it, with it skipped they are accepted; after the commit accepted
      6  every refusal the header lists for the four calls; bmu_topk accepts the CLR member; a skipped member may hold any k
      7  destroy, single-context queries on former members, create over a permuted subset and a second ensemble over an
         overlapping subset in another order, queries alternating between the two, an upload that leaves a member B = 0
      8  G (ensq_own): an epoch under VSOM_SIGMA_LAZY before the first create, create, a batch epoch, similarity_masked
         covering G on its single-call path"""
    g = _EnsqGen(cfg_name, seed)
    g.ops.append(("config", {"name": cfg_name, "seed": seed, "profile": "ensemble_query"}))
    own = "G" in g.all
    for n in g.all:
        g.m(n, "set_state", seed=seed + config(n).get("map_seed", 0), parts="init")
    if own:
        g.emit("run", id=8)
        g.m("G", "sigma_mode", mode="lazy")
        g.m("G", "upload", chunk=0, asynchronous=False)
        g.m("G", "epoch", sigma=g.sigma(), first=True)
        g.emit("sigma_stats", k="G", expect=[1, 0, 0, 1])
    for n in g.all:
        if n not in ("C", "G", "Q"):
            g.m(n, "upload", chunk=0, asynchronous=False)
    g.emit("ens_create", e=0, order=list(g.all))
    g.ens[0] = list(g.all)
    if own:
        g.emit("sigma_stats", k="G", expect=[1, 0, 1, 0])
    # C and Q have no chunk yet: refused where covered, accepted where skipped
    g.emit("run", id=6)
    g.q("ens_topk", 0, cover=["A", "C"])
    for kind in ENSQ_MASKED:
        g.q(kind, 0, cover=["A", "Q"])
    g.four(0, cover=["A", "D", "D2"], labels=["no_chunk_skipped"])
    g.emit("run_end", id=6)
    g.upload(0, {n: 0 for n in g.all})
    if own:
        g.train("ens_epoch", 0, first=True)
        g.q("ens_similarity_masked", 0, cover=["A", "Q", "G"], flags={"delta": True}, labels=["lazy_sigma"])
        g.m("G", "get_state")
        g.emit("run_end", id=8)
    slots = sorted(g.rs.choice(np.arange(0, n_ops), 6, replace=False)) if n_ops >= 6 else [0] * 6
    runs = [int(r) for r in g.rs.permutation(6) + 1]
    for k in range(n_ops):
        while slots and k >= slots[0]:
            slots.pop(0)
            g.qrun(runs.pop(0))
        g.random_op()
    while runs:
        g.qrun(runs.pop(0))
    g.qrun(7)
    for n in g.all:
        g.m(n, "get_state")
    return g.ops


def ensq_conditions(cfg_name, stats, gpu=False):
    """what a walk of the ensemble_query profile must have met, from run_ensemble_walk's counts: it cannot pass vacuously"""
    own = not ENSQ_CONFIGS[cfg_name]["one_stream"]
    q = stats["q"]
    assert all(q["accepted"][c] >= 4 for c in ENSQ_CALLS), q["accepted"]
    # each call: two or more members in the many-member kernel, one on its single call and one skipped, together
    assert all(q["mixed"][c] >= 1 for c in ENSQ_CALLS), q["mixed"]
    for label in ENSQ_REFUSALS + (ENSQ_REFUSALS_OWN if own else ()):
        assert stats["refusals"].get("q_" + label, 0) >= 1, (label, stats["refusals"])
    for label in ("no_chunk_skipped", "topk_clr", "k_of_a_skipped_member", "b0"):
        assert q["met"].get(label, 0) >= 1, (label, q["met"])
    assert stats["refusals"].get("q_staged", 0) == (4 if own else 0) and q["ahead_skipped"] == (4 if own else 0), (stats, q)
    assert q["padded"] >= 1 and q["novalid"] >= 1 and q["b0"] >= 1, q
    assert q["applies"] >= 20, q
    for n in ENSQ_MASKABLE:                  # the sample rule of the large members is the only place the model leaves rows out
        assert q["covered_rows"].get(n, 0) == q["model_rows"].get(n, 0), (n, q["covered_rows"], q["model_rows"])
        assert n not in ens_config(cfg_name)["members"] or q["covered_rows"].get(n, 0) > 0, n
    if gpu:
        assert stats["nowait"] >= 2, stats
