"""GPU: seeded random walks over the single-context C ABI (tests/callseq.py) against the CPU oracle.

Asynchronous ingest is correct only if every entry point keeps the context's staging flags right, along every call order
a C caller can make -- not only the orders other tests script.  Each walk mixes uploads, prefetches from pinned and
pageable memory, chunks handed over in HBM, commits, whole and split batch epochs, online chunks with and without a
wait, single steps, searches, distance queries, lastBMU / state reads and writes and search-mode switches; it holds by
construction the runs in which nothing synchronises between an asynchronous epoch and a prefetch's staging.  Every
accepted call returns the oracle's values bit for bit; a call that reads the staged rows while a chunk is pending may be
refused (naming the commit).  A failure prints the seed and the ops; callseq.replay(ops) reruns them.

The sigma walks (callseq.generate_sigma) do the same for the pending sigmaMap (include/vsom_hip.h, vsom_set_sigma_mode):
under VSOM_SIGMA_LAZY and VSOM_SIGMA_AUTO they mix the sigma modes, the flush, the column compaction, whole-map phase-2
ranges, empty chunks, the masked epoch, partial vsom_set_state calls, the sigmaMap readers and the arena queries into the
ingest ops, and hold the runs that keep a record pending across a stage-ahead and its commit, a lastBMU write, a
reallocating upload, an empty chunk, an online chunk without a wait and a weight-only state write.  After every call
vsom_sigma_stats must equal what the header's contract gives (callseq.SigmaRecord); what the readers, the arena queries and
the masked epoch return must equal, bit for bit, what a second context fixed at VSOM_SIGMA_EAGER returns for the same calls;
the state of both is the oracle's.  std80 launches 700 chain workgroups, so its deferred epochs take the two-quad mean-only
kernels (callseq.two_quad_launch mirrors the rule; the library cannot say which kernel ran: the counters prove the
deferral, tests/test_gpu_mean_nt8.py explains).

Cost of a sigma walk, measured as the walk against the CPU fake of tests/test_call_sequences_model.py at this test's scale.
The fake runs the oracle a second time, so the model's share -- what this test pays beside the GPU calls -- is about half
of each figure.  Seeds 1 and 2, lazy / auto, in seconds: std48 4.1, 3.5 / 4.0, 3.9; med48 4.7, 4.6 / 7.7, 4.4; std80 2.2,
2.8 / 2.2, 2.9; std12, clr12, custom12 at most 0.1 each.  (The ingest walks measure 0.03 to 15 the same way.)  The oracle's
serial online scan is what a walk can spend most on: the sigma profile draws it less often, on chunks of at most 512 rows,
and less often still for med48 and std80 (callseq.CONFIGS, "sigma_weights" / "weights").

The accum walks (callseq.generate_accum) do the same for the accumulated batch epoch (include/vsom_hip.h,
vsom_batch_accum_begin / _chunk / _chunk_masked / _end / _abort), the one protocol whose state lives across calls that do not
block: the pinned validity halves used alternately, chunk scratch in the query arena shared with the queries, staged rows
overwritten behind enqueued chains, the neighbourhood table, the ever-dirty column list, a pending sigmaMap.  Under
VSOM_SIGMA_LAZY and VSOM_SIGMA_AUTO a walk makes callseq.ACCUM_DRAWS random draws -- the sigma profile's ops, whole epochs
of plain and masked chunks ended or aborted, stray calls, the masked scoring calls -- around nine runs it holds by
construction (callseq's module docstring): three masked chunks with no wait between them, growing chunks with an arena query
between, plain / masked / plain in a non-first epoch, an abort and a plain epoch behind it, the stage-ahead refusal, every
refusal of the header (each followed by a comparison of the whole state) with the empty epoch and the empty chunk, a pending
sigmaMap meeting begin, a model rewritten in mid-epoch, and queries in mid-epoch.  The five calls go to the C ABI directly;
the validity bytes are zeroed as soon as a masked chunk call returns; a masked chunk call is given rows with NaN / inf under
every invalid entry of its mask.  The two no-wait runs go to the first context back to back, before the twin or the model
sees a call of them; everywhere else the twin's wait and the model's work stand between two calls, so there the walk tests
the state logic and not the ordering.  Where a prefetch behind an asynchronous epoch stages ahead (callseq.stages_ahead)
the chunk call of run 5 must be refused, and the whole state is compared behind that refusal as behind every other.  Every call returns the oracle's values bit for bit (callseq.Model: phase 1 per chunk, the running MSE
over total_rows, phase 2 over the concatenation at end, dirty columns from tests/masked_train_ref.py), vsom_sigma_stats
follows the header's contract, and a second context -- VSOM_SIGMA_EAGER, fed from pageable memory, synchronised after every
call -- returns the same bits from the readers, the arena queries, the masked epoch and the masked scoring calls, and ends
in the oracle's state.  On clr12 and custom12 begin is refused, every other accum call with it, and the rest of the walk
matches the oracle.

Cost of an accum walk, measured the same way (against the CPU fake, at this test's scale; the model's share is about half).
Seeds 1 and 2, lazy / auto, in seconds: std48 7.3, 5.9 / 6.9, 6.6; med48 7.2, 8.9 / 7.3, 8.8; std80 7.7, 7.9 / 7.8, 8.6;
std12 1.8, 1.5 / 1.8, 2.0; clr12, custom12 at most 0.1.  On an MI355X the tests themselves took 1.7 to 2.6 s (std48), 2.0 s
(med48), 2.0 to 2.2 s (std80), 0.4 to 0.5 s (std12) and under 0.8 s.  The dearest op is the model's full masked search
(tests/masked_train_ref.py, pure Python, 12 us a distance): only run 1 puts masked chunks into a first epoch, three of
them, on chunks of the accum profile alone that are short enough (callseq.CONFIGS, "accum_chunks"; callseq.maskable caps
rows x nodes at callseq.MASK_DISTANCES, 8 times that for the local walk), and a walk makes 12 random draws around its runs
(callseq.ACCUM_DRAWS; with 24 the large maps measured 9 to 17 s); the rest is the phase 2 at end -- run 2 ends on the
configuration's largest chunk by design, and every dirty column costs one single-column oracle run.

The ensemble walks (callseq.generate_ensemble) do the same for the nine vsom_ensemble_* calls (include/vsom_hip.h,
"ensembles"), the object of the C ABI that keeps the most state between calls and shares it between contexts: two descriptor
slots behind events, which also carry the masked calls' tables and validity image, the grow-only raw upload buffer read by
stagings on several streams, the members' neighbourhood-table slots, schedule tables shared between members, and the flag that
changes what the single-context calls do on a member, past or present.  The members (callseq.ENS_MEMBERS) have row counts at
the borders of the path predicates -- a 10 x 10 x 9 map takes the one-launch batch kernel at 160 rows and not at 170, a
12 x 9 x 20 map at 121 and not at 122 -- restated in callseq.batch_tiny / masked_batch_tiny / online_tiny; at every masked call
the walk asks vsom_masked_tiny_applies / vsom_online_masked_tiny_applies for every masked member and fails where a restated
predicate disagrees.  ens_shared puts A, A2 (A's rows by equal offsets), B, C, D, E on one stream, ens_own gives A, B, C, E, F
(custom), G (48 x 48, created under VSOM_SIGMA_LAZY) a stream each.  A walk makes callseq.ENS_DRAWS random draws -- ensemble
calls, masked blocks on poisoned rows, single-context calls on members (uploads, prefetch and commit, partial vsom_set_state,
lastBMU writes, epochs, online chunks, searches, U-matrices, search modes, vsom_batch_schedule and its masked form) -- around
the runs of generate_ensemble's docstring: the no-wait run (six descriptor sizes through two slots, the raw buffer rewritten
behind stagings; sent to the ensemble back to back before the twins and the model see it), the running MSE across ensemble
and single calls, members crossing path borders between two calls of each kind (rows, search mode, a NaN sigma, epochs[k] = 0),
the stage-ahead refusal naming G, every refusal the header lists, state rewritten between ensemble calls, destroy / create
over a permuted subset / two overlapping ensembles, G's pending sigmaMap meeting create, and an accumulated epoch open on A
when it joins.  Every output equals the oracle's (one callseq.Model per member, the single call on every member in index
order) and the return of a twin of each member that never joins and makes the single calls one by one; every refusal names
the member the header says and is followed by a comparison of the whole state, lastBMU and MSE word of every member; where
the header gives a member another answer than its twin (vsom_train_online_chunk_masked, vsom_batch_accum_begin) the member
must refuse.  callseq.ens_conditions asserts from the walk's counts that it did not pass vacuously.

Cost of an ensemble walk, measured the same way (against the CPU fake; the model's share is about half), seeds 1 and 2, in
seconds: ens_shared 6.2, 7.2; ens_own 7.5, 7.0.  On an MI355X the tests themselves took 1.7 to 2.2 s (ens_shared) and
2.8 to 4.3 s (ens_own).  The dearest ops are the model's masked calls (tests/masked_train_ref.py and
tests/online_masked_ref.py, pure Python): they name A, A2, B and D only, the masked online chunk takes the local walk
(sigma <= 1) on more than 40 rows and D's 512 columns on 3 rows, and E's 1100 and G's 300 rows are loaded once per walk.

The ensemble query walks (callseq.generate_ensemble_query) add the four calls that return through state shared with the rest
of the ensemble: vsom_ensemble_bmu_masked_batch, vsom_ensemble_similarity_masked_batch, vsom_ensemble_bmu_topk_batch and
vsom_ensemble_bmu_topk_masked_batch (with vsom_ensemble_topk_applies).  They take the descriptor slot the masked training
calls use for their tables and grow its validity image in place; all four return through one grow-only pinned pair whose
word layout depends on the call, on each member's k and on who asked for fill / delta; they join the covered members' streams
only, so a query right behind vsom_ensemble_upload_chunks(wait = 0) or a member's own asynchronous epoch is ordered by that
join alone; a skipped member must be untouched and must not make the call refuse; and they promise to leave lastBMU, sqres
and the state alone while reading the live bmuHits, map and sigmaMap.  Two members join the ensemble profile's
(callseq.ENSQ_MEMBERS): Q, 10 x 10 x 9 with chunks of 1, 63, 64, 65, 128 and 129 rows -- the many-member kernels take one
workgroup per (member, 64 rows) --, and D2, 4 x 2 x 513, whose N * D = 4104 is the first size beyond the fast path's 4096,
beside D's 4096.  ensq_shared puts A, A2, B, C, D, D2, Q, E on one stream, ensq_own gives A, B, C, D, D2, Q, F, G a stream
each.  Around callseq.ENSQ_DRAWS random draws (the four queries and single-context queries on members mixed into the
ensemble profile's draws) a walk holds the runs of generate_ensemble_query's docstring: the no-wait run (six images of
different sizes through the two slots, training tables and query images in turn, then bmu_topk at once behind a second,
larger wait = 0 upload; sent to the ensemble back to back -- the pinned rows are overwritten with NaN only once a call that
covers every member has returned), result buffers that shrink and change layout, the read-only promise and the live state
(a written lastBMU must survive four queries and feed batch_epoch(is_first = 0); bmuHits all zero make rows with count < k),
path borders between two calls of each kind, the stage-ahead (covered: refused naming G; skipped: accepted), every refusal
the header lists, two ensembles over overlapping subsets in different orders with a member of B = 0, and G's sigmaMap behind
a lazy epoch, create and an ensemble epoch.  Before every top-k call the walk asks vsom_ensemble_topk_applies for every
covered member, and with an index past the end, and fails where the library and callseq.topk_fast disagree.  The calls go to
the C ABI with every output array of every member -- covered, skipped, asked for or not -- filled with a canary and followed
by a guard: what the call was given for a covered member must be overwritten, everything else, every array of a refused call
and every guard must stay.  Every output is held twice: on the words (NaN payloads included) to the member's twin, which makes
the single call over [0, B) from pageable memory, every row; and to the model, which computes it from the member's oracle
state
with tests/masked_score_ref.py and tests/topk_masked_ref.py, on the words as well wherever the header defines the word
(the units, 0x7FC00000 for a NaN distance and for a short list's padding, the counts); NaN equals NaN only in dmax, first,
amax, delta and fill, where a NaN was computed from a NaN in the map or sigmaMap and carries the host's payload -- every
row where B * N <= 32768, on E and G a seeded sample of 8 rows with row 0, the last row and the row
without a valid column.  callseq.ensq_conditions asserts that the walk was not vacuous and that on A, A2, B, D, D2 and Q the
model checked every covered row.  The single-context queries drawn on members (callseq.member_query) are held to the twin
on the words and to the model too: the lists and the similarity words bit for bit, blend within topk_masked_ref.blend_bound,
the BMD's norm and prob within the relative 1e-15 of tests/test_gpu_bmd_masked.py, the records within generate_ref.bound, a
draw exactly unless it lies within bmd_masked_ref.NEAR of a cumulative boundary.

Cost of an ensemble query walk, seeds 1 and 2, in seconds, against the CPU fake: ensq_shared 11.4, 10.2; ensq_own 15.2, 14.7;
the ensemble walks, measured beside them: ens_shared 7.5, 8.2; ens_own 10.8, 8.8.  On an MI355X the tests themselves took
5.4, 4.6 (ensq_shared) and 7.6, 8.0 (ensq_own), the ensemble walks beside them 2.2, 2.0 (ens_shared) and 4.3, 4.1
(ens_own): within twice the slowest of those, with little to spare on ensq_own.  The model's masked distance is pure Python
(about 12 us a distance, twice that with its call overhead) and is most of the cost: the runs load the members' shortest
chunks wherever a run is not about the row count, the calls of one block share their masks and, through a cache keyed by the
bytes of the map, the rows and the mask, their distances, and a walk makes 6 random draws."""
import pytest

import callseq as cs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("cfg", list(cs.CONFIGS))
def test_call_sequence_walk_matches_oracle(cfg, seed):
    stats = cs.run_walk(cs.generate(cfg, seed), cs.GpuBackend)
    assert stats["ops"] >= 30


DEFERRING = ("std48", "med48", "std80")


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("mode", ["lazy", "auto"])
@pytest.mark.parametrize("cfg", list(cs.CONFIGS))
def test_sigma_walk_matches_oracle(cfg, mode, seed):
    if cfg == "std80":
        assert cs.two_quad_launch(cs.CONFIGS[cfg]) == (700, True)
    stats = cs.run_walk(cs.generate(cfg, seed, profile="sigma", mode=mode), cs.GpuBackend)
    assert stats["ops"] >= 40
    deferred, dropped, materialised, _ = stats["sigma"]
    if cfg in DEFERRING:
        # (tests/test_call_sequences_model.py, test_gpu_seeds_defer_drop_and_materialise: these walks do)
        assert deferred >= 1 and dropped >= 1 and materialised >= 1, stats
    else:
        assert (deferred, dropped, materialised) == (0, 0, 0), stats     # "always eager"


ACCEPTING = ("std48", "med48", "std12", "std80")


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("mode", ["lazy", "auto"])
@pytest.mark.parametrize("cfg", list(cs.CONFIGS))
def test_accum_walk_matches_oracle(cfg, mode, seed):
    ops = cs.generate(cfg, seed, n_ops=cs.ACCUM_DRAWS, profile="accum", mode=mode)
    # (run_walk itself fails a walk in which a call of runs 1-4 or 6-9 is refused where the header accepts it, or accepted
    # where the header refuses it)
    stats = cs.run_walk(ops, cs.GpuBackend)
    assert stats["ops"] >= 50
    a = stats["accum"]
    if cfg in ACCEPTING:
        # (tests/test_call_sequences_model.py, test_gpu_accum_walks_meet_their_conditions: these walks do)
        assert a["chunks"] >= 8 and a["masked"] >= 3 and a["ends"] >= 2 and a["aborts"] >= 1, stats
        # run 5: the chunk call behind a chunk staged ahead was refused (run_walk fails the walk where it is not)
        assert a["staged"] >= (1 if cs.stages_ahead(cs.CONFIGS[cfg]) else 0), stats
    else:
        assert not any(a.values()), stats            # vsom_batch_accum_begin is refused, and so every call behind it
    if cfg not in DEFERRING:
        assert stats["sigma"][:3] == (0, 0, 0), stats


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("cfg", list(cs.ENS_CONFIGS))
def test_ensemble_walk_matches_oracle(cfg, seed):
    # (run_ensemble_walk itself fails a walk in which an ensemble call is refused where the header accepts it, accepted
    # where it refuses it, names another member, or where a restated path predicate disagrees with the library's)
    stats = cs.run_ensemble_walk(cs.generate_ensemble(cfg, seed), cs.EnsGpuBackend)
    # (tests/test_call_sequences_model.py, test_faithful_fake_passes_ensemble_walks: these walks meet them)
    cs.ens_conditions(cfg, stats, gpu=True)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("cfg_name", list(cs.ENSQ_CONFIGS))
def test_ensemble_query_walk_matches_oracle(cfg_name, seed):
    stats = cs.run_ensemble_walk(cs.generate_ensemble_query(cfg_name, seed), cs.EnsGpuBackend)
    cs.ensq_conditions(cfg_name, stats, gpu=True)
