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
and less often still for med48 and std80 (callseq.CONFIGS, "sigma_weights" / "weights")."""
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
