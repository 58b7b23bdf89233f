"""GPU: seeded random walks over the single-context C ABI (tests/callseq.py) against the CPU oracle.

Asynchronous ingest is correct only if every entry point keeps the context's staging flags right, along every call order
a C caller can make -- not only the orders other tests script.  Each walk mixes uploads, prefetches from pinned and
pageable memory, chunks handed over in HBM, commits, whole and split batch epochs, online chunks with and without a
wait, single steps, searches, distance queries, lastBMU / state reads and writes and search-mode switches; it holds by
construction the runs in which nothing synchronises between an asynchronous epoch and a prefetch's staging.  Every
accepted call returns the oracle's values bit for bit; a call that reads the staged rows while a chunk is pending may be
refused (naming the commit).  A failure prints the seed and the ops; callseq.replay(ops) reruns them."""
import pytest

import callseq as cs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("cfg", list(cs.CONFIGS))
def test_call_sequence_walk_matches_oracle(cfg, seed):
    stats = cs.run_walk(cs.generate(cfg, seed), cs.GpuBackend)
    assert stats["ops"] >= 30
