"""GPU: the chunk and distance queries share one scratch arena per context (vsom_layout, csrc/vsom_buf.hpp), so a query could
read what the previous query's layout left there, or keep a pointer across a regrowth.  One context runs the queries one
after another, and every result is held bit for bit to the same call on a fresh context (same state, same chunk) that has
run nothing else.

Shapes: maps 9 x 7 (63 nodes: one node tile, partially filled) and 20 x 20 (400 nodes: seven node tiles, several node
groups); J = 37 (a K-chunk remainder, a 4-remainder and a scalar tail); B = 150 (three row tiles, the last one ragged);
Standard, and one CLR context (J = 8, 20 x 20) for the queries that accept CLR.

Orders: ORDER is large layouts first (the restricted BMD with probabilities), then smaller ones, the largest top-k, and
small ones again.  ASCENDING starts with the smallest layouts, so that on the 20 x 20 Standard map the arena regrows before
almost every call: 10 pairs and one row of distances (4 KiB), evaluate (~9 KiB), similarity with its dense report
(~33 KiB), the masked search with imputation (48 KiB), top-k with k = 5 (~51 KiB) and k = 64 (~640 KiB), the BMD with
probabilities (~1 MiB).

vsom_bmu_topk_batch refuses a row range beyond the staged chunk before it allocates anything, and a slice's layout is
bounded by the slice budget whatever the range, so no argument makes the arena's allocation fail on a context that holds
its chunk: there is no out-of-memory case here (the arena's failure path is covered on the host, test_buffer_sets.py)."""
import functools
import os
import sys

import numpy as np
import pytest

import vsom_amd
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen  # noqa: E402

pytestmark = pytest.mark.gpu
B = 150
CASES = [(po.STANDARD, 9, 7, 37), (po.STANDARD, 20, 20, 37), (po.CLR, 20, 20, 8)]
IDS = ["std-9x7", "std-20x20", "clr-20x20"]


@functools.lru_cache(maxsize=None)
def inputs(tr, W, H, J):
    """state, chunk and call arguments of a case; made once, read-only"""
    N = W * H
    D = J * (J - 1) if tr == po.CLR else J
    rng = np.random.default_rng(1000 * N + J)
    d = {"map": rng.uniform(0.02, 0.98, (N, D)).astype(np.float32),
         "sigma": rng.uniform(0.01, 0.3, (N, D)).astype(np.float32),
         "hits": rng.integers(0, 6, N).astype(np.uint64),                 # (some nodes below min_hits = 2)
         "X": rng.uniform(0.05, 1.0, (B, J)).astype(np.float32),
         "u": rng.random(B),
         "valid": (rng.random((B, J)) < 0.8).astype(np.uint8),
         "mask": (rng.random(J) < 0.7).astype(np.uint8),
         "binary": (rng.random(J) < 0.5).astype(np.float32),
         "continuous": (rng.random(J) < 0.85).astype(np.float32),
         "nodes": rng.integers(0, N, 10).astype(np.uint64),
         "rows": rng.integers(0, B, 10).astype(np.uint64)}
    d["hits"][:3] = (5, 0, 2)
    d["valid"][:, 0] = 1                                                  # (every row keeps a valid column)
    d["mask"][0] = 1
    for a in d.values():
        a.setflags(write=False)
    return d


def context(case):
    tr, W, H, J = case
    d = inputs(*case)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=d["map"], sigma=d["sigma"], hits=d["hits"])
    ctx.upload_chunk(d["X"])
    return ctx


STEPS = {
    "bmd_probs": lambda c, d: c.restricted_bmd(2, u=d["u"], probs=True),
    "topk5": lambda c, d: c.bmu_topk(5),
    "masked_fill": lambda c, d: c.bmu_masked(d["valid"], min_hits=2, fill=True),
    "similarity_delta": lambda c, d: c.similarity(2, 3, valid=d["valid"], delta=True),
    "evaluate": lambda c, d: c.evaluate(d["binary"], d["continuous"], valid=d["valid"]),
    "distances": lambda c, d: c.distances(d["nodes"], d["rows"]),
    "distances_row": lambda c, d: c.distances_row(11),
    "topk_max": lambda c, d: c.bmu_topk(min(64, c.n_nodes)),
    "masked_one": lambda c, d: c.bmu_masked(d["mask"]),
    "bmd_range": lambda c, d: c.restricted_bmd(2, r0=7, r1=23),
    "similarity": lambda c, d: c.similarity(0, 3),
}
ORDER = tuple(STEPS)
ASCENDING = ("distances", "distances_row", "evaluate", "similarity_delta", "masked_fill", "topk5", "topk_max", "bmd_probs",
             "masked_one", "bmd_range", "similarity")


def steps_of(case, order):
    return [s for s in order if not (case[0] == po.CLR and s.startswith("masked"))]   # (the masked search refuses CLR)


def flat(res):
    """the arrays of a result, in a fixed order"""
    if isinstance(res, dict):
        res = [res[k] for k in sorted(res)]
    elif not isinstance(res, (tuple, list)):
        res = [res]
    return [np.ascontiguousarray(np.float64(a) if isinstance(a, float) else a) for a in res if a is not None]


def same_bits(a, b, what):
    fa, fb = flat(a), flat(b)
    assert len(fa) == len(fb), what
    for x, y in zip(fa, fb):
        assert x.dtype == y.dtype and x.shape == y.shape, what
        assert np.array_equal(x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8)), what


@functools.lru_cache(maxsize=None)
def fresh(case):
    """every step on a context of its own that runs nothing else; computed once per case, shared by the tests"""
    out = {}
    for s in steps_of(case, ORDER):
        ctx = context(case)
        out[s] = STEPS[s](ctx, inputs(*case))
        ctx.close()
    return out


def run_order(case, order, monkeypatch=None, masked_slice=None):
    ref = fresh(case)
    ctx = context(case)
    for i, s in enumerate(steps_of(case, order)):
        if masked_slice and s.startswith("masked"):
            monkeypatch.setenv("VSOM_MASKED_SLICE_ROWS", str(masked_slice))
        got = STEPS[s](ctx, inputs(*case))
        if monkeypatch:
            monkeypatch.delenv("VSOM_MASKED_SLICE_ROWS", raising=False)
        same_bits(got, ref[s], "step %d (%s)" % (i + 1, s))
    ctx.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_context_gives_the_fresh_contexts_bits(case):
    run_order(case, ORDER)


def test_the_arena_regrows_between_calls():
    run_order(CASES[1], ASCENDING)


@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_masked_slice_boundaries_inside_the_chunk(case, monkeypatch):
    """64-row slices of the masked search (three slices, the last one ragged) between the other queries' layouts"""
    run_order(case, ORDER, monkeypatch, masked_slice=64)
