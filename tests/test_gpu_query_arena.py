"""GPU: the chunk and distance queries share one scratch arena per context (vsom_layout, csrc/vsom_buf.hpp), so a query could
read what the previous query's layout left there, or keep a pointer across a regrowth.  One context runs the queries one
after another, and every result is held bit for bit to the same call on a fresh context (same state, same chunk) that has
run nothing else.

Shapes: maps 9 x 7 (63 nodes: one node tile, partially filled) and 20 x 20 (400 nodes: seven node tiles, several node
groups); J = 37 (a K-chunk remainder, a 4-remainder and a scalar tail); B = 150 (three row tiles, the last one ragged);
Standard, and one CLR context (J = 8, 20 x 20) for the queries that accept CLR.

Orders: ORDER is large layouts first (the restricted BMD with probabilities), then smaller ones, the largest top-k, and
small ones again.  ASCENDING starts with the smallest layouts, so that on the 20 x 20 Standard map the arena regrows before
almost every call: 10 pairs and one row of distances (4 KiB), evaluate (~9 KiB), the masked evaluate (~29 KiB: the masked
search's pieces and ~15 KiB of validity bytes, raw and packed), similarity with its dense report (~33 KiB), the masked
search with imputation (48 KiB), top-k with k = 5 (~51 KiB), the masked top-k with k = 5 (~66 KiB), generate (~568 KiB: the
BMD's 152 x 400 doubles, logits and records), top-k with k = 64 (~640 KiB), the masked top-k with k = 64 and blend
(~697 KiB), the masked generate with 3 draws (~763 KiB), the BMD with probabilities (~950 KiB) and the masked BMD with
probabilities (~965 KiB).  The figures are the sums of the pieces each call adds to its vsom_layout (the lay.add lines of
csrc/vsom_topk.hip, vsom_bmd.hip, vsom_generate.hip, vsom_evaluate.hip, vsom_masked.hip) at N = 400, J = 37, B = 150 in one
slice: seven node groups, a BMD pitch of 152 rows in two node chunks, validity bytes raw (150 x 37) and packed (150 x 64).

The queries added since the arena -- the masked top-k with and without blend, the masked BMD, generate and its masked form
with several draws, the masked evaluate -- are steps like the others; the masked ones refuse CLR and are left out there.

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
    # (drawn behind the older arrays, which keep their values: uniforms and logits of generate and of 3 masked draws)
    d.update(u3=rng.random((B, 3)), l=0.05 + 0.9 * rng.random((B, min(J, D))), l3=0.05 + 0.9 * rng.random((B, 3, J)))
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
    "topk_masked5": lambda c, d: c.bmu_topk_masked(5, d["valid"], min_hits=2),
    "topk_masked_max_blend": lambda c, d: c.bmu_topk_masked(min(64, c.n_nodes), d["mask"], min_hits=2, blend=True),
    "bmd_masked_probs": lambda c, d: c.restricted_bmd_masked(d["valid"], 2, u=d["u"], probs=True),
    "generate": lambda c, d: c.generate(2, d["u"], d["l"]),
    "generate_masked3": lambda c, d: c.generate_masked(d["valid"], 2, d["u3"], d["l3"], draws=3),
    "evaluate_masked": lambda c, d: c.evaluate_masked(d["valid"], d["binary"], d["continuous"], min_hits=2),
}
ORDER = tuple(STEPS)
ASCENDING = ("distances", "distances_row", "evaluate", "evaluate_masked", "similarity_delta", "masked_fill", "topk5",
             "topk_masked5", "generate", "topk_max", "topk_masked_max_blend", "generate_masked3", "bmd_probs",
             "bmd_masked_probs", "masked_one", "bmd_range", "similarity")
# the steps that refuse a CLR context: the masked search and every query built on the masked distance
NO_CLR = ("masked_fill", "masked_one", "topk_masked5", "topk_masked_max_blend", "bmd_masked_probs", "generate_masked3",
          "evaluate_masked")


def steps_of(case, order):
    return [s for s in order if not (case[0] == po.CLR and s in NO_CLR)]


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
