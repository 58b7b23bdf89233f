"""GPU: every consumer of the 64 x 64 distance tile -- the exact search (bmu_tile_kernel, vsom_bmu.hip) and the callers of
vsom_dist_tile (vsom_dist_tile.hpp: top-k, the masked search, the restricted BMD) -- walked through the tile's length
cases on one shape: a 7 x 10 map (70 nodes: a full node tile and a ragged one) and 70 rows (a ragged second row tile; for
CLR two tiles of 32 and a ragged one).

Comparer lengths L.  Standard: 1, 3, 4, 5, 7, 8, 11, 12, 15, 32, 33, 36, 39, 40, 64, 69, 100 -- every L % 8 with and
without whole 8-blocks, the `rem >= 4` branch on both sides, 1 to 4 K-chunks of 32.  CLR compares P = J (J - 1) / 2 pairs, so
J = 2, 3, 4, 5, 6, 7, 9, 16 gives P = 1, 3, 6, 10, 15, 21, 36, 120: one per residue class of P % 8.

Distances, indices and masked results are held bit for bit (NaN equal to NaN) to the oracle, with the helpers of
test_gpu_topk.py and test_gpu_masked.py.  The BMD rows go through test_gpu_bmd_batch.py's check_rows: the distance inside
p = exp(-d * d / 2) is the tile's, but the device's double-precision exp and libm's each round within an ulp of the true
value and need not agree in the last bit, so prob and norm are held to the oracle within that file's RTOL = 1e-15 (a few
ulps of a double, the sum of N such terms included), the NaN pattern (0 / 0 where a row has no mass) exactly."""
import functools
import os
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen  # noqa: E402
from test_gpu_bmd_batch import check_rows  # noqa: E402
from test_gpu_masked import bits_eq, checker  # noqa: E402
from test_gpu_topk import beq, expected, oracle_dists  # noqa: E402

pytestmark = pytest.mark.gpu
W, H, B = 7, 10, 70
N = W * H
STD_L = (1, 3, 4, 5, 7, 8, 11, 12, 15, 32, 33, 36, 39, 40, 64, 69, 100)
CLR_J = (2, 3, 4, 5, 6, 7, 9, 16)
CASES = [(po.STANDARD, L) for L in STD_L] + [(po.CLR, J) for J in CLR_J]
IDS = ["std-L%d" % L for L in STD_L] + ["clr-J%d-P%d" % (J, J * (J - 1) // 2) for J in CLR_J]


@functools.lru_cache(maxsize=None)
def reference(tr, J):
    """rows, map and the oracle's distance of every (row, node) pair; computed once per case, read-only"""
    X = gen.blobs(B, J, 4, 3, 2)
    if tr == po.CLR:
        X = (np.abs(X) + np.float32(0.5)).astype(np.float32)
    o = po.OracleSom(W, H, J, tr)
    M = gen.random_map(N, o.depth, seed=13)
    o.set_state(map=M)
    D = oracle_dists(o, X)
    for a in (X, M, D):
        a.setflags(write=False)
    return X, M, D, o


def context(tr, J):
    X, M, D, o = reference(tr, J)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=M)
    ctx.upload_chunk(X)
    return ctx, X, M, D, o


def test_the_cases_cover_the_lengths():
    assert [po.length(po.STANDARD, L) for L in STD_L] == list(STD_L)
    P = [po.length(po.CLR, J) // 2 for J in CLR_J]
    assert P == [J * (J - 1) // 2 for J in CLR_J] and sorted(p % 8 for p in P) == list(range(8))
    assert {L % 8 for L in STD_L if L < 8} | {0} == {L % 8 for L in STD_L if L >= 8}      # each residue, with and without blocks
    assert {(L + 31) // 32 for L in STD_L} == {1, 2, 3, 4}


@pytest.mark.parametrize("tr, J", CASES, ids=IDS)
def test_topk_and_exact_search(tr, J):
    ctx, X, M, D, o = context(tr, J)
    k = min(64, N)
    idx, dist = ctx.bmu_topk(k)
    ei, ed = expected(D, k)
    assert (idx == ei).all(), np.argwhere(idx != ei)[:4]
    assert beq(dist, ed)
    ctx.set_bmu_mode(capi.BMU_EXACT)
    bi, bd = ctx.bmu_batch()
    assert (bi == ei[:, 0]).all(), np.flatnonzero(bi != ei[:, 0])[:4]
    assert beq(bd, ed[:, 0])
    ctx.close()


@pytest.mark.parametrize("L", STD_L)
def test_masked_all_valid(L):
    ctx, X, M, D, o = context(po.STANDARD, L)
    ei, ed = expected(D, 1)
    for valid in (np.ones((B, L), np.uint8), np.ones(L, np.uint8)):    # a mask per row, one_mask
        got = ctx.bmu_masked(valid)
        assert (got["bmu"] == ei[:, 0]).all(), (valid.ndim, np.flatnonzero(got["bmu"] != ei[:, 0])[:4])
        assert beq(got["dist"], ed[:, 0]), valid.ndim
    ctx.close()


@pytest.mark.parametrize("L", STD_L)
def test_masked_random_mask(L):
    ctx, X, M, D, o = context(po.STANDARD, L)
    hits = np.zeros(N, np.uint64)
    valid = np.random.default_rng(200 + L).random((B, L)) < 0.7
    for v in (valid, valid[0].copy()):                                  # a mask per row, row 0's pattern as one_mask
        got = ctx.bmu_masked(v)
        eb, ed = checker(po.STANDARD, X, M, v, hits, 0)
        assert (got["bmu"] == eb).all(), (v.ndim, np.flatnonzero(got["bmu"] != eb)[:4])
        assert bits_eq(got["dist"], ed), (v.ndim, np.flatnonzero(got["dist"].view(np.uint32) != ed.view(np.uint32))[:4])
    ctx.close()


@pytest.mark.parametrize("tr, J", CASES, ids=IDS)
def test_bmd(tr, J):
    ctx, X, M, D, o = context(tr, J)
    res = ctx.restricted_bmd(0, probs=True)
    check_rows(ctx, o, X, 0, range(8), res, "tile consumers/%d/%d" % (tr, J))
    ctx.close()
