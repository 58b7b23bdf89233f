"""GPU: every instantiation of the one-launch online chunk of tiny maps (csrc/vsom_online_tiny.hip) -- kind {Standard,
Median} x search {sigma 3.0: global, sigma 1.0: the local walk} x values per thread {1, 2, 4}, each as flavour {plain, over
valid entries} x form {the context's own launch, one workgroup per map in an ensemble call}.  The other online tests thin
this grid out by alternating kind and decay over their shapes; here every one of the 48 kernels runs once.

Shapes (W, H, J), the smallest that select each count of values per thread: (4, 3, 2) one; (12, 9, 12) N D = 1296, two;
(12, 9, 20) N D = 2160, four, with a packet tail of 4.  B = 3: both key parities, and the last sample's post step behind
the loop.  The decays alternate over the cases.  Masked cases: a fixed-seed mask with about 70 % valid entries and NaN at
the invalid positions of the rows.

Yardsticks, never the library's own per-sample loop: the C oracle (oracle/pyoracle.py) for the plain chunk,
tests/online_masked_ref.py for the masked one; each reference is computed once and shared by the two forms.  Compared on
the bits: map, SMap, sigmaMap, weightMap, bmuHits, lastBMU, MSE.  Every case asserts the path it meant to take:
vsom_online_masked_tiny_applies holds (its conditions are the plain chunk's with a larger LDS need), and the image-bounded
search of the per-sample loop has seen no sample afterwards."""
import functools
import os
import sys

import numpy as np
import pytest

import vsom_amd
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_masked_cases as oc  # noqa: E402
from online_masked_cases import ETA, same  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
B = 3
SHAPES = ((4, 3, 2), (12, 9, 12), (12, 9, 20))
# in the order of the kernels' groups: (Median ? 6 : 0) + (local ? 3 : 0) + (0, 1, 2 for 1, 2, 4 values per thread)
GRID = [(tr, sigma, shape) for tr in oc.KINDS for sigma in (3.0, 1.0) for shape in SHAPES]
PLAIN_AMONG_MASKED = (3, 8)          # the two plain members of the masked ensemble call


def decay(ci, masked):
    return oc.DECAYS[(ci + int(masked)) % 2]


@functools.lru_cache(maxsize=None)
def case(ci, masked):
    """the rows as uploaded, the validity (None: plain), map, SMap, the starting lastBMU, and the reference's snapshot"""
    tr, sigma, (W, H, J) = GRID[ci]
    X, M, valid, S, start = oc.data(W, H, J, B, seed=100 + ci)
    fn = decay(ci, masked)
    lb = oc.start_of(sigma, start, B)
    if masked:
        rows = np.where(valid, X, f32(np.nan)).astype(f32)
        r = oc.ref_new(tr, W, H, J, M, S)
        mse = r.train_chunk(rows, valid, lb, ETA, sigma, fn)
        want = r.snapshot(lb, mse)
    else:
        rows, valid = X, None
        want = oc.oracle_chunk(tr, W, H, J, M, S, X, lb, ETA, sigma, fn)
    return rows, valid, M, S, start, want


def loaded_context(ci, masked):
    tr, sigma, (W, H, J) = GRID[ci]
    rows, valid, M, S, start, _ = case(ci, masked)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=M, S=S)
    ctx.upload_chunk(np.ascontiguousarray(rows, dtype=f32))
    if sigma <= 1:
        ctx.set_last_bmu(start)
    assert ctx.online_masked_tiny_applies(sigma)
    return ctx


def check(ctx, mse, lb, ci, masked, what):
    st = ctx.get_state()
    got = {"map": st["map"], "S": st["S"], "sigma": st["sigma"], "weight": st["weight"], "hits": st["hits"],
           "lastbmu": np.array(lb, np.uint64), "mse": np.array([mse], f32)}
    same(got, case(ci, masked)[5], (what, ci, GRID[ci]))
    assert (ctx.get_last_bmu() == got["lastbmu"]).all()
    assert ctx.online_search_stats()["samples"] == 0


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("ci", range(len(GRID)))
def test_single_context(ci, masked):
    sigma = GRID[ci][1]
    ctx = loaded_context(ci, masked)
    if masked:
        mse, lb = ctx.train_online_chunk_masked(ETA, sigma, decay(ci, True), case(ci, True)[1])
    else:
        mse, lb = ctx.train_online_chunk_fetch(ETA, sigma, decay(ci, False))
    check(ctx, mse, lb, ci, masked, "single")
    ctx.close()


def ensemble_call(flavours):
    """one call over twelve members, one per kernel group; flavours[ci]: member ci is masked"""
    n = len(GRID)
    members = [loaded_context(ci, flavours[ci]) for ci in range(n)]
    ens = vsom_amd.Ensemble(members)
    sigmas = [g[1] for g in GRID]
    fns = [decay(ci, flavours[ci]) for ci in range(n)]
    if any(flavours):
        valids = [case(ci, True)[1] if flavours[ci] else None for ci in range(n)]
        mse, lbs = ens.train_online_chunk_masked(ETA, sigmas, fns, valids)
    else:
        mse, lbs = ens.train_online_chunk_fetch(ETA, sigmas, fns)
    for ci, ctx in enumerate(members):
        check(ctx, mse[ci], lbs[ci], ci, flavours[ci], "ensemble")
    ens.close()
    for ctx in members:
        ctx.close()


def test_ensemble_of_plain_members():
    ensemble_call([False] * len(GRID))


def test_ensemble_of_masked_members_with_two_plain_ones():
    ensemble_call([ci not in PLAIN_AMONG_MASKED for ci in range(len(GRID))])
