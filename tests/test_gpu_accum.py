"""GPU: vsom_batch_accum_begin / _chunk / _end / _abort -- one batch epoch over a data set that loads in several chunks.
Every comparison is on the bits (NaN equals NaN).  The reference is the CPU oracle's batch_epoch on the CONCATENATED rows
(with the concatenated lastBMU), and, for the shape on the large route, vsom_batch_epoch of a second context that holds
all rows as one chunk.

Shapes: 7x5x9 with 70 rows (splits that cross the 64-row edge, the chains' groups of 8 and the neighbourhood pass's groups
of 16; empty chunks; seventy chunks of one row), 12x11x33 with 257 rows (132 nodes: a partly filled third wavefront of the
neighbourhood pass and second node group of the chains; 33 columns: a ragged fifth column block of 8), 5x4x1, 9x7 (W != H),
48x48x196 with 2 x 1100 rows (shortlist search, lane = node chains in vsom_batch_epoch)."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from vsom_amd import som as vs
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_hooks as hooks  # noqa: E402
import gen  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")
KINDS = (po.STANDARD, po.MEDIAN)
# first epoch, then two local epochs, sigma 3 -> 2.2
SCHEDULE = tuple((3.0 * math.exp(-0.155 * e), e == 0) for e in range(3))
FIELDS = ("map", "sigma", "weight", "hits", "S", "lastbmu", "sqres", "mse")


def beq(a, b):
    """bitwise equality; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def rows_and_map(W, H, J, B, seed=3):
    return gen.blobs(B, J, 4, seed, 2), gen.random_map(W * H, J, seed=seed + 10)


def snapshot(ctx, mse, lastbmu=None, sqres=None):
    st = ctx.get_state()
    return {"map": st["map"], "sigma": st["sigma"], "S": st["S"], "weight": st["weight"], "hits": st["hits"],
            "lastbmu": ctx.get_last_bmu() if lastbmu is None else lastbmu,
            "sqres": ctx.get_sqres() if sqres is None else sqres, "mse": np.array([mse], np.float32)}


def same_runs(a, b, what, keys=FIELDS):
    assert len(a) == len(b)
    for e, (sa, sb) in enumerate(zip(a, b)):
        for k in keys:
            assert beq(sa[k], sb[k]), (what, "epoch", e, k)


def accum_epoch(ctx, X, splits, lb_in, sigma, first, finish="end"):
    """begin, one chunk call per split (lastBMU set from lb_in: a load zeroes it), end; lastBMU and sqres are fetched after
    every chunk and concatenated"""
    assert sum(splits) == X.shape[0]
    ctx.batch_accum_begin(sigma, first, X.shape[0])
    lbs, sqs, off = [np.zeros(0, np.uint64)], [np.zeros(0, np.float32)], 0
    for B in splits:
        ctx.upload_chunk(X[off:off + B])
        ctx.set_last_bmu(lb_in[off:off + B])
        ctx.batch_accum_chunk()
        lbs.append(ctx.get_last_bmu())
        sqs.append(ctx.get_sqres())
        off += B
    if finish == "abort":
        ctx.batch_accum_abort()
        mse = ctx.get_mse()
    else:
        mse = ctx.batch_accum_end()
        assert beq(np.float32(ctx.get_mse()), np.float32(mse))
    return snapshot(ctx, mse, np.concatenate(lbs), np.concatenate(sqs))


def run_accum(tr, W, H, J, init, X, splits, schedule=SCHEDULE, S=None):
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init, S=S)
    ptrs = [ctx.device_ptr(w) for w in (capi.BUF_MAP, capi.BUF_SIGMA, capi.BUF_WEIGHT, capi.BUF_S)]
    lb = np.zeros(X.shape[0], np.uint64)
    out = []
    for sigma, first in schedule:
        out.append(accum_epoch(ctx, X, splits, lb, sigma, first))
        lb = out[-1]["lastbmu"]
    assert ptrs == [ctx.device_ptr(w) for w in (capi.BUF_MAP, capi.BUF_SIGMA, capi.BUF_WEIGHT, capi.BUF_S)]
    ctx.close()
    return out


def run_plain(tr, W, H, J, init, X, schedule=SCHEDULE, S=None):
    """vsom_batch_epoch on all rows as one chunk (lastBMU stays on the device between the epochs)"""
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init, S=S)
    ctx.upload_chunk(X)
    out = [snapshot(ctx, ctx.batch_epoch(sigma, first)) for sigma, first in schedule]
    ctx.close()
    return out


def oracle_epoch(o, X, lb, sigma, first):
    """OracleSom.batch_epoch on the rows; sqres from its phase 1 (which changes no state); lb is updated in place"""
    lb2, sq = lb.copy(), np.zeros(X.shape[0], np.float32)
    o.batch_phase1_range(X, 0, X.shape[0], lb2, sq, first)
    mse = o.batch_epoch(X, lb, sigma, first)
    assert (lb2 == lb).all()
    return {"map": o.map.copy(), "sigma": o.sigma.copy(), "S": o.S.copy(), "weight": o.weight.copy(), "hits": o.hits.copy(),
            "lastbmu": lb.copy(), "sqres": sq, "mse": np.array([mse], np.float32)}


@functools.lru_cache(maxsize=None)
def reference(tr, W, H, J, B, schedule=SCHEDULE):
    """the oracle's snapshots on the concatenated rows (computed once per shape; callers do not modify them)"""
    X, init = rows_and_map(W, H, J, B)
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=init)
    lb = np.zeros(B, np.uint64)
    return [oracle_epoch(o, X, lb, sigma, first) for sigma, first in schedule]


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------
SPLITS = [
    (7, 5, 9, 70, (70,)), (7, 5, 9, 70, (1, 69)), (7, 5, 9, 70, (35, 35)), (7, 5, 9, 70, (63, 7)), (7, 5, 9, 70, (64, 6)),
    (7, 5, 9, 70, (0, 70, 0)), (7, 5, 9, 70, (1,) * 70),
    (12, 11, 33, 257, (128, 129)), (12, 11, 33, 257, (65, 64, 64, 64)), (12, 11, 33, 257, (255, 2)),
    (5, 4, 1, 70, (33, 37)),
    (9, 7, 9, 110, (70, 40)),
]


@pytest.mark.parametrize("tr", KINDS)
@pytest.mark.parametrize("W, H, J, B, splits", SPLITS)
def test_against_the_oracle(tr, W, H, J, B, splits):
    X, init = rows_and_map(W, H, J, B)
    got = run_accum(tr, W, H, J, init, X, splits)
    same_runs(got, reference(tr, W, H, J, B), splits)
    assert np.isfinite(got[-1]["map"]).all() and got[-1]["hits"].sum() == 3 * B
    assert not got[-1]["S"].any()                 # SMap is untouched in batch mode


# ---- 2. the split does not matter, whatever vsom_batch_epoch itself does ---------------------------------------------------
ENVS = [{}, {"VSOM_NO_TINY": "1"}, {"VSOM_NO_TINY": "1", "VSOM_NO_CHAIN": "1"}, {"VSOM_SIGMA_MODE": "eager"},
        {"VSOM_SIGMA_MODE": "lazy", "VSOM_NO_CHAIN": "1"}]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: "+".join(f"{k[5:]}={v}" for k, v in e.items()) or "default")
@pytest.mark.parametrize("tr, W, H, J, B", [(po.STANDARD, 7, 5, 9, 70), (po.MEDIAN, 7, 5, 9, 70), (po.STANDARD, 12, 11, 33, 257)])
def test_the_split_does_not_matter(monkeypatch, env, tr, W, H, J, B):
    for k, v in env.items():
        monkeypatch.setenv(k, v)         # (read when a context is created)
    X, init = rows_and_map(W, H, J, B)
    S = gen.random_map(W * H, J, seed=77)
    plain = run_plain(tr, W, H, J, init, X, S=S)
    for _, _, _, _, splits in [s for s in SPLITS if s[:4] == (W, H, J, B) and len(s[4]) < 70]:
        same_runs(run_accum(tr, W, H, J, init, X, splits, S=S), plain, (env, splits))
    assert beq(plain[-1]["S"], S)


# ---- 3. 0/0 chains stay NaN across the chunk border ------------------------------------------------------------------------
@pytest.mark.parametrize("tr", KINDS)
def test_sigma_one(tr):
    W, H, J, B = 7, 5, 9, 70
    X, init = rows_and_map(W, H, J, B)
    sched = ((1.0, True),)
    got = run_accum(tr, W, H, J, init, X, (35, 35), sched)
    same_runs(got, reference(tr, W, H, J, B, sched), "sigma 1")
    m = got[0]["map"]
    assert np.isnan(m).any() and np.isfinite(m).any()
    # the chain of a node is finite exactly where the first row of the whole epoch chose it
    assert (np.isfinite(m).all(axis=1) == (np.arange(W * H) == int(got[0]["lastbmu"][0]))).all()


@pytest.mark.parametrize("tr", KINDS)
def test_weight_zero_in_the_first_chunk_and_a_hit_in_the_second(tr):
    # sigma 1.05: (float)exp(-d^2 / 2 sigma^2) is 0 from a distance of 16 units on.  The first chunk's rows are the model
    # vectors of units in columns 0-1, the second chunk's those of columns 18-19: the units on the right have W = 0 (c = 0/0)
    # through the first chunk and a positive weightMap after the second
    W, H, J, sigma = 20, 3, 5, 1.05
    assert np.float32(math.exp(-(16.0 ** 2) / 2 / sigma / sigma)) == 0 and np.float32(math.exp(-(15.0 ** 2) / 2 / sigma / sigma)) > 0
    init = gen.random_map(W * H, J, seed=5)
    left = [y * W + x for y in range(H) for x in (0, 1)]
    right = [y * W + x for y in range(H) for x in (18, 19)]
    X = np.ascontiguousarray(np.concatenate([init[left], init[left], init[right]]), np.float32)
    splits = (2 * len(left), len(right))
    got = run_accum(tr, W, H, J, init, X, splits, ((sigma, True),))
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=init)
    want = [oracle_epoch(o, X, np.zeros(X.shape[0], np.uint64), sigma, True)]
    same_runs(got, want, "weight 0 then a hit")
    assert (got[0]["lastbmu"] == np.array(left + left + right, np.uint64)).all()
    far = np.array([y * W + x for y in range(H) for x in (17, 18, 19)])
    assert np.isnan(got[0]["map"][far]).all() and (got[0]["weight"][far] > 0).all()
    assert np.isfinite(got[0]["map"][left]).all()


# ---- 4. a map on the large route: shortlist search, against vsom_batch_epoch on one chunk ----------------------------------
def big_case():
    W = H = 48
    J = 196
    xs = [gen.mnist_like(1100, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    return W, H, J, xs, init


@functools.lru_cache(maxsize=None)
def big_reference():
    """vsom_batch_epoch (eager) on the 2200 rows as one chunk: first epoch and one local epoch"""
    W, H, J, xs, init = big_case()
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_sigma_mode(capi.SIGMA_EAGER)
    ctx.set_state(map=init)
    ctx.upload_chunk(np.concatenate(xs))
    assert not capi.lib().vsom_small_map_chains(ctx._h, W * H)
    out = [snapshot(ctx, ctx.batch_epoch(s, f)) for s, f in ((10.0, True), (8.0, False))]
    ctx.close()
    return out


@pytest.mark.parametrize("loader", ["upload", "prefetch"])
def test_large_route(loader):
    W, H, J, xs, init = big_case()
    want = big_reference()
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    assert not capi.lib().vsom_small_map_chains(ctx._h, W * H)
    pbs = []
    for x in xs:
        pbs.append(capi.PinnedBuffer(x.shape))
        pbs[-1].array[...] = x
    lb = np.zeros(2200, np.uint64)
    got = []
    for sigma, first in ((10.0, True), (8.0, False)):
        ctx.batch_accum_begin(sigma, first, 2200)
        lbs, sqs = [], []
        if loader == "upload":
            for k in range(2):
                ctx.upload_chunk(xs[k])
                ctx.set_last_bmu(lb[1100 * k:1100 * (k + 1)])
                ctx.batch_accum_chunk()
                lbs.append(ctx.get_last_bmu())
                sqs.append(ctx.get_sqres())
        else:                                         # the ingest pipeline: prefetch(k+1) -> accum_chunk(k) -> commit
            ctx.upload_chunk(xs[0])
            ctx.set_last_bmu(lb[:1100])
            ctx.prefetch_chunk(pbs[1].array)
            ctx.batch_accum_chunk()
            lbs.append(ctx.get_last_bmu())
            sqs.append(ctx.get_sqres())
            ctx.commit_chunk()
            ctx.set_last_bmu(lb[1100:])
            ctx.batch_accum_chunk()
            lbs.append(ctx.get_last_bmu())
            sqs.append(ctx.get_sqres())
        mse = ctx.batch_accum_end()
        got.append(snapshot(ctx, mse, np.concatenate(lbs), np.concatenate(sqs)))
        lb = got[-1]["lastbmu"]
        if first:
            st = ctx.shortlist_stats()
            assert st["searches"] >= 2 and st["samples"] == 1100, st     # the shortlist search ran on both chunks
    same_runs(got, want, loader)
    assert np.isfinite(got[-1]["map"]).all()
    ctx.close()
    for pb in pbs:
        pb.free()


# ---- 5. a pending sigmaMap is materialised by the first of the calls -------------------------------------------------------
@pytest.mark.parametrize("finish", ["abort", "end"])
def test_pending_sigma(finish):
    W, H, J, xs, init = big_case()
    runs = []
    for mode in (capi.SIGMA_LAZY, capi.SIGMA_EAGER):
        ctx = vsom_amd.Context(W, H, J)
        ctx.set_sigma_mode(mode)
        ctx.set_state(map=init)
        ctx.upload_chunk(xs[0])
        ctx.batch_epoch(10.0, True)
        stats = ctx.sigma_stats()
        assert stats["pending"] == (mode == capi.SIGMA_LAZY) and stats["materialised"] == 0
        snap = accum_epoch(ctx, xs[1], (1100,), np.zeros(1100, np.uint64), 8.0, True, finish)
        stats = ctx.sigma_stats()
        assert not stats["pending"] and stats["materialised"] == (1 if mode == capi.SIGMA_LAZY else 0), stats
        assert stats["deferred"] == (1 if mode == capi.SIGMA_LAZY else 0), stats     # the accumulated epoch never defers
        runs.append(snap)
        ctx.close()
    same_runs([runs[0]], [runs[1]], finish)
    first = big_reference_first_chunk()
    if finish == "abort":        # sigmaMap of the deferred epoch, as the eager epoch wrote it
        assert beq(runs[0]["sigma"], first["sigma"]) and beq(runs[0]["map"], first["map"])
    else:
        assert not beq(runs[0]["sigma"], first["sigma"])


@functools.lru_cache(maxsize=None)
def big_reference_first_chunk():
    W, H, J, xs, init = big_case()
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_sigma_mode(capi.SIGMA_EAGER)
    ctx.set_state(map=init)
    ctx.upload_chunk(xs[0])
    snap = snapshot(ctx, ctx.batch_epoch(10.0, True))
    ctx.close()
    return snap


# ---- 6. abort and refusals -------------------------------------------------------------------------------------------------
def oracle_follows(ctx, o, X, what):
    """a following vsom_batch_epoch matches the oracle"""
    lbo = np.zeros(X.shape[0], np.uint64)
    ctx.upload_chunk(X)
    assert np.float32(ctx.batch_epoch(1.5, True)) == np.float32(o.batch_epoch(X, lbo, 1.5, True)), what
    st = ctx.get_state()
    for k, ref in (("map", o.map), ("sigma", o.sigma), ("S", o.S), ("weight", o.weight)):
        assert beq(st[k], ref), (what, k)
    assert (ctx.get_last_bmu() == lbo).all(), what


@pytest.mark.parametrize("tr", KINDS)
def test_abort_leaves_the_model_state(tr):
    W, H, J, B = 7, 5, 9, 70
    X, init = rows_and_map(W, H, J, B)
    S = gen.random_map(W * H, J, seed=77)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init, S=S)
    ctx.upload_chunk(X)
    ctx.batch_epoch(3.0, True)                     # a state with sigmaMap and weightMap set
    before = ctx.get_state()
    snap = accum_epoch(ctx, X, (35, 35), np.zeros(B, np.uint64), 2.5, True, "abort")
    for k in ("map", "sigma", "weight", "S"):
        assert beq(snap[k], before[k]), k
    assert snap["hits"].sum() == before["hits"].sum() + B          # what the chunk calls did stays
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=before["map"], sigma=before["sigma"], S=before["S"], weight=before["weight"])
    oracle_follows(ctx, o, X, "after the abort")
    # and a new epoch can be opened
    lb = np.zeros(B, np.uint64)
    got = accum_epoch(ctx, X, (64, 6), lb, 2.0, True)
    want = oracle_epoch(o, X, lb, 2.0, True)
    same_runs([got], [want], "an epoch after the abort", keys=("map", "sigma", "weight", "S", "lastbmu", "sqres", "mse"))
    ctx.close()


def test_refusals_leave_the_state_alone():
    W, H, J, rows = 6, 5, 7, 20
    init = gen.random_map(W * H, J, seed=1)
    X = gen.blobs(rows, J, 3, 1, 2)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    L = capi.lib()
    h = ctx._h

    def refused(code, word):
        assert code == -1, word
        assert word in L.vsom_last_error().decode(), (word, L.vsom_last_error().decode())

    refused(L.vsom_batch_accum_begin(None, 2.0, 1, 20), "null context")
    refused(L.vsom_batch_accum_chunk(None), "null context")
    refused(L.vsom_batch_accum_end(None, None), "null context")
    refused(L.vsom_batch_accum_abort(None), "null context")
    for call in (lambda: L.vsom_batch_accum_chunk(h), lambda: L.vsom_batch_accum_end(h, None), lambda: L.vsom_batch_accum_abort(h)):
        refused(call(), "no accumulated epoch is open")
    for mode in (capi.UPDATE_FMA, capi.UPDATE_FMA_SIGMA):
        ctx.set_update_mode(mode)
        refused(L.vsom_batch_accum_begin(h, 2.0, 1, 20), "strict")
    ctx.set_update_mode(capi.UPDATE_STRICT)
    refused(L.vsom_batch_accum_chunk(h), "no accumulated epoch is open")      # the refused begins opened nothing

    assert L.vsom_batch_accum_begin(h, 2.0, 1, rows) == 0
    refused(L.vsom_batch_accum_begin(h, 2.0, 1, rows), "already open")
    refused(L.vsom_batch_accum_chunk(h), "no chunk loaded")
    ctx.upload_chunk(gen.blobs(rows + 1, J, 3, 1, 2))
    refused(L.vsom_batch_accum_chunk(h), "exceed total_rows")
    # one row short: end is refused and the epoch stays open; the missing row's chunk completes it
    ctx.upload_chunk(X[:rows - 1])
    assert L.vsom_batch_accum_chunk(h) == 0
    lb0, sq0 = ctx.get_last_bmu(), ctx.get_sqres()
    mse = ctypes.c_float()
    refused(L.vsom_batch_accum_end(h, ctypes.byref(mse)), "rows accumulated")
    st = ctx.get_state()
    assert beq(st["map"], init) and not st["sigma"].any() and not st["weight"].any()     # nothing written yet
    ctx.upload_chunk(X[rows - 1:])
    refused(L.vsom_batch_accum_begin(h, 2.0, 1, rows), "already open")
    assert L.vsom_batch_accum_chunk(h) == 0
    refused(L.vsom_batch_accum_chunk(h), "exceed total_rows")      # the same chunk once more
    lb1, sq1 = ctx.get_last_bmu(), ctx.get_sqres()
    assert L.vsom_batch_accum_end(h, ctypes.byref(mse)) == 0
    refused(L.vsom_batch_accum_end(h, None), "no accumulated epoch is open")
    o = po.OracleSom(W, H, J)
    o.set_state(map=init)
    want = oracle_epoch(o, X, np.zeros(rows, np.uint64), 2.0, True)
    got = snapshot(ctx, mse.value, np.concatenate([lb0, lb1]), np.concatenate([sq0, sq1]))
    same_runs([got], [want], "after the refusals")
    oracle_follows(ctx, o, X, "an epoch after the refusals")

    # an ensemble member, also after the ensemble is gone
    ens = capi.Ensemble([ctx])
    refused(L.vsom_batch_accum_begin(h, 2.0, 1, rows), "group or an ensemble")
    ens.close()
    refused(L.vsom_batch_accum_begin(h, 2.0, 1, rows), "group or an ensemble")
    ctx.close()

    # a group member
    grp = capi.Group(W, H, J, devices=[0, 0])
    member = grp.member(0)
    refused(L.vsom_batch_accum_begin(member._h, 2.0, 1, rows), "group or an ensemble")
    grp.close()

    # CLR contexts
    Xc = (np.abs(gen.blobs(rows, 5, 3, 1, 2)) + np.float32(0.5)).astype(np.float32)
    clr = vsom_amd.Context(4, 4, 5, po.CLR)
    oc = po.OracleSom(4, 4, 5, po.CLR)
    initc = gen.random_map(16, oc.depth, seed=2)
    clr.set_state(map=initc)
    oc.set_state(map=initc)
    with pytest.raises(capi.VsomError, match="CLR"):
        clr.batch_accum_begin(2.0, True, rows)
    with pytest.raises(capi.VsomError, match="no accumulated epoch is open"):
        clr.batch_accum_chunk()
    oracle_follows(clr, oc, Xc, "CLR after the refusal")
    clr.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_batch_accum_begin"):
        cu.batch_accum_begin(2.0, True, 10)
    cu.bmu_batch()
    cu.close()


def test_chunk_refuses_a_chunk_staged_ahead():
    W, H, J, xs, init = big_case()
    ctx = vsom_amd.Context(W, H, J)
    pb = capi.PinnedBuffer(xs[1].shape)
    pb.array[...] = xs[1]
    ctx.set_state(map=init)
    ctx.upload_chunk(xs[0])
    ctx.batch_accum_begin(10.0, True, 2200)
    ctx.batch_epoch_async(10.0, True)              # (rewrites the state: only to have the next chunk staged ahead)
    ctx.prefetch_chunk(pb.array)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        ctx.batch_accum_chunk()
    ctx.commit_chunk()
    ctx.batch_accum_chunk()                        # the context stays usable
    ctx.batch_accum_abort()
    ctx.close()
    pb.free()


# ---- 7. what follows an accumulated epoch sees its map ---------------------------------------------------------------------
@pytest.mark.parametrize("tr", KINDS)
def test_followers_see_the_new_map(tr):
    W, H, J, B = 12, 11, 33, 257
    X, init = rows_and_map(W, H, J, B)
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=init)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init)
    lb = np.zeros(B, np.uint64)
    got = accum_epoch(ctx, X, (128, 129), lb, 3.0, True)
    same_runs([got], [oracle_epoch(o, X, lb, 3.0, True)], "the epoch")
    Y = gen.blobs(40, J, 4, 9, 8)
    ctx.upload_chunk(Y)
    idx, dist = ctx.bmu_batch()
    lbo, sq = np.zeros(40, np.uint64), np.zeros(40, np.float32)
    o.batch_phase1_range(Y, 0, 40, lbo, sq, True)
    assert beq(idx, lbo) and beq(dist, sq)
    assert beq(ctx.umatrix().view(np.uint32), o.update_umatrix().view(np.uint32))
    lbo = np.zeros(40, np.uint64)
    mse_o = o.train_online_chunk(Y, lbo, 0.1, 2.0, po.EXPONENTIAL)
    ctx.upload_chunk(Y)
    mse_g = ctx.train_online_chunk(0.1, 2.0, capi.EXPONENTIAL)
    assert beq(np.float32(mse_g), np.float32(mse_o)) and beq(ctx.get_last_bmu(), lbo)
    st = ctx.get_state()
    for k in ("map", "S", "sigma", "weight", "hits"):
        assert beq(st[k], getattr(o, k)), k
    assert beq(ctx.umatrix().view(np.uint32), o.update_umatrix().view(np.uint32))
    ctx.close()


# ---- 8. two runs give the same bits ----------------------------------------------------------------------------------------
def test_deterministic():
    W, H, J, B = 12, 11, 33, 257
    X, init = rows_and_map(W, H, J, B)
    same_runs(run_accum(po.STANDARD, W, H, J, init, X, (100, 100, 57)), run_accum(po.STANDARD, W, H, J, init, X, (100, 100, 57)),
              "second run")


# ---- 9. mirrors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset_bmu", [True, False])
def test_som_mirror_equals_the_manual_loop_and_the_oracle(reset_bmu):
    W, H, J, B, chunk = 9, 7, 9, 110, 70
    X, init = rows_and_map(W, H, J, B)
    epochs, sigma0, decay = 4, 3.0, 0.5           # sigma 3, 1.82, 1.10, then 0.67 < 1: the fourth epoch does not run
    s = vs.Som(W, H, J)
    s.setState(map=init)
    ds = vs.ArrayDataSet(X, chunk)
    s.trainBatchSomWhole(ds, epochs, sigma0, decay, reset_bmu=reset_bmu)
    got = s.state()

    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    o = po.OracleSom(W, H, J)
    o.set_state(map=init)
    lb = np.zeros(B, np.uint64)
    metrics = []
    for e in range(3):
        sigma = sigma0 * math.exp(-decay * float(e))
        if reset_bmu:
            lb = np.zeros(B, np.uint64)           # a load zeroes lastBMU
        manual = accum_epoch(ctx, X, (70, 40), lb, sigma, e == 0)
        want = oracle_epoch(o, X, lb, sigma, e == 0)
        same_runs([manual], [want], ("manual loop", e), keys=("map", "sigma", "weight", "hits", "S", "lastbmu", "mse"))
        metrics.append(want["mse"][0])
    for k in ("map", "sigma", "S", "weight", "hits"):
        assert beq(got[k], getattr(o, k)), k
    assert beq(np.array(s.metrics.MeanSquaredError[:3], np.float32), np.array(metrics, np.float32))
    assert s.metrics.MeanSquaredError[3] == 0.0
    assert (ds.lastBMU == lb[70:]).all() and ds.lastBMU.size == 40
    assert ds.isAtStartOfDataStream() and not ds.hasReadWholeDataStream()
    ctx.close()
    s.close()


def test_som_mirror_on_one_chunk_equals_train_batch_som():
    W, H, J, B = 9, 7, 9, 110
    X, init = rows_and_map(W, H, J, B)
    a, b = vs.Som(W, H, J), vs.Som(W, H, J)
    dsa, dsb = vs.ArrayDataSet(X), vs.ArrayDataSet(X)
    a.setState(map=init)
    b.setState(map=init)
    a.trainBatchSomWhole(dsa, 3, 3.0, 0.2, updateUMatrixAfterEpoch=True)
    b.trainBatchSom(dsb, 3, 3.0, 0.2, updateUMatrixAfterEpoch=True)
    sa, sb = a.state(), b.state()
    for k in sa:
        assert beq(sa[k], sb[k]), k
    assert beq(np.array(a.metrics.MeanSquaredError, np.float32), np.array(b.metrics.MeanSquaredError, np.float32))
    assert (dsa.lastBMU == dsb.lastBMU).all()
    assert beq(a.getUMatrix().view(np.uint32), b.getUMatrix().view(np.uint32))
    a.close()
    b.close()


def test_cpp_mirror_driver():
    exe = os.path.join(HOST, "host_accum_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_accum_test ok" in res.stdout
