"""GPU: vsom_batch_accum_chunk_masked -- the masked chunk call of an accumulated batch epoch.  Every comparison is on the
bits (NaN equals NaN).  The reference is tests/masked_train_ref.py (MaskedOracle.epoch) on the CONCATENATED rows, mask and
lastBMU, and, GPU against GPU, vsom_batch_epoch_masked of a second context that holds all rows as one chunk.

Shapes: 9x7 (63 nodes) and 13x5 (65 nodes: a second node group with one live lane); J = 13 (a ragged block of 8 columns
for the carried chains) and J = 37 (past one 32-byte packed validity row); 107 rows as (37, 5, 64, 1) and 103 rows as
(33, 70) -- chunk borders off the 32-row validity word, a chunk of one row --, each also as one chunk and as a third split.
Every mask carries: column 0 and 5 clean, column 1 dirty in chunk 0 only, column 2 dirty in the last row only (fresh in the
last chunk), column 3 without a valid row in rows 0-36 (all of chunk 0, valid later), column 4 without a valid row at all, 10 %
invalid entries elsewhere, and NaN / inf / 1e30 at the invalid positions.  The ever-dirty columns (11 of 13, 35 of 37) leave
a ragged last block of four."""
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
import gen  # noqa: E402
import masked_train_ref as mref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")
KINDS = (po.STANDARD, po.MEDIAN)
SCHEDULE = ((3.0, True), (2.5, False))        # the exact search, then the local walk from the first epoch's BMUs
POISON = (np.float32(np.nan), np.float32(np.inf), np.float32(1e30))
FIELDS = ("map", "sigma", "weight", "hits", "lastbmu", "sqres", "mse")
SPLITS = {107: ((37, 5, 64, 1), (107,), (64, 43)), 103: ((33, 70), (103,), (70, 1, 32))}
CLEAN, CHUNK0, LAST_ROW, LATE, DEAD = (0, 5), 1, 2, 3, 4


def beq(a, b):
    """bitwise equality; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def same(a, b, what, keys=FIELDS):
    assert len(a) == len(b)
    for e, (sa, sb) in enumerate(zip(a, b)):
        for k in keys:
            assert beq(sa[k], sb[k]), (what, "epoch", e, k)


def engineered_mask(B, J, seed=11):
    valid = np.random.default_rng(seed).random((B, J)) < 0.9
    valid[:, list(CLEAN)] = True
    valid[:, CHUNK0] = True
    valid[[3, 17, 31], CHUNK0] = False
    valid[:, LAST_ROW] = True
    valid[B - 1, LAST_ROW] = False
    valid[:, LATE] = True
    valid[:37, LATE] = False
    valid[:, DEAD] = False
    assert (~valid).any(axis=0).sum() % 4 != 0          # a ragged last block of ever-dirty columns
    return valid


def poisoned(X, valid):
    X2 = X.copy()
    for i, (r, d) in enumerate(np.argwhere(~valid)):
        X2[r, d] = POISON[i % 3]
    return X2


@functools.lru_cache(maxsize=None)
def case(W, H, J, B, seed=3):
    """rows (poisoned at the invalid positions), mask, start map; callers do not modify them"""
    X, init = gen.blobs(B, J, 4, seed, 2), gen.random_map(W * H, J, seed=seed + 10)
    valid = engineered_mask(B, J)
    return poisoned(X, valid), valid, init


def snapshot(ctx, mse, lastbmu=None, sqres=None):
    st = ctx.get_state()
    return {"map": st["map"], "sigma": st["sigma"], "S": st["S"], "weight": st["weight"], "hits": st["hits"],
            "lastbmu": ctx.get_last_bmu() if lastbmu is None else lastbmu,
            "sqres": ctx.get_sqres() if sqres is None else sqres, "mse": np.array([mse], np.float32)}


def accum_epoch(ctx, X, valid, splits, lb_in, sigma, first, plain=(), finish="end"):
    """begin, one chunk call per split (masked with the chunk's rows of `valid`; the chunks listed in `plain` with the
    unmasked call), end; lastBMU and sqres of every chunk concatenated.  valid 1-D: the one_mask form."""
    assert sum(splits) == X.shape[0]
    ctx.batch_accum_begin(sigma, first, X.shape[0])
    lbs, sqs, off = [np.zeros(0, np.uint64)], [np.zeros(0, np.float32)], 0
    for k, B in enumerate(splits):
        ctx.upload_chunk(X[off:off + B])
        ctx.set_last_bmu(lb_in[off:off + B])
        if k in plain:
            ctx.batch_accum_chunk()
        else:
            v = np.array(valid if valid.ndim == 1 else valid[off:off + B])
            ctx.batch_accum_chunk_masked(v)
            v[...] = 0                       # the call has copied the bytes: what the caller does to them afterwards is its own
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


def run_accum(tr, W, H, J, init, X, valid, splits, schedule=SCHEDULE, plain=(), S=None):
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init, S=S)
    lb = np.zeros(X.shape[0], np.uint64)
    out = []
    for sigma, first in schedule:
        out.append(accum_epoch(ctx, X, valid, splits, lb, sigma, first, plain))
        lb = out[-1]["lastbmu"]
    ctx.close()
    return out


def run_one_chunk(tr, W, H, J, init, X, valid, schedule=SCHEDULE, S=None):
    """vsom_batch_epoch_masked on all rows as one chunk (lastBMU stays on the device between the epochs)"""
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init, S=S)
    ctx.upload_chunk(X)
    out = [snapshot(ctx, ctx.batch_epoch_masked(sigma, first, valid)) for sigma, first in schedule]
    ctx.close()
    return out


def oracle_runs(tr, W, H, J, init, X, valid, schedule):
    ref = mref.MaskedOracle(W, H, J, tr, init)
    lb = np.zeros(X.shape[0], np.uint64)
    out = []
    for sigma, first in schedule:
        mse, sq = ref.epoch(np.where(valid, X, np.float32(0)), valid, lb, sigma, first)
        out.append({"map": ref.map, "sigma": ref.sigma, "weight": ref.weight, "hits": ref.hits, "lastbmu": lb.copy(),
                    "sqres": sq, "mse": np.array([mse], np.float32)})
    return out


@functools.lru_cache(maxsize=None)
def reference(tr, W, H, J, B, schedule=SCHEDULE):
    """the helper's snapshots on the concatenated rows (computed once per case; callers do not modify them)"""
    X, valid, init = case(W, H, J, B)
    return oracle_runs(tr, W, H, J, init, X, valid, schedule)


# ---- 1. against the oracle, against the one-chunk masked epoch, and every split against every other ------------------------
@pytest.mark.parametrize("tr", KINDS)
@pytest.mark.parametrize("B", sorted(SPLITS))
@pytest.mark.parametrize("W, H, J", [(9, 7, 13), (13, 5, 37), (9, 7, 37), (13, 5, 13)])
def test_against_the_oracle_and_across_splits(tr, W, H, J, B):
    X, valid, init = case(W, H, J, B)
    S = gen.random_map(W * H, J, seed=77)
    want = reference(tr, W, H, J, B)
    one = run_one_chunk(tr, W, H, J, init, X, valid, S=S)
    same(one, want, "vsom_batch_epoch_masked")
    for splits in SPLITS[B]:
        got = run_accum(tr, W, H, J, init, X, valid, splits, S=S)
        same(got, want, splits)
        same(got, one, (splits, "one chunk"), keys=FIELDS + ("S",))     # (hence every split equals every other)
        assert beq(got[-1]["S"], S)                                     # SMap is untouched in batch mode
    m, s = got[-1]["map"], got[-1]["sigma"]
    assert (m[:, DEAD].view(np.uint32) == 0).all() and np.isnan(s[:, DEAD]).all()      # no valid row: +0 / NaN
    live = [d for d in range(J) if d != DEAD]
    assert np.isfinite(m[:, live]).all() and np.isfinite(s[:, live]).all()             # the poison reached nothing
    assert got[-1]["hits"].sum() == len(SCHEDULE) * B


# ---- 2. 0/0 chains stay NaN across the chunk border ------------------------------------------------------------------------
@pytest.mark.parametrize("tr", KINDS)
def test_sigma_one(tr):
    W, H, J, B = 9, 7, 13, 107
    X, valid, init = case(W, H, J, B)
    sched = ((1.0, True),)
    got = run_accum(tr, W, H, J, init, X, valid, SPLITS[B][0], sched)
    same(got, reference(tr, W, H, J, B, sched), "sigma 1")
    # w = 0 before a node's first hit: the chain of (node, column) is finite exactly where the first row valid at the column
    # chose the node -- for column LATE that row lies in the second chunk
    lb = got[0]["lastbmu"].astype(np.int64)
    some = valid.any(axis=0)
    first = valid.argmax(axis=0)
    assert first[LATE] == 37
    finite = lb[first][None, :] == np.arange(W * H)[:, None]
    assert (np.isnan(got[0]["map"][:, some]) == ~finite[:, some]).all()
    assert (got[0]["map"][:, DEAD].view(np.uint32) == 0).all()


# ---- 3. a column mask is the per-row mask replicated; all-valid masks are the plain sequence -------------------------------
@pytest.mark.parametrize("tr", KINDS)
def test_one_mask_equals_replicated_rows(tr):
    W, H, J, B = 13, 5, 37, 103
    X, _, init = case(W, H, J, B)
    col = np.random.default_rng(J).random(J) < 0.6
    col[0], col[J - 1], col[32] = True, False, False
    rep = np.broadcast_to(col, X.shape).copy()
    X = poisoned(np.where(np.isfinite(X) & (np.abs(X) < 1e20), X, np.float32(0.5)), rep)
    one = run_accum(tr, W, H, J, init, X, col, SPLITS[B][0])
    rows = run_accum(tr, W, H, J, init, X, rep, SPLITS[B][0])
    same(one, rows, "one_mask")
    same(one, run_one_chunk(tr, W, H, J, init, X, col), "one_mask, one chunk")
    assert np.isnan(one[-1]["sigma"][:, ~col]).all() and (one[-1]["map"][:, ~col].view(np.uint32) == 0).all()
    assert np.isfinite(one[-1]["map"][:, col]).all()


def plain_sequence(tr, W, H, J, init, X, splits, schedule=SCHEDULE):
    """the unmasked vsom_batch_accum_* sequence"""
    return run_accum(tr, W, H, J, init, X, None, splits, schedule, plain=range(len(splits)))


@pytest.mark.parametrize("tr", KINDS)
@pytest.mark.parametrize("W, H, J, B", [(9, 7, 13, 107), (13, 5, 37, 103)])
def test_all_valid_masks_equal_the_plain_sequence(tr, W, H, J, B):
    _, _, init = case(W, H, J, B)
    X = gen.blobs(B, J, 4, 3, 2)
    want = plain_sequence(tr, W, H, J, init, X, SPLITS[B][0])
    same(run_accum(tr, W, H, J, init, X, np.ones((B, J), np.uint8), SPLITS[B][0]), want, "B x J ones")
    same(run_accum(tr, W, H, J, init, X, np.ones(J, np.uint8), SPLITS[B][0]), want, "one row of ones")


# ---- 4. a plain chunk between masked chunks counts as all valid ------------------------------------------------------------
@pytest.mark.parametrize("tr", KINDS)
@pytest.mark.parametrize("plain", [(1,), (0,), (3,), (1, 2)])
def test_plain_chunks_among_masked_chunks(tr, plain):
    W, H, J, B = 13, 5, 13, 107
    splits = SPLITS[B][0]
    X, valid, init = case(W, H, J, B)
    valid = valid.copy()
    off = np.cumsum((0,) + splits)
    for k in plain:
        valid[off[k]:off[k + 1]] = True
    X = np.where(valid, np.where(np.isfinite(X) & (np.abs(X) < 1e20), X, np.float32(0.25)), X)    # a plain chunk reads every entry
    got = run_accum(tr, W, H, J, init, X, valid, splits, plain=plain)
    same(got, oracle_runs(tr, W, H, J, init, X, valid, SCHEDULE), plain)
    same(got, run_one_chunk(tr, W, H, J, init, X, valid), (plain, "one chunk"))


# ---- 5. the prefetch / commit pipeline behind a masked chunk ---------------------------------------------------------------
def test_pipeline_behind_masked_chunks():
    tr, W, H, J, B = po.STANDARD, 13, 5, 37, 107
    splits = SPLITS[B][0]
    X, valid, init = case(W, H, J, B)
    want = reference(tr, W, H, J, B)
    off = np.cumsum((0,) + splits)
    pbs = []
    for k in range(len(splits)):
        pbs.append(capi.PinnedBuffer((splits[k], J)))
        pbs[-1].array[...] = X[off[k]:off[k + 1]]
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init)
    lb = np.zeros(B, np.uint64)
    got = []
    for sigma, first in SCHEDULE:
        ctx.batch_accum_begin(sigma, first, B)
        lbs, sqs = [], []
        ctx.prefetch_chunk(pbs[0].array)
        for k in range(len(splits)):
            ctx.commit_chunk()
            ctx.set_last_bmu(lb[off[k]:off[k + 1]])
            v = valid[off[k]:off[k + 1]].astype(np.uint8)
            ctx.batch_accum_chunk_masked(v)
            v[...] = 0
            if k + 1 < len(splits):
                ctx.prefetch_chunk(pbs[k + 1].array)          # copied beside the chunk's chains, staged at the commit
            lbs.append(ctx.get_last_bmu())
            sqs.append(ctx.get_sqres())
        mse = ctx.batch_accum_end()
        got.append(snapshot(ctx, mse, np.concatenate(lbs), np.concatenate(sqs)))
        lb = got[-1]["lastbmu"]
    same(got, want, "pipeline")
    ctx.close()
    for pb in pbs:
        pb.free()


# ---- 6. abort, refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", KINDS)
def test_abort_restores_the_state(tr):
    W, H, J, B = 9, 7, 13, 107
    X, valid, init = case(W, H, J, B)
    S = gen.random_map(W * H, J, seed=77)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init, S=S)
    ctx.upload_chunk(X)
    ctx.batch_epoch_masked(3.0, True, valid)          # a state with sigmaMap and weightMap set
    before = ctx.get_state()
    snap = accum_epoch(ctx, X, valid, SPLITS[B][0], np.zeros(B, np.uint64), 2.5, True, finish="abort")
    for k in ("map", "sigma", "weight", "S"):
        assert beq(snap[k], before[k]), k
    assert snap["hits"].sum() == before["hits"].sum() + B          # what the chunk calls did stays
    # a new epoch starts without an ever-dirty column: on clean rows the unmasked sequence, then a masked one
    Xc = gen.blobs(B, J, 4, 3, 2)
    lb = np.zeros(B, np.uint64)
    got = accum_epoch(ctx, Xc, None, (64, 43), lb, 2.0, True, plain=(0, 1))
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=before["map"], sigma=before["sigma"], S=before["S"], weight=before["weight"])
    lbo = np.zeros(B, np.uint64)
    mse = o.batch_epoch(Xc, lbo, 2.0, True)
    for k, ref in (("map", o.map), ("sigma", o.sigma), ("weight", o.weight), ("lastbmu", lbo), ("mse", np.array([mse], np.float32))):
        assert beq(got[k], ref), k
    ref = mref.MaskedOracle(W, H, J, tr, got["map"])
    lb = np.zeros(B, np.uint64)
    mse, sq = ref.epoch(np.where(valid, X, np.float32(0)), valid, lb, 2.0, True)
    got = accum_epoch(ctx, X, valid, SPLITS[B][0], np.zeros(B, np.uint64), 2.0, True)
    for k, r in (("map", ref.map), ("sigma", ref.sigma), ("weight", ref.weight), ("lastbmu", lb), ("sqres", sq),
                 ("mse", np.array([mse], np.float32))):
        assert beq(got[k], r), k
    ctx.close()


def test_refusals_leave_the_state_alone():
    W, H, J, rows = 9, 7, 13, 20
    X, valid, init = case(W, H, J, 107)
    X, valid = X[40:40 + rows], valid[40:40 + rows]
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    L = capi.lib()
    h = ctx._h
    u8 = ctypes.POINTER(ctypes.c_uint8)
    ones = np.ones((rows + 1, J), np.uint8)

    def call(handle=h, v=ones, one=0):
        return L.vsom_batch_accum_chunk_masked(handle, None if v is None else v.ctypes.data_as(u8), one)

    def refused(code, word):
        assert code == -1, word
        assert word in L.vsom_last_error().decode(), (word, L.vsom_last_error().decode())

    refused(call(handle=None), "null context")
    refused(call(), "no accumulated epoch is open")
    ctx.batch_accum_begin(2.0, True, rows)
    refused(call(v=None), "valid_host")
    refused(call(), "no chunk loaded")
    ctx.upload_chunk(gen.blobs(rows + 1, J, 3, 1, 2))
    refused(call(), "exceed total_rows")
    with pytest.raises(ValueError):
        ctx.batch_accum_chunk_masked(np.ones((rows, J), np.uint8))           # the loaded chunk has rows + 1
    st = ctx.get_state()
    assert beq(st["map"], init) and not st["sigma"].any() and not st["weight"].any() and not st["hits"].any()
    # the context stays usable: one row short, end is refused; the missing row's chunk completes the epoch
    ctx.upload_chunk(X[:rows - 1])
    ctx.batch_accum_chunk_masked(valid[:rows - 1])
    lb0, sq0 = ctx.get_last_bmu(), ctx.get_sqres()
    refused(L.vsom_batch_accum_end(h, None), "rows accumulated")
    refused(call(), "exceed total_rows")
    ctx.upload_chunk(X[rows - 1:])
    ctx.batch_accum_chunk_masked(valid[rows - 1:])
    refused(call(v=np.ones((1, J), np.uint8)), "exceed total_rows")          # the same chunk once more
    lb1, sq1 = ctx.get_last_bmu(), ctx.get_sqres()
    mse = ctx.batch_accum_end()
    refused(call(), "no accumulated epoch is open")
    got = snapshot(ctx, mse, np.concatenate([lb0, lb1]), np.concatenate([sq0, sq1]))
    same([got], oracle_runs(po.STANDARD, W, H, J, init, X, valid, ((2.0, True),)), "after the refusals")
    ctx.close()

    # CLR: no epoch can be open
    clr = vsom_amd.Context(4, 4, 5, po.CLR)
    clr.upload_chunk((np.abs(gen.blobs(rows, 5, 3, 1, 2)) + np.float32(0.5)).astype(np.float32))
    with pytest.raises(capi.VsomError, match="no accumulated epoch is open"):
        clr.batch_accum_chunk_masked(np.ones(5, np.uint8))
    clr.close()


def test_large_map_and_a_chunk_staged_ahead():
    """48x48x196 with 2 x 1100 rows (36 node groups, search slices, the shortlist search of the plain chunk), GPU against
    GPU: masked chunk, plain chunk; and the masked call refuses a chunk staged ahead over the current rows"""
    W = H = 48
    J = 196
    xs = [gen.mnist_like(1100, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    v0 = np.random.default_rng(5).random((1100, J)) < 0.9
    late = int(np.argmax(xs[1].std(axis=0)))       # a column with data: without a valid row in chunk 0, valid in chunk 1
    v0[:, late] = False
    valid = np.concatenate([v0, np.ones((1100, J), bool)])
    want = run_one_chunk(po.STANDARD, W, H, J, init, np.concatenate(xs), valid, ((10.0, True),))
    ctx = vsom_amd.Context(W, H, J)
    pb = capi.PinnedBuffer(xs[1].shape)
    pb.array[...] = xs[1]
    ctx.set_state(map=init)
    ctx.upload_chunk(xs[0])
    ctx.batch_accum_begin(10.0, True, 2200)
    ctx.batch_epoch_async(10.0, True)              # (rewrites the state: only to have the next chunk staged ahead)
    ctx.prefetch_chunk(pb.array)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        ctx.batch_accum_chunk_masked(np.ones(J, np.uint8))
    ctx.commit_chunk()
    ctx.batch_accum_chunk_masked(np.ones(J, np.uint8))     # the context stays usable
    ctx.batch_accum_abort()
    ctx.set_state(map=init, sigma=np.zeros_like(init), weight=np.zeros(W * H, np.float32), hits=np.zeros(W * H, np.uint64))
    ctx.batch_accum_begin(10.0, True, 2200)
    ctx.upload_chunk(xs[0])
    ctx.batch_accum_chunk_masked(v0)
    lb0, sq0 = ctx.get_last_bmu(), ctx.get_sqres()
    ctx.upload_chunk(xs[1])
    ctx.batch_accum_chunk()
    lb1, sq1 = ctx.get_last_bmu(), ctx.get_sqres()
    got = snapshot(ctx, ctx.batch_accum_end(), np.concatenate([lb0, lb1]), np.concatenate([sq0, sq1]))
    same([got], want, "large map")
    assert (got["map"][:, late].view(np.uint32) != 0).any() and np.isfinite(got["sigma"][:, late]).all()
    ctx.close()
    pb.free()


# ---- 7. the staged chunk stays, two runs give the same bits ----------------------------------------------------------------
def test_chunk_unchanged_and_deterministic():
    tr, W, H, J, B = po.MEDIAN, 13, 5, 37, 103
    X, valid, init = case(W, H, J, B)
    Xz = np.where(valid, X, np.float32(0))           # (finite rows: they are read back through an all-valid query)
    runs = []
    for _ in range(2):
        ctx = vsom_amd.Context(W, H, J, tr)
        ctx.set_state(map=init)
        ctx.upload_chunk(Xz)
        chunk = ctx.device_ptr(capi.BUF_CHUNK)
        ctx.batch_accum_begin(3.0, True, B)
        ctx.batch_accum_chunk_masked(valid)
        assert ctx.device_ptr(capi.BUF_CHUNK) == chunk and ctx.chunk_size == B
        assert beq(ctx.bmu_masked(np.ones(J, np.uint8), fill=True)["fill"], Xz)       # the staged rows, read back
        lb, sq = ctx.get_last_bmu(), ctx.get_sqres()
        runs.append([snapshot(ctx, ctx.batch_accum_end(), lb, sq)])
        ctx.close()
    same(runs[0], runs[1], "second run")
    same(runs[0], run_accum(tr, W, H, J, init, X, valid, SPLITS[B][0], SCHEDULE[:1]), "poison or zeros at the invalid positions")


# ---- 8. mirrors ------------------------------------------------------------------------------------------------------------
class ValidDataSet(vs.ArrayDataSet):
    """an ArrayDataSet whose loaded rows carry validity flags"""

    def __init__(self, X, validity, maxLoadCount):
        super().__init__(X, maxLoadCount)
        self._validity = validity
        self.validity = validity[0:0]

    def loadNextDataFromStream(self):
        start = self._pos
        super().loadNextDataFromStream()
        self.validity = self._validity[start:start + self.data.shape[0]]


@pytest.mark.parametrize("reset_bmu", [True, False])
def test_som_mirror_equals_the_manual_loop(reset_bmu):
    W, H, J, B, chunk = 9, 7, 13, 107, 37
    X, valid, init = case(W, H, J, B)
    epochs, sigma0, decay = 4, 3.0, 0.5           # sigma 3, 1.82, 1.10, then 0.67 < 1: the fourth epoch does not run
    s = vs.Som(W, H, J)
    s._verbose = False
    s.setState(map=init)
    ds = ValidDataSet(X, valid, chunk)
    s.trainBatchSomWholeMasked(ds, epochs, sigma0, decay, reset_bmu=reset_bmu)
    got = s.state()

    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    lb = np.zeros(B, np.uint64)
    metrics = []
    for e in range(3):
        if reset_bmu:
            lb = np.zeros(B, np.uint64)           # a load zeroes lastBMU
        snap = accum_epoch(ctx, X, valid, (37, 37, 33), lb, sigma0 * math.exp(-decay * float(e)), e == 0)
        lb = snap["lastbmu"]
        metrics.append(snap["mse"][0])
    want = ctx.get_state()
    ctx.close()
    for k in want:
        assert beq(got[k], want[k]), k
    assert beq(np.array(s.metrics.MeanSquaredError[:3], np.float32), np.array(metrics, np.float32))
    assert s.metrics.MeanSquaredError[3] == 0.0
    assert (ds.lastBMU == lb[74:]).all() and ds.lastBMU.size == 33
    assert ds.isAtStartOfDataStream() and not ds.hasReadWholeDataStream()
    # without a validity attribute every column counts: trainBatchSomWhole
    a, b = vs.Som(W, H, J), vs.Som(W, H, J)
    Xz = np.where(valid, X, np.float32(0))
    for m, t in ((a, "trainBatchSomWholeMasked"), (b, "trainBatchSomWhole")):
        m._verbose = False
        m.setState(map=init)
        getattr(m, t)(vs.ArrayDataSet(Xz, chunk), 2, 3.0, 0.2, reset_bmu=reset_bmu)
    sa, sb = a.state(), b.state()
    for k in sa:
        assert beq(sa[k], sb[k]), k
    assert beq(np.array(a.metrics.MeanSquaredError, np.float32), np.array(b.metrics.MeanSquaredError, np.float32))
    for m in (s, a, b):
        m.close()


def test_cpp_mirror_driver_equals_the_python_one(tmp_path):
    exe = os.path.join(HOST, "host_accum_masked_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    out = str(tmp_path / "state.bin")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_accum_masked_test ok" in res.stdout
    # the program's flagged run (host/tests/host_accum_masked_test.cpp: make_rows, FlaggedLoader::valid, run) in Python
    W, H, J, B, chunk = 9, 7, 11, 30, 7
    vals, s = [], 2718
    for _ in range(B * J):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        vals.append(np.float32(np.float32((s >> 8) & 0xFFFF) / np.float32(65536.0) * np.float32(2.0) - np.float32(1.0)))
    X = np.array(vals, np.float32).reshape(B, J)
    r, d = np.meshgrid(np.arange(B), np.arange(J), indexing="ij")
    valid = (d == 0) | ((r * 7 + d * 3) % 5 != 0)
    valid[:, 4] = False
    valid[:, 6] = r[:, 6] < 24
    valid[:, 9] = r[:, 9] > 2
    som = vs.Som(W, H, J)
    som._verbose = False
    som.randomInitialize(7, 1)
    som.trainBatchSomWholeMasked(ValidDataSet(X, valid, chunk), 5, 3.0, 0.3, reset_bmu=False)
    st = som.state()
    N = W * H
    raw = open(out, "rb").read()
    assert len(raw) == (2 * N * J + N) * 4 + N * 8 + 5 * 4
    f = np.frombuffer(raw, np.float32, 2 * N * J + N)
    assert beq(f[:N * J].reshape(N, J), st["map"]) and beq(f[N * J:2 * N * J].reshape(N, J), st["sigma"])
    assert beq(f[2 * N * J:], st["weight"])
    assert beq(np.frombuffer(raw, np.uint64, N, (2 * N * J + N) * 4), st["hits"])
    assert beq(np.frombuffer(raw, np.float32, 5, (2 * N * J + N) * 4 + N * 8), np.array(som.metrics.MeanSquaredError, np.float32))
    som.close()
