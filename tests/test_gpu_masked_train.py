"""GPU: vsom_batch_epoch_masked -- the batch epoch over the valid entries of the chunk only.  Every comparison is on the
bits (NaN equals NaN).  The all-valid mask is checked against vsom_batch_epoch on every route that call takes (the
one-workgroup epoch of tiny maps, the small-map chains, the general kernels: chosen by shape and forced with VSOM_NO_TINY /
VSOM_NO_CHAIN); general masks against tests/masked_train_ref.py, which restates the contract on the CPU oracle.

Shapes: 7x5x9 with 70 rows (base), 12x11x33 with 257 rows (132 nodes: a second, partly filled wavefront; 33 columns cross
the 32-byte packing; 257 rows cross the 32- and 64-row words), J = 1, B in {1, 63, 65} (row-word edges), 10x10x9 with 20 rows
(the tiny route).  Every random mask carries a never-invalid column, a never-valid one, one valid in exactly one row and one
valid in the last row only (J = 1: the single column takes each of the four roles in turn).  13x5x13 with B in {1, 7, 8, 9, 31,
32, 33, 40} drives the chains' row walk across its group of 8 rows and its 32-row validity word, against the helper and
against masked accumulated epochs on the same rows (section 2b)."""
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
import masked_train_ref as mref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")
KINDS = (po.STANDARD, po.MEDIAN)
# first epoch, then two local epochs, sigma 3 -> 2.2
SCHEDULE = tuple((3.0 * math.exp(-0.155 * e), e == 0) for e in range(3))
POISON = (np.float32(np.nan), np.float32(np.inf), np.float32(1e30))
ROLES = ("clean", "dead", "one_row", "last_row")


def beq(a, b):
    """bitwise equality; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def rows_and_map(W, H, J, B, seed=3):
    return gen.blobs(B, J, 4, seed, 2), gen.random_map(W * H, J, seed=seed + 10)


def engineer(valid, col, role):
    B = valid.shape[0]
    valid[:, col] = role == "clean"
    if role == "one_row":
        valid[B // 2, col] = True
    if role == "last_row":
        valid[B - 1, col] = True


def random_mask(B, J, seed, role0=None):
    """30 % invalid entries and the engineered columns (module docstring); role0: the role of column 0 when J < 4"""
    valid = np.random.default_rng(seed).random((B, J)) < 0.7
    if J >= 4:
        for col, role in zip((1, J - 1, 0, J // 2), ROLES):     # (33 columns: column 32 lies past the 32-byte packing)
            engineer(valid, col, role)
    else:
        engineer(valid, 0, role0)
    return valid


def poisoned(X, valid):
    X2 = X.copy()
    at = np.argwhere(~valid)
    for i, (r, d) in enumerate(at):
        X2[r, d] = POISON[i % 3]
    return X2


def snapshot(ctx, mse):
    st = ctx.get_state()
    return {"map": st["map"], "sigma": st["sigma"], "S": st["S"], "weight": st["weight"], "hits": st["hits"],
            "lastbmu": ctx.get_last_bmu(), "sqres": ctx.get_sqres(), "mse": np.array([mse], np.float32)}


def run_gpu(tr, W, H, J, init, X, valid, schedule=SCHEDULE):
    """the snapshots after every epoch of a schedule; valid None: vsom_batch_epoch"""
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init)
    ctx.upload_chunk(X)
    out = []
    for sigma, first in schedule:
        mse = ctx.batch_epoch(sigma, first) if valid is None else ctx.batch_epoch_masked(sigma, first, valid)
        out.append(snapshot(ctx, mse))
    ctx.close()
    return out


def same_runs(a, b, what, keys=None):
    assert len(a) == len(b)
    for e, (sa, sb) in enumerate(zip(a, b)):
        for k in keys or sa:
            assert beq(sa[k], sb[k]), (what, "epoch", e, k)


@functools.lru_cache(maxsize=None)
def reference(tr, W, H, J, B, mask_seed, role0, schedule=SCHEDULE):
    """the helper's snapshots (computed once per case; callers do not modify them)"""
    X, init = rows_and_map(W, H, J, B)
    valid = random_mask(B, J, mask_seed, role0)
    ref = mref.MaskedOracle(W, H, J, tr, init)
    lb = np.zeros(B, np.uint64)
    out = []
    for sigma, first in schedule:
        mse, sq = ref.epoch(np.where(valid, X, np.float32(0)), valid, lb, sigma, first)
        out.append({"map": ref.map, "sigma": ref.sigma, "weight": ref.weight, "hits": ref.hits, "lastbmu": lb.copy(),
                    "sqres": sq, "mse": np.array([mse], np.float32)})
    return out


# ---- 1. the all-valid mask is vsom_batch_epoch, on every route -------------------------------------------------------------
ROUTES = [  # W, H, J, B, environment, (tiny, small-map chains) that vsom_batch_epoch takes
    (10, 10, 9, 20, {}, (True, True)),
    (7, 5, 9, 70, {"VSOM_NO_TINY": "1"}, (False, True)),
    (7, 5, 9, 70, {"VSOM_NO_TINY": "1", "VSOM_NO_CHAIN": "1"}, (False, False)),
    (12, 11, 33, 257, {}, (False, True)),
    (12, 11, 33, 257, {"VSOM_NO_CHAIN": "1"}, (False, False)),
    (5, 4, 1, 70, {}, (True, True)),
    (7, 5, 9, 1, {}, (True, True)),
    (7, 5, 9, 63, {"VSOM_NO_TINY": "1"}, (False, True)),
    (7, 5, 9, 65, {"VSOM_NO_TINY": "1", "VSOM_NO_CHAIN": "1"}, (False, False)),
]


@pytest.mark.parametrize("tr", KINDS)
@pytest.mark.parametrize("W, H, J, B, env, route", ROUTES)
def test_all_valid_equals_batch_epoch(monkeypatch, tr, W, H, J, B, env, route):
    for k, v in env.items():
        monkeypatch.setenv(k, v)         # (read when a context is created)
    X, init = rows_and_map(W, H, J, B)
    probe = vsom_amd.Context(W, H, J, tr)
    probe.upload_chunk(X)
    tiny = "VSOM_NO_TINY" not in env and B <= 256 and W * H * J <= 4096 and B * W * H <= 16384 and W * H * J * B <= 262144
    assert tiny == route[0]
    assert bool(capi.lib().vsom_small_map_chains(probe._h, W * H)) == route[1]
    probe.close()
    plain = run_gpu(tr, W, H, J, init, X, None)
    same_runs(run_gpu(tr, W, H, J, init, X, np.ones((B, J), np.uint8)), plain, "per-row mask")
    same_runs(run_gpu(tr, W, H, J, init, X, np.ones(J, np.uint8)), plain, "one_mask")
    assert np.isfinite(plain[-1]["map"]).all() and (plain[-1]["hits"].sum() == 3 * B)


# ---- 2. random masks against the helper; garbage at invalid positions -----------------------------------------------------
MASKED = [(7, 5, 9, 70, None, {}), (12, 11, 33, 257, None, {}), (12, 11, 33, 257, None, {"VSOM_NO_CHAIN": "1"}),
          (7, 5, 9, 1, None, {}), (7, 5, 9, 63, None, {}), (7, 5, 9, 65, None, {"VSOM_NO_TINY": "1", "VSOM_NO_CHAIN": "1"})] + \
         [(5, 4, 1, 70, role, {}) for role in ROLES]


@pytest.mark.parametrize("tr", KINDS)
@pytest.mark.parametrize("W, H, J, B, role0, env", MASKED)
def test_random_masks_against_the_helper(monkeypatch, tr, W, H, J, B, role0, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    X, init = rows_and_map(W, H, J, B)
    valid = random_mask(B, J, 100 + J + B, role0)
    if J >= 4 and B > 1:
        assert valid[:, 1].all() and not valid[:, J - 1].any() and valid[:, 0].sum() == 1
        assert valid[:, J // 2].sum() == 1 and valid[B - 1, J // 2]
    want = reference(tr, W, H, J, B, 100 + J + B, role0)
    zeros = run_gpu(tr, W, H, J, init, np.where(valid, X, np.float32(0)), valid)
    junk = run_gpu(tr, W, H, J, init, poisoned(X, valid), valid)
    same_runs(junk, zeros, "garbage at invalid positions")
    same_runs(zeros, want, "helper", keys=("lastbmu", "sqres", "mse", "hits", "weight", "map", "sigma"))
    for snap in zeros:
        assert beq(snap["S"], np.zeros_like(snap["S"]))            # SMap is untouched in batch mode
        dead = ~valid.any(axis=0)
        assert (snap["map"][:, dead].view(np.uint32) == 0).all() and np.isnan(snap["sigma"][:, dead]).all()


# ---- 2b. the borders of the chains' row walk: the group of 8 rows and the 32-row validity word ------------------------------
# 13x5 (65 nodes: a second node group with one live lane), J = 13.  Column 0 is clean, column 1 has no valid row, column 2 is
# invalid in the last row only, column 3 in row 0 only; the other columns are 80 % valid from BORDER_SEED, which was picked
# so that one of them stays valid through all 40 rows: the dirty columns (7, 10, then 11) never fill their last block of 4.
BORDER_ROWS = (1, 7, 8, 9, 31, 32, 33, 40)
BORDER_SCHEDULE = ((3.0, True), (2.5, False))
BORDER_SEED = 1793
BORDER_KEYS = ("map", "sigma", "weight", "hits", "lastbmu", "sqres", "mse")


def border_mask(B, J):
    valid = np.random.default_rng(BORDER_SEED).random((B, J)) < 0.8
    valid[:, 0] = True
    valid[:, 1] = False
    valid[:, 2] = True
    valid[B - 1, 2] = False
    valid[:, 3] = True
    valid[0, 3] = False
    return valid


@functools.lru_cache(maxsize=None)
def border_reference(tr, W, H, J, B):
    """the helper's snapshots (computed once per case; callers do not modify them)"""
    X, init = rows_and_map(W, H, J, B)
    valid = border_mask(B, J)
    ref = mref.MaskedOracle(W, H, J, tr, init)
    lb = np.zeros(B, np.uint64)
    out = []
    for sigma, first in BORDER_SCHEDULE:
        mse, sq = ref.epoch(np.where(valid, X, np.float32(0)), valid, lb, sigma, first)
        out.append({"map": ref.map, "sigma": ref.sigma, "weight": ref.weight, "hits": ref.hits, "lastbmu": lb.copy(),
                    "sqres": sq, "mse": np.array([mse], np.float32)})
    return out


def run_accum_masked(tr, W, H, J, init, X, valid, splits):
    """BORDER_SCHEDULE as masked accumulated epochs over the rows cut into `splits`; lastBMU and sqres concatenated"""
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init)
    lb = np.zeros(X.shape[0], np.uint64)
    out = []
    for sigma, first in BORDER_SCHEDULE:
        ctx.batch_accum_begin(sigma, first, X.shape[0])
        lbs, sqs, off = [], [], 0
        for n in splits:
            ctx.upload_chunk(X[off:off + n])
            ctx.set_last_bmu(lb[off:off + n])
            ctx.batch_accum_chunk_masked(valid[off:off + n])
            lbs.append(ctx.get_last_bmu())
            sqs.append(ctx.get_sqres())
            off += n
        mse = ctx.batch_accum_end()
        lb = np.concatenate(lbs)
        out.append(dict(snapshot(ctx, mse), lastbmu=lb, sqres=np.concatenate(sqs)))
    ctx.close()
    return out


@pytest.mark.parametrize("tr", KINDS)
@pytest.mark.parametrize("B", BORDER_ROWS)
def test_row_group_and_validity_word_borders(tr, B):
    W, H, J = 13, 5, 13
    X, init = rows_and_map(W, H, J, B)
    valid = border_mask(B, J)
    assert valid[:, 0].all() and not valid[:, 1].any()
    assert (~valid).any(axis=0).sum() % 4 != 0                  # a ragged last block of dirty columns
    X = poisoned(X, valid)
    want = border_reference(tr, W, H, J, B)
    got = run_gpu(tr, W, H, J, init, X, valid, BORDER_SCHEDULE)
    same_runs(got, want, "helper", keys=BORDER_KEYS)
    for snap in got:
        assert (snap["map"][:, 1].view(np.uint32) == 0).all() and np.isnan(snap["sigma"][:, 1]).all()
    for splits in ((B,), (B // 2, B - B // 2))[:1 if B < 2 else 2]:
        same_runs(run_accum_masked(tr, W, H, J, init, X, valid, splits), got, ("accumulated", splits), keys=BORDER_KEYS)


# ---- 3. winner takes all ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", KINDS)
def test_sigma_one(tr):
    W, H, J, B = 7, 5, 9, 70
    X, init = rows_and_map(W, H, J, B)
    valid = random_mask(B, J, 7, None)
    sched = ((1.0, True),)
    want = reference(tr, W, H, J, B, 7, None, sched)
    got = run_gpu(tr, W, H, J, init, poisoned(X, valid), valid, sched)
    same_runs(got, want, "sigma 1", keys=("lastbmu", "sqres", "mse", "hits", "weight", "map", "sigma"))
    # the chain of (node, column) turns NaN at the first valid row it meets with W_d = 0 (0/0) and stays NaN: it is finite
    # exactly where the first row valid at the column chose the node
    lb = got[0]["lastbmu"].astype(np.int64)
    some = valid.any(axis=0)           # (a column without a valid row keeps M = +0)
    first = valid.argmax(axis=0)
    finite = lb[first][None, :] == np.arange(W * H)[:, None]
    assert (np.isnan(got[0]["map"][:, some]) == ~finite[:, some]).all()
    assert np.isnan(got[0]["map"]).any() and not np.isnan(got[0]["map"]).all()


# ---- 4. a column mask is the per-row mask replicated -----------------------------------------------------------------------
@pytest.mark.parametrize("tr", KINDS)
@pytest.mark.parametrize("W, H, J, B", [(7, 5, 9, 70), (12, 11, 33, 257)])
def test_one_mask_equals_replicated_rows(tr, W, H, J, B):
    X, init = rows_and_map(W, H, J, B)
    col = np.random.default_rng(J).random(J) < 0.6
    col[0], col[J - 1] = True, False
    X = poisoned(X, np.broadcast_to(col, X.shape))
    one = run_gpu(tr, W, H, J, init, X, col)
    rows = run_gpu(tr, W, H, J, init, X, np.broadcast_to(col, X.shape).copy())
    same_runs(one, rows, "one_mask")
    assert np.isnan(one[-1]["sigma"][:, ~col]).all() and (one[-1]["map"][:, ~col].view(np.uint32) == 0).all()
    assert np.isfinite(one[-1]["map"][:, col]).all()


# ---- 5. the chunk and SMap stay, two runs give the same bits ----------------------------------------------------------------
def test_chunk_and_smap_unchanged_and_deterministic():
    tr, W, H, J, B = po.STANDARD, 12, 11, 33, 257
    X, init = rows_and_map(W, H, J, B)
    valid = random_mask(B, J, 5)
    S = gen.random_map(W * H, J, seed=77)
    runs = []
    for _ in range(2):
        ctx = vsom_amd.Context(W, H, J, tr)
        ctx.set_state(map=init, S=S)
        ctx.upload_chunk(X)
        chunk = ctx.device_ptr(capi.BUF_CHUNK)
        snaps = [snapshot(ctx, ctx.batch_epoch_masked(s, f, valid)) for s, f in SCHEDULE]
        assert ctx.device_ptr(capi.BUF_CHUNK) == chunk and ctx.chunk_size == B
        assert beq(ctx.bmu_masked(np.ones(J, np.uint8), fill=True)["fill"], X)      # the staged rows, read back
        assert all(beq(s["S"], S) for s in snaps)
        runs.append(snaps)
        ctx.close()
    same_runs(runs[0], runs[1], "second run")


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def oracle_follows(ctx, o, X, what):
    """a following vsom_batch_epoch matches the oracle: the refusals left the state alone"""
    lbo = np.zeros(X.shape[0], np.uint64)
    assert np.float32(ctx.batch_epoch(1.5, True)) == np.float32(o.batch_epoch(X, lbo, 1.5, True)), what
    st = ctx.get_state()
    for k, ref in (("map", o.map), ("sigma", o.sigma), ("S", o.S), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], ref), (what, k)
    assert (ctx.get_last_bmu() == lbo).all(), what


def test_refusals_leave_the_state_alone():
    W, H, J, rows = 6, 5, 7, 20
    init = gen.random_map(W * H, J, seed=1)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    L = capi.lib()
    u8 = ctypes.POINTER(ctypes.c_uint8)
    valid = np.ones((rows, J), np.uint8)
    mse = ctypes.c_float()

    def rc(h=ctx._h, v=valid, m=mse):
        return L.vsom_batch_epoch_masked(h, 2.0, 1, None if v is None else v.ctypes.data_as(u8), 0,
                                         None if m is None else ctypes.byref(m))

    def refused(code, word):
        assert code == -1, word
        assert word in L.vsom_last_error().decode(), (word, L.vsom_last_error().decode())

    refused(rc(), "no chunk")
    refused(rc(h=None), "null context")
    X = gen.blobs(rows, J, 3, 1, 2)
    ctx.upload_chunk(X)
    before = ctx.get_state()
    refused(rc(v=None), "valid_host")
    refused(rc(m=None), "mse_out")
    ctx.set_update_mode(capi.UPDATE_FMA)
    refused(rc(), "strict")
    ctx.set_update_mode(capi.UPDATE_FMA_SIGMA)
    refused(rc(), "strict")
    ctx.set_update_mode(capi.UPDATE_STRICT)
    after = ctx.get_state()
    for k in before:
        assert beq(before[k], after[k]), k
    o = po.OracleSom(W, H, J)
    o.set_state(map=init)
    oracle_follows(ctx, o, X, "after refusals")
    ctx.close()

    # CLR contexts
    Xc = (np.abs(gen.blobs(rows, 5, 3, 1, 2)) + np.float32(0.5)).astype(np.float32)
    clr = vsom_amd.Context(4, 4, 5, po.CLR)
    oc = po.OracleSom(4, 4, 5, po.CLR)
    initc = gen.random_map(16, oc.depth, seed=2)
    clr.set_state(map=initc)
    oc.set_state(map=initc)
    clr.upload_chunk(Xc)
    with pytest.raises(capi.VsomError, match="CLR"):
        clr.batch_epoch_masked(2.0, True, np.ones((rows, 5), np.uint8))
    oracle_follows(clr, oc, Xc, "CLR after the refusal")
    clr.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_batch_epoch_masked"):
        cu.batch_epoch_masked(2.0, True, np.ones((10, 5), np.uint8))
    cu.bmu_batch()
    cu.close()

    # a chunk staged ahead (as tests/test_gpu_masked.py): refused until it is committed
    W = H = 48
    J = 196
    xs = [gen.mnist_like(1100, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    big = vsom_amd.Context(W, H, J)
    ref = vsom_amd.Context(W, H, J)
    pb = capi.PinnedBuffer(xs[1].shape)
    pb.array[...] = xs[1]
    for c in (big, ref):
        c.set_state(map=init)
        c.upload_chunk(xs[0])
        c.batch_epoch_async(10.0, True)
    big.prefetch_chunk(pb.array)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        big.batch_epoch_masked(8.0, True, np.ones(J, np.uint8))
    big.commit_chunk()
    ref.upload_chunk(xs[1])
    a = snapshot(big, big.batch_epoch_masked(8.0, True, np.ones(J, np.uint8)))
    b = snapshot(ref, ref.batch_epoch(8.0, True))
    same_runs([a], [b], "after the commit")
    big.close()
    ref.close()
    pb.free()


# ---- 4b. an empty chunk ----------------------------------------------------------------------------------------------------
def test_empty_chunk_behaves_as_batch_epoch():
    W, H, J = 6, 5, 7
    init = gen.random_map(W * H, J, seed=1)
    snaps = []
    for masked in (False, True):
        ctx = vsom_amd.Context(W, H, J)
        ctx.set_state(map=init)
        ctx.upload_chunk(np.zeros((0, J), np.float32))
        mse = ctx.batch_epoch_masked(2.0, True, np.zeros((0, J), np.uint8)) if masked else ctx.batch_epoch(2.0, True)
        st = ctx.get_state()
        snaps.append({"map": st["map"], "sigma": st["sigma"], "S": st["S"], "weight": st["weight"], "hits": st["hits"],
                      "mse": np.array([mse], np.float32)})
        ctx.close()
    same_runs([snaps[1]], [snaps[0]], "empty chunk")
    assert np.isnan(snaps[1]["sigma"]).all() and not snaps[1]["map"].any()


# ---- 7. mirrors ------------------------------------------------------------------------------------------------------------
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


def test_som_mirror_equals_the_manual_loop():
    W, H, J, B, chunk = 9, 7, 9, 110, 70
    X, init = rows_and_map(W, H, J, B)
    valid = random_mask(B, J, 9)
    X = poisoned(X, valid)
    epochs, sigma0, decay = 4, 3.0, 0.5           # sigma 3, 1.82, 1.10, then 0.67 < 1: the fourth epoch does not run
    s = vs.Som(W, H, J)
    s._verbose = False
    s.setState(map=init)
    ds = ValidDataSet(X, valid, chunk)
    s.trainBatchSomMasked(ds, epochs, sigma0, decay)
    got = s.state()

    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    metrics = []
    for e in range(epochs):
        sigma = sigma0 * math.exp(-decay * float(e))
        if sigma < 1.0:
            break
        mse = np.float32(0)
        for r0 in (0, chunk):
            ctx.upload_chunk(X[r0:r0 + chunk])
            if e:
                ctx.set_last_bmu(np.zeros(X[r0:r0 + chunk].shape[0], np.uint64))     # a load zeroes lastBMU
            mse = np.float32(mse + ctx.batch_epoch_masked(sigma, e == 0, valid[r0:r0 + chunk]))
        metrics.append(np.float32(mse / np.float32(2)))
        last = ctx.get_last_bmu()
    want = ctx.get_state()
    ctx.close()
    assert len(metrics) == 3
    for k in want:
        assert beq(got[k], want[k]), k
    assert beq(np.array(s.metrics.MeanSquaredError[:3], np.float32), np.array(metrics, np.float32))
    assert s.metrics.MeanSquaredError[3] == 0.0
    assert (ds.lastBMU == last).all()
    # without a validity attribute every column counts: trainBatchSom
    a, b = vs.Som(W, H, J), vs.Som(W, H, J)
    Xz = np.where(valid, X, np.float32(0))
    for m, t in ((a, "trainBatchSomMasked"), (b, "trainBatchSom")):
        m._verbose = False
        m.setState(map=init)
        getattr(m, t)(vs.ArrayDataSet(Xz, chunk), 2, 3.0, 0.2)
    sa, sb = a.state(), b.state()
    for k in sa:
        assert beq(sa[k], sb[k]), k
    assert beq(np.array(a.metrics.MeanSquaredError, np.float32), np.array(b.metrics.MeanSquaredError, np.float32))
    for m in (s, a, b):
        m.close()


def test_cpp_mirror_driver():
    exe = os.path.join(HOST, "host_masked_train_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_masked_train_test ok" in res.stdout
