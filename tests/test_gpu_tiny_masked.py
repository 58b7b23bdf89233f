"""GPU: the masked one-workgroup epoch -- vsom_batch_schedule_masked, vsom_ensemble_batch_epoch_masked,
vsom_ensemble_batch_schedule_masked, vsom_masked_tiny_applies.  Every comparison is on the bits (NaN equals NaN).

Two references, neither of them the kernel under test: tests/masked_train_ref.py::MaskedOracle (the CPU oracle restated per
column) and the general masked path on a twin context -- the loop of vsom_batch_epoch_masked calls the contract names (for
a plain member vsom_batch_epoch / vsom_batch_schedule).  Masks are test_gpu_masked_train.random_mask: 30 % invalid entries
and four engineered columns (never invalid, never valid, valid in one row only, valid in the last row only); every masked
case runs a second time with NaN / inf / 1e30 at the invalid positions.

Shapes: 10x10x9 B = 20 (the reference's perf scenario), 7x5x9 with B in {1, 31, 32, 33, 70} (the edges of the 32-row
validity word), 5x4x33 (column 32 past a word of 32 columns), 5x4x1 (the single column in each role), 16x16x16 B = 64 (on
all three bounds of the one-launch path), 6x4x41 B = 256 (rows not staged in LDS), 7x5x9 B = 257 (off the fast path)."""
import ctypes as C
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
import schedule_ref as sref  # noqa: E402
from test_gpu_masked_train import ROLES, ValidDataSet, beq, poisoned, random_mask, rows_and_map  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")
KINDS = (po.STANDARD, po.MEDIAN)
SIGMAS = tuple(3.0 * math.exp(-0.155 * e) for e in range(3))
KEYS = ("map", "sigma", "S", "weight", "hits", "lastbmu", "sqres", "mse")
MAXE = capi.SCHEDULE_MAX_EPOCHS


def snapshot(ctx):
    st = ctx.get_state()
    return {"map": st["map"], "sigma": st["sigma"], "S": st["S"], "weight": st["weight"], "hits": st["hits"],
            "lastbmu": ctx.get_last_bmu(), "sqres": ctx.get_sqres(), "mse": np.array([ctx.get_mse()], np.float32)}


def same_state(a, b, what, keys=KEYS):
    for k in keys:
        assert beq(a[k], b[k]), (what, k)


def context(tr, W, H, J, init, X=None):
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init)
    if X is not None:
        ctx.upload_chunk(X)
    return ctx


def loop(ctx, sigmas, valid, reset, first=True):
    """the contract: the loop of single masked epochs on a context whose chunk is loaded (valid None: the plain loop)"""
    if valid is None:
        return sref.twin_loop(ctx, sigmas, reset_bmu=reset)
    zeros = np.zeros(ctx.chunk_size, np.uint64)
    mse = np.zeros(len(sigmas), np.float32)
    for ep, sigma in enumerate(sigmas):
        if ep > 0 and reset:
            ctx.set_last_bmu(zeros)
        mse[ep] = ctx.batch_epoch_masked(sigma, first and ep == 0, valid)
    return mse


def scheduled(tr, W, H, J, init, X, valid, sigmas, reset):
    ctx = context(tr, W, H, J, init, X)
    mse = ctx.batch_schedule_masked(sigmas, valid, reset_bmu=reset)
    assert mse.dtype == np.float32 and mse.shape == (len(sigmas),)
    snap = snapshot(ctx)
    ctx.close()
    return mse, snap


def looped(tr, W, H, J, init, X, valid, sigmas, reset):
    ctx = context(tr, W, H, J, init, X)
    mse = loop(ctx, sigmas, valid, reset)
    snap = snapshot(ctx)
    ctx.close()
    return mse, snap


# ---- 1. the path predicate, both sides of every threshold ----------------------------------------------------------------
def applies(W, H, J, B, tr=po.STANDARD, one=False, mode=None):
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.upload_chunk(gen.correlated(B, J, 1) if tr == po.CLR else gen.blobs(B, J, 2, 1, 2))
    if mode is not None:
        ctx.set_update_mode(mode)
    got = ctx.masked_tiny_applies(one)
    ctx.close()
    return got


def test_path_predicate(monkeypatch):
    for one in (False, True):
        assert applies(10, 10, 9, 20, one=one)
        assert applies(16, 16, 16, 64, one=one)        # 4096 chains, B N = 16384, chains B = 262144
        assert applies(6, 4, 41, 256, one=one)         # rows J = 10496 > 10240: the rows are not staged in LDS
        assert applies(10, 10, 9, 20, po.MEDIAN, one=one)
        assert not applies(16, 16, 16, 65, one=one)
        assert not applies(7, 5, 9, 257, one=one)
        assert not applies(7, 7, 6, 20, po.CLR, one=one)
        assert not applies(10, 10, 9, 20, mode=capi.UPDATE_FMA, one=one)
        assert not applies(10, 10, 9, 20, mode=capi.UPDATE_FMA_SIGMA, one=one)
    no_chunk = vsom_amd.Context(10, 10, 9)
    assert not no_chunk.masked_tiny_applies()
    no_chunk.close()
    assert capi.lib().vsom_masked_tiny_applies(None, 0) == 0
    monkeypatch.setenv("VSOM_NO_TINY", "1")             # (read when a context is created)
    assert not applies(10, 10, 9, 20)


# ---- 2. the all-valid mask is vsom_batch_schedule ------------------------------------------------------------------------
@pytest.mark.parametrize("reset", [1, 0])
@pytest.mark.parametrize("tr", KINDS)
@pytest.mark.parametrize("W, H, J, B", [(10, 10, 9, 20), (5, 4, 1, 70), (7, 5, 9, 1)])
def test_all_valid_equals_batch_schedule(W, H, J, B, tr, reset):
    X, init = rows_and_map(W, H, J, B)
    plain = context(tr, W, H, J, init, X)
    mse_p = plain.batch_schedule(SIGMAS, reset_bmu=reset)
    want = snapshot(plain)
    plain.close()
    for valid in (np.ones((B, J), np.uint8), np.ones(J, np.uint8)):
        mse, got = scheduled(tr, W, H, J, init, X, valid, SIGMAS, reset)
        assert beq(mse, mse_p), ("per-epoch MSE", valid.ndim)
        same_state(got, want, ("all valid", valid.ndim))
    assert np.isfinite(want["map"]).all() and want["hits"].sum() == 3 * B


# ---- 3. random masks: the oracle epoch by epoch, and the loop ------------------------------------------------------------
MASKED = [(10, 10, 9, 20, None)] + [(7, 5, 9, B, None) for B in (1, 31, 32, 33, 70)] + [(5, 4, 33, 40, None)] + \
         [(5, 4, 1, 70, role) for role in ROLES] + [(16, 16, 16, 64, None), (6, 4, 41, 256, None)]


@functools.lru_cache(maxsize=None)
def oracle_epochs(tr, W, H, J, B, role0, reset):
    """MaskedOracle's snapshot after every epoch of SIGMAS (computed once per case; callers do not modify them)"""
    X, init = rows_and_map(W, H, J, B)
    valid = random_mask(B, J, 100 + J + B, role0)
    ref = mref.MaskedOracle(W, H, J, tr, init)
    lb = np.zeros(B, np.uint64)
    out = []
    for ep, sigma in enumerate(SIGMAS):
        if ep > 0 and reset:
            lb[:] = 0
        mse, sq = ref.epoch(np.where(valid, X, np.float32(0)), valid, lb, sigma, ep == 0)
        out.append({"map": ref.map.copy(), "sigma": ref.sigma.copy(), "weight": ref.weight.copy(), "hits": ref.hits.copy(),
                    "lastbmu": lb.copy(), "sqres": sq.copy(), "mse": np.array([mse], np.float32)})
    return out


@pytest.mark.parametrize("reset", [1, 0])
@pytest.mark.parametrize("tr", KINDS)
@pytest.mark.parametrize("W, H, J, B, role0", MASKED)
def test_random_masks_against_the_oracle_and_the_loop(W, H, J, B, role0, tr, reset):
    X, init = rows_and_map(W, H, J, B)
    valid = random_mask(B, J, 100 + J + B, role0)
    if J >= 4 and B > 1:
        assert valid[:, 1].all() and not valid[:, J - 1].any() and valid[:, 0].sum() == 1
        assert valid[:, J // 2].sum() == 1 and valid[B - 1, J // 2]
    probe = context(tr, W, H, J, init, X)
    assert probe.masked_tiny_applies()                   # every case here runs the one-workgroup kernel
    probe.close()
    Xz = np.where(valid, X, np.float32(0))
    want = oracle_epochs(tr, W, H, J, B, role0, reset)
    okeys = ("lastbmu", "sqres", "mse", "hits", "weight", "map", "sigma")
    # epoch by epoch: the schedule's prefixes against the oracle's snapshots
    for n in range(1, len(SIGMAS) + 1):
        mse, got = scheduled(tr, W, H, J, init, Xz, valid, SIGMAS[:n], reset)
        same_state(got, want[n - 1], ("oracle", n), okeys)
        assert beq(mse, np.concatenate([w["mse"] for w in want[:n]])), ("oracle, every MSE", n)
        assert beq(got["S"], np.zeros_like(got["S"]))                  # SMap is untouched in batch mode
        dead = ~valid.any(axis=0)
        assert (got["map"][:, dead].view(np.uint32) == 0).all() and np.isnan(got["sigma"][:, dead]).all()
    # the whole schedule against the loop on a twin, and with garbage at the invalid positions
    mse_l, twin = looped(tr, W, H, J, init, Xz, valid, SIGMAS, reset)
    same_state(got, twin, "loop")
    assert beq(mse, mse_l), "loop, every MSE"
    mse_j, junk = scheduled(tr, W, H, J, init, poisoned(X, valid), valid, SIGMAS, reset)
    same_state(junk, got, "garbage at invalid positions")
    assert beq(mse_j, mse)


def test_reset_bmu_matters():
    """reset_bmu 0 and 1 end differently on the 10x10x9 scenario (else the pairs above would show nothing about it)"""
    W, H, J, B = 10, 10, 9, 20
    differ = False
    for tr in KINDS:
        a, b = oracle_epochs(tr, W, H, J, B, None, 1)[-1], oracle_epochs(tr, W, H, J, B, None, 0)[-1]
        differ = differ or not all(beq(a[k], b[k]) for k in ("map", "lastbmu", "sqres", "mse"))
    assert differ


def test_one_mask_equals_replicated_rows():
    W, H, J, B = 10, 10, 9, 20
    X, init = rows_and_map(W, H, J, B)
    col = np.random.default_rng(J).random(J) < 0.6
    col[0], col[J - 1] = True, False
    full = np.broadcast_to(col, X.shape).copy()
    X = poisoned(X, full)
    for tr in KINDS:
        mse_o, one = scheduled(tr, W, H, J, init, X, col, SIGMAS, 1)
        mse_r, rows = scheduled(tr, W, H, J, init, X, full, SIGMAS, 1)
        mse_l, twin = looped(tr, W, H, J, init, X, col, SIGMAS, 1)
        same_state(one, rows, "one_mask against replicated rows")
        same_state(one, twin, "one_mask against the loop")
        assert beq(mse_o, mse_r) and beq(mse_o, mse_l)
        assert np.isnan(one["sigma"][:, ~col]).all() and (one["map"][:, ~col].view(np.uint32) == 0).all()


# ---- 4. off the fast path: the loop inside the library -------------------------------------------------------------------
@pytest.mark.parametrize("how", ["B257", "no_tiny", "nan_sigma"])
def test_off_the_fast_path(monkeypatch, how):
    W, H, J, B = 7, 5, 9, 257 if how == "B257" else 70
    if how == "no_tiny":
        monkeypatch.setenv("VSOM_NO_TINY", "1")
    sigmas = (3.0, float("nan"), 2.0) if how == "nan_sigma" else SIGMAS
    X, init = rows_and_map(W, H, J, B)
    valid = random_mask(B, J, 7)
    X = poisoned(X, valid)
    for tr in KINDS:
        probe = context(tr, W, H, J, init, X)
        assert probe.masked_tiny_applies() == (how == "nan_sigma")
        probe.close()
        mse, got = scheduled(tr, W, H, J, init, X, valid, sigmas, 1)
        mse_l, twin = looped(tr, W, H, J, init, X, valid, sigmas, 1)
        same_state(got, twin, how)
        assert beq(mse, mse_l)


# ---- 5. launch rounds ----------------------------------------------------------------------------------------------------
def test_schedule_longer_than_one_launch():
    W, H, J, B = 2, 2, 1, 3
    X, init = rows_and_map(W, H, J, B)
    valid = np.array([[1], [0], [1]], np.uint8)
    sigmas = [1.5] * (MAXE + 1)
    mse, got = scheduled(po.STANDARD, W, H, J, init, X, valid, sigmas, 1)
    mse_l, twin = looped(po.STANDARD, W, H, J, init, X, valid, sigmas, 1)
    assert mse.shape == (MAXE + 1,) and beq(mse, mse_l)
    same_state(got, twin, "1025 epochs")
    assert got["hits"].sum() == (MAXE + 1) * B


# ---- 6. ensembles --------------------------------------------------------------------------------------------------------
class Member:
    def __init__(self, W, H, J, tr, B, seed, masked, one=False, X=None):
        self.W, self.H, self.J, self.tr, self.B = W, H, J, tr, B
        self.X = X if X is not None else (gen.correlated(B, J, seed) if tr == po.CLR else gen.blobs(B, J, 4, seed, seed + 1))
        self.init = gen.random_map(W * H, po.length(tr, J), seed=seed + 3)
        self.m, self.t = context(tr, W, H, J, self.init), context(tr, W, H, J, self.init)
        self.valid = None
        if masked:
            self.valid = random_mask(B, J, seed + 50)
            if one:
                self.valid = self.valid[B // 3].copy()
                self.valid[0] = True

    def rows(self, seed):
        return gen.correlated(self.B, self.J, seed) if self.tr == po.CLR else gen.blobs(self.B, self.J, 3, seed, seed + 2)

    def check(self, what):
        same_state(snapshot(self.m), snapshot(self.t), what)

    def close(self):
        self.m.close()
        self.t.close()


def six_members():
    shared = gen.blobs(20, 9, 4, 61, 62)
    return [Member(10, 10, 9, po.STANDARD, 20, 61, True, X=shared),
            Member(10, 10, 9, po.MEDIAN, 20, 62, True, one=True, X=shared),     # the same host rows as member 0
            Member(5, 4, 33, po.STANDARD, 40, 63, True),
            Member(7, 5, 9, po.STANDARD, 257, 64, True),                        # off the fast path
            Member(7, 7, 6, po.CLR, 30, 65, False),
            Member(6, 5, 7, po.STANDARD, 30, 66, False)]


_STREAM = []


def shared_stream():
    """one stream for the members of an ensemble, alive for the whole module (contexts keep the handle)"""
    import torch
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream(device=torch.device("cuda", 0)))
    return _STREAM[0]


@pytest.mark.parametrize("shared", [True, False])
def test_ensemble_of_masked_and_plain_members(shared):
    members = six_members()
    n = len(members)
    stream = shared_stream() if shared else None
    if shared:
        for mb in members:
            mb.m.set_stream(stream.cuda_stream)
    ens = vsom_amd.Ensemble([mb.m for mb in members])
    valids = [mb.valid for mb in members]
    flags = [mb.m.masked_tiny_applies(mb.valid is not None and mb.valid.ndim == 1) for mb in members]
    ens.upload_chunks([mb.X for mb in members])          # members 0 and 1 name one array: packed once
    for mb in members:
        mb.t.upload_chunk(mb.X)
    assert [mb.m.masked_tiny_applies(mb.valid is not None and mb.valid.ndim == 1) for mb in members] == \
        [True, True, True, False, False, True] and flags == [False] * n

    def single_epoch(mb, sigma, first):
        return mb.t.batch_epoch(sigma, first) if mb.valid is None else mb.t.batch_epoch_masked(sigma, first, mb.valid)

    # the exact epoch, then a local one
    for first, base in ((True, 3.0), (False, 2.4)):
        sig = [base + 0.1 * k for k in range(n)]
        mse = ens.batch_epoch_masked(sig, first, valids)
        assert mse.shape == (n,) and mse.dtype == np.float32
        for k, mb in enumerate(members):
            assert beq(mse[k], np.float32(single_epoch(mb, sig[k], first))), ("epoch MSE", first, k)
            mb.check(("epoch", first, k))
    # schedules of different lengths, one of them empty
    for reset in (1, 0):
        per = [[3.0, 2.5, 2.0], [2.8, 2.2], [], [3.0, 2.0], [2.5, 2.0, 1.6], [3.0]]
        before = snapshot(members[2].m)
        mses = ens.batch_schedule_masked(per, valids, reset_bmu=reset)
        same_state(snapshot(members[2].m), before, "the member without epochs")
        for k, mb in enumerate(members):
            assert beq(mses[k], loop(mb.t, per[k], mb.valid, reset)), ("schedule MSEs", reset, k)
            mb.check(("schedule", reset, k))
    # a call right behind an asynchronous upload sees the new rows
    news = [mb.rows(200 + k) for k, mb in enumerate(members)]
    offs, total = [], 0
    for X in news:
        offs.append(total)
        total += X.size
    pin = capi.PinnedBuffer((total,))
    for X, o in zip(news, offs):
        pin.array[o:o + X.size] = X.reshape(-1)
    ens.upload_chunks_async(pin, offs, [mb.B for mb in members])
    mse = ens.batch_epoch_masked(2.0, True, valids)
    for k, mb in enumerate(members):
        mb.t.upload_chunk(news[k])
        assert beq(mse[k], np.float32(single_epoch(mb, 2.0, True))), ("behind the upload", k)
        mb.check(("behind the upload", k))
    ens.close()
    if stream is not None:
        stream.synchronize()
    pin.free()
    for mb in members:
        mb.close()


def test_ensemble_launch_rounds():
    """a masked member past VSOM_SCHEDULE_MAX_EPOCHS beside a short one, each on its own stream"""
    a = Member(2, 2, 1, po.STANDARD, 3, 71, False)
    b = Member(3, 3, 2, po.MEDIAN, 4, 72, False)
    a.valid = np.array([[1], [0], [1]], np.uint8)
    b.valid = np.array([1, 1], np.uint8)
    for mb in (a, b):
        mb.m.upload_chunk(mb.X)
        mb.t.upload_chunk(mb.X)
    ens = vsom_amd.Ensemble([a.m, b.m])
    per = [[1.5] * (MAXE + 2), [1.5, 1.2]]
    mses = ens.batch_schedule_masked(per, [a.valid, b.valid])
    for k, mb in enumerate((a, b)):
        assert beq(mses[k], loop(mb.t, per[k], mb.valid, 1)), k
        mb.check(("rounds", k))
    ens.close()
    a.close()
    b.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_member_untouched():
    L = capi.lib()
    u8p, dp, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_float)
    W, H, J, B = 10, 10, 9, 20
    X, init = rows_and_map(W, H, J, B)
    valid = random_mask(B, J, 3).astype(np.uint8)
    sig = (C.c_double * 2)(3.0, 2.0)
    out = (C.c_float * 2)()

    def refused(code, word):
        assert code == -1, word
        assert word in L.vsom_last_error().decode(), (word, L.vsom_last_error().decode())

    # the single call
    a, a_t = context(po.STANDARD, W, H, J, init), context(po.STANDARD, W, H, J, init)
    vp = valid.ctypes.data_as(u8p)
    refused(L.vsom_batch_schedule_masked(None, sig, 2, 1, vp, 0, out), "null context")
    refused(L.vsom_batch_schedule_masked(a._h, sig, 2, 1, vp, 0, out), "no chunk")
    a.upload_chunk(X)
    a_t.upload_chunk(X)
    a.batch_epoch(3.0, True)
    a_t.batch_epoch(3.0, True)
    before = snapshot(a)
    refused(L.vsom_batch_schedule_masked(a._h, sig, 2, 1, None, 0, out), "valid_host")
    refused(L.vsom_batch_schedule_masked(a._h, None, 2, 1, vp, 0, out), "null sigma")
    refused(L.vsom_batch_schedule_masked(a._h, sig, 2, 1, vp, 0, None), "mse_out")
    assert L.vsom_batch_schedule_masked(a._h, None, 0, 1, None, 0, None) == 0      # nothing to do: no array is read
    for mode in (capi.UPDATE_FMA, capi.UPDATE_FMA_SIGMA):
        a.set_update_mode(mode)
        refused(L.vsom_batch_schedule_masked(a._h, sig, 2, 1, vp, 0, out), "strict")
    a.set_update_mode(capi.UPDATE_STRICT)
    same_state(snapshot(a), before, "after the single refusals")

    # ensembles: a masked CLR member, a masked custom member, a member without a chunk, a contracted member
    Xc = gen.correlated(B, 6, 5)
    clr, clr_t = (context(po.CLR, 7, 7, 6, gen.random_map(49, po.length(po.CLR, 6), seed=9), Xc) for _ in range(2))
    d, r = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=d, residual_len=r)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    empty = context(po.STANDARD, W, H, J, init)
    b, b_t = context(po.STANDARD, W, H, J, init, X), context(po.STANDARD, W, H, J, init, X)
    vc, vu = np.ones((B, 6), np.uint8), np.ones((10, 5), np.uint8)

    def untouched(ctxs, befores, what):
        for k, (ctx, snap) in enumerate(zip(ctxs, befores)):
            same_state(snapshot(ctx), snap, (what, k))

    for others, valids, word in (((clr,), (vc,), "member 2: CLR"), ((cu,), (vu,), "member 2: a custom context"),
                                 ((empty,), (valid[:0],), "member 2: no chunk loaded")):
        ens = vsom_amd.Ensemble([a, b, *others])
        befores = [snapshot(a), snapshot(b)] + ([snapshot(clr)] if others[0] is clr else [])
        for call in (lambda: ens.batch_epoch_masked(2.0, True, [valid, None, *valids]),
                     lambda: ens.batch_schedule_masked([3.0, 2.0], [valid, None, *valids])):
            with pytest.raises(capi.VsomError, match=word):
                call()
            untouched([a, b] + ([clr] if others[0] is clr else []), befores, word)
        ens.close()
    ens = vsom_amd.Ensemble([a, b, clr])
    befores = [snapshot(a), snapshot(b), snapshot(clr)]
    b.set_update_mode(capi.UPDATE_FMA)
    with pytest.raises(capi.VsomError, match="member 1: .*strict"):
        ens.batch_schedule_masked([3.0, 2.0], [valid, valid, None])
    with pytest.raises(capi.VsomError, match="member 1: .*strict"):
        ens.batch_epoch_masked(2.0, True, [valid, valid, None])
    b.set_update_mode(capi.UPDATE_STRICT)
    refused(L.vsom_ensemble_batch_epoch_masked(ens._h, (C.c_double * 3)(2.0, 2.0, 2.0), 1, None, None, None), "valid_host")
    sigs = (dp * 3)(*[C.cast(sig, dp)] * 3)
    outs = (fp * 3)(*[C.cast(out, fp)] * 3)
    cnt = (C.c_size_t * 3)(2, 2, 2)
    refused(L.vsom_ensemble_batch_schedule_masked(ens._h, sigs, cnt, 1, None, None, outs), "valid_host")
    refused(L.vsom_ensemble_batch_schedule_masked(None, sigs, cnt, 1, None, None, outs), "null ensemble")
    vps = (u8p * 3)(vp, vp, u8p())
    refused(L.vsom_ensemble_batch_schedule_masked(ens._h, sigs, None, 1, vps, None, outs), "epochs")
    refused(L.vsom_ensemble_batch_schedule_masked(ens._h, None, cnt, 1, vps, None, outs), "member 0")
    untouched([a, b, clr], befores, "after the ensemble refusals")
    # the next legal call gives the reference result: a masked and plain, a masked plain CLR member beside them
    mses = ens.batch_schedule_masked([3.0, 2.0], [valid, None, None])
    for k, (m, t, v) in enumerate(((a, a_t, valid), (b, b_t, None), (clr, clr_t, None))):
        assert beq(mses[k], loop(t, [3.0, 2.0], v, 1)), k
        same_state(snapshot(m), snapshot(t), ("after the refusals", k))
    ens.close()
    cu.bmu_batch()
    for ctx in (a, a_t, b, b_t, clr, clr_t, cu, empty):
        ctx.close()


def test_a_chunk_staged_ahead_is_refused():
    """a map whose batch epoch frees the staged rows early, so that a prefetch stages the next chunk over them (as
    tests/test_gpu_masked_train.py): the masked schedule must not read those rows"""
    W = H = 48
    J = 196
    xs = [gen.mnist_like(1100, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    big = context(po.STANDARD, W, H, J, init, xs[0])
    pb = capi.PinnedBuffer(xs[1].shape)
    pb.array[...] = xs[1]
    Xs, inits = rows_and_map(10, 10, 9, 20)
    small = context(po.STANDARD, 10, 10, 9, inits, Xs)
    ens = vsom_amd.Ensemble([small, big])
    big.batch_epoch_async(10.0, True)
    big.prefetch_chunk(pb.array)         # staged beside the chains of chunk 0
    before = snapshot(small)
    ones = np.ones(J, np.uint8)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        big.batch_schedule_masked([8.0], ones)
    with pytest.raises(capi.VsomError, match="member 1: the next chunk is staged ahead"):
        ens.batch_schedule_masked([3.0, 2.0], [np.ones(9, np.uint8), ones])
    with pytest.raises(capi.VsomError, match="member 1: the next chunk is staged ahead"):
        ens.batch_epoch_masked(3.0, True, [np.ones(9, np.uint8), ones])
    same_state(snapshot(small), before, "the small member")
    big.commit_chunk()
    mses = ens.batch_schedule_masked([[3.0, 2.0], [12.0]], [np.ones(9, np.uint8), ones])
    assert len(mses[0]) == 2 and len(mses[1]) == 1
    ens.close()
    for ctx in (big, small):
        ctx.close()
    pb.free()


# ---- 8. bookkeeping ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", KINDS)
def test_what_follows_the_schedule_follows_the_loop(tr):
    """get_state, a plain batch_epoch and get_state again give the same bits behind the schedule and behind the loop (the
    sigma mode at its default); the chunk and S stay; two runs give identical bits"""
    W, H, J, B = 10, 10, 9, 20
    assert "VSOM_SIGMA_MODE" not in os.environ
    X, init = rows_and_map(W, H, J, B)
    valid = random_mask(B, J, 11)
    S = gen.random_map(W * H, J, seed=77)
    runs = []
    for how in ("schedule", "schedule", "loop"):
        ctx = vsom_amd.Context(W, H, J, tr)
        ctx.set_state(map=init, S=S)
        ctx.upload_chunk(X)
        chunk = ctx.device_ptr(capi.BUF_CHUNK)
        mse = ctx.batch_schedule_masked(SIGMAS, valid, reset_bmu=False) if how == "schedule" else loop(ctx, SIGMAS, valid, 0)
        first = snapshot(ctx)
        follow = ctx.batch_epoch(1.9, False)
        second = snapshot(ctx)
        assert ctx.device_ptr(capi.BUF_CHUNK) == chunk and ctx.chunk_size == B
        assert beq(ctx.bmu_masked(np.ones(J, np.uint8), fill=True)["fill"], X)      # the staged rows, read back
        assert beq(first["S"], S) and beq(second["S"], S)
        runs.append((mse, first, np.float32(follow), second))
        ctx.close()
    for other, what in ((runs[1], "second run"), (runs[2], "loop")):
        assert beq(runs[0][0], other[0]) and beq(runs[0][2], other[2]), what
        same_state(runs[0][1], other[1], (what, "behind the schedule"))
        same_state(runs[0][3], other[3], (what, "behind the following epoch"))


# ---- 9. mirrors ----------------------------------------------------------------------------------------------------------
def test_som_mirror_equals_train_batch_som_masked():
    W, H, J, B = 10, 10, 9, 20
    X, init = rows_and_map(W, H, J, B)
    valid = random_mask(B, J, 9)
    X = poisoned(X, valid)
    out = []
    for name in ("trainBatchSomResidentMasked", "trainBatchSomMasked"):
        s = vs.Som(W, H, J)
        s._verbose = False
        s.setState(map=init)
        ds = ValidDataSet(X, valid, B)
        getattr(s, name)(ds, 8, 3.0, 0.2)             # sigma 3 .. 1.1, then 0.9 < 1: six epochs run
        out.append((s.state(), list(s.metrics.MeanSquaredError), ds.lastBMU.copy()))
        s.close()
    (sa, ma, la), (sb, mb, lb) = out
    for k in sa:
        assert beq(sa[k], sb[k]), k
    assert beq(np.array(ma, np.float32), np.array(mb, np.float32)) and ma[5] > 0 and ma[6:] == [0.0, 0.0]
    assert (la == lb).all()


def test_cpp_mirror_driver():
    exe = os.path.join(HOST, "host_resident_masked_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_resident_masked_test ok" in res.stdout
