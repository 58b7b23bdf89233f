"""GPU: vsom_train_online_chunk_masked -- the online chunk over the valid entries of the rows only.  Every comparison is on
the bits (NaN equals NaN; the untouched-column test compares the NaN payloads too), after every chunk, against
tests/online_masked_ref.py (pinned to the oracle by tests/test_online_masked_ref.py); all-valid masks also against
vsom_train_online_chunk_fetch on a twin context and against the oracle.

Shapes (tests/online_masked_cases.py): 7x5x9 (35 nodes: no multiple of a scan workgroup's 32; one packet block + a scalar
tail), 12x9x20 (a packet tail of 4), 16x16x33, 40x36x70 (45 scan workgroups: the 16 key slots wrap).  sigma 3.0 (window
clipped at the edges), 1.5, 1.0 (the one-launch step, walking from a given lastBMU), 0.3 (empty window)."""
import ctypes
import json
import math
import os
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
import online_masked_cases as oc  # noqa: E402
from online_masked_cases import ETA, beq, same  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
EXP, INV = po.EXPONENTIAL, po.INVERSE_PROPORTIONAL


def snapshot(ctx, mse, lb):
    st = ctx.get_state()
    return {"map": st["map"], "S": st["S"], "sigma": st["sigma"], "weight": st["weight"], "hits": st["hits"],
            "lastbmu": np.array(lb, np.uint64), "mse": np.array([mse], f32)}


def new_ctx(tr, W, H, J, M, S, **more):
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=M, S=S, **more)
    return ctx


def load(ctx, X, sigma, start):
    ctx.upload_chunk(np.ascontiguousarray(X, dtype=f32))
    if sigma <= 1:
        ctx.set_last_bmu(start)


def gpu_chunk(tr, W, H, J, M, S, X, valid, start, sigma, fn, state=None):
    """one masked chunk on a fresh context (state: more of its starting state); valid None: vsom_train_online_chunk_fetch"""
    ctx = new_ctx(tr, W, H, J, M, S, **(state or {}))
    load(ctx, X, sigma, start)
    if valid is None:
        mse, lb = ctx.train_online_chunk_fetch(ETA, sigma, fn)
    else:
        mse, lb = ctx.train_online_chunk_masked(ETA, sigma, fn, valid)
    assert (lb == ctx.get_last_bmu()).all()
    snap = snapshot(ctx, mse, lb)
    ctx.close()
    return snap


def ref_chunk(tr, W, H, J, M, S, X, valid, start, sigma, fn, state=None):
    r = oc.ref_new(tr, W, H, J, M, S)
    r.set_state(**(state or {}))
    lb = oc.start_of(sigma, start, X.shape[0])
    mse = r.train_chunk(X, valid, lb, ETA, sigma, fn)
    return r.snapshot(lb, mse)


# ---- 1. all-valid masks: the unmasked chunk, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("sigma", oc.SIGMAS)
@pytest.mark.parametrize("fn", oc.DECAYS)
@pytest.mark.parametrize("tr", oc.KINDS)
@pytest.mark.parametrize("shape", oc.SMALL)
def test_all_valid_is_the_unmasked_chunk(shape, tr, fn, sigma):
    W, H, J, B = shape
    X, M, valid, S, start = oc.data(W, H, J, B)
    want = oc.oracle_chunk(tr, W, H, J, M, S, X, oc.start_of(sigma, start, B), ETA, sigma, fn)
    same(gpu_chunk(tr, W, H, J, M, S, X, None, start, sigma, fn), want, "the twin's vsom_train_online_chunk_fetch")
    same(gpu_chunk(tr, W, H, J, M, S, X, np.ones((B, J), np.uint8), start, sigma, fn), want, "per-row mask")
    same(gpu_chunk(tr, W, H, J, M, S, X, np.ones(J, np.uint8), start, sigma, fn), want, "one_mask")


# ---- 2. random masks, NaN / inf at the invalid positions ---------------------------------------------------------------
@pytest.mark.parametrize("sigma", oc.SIGMAS)
@pytest.mark.parametrize("fn", oc.DECAYS)
@pytest.mark.parametrize("tr", oc.KINDS)
@pytest.mark.parametrize("shape", oc.SMALL)
def test_random_mask(shape, tr, fn, sigma):
    W, H, J, B = shape
    X, M, valid, S, start = oc.data(W, H, J, B)
    want = oc.reference(tr, W, H, J, B, fn, sigma)
    same(gpu_chunk(tr, W, H, J, M, S, oc.poisoned(X, valid), valid, start, sigma, fn), want, "poisoned rows")
    same(gpu_chunk(tr, W, H, J, M, S, np.where(valid, X, f32(0)), valid, start, sigma, fn), want, "zero-filled rows")


@pytest.mark.parametrize("fn", oc.DECAYS)
def test_random_mask_more_workgroups_than_key_slots(fn):
    W, H, J, B = oc.BIG
    X, M, valid, S, start = oc.data(W, H, J, B)
    want = oc.reference(po.STANDARD, W, H, J, B, fn, 3.0)
    same(gpu_chunk(po.STANDARD, W, H, J, M, S, oc.poisoned(X, valid), valid, start, 3.0, fn), want, "40x36x70")


@pytest.mark.parametrize("sigma", (3.0, 1.0))
@pytest.mark.parametrize("tr", oc.KINDS)
@pytest.mark.parametrize("B", (1, 2, 3, 37))
def test_chunk_sizes_across_the_sample_parity(B, tr, sigma):
    W, H, J = 7, 5, 9
    X, M, valid, S, start = oc.data(W, H, J, B, seed=20 + B)
    Xp = oc.poisoned(X, valid)
    want = ref_chunk(tr, W, H, J, M, S, Xp, valid, start, sigma, EXP)
    same(gpu_chunk(tr, W, H, J, M, S, Xp, valid, start, sigma, EXP), want, f"B = {B}")


# ---- 3. column masks, empty rows, a column valid in no row --------------------------------------------------------------
@pytest.mark.parametrize("sigma", (3.0, 1.0))
@pytest.mark.parametrize("tr", oc.KINDS)
def test_column_mask(tr, sigma):
    W, H, J, B = oc.SMALL[1]
    X, M, _, S, start = oc.data(W, H, J, B)
    cols = np.ones(J, np.uint8)
    cols[[0, 5, 8, 16, J - 1]] = 0       # in the packet blocks, the packet tail's last element
    Xp = oc.poisoned(X, cols != 0)
    for fn in oc.DECAYS:
        want = ref_chunk(tr, W, H, J, M, S, Xp, cols, start, sigma, fn)
        same(gpu_chunk(tr, W, H, J, M, S, Xp, cols, start, sigma, fn), want, "one_mask")
        same(gpu_chunk(tr, W, H, J, M, S, Xp, np.tile(cols, (B, 1)), start, sigma, fn), want, "the same mask per row")


@pytest.mark.parametrize("sigma", (3.0, 1.5, 1.0, 0.3))
def test_a_row_without_a_valid_column(sigma):
    W, H, J, B = oc.SMALL[0]
    X, M, valid, S, start = oc.data(W, H, J, B)
    valid = np.array(valid)
    empty = (0, 4, B - 1)
    valid[list(empty)] = False
    Xp = oc.poisoned(X, valid)
    for fn in oc.DECAYS:
        want = ref_chunk(po.STANDARD, W, H, J, M, S, Xp, valid, start, sigma, fn)
        got = gpu_chunk(po.STANDARD, W, H, J, M, S, Xp, valid, start, sigma, fn)
        same(got, want, "empty rows")
        for j in empty:                  # every distance is +0: node 0, or the walk stays where it starts
            assert got["lastbmu"][j] == (0 if sigma > 1 else start[j])
    # a chunk of empty rows only: map, SMap and sigmaMap keep their bits, the MSE is 0
    none = np.zeros((B, J), np.uint8)
    got = gpu_chunk(po.STANDARD, W, H, J, M, S, Xp, none, start, sigma, EXP)
    assert beq(got["map"], M) and beq(got["S"], S) and not got["sigma"].any() and got["mse"][0] == 0
    assert got["hits"].sum() == B
    assert (got["weight"] != 0).any() == (sigma >= 0.4)


def nan_payloads(shape, base):
    """distinct quiet-NaN payloads, one per element"""
    n = int(np.prod(shape))
    return (np.uint32(0x7FC00000) + np.uint32(base) + np.arange(n, dtype=np.uint32)).view(f32).reshape(shape)


@pytest.mark.parametrize("sigma", (3.0, 1.0))
@pytest.mark.parametrize("tr", oc.KINDS)
def test_a_column_valid_in_no_row_keeps_its_bits(tr, sigma):
    W, H, J, B = oc.SMALL[0]
    X, M, valid, S, start = oc.data(W, H, J, B)
    valid = np.array(valid)
    dead = (2, J - 1)                    # a packet-block column and the scalar tail
    valid[:, dead] = False
    M2, S2, G2 = np.array(M), np.array(S), np.zeros_like(M)
    for i, d in enumerate(dead):
        M2[:, d] = nan_payloads(W * H, 0x1000 * (3 * i + 1))
        S2[:, d] = nan_payloads(W * H, 0x1000 * (3 * i + 2))
        G2[:, d] = nan_payloads(W * H, 0x1000 * (3 * i + 3))
    Xp = oc.poisoned(X, valid)
    for fn in oc.DECAYS:
        got = gpu_chunk(tr, W, H, J, M2, S2, Xp, valid, start, sigma, fn, state={"sigma": G2})
        for k, before in (("map", M2), ("S", S2), ("sigma", G2)):
            for d in dead:
                assert (got[k][:, d].view(np.uint32) == before[:, d].view(np.uint32)).all(), (k, d)
        same(got, ref_chunk(tr, W, H, J, M2, S2, Xp, valid, start, sigma, fn, state={"sigma": G2}), "beside the dead columns")


# ---- 4. engineered searches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("twin_low", (True, False))
def test_rows_that_differ_at_invalid_columns_only_tie(twin_low):
    """two map rows equal at the sample's valid columns: the masked distances tie and the lower index wins"""
    W, H, J, B = 7, 5, 9, 1
    X, M, _, S, start = oc.data(W, H, J, B)
    valid = np.ones((1, J), np.uint8)
    valid[0, [1, 8]] = 0
    M = (np.array(M) + f32(2)).astype(f32)            # far from the sample
    a, b = (9, 23) if twin_low else (23, 9)           # a: the sample's own row; b: its twin
    M[a] = X[0]
    M[b] = X[0]
    M[b, [1, 8]] = X[0, [1, 8]] + f32(0.5)            # differs where the sample is invalid
    M[a, [1, 8]] = X[0, [1, 8]] - f32(0.25)
    got = gpu_chunk(po.STANDARD, W, H, J, M, S, X, valid, start, 3.0, EXP)
    assert got["lastbmu"][0] == min(a, b)
    same(got, ref_chunk(po.STANDARD, W, H, J, M, S, X, valid, start, 3.0, EXP), "tie")
    # without the mask the rows do not tie: the sample's own row at the valid AND invalid columns is neither of them
    plain = gpu_chunk(po.STANDARD, W, H, J, M, S, X, np.ones((1, J), np.uint8), start, 3.0, EXP)
    assert plain["lastbmu"][0] == a


def test_nan_in_node_0():
    W, H, J, B = oc.SMALL[0]
    X, M, valid, S, start = oc.data(W, H, J, B)
    valid = np.array(valid)
    valid[:, 3] = True
    valid[:, 6] = False
    Xp = oc.poisoned(X, valid)
    # at a valid column: d_0 is NaN and keeps node 0 for every sample
    M1 = np.array(M)
    M1[0, 3] = np.nan
    got = gpu_chunk(po.STANDARD, W, H, J, M1, S, Xp, valid, start, 3.0, EXP)
    assert not got["lastbmu"].any() and got["hits"][0] == B
    same(got, ref_chunk(po.STANDARD, W, H, J, M1, S, Xp, valid, start, 3.0, EXP), "NaN at a valid column of node 0")
    # at an invalid column: no effect on anything but that entry, which keeps its bits
    M2 = np.array(M)
    M2[0, 6] = np.nan
    got = gpu_chunk(po.STANDARD, W, H, J, M2, S, Xp, valid, start, 3.0, EXP)
    base = gpu_chunk(po.STANDARD, W, H, J, M, S, Xp, valid, start, 3.0, EXP)
    assert got["lastbmu"].any() and np.isnan(got["map"][0, 6])
    got["map"][0, 6] = base["map"][0, 6]
    same(got, base, "NaN at an invalid column of node 0")


# ---- 5. two chunks of one epoch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", (3.0, 1.0))
def test_two_chunks_continue_the_running_mse(sigma):
    W, H, J, B = oc.SMALL[1]
    X, M, valid, S, start = oc.data(W, H, J, B)
    X2, _, valid2, _, start2 = oc.data(W, H, J, 5, seed=31)
    ctx = new_ctx(po.MEDIAN, W, H, J, M, S)
    r = oc.ref_new(po.MEDIAN, W, H, J, M, S)
    mse_r = f32(0)
    for first, (Xc, vc, sc) in zip((True, False), ((X, valid, start), (X2, valid2, start2))):
        Xp = oc.poisoned(Xc, vc)
        load(ctx, Xp, sigma, sc)
        mse, lb = ctx.train_online_chunk_masked(ETA, sigma, INV, vc, first_chunk=first)
        lbr = oc.start_of(sigma, sc, Xc.shape[0])
        mse_r = r.train_chunk(Xp, vc, lbr, ETA, sigma, INV, mse_start=mse_r)
        same(snapshot(ctx, mse, lb), r.snapshot(lbr, mse_r), f"chunk first={first}")
        assert ctx.get_mse() == mse
    ctx.close()


# ---- 6. call orders -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (11, 4))           # odd and even: the chunk ends on either key parity
def test_masked_unmasked_masked(B):
    W, H, J = 16, 16, 33                         # (the unmasked chunk takes the per-sample loop: no tiny map)
    X, M, valid, S, start = oc.data(W, H, J, B, seed=40 + B)
    Xp = oc.poisoned(X, valid)
    Xz = np.where(valid, X, f32(0))
    ctx = new_ctx(po.STANDARD, W, H, J, M, S)
    r = oc.ref_new(po.STANDARD, W, H, J, M, S)
    ones = np.ones((B, J), bool)
    for step, (rows, mask) in enumerate(((Xp, valid), (Xz, None), (Xp, valid))):
        ctx.upload_chunk(rows)
        if mask is None:
            mse, lb = ctx.train_online_chunk_fetch(ETA, 3.0, EXP)
        else:
            mse, lb = ctx.train_online_chunk_masked(ETA, 3.0, EXP, mask)
        lbr = np.zeros(B, np.uint64)
        mse_r = r.train_chunk(rows, ones if mask is None else mask, lbr, ETA, 3.0, EXP)
        same(snapshot(ctx, mse, lb), r.snapshot(lbr, mse_r), f"step {step}")
    ctx.close()


def test_after_a_batch_epoch_with_a_deferred_sigma_map():
    W, H, J, B = 16, 16, 33, 37
    X, M, valid, S, start = oc.data(W, H, J, B)
    Xz = np.where(valid, X, f32(0))
    ctx = new_ctx(po.STANDARD, W, H, J, M, S)
    ctx.upload_chunk(Xz)
    ctx.batch_epoch(3.0, True)                   # (default sigma mode: sigmaMap may stay pending)
    o = po.OracleSom(W, H, J, po.STANDARD)
    o.set_state(map=M, S=S)
    o.batch_epoch(Xz, np.zeros(B, np.uint64), 3.0, True)
    r = oc.ref_new(po.STANDARD, W, H, J, o.map, o.S)
    r.set_state(sigma=o.sigma, weight=o.weight, hits=o.hits)
    batch_sigma = o.sigma.copy()
    o.close()
    mse, lb = ctx.train_online_chunk_masked(ETA, 1.5, EXP, valid)        # walks from nothing: sigma > 1
    lbr = np.zeros(B, np.uint64)
    mse_r = r.train_chunk(Xz, valid, lbr, ETA, 1.5, EXP)
    got = snapshot(ctx, mse, lb)
    same(got, r.snapshot(lbr, mse_r), "after the batch epoch")
    untouched = got["sigma"].view(np.uint32) == batch_sigma.view(np.uint32)
    assert untouched.any() and not untouched.all()       # outside the windows sigmaMap is the batch epoch's
    ctx.close()


def test_the_masked_search_sees_the_trained_map():
    W, H, J, B = oc.SMALL[1]
    X, M, valid, S, start = oc.data(W, H, J, B)
    Xp = oc.poisoned(X, valid)
    ctx = new_ctx(po.STANDARD, W, H, J, M, S)
    ctx.upload_chunk(Xp)
    ctx.train_online_chunk_masked(ETA, 3.0, EXP, valid)
    rep = ctx.bmu_masked(valid)
    ctx.close()
    want = oc.reference(po.STANDARD, W, H, J, B, EXP, 3.0)
    s = oc.ref_new(po.STANDARD, W, H, J, want["map"], want["S"])
    for j in range(B):
        s.valid = valid[j]
        bmu = s.find_bmu(Xp[j])
        assert rep["bmu"][j] == bmu and beq(rep["dist"][j], f32(s.dist(bmu, Xp[j]))), j


# ---- 7. search modes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", (3.0, 1.0))
def test_every_bmu_mode_gives_the_same_results(sigma):
    W, H, J, B = oc.SMALL[2]
    X, M, valid, S, start = oc.data(W, H, J, B)
    want = oc.reference(po.STANDARD, W, H, J, B, EXP, sigma)
    for mode in (capi.BMU_AUTO, capi.BMU_EXACT, capi.BMU_SHORTLIST):
        ctx = new_ctx(po.STANDARD, W, H, J, M, S)
        ctx.set_bmu_mode(mode)
        load(ctx, oc.poisoned(X, valid), sigma, start)
        mse, lb = ctx.train_online_chunk_masked(ETA, sigma, EXP, valid)
        same(snapshot(ctx, mse, lb), want, f"mode {mode}")
        assert ctx.online_search_stats()["samples"] == 0
        ctx.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    W, H, J, B = oc.SMALL[0]
    X, M, valid, S, start = oc.data(W, H, J, B)
    L = capi.lib()
    u8 = ctypes.POINTER(ctypes.c_uint8)
    vb = np.ascontiguousarray(valid, dtype=np.uint8)
    mse = ctypes.c_float()
    lbo = np.zeros(B, np.uint64)

    def rc(h, v=vb, fn=EXP):
        return L.vsom_train_online_chunk_masked(h, ETA, 3.0, fn, 1, None if v is None else v.ctypes.data_as(u8), 0,
                                                lbo.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(mse))

    def refused(code, word):
        assert code == -1, word
        assert word in L.vsom_last_error().decode(), (word, L.vsom_last_error().decode())

    ctx = new_ctx(po.STANDARD, W, H, J, M, S)
    h = ctx._h
    refused(rc(None), "null context")
    refused(rc(h), "no chunk")
    ctx.upload_chunk(np.array(X))
    before = snapshot(ctx, 0, ctx.get_last_bmu())
    refused(rc(h, v=None), "valid_host")
    refused(rc(h, fn=po.BATCHMAP), "Exponential or InverseProportional")
    refused(rc(h, fn=7), "Exponential or InverseProportional")
    ens = capi.Ensemble([ctx])
    refused(rc(h), "group or an ensemble")
    ens.close()
    same(snapshot(ctx, 0, ctx.get_last_bmu()), before, "after the refusals")
    ctx.close()
    # a following legal call succeeds and is right (a fresh context: an ensemble member stays one)
    want = oc.reference(po.STANDARD, W, H, J, B, EXP, 3.0)
    ctx = new_ctx(po.STANDARD, W, H, J, M, S)
    refused(rc(ctx._h), "no chunk")
    ctx.upload_chunk(oc.poisoned(X, valid))
    refused(rc(ctx._h, v=None), "valid_host")
    refused(rc(ctx._h, fn=po.BATCHMAP), "Exponential or InverseProportional")
    assert rc(ctx._h) == 0
    same(snapshot(ctx, mse.value, lbo), want, "the legal call after the refusals")
    ctx.close()

    # a group member
    grp = capi.Group(W, H, J, devices=[0, 0])
    refused(rc(grp.member(0)._h), "group or an ensemble")
    grp.close()

    # CLR contexts
    clr = vsom_amd.Context(4, 4, 5, po.CLR)
    Xc = (np.abs(gen.blobs(B, 5, 3, 1, 2)) + f32(0.5)).astype(f32)
    clr.upload_chunk(Xc)
    st = clr.get_state()
    with pytest.raises(capi.VsomError, match="CLR"):
        clr.train_online_chunk_masked(ETA, 3.0, EXP, np.ones((B, 5), np.uint8))
    st2 = clr.get_state()
    assert all(beq(st[k], st2[k]) for k in st)
    clr.train_online_chunk_fetch(ETA, 3.0, EXP)
    clr.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_train_online_chunk_masked"):
        cu.train_online_chunk_masked(ETA, 3.0, EXP, np.ones((10, 5), np.uint8))
    cu.bmu_batch()
    cu.close()


def test_a_chunk_staged_ahead_is_refused_until_it_is_committed():
    """as tests/test_gpu_masked_train.py: the next chunk is staged beside a running batch epoch"""
    W = H = 48
    J = 196
    xs = [gen.mnist_like(300, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * f32(100) + f32(100)).astype(f32)
    big, ref = vsom_amd.Context(W, H, J), vsom_amd.Context(W, H, J)
    pb = capi.PinnedBuffer(xs[1].shape)
    pb.array[...] = xs[1]
    for c in (big, ref):
        c.set_state(map=init)
        c.upload_chunk(xs[0])
        c.batch_epoch_async(10.0, True)
    big.prefetch_chunk(pb.array)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        big.train_online_chunk_masked(ETA, 3.0, EXP, np.ones(J, np.uint8))
    big.commit_chunk()
    ref.upload_chunk(xs[1])
    ref.set_bmu_mode(capi.BMU_EXACT)
    mse, lb = big.train_online_chunk_masked(ETA, 3.0, EXP, np.ones(J, np.uint8))
    mse_r, lb_r = ref.train_online_chunk_fetch(ETA, 3.0, EXP)
    same(snapshot(big, mse, lb), snapshot(ref, mse_r, lb_r), "after the commit")
    big.close()
    ref.close()
    pb.free()


# ---- 9. Som.trainBasicSomMasked -----------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("fn", oc.DECAYS)
def test_train_basic_som_masked(fn):
    W, H, J = 10, 10, 9
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ican_fixture.json")))
    X = np.array(fx["rows"], f32)
    assert X.shape[1] == J
    rows = X.shape[0]
    chunk = (rows + 1) // 2                      # two chunks per epoch
    rng = np.random.default_rng(8)
    valid = rng.random(X.shape) < 0.7
    Xp = oc.poisoned(X, valid)
    M = rng.random((W * H, J), dtype=f32)
    epochs, eta0, eta_decay, sigma0, sigma_decay = 5, 0.5, 0.1, 3.0, 0.4      # sigma 3, 2.01, 1.35, then the clamp at 1.0
    s = vs.Som(W, H, J)
    s._verbose = False
    s.setState(map=M)
    ds = ValidDataSet(Xp, valid, chunk)
    s.trainBasicSomMasked(ds, epochs, eta0, eta_decay, sigma0, sigma_decay, fn)
    got = s.state()
    metrics = np.array(s.metrics.MeanSquaredError[:epochs], f32)
    s.close()

    r = oc.ref_new(po.STANDARD, W, H, J, M, np.zeros_like(M))
    want_metrics, clamped = [], 0
    for e in range(epochs):
        eta = eta0 * math.exp(-eta_decay * float(e))
        sigma = sigma0 * math.exp(-sigma_decay * float(e))
        if sigma < 1.0:
            sigma, clamped = 1.0, clamped + 1
        mse = f32(0)
        for r0 in range(0, rows, chunk):
            lb = np.zeros(min(chunk, rows - r0), np.uint64)           # a load zeroes lastBMU
            mse = r.train_chunk(Xp[r0:r0 + chunk], valid[r0:r0 + chunk], lb, eta, sigma, fn, mse_start=mse)
        want_metrics.append(f32(mse / f32(2)))
    assert clamped >= 1
    for k, ref in (("map", r.map), ("sigma", r.sigma), ("weight", r.weight), ("hits", r.hits)):
        assert beq(got[k], ref), k
    assert beq(metrics, np.array(want_metrics, f32))
    assert (ds.lastBMU == lb).all()
