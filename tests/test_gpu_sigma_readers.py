"""GPU: who materialises a pending sigmaMap (include/vsom_hip.h, vsom_set_sigma_mode).  A VSOM_SIGMA_LAZY and a
VSOM_SIGMA_EAGER context go through the same calls on a 40x40x300 map (the lane = node chain kernels); after an epoch
whose sigmaMap the LAZY one left pending -- asserted through vsom_sigma_stats -- ONE reader runs on both and must return
the same bits, and leave the same state, as on the EAGER one, whose state after the epoch equals the oracle's.
Then the call orders that overwrite what a pending sigmaMap is made from while it is pending, and AUTO's rule."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import gen
import vsom_amd
from vsom_amd import capi
from vsom_amd import dist
from oracle import pyoracle as po
from test_gpu_sigma_deferred import W, H, J, _same, sparse_rows, dense_rows

pytestmark = pytest.mark.gpu
THREADS = max(1, min(64, po.max_threads()))
N = W * H
B = 77
SIGMA = 6.0
INIT = gen.random_map(N, J, 42) * np.float32(100)
XA, XB, XBIG = sparse_rows(B, 3), sparse_rows(B, 4), sparse_rows(200, 5)
_oracle = {}


def oracle_after(key, epochs):
    """the oracle after `epochs` = [(rows, sigma, is_first)] from INIT, computed once per key"""
    if key not in _oracle:
        orc = po.OracleSom(W, H, J, po.STANDARD)
        orc.set_state(map=INIT)
        for X, sigma, first in epochs:
            orc.batch_epoch(X, np.zeros(X.shape[0], np.uint64), sigma, first, nthreads=THREADS)
        _oracle[key] = {"map": orc.map.copy(), "sigma": orc.sigma.copy(), "weight": orc.weight.copy(), "hits": orc.hits.copy()}
    return _oracle[key]


def make(sigma_mode, compaction=1):
    ctx = vsom_amd.Context(W, H, J, capi.STANDARD)
    ctx.set_sigma_mode(sigma_mode)
    ctx.set_column_compaction(compaction)
    ctx.set_state(map=INIT)
    return ctx


def epoch(ctx, X, sigma=SIGMA, first=True):
    ctx.upload_chunk(X)
    return ctx.batch_epoch(sigma, first)


def pair_after_epoch(compaction=1, X=XA):
    lazy, eager = make(capi.SIGMA_LAZY, compaction), make(capi.SIGMA_EAGER, compaction)
    for c in (lazy, eager):
        epoch(c, X)
    s = lazy.sigma_stats()
    assert s["deferred"] == 1 and s["pending"] and s["materialised"] == 0, s
    assert eager.sigma_stats()["deferred"] == 0
    return lazy, eager


def states_equal(lazy, eager, oracle=None):
    a, b = lazy.get_state(S=False), eager.get_state(S=False)
    for k in ("map", "sigma", "weight", "hits"):
        assert _same(a[k], b[k]), k
        if oracle is not None:
            assert _same(b[k], oracle[k]), ("oracle", k)


def same_result(a, b):
    if isinstance(a, dict):
        for k in a:
            if a[k] is not None:
                assert same_result(a[k], b[k]), k
        return True
    if isinstance(a, (tuple, list)):
        return all(same_result(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
    return _same(a, b)


def _device_sigma(ctx):
    ptr = ctx.device_ptr(capi.BUF_SIGMA)          # materialises: the rows are current for work enqueued behind this call
    ctx.synchronize()
    rows = dist.device_tensor(ptr, (N, ctx.pitch), torch.float32, torch.device("cuda", 0))
    return rows[:, :J].cpu().numpy().copy()


_rs = np.random.RandomState(9)
_U, _L = _rs.rand(B), _rs.rand(B, J) * 0.98 + 0.01
_NODES = _rs.randint(0, N, size=64).astype(np.uint64)
_ROWS = _rs.randint(0, B, size=64).astype(np.uint64)
_VALID = (_rs.rand(B, J) < 0.8)

READERS = {
    "get_state": lambda c: c.get_state(S=False),
    "evaluate": lambda c: c.evaluate(np.ones(J, np.float32), np.ones(J, np.float32)),
    "similarity": lambda c: c.similarity(0, 2, delta=True),
    "generate": lambda c: c.generate(0, _U, _L),
    "umatrix": lambda c: c.umatrix(),
    "distances_raw": lambda c: c.distances_raw(_NODES, _ROWS, False),
    "online_chunk": lambda c: c.train_online_chunk(0.1, 3.0, capi.EXPONENTIAL),
    "set_state_sigma": lambda c: c.set_state(sigma=INIT),
    "partial_phase2": lambda c: (c.batch_phase2_async(SIGMA, 64, 640), c.synchronize()),
    "epoch_masked": lambda c: c.batch_epoch_masked(5.0, False, _VALID),
    "device_ptr": _device_sigma,
}


@pytest.mark.parametrize("reader", list(READERS))
def test_reader_materialises_a_pending_sigma(reader):
    lazy, eager = pair_after_epoch()
    got, ref = READERS[reader](lazy), READERS[reader](eager)
    s = lazy.sigma_stats()
    assert s["materialised"] == 1 and not s["pending"] and s["dropped"] == 0, (reader, s)
    if got is not None:
        assert same_result(got, ref), reader
    states_equal(lazy, eager, oracle_after("A", [(XA, SIGMA, True)]) if reader in ("get_state", "device_ptr", "umatrix") else None)
    lazy.close()
    eager.close()


def test_dense_rows_materialise_through_sigma_finalize():
    X = dense_rows(B, 3)
    lazy, eager = pair_after_epoch(compaction=-1, X=X)
    states_equal(lazy, eager, oracle_after("dense", [(X, SIGMA, True)]))
    assert lazy.sigma_stats()["materialised"] == 1
    lazy.close()
    eager.close()


def test_sigma_flush():
    lazy, eager = pair_after_epoch()
    lazy.sigma_flush()
    s = lazy.sigma_stats()
    assert s["materialised"] == 1 and not s["pending"]
    lazy.sigma_flush()                                        # nothing pending: a no-op
    assert lazy.sigma_stats()["materialised"] == 1
    states_equal(lazy, eager)
    lazy.close()
    eager.close()


def _order_commit(c):
    c.prefetch_chunk(XB)
    c.commit_chunk()                      # staging at commit: the live-column record of XB replaces XA's


def _order_stage_ahead(c):
    t = torch.from_numpy(XB).cuda()
    c.stage_next_device(t.data_ptr(), XB.shape[0])       # staged beside whatever runs, into the alternate record
    c.commit_chunk()
    c.synchronize()


def _order_update_mode(c):
    c.set_update_mode(capi.UPDATE_FMA)    # the pending epoch ran strict: its sigmaMap must be the strict one


def _order_larger_chunk(c):
    c.upload_chunk(XBIG)                  # the chunk buffers are reallocated; B no longer is the pending epoch's


ORDERS = {"commit_next_chunk": _order_commit, "stage_ahead": _order_stage_ahead, "set_update_mode": _order_update_mode,
          "upload_larger_chunk": _order_larger_chunk}


@pytest.mark.parametrize("order", list(ORDERS))
def test_inputs_overwritten_while_pending(order):
    lazy, eager = pair_after_epoch()
    for c in (lazy, eager):
        ORDERS[order](c)
    s = lazy.sigma_stats()
    assert s["pending"] and s["materialised"] == 0, (order, s)     # none of these calls reads sigmaMap
    states_equal(lazy, eager, oracle_after("A", [(XA, SIGMA, True)]))
    assert lazy.sigma_stats()["materialised"] == 1
    lazy.close()
    eager.close()


def test_larger_chunk_then_epoch_drops_and_defers_anew():
    lazy, eager = pair_after_epoch()
    for c in (lazy, eager):
        epoch(c, XBIG, 5.0, False)        # the chunk buffers, the transposed chunk and the (c,w) array all grow
    s = lazy.sigma_stats()
    assert s == {"deferred": 2, "dropped": 1, "materialised": 0, "pending": True}, s
    states_equal(lazy, eager, oracle_after("A+BIG", [(XA, SIGMA, True), (XBIG, 5.0, False)]))
    assert lazy.sigma_stats()["materialised"] == 1
    lazy.close()
    eager.close()


def test_empty_chunk_epoch_drops():
    lazy, eager = pair_after_epoch()
    empty = np.zeros((0, J), np.float32)
    for c in (lazy, eager):
        epoch(c, empty, 5.0, False)       # rewrites every row: zero vector, NaN sigmaMap, zero weight
    s = lazy.sigma_stats()
    assert s["dropped"] == 1 and not s["pending"] and s["materialised"] == 0, s
    states_equal(lazy, eager)
    st = lazy.get_state(S=False)
    assert (st["map"] == 0).all() and np.isnan(st["sigma"]).all() and (st["weight"] == 0).all()
    lazy.close()
    eager.close()


def test_auto_defers_only_after_two_unread_epochs():
    ctx, eager = make(capi.SIGMA_AUTO), make(capi.SIGMA_EAGER)
    chunks = (XA, XB)
    # a read after every epoch: never deferred
    for e in range(4):
        epoch(ctx, chunks[e % 2], SIGMA, e == 0)
        epoch(eager, chunks[e % 2], SIGMA, e == 0)
        ctx.get_state(S=False)
    assert ctx.sigma_stats()["deferred"] == 0
    # three unread epochs: the third is deferred (the MSE and lastBMU read-backs are not reads of sigmaMap)
    for e in range(3):
        for c in (ctx, eager):
            epoch(c, chunks[e % 2], SIGMA, False)
            c.get_last_bmu()
        assert ctx.sigma_stats()["deferred"] == (1 if e == 2 else 0), e
    assert ctx.sigma_stats()["pending"]
    states_equal(ctx, eager)                                  # the read materialises and resets the count
    s = ctx.sigma_stats()
    assert s["materialised"] == 1 and s["deferred"] == 1
    for e in range(2):
        for c in (ctx, eager):
            epoch(c, chunks[e % 2], SIGMA, False)
    assert ctx.sigma_stats()["deferred"] == 1                 # two epochs after the read: still eager
    for c in (ctx, eager):
        epoch(c, XA, SIGMA, False)
    assert ctx.sigma_stats()["deferred"] == 2
    states_equal(ctx, eager)
    ctx.close()
    eager.close()


# ---- the C++ mirror as a reader: Som::getMaxSigmaOfFeature -> refreshHost -> vsom_get_state (host/tests/host_api_test.cpp,
# mode `sigma`): a host copy cached after one epoch must be replaced, after three more epochs that never read sigmaMap, by
# the last epoch's -- materialised by that read -- and equal the oracle's
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "variational-self-organizing-maps_amd", "host")
MIRROR_ROWS = np.concatenate([sparse_rows(B, 3), sparse_rows(B, 4), sparse_rows(B, 5)])
MIRROR_OFF = [0, B, 2 * B, 3 * B]


def mirror_oracle():
    if "mirror" not in _oracle:
        o = po.OracleSom(W, H, J, po.STANDARD)
        o.random_initialize(5, 1.0)
        out = []
        for epochs in (1, 3):
            done, mse = o.train_batch(MIRROR_ROWS, MIRROR_OFF, epochs, 8.0, 0.2, nthreads=THREADS)
            assert done == epochs
            out.append({"map": o.map.copy(), "sigma": o.sigma.copy(), "weight": o.weight.copy(), "hits": o.hits.copy(),
                        "mse": np.asarray(mse, np.float32).copy()})
        _oracle["mirror"] = out
    return _oracle["mirror"]


@pytest.mark.parametrize("rows_path", ["dense_path", "compacted"])
def test_host_mirror_refreshes_its_cached_sigma(tmp_path, rows_path):
    from test_gpu_host_cpp import read_dump
    exe = os.path.join(HOST, "host_api_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    MIRROR_ROWS.tofile(str(tmp_path / "rows.f32"))
    ref = mirror_oracle()
    for mode in ("lazy", "eager"):
        out = tmp_path / mode
        out.mkdir()
        env = dict(os.environ, VSOM_SIGMA_MODE=mode)
        env.pop("VSOM_DEVICES", None)
        env["VSOM_COMPACT_MIN_ROWS"] = "1" if rows_path == "compacted" else "-1"
        res = subprocess.run([exe, "sigma", str(tmp_path / "rows.f32"), str(3 * B), str(J), str(B), str(W), str(H), "3", str(out)],
                             capture_output=True, text=True, timeout=120, env=env)
        assert res.returncode == 0, res.stdout[-400:] + res.stderr[-400:]
        rep = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
        if mode == "lazy":
            assert rep["deferred"] >= 4 and rep["pending_before_read"] == 1, rep
            assert rep["materialised"] == rep["materialised_before_read"] + 1, rep      # the read behind train() did it
        else:
            assert rep["deferred"] == 0 and rep["pending_before_read"] == 0 and rep["materialised"] == 0, rep
        assert rep["downloads_last"] > rep["downloads_first"] >= 1, rep                 # the cached copy was replaced
        for name, o in (("sigma_a.bin", ref[0]), ("sigma_b.bin", ref[1])):
            d = read_dump(str(out / name))
            for k in ("map", "sigma", "weight", "hits", "mse"):
                assert _same(d[k], o[k]), (mode, name, k)
    assert not _same(ref[0]["sigma"], ref[1]["sigma"])       # (a copy that was not refreshed could not have passed)
