"""GPU: caller-defined Transformation hooks as device source (vsom_create_custom, csrc/vsom_custom.hip).

Standard, Median and CLR restated through the hook contract train batch and online on ragged, non-square maps and must
give the oracle's bits for map, sigmaMap, SMap, weightMap, bmuHits, lastBMU and the MSE (NaN == NaN).  A hook that is
not a built-in must give the bits of the host path for custom hooks (host/src/vsom_custom.cpp) driven with the same
hook as C++ lambdas (host_custom_device_test).  Refused calls return VSOM_ERR_INVALID and leave the context usable."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gen
import custom_hooks as hooks
from vsom_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"standard": po.STANDARD, "median": po.MEDIAN, "clr": po.CLR}


def beq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def custom_ctx(kind, W, H, J):
    depth, rlen = hooks.shape(kind, J)
    return capi.Context(W, H, J, capi.CUSTOM, source=hooks.SOURCES[kind], depth=depth, residual_len=rlen)


def assert_state(ctx, o, what):
    st = ctx.get_state()
    for k, ref in (("map", o.map), ("sigma", o.sigma), ("S", o.S), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], ref), f"{what}: {k} differs from the oracle"


def init_state(kind, W, H, J, seed):
    o = po.OracleSom(W, H, J, KINDS[kind])
    init = gen.random_map(W * H, o.depth, seed)
    if kind == "clr":
        init = (init * np.float32(0.2)).astype(np.float32)
    sig = (np.abs(gen.random_map(W * H, o.depth, seed + 1)) * np.float32(0.5)).astype(np.float32)
    sig[:, ::3] = 0.0                      # exercises the 1e-5 floor of the distance
    o.set_state(map=init, sigma=sig)
    return o, init, sig


# (kind, W, H, J, B, sigmas of the epochs)
BATCH = [
    ("standard", 7, 5, 3, 61, (2.5, 1.7, 1.0)),
    ("standard", 12, 9, 794, 100, (3.0, 1.5)),
    ("median", 9, 6, 17, 77, (2.0, 1.2)),
    ("median", 5, 11, 33, 40, (0.8, 0.5)),
    ("clr", 6, 7, 6, 50, (2.2, 1.3)),
    ("clr", 4, 5, 9, 33, (1.5,)),
]


@pytest.mark.parametrize("kind,W,H,J,B,sigmas", BATCH)
def test_batch_matches_oracle(kind, W, H, J, B, sigmas):
    o, init, sig = init_state(kind, W, H, J, 5 + J)
    X = gen.blobs(B, J, 4, 1, 2 + J)
    ctx = custom_ctx(kind, W, H, J)
    ctx.set_state(map=init, sigma=sig)
    lbo = np.zeros(B, np.uint64)
    for e, sigma in enumerate(sigmas):
        ctx.upload_chunk(X)
        if e:
            ctx.set_last_bmu(lbo)
        mse_o = o.batch_epoch(X, lbo, sigma, e == 0)
        mse = ctx.batch_epoch(sigma, e == 0)
        assert beq(ctx.get_last_bmu(), lbo), f"epoch {e}: lastBMU"
        assert np.float32(mse) == mse_o or (np.isnan(mse) and np.isnan(mse_o)), (e, mse, mse_o)
        assert_state(ctx, o, f"epoch {e}")
    ctx.close()


# (kind, W, H, J, B, decay, sigma)
ONLINE = [
    ("standard", 10, 10, 9, 40, po.EXPONENTIAL, 2.2),
    ("standard", 10, 7, 9, 40, po.INVERSE_PROPORTIONAL, 0.7),
    ("standard", 8, 6, 794, 12, po.EXPONENTIAL, 2.5),
    ("median", 9, 9, 17, 30, po.INVERSE_PROPORTIONAL, 3.0),
    ("median", 11, 6, 17, 30, po.EXPONENTIAL, 1.0),
    ("clr", 7, 7, 6, 25, po.EXPONENTIAL, 2.0),
    ("clr", 7, 5, 5, 25, po.INVERSE_PROPORTIONAL, 0.9),
]


@pytest.mark.parametrize("kind,W,H,J,B,fn,sigma", ONLINE)
def test_online_matches_oracle(kind, W, H, J, B, fn, sigma):
    o, init, sig = init_state(kind, W, H, J, 9 + J)
    X = gen.blobs(B, J, 3, 4, 5 + J)
    ctx = custom_ctx(kind, W, H, J)
    ctx.set_state(map=init, sigma=sig)
    lbo = np.zeros(B, np.uint64)
    run_o = 0.0
    for c in range(2):                     # two chunks of one epoch: one running MSE
        run_o = o.train_online_chunk(X, lbo, 0.3, sigma, fn, mse_start=0.0 if c == 0 else float(run_o))
        ctx.upload_chunk(X)
        if c:
            ctx.set_last_bmu(lbo_prev)
        run = ctx.train_online_chunk(0.3, sigma, fn, first_chunk=(c == 0))
        lbo_prev = lbo.copy()
        assert beq(ctx.get_last_bmu(), lbo), f"chunk {c}: lastBMU"
        assert np.float32(run) == run_o, (c, run, run_o)
        assert_state(ctx, o, f"chunk {c}")
    ctx.close()


@pytest.mark.parametrize("kind,fn,sigma", [("standard", po.EXPONENTIAL, 1.8), ("clr", po.INVERSE_PROPORTIONAL, 0.8)])
def test_train_single_and_searches_match_oracle(kind, fn, sigma):
    W, H, J = 6, 8, 7
    o, init, sig = init_state(kind, W, H, J, 31)
    X = gen.blobs(12, J, 3, 7, 8)
    ctx = custom_ctx(kind, W, H, J)
    ctx.set_state(map=init, sigma=sig)
    last_o = last_g = 0
    for v in X:
        bo, ro, do, last_o = o.train_single(v, 0.2, sigma, last_o, fn)
        bg, rg, dg, last_g = ctx.train_single(v, 0.2, sigma, last_g, fn)
        assert (bo, last_o) == (bg, last_g)
        assert beq(rg, ro) and np.float32(dg) == do
    assert_state(ctx, o, "train_single")
    v = X[3]
    assert ctx.find_bmu(v)[0] == o.find_bmu(v)
    assert ctx.find_local_bmu(v, 5)[0] == o.find_local_bmu(v, 5)
    assert np.float32(ctx.dist_single(v, 7)) == np.float32(o.dist(7, v))
    ctx.upload_chunk(X)
    idx, dist = ctx.bmu_batch()
    assert [int(i) for i in idx] == [o.find_bmu(x) for x in X]
    assert beq(dist, np.array([o.dist(int(i), x) for i, x in zip(idx, X)], np.float32))
    nodes = np.array([0, 5, 47, 13], np.uint64)
    rows = np.array([0, 11, 2, 2], np.uint64)
    assert beq(ctx.distances(nodes, rows), np.array([o.dist(int(n), X[int(r)]) for n, r in zip(nodes, rows)], np.float32))
    ctx.close()


def test_non_builtin_hook_matches_host_path():
    exe = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host", "host_custom_device_test")
    if not os.path.exists(exe):
        import __graft_entry__
        __graft_entry__.build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "custom device parity ok" in r.stdout


def test_python_som_trains_custom_source():
    from vsom_amd import som
    J, W, H = 9, 6, 5
    X = gen.blobs(40, J, 3, 2, 3)
    t = som.Transformation.Custom(hooks.MEDIAN, J, J)
    s = som.Som(W, H, som.ArrayDataSet(X), t)
    o = po.OracleSom(W, H, J, po.MEDIAN)
    init = gen.random_map(W * H, J, 4)
    s.setState(map=init)
    o.set_state(map=init)
    data = som.ArrayDataSet(X)
    s.trainBatchSom(data, 2, 2.0, 0.3)
    o.train_batch(X, [0, 40], 2, 2.0, 0.3)
    st = s.state()
    assert beq(st["map"], o.map) and beq(st["sigma"], o.sigma) and beq(st["weight"], o.weight)
    s.close()


def test_refused_calls_leave_the_context_usable():
    W, H, J = 5, 4, 6
    ctx = custom_ctx("standard", W, H, J)
    L, h = capi.lib(), ctx._h
    X = gen.blobs(10, J, 2, 1, 1)
    ctx.upload_chunk(X)
    v = X[0].copy()
    f = (C.c_float * (W * H))()
    u = C.c_uint64()
    n1 = np.zeros(1, np.uint64)
    refused = [
        L.vsom_set_update_mode(h, capi.UPDATE_FMA),
        L.vsom_set_column_compaction(h, 10),
        L.vsom_set_row_dedupe(h, 0.0),
        L.vsom_bmu_restricted_batch(h, 1, None, None),
        L.vsom_distances_row(h, 0, f),
        L.vsom_distances_raw(h, capi._u(n1), capi._u(n1), 1, 1, f),
        L.vsom_find_restricted_bmu(h, capi._f(v), 1, C.byref(u), None),
        L.vsom_distances_single(h, capi._f(v), f),
        L.vsom_batch_phase1_async(h, 0, 10, 1),
        L.vsom_batch_finish_async(h),
        L.vsom_batch_phase2_async(h, 2.0, 0, W * H),
        L.vsom_set_chunk_device(h, None, 0),
        L.vsom_get_shortlist_stats(h, (C.c_uint32 * 4)()),
    ]
    assert refused == [-1] * len(refused)
    assert "custom" in L.vsom_last_error().decode()
    assert ctx.residual_len == J
    o, init, sig = init_state("standard", W, H, J, 3)
    ctx.set_state(map=init, sigma=sig)
    ctx.upload_chunk(X)
    lbo = np.zeros(10, np.uint64)
    mse = ctx.batch_epoch(1.5, True)
    assert np.float32(mse) == o.batch_epoch(X, lbo, 1.5, True)
    assert_state(ctx, o, "after refusals")
    ctx.close()


def test_compile_error_on_create():
    with pytest.raises(capi.VsomError, match="does not compile"):
        capi.Context(4, 4, 3, capi.CUSTOM, source="__device__ float vsom_compare(", depth=3, residual_len=3)
