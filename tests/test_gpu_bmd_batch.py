"""GPU: vsom_bmd_batch -- Som::findRestrictedBmd (Som.cpp:457-487) for a range of chunk rows in one call, with the
normalising mass C of every row and one draw per row from caller-given uniforms.  Probabilities and norms are held
against the oracle (only exp may differ, by an ulp), draws against a numpy restatement of the rule on the oracle's
distances."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_hooks as hooks  # noqa: E402
import gen  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODRAW = np.uint64(0xFFFFFFFFFFFFFFFF)
RTOL = 1e-15
ULPS = []          # largest ulp distance of prob / norm from the oracle per case (printed at the end of the module)


def beq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        w = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return ((a.view(w) == b.view(w)) | (np.isnan(a) & np.isnan(b))).all()
    return (a == b).all()


def ulp_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    if not ok.any():
        return 0
    ia, ib = a[ok].view(np.int64), b[ok].view(np.int64)
    return int(np.abs(ia - ib).max())


def trained(W, H, J, tr, X, epochs=2, sigma=3.0):
    """a context after `epochs` batch epochs on X (hits from real epochs: some nodes have none) and an oracle holding
    the same map and hits"""
    ctx = vsom_amd.Context(W, H, J, tr)
    o = po.OracleSom(W, H, J, tr)
    ctx.set_state(map=gen.random_map(W * H, o.depth, seed=11))
    ctx.upload_chunk(X)
    for e in range(epochs):
        ctx.batch_epoch(sigma, e == 0)
    st = ctx.get_state()
    o.set_state(map=st["map"], hits=st["hits"])
    return ctx, o


def oracle_p(o, row, min_hits):
    """p_i of Som.cpp:468-479 from the oracle's distances"""
    d = np.array([o.dist(i, row) for i in range(o.n_nodes)], np.float64)
    p = np.exp(-d * d / 2)
    return np.where(o.hits >= np.uint64(min_hits), p, 0.0)


def np_draw(p, u):
    """the draw rule: smallest i with cum_i > u * C, else the last i with p_i > 0; none when C is 0 or not finite.
    Also returns the relative distance of t to the nearest cumulative boundary."""
    cum = np.cumsum(p)                       # sequential, in node order
    Cn = cum[-1]
    if not (Cn > 0 and np.isfinite(Cn)):
        return NODRAW, np.inf
    t = u * Cn
    above = np.nonzero(cum > t)[0]
    i = np.uint64(above[0]) if above.size else np.uint64(np.nonzero(p > 0)[0][-1])
    near = np.min(np.abs(cum - t)) / max(t, np.finfo(np.float64).tiny)
    return i, near


def check_rows(ctx, o, X, min_hits, rows, res, tag):
    """prob and norm of the listed rows against the oracle"""
    worst = 0
    for r in rows:
        ref = o.find_restricted_bmd(X[r], min_hits)
        got = res["prob"][r] if res["prob"] is not None else None
        p = oracle_p(o, X[r], min_hits)
        cn = np.cumsum(p)[-1]
        assert np.isclose(res["norm"][r], cn, rtol=RTOL, atol=0, equal_nan=True), (tag, r, res["norm"][r], cn)
        worst = max(worst, ulp_dist(res["norm"][r], cn))
        if got is None:
            continue
        assert (np.isnan(got) == np.isnan(ref)).all(), (tag, r)
        if cn > 0 and np.isfinite(cn):
            masked = o.hits < np.uint64(min_hits)
            assert (got[masked] == 0).all(), (tag, r)
        assert np.allclose(got, ref, rtol=RTOL, atol=0, equal_nan=True), (tag, r, np.abs(got - ref).max())
        worst = max(worst, ulp_dist(got, ref))
    ULPS.append((tag, worst))


def fixture_rows():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ican_fixture.json")))
    return np.array(fx["rows"], np.float32)


CASES = [   # (id, W, H, J, transform, rows)
    ("ican_10x10x9", 10, 10, 9, po.STANDARD, None),
    ("ns_7x11_d794", 7, 11, 794, po.STANDARD, 70),
    ("std_32x32x784", 32, 32, 784, po.STANDARD, 96),
    ("median_16x16x32", 16, 16, 32, po.MEDIAN, 150),
    ("clr_9x8_j7", 9, 8, 7, po.CLR, 60),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_parity_with_oracle(case):
    name, W, H, J, tr, B = case
    if B is None:
        X = fixture_rows()
    elif J == 784:      # pixel values scaled down: distances of order 1, so that the rows have mass to compare
        X = (gen.mnist_like(B, seed=5, dim=J) * np.float32(0.05 / 255)).astype(np.float32)
    else:
        X = gen.blobs(B, J, 4, 1, 2)
        if J > 100:
            X = (X * np.float32(0.05)).astype(np.float32)
    ctx, o = trained(W, H, J, tr, X, epochs=1)
    hmax = int(o.hits.max())
    assert (o.hits == 0).any() and hmax >= 3         # one epoch over fewer rows than nodes
    for mh in (0, 1, 3, hmax + 1):
        res = ctx.restricted_bmd(mh, probs=True)
        assert res["draw"] is None and res["prob"].shape == (X.shape[0], W * H)
        check_rows(ctx, o, X, mh, range(X.shape[0]), res, f"{name}/min_hits={mh}")
        if mh == 0:     # (most rows of the fixture lie far from every node of this map: C = 0 there, 0 / 0 = NaN)
            assert (res["norm"] > 0).any() and np.isfinite(res["norm"]).all()
        if mh == hmax + 1:
            assert (res["norm"] == 0).all() and np.isnan(res["prob"]).all()   # 0 / 0, as the reference divides
    ctx.close()


def test_draws_match_numpy_restatement():
    W, H, J, B = 16, 16, 32, 4096
    X = gen.blobs(B, J, 6, 3, 4, sigma=0.3)
    ctx, o = trained(W, H, J, po.STANDARD, X, epochs=1)
    u = np.random.default_rng(7).random(B)
    res = ctx.restricted_bmd(1, u=u)
    d = np.array([[o.dist(i, X[r]) for i in range(W * H)] for r in range(B)], np.float64)
    P = np.where(o.hits >= np.uint64(1), np.exp(-d * d / 2), 0.0)
    excluded = 0
    for r in range(B):
        want, near = np_draw(P[r], u[r])
        if near <= 1e-12:
            excluded += 1
            continue
        assert res["draw"][r] == want, (r, res["draw"][r], want)
    assert excluded <= 1
    assert np.allclose(res["norm"], np.cumsum(P, axis=1)[:, -1], rtol=RTOL, atol=0)
    ctx.close()


def _ctx_with(W, H, J, M, hits, X):
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=M, hits=hits)
    ctx.upload_chunk(X)
    return ctx


def test_engineered_draws():
    W, H, J = 5, 4, 6
    N = W * H
    rs = np.random.RandomState(3)
    x = rs.uniform(-1, 1, (1, J)).astype(np.float32)
    M = (x + rs.uniform(-0.3, 0.3, (N, J))).astype(np.float32)     # every node has mass of the same order
    hits = np.arange(N, dtype=np.uint64) % 3                        # 0, 1, 2, ...: nodes 0, 3, 6, ... masked at 1
    X = np.repeat(x, 8, axis=0)
    ctx = _ctx_with(W, H, J, M, hits, X)
    pos = np.nonzero(hits >= 1)[0]
    # u = 0: the first node with mass; u = nextafter(1, 0): the last
    r = ctx.restricted_bmd(1, u=np.zeros(8))
    assert (r["draw"] == pos[0]).all()
    r = ctx.restricted_bmd(1, u=np.full(8, np.nextafter(1.0, 0.0)))
    assert (r["draw"] == pos[-1]).all()
    # exactly one eligible node is always drawn
    h1 = np.zeros(N, np.uint64)
    h1[13] = 4
    ctx.set_state(hits=h1)
    r = ctx.restricted_bmd(1, u=np.random.default_rng(1).random(8), probs=True)
    assert (r["draw"] == 13).all() and (r["prob"][:, 13] == 1.0).all()
    # a masked node holding a NaN model row has no effect
    ctx.set_state(hits=hits)
    u = np.random.default_rng(2).random(8)
    base = ctx.restricted_bmd(1, u=u, probs=True)
    Mn = M.copy()
    Mn[3] = np.nan                                                  # hits[3] = 0: masked
    ctx.set_state(map=Mn)
    ctx.upload_chunk(X)
    r = ctx.restricted_bmd(1, u=u, probs=True)
    assert beq(r["norm"], base["norm"]) and beq(r["draw"], base["draw"]) and beq(r["prob"], base["prob"])
    # an eligible NaN: norm NaN, no draw
    r = ctx.restricted_bmd(0, u=u, probs=True)
    assert np.isnan(r["norm"]).all() and (r["draw"] == NODRAW).all() and np.isnan(r["prob"]).all()
    # min_hits above every count: no mass
    r = ctx.restricted_bmd(100, u=u)
    assert (r["norm"] == 0).all() and (r["draw"] == NODRAW).all()
    ctx.close()


def test_slices_concatenate_and_large_chunk():
    W, H, J, B = 12, 10, 20, 301
    X = gen.blobs(B, J, 5, 1, 2)
    ctx, o = trained(W, H, J, po.STANDARD, X)
    u = np.random.default_rng(3).random(B)
    full = ctx.restricted_bmd(1, u=u, probs=True)
    cuts = [0, 1, 64, 65, 200, 300, 301]
    parts = [ctx.restricted_bmd(1, a, b, u=u[a:b], probs=True) for a, b in zip(cuts[:-1], cuts[1:])]
    for k in ("norm", "draw", "prob"):
        assert beq(np.concatenate([p[k] for p in parts]), full[k]), k
    empty = ctx.restricted_bmd(1, 5, 5, u=u[5:5], probs=True)
    assert empty["norm"].size == 0 and empty["draw"].size == 0
    ctx.close()

    # 128 x 128 nodes: 2048 rows per slice (256 MiB of p), 5000 rows cross the bound twice
    W = H = 128
    J, B = 16, 5000
    X = gen.blobs(B, J, 8, 5, 6, sigma=0.5)
    ctx, o = trained(W, H, J, po.STANDARD, X, epochs=1, sigma=20.0)
    u = np.random.default_rng(4).random(B)
    res = ctx.restricted_bmd(1, u=u, probs=True)
    rows = [0, 1, 2047, 2048, 2049, 3000, 4095, 4096, 4097, 4999]
    check_rows(ctx, o, X, 1, rows, res, "128x128x16/5000 rows")
    for r in rows:
        want, near = np_draw(oracle_p(o, X[r], 1), u[r])
        assert near <= 1e-12 or res["draw"][r] == want, r
    ctx.close()


def test_read_only():
    W, H, J, B = 9, 7, 12, 120
    X = gen.blobs(B, J, 3, 1, 2)
    ctx = vsom_amd.Context(W, H, J)
    twin = vsom_amd.Context(W, H, J)
    init = gen.random_map(W * H, J, seed=4)
    for c in (ctx, twin):
        c.set_state(map=init)
        c.upload_chunk(X)
        c.batch_epoch(3.0, True)
    before = ctx.get_state(), ctx.get_last_bmu(), ctx.get_sqres()
    ctx.restricted_bmd(1, u=np.random.default_rng(5).random(B), probs=True)
    after = ctx.get_state(), ctx.get_last_bmu(), ctx.get_sqres()
    for k in ("map", "sigma", "S", "weight", "hits"):
        assert beq(before[0][k], after[0][k]), k
    assert beq(before[1], after[1]) and beq(before[2], after[2])
    m1, m2 = ctx.batch_epoch(2.0, False), twin.batch_epoch(2.0, False)
    assert beq(np.float32(m1), np.float32(m2))
    a, b = ctx.get_state(), twin.get_state()
    for k in ("map", "sigma", "S", "weight", "hits"):
        assert beq(a[k], b[k]), k
    assert beq(ctx.get_last_bmu(), twin.get_last_bmu())
    ctx.close()
    twin.close()


def _raw(ctx, min_hits, r0, r1, u, draw, norm):
    dp = C.POINTER(C.c_double)
    return capi.lib().vsom_bmd_batch(ctx._h, min_hits, r0, r1, None if u is None else u.ctypes.data_as(dp),
                                     None if draw is None else draw.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     None if norm is None else norm.ctypes.data_as(dp), None)


def test_refusals_leave_the_context_usable():
    W, H, J, B = 8, 6, 10, 60
    X = gen.blobs(B, J, 3, 1, 2)
    init = gen.random_map(W * H, J, seed=8)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    norm, draw = np.empty(B), np.empty(B, np.uint64)
    assert _raw(ctx, 0, 0, 0, None, None, norm) == -1                 # no chunk loaded
    ctx.upload_chunk(X)
    u = np.random.default_rng(6).random(B)
    bad = [(0, 5, 4, u, draw), (0, 0, B + 1, u, draw), (0, 0, B, None, draw)]
    for v in (np.nan, 1.0, -0.25, 2.0, np.inf):
        ub = u.copy()
        ub[17] = v
        bad.append((0, 0, B, ub, draw))
    for mh, r0, r1, uu, dd in bad:
        assert _raw(ctx, mh, r0, r1, uu, dd, norm) == -1, (r0, r1)
    # the context then trains as the oracle does
    o = po.OracleSom(W, H, J)
    o.set_state(map=init)
    lbo = np.zeros(B, np.uint64)
    for e in range(2):
        mse = ctx.batch_epoch(3.0, e == 0)
        mse_o = o.batch_epoch(X, lbo, 3.0, e == 0)
        assert np.float32(mse) == np.float32(mse_o)
    st = ctx.get_state()
    for k, ref in (("map", o.map), ("sigma", o.sigma), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], ref), k
    assert beq(ctx.get_last_bmu(), lbo)
    ctx.close()

    # custom contexts are refused
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_bmd_batch"):
        cu.restricted_bmd(0)
    cu.close()

    # a chunk staged ahead (as tests/test_gpu_ensemble.py): refused until it is committed
    W = H = 48
    J = 196
    xs = [gen.mnist_like(1100, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    big = vsom_amd.Context(W, H, J)
    pb = capi.PinnedBuffer(xs[1].shape)
    pb.array[...] = xs[1]
    big.set_state(map=init)
    big.upload_chunk(xs[0])
    big.batch_epoch_async(10.0, True)
    big.prefetch_chunk(pb.array)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        big.restricted_bmd(0)
    big.commit_chunk()
    res = big.restricted_bmd(0, 0, 4)
    assert res["norm"].shape == (4,)
    big.close()
    pb.free()


def test_group_member_equals_single_context():
    W, H, J, B = 14, 10, 24, 200
    X = gen.blobs(B, J, 4, 1, 2)
    init = gen.random_map(W * H, J, seed=42)
    g = vsom_amd.Group(W, H, J, capi.STANDARD, devices=[0, 0])
    g.set_state(map=init)
    g.upload_chunk(X)
    c = vsom_amd.Context(W, H, J, capi.STANDARD)
    c.set_state(map=init)
    c.upload_chunk(X)
    for e in range(2):
        g.batch_epoch(3.0, e == 0)
        c.batch_epoch(3.0, e == 0)
    g.synchronize()
    u = np.random.default_rng(9).random(B)
    want = c.restricted_bmd(1, u=u, probs=True)
    for rank in range(2):
        got = g.member(rank).restricted_bmd(1, u=u, probs=True)
        for k in ("norm", "draw", "prob"):
            assert beq(got[k], want[k]), (rank, k)
    c.close()
    g.close()


def test_python_som_methods():
    W, H, J, B = 10, 8, 9, 40
    X = gen.blobs(B, J, 3, 1, 2)
    ctx, o = trained(W, H, J, po.STANDARD, X)
    st = ctx.get_state()
    ctx.close()
    from vsom_amd import som as vs
    som = vs.Som(W, H, J)
    som.setState(map=st["map"], hits=st["hits"])
    p = som.findRestrictedBmd(X[3], minBmuHits=1)
    assert np.allclose(p, o.find_restricted_bmd(X[3], 1), rtol=RTOL, atol=0)
    u = np.random.default_rng(10).random(B)
    d = som.drawModelVectors(X, 1, u)
    for r in range(B):
        want, near = np_draw(oracle_p(o, X[r], 1), u[r])
        assert near <= 1e-12 or d[r] == want
    v = som.variationalAutoEncoder(X, 1, seed=3)
    assert v == int(som.drawModelVectors(X[-1:], 1, np.random.default_rng(3).random(1))[0])
    assert som.variationalAutoEncoder(X, 10 ** 9) == 0
    som.close()


def test_zz_report_ulps():
    """the largest ulp distances of prob / norm from the oracle seen above (only exp may differ)"""
    for tag, u in ULPS:
        print(f"bmd ulp {tag}: {u}")
