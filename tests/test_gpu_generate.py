"""GPU: vsom_generate_batch / vsom_decode_nodes -- Som::autoEncoder's records (Som.cpp:568-623) sampled on the device.  Units
are held bit for bit against vsom_bmd_batch's draws (PER_ROW: the same rows and uniforms; AS_WRITTEN: the chunk's last row,
once per uniform), records against the float64 restatement of tests/generate_ref.py within the bound of include/vsom_hip.h,
and bit for bit on the cases that carry no tolerance."""
import ctypes
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
import generate_ref as ref  # noqa: E402
from generate_ref import NO_UNIT, beq  # noqa: E402

pytestmark = pytest.mark.gpu
AW, PR = capi.GENERATE_AS_WRITTEN, capi.GENERATE_PER_ROW
WORST = {"ratio": 0.0, "where": "", "values": 0}


def make(tr, W, H, J, B, seed=0, spread=0.3):
    """a context whose model rows lie within `spread` of one centre, rows around the same centre (every row has mass on
    every node), sigma in [0.05, 1), hits 0..4; returns (ctx, state as vsom_get_state returns it, X)"""
    rng = np.random.default_rng(seed)
    ctx = vsom_amd.Context(W, H, J, tr)
    N, D = ctx.n_nodes, ctx.depth
    centre = rng.uniform(0.5, 1.5, J).astype(np.float32)
    X = (centre + rng.uniform(-spread, spread, (B, J))).astype(np.float32)
    if tr == po.CLR:
        M = rng.uniform(-spread, spread, (N, D)).astype(np.float32)
    else:
        M = (centre + rng.uniform(-spread, spread, (N, D))).astype(np.float32)
    S = rng.uniform(0.05, 1.0, (N, D)).astype(np.float32)
    hits = rng.integers(0, 5, N).astype(np.uint64)
    hits[N - 1] = 4
    ctx.set_state(map=M, sigma=S, hits=hits)
    ctx.upload_chunk(X)
    return ctx, ctx.get_state(), X


def logits(rng, n, C):
    L = rng.uniform(0.001, 0.999, (n, C))
    L[0, 0] = 0.5
    return L


def bmd_last_row(ctx, mh, u):
    """vsom_bmd_batch on range [B - 1, B), called once per uniform"""
    B = ctx.chunk_size
    return np.array([ctx.restricted_bmd(mh, B - 1, B, u=u[i:i + 1])["draw"][0] for i in range(len(u))], np.uint64)


def check_records(st, units, L, got, where):
    want, zs = ref.decode(st["map"], st["sigma"], units, L)
    ok, worst = ref.within(got, want, zs)
    print(f"{where}: worst error {worst:.3f} of its bound over {got.size} values")
    if worst > WORST["ratio"]:
        WORST.update(ratio=worst, where=where)
    WORST["values"] += got.size
    assert ok, (where, worst)


def snapshot(ctx):
    st = ctx.get_state()
    return [st[k] for k in ("map", "sigma", "S", "weight", "hits")] + [ctx.get_last_bmu(), ctx.get_sqres()]


def same_snapshot(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


SHAPES = [(tr, 5, 4, J) for tr in (po.STANDARD, po.MEDIAN) for J in (1, 3, 13, 70)] + \
         [(po.STANDARD, 9, 29, 6), (po.MEDIAN, 9, 29, 6), (po.CLR, 5, 4, 2), (po.CLR, 5, 4, 4)]


# ---- 1. both rules against vsom_bmd_batch and the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", SHAPES, ids=[f"{'SMC'[s[0]]}{s[1]}x{s[2]}x{s[3]}" for s in SHAPES])
def test_units_and_records(tr, W, H, J):
    for B in (1, 7):
        ctx, st, X = make(tr, W, H, J, B, seed=J + B)
        C = min(J, ctx.depth)
        assert C == J
        rng = np.random.default_rng(B)
        u, L = rng.random(B), logits(rng, B, C)
        ctx.bmu_batch()                                  # lastBMU / sqres hold something to leave alone
        before = snapshot(ctx)
        for mh in (0, 2):
            tag = f"{'SMC'[tr]} {W}x{H}x{J} B={B} min_hits={mh}"
            per = ctx.generate(mh, u, L, PR)
            assert per["unit"].dtype == np.uint64 and per["record"].shape == (B, C)
            assert (per["unit"] == ctx.restricted_bmd(mh, u=u)["draw"]).all(), tag
            aw = ctx.generate(mh, u, L, AW)
            assert (aw["unit"] == bmd_last_row(ctx, mh, u)).all(), tag
            assert (per["unit"] < ctx.n_nodes).all() and (aw["unit"] < ctx.n_nodes).all(), tag   # the rows have mass
            assert (st["hits"][per["unit"].astype(int)] >= mh).all()
            for name, rep in (("per_row", per), ("as_written", aw)):
                check_records(st, rep["unit"], L, rep["record"], f"{tag} {name}")
                # L = 0.5: the unit's value, bit for bit
                assert rep["record"][0, 0] == np.float64(st["map"][int(rep["unit"][0]), 0])
                assert beq(ctx.decode_nodes(rep["unit"], L), rep["record"]), tag
            if B > 4:                                    # a range inside the chunk; AS_WRITTEN still draws from row B - 1
                for rule, whole in ((PR, per), (AW, aw)):
                    part = ctx.generate(mh, u[2:6], L[2:6], rule, 2, 6)
                    assert (part["unit"] == whole["unit"][2:6]).all() and beq(part["record"], whole["record"][2:6]), tag
        assert same_snapshot(before, snapshot(ctx))
        assert ctx.chunk_size == B and (ctx.bmu_batch()[0] == before[5]).all()      # the chunk itself
        ctx.close()


# ---- 2. draws placed in the row pass's chunks (N = 261 > 256) -----------------------------------------------------------------
@pytest.mark.parametrize("tr", [po.STANDARD, po.MEDIAN])
def test_draws_in_every_chunk(tr):
    W, H, J, B = 9, 29, 5, 3
    ctx, st, X = make(tr, W, H, J, B, seed=5, spread=0.2)
    N = ctx.n_nodes
    assert N == 261
    hits = np.full(N, 3, np.uint64)
    ctx.set_state(hits=hits)
    top = 1.0 - 2.0 ** -53
    cum = np.cumsum(ref.bmd_p(ctx.distances_row(B - 1), hits, 1))
    mid = lambda c, i: float((c[i - 1] + c[i]) / 2 / c[-1])          # noqa: E731  (the middle of node i's interval)
    # chunk 0, chunk 1, node 260, the largest double below 1, 0, and the two sides of the chunk boundary
    u = np.array([mid(cum, 100), mid(cum, 257), mid(cum, 260), top, 0.0, mid(cum, 255), mid(cum, 256)])
    want = np.array([100, 257, 260, 260, 0, 255, 256], np.uint64)
    L = logits(np.random.default_rng(2), len(u), J)
    # AS_WRITTEN takes one uniform per row of the range: a chunk of len(u) rows, every one of them X[B - 1]
    ctx.upload_chunk(np.repeat(X[B - 1:B], len(u), axis=0))
    got = ctx.generate(1, u, L, AW)
    assert (got["unit"] == want).all(), (got["unit"], want)
    assert (got["unit"] == bmd_last_row(ctx, 1, u)).all()
    per = ctx.generate(1, u, L, PR)                      # every row is that row: the same draws
    assert (per["unit"] == want).all() and beq(per["record"], got["record"])
    check_records(st, got["unit"], L, got["record"], f"{'SMC'[tr]} chunks")
    # the second chunk without mass: the largest double below 1 ends on the last node with mass, in chunk 0
    hits[250:] = 0
    ctx.set_state(hits=hits)
    cum = np.cumsum(ref.bmd_p(ctx.distances_row(0), hits, 1))
    u2 = np.array([top, mid(cum, 100)])
    for rule in (AW, PR):
        g = ctx.generate(1, u2, L[:2], rule, 0, 2)
        assert (g["unit"] == ctx.restricted_bmd(1, 0, 2, u=u2)["draw"]).all()
        assert g["unit"][0] == 249 and g["unit"][1] == 100
    # mass in the second chunk only
    hits[:] = 0
    hits[258] = 1
    ctx.set_state(hits=hits)
    for rule in (AW, PR):
        g = ctx.generate(1, u, L, rule)
        assert (g["unit"] == 258).all()
    ctx.close()


# ---- 3. the cases without a tolerance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, J", [(po.STANDARD, 13), (po.MEDIAN, 70), (po.CLR, 2), (po.CLR, 4)])
def test_exact_cases(tr, J):
    W, H, B = 5, 4, 7
    ctx, st, X = make(tr, W, H, J, B, seed=9)
    N, C = ctx.n_nodes, min(J, ctx.depth)
    M, S = st["map"].copy(), st["sigma"].copy()
    S[3] = 0                                             # a unit without spread
    S[5, C - 1] = np.nan                                 # NaN and inf in the state of units the draws can take
    S[6, 0] = np.inf
    hits = np.zeros(N, np.uint64)
    rng = np.random.default_rng(4)
    L = rng.uniform(0.01, 0.99, (B, C))
    L[1] = 0.5
    L[2, 0], L[2, C - 1] = 0.0, 1.0
    L[4, 0], L[4, C - 1] = -0.25, 1.5
    u = rng.random(B)
    for k in (3, 5, 6, 8):                               # exactly one eligible node: every draw takes it
        hits[:] = 0
        hits[k] = 2
        ctx.set_state(map=M, sigma=S, hits=hits)
        for rule in (AW, PR):
            g = ctx.generate(1, u, L, rule)
            assert (g["unit"] == k).all()
            want, zs = ref.decode(M, S, g["unit"], L)
            m = M[k, :C].astype(np.float64)
            if k in (3, 8):
                assert beq(g["record"][1], m)                                # L = 0.5 (0 * inf and 0 * NaN are NaN)
            if k == 3:
                assert beq(g["record"][[0, 3, 5, 6]], np.tile(m, (4, 1)))    # s = 0, a finite g
                assert np.isnan(g["record"][2, [0, C - 1]]).all()            # s = 0 beside an infinite g
            if k == 8:
                assert g["record"][2, 0] == -np.inf and g["record"][2, C - 1] == np.inf
            assert np.isnan(g["record"][4, [0, C - 1]]).all()
            if k == 5:
                assert np.isnan(g["record"][[0, 3], C - 1]).all()
            if k == 6:
                assert np.isinf(g["record"][0, 0])
            ok, _ = ref.within(g["record"], want, zs)                        # inf and NaN where the restatement has them
            assert ok
    # NaN and inf in the map: an eligible unit holding one has no distance, so they reach a record through decode_nodes
    Mn = M.copy()
    Mn[2, 0], Mn[2, C - 1], Mn[4, 0] = np.nan, np.inf, -np.inf
    ctx.set_state(map=Mn)
    nodes = np.array([2, 4, 2, 3, 8, 4, 5], np.uint64)
    rec = ctx.decode_nodes(nodes, L)
    want, zs = ref.decode(Mn, S, nodes, L)
    assert np.isnan(rec[0, 0]) and np.isnan(rec[2, 0]) and rec[1, 0] == -np.inf
    if C > 1:
        assert rec[0, C - 1] == np.inf
    ok, _ = ref.within(rec, want, zs)
    assert ok
    assert beq(rec[3], Mn[3, :C].astype(np.float64))                         # s = 0
    # ... and a masked node holding them changes nothing
    hits[:] = 2
    hits[[2, 4]] = 0
    ctx.set_state(map=M, hits=hits)
    base = ctx.generate(1, u, L, PR)
    ctx.set_state(map=Mn)
    ctx.upload_chunk(X)
    again = ctx.generate(1, u, L, PR)
    assert (base["unit"] == again["unit"]).all() and beq(base["record"], again["record"])
    assert (base["unit"] < N).all()
    ctx.close()


# ---- 4. rows without mass ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", [(po.STANDARD, 5, 4, 3), (po.MEDIAN, 9, 29, 13), (po.CLR, 5, 4, 4)])
def test_rows_without_mass(tr, W, H, J):
    B = 7
    ctx, st, X = make(tr, W, H, J, B, seed=2)
    C = min(J, ctx.depth)
    rng = np.random.default_rng(8)
    u, L = rng.random(B), logits(rng, B, C)

    def none(rep, rows):
        assert (rep["unit"][rows] == NO_UNIT).all()
        assert (np.ascontiguousarray(rep["record"][rows]).view(np.uint64) == ref.QNAN_BITS).all()

    # min_hits above every hit
    for rule in (AW, PR):
        none(ctx.generate(5, u, L, rule), slice(None))
    # rows 1e3 away from the map: every exp underflows
    far = X.copy()
    far[[1, 4, 6]] += np.float32(1e3)
    ctx.upload_chunk(far)
    per = ctx.generate(0, u, L, PR)
    assert (per["unit"] == ctx.restricted_bmd(0, u=u)["draw"]).all()
    none(per, [1, 4, 6])
    near = [0, 2, 3, 5]
    assert (per["unit"][near] < ctx.n_nodes).all()
    check_records(st, per["unit"], L, per["record"], f"{'SMC'[tr]} far rows")
    none(ctx.generate(0, u, L, AW), slice(None))                             # the last row is one of them
    aw = ctx.generate(0, u[:6], L[:6], AW, 0, 6)                             # ... whatever the range
    none(aw, slice(None))
    ctx.upload_chunk(far[:6])                                                # the last row has mass again
    aw = ctx.generate(0, u[:6], L[:6], AW)
    assert (aw["unit"] < ctx.n_nodes).all() and (aw["unit"] == bmd_last_row(ctx, 0, u[:6])).all()
    ctx.close()


# ---- 5. slices -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", [(po.STANDARD, 9, 29, 13), (po.CLR, 5, 4, 4)])
def test_row_slices(monkeypatch, tr, W, H, J):
    """a slice forced to 100 rows (VSOM_GENERATE_SLICE_ROWS, read at every call): 333 rows cross it three times"""
    B = 333
    ctx, st, X = make(tr, W, H, J, B, seed=6)
    C = min(J, ctx.depth)
    rng = np.random.default_rng(3)
    u, L = rng.random(B), logits(rng, B, C)
    nodes = rng.integers(0, ctx.n_nodes, B).astype(np.uint64)
    whole = {rule: ctx.generate(2, u, L, rule) for rule in (AW, PR)}
    dec = ctx.decode_nodes(nodes, L)
    monkeypatch.setenv("VSOM_GENERATE_SLICE_ROWS", "100")
    sliced = {rule: ctx.generate(2, u, L, rule) for rule in (AW, PR)}
    part = {rule: ctx.generate(2, u[50:301], L[50:301], rule, 50, 301) for rule in (AW, PR)}
    dec_sliced = ctx.decode_nodes(nodes, L)
    monkeypatch.delenv("VSOM_GENERATE_SLICE_ROWS")
    assert (whole[PR]["unit"] == ctx.restricted_bmd(2, u=u)["draw"]).all()
    assert len(np.unique(whole[AW]["unit"])) > 3 and (whole[AW]["unit"][:20] == bmd_last_row(ctx, 2, u[:20])).all()
    for rule in (AW, PR):
        assert (sliced[rule]["unit"] == whole[rule]["unit"]).all() and beq(sliced[rule]["record"], whole[rule]["record"])
        assert (part[rule]["unit"] == whole[rule]["unit"][50:301]).all()
        assert beq(part[rule]["record"], whole[rule]["record"][50:301])
        check_records(st, whole[rule]["unit"], L, whole[rule]["record"], f"{'SMC'[tr]} B=333 rule {rule}")
    assert beq(dec, dec_sliced)
    check_records(st, nodes, L, dec, f"{'SMC'[tr]} decode_nodes")
    ctx.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    W, H, J, B = 6, 5, 7, 20
    ctx, st, X = make(po.STANDARD, W, H, J, B, seed=1)
    fresh = vsom_amd.Context(W, H, J)
    lib = capi.lib()
    dp, up = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)
    rng = np.random.default_rng(1)
    u, L = rng.random(B), logits(rng, B, J)
    unit = np.full(B, 7, np.uint64)
    record = np.full((B, J), -1.0)
    out = capi.GenerateOut(unit.ctypes.data_as(up), record.ctypes.data_as(dp))
    pu, pl = u.ctypes.data_as(dp), L.ctypes.data_as(dp)

    def rc(r0=0, r1=B, rule=PR, uu=pu, ll=pl, o=out, h=None):
        return lib.vsom_generate_batch(h or ctx._h, 1, rule, r0, r1, uu, ll, None if o is None else ctypes.byref(o))

    assert rc(h=fresh._h, r1=0) == -1 and "no chunk" in lib.vsom_last_error().decode()
    fresh.close()
    good = ctx.generate(1, u, L)
    bad_u = [u.copy() for _ in range(4)]
    bad_u[0][3], bad_u[1][B - 1], bad_u[2][0], bad_u[3][5] = np.nan, 1.0, -1e-300, np.inf
    cases = [dict(r0=5, r1=4), dict(r1=B + 1), dict(r0=B + 1, r1=B + 2), dict(rule=2), dict(rule=-1), dict(uu=None),
             dict(ll=None), dict(o=None)] + [dict(uu=b.ctypes.data_as(dp)) for b in bad_u]
    for kw in cases:
        assert rc(**kw) == -1, kw
        assert (unit == 7).all() and (record == -1.0).all(), kw              # nothing was written
        again = ctx.generate(1, u, L)
        assert (again["unit"] == good["unit"]).all() and beq(again["record"], good["record"]), kw
    assert rc(r0=3, r1=3) == 0 and (unit == 7).all() and (record == -1.0).all()      # an empty range
    assert rc() == 0 and (unit == good["unit"]).all() and beq(record, good["record"])
    assert rc(o=capi.GenerateOut()) == 0                                             # no output at all
    only_unit = capi.GenerateOut(unit.ctypes.data_as(up), None)
    unit[:] = 7
    assert rc(o=only_unit) == 0 and (unit == good["unit"]).all()

    # vsom_decode_nodes
    nodes = rng.integers(0, W * H, B).astype(np.uint64)
    rec = np.full((B, J), -1.0)

    def rd(n=nodes, count=B, ll=pl, r=rec):
        return lib.vsom_decode_nodes(ctx._h, None if n is None else n.ctypes.data_as(up), count, ll,
                                     None if r is None else r.ctypes.data_as(dp))

    bad = nodes.copy()
    bad[B - 1] = W * H
    worse = nodes.copy()
    worse[0] = NO_UNIT
    for kw in (dict(n=None), dict(n=bad), dict(n=worse), dict(ll=None), dict(r=None)):
        assert rd(**kw) == -1, kw
        assert (rec == -1.0).all()
    assert rd(count=0) == 0 and rd(n=None, count=0) == 0 and (rec == -1.0).all()
    assert rd() == 0 and beq(rec, ctx.decode_nodes(nodes, L))
    check_records(st, nodes, L, rec, "decode_nodes")
    with pytest.raises(ValueError):
        ctx.decode_nodes(bad, L)
    # no chunk is needed
    fresh = vsom_amd.Context(W, H, J)
    fresh.set_state(map=st["map"], sigma=st["sigma"])
    assert beq(fresh.decode_nodes(nodes, L), rec)
    fresh.close()
    ctx.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    cols = min(5, cu.depth)
    with pytest.raises(capi.VsomError, match="vsom_generate_batch"):
        cu.generate(0, np.zeros(10), np.full((10, cols), 0.5))
    with pytest.raises(capi.VsomError, match="vsom_decode_nodes"):
        cu.decode_nodes([0], np.full((1, cols), 0.5))
    cu.bmu_batch()
    cu.close()

    # no columns: CLR of one column has depth J (J - 1) = 0
    try:
        c0 = capi.Context(3, 3, 1, capi.CLR)
    except capi.VsomError:
        c0 = None                                        # (the library does not build such a context at all)
    if c0 is not None:
        assert c0.depth == 0
        one = np.full(2, 0.5)
        assert lib.vsom_generate_batch(c0._h, 0, PR, 0, 2, one.ctypes.data_as(dp), one.ctypes.data_as(dp),
                                       ctypes.byref(capi.GenerateOut())) == -1
        assert "no columns" in lib.vsom_last_error().decode()
        assert lib.vsom_decode_nodes(c0._h, np.zeros(1, np.uint64).ctypes.data_as(up), 1, one.ctypes.data_as(dp),
                                     one.ctypes.data_as(dp)) == -1
        c0.close()

    # a chunk staged ahead (as tests/test_gpu_bmd_batch.py): refused until it is committed; decode_nodes reads no rows
    W = H = 48
    J = 196
    xs = [gen.mnist_like(1100, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    big = vsom_amd.Context(W, H, J)
    pin = capi.PinnedBuffer(xs[1].shape)
    pin.array[...] = xs[1]
    big.set_state(map=init)
    big.upload_chunk(xs[0])
    big.batch_epoch_async(10.0, True)
    big.prefetch_chunk(pin.array)
    u4, L4 = np.full(4, 0.5), np.full((4, J), 0.25)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        big.generate(0, u4, L4, PR, 0, 4)
    dec = big.decode_nodes([0, 1, 2, 3], L4)
    big.commit_chunk()
    got = big.generate(0, u4, L4, PR, 0, 4)
    assert (got["unit"] == big.restricted_bmd(0, 0, 4, u=u4)["draw"]).all()
    st = big.get_state()
    check_records(st, np.arange(4, dtype=np.uint64), L4, dec, "decode beside a staged chunk")
    big.close()
    pin.free()


# ---- 7. the shared arena --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", [po.STANDARD, po.CLR])
def test_between_other_queries(tr):
    W, H, J, B = (9, 29, 13, 60) if tr == po.STANDARD else (5, 4, 4, 60)
    ctx, st, X = make(tr, W, H, J, B, seed=12)
    rng = np.random.default_rng(5)
    u, L = rng.random(B), logits(rng, B, J)
    nodes = rng.integers(0, ctx.n_nodes, 9).astype(np.uint64)

    def others():
        r = ctx.restricted_bmd(1, u=u, probs=True)
        k = ctx.bmu_topk(3)
        s = ctx.similarity(1, 2, delta=True)
        e = ctx.evaluate(np.ones(J), np.ones(J))
        d = ctx.distances_row(B - 1)
        return [r["norm"], r["draw"], r["prob"], k[0], k[1], s["bmu"], s["amax"], s["delta"], e["bsum"], d]

    def mine():
        a, p = ctx.generate(1, u, L, AW), ctx.generate(1, u, L, PR)
        return [a["unit"], a["record"], p["unit"], p["record"], ctx.decode_nodes(nodes, L[:9])]

    same = lambda x, y: all(a.tobytes() == b.tobytes() for a, b in zip(x, y))     # noqa: E731
    o1, m1 = others(), mine()
    o2, m2 = others(), mine()
    assert same(o1, o2) and same(m1, m2)
    fresh, _, _ = make(tr, W, H, J, B, seed=12)          # a context that has run nothing else
    a, p = fresh.generate(1, u, L, AW), fresh.generate(1, u, L, PR)
    assert same(m1[:4], [a["unit"], a["record"], p["unit"], p["record"]])
    fresh.close()
    ctx.close()


# ---- 8. timers ------------------------------------------------------------------------------------------------------------------
def test_timers():
    ctx, st, X = make(po.STANDARD, 5, 4, 3, 7, seed=3)
    rng = np.random.default_rng(1)
    u, L = rng.random(7), logits(rng, 7, 3)
    ctx.enable_timing(True)
    ctx.get_timing()
    ctx.generate(0, u, L, PR)
    t = ctx.get_timing()
    assert t["bmu"][1] == 1 and t["finish"][1] == 1 and all(t[k][1] == 0 for k in ("stage", "cw", "update", "online", "sigma"))
    ctx.generate(0, u, L, AW)
    t = ctx.get_timing()
    assert t["bmu"][1] == 2 and t["finish"][1] == 1      # the last row's distribution, the draws
    ctx.decode_nodes([1, 2], L[:2])
    t = ctx.get_timing()
    assert t["bmu"][1] == 0 and t["finish"][1] == 1
    ctx.close()


# ---- 9. Som mirror --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", [(po.STANDARD, 6, 5, 9), (po.MEDIAN, 9, 29, 13), (po.CLR, 5, 4, 4)])
def test_som_mirror(tr, W, H, J):
    B = 20
    ctx, st, X = make(tr, W, H, J, B, seed=7)
    rng = np.random.default_rng(2)
    u, L = rng.random(B), logits(rng, B, J)
    want = {rule: ctx.generate(2, u, L, rule) for rule in (AW, PR)}
    ctx.close()
    t = {po.STANDARD: vs.Transformation.Standard(), po.MEDIAN: vs.Transformation.StandardMedianEstimator(),
         po.CLR: vs.Transformation.CombinatorialLinearRegression()}[tr]
    s = vs.Som(W, H, st["map"].shape[1], t)
    s.setState(map=st["map"], sigma=st["sigma"], hits=st["hits"])
    for per_row, rule in ((True, PR), (False, AW)):
        got = s.generateRows(X, 2, u, L, perRow=per_row)
        assert (got["unit"] == want[rule]["unit"]).all() and beq(got["record"], want[rule]["record"])
    assert beq(s.decodeUnits(want[PR]["unit"], L), want[PR]["record"])
    empty = s.generateRows(X[:0], 2, u[:0], L[:0])
    assert empty["unit"].shape == (0,) and empty["record"].shape == (0, J)
    # autoEncoder: as written, the generator's numbers, deterministic under a seed
    unit, record = s.autoEncoder(X, 2, seed=11)
    g = np.random.default_rng(11)
    ua = g.random(B)
    La = g.integers(0, 1000, (B, J)).astype(np.float64) / 1000.0
    s.ctx.upload_chunk(X)
    ref_aw = s.ctx.generate(2, ua, La, AW)
    assert (unit == ref_aw["unit"]).all() and beq(record, ref_aw["record"]) and (unit < W * H).all()
    unit2, record2 = s.autoEncoder(X, 2, seed=11)
    assert (unit == unit2).all() and beq(record, record2)
    # no mass: node 0, as the reference's discrete_distribution returns then
    unit0, record0 = s.autoEncoder(X, 5, seed=11)
    assert (unit0 == 0).all() and beq(record0, s.decodeUnits(np.zeros(B, np.uint64), La))
    check_records(st, unit0, La, record0, f"{'SMC'[tr]} autoEncoder, node 0")
    s.close()


def test_zz_report():
    """the largest error, in units of its bound, over every tolerance check of this run"""
    print(f"vsom_generate_batch: worst error {WORST['ratio']:.3f} of the bound over {WORST['values']} values, "
          f"at {WORST['where']}")
