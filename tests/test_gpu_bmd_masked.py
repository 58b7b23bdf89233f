"""GPU: vsom_bmd_masked_batch -- Som::findRestrictedBmd over the VALID columns of every chunk row, with the normalising mass
and one draw per row.  With an all-valid mask everything is vsom_bmd_batch's bit for bit; under random masks prob and norm are
held against the float64 restatement on the oracle's masked distances (tests/bmd_masked_ref.py; only exp may differ, the
figure of tests/test_gpu_bmd_batch.py), the zero pattern exactly, the draws against the numpy rule except those
tests/test_bmd_masked_api.py counted as near a cumulative boundary (at most one per case).
Shapes: maps of 35 nodes (under one node tile), 135 (two tiles and a ragged one) and 272 (a second 256-node chunk of 16 nodes:
the draw's chunk search and re-walk run), J of 3 / 9 / 37 / 70, 70 rows (one 64-row tile and 6; no multiple of the 8 rows of
a row-pass workgroup), Standard and Median."""
import ctypes
import os
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bmd_masked_ref as ref  # noqa: E402
import custom_hooks as hooks  # noqa: E402
import gen  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
B = ref.B
RTOL = 1e-15
NODRAW = ref.NO_UNIT
KEYS = ("norm", "draw", "prob")
ULPS = []          # largest ulp distance of prob / norm from the restatement per case (printed at the end of the module)


def beq(a, b):
    """bitwise equality of arrays of one type; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        w = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return bool(((a.view(w) == b.view(w)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def same(a, b, what=None):
    for k in KEYS:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert beq(a[k], b[k]), (what, k)


def ulp_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    if not ok.any():
        return 0
    return int(np.abs(a[ok].view(np.int64) - b[ok].view(np.int64)).max())


def context(c, X=None):
    ctx = vsom_amd.Context(c["W"], c["H"], c["J"], c["tr"])
    ctx.set_state(map=c["M"], sigma=c["S"], hits=c["hits"])
    ctx.upload_chunk(c["X"] if X is None else X)
    return ctx


def teardown_module(module):
    for tag, worst in ULPS:
        print(f"[bmd_masked] {tag}: worst ulp distance of prob / norm {worst}")


# ---- 1. an all-valid mask is the unmasked call ------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", ref.SHAPES)
def test_all_valid_equals_restricted_bmd(tr, W, H, J):
    c = ref.case(tr, W, H, J)
    X = ref.unit_rows(B, J, 77)
    ctx = context(c, X)
    u = c["U"][:, 0]
    for min_hits in ref.MIN_HITS:
        want = ctx.restricted_bmd(min_hits, u=u, probs=True)
        assert (want["norm"] > 0).all() and (want["draw"] != NODRAW).all()
        same(ctx.restricted_bmd_masked(np.ones((B, J), np.uint8), min_hits, u=u, probs=True), want, ("rows", min_hits))
        same(ctx.restricted_bmd_masked(np.ones(J, np.uint8), min_hits, u=u, probs=True), want, ("column mask", min_hits))
    ctx.close()


# ---- 2. random masks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", ref.SHAPES)
def test_random_masks(tr, W, H, J):
    c = ref.case(tr, W, H, J)
    ctx = context(c)
    u = c["U"][:, 0]
    moved = 0
    for min_hits in ref.MIN_HITS:
        P, norm, prob, unit, near = ref.case_draws(c, min_hits)
        got = ctx.restricted_bmd_masked(c["valid"], min_hits, u=u, probs=True)
        worst = max(ulp_dist(got["norm"], norm), ulp_dist(got["prob"], prob))
        print(f"[bmd_masked] {tr}/{W}x{H}x{J}/min_hits={min_hits}: worst ulp distance {worst}")
        ULPS.append((f"{tr}/{W}x{H}x{J}/min_hits={min_hits}", worst))
        assert np.allclose(got["norm"], norm, rtol=RTOL, atol=0), np.abs(got["norm"] / norm - 1).max()
        assert np.allclose(got["prob"], prob, rtol=RTOL, atol=0), np.abs(got["prob"] - prob).max()
        zero = np.broadcast_to(c["hits"] < np.uint64(min_hits), prob.shape)
        assert ((got["prob"] == 0) == zero).all() and not np.signbit(got["prob"]).any()     # the zero pattern, exactly
        count = int((c["hits"] >= np.uint64(min_hits)).sum())
        r = ref.NO_VALID_ROW                               # no valid column: exactly uniform over the qualifying nodes
        assert got["norm"][r] == count and (got["prob"][r][~zero[r]] == 1.0 / count).all()
        assert got["draw"][r] == np.flatnonzero(~zero[r])[min(int(np.floor(u[r] * count)), count - 1)]
        clear = near[:, 0] > ref.NEAR
        assert int((~clear).sum()) <= ref.NEAR_CAP
        assert (got["draw"][clear] == unit[:, 0][clear]).all(), np.flatnonzero(got["draw"] != unit[:, 0])
        # the mask moved something: the unmasked call takes the NaN at the invalid positions for measured values
        plain = ctx.restricted_bmd(min_hits, probs=True)
        X0 = np.where(c["valid"], c["X"], f32(0))
        ctx.upload_chunk(X0)                               # ... or, with placeholders of 0, for measured zeros
        zeros = ctx.restricted_bmd(min_hits, probs=True)
        ctx.upload_chunk(c["X"])
        assert np.isnan(plain["norm"][~c["valid"].all(axis=1)]).all()
        moved += int((np.argmax(got["prob"], axis=1) != np.argmax(zeros["prob"], axis=1)).sum())
    assert moved > 0
    ctx.close()


# ---- 3. mass recovered ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,J", [(7, 5, 9), (17, 16, 37)])
def test_mass_recovered(W, H, J):
    c = ref.case(po.STANDARD, W, H, J)
    N = W * H
    rng = np.random.default_rng(12)
    units = rng.integers(0, N, B)
    cols = rng.integers(0, J, B)
    X = c["M"][units].copy()
    X[np.arange(B), cols] = f32(100)                       # one wild placeholder per row
    valid = np.ones((B, J), bool)
    valid[np.arange(B), cols] = False
    ctx = context(c, X)
    plain = ctx.restricted_bmd(0, u=c["U"][:, 0])
    assert (plain["norm"] == 0).all() and (plain["draw"] == NODRAW).all()           # the whole row's mass is gone
    got = ctx.restricted_bmd_masked(valid, 0, u=c["U"][:, 0], probs=True)
    assert (got["norm"] >= 1).all() and np.isfinite(got["norm"]).all()              # the unit itself has p = 1
    assert (np.argmax(got["prob"], axis=1) == units).all()
    assert (got["prob"][np.arange(B), units] == 1.0 / got["norm"]).all()            # p = exp(-0) = 1, exactly
    ctx.close()


# ---- 4. engineered draws under a mask -----------------------------------------------------------------------------------------
def test_engineered_draws():
    W, H, J = 5, 4, 6
    N = W * H
    rs = np.random.RandomState(3)
    x = rs.uniform(-1, 1, (1, J)).astype(f32)
    M = (x + rs.uniform(-0.3, 0.3, (N, J))).astype(f32)       # every node has mass of the same order
    hits = np.arange(N, dtype=np.uint64) % 3                  # 0, 1, 2, ...: nodes 0, 3, 6, ... masked at 1
    X = np.repeat(x, 8, axis=0)
    X[:, 2] = f32(np.nan)                                     # an invalid column holding NaN in every row
    valid = np.ones(J, np.uint8)
    valid[2] = 0
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=M, hits=hits)
    ctx.upload_chunk(X)
    pos = np.nonzero(hits >= 1)[0]
    for v in (valid, np.repeat(valid[None], 8, axis=0)):
        r = ctx.restricted_bmd_masked(v, 1, u=np.zeros(8))
        assert (r["draw"] == pos[0]).all()                    # u = 0: the first qualifying node
        r = ctx.restricted_bmd_masked(v, 1, u=np.full(8, np.nextafter(1.0, 0.0)))
        assert (r["draw"] == pos[-1]).all()                   # u = nextafter(1, 0): the last
    # exactly one eligible node is always drawn
    h1 = np.zeros(N, np.uint64)
    h1[13] = 4
    ctx.set_state(hits=h1)
    r = ctx.restricted_bmd_masked(valid, 1, u=np.random.default_rng(1).random(8), probs=True)
    assert (r["draw"] == 13).all() and (r["prob"][:, 13] == 1.0).all()
    # a NaN model entry at the invalid column has no effect
    ctx.set_state(hits=hits)
    u = np.random.default_rng(2).random(8)
    base = ctx.restricted_bmd_masked(valid, 0, u=u, probs=True)
    base1 = ctx.restricted_bmd_masked(valid, 1, u=u, probs=True)
    assert np.isfinite(base["norm"]).all() and (base["norm"] > 0).all()
    Mn = M.copy()
    Mn[:, 2] = np.nan
    Mn[4, 2] = np.inf
    ctx.set_state(map=Mn)
    same(ctx.restricted_bmd_masked(valid, 0, u=u, probs=True), base, "NaN at the invalid column of the model rows")
    # a NaN at a valid column of an eligible node: norm NaN, no draw; of a node without the hits: no effect
    Mv = M.copy()
    Mv[3, 1] = np.nan                                         # hits[3] = 0
    ctx.set_state(map=Mv)
    same(ctx.restricted_bmd_masked(valid, 1, u=u, probs=True), base1, "NaN in a node without the hits")
    r = ctx.restricted_bmd_masked(valid, 0, u=u, probs=True)
    assert np.isnan(r["norm"]).all() and (r["draw"] == NODRAW).all() and np.isnan(r["prob"]).all()
    ctx.close()


# ---- 6. column mask and sub-ranges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", [(po.STANDARD, 9, 15, 37), (po.MEDIAN, 17, 16, 9)])
def test_one_mask_and_sub_ranges(tr, W, H, J):
    c = ref.case(tr, W, H, J)
    ctx = context(c, np.where(c["valid"], c["X"], f32(0.5)).astype(f32))
    u = c["U"][:, 0]
    col = c["valid"][1]
    assert 0 < col.sum() < J
    full = ctx.restricted_bmd_masked(c["valid"], 3, u=u, probs=True)
    one = ctx.restricted_bmd_masked(col, 3, u=u, probs=True)
    same(ctx.restricted_bmd_masked(np.repeat(col[None], B, axis=0), 3, u=u, probs=True), one, "1-D mask against its rows")
    assert not beq(one["norm"], full["norm"])
    for want, v in ((full, c["valid"]), (one, col)):
        pieces = []
        for r0, r1 in ((0, 1), (1, 5), (5, 5), (5, 63), (63, 70)):
            vv = v if v.ndim == 1 else v[r0:r1]
            pieces.append(ctx.restricted_bmd_masked(vv, 3, r0=r0, r1=r1, u=u[r0:r1], probs=True))
            assert pieces[-1]["norm"].shape == (r1 - r0,) and pieces[-1]["prob"].shape == (r1 - r0, W * H)
        for k in KEYS:
            assert beq(np.concatenate([p[k] for p in pieces]), want[k]), k
    # outputs are optional: norm alone, no uniforms
    alone = ctx.restricted_bmd_masked(col, 3)
    assert alone["draw"] is None and alone["prob"] is None and beq(alone["norm"], one["norm"])
    ctx.close()


# ---- 7. slices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", [(po.STANDARD, 17, 16, 37)])
def test_row_slices(monkeypatch, tr, W, H, J):
    c = ref.case(tr, W, H, J)
    ctx = context(c)
    u = c["U"][:, 0]
    col = c["valid"][1]
    want = ctx.restricted_bmd_masked(c["valid"], 3, u=u, probs=True)
    want1 = ctx.restricted_bmd_masked(col, 3, u=u, probs=True)
    for rows in ("20", "1", "64"):                           # 20: a pitch of 24 for 20 rows; 64: the tile, then 6 rows
        monkeypatch.setenv("VSOM_MASKED_SLICE_ROWS", rows)
        monkeypatch.setenv("VSOM_GENERATE_SLICE_ROWS", rows)
        same(ctx.restricted_bmd_masked(c["valid"], 3, u=u, probs=True), want, ("sliced", rows))
        same(ctx.restricted_bmd_masked(col, 3, u=u, probs=True), want1, ("sliced, column mask", rows))
        part = ctx.restricted_bmd_masked(c["valid"][7:66], 3, r0=7, r1=66, u=u[7:66], probs=True)
        for k in KEYS:
            assert beq(part[k], want[k][7:66]), (rows, k)
    ctx.close()


# ---- 8. read-only -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", [(po.STANDARD, 9, 15, 37), (po.MEDIAN, 7, 5, 9)])
def test_read_only(tr, W, H, J):
    X = gen.blobs(B, J, 4, 15, 2)
    init = gen.random_map(W * H, J, seed=16)
    ctx = vsom_amd.Context(W, H, J, tr)
    o = po.OracleSom(W, H, J, tr)
    ctx.set_state(map=init)
    o.set_state(map=init)
    ctx.upload_chunk(X)
    lbo = np.zeros(B, np.uint64)
    assert f32(ctx.batch_epoch(3.0, True)) == f32(o.batch_epoch(X, lbo, 3.0, True))
    before, lb, sq = ctx.get_state(), ctx.get_last_bmu(), ctx.get_sqres()
    valid = np.random.default_rng(3).random((B, J)) < 0.7
    u = np.random.default_rng(4).random(B)
    a = ctx.restricted_bmd_masked(valid, 1, u=u, probs=True)
    ctx.restricted_bmd_masked(valid[0], 0, r0=10, r1=50, u=u[10:50])
    same(ctx.restricted_bmd_masked(valid, 1, u=u, probs=True), a, "repeated")
    after = ctx.get_state()
    for k in before:
        assert beq(before[k], after[k]), k
    assert (ctx.get_last_bmu() == lb).all() and (lb == lbo).all() and beq(ctx.get_sqres(), sq)
    assert beq(ctx.bmu_masked(np.ones(J, np.uint8), fill=True)["fill"], X)      # the chunk, read back
    assert f32(ctx.batch_epoch(2.0, False)) == f32(o.batch_epoch(X, lbo, 2.0, False))
    st = ctx.get_state()
    for k, want in (("map", o.map), ("sigma", o.sigma), ("S", o.S), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], want), ("the epoch after the masked distribution", k)
    assert (ctx.get_last_bmu() == lbo).all()
    ctx.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    W, H, J, rows = 6, 5, 7, 20
    init = gen.random_map(W * H, J, seed=1)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    L = capi.lib()
    u8, dp = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_double)
    valid = np.ones((rows, J), np.uint8)
    u = np.full(rows, 0.5)
    norm, draw = np.zeros(rows), np.zeros(rows, np.uint64)

    def bmd(r0, r1, h=ctx._h, v=valid, uu=u, d=draw):
        return L.vsom_bmd_masked_batch(h, 0, r0, r1, None if v is None else v.ctypes.data_as(u8), 0,
                                       None if uu is None else uu.ctypes.data_as(dp), capi._u(d), norm.ctypes.data_as(dp), None)

    def refused(code, word):
        assert code == -1, word
        assert word in L.vsom_last_error().decode(), (word, L.vsom_last_error().decode())

    refused(bmd(0, 0), "no chunk")
    refused(bmd(0, 1, h=None), "null context")
    X = gen.blobs(rows, J, 3, 1, 2)
    ctx.upload_chunk(X)
    good = ctx.restricted_bmd_masked(valid, 0, u=u, probs=True)
    refused(bmd(0, rows, v=None), "valid_host")
    for r0, r1 in ((5, 4), (0, rows + 1), (rows + 1, rows + 2)):
        refused(bmd(r0, r1), "row range")
    refused(bmd(0, rows, uu=None), "uniform")               # draws without uniforms
    for bad in (1.0, -0.125, np.nan, np.inf):
        ub = u.copy()
        ub[rows - 1] = bad
        refused(bmd(0, rows, uu=ub), "uniform " + str(rows - 1))
        assert bmd(0, rows - 1, uu=ub) == 0                 # (outside the range: not read)
    same(ctx.restricted_bmd_masked(valid, 0, u=u, probs=True), good, "after refusals")
    assert bmd(3, 3) == 0                                   # an empty range
    assert bmd(0, rows, uu=None, d=None) == 0 and beq(norm, good["norm"])       # norm alone
    assert bmd(0, rows) == 0 and (draw == good["draw"]).all()
    o = po.OracleSom(W, H, J)
    o.set_state(map=init)
    lbo = np.zeros(rows, np.uint64)
    assert f32(ctx.batch_epoch(1.5, True)) == f32(o.batch_epoch(X, lbo, 1.5, True))
    st = ctx.get_state()
    for k, want in (("map", o.map), ("sigma", o.sigma), ("S", o.S), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], want), ("after refusals", k)
    ctx.close()

    # CLR contexts
    Xc = (np.abs(gen.blobs(rows, 5, 3, 1, 2)) + f32(0.5)).astype(f32)
    clr = vsom_amd.Context(4, 4, 5, po.CLR)
    oc = po.OracleSom(4, 4, 5, po.CLR)
    initc = gen.random_map(16, oc.depth, seed=2)
    clr.set_state(map=initc)
    oc.set_state(map=initc)
    clr.upload_chunk(Xc)
    with pytest.raises(capi.VsomError, match="vsom_bmd_masked_batch: CLR"):
        clr.restricted_bmd_masked(np.ones((rows, 5), np.uint8), 0)
    assert f32(clr.batch_epoch(1.5, True)) == f32(oc.batch_epoch(Xc, lbo, 1.5, True))
    stc = clr.get_state()
    for k, want in (("map", oc.map), ("sigma", oc.sigma), ("weight", oc.weight), ("hits", oc.hits)):
        assert beq(stc[k], want), ("CLR after the refusal", k)
    clr.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_bmd_masked_batch"):
        cu.restricted_bmd_masked(np.ones((10, 5), np.uint8), 0)
    cu.bmu_batch()
    cu.close()

    # a chunk staged ahead (as tests/test_gpu_masked.py): refused until it is committed
    W = H = 48
    J = 196
    xs = [gen.mnist_like(1100, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * f32(100) + f32(100)).astype(f32)
    big = vsom_amd.Context(W, H, J)
    pb = capi.PinnedBuffer(xs[1].shape)
    pb.array[...] = xs[1]
    big.set_state(map=init)
    big.upload_chunk(xs[0])
    big.batch_epoch_async(10.0, True)
    big.prefetch_chunk(pb.array)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        big.restricted_bmd_masked(np.ones(J, np.uint8), 0)
    big.commit_chunk()
    got = big.restricted_bmd_masked(np.ones(J, np.uint8), 0, r0=0, r1=4, u=np.full(4, 0.5), probs=True)
    same(got, big.restricted_bmd(0, r0=0, r1=4, u=np.full(4, 0.5), probs=True), "after the commit")
    big.close()
    pb.free()
