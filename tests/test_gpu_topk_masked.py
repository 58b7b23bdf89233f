"""GPU: vsom_bmu_topk_masked_batch -- the k best matching units of every chunk row over its VALID columns, among node 0 and
the nodes with enough hits, and the record blended from them.  With an all-valid mask and min_hits = 0 the lists are
vsom_bmu_topk_batch's bit for bit; under random masks idx, dist, count and nvalid are the numpy restatement's
(tests/topk_masked_ref.py) bit for bit and column 0 is vsom_bmu_masked_batch's; blend is held against the float64 restatement
within (k + 2) * 2^-51 * max_j |m[j][d]| (only exp may differ, by an ulp on either side; the sums, products and the quotient
are the same operations in the same order).
Shapes (tests/bmd_masked_ref.py): maps of 35 nodes (under one node tile; k = 35 pads under min_hits = 3), 135 (two tiles and a
ragged one) and 272 (several), J of 3 / 9 / 37 / 70, 70 rows (one 64-row tile and 6), Standard and Median."""
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
import topk_masked_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
B = ref.B
beq = ref.beq
KEYS = ("idx", "dist", "count", "nvalid", "blend")
RATIOS = []        # worst |blend - ref| / bound per case (printed at the end of the module)


def ks(N):
    return (1, 2, 7, min(64, N))


def same(a, b, what=None, keys=KEYS):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert beq(a[k], b[k]), (what, k)


def context(c, X=None):
    ctx = vsom_amd.Context(c["W"], c["H"], c["J"], c["tr"])
    ctx.set_state(map=c["M"], sigma=c["S"], hits=c["hits"])
    ctx.upload_chunk(c["X"] if X is None else X)
    return ctx


def check_padding(got, k):
    """from entry count on: idx = UINT64_MAX, dist = 0x7FC00000, on the bits; every real entry is a node"""
    pad = np.arange(k)[None, :] >= got["count"][:, None]
    assert (got["idx"][pad] == ref.NO_UNIT).all() and (got["dist"].view(np.uint32)[pad] == ref.QNAN32).all()
    assert (got["idx"][~pad] != ref.NO_UNIT).all()
    assert (got["dist"].view(np.uint32)[np.isnan(got["dist"])] == ref.QNAN32).all()


def check_blend(got, X, valid, M, k, tag):
    """valid columns (double)x on the bits; without mass the quiet NaN; with mass within the bound of the float64 restatement
    evaluated on the lists the call returned.  Returns the worst ratio to the bound."""
    valid = np.broadcast_to(np.asarray(valid) != 0, X.shape)
    want, mass = ref.blend(X, valid, M, got["idx"], got["dist"], got["count"])
    b = got["blend"]
    assert beq(b[valid], X[valid].astype(np.float64)), tag
    nomass = ~mass[:, None] & ~valid
    assert (b.view(np.uint64)[nomass] == ref.QNAN64).all(), tag
    m = mass[:, None] & ~valid
    bound = ref.blend_bound(M, got["idx"], got["count"], k)
    with np.errstate(all="ignore"):
        fin = m & np.isfinite(want)
        assert beq(np.isnan(b[m]), np.isnan(want[m])) and beq(b[m & ~fin], want[m & ~fin]), tag
        err = np.abs(b - want)[fin]
        assert (err <= bound[fin]).all(), (tag, float((err / bound[fin]).max()))
        return float((err[bound[fin] > 0] / bound[fin][bound[fin] > 0]).max()) if (bound[fin] > 0).any() else 0.0


def teardown_module(module):
    for tag, worst in RATIOS:
        print(f"[topk_masked] {tag}: worst |blend - ref| / bound {worst:.3f}")


# ---- 1. an all-valid mask, min_hits = 0: the unmasked call ----------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", ref.SHAPES)
def test_all_valid_equals_topk(tr, W, H, J):
    c = ref.case(tr, W, H, J)
    X = ref.bmr.unit_rows(B, J, 77)
    ctx = context(c, X)
    for k in ks(W * H):
        idx, dist = ctx.bmu_topk(k)
        for v in (np.ones((B, J), np.uint8), np.ones(J, np.uint8)):
            got = ctx.bmu_topk_masked(k, v, blend=True)
            assert (got["idx"] == idx).all() and beq(got["dist"], dist), (k, v.ndim)
            assert (got["count"] == k).all() and (got["nvalid"] == J).all()
            assert beq(got["blend"], X.astype(np.float64))
    ctx.close()


# ---- 2. random masks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", ref.SHAPES)
def test_random_masks(tr, W, H, J):
    c = ref.case(tr, W, H, J)
    ctx = context(c)
    N = W * H
    moved = padded = 0
    for min_hits in ref.MIN_HITS:
        bm = ctx.bmu_masked(c["valid"], min_hits=min_hits)
        for k in ks(N):
            idx, dist, count = ref.lists(c["d"], c["hits"], min_hits, k)
            got = ctx.bmu_topk_masked(k, c["valid"], min_hits=min_hits)
            assert (got["idx"] == idx).all(), (min_hits, k, np.argwhere(got["idx"] != idx)[:4])
            assert beq(got["dist"], dist) and (got["count"] == count).all(), (min_hits, k)
            assert (got["nvalid"] == ref.nvalid(c["valid"], B)).all()
            assert (got["idx"][:, 0] == bm["bmu"]).all() and beq(got["dist"][:, 0], bm["dist"]), (min_hits, k)
            check_padding(got, k)
            padded += int((got["count"] < k).sum())
            r = ref.NO_VALID_ROW                               # no valid column: the first candidates, every distance +0
            n = int(count[r])
            assert (got["idx"][r, :n] == ref.candidates(c["hits"], min_hits)[:n]).all() and got["nvalid"][r] == 0
            assert (got["dist"].view(np.uint32)[r, :n] == 0).all()
        assert (count == min(k, ref.candidates(c["hits"], min_hits).size)).all()
    assert padded > 0                                          # (min_hits = 6 leaves node 0 alone)
    # the mask moved something: with placeholders of 0 the unmasked call takes them for measured zeros
    ctx.upload_chunk(np.where(c["valid"], c["X"], f32(0)))
    zi, _ = ctx.bmu_topk(2)
    ctx.upload_chunk(c["X"])
    moved += int((ctx.bmu_topk_masked(2, c["valid"])["idx"] != zi).sum())
    assert moved > 0
    ctx.close()


# ---- 3. a column mask, sub-ranges and slices ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", [(po.STANDARD, 9, 15, 37), (po.MEDIAN, 17, 16, 9)])
def test_one_mask_sub_ranges_and_slices(monkeypatch, tr, W, H, J):
    c = ref.case(tr, W, H, J)
    X = np.where(c["valid"], c["X"], f32(0.5)).astype(f32)
    ctx = context(c, X)
    col = c["valid"][1]
    assert 0 < col.sum() < J
    k = 7
    full = ctx.bmu_topk_masked(k, c["valid"], min_hits=3, blend=True)
    one = ctx.bmu_topk_masked(k, col, min_hits=3, blend=True)
    same(ctx.bmu_topk_masked(k, np.repeat(col[None], B, axis=0), min_hits=3, blend=True), one, "1-D mask against its rows")
    idx, dist, count = ref.lists(ref.masked_d(tr, X, c["M"], col), c["hits"], 3, k)
    assert (one["idx"] == idx).all() and beq(one["dist"], dist) and (one["nvalid"] == col.sum()).all()
    assert not (one["idx"] == full["idx"]).all()
    for want, v in ((full, c["valid"]), (one, col)):
        pieces = []
        for r0, r1 in ((0, 1), (1, 5), (5, 5), (5, 70), (64, 70)):
            vv = v if v.ndim == 1 else v[r0:r1]
            p = ctx.bmu_topk_masked(k, vv, r0=r0, r1=r1, min_hits=3, blend=True)
            assert p["idx"].shape == (r1 - r0, k) and p["blend"].shape == (r1 - r0, J) and p["count"].shape == (r1 - r0,)
            for key in KEYS:
                assert beq(p[key], want[key][r0:r1]), (r0, r1, key)
            pieces.append(p)
        for key in KEYS:
            assert beq(np.concatenate([p[key] for p in pieces[:4]]), want[key]), key
    # outputs are optional
    alone = ctx.bmu_topk_masked(k, col, min_hits=3, dist=False)
    assert alone["dist"] is None and alone["blend"] is None and (alone["idx"] == one["idx"]).all()
    for rows in ("1", "7", "64"):                            # 64: the tile, then 6 rows
        monkeypatch.setenv("VSOM_MASKED_SLICE_ROWS", rows)
        same(ctx.bmu_topk_masked(k, c["valid"], min_hits=3, blend=True), full, ("sliced", rows))
        same(ctx.bmu_topk_masked(k, col, min_hits=3, blend=True), one, ("sliced, column mask", rows))
        part = ctx.bmu_topk_masked(k, c["valid"][7:66], r0=7, r1=66, min_hits=3, blend=True)
        for key in KEYS:
            assert beq(part[key], full[key][7:66]), (rows, key)
    ctx.close()


# ---- 4. poison ----------------------------------------------------------------------------------------------------------------
def test_poison():
    tr, W, H, J = po.STANDARD, 9, 15, 37
    c = ref.case(tr, W, H, J)
    N, k = W * H, 7
    col = c["valid"][1].copy()
    bad = np.flatnonzero(~col)
    X = np.where(col, ref.bmr.unit_rows(B, J, 5), f32(0.5)).astype(f32)
    ctx = context(c, X)
    base = ctx.bmu_topk_masked(k, c["valid"], min_hits=3, blend=True)
    base1 = ctx.bmu_topk_masked(k, col, min_hits=3, blend=True)
    ok = np.ones(J, bool)
    ok[bad] = False
    for junk in (f32(np.nan), f32(np.inf), f32(-np.inf), f32(1e30)):
        # rows: at the invalid positions of a per-row mask nothing changes, blend included (it selects x at valid columns only)
        ctx.upload_chunk(np.where(c["valid"], X, junk).astype(f32))
        same(ctx.bmu_topk_masked(k, c["valid"], min_hits=3, blend=True), base, ("rows", junk))
        # rows and model rows, at the columns a column mask declares invalid for every row: no idx, dist, count or nvalid
        # bit changes; blend reads the model there (that is the imputation), so it is compared at the other columns
        ctx.upload_chunk(np.where(col, X, junk).astype(f32))
        ctx.set_state(map=np.where(col, c["M"], junk).astype(f32))
        got = ctx.bmu_topk_masked(k, col, min_hits=3, blend=True)
        same(got, base1, ("rows and model rows", junk), keys=("idx", "dist", "count", "nvalid"))
        assert beq(got["blend"][:, ok], base1["blend"][:, ok]), junk
        ctx.set_state(map=c["M"])
    assert np.isfinite(base["dist"]).all() and np.isfinite(base1["blend"]).all()
    # a NaN at a valid position of a row: every distance NaN -- the node-0 rule, and a blend row without mass
    Xn = X.copy()
    v = np.flatnonzero(col)[0]
    Xn[3, v] = np.nan
    ctx.upload_chunk(Xn)
    got = ctx.bmu_topk_masked(k, col, min_hits=3, blend=True)
    cand = ref.candidates(c["hits"], 3)
    assert (got["idx"][3] == cand[:k]).all() and got["idx"][3, 0] == 0 and got["count"][3] == k
    assert (got["dist"].view(np.uint32)[3] == ref.QNAN32).all()
    assert np.isnan(got["blend"][3, v]) and (got["blend"].view(np.uint64)[3, bad] == ref.QNAN64).all()
    assert beq(got["blend"][3, col], Xn[3, col].astype(np.float64))
    keep = np.arange(B) != 3
    same({key: got[key][keep] for key in KEYS}, {key: base1[key][keep] for key in KEYS}, "the other rows")
    # a NaN in node 0 only: d_0 is NaN, node 0 is entry 0, the others follow in key order and carry the mass
    M0 = c["M"].copy()
    M0[0, v] = np.nan
    ctx.upload_chunk(X)
    ctx.set_state(map=M0)
    got = ctx.bmu_topk_masked(k, col, min_hits=3, blend=True)
    idx, dist, count = ref.lists(ref.masked_d(tr, X, M0, col), c["hits"], 3, k)
    assert (got["idx"] == idx).all() and beq(got["dist"], dist) and (got["idx"][:, 0] == 0).all()
    assert np.isnan(got["dist"][:, 0]).all() and np.isfinite(got["dist"][:, 1:]).all()
    bm = ctx.bmu_masked(col, min_hits=3)
    assert (bm["bmu"] == 0).all() and beq(bm["dist"], got["dist"][:, 0])
    RATIOS.append(("node 0 NaN", check_blend(got, X, col, M0, k, "node 0 NaN")))
    assert np.isfinite(got["blend"][:, bad]).all()
    # a model row of 3e38: +inf distances, last among the candidates, skipped in blend
    few = np.zeros(N, np.uint64)
    chosen = np.arange(7, N, 13)[:10]                         # ten nodes with hits, and node 0: k = 11 takes them all
    few[chosen] = 5
    Mi = c["M"].copy()
    big = chosen[2:5]
    Mi[big] = f32(3e38)
    ctx.set_state(map=Mi, hits=few)
    kk = chosen.size + 1
    got = ctx.bmu_topk_masked(kk, col, min_hits=3, blend=True)
    idx, dist, count = ref.lists(ref.masked_d(tr, X, Mi, col), few, 3, kk)
    assert (got["idx"] == idx).all() and beq(got["dist"], dist) and (got["count"] == kk).all()
    assert np.isinf(got["dist"][:, -3:]).all() and (got["idx"][:, -3:] == big).all()      # tied at +inf: index order
    RATIOS.append(("3e38 rows", check_blend(got, X, col, Mi, kk, "3e38 rows")))
    assert np.isfinite(got["blend"]).all() and (np.abs(got["blend"][:, bad]) <= 1.0).all()
    ctx.close()


# ---- 5. ties ------------------------------------------------------------------------------------------------------------------
def test_ties():
    W, H, J, rows = 6, 5, 9, 12
    N = W * H
    rng = np.random.default_rng(5)
    M = rng.uniform(0.1, 0.9, (N, J)).astype(f32)
    X = rng.uniform(0.1, 0.9, (rows, J)).astype(f32)
    valid = np.ones((rows, J), bool)
    valid[:, 4] = False
    valid[::2, 7] = False
    M[11] = M[3]
    M[11, 4] = f32(0.77)              # differs from node 3 only in a column invalid for every row
    M[20] = M[3]                      # bit-identical to node 3
    M[25] = M[3]
    M[25, 7] = f32(0.01)              # differs from node 3 in a column invalid for the even rows only
    X = (M[3][None] + rng.uniform(-0.01, 0.01, (rows, J))).astype(f32)      # every row next to node 3
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=M)
    ctx.upload_chunk(X)
    got = ctx.bmu_topk_masked(6, valid, blend=True)
    idx, dist, count = ref.lists(ref.masked_d(po.STANDARD, X, M, valid), np.zeros(N, np.uint64), 0, 6)
    assert (got["idx"] == idx).all() and beq(got["dist"], dist)
    assert (got["idx"][::2, :4] == [3, 11, 20, 25]).all()                 # four-way tie on the bits, in index order
    assert (got["dist"].view(np.uint32)[::2, :4] == got["dist"].view(np.uint32)[::2, :1]).all()
    assert (got["idx"][1::2, :3] == [3, 11, 20]).all()                    # (column 7 counts for the odd rows)
    assert (got["dist"].view(np.uint32)[1::2, 3] != got["dist"].view(np.uint32)[1::2, 0]).all()
    assert (got["dist"].view(np.uint32)[1::2, :3] == got["dist"].view(np.uint32)[1::2, :1]).all()
    # under a hit restriction node 3 leaves and its twins stay, in index order
    hits = np.full(N, 2, np.uint64)
    hits[3] = 0
    ctx.set_state(hits=hits)
    got = ctx.bmu_topk_masked(3, valid, min_hits=1)
    assert (got["idx"][::2] == [11, 20, 25]).all() and (got["idx"][1::2, :2] == [11, 20]).all()
    bm = ctx.bmu_masked(valid, min_hits=1)
    assert (bm["bmu"] == 11).all() and beq(bm["dist"], got["dist"][:, 0])
    ctx.close()


# ---- 6. blend -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", ref.SHAPES)
def test_blend(tr, W, H, J):
    c = ref.case(tr, W, H, J)
    ctx = context(c)
    N = W * H
    worst = 0.0
    for min_hits in ref.MIN_HITS:
        for k in (2, 7, min(64, N)):
            got = ctx.bmu_topk_masked(k, c["valid"], min_hits=min_hits, blend=True)
            worst = max(worst, check_blend(got, c["X"], c["valid"], c["M"], k, (min_hits, k)))
            # the row without a valid column: the plain mean of its first `count` candidates
            r = ref.NO_VALID_ROW
            n = int(got["count"][r])
            mean = c["M"][got["idx"][r, :n].astype(np.int64)].astype(np.float64).mean(axis=0)
            bound = ref.blend_bound(c["M"], got["idx"][r:r + 1], got["count"][r:r + 1], k)[0]
            assert (np.abs(got["blend"][r] - mean) <= bound).all(), (min_hits, k)
            if n == 1:                                         # one unit: its model row, exactly
                assert beq(got["blend"][r], c["M"][int(got["idx"][r, 0])].astype(np.float64))
    print(f"[topk_masked] {tr}/{W}x{H}x{J}: worst |blend - ref| / bound {worst:.3f}")
    RATIOS.append((f"{tr}/{W}x{H}x{J}", worst))
    # one unit: the point imputation of bmu_masked, widened
    got = ctx.bmu_topk_masked(1, c["valid"], min_hits=3, blend=True)
    fill = ctx.bmu_masked(c["valid"], min_hits=3, fill=True)["fill"]
    assert beq(got["blend"], fill.astype(np.float64))
    ctx.close()


# ---- 7. read-only and deterministic ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", [(po.STANDARD, 9, 15, 37), (po.MEDIAN, 7, 5, 9)])
def test_read_only(tr, W, H, J):
    X = gen.blobs(B, J, 4, 15, 2)
    init = gen.random_map(W * H, J, seed=16)
    ctx, twin = vsom_amd.Context(W, H, J, tr), vsom_amd.Context(W, H, J, tr)
    o = po.OracleSom(W, H, J, tr)
    for t in (ctx, twin):
        t.set_state(map=init)
        t.upload_chunk(X)
    o.set_state(map=init)
    lbo = np.zeros(B, np.uint64)
    assert f32(ctx.batch_epoch(3.0, True)) == f32(o.batch_epoch(X, lbo, 3.0, True))
    twin.batch_epoch(3.0, True)
    before, lb, sq = ctx.get_state(), ctx.get_last_bmu(), ctx.get_sqres()
    valid = np.random.default_rng(3).random((B, J)) < 0.7
    a = ctx.bmu_topk_masked(5, valid, min_hits=1, blend=True)
    ctx.bmu_topk_masked(2, valid[0], r0=10, r1=50)
    same(ctx.bmu_topk_masked(5, valid, min_hits=1, blend=True), a, "repeated")
    after = ctx.get_state()
    for k in before:
        assert beq(before[k], after[k]), k
    assert (ctx.get_last_bmu() == lb).all() and (lb == lbo).all() and beq(ctx.get_sqres(), sq)
    assert beq(ctx.bmu_masked(np.ones(J, np.uint8), fill=True)["fill"], X)      # the chunk, read back
    assert f32(ctx.batch_epoch(2.0, False)) == f32(o.batch_epoch(X, lbo, 2.0, False))
    twin.batch_epoch(2.0, False)
    st, tw = ctx.get_state(), twin.get_state()
    for k, want in (("map", o.map), ("sigma", o.sigma), ("S", o.S), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], want) and beq(st[k], tw[k]), ("the epoch after the masked top-k", k)
    assert (ctx.get_last_bmu() == lbo).all() and (twin.get_last_bmu() == lbo).all()
    ctx.close()
    twin.close()


def test_a_pending_sigma_stays_pending():
    W = H = 40
    J, rows = 300, 77
    init = gen.random_map(W * H, J, 42) * f32(100)
    X = gen.mnist_like(rows, 3, J)
    valid = np.random.default_rng(8).random((rows, J)) < 0.7
    res = {}
    for mode in (capi.SIGMA_LAZY, capi.SIGMA_EAGER):
        ctx = vsom_amd.Context(W, H, J, capi.STANDARD)
        ctx.set_sigma_mode(mode)
        ctx.set_column_compaction(1)
        ctx.set_state(map=init)
        ctx.upload_chunk(X)
        ctx.batch_epoch(6.0, True)
        s = ctx.sigma_stats()
        assert s["pending"] == (mode == capi.SIGMA_LAZY), (mode, s)
        out = ctx.bmu_topk_masked(5, valid, min_hits=1, blend=True)
        assert ctx.sigma_stats() == s, (mode, s, ctx.sigma_stats())           # still pending, nothing materialised
        res[mode] = (out, ctx.get_state(S=False))
        ctx.close()
    same(res[capi.SIGMA_LAZY][0], res[capi.SIGMA_EAGER][0], "lazy against eager")
    for k in ("map", "sigma", "weight", "hits"):
        assert beq(res[capi.SIGMA_LAZY][1][k], res[capi.SIGMA_EAGER][1][k]), k


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    W, H, J, rows = 6, 5, 7, 20
    N = W * H
    init = gen.random_map(N, J, seed=1)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    L = capi.lib()
    u8 = ctypes.POINTER(ctypes.c_uint8)
    valid = np.ones((rows, J), np.uint8)
    idx = np.zeros((rows, 64), np.uint64)

    def topk(r0, r1, k=2, h=ctx._h, v=valid, out=True, with_idx=True):
        o = capi.TopkMaskedOut()
        if with_idx:
            o.idx = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        return L.vsom_bmu_topk_masked_batch(h, k, 0, r0, r1, None if v is None else v.ctypes.data_as(u8), 0,
                                            ctypes.byref(o) if out else None)

    def refused(code, word):
        assert code == -1, word
        assert word in L.vsom_last_error().decode(), (word, L.vsom_last_error().decode())

    refused(topk(0, 0), "no chunk")
    refused(topk(0, 1, h=None), "null context")
    X = gen.blobs(rows, J, 3, 1, 2)
    ctx.upload_chunk(X)
    good = ctx.bmu_topk_masked(3, valid, blend=True)
    refused(topk(0, rows, v=None), "valid_host")
    refused(topk(0, rows, out=False), "out is null")
    refused(topk(0, rows, with_idx=False), "idx")
    for r0, r1 in ((5, 4), (0, rows + 1), (rows + 1, rows + 2)):
        refused(topk(r0, r1), "row range")
    for k in (0, 65, N + 1):
        refused(topk(0, rows, k=k), "k must be")
    same(ctx.bmu_topk_masked(3, valid, blend=True), good, "after refusals")
    idx[:] = 7
    assert topk(3, 3) == 0 and (idx == 7).all()                # an empty range: OK, nothing written
    assert topk(0, rows, k=N) == 0                             # k = N is allowed
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
    with pytest.raises(capi.VsomError, match="vsom_bmu_topk_masked_batch: CLR"):
        clr.bmu_topk_masked(2, np.ones((rows, 5), np.uint8))
    assert f32(clr.batch_epoch(1.5, True)) == f32(oc.batch_epoch(Xc, lbo, 1.5, True))
    stc = clr.get_state()
    for k, want in (("map", oc.map), ("sigma", oc.sigma), ("weight", oc.weight), ("hits", oc.hits)):
        assert beq(stc[k], want), ("CLR after the refusal", k)
    clr.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_bmu_topk_masked_batch"):
        cu.bmu_topk_masked(2, np.ones((10, 5), np.uint8))
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
        big.bmu_topk_masked(2, np.ones(J, np.uint8))
    big.commit_chunk()
    got = big.bmu_topk_masked(4, np.ones(J, np.uint8), r0=0, r1=4)
    ti, td = big.bmu_topk(4, 0, 4)
    assert (got["idx"] == ti).all() and beq(got["dist"], td)
    big.close()
    pb.free()


# ---- 9. the Som mirror ----------------------------------------------------------------------------------------------------------
class ValidDataSet(vs.ArrayDataSet):
    """an ArrayDataSet with validity flags"""

    def __init__(self, X, validity):
        super().__init__(X)
        self.validity = validity


def test_som_mirror():
    tr, W, H, J = po.STANDARD, 9, 15, 9
    c = ref.case(tr, W, H, J)
    s = vs.Som(W, H, J)
    s.setState(map=c["M"], hits=c["hits"])
    ds = ValidDataSet(c["X"], c["valid"])
    ds.loadNextDataFromStream()
    for min_hits in (3, 6):
        idx, dist, count = ref.lists(c["d"], c["hits"], min_hits, 5)
        rep = s.findBestMatchingUnitsMasked(ds, 5, min_hits, dist=True)
        assert sorted(rep) == ["count", "dist", "idx", "nvalid"]
        assert (rep["idx"] == idx).all() and beq(rep["dist"], dist) and (rep["count"] == count).all()
        assert "dist" not in s.findBestMatchingUnitsMasked(ds, 5, min_hits)
        i2, _, c2 = ref.lists(c["d"], c["hits"], min_hits, 2)
        keep = (ref.nvalid(c["valid"], B) >= 1) & (c2 >= 2)
        te, counted = s.topographicErrorMasked(ds, min_hits)
        assert counted == int(keep.sum()) and te == vs.topographic_error(i2[keep], W)
        if min_hits == 3:
            assert counted == B - 1                           # the row without a valid column is excluded
        else:
            assert counted == 0 and te == 0.0                 # node 0 alone: no second unit anywhere
        blend = s.imputeBlend(ds, 5, min_hits)
        assert blend.dtype == np.float64 and blend.shape == (B, J)
        assert beq(blend, s.ctx.bmu_topk_masked(5, c["valid"], min_hits=min_hits, blend=True)["blend"])
    # no validity attribute: every column counts
    X = ref.bmr.unit_rows(B, J, 9)
    plain = s.findBestMatchingUnitsMasked(X, 4, 0, dist=True)
    pi, pd = s.findBestMatchingUnits(X, 4, dist=True)
    assert (plain["idx"] == pi).all() and beq(plain["dist"], pd)
    assert s.topographicErrorMasked(X) == (s.topographicError(X), B)
    assert beq(s.imputeBlend(X, 4), X.astype(np.float64))
    empty = s.findBestMatchingUnitsMasked(np.zeros((0, J), f32), 4)
    assert empty["idx"].shape == (0, 4) and s.topographicErrorMasked(np.zeros((0, J), f32)) == (0.0, 0)
