"""GPU: vsom_bmu_masked_batch -- the best matching unit of chunk rows [r0, r1) over their valid columns, and the record
imputed from it.  General masks are checked bit for bit against the oracle's Comparer and dot product with the residual
set to +0 at invalid columns, and findRestrictedBmu's argmin rule restated here; the all-valid mask against
vsom_bmu_restricted_batch and vsom_bmu_batch.  Shapes: maps of 35 nodes (less than one node tile) and 135 (two tiles and a
ragged one), J of 3 / 9 / 37 / 70 (no whole packet, a packet and a tail, an odd tail past one K-chunk, several K-chunks),
70 rows (one row tile and 6 rows)."""
import ctypes
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")
QNAN = np.uint32(0x7FC00000)
B = 70
MAPS = ((7, 5), (9, 15))
DEPTHS = (3, 9, 37, 70)
KINDS = (po.STANDARD, po.MEDIAN)
SHAPES = [(tr, W, H, J) for tr in KINDS for (W, H) in MAPS for J in DEPTHS]


def beq(a, b):
    """bitwise equality; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()
    return (a == b).all()


def bits_eq(a, b):
    """bitwise equality, NaN payloads and the sign of zero included"""
    return (np.asarray(a, np.float32).view(np.uint32) == np.asarray(b, np.float32).view(np.uint32)).all()


def masked_dists(kind, x, M, valid):
    """the masked distance of row x to every node: the oracle's Comparer, +0 at invalid columns, the oracle's dot"""
    return np.array([po.dot_self(np.where(valid, po.comparer(kind, x, m), np.float32(0))) for m in M], np.float32)


def argmin_rule(d, hits, min_hits):
    """Som::findRestrictedBmu (Som.cpp:313-332): node 0 seeds, then strict < over the nodes with enough hits"""
    best, bd = 0, d[0]
    for n in range(len(d)):
        if d[n] < bd and hits[n] >= min_hits:
            best, bd = n, d[n]
    return best, bd


def checker(kind, X, M, valid, hits, min_hits, rows=None):
    rows = range(X.shape[0]) if rows is None else rows
    bmu, dist = [], []
    for r in rows:
        v = valid if valid.ndim == 1 else valid[r]
        b, d = argmin_rule(masked_dists(kind, X[r], M, v), hits, min_hits)
        bmu.append(b)
        dist.append(d)
    dist = np.array(dist, np.float32)
    dist[np.isnan(dist)] = QNAN.view(np.float32)
    return np.array(bmu, np.uint64), dist


def state(W, H, J, seed):
    """a random map and mixed hit counts (0 .. 5, node 0 without hits)"""
    M = gen.random_map(W * H, J, seed=seed)
    hits = np.random.default_rng(seed).integers(0, 6, W * H).astype(np.uint64)
    hits[0] = 0
    return M, hits


def make(tr, W, H, J, seed=3, rows=B):
    X = gen.blobs(rows, J, 4, seed, 2)
    M, hits = state(W, H, J, seed + 10)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=M, hits=hits)
    ctx.upload_chunk(X)
    return ctx, X, M, hits


def check_against(ctx, kind, X, M, valid, hits, min_hits, what):
    got = ctx.bmu_masked(valid, min_hits=min_hits, fill=True)
    eb, ed = checker(kind, X, M, valid, hits, min_hits)
    assert (got["bmu"] == eb).all(), (what, np.flatnonzero(got["bmu"] != eb)[:5])
    assert bits_eq(got["dist"], ed), (what, np.flatnonzero(got["dist"].view(np.uint32) != ed.view(np.uint32))[:5])
    v2 = np.broadcast_to(valid, X.shape)
    assert (got["nvalid"] == v2.sum(axis=1)).all(), what
    assert bits_eq(got["fill"], np.where(v2, X, M[eb.astype(np.int64)])), what
    return got


# ---- 1. the all-valid mask is the unmasked search ----------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", SHAPES)
def test_all_valid_equals_the_unmasked_searches(tr, W, H, J):
    ctx, X, M, hits = make(tr, W, H, J)
    ones = np.ones((B, J), np.uint8)
    for min_hits in (0, 3):
        got = ctx.bmu_masked(ones, min_hits=min_hits)
        ri, rd = ctx.bmu_restricted_batch(min_hits)
        assert (got["bmu"] == ri).all() and bits_eq(got["dist"], rd), min_hits
        assert (got["nvalid"] == J).all()
    assert (ctx.bmu_masked(ones, min_hits=3)["bmu"] != ctx.bmu_masked(ones)["bmu"]).any()   # the restriction restricts
    got = ctx.bmu_masked(ones)
    for mode in (capi.BMU_AUTO, capi.BMU_EXACT, capi.BMU_SHORTLIST):
        ctx.set_bmu_mode(mode)
        bi, bd = ctx.bmu_batch()
        assert (got["bmu"] == bi).all() and bits_eq(got["dist"], bd), mode
    ctx.close()


# ---- 2. random masks against the checker ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", SHAPES)
def test_random_masks(tr, W, H, J):
    ctx, X, M, hits = make(tr, W, H, J, seed=5)
    rng = np.random.default_rng(100 + J)
    valid = rng.random((B, J)) < 0.7
    valid[11] = False                                  # a row without a valid column
    valid[12] = False
    valid[12, J // 2] = True                           # a row with exactly one
    X = X.copy()
    poison = (np.float32(np.nan), np.float32(np.inf), np.float32(1e30))
    for i, r in enumerate((3, 11, 20, 37, 64, 66, 69)):   # NaN, +inf and 1e30 stored at invalid positions (rows of the
        valid[r, r % J] = False                           # ragged row tile among them)
        cols = np.flatnonzero(~valid[r])
        X[r, cols] = poison[i % 3]
        if cols.size > 1:
            X[r, cols[-1]] = poison[(i + 1) % 3]
    ctx.upload_chunk(X)
    for min_hits in (0, 3):
        got = check_against(ctx, tr, X, M, valid, hits, min_hits, (min_hits,))
        assert got["bmu"][11] == 0 and got["dist"][11].view(np.uint32) == 0 and got["nvalid"][11] == 0
        assert got["nvalid"][12] == 1
        assert np.isfinite(got["dist"]).all()          # nothing stored at an invalid position reaches a distance
    ctx.close()


# ---- 3. engineered ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", [(tr, W, H, J) for tr in KINDS for (W, H) in MAPS for J in (9, 37, 70)])
def test_engineered_ties(tr, W, H, J):
    ctx, X, M, hits = make(tr, W, H, J, seed=7)
    N = W * H
    hits = np.full(N, 4, np.uint64)
    M = M.copy()
    hi, lo, twin = N - 2, N // 3, N - 1                # the true BMU of rows 0..3, its look-alike, its twin
    col = J - 1                                        # (in the scalar tail of the dot product for J = 9 / 37 / 70)
    X = X.copy()
    X[:4] = M[hi] + np.float32(1e-3)                   # rows 0..3 sit next to node hi
    M[twin] = M[hi]                                    # two bit-identical model rows: the lower index must win
    M[lo] = M[hi]
    M[lo, col] += np.float32(0.75)                     # differs from the true BMU in one column only
    ctx.set_state(map=M, hits=hits)
    ctx.upload_chunk(X)
    allv = np.ones((B, J), bool)
    got = check_against(ctx, tr, X, M, allv, hits, 0, "all valid")
    assert (got["bmu"][:4] == hi).all()                # hi before its twin, and the look-alike does not win
    masked = allv.copy()
    masked[:4, col] = False                            # with that column masked the look-alike ties, and is lower
    got = check_against(ctx, tr, X, M, masked, hits, 0, "masked column")
    assert (got["bmu"][:4] == lo).all()
    colmask = np.ones(J, bool)
    colmask[col] = False
    got1 = check_against(ctx, tr, X, M, colmask, hits, 0, "column mask")
    assert (got1["bmu"][:4] == lo).all()
    hits[lo] = 0                                       # without the hits the look-alike cannot shadow hi
    ctx.set_state(hits=hits)
    got = check_against(ctx, tr, X, M, masked, hits, 2, "masked column, restricted")
    assert (got["bmu"][:4] == hi).all()
    ctx.close()


# ---- 4. NaN rules -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", [(po.STANDARD, 9, 15, 37), (po.MEDIAN, 7, 5, 9), (po.STANDARD, 7, 5, 70)])
def test_nan_rules(tr, W, H, J):
    ctx, X, M, hits = make(tr, W, H, J, seed=9)
    rng = np.random.default_rng(J)
    valid = rng.random((B, J)) < 0.7
    valid[:, 1] = True
    valid[:35, 4 % J] = False                          # column 4 % J: invalid for the first half of the rows
    M0 = M.copy()
    M0[0, 1] = np.nan                                  # NaN at a valid column of node 0: node 0, NaN distance
    ctx.set_state(map=M0)
    got = check_against(ctx, tr, X, M0, valid, hits, 0, "node 0 NaN")
    assert (got["bmu"] == 0).all() and (got["dist"].view(np.uint32) == QNAN).all()
    M1 = M.copy()
    M1[0, 4 % J] = np.nan                              # the same under an invalid column is ignored
    ctx.set_state(map=M1)
    got = check_against(ctx, tr, X, M1, valid, hits, 0, "node 0 NaN, masked")
    assert np.isfinite(got["dist"][:35]).all() and (got["bmu"][:35] != 0).any()
    assert (got["bmu"][35:][valid[35:, 4 % J]] == 0).all()
    ctx.set_state(map=M)
    winners = np.unique(ctx.bmu_masked(valid)["bmu"])
    winners = winners[winners != 0]
    M2 = M.copy()
    M2[winners.astype(np.int64), 1] = np.nan           # NaN at a valid column of another node: it never wins
    ctx.set_state(map=M2)
    got = check_against(ctx, tr, X, M2, valid, hits, 0, "other nodes NaN")
    assert not np.isin(got["bmu"], winners).any() and np.isfinite(got["dist"]).all()
    ctx.close()


# ---- 5. / 6. one_mask, sub-ranges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", SHAPES)
def test_one_mask_and_sub_ranges(tr, W, H, J):
    ctx, X, M, hits = make(tr, W, H, J, seed=11)
    rng = np.random.default_rng(J + 1)
    col = rng.random(J) < 0.6
    col[0] = True
    a = ctx.bmu_masked(col, min_hits=2, fill=True)
    b = ctx.bmu_masked(np.tile(col, (B, 1)), min_hits=2, fill=True)
    for k in a:
        assert bits_eq(a[k], b[k]) if a[k].dtype.kind == "f" else (a[k] == b[k]).all(), k
    assert (a["nvalid"] == col.sum()).all()
    valid = rng.random((B, J)) < 0.7
    full = ctx.bmu_masked(valid, min_hits=2, fill=True)
    for r0, r1 in ((0, 70), (5, 69), (64, 70)):
        part = ctx.bmu_masked(valid[r0:r1], r0, r1, min_hits=2, fill=True)
        one = ctx.bmu_masked(col, r0, r1, min_hits=2, fill=True)
        for k in part:
            eq = bits_eq if part[k].dtype.kind == "f" else (lambda x, y: (x == y).all())
            assert eq(part[k], full[k][r0:r1]), (k, r0, r1)
            assert eq(one[k], a[k][r0:r1]), (k, r0, r1)
    empty = ctx.bmu_masked(valid[7:7], 7, 7, fill=True)
    assert empty["bmu"].shape == (0,) and empty["fill"].shape == (0, J)
    out = capi.MaskedOut()
    v = np.ones(J, np.uint8)
    assert capi.lib().vsom_bmu_masked_batch(ctx._h, 0, 7, 7, v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 1,
                                            ctypes.byref(out)) == 0
    ctx.close()


# ---- 7. fill ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", [(po.STANDARD, 9, 15, 37), (po.MEDIAN, 7, 5, 9), (po.STANDARD, 7, 5, 3),
                                         (po.MEDIAN, 9, 15, 70)])
def test_fill_carries_bits(tr, W, H, J):
    ctx, X, M, hits = make(tr, W, H, J, seed=13)
    M = M.copy()
    M[:, J - 1] = np.float32(-0.0)                     # a -0.0 and a NaN (with a payload) in every model row,
    M[:, J - 2] = np.array([0x7FC01234], np.uint32).view(np.float32)[0]   # both under columns no row has valid
    X = X.copy()
    X[5, 0] = np.float32(-0.0)                         # and a -0.0 / a payload NaN among the values of x
    X[6, 0] = np.array([0xFFC00055], np.uint32).view(np.float32)[0]
    valid = np.random.default_rng(J).random((B, J)) < 0.6
    valid[:, J - 2:] = False
    valid[5, 0] = True
    valid[6, 0] = False
    ctx.set_state(map=M)
    ctx.upload_chunk(X)
    got = check_against(ctx, tr, X, M, valid, hits, 1, "fill")
    f = got["fill"].view(np.uint32)
    assert (f[:, J - 1] == 0x80000000).all() and (f[:, J - 2] == 0x7FC01234).all()
    assert f[5, 0] == 0x80000000 and f[6, 0] == M[int(got["bmu"][6]), 0].view(np.uint32)
    assert (got["nvalid"] == valid.sum(axis=1)).all()
    nofill = ctx.bmu_masked(valid, min_hits=1)
    assert nofill["fill"] is None and (nofill["bmu"] == got["bmu"]).all()
    ctx.close()


# ---- 8. read-only -------------------------------------------------------------------------------------------------------------
def assert_oracle_state(ctx, o, what):
    st = ctx.get_state()
    for k, ref in (("map", o.map), ("sigma", o.sigma), ("S", o.S), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], ref), (what, k)


@pytest.mark.parametrize("tr, W, H, J", [(po.STANDARD, 9, 15, 37), (po.MEDIAN, 7, 5, 9)])
def test_read_only(tr, W, H, J):
    X = gen.blobs(B, J, 4, 15, 2)
    init = gen.random_map(W * H, J, seed=16)
    ctx = vsom_amd.Context(W, H, J, tr)
    o = po.OracleSom(W, H, J, tr)
    ctx.set_state(map=init)
    o.set_state(map=init)
    ctx.upload_chunk(X)
    lbo = np.zeros(B, np.uint64)
    assert np.float32(ctx.batch_epoch(3.0, True)) == np.float32(o.batch_epoch(X, lbo, 3.0, True))
    before, lb, sq = ctx.get_state(), ctx.get_last_bmu(), ctx.get_sqres()
    valid = np.random.default_rng(3).random((B, J)) < 0.7
    a = ctx.bmu_masked(valid, min_hits=1, fill=True)
    b = ctx.bmu_masked(valid, min_hits=1, fill=True)
    ctx.bmu_masked(valid[0], fill=True)
    for k in a:
        assert bits_eq(a[k], b[k]) if a[k].dtype.kind == "f" else (a[k] == b[k]).all(), k
    after = ctx.get_state()
    for k in before:
        assert beq(before[k], after[k]), k
    assert (ctx.get_last_bmu() == lb).all() and (lb == lbo).all() and bits_eq(ctx.get_sqres(), sq)
    assert np.float32(ctx.batch_epoch(2.0, False)) == np.float32(o.batch_epoch(X, lbo, 2.0, False))
    assert_oracle_state(ctx, o, "the epoch after the masked calls")
    assert (ctx.get_last_bmu() == lbo).all()
    ctx.close()


# ---- 9. slicing ---------------------------------------------------------------------------------------------------------------
def test_row_slices(monkeypatch):
    """a slice forced to 100 rows (VSOM_MASKED_SLICE_ROWS, read at every call): 333 rows cross it three times, the last
    slice ragged in rows and in its row tile"""
    tr, W, H, J, rows = po.STANDARD, 9, 15, 37, 333
    ctx, X, M, hits = make(tr, W, H, J, seed=17, rows=rows)
    rng = np.random.default_rng(9)
    valid = rng.random((rows, J)) < 0.7
    col = rng.random(J) < 0.6
    masks = {"valid": valid, "col": col, "ones": np.ones((rows, J), bool)}
    whole = {k: ctx.bmu_masked(m, min_hits=2, fill=True) for k, m in masks.items()}
    monkeypatch.setenv("VSOM_MASKED_SLICE_ROWS", "100")
    sliced = {k: ctx.bmu_masked(m, min_hits=2, fill=True) for k, m in masks.items()}
    part = ctx.bmu_masked(valid[50:301], 50, 301, min_hits=2, fill=True)
    monkeypatch.delenv("VSOM_MASKED_SLICE_ROWS")
    ri, rd = ctx.bmu_restricted_batch(2)
    assert (sliced["ones"]["bmu"] == ri).all() and bits_eq(sliced["ones"]["dist"], rd)   # all-valid, every row
    for k in masks:
        for f in ("bmu", "nvalid"):
            assert (sliced[k][f] == whole[k][f]).all(), (k, f)
        for f in ("dist", "fill"):
            assert bits_eq(sliced[k][f], whole[k][f]), (k, f)
    assert (part["bmu"] == whole["valid"]["bmu"][50:301]).all() and bits_eq(part["fill"], whole["valid"]["fill"][50:301])
    sample = [0, 63, 64, 99, 100, 101, 127, 128, 199, 200, 255, 256, 299, 300, 320, 332]   # 16 rows around the boundaries
    eb, ed = checker(tr, X, M, valid, hits, 2, sample)
    assert (sliced["valid"]["bmu"][sample] == eb).all() and bits_eq(sliced["valid"]["dist"][sample], ed)
    eb, ed = checker(tr, X, M, col, hits, 2, sample)
    assert (sliced["col"]["bmu"][sample] == eb).all() and bits_eq(sliced["col"]["dist"][sample], ed)
    ctx.close()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    W, H, J = 6, 5, 7
    rows = 20
    init = gen.random_map(W * H, J, seed=1)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    L = capi.lib()
    u8 = ctypes.POINTER(ctypes.c_uint8)
    valid = np.ones((rows, J), np.uint8)
    bmu = np.zeros(rows, np.uint64)
    out = capi.MaskedOut()
    out.bmu = capi._u(bmu)

    def rc(r0, r1, h=ctx._h, v=valid, o=out):
        return L.vsom_bmu_masked_batch(h, 0, r0, r1, None if v is None else v.ctypes.data_as(u8), 0,
                                       None if o is None else ctypes.byref(o))

    def refused(code, word):
        assert code == -1, word
        assert word in L.vsom_last_error().decode(), (word, L.vsom_last_error().decode())

    refused(rc(0, 0), "no chunk")                      # no chunk loaded
    refused(rc(0, 1, h=None), "null context")
    X = gen.blobs(rows, J, 3, 1, 2)
    ctx.upload_chunk(X)
    good = ctx.bmu_masked(valid, fill=True)
    refused(rc(0, rows, v=None), "valid_host")
    refused(rc(0, rows, o=None), "out is null")
    for r0, r1 in ((5, 4), (0, rows + 1), (rows + 1, rows + 2)):
        refused(rc(r0, r1), "row range")
        again = ctx.bmu_masked(valid, fill=True)
        assert (again["bmu"] == good["bmu"]).all() and bits_eq(again["fill"], good["fill"])
    assert rc(3, 3) == 0                               # an empty range
    assert rc(0, rows) == 0 and (bmu == good["bmu"]).all()     # a single output pointer
    assert rc(0, rows, o=capi.MaskedOut()) == 0        # none at all
    o = po.OracleSom(W, H, J)
    o.set_state(map=init)
    lbo = np.zeros(rows, np.uint64)
    assert np.float32(ctx.batch_epoch(1.5, True)) == np.float32(o.batch_epoch(X, lbo, 1.5, True))
    assert_oracle_state(ctx, o, "after refusals")
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
        clr.bmu_masked(np.ones((rows, 5), np.uint8))
    assert np.float32(clr.batch_epoch(1.5, True)) == np.float32(oc.batch_epoch(Xc, lbo, 1.5, True))
    assert_oracle_state(clr, oc, "CLR after the refusal")
    clr.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_bmu_masked_batch"):
        cu.bmu_masked(np.ones((10, 5), np.uint8))
    cu.bmu_batch()
    cu.close()

    # a chunk staged ahead (as tests/test_gpu_bmd_batch.py): refused until it is committed
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
        big.bmu_masked(np.ones(J, np.uint8))
    big.commit_chunk()
    got = big.bmu_masked(np.ones(J, np.uint8), 0, 4)
    bi, bd = big.bmu_batch()
    assert (got["bmu"] == bi[:4]).all() and bits_eq(got["dist"], bd[:4])
    big.close()
    pb.free()


# ---- 11. mirrors --------------------------------------------------------------------------------------------------------------
class ValidDataSet(vs.ArrayDataSet):
    """an ArrayDataSet with validity flags"""

    def __init__(self, X, validity):
        super().__init__(X)
        self.validity = validity


def test_som_mirrors():
    W, H, F, C, rows = 9, 15, 12, 5, 70
    J = F + C
    feats = gen.blobs(rows, F, C, 2, 2)
    labels = np.arange(rows) % C
    X = np.concatenate([feats, np.eye(C, dtype=np.float32)[labels]], axis=1)    # one-hot label columns appended
    M, hits = state(W, H, J, 21)
    M[::2, F + 1] = M[::2, F + 3] = np.float32(2.0)    # every other node: two label columns tie for the largest value
    s = vs.Som(W, H, J)
    s.setState(map=M, hits=hits)
    cols = np.arange(F, J)
    colmask = np.ones(J, bool)
    colmask[cols] = False
    for min_hits in (0, 3):
        eb, ed = checker(po.STANDARD, X, M, colmask, hits, min_hits)
        lab, bmu = s.classify(X, cols, min_hits)
        assert (bmu == eb).all()
        want = np.array([int(np.argmax(M[int(b), F:])) for b in eb])
        assert (lab == want).all()
        # what the rows hold in the label columns does not matter
        X2 = X.copy()
        X2[:, F:] = np.nan
        lab2, bmu2 = s.classify(X2, cols, min_hits)
        assert (lab2 == lab).all() and (bmu2 == bmu).all()
        assert (lab[eb % 2 == 0] == 1).all() and (eb % 2 == 0).any()     # the lowest column on ties
    valid = np.random.default_rng(4).random((rows, J)) < 0.7
    ds = ValidDataSet(X, valid)
    ds.loadNextDataFromStream()
    rep = s.findBmuMasked(ds, 3)
    eb, ed = checker(po.STANDARD, X, M, valid, hits, 3)
    assert (rep["bmu"] == eb).all() and bits_eq(rep["dist"], ed) and (rep["nvalid"] == valid.sum(axis=1)).all()
    filled = s.impute(ds, 3)
    assert bits_eq(filled, s.ctx.bmu_masked(valid, min_hits=3, fill=True)["fill"])
    assert bits_eq(filled, np.where(valid, X, M[eb.astype(np.int64)]))
    plain = s.findBmuMasked(X, 3)                      # no validity attribute: every column counts
    s.ctx.upload_chunk(X)
    ri, rd = s.ctx.bmu_restricted_batch(3)
    assert (plain["bmu"] == ri).all() and bits_eq(plain["dist"], rd)
    s.close()


def test_cpp_mirror_driver():
    exe = os.path.join(HOST, "host_masked_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "state_downloads=0" in res.stdout
    assert "host_masked_test ok" in res.stdout
