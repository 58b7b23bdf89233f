"""GPU: vsom_similarity_batch -- every chunk row searched and scored against its BMU in one call.  Expected values come
from a numpy fp32 restatement of Som::measureSimilarity (tests/similarity_ref.py) over the oracle's find_restricted_bmu,
map and sigma.  Everything is held bit for bit, NaN equal to NaN: the feature has no transcendental and no reordered sum."""
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
import similarity_ref as ref  # noqa: E402
from similarity_ref import beq  # noqa: E402

pytestmark = pytest.mark.gpu
ROW_KEYS = ("dmax", "dmax_col", "first", "amax", "amax_col", "outside")
ALL_KEYS = ("bmu", "dist") + ROW_KEYS
NEVER = 10 ** 9                                        # a hit count nothing reaches


def rows_for(tr, B, J, seed):
    X = gen.blobs(B, J, 4, seed, 2)
    return X if tr != po.CLR else (np.abs(X) + np.float32(0.5)).astype(np.float32)


def trained(tr, W, H, J, B, epochs=3, seed=3):
    """an oracle map after a few batch epochs (sigmaMap and bmuHits are real), the same state on the device, X staged"""
    X = rows_for(tr, B, J, seed)
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=gen.random_map(W * H, o.depth, seed=seed + 10))
    o.train_batch(X, [0, B], epochs, max(W, H) / 2.0, 0.3)
    ctx = vsom_amd.Context(W, H, J, tr)
    push(ctx, o)
    ctx.upload_chunk(X)
    return ctx, o, X


def push(ctx, o):
    ctx.set_state(map=o.map, sigma=o.sigma, S=o.S, weight=o.weight, hits=o.hits)


def oracle_bmus(o, X, min_hits):
    return np.array([o.find_restricted_bmu(x, min_hits) for x in X], np.uint64)


def expected(o, X, bmu, num_sigmas, floor, valid=None):
    C = min(o.in_len, o.depth)
    b = bmu.astype(np.int64)
    return ref.report(X[:, :C], o.map[b][:, :C], o.sigma[b][:, :C], num_sigmas, floor, valid)


def check(got, exp, bmu, what, delta=True):
    assert (got["bmu"] == bmu).all(), (what, np.flatnonzero(got["bmu"] != bmu)[:5])
    for k in ROW_KEYS:
        assert beq(got[k], exp[k]), (what, k, got[k][:8], exp[k][:8])
    if delta:
        assert beq(got["delta"], exp["delta"]), (what, "delta")
    else:
        assert got["delta"] is None
    for k in ("dist", "first"):                        # NaN is stored as the quiet NaN 0x7FC00000
        assert (got[k].view(np.uint32)[np.isnan(got[k])] == ref.QNAN).all(), (what, k)


def same(a, b, keys=ALL_KEYS + ("delta",)):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert beq(a[k], b[k]), k


# ---- 1. parity with the restated reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J, B", [(po.STANDARD, 9, 11, 13, 70), (po.MEDIAN, 7, 11, 3, 33), (po.CLR, 5, 9, 7, 40),
                                            (po.STANDARD, 10, 9, 794, 20), (po.STANDARD, 12, 5, 9, 64), (po.CLR, 4, 6, 3, 9),
                                            (po.MEDIAN, 6, 10, 130, 37), (po.CLR, 3, 3, 2, 11)])
def test_parity(tr, W, H, J, B):
    ctx, o, X = trained(tr, W, H, J, B)
    C = min(J, o.depth)
    rng = np.random.default_rng(J)
    valid = rng.random((B, J)) < 0.7
    valid[B // 2] = False                              # a row without a valid column
    assert o.sigma.max() > 1e-5 and o.hits.max() > 1
    for min_hits in (0, 1, NEVER):
        bmu = oracle_bmus(o, X, min_hits)
        if min_hits == NEVER:
            assert (bmu == 0).all()                    # nothing qualifies: node 0 seeds (Som.cpp:316-317)
        _, rd = ctx.bmu_restricted_batch(min_hits)
        for ns in (1, 3, 1000000):
            for floor in (False, True):
                for v in (None, valid):
                    exp = expected(o, X, bmu, ns, floor, v)
                    for delta in (False, True):
                        got = ctx.similarity(min_hits, ns, capi.SIGMA_FLOOR if floor else capi.SIGMA_AS_WRITTEN,
                                             valid=v, delta=delta)
                        check(got, exp, bmu, (min_hits, ns, floor, v is not None, delta), delta)
                        assert beq(got["dist"], rd)
                        if delta:
                            assert got["delta"].shape == (B, C)
    ctx.close()


# ---- 2. row ranges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J, B", [(po.STANDARD, 9, 7, 13, 70), (po.CLR, 5, 4, 5, 41), (po.STANDARD, 6, 6, 794, 23)])
def test_row_ranges_are_slices_of_the_whole_chunk(tr, W, H, J, B):
    ctx, o, X = trained(tr, W, H, J, B, seed=5)
    valid = np.random.default_rng(1).random((B, J)) < 0.6
    whole = ctx.similarity(1, 3, valid=valid, delta=True)
    for r0, r1 in ((0, 7), (B // 3, min(B // 3 + 17, B)), (B - 5, B), (4, 4), (0, 0), (B, B), (9, 10), (B - 1, B), (0, B), (1, B - 1)):
        part = ctx.similarity(1, 3, r0=r0, r1=r1, valid=valid[r0:r1], delta=True)
        for k in ALL_KEYS + ("delta",):
            assert part[k].shape[0] == r1 - r0
            assert beq(part[k], whole[k][r0:r1]), (k, r0, r1)
    ctx.close()


def test_dense_report_in_slices():
    """more rows than one slice of the dense report holds (64 MiB / (4 C) rows): C = 794 -> 21130 rows"""
    W, H, J, B = 4, 4, 794, 21130 + 517
    o = po.OracleSom(W, H, J)
    o.set_state(map=gen.random_map(W * H, J, seed=2), sigma=np.abs(gen.random_map(W * H, J, seed=3)) * np.float32(1e-5))
    X = np.tile(gen.blobs(997, J, 4, 7, 2), (B // 997 + 1, 1))[:B].copy()
    X[21129:21133, :5] = np.arange(20, dtype=np.float32).reshape(4, 5)      # rows around the slice boundary differ
    ctx = vsom_amd.Context(W, H, J)
    push(ctx, o)
    ctx.upload_chunk(X)
    got = ctx.similarity(0, 3, delta=True)
    rows = np.r_[0:40, 21100:21160, B - 40:B]
    bmu = oracle_bmus(o, X[rows], 0)
    exp = expected(o, X[rows], bmu, 3, True)
    assert (got["bmu"][rows] == bmu).all()
    for k in ROW_KEYS + ("delta",):
        assert beq(got[k][rows], exp[k]), k
    # every repeated row reports what its first copy reports
    assert beq(got["delta"][997:2 * 997], got["delta"][:997]) and beq(got["amax"][997:2 * 997], got["amax"][:997])
    ctx.close()


# ---- 3. engineered states ----------------------------------------------------------------------------------------------
def special_sigmas():
    f = np.float32
    e = f(0.00001)
    return np.array([0.0, 1e-42, 1.4e-45, e, np.nextafter(e, f(1)), np.nextafter(e, f(0)), np.nan, np.inf, -1.0, -0.0,
                     0.5, 3.0e-6, 2.0, 1e-30, -np.inf, 7.0e-3], np.float32)


@pytest.mark.parametrize("tr", [po.STANDARD, po.MEDIAN, po.CLR])
def test_engineered_sigma_map_and_rows(tr):
    W, H, J, B = 5, 4, (16 if tr != po.CLR else 6), 48
    o = po.OracleSom(W, H, J, tr)
    N, D = W * H, o.depth
    C = min(J, D)
    rng = np.random.default_rng(11)
    m = gen.random_map(N, D, seed=8)
    sp = special_sigmas()
    sg = np.stack([np.roll(np.resize(sp, D), n) for n in range(N)]).astype(np.float32)
    m[3, 1] = np.nan
    m[5, 2] = np.inf
    m[7, 0] = -np.inf
    hits = (np.arange(N) % 3).astype(np.uint64)
    o.set_state(map=m, sigma=sg, hits=hits)
    X = rows_for(tr, B, J, 4)
    X[:N] = m[:, :J] if tr != po.CLR else X[:N]        # rows that sit on a node: delta = 0 / 0-over-0 columns
    X[:N] = np.where(np.isfinite(X[:N]), X[:N], np.float32(0.25))
    X[2, 1] = np.nan
    X[4, 3] = np.inf
    X[6, 0] = -np.inf
    X[9, :] = np.nan
    for ns in (1, 3, 1000000, 0, -2):
        for floor in (False, True):
            Xc = X.copy()
            # rows exactly on lo / hi of their BMU's interval, and one ulp outside
            bm = oracle_bmus(o, Xc, 1).astype(np.int64)
            _, lo, hi = ref.columns(Xc[:, :C], o.map[bm][:, :C], o.sigma[bm][:, :C], ns, floor)
            for r, c, val in ((20, 0, hi[20, 0]), (21, 1, lo[21, 1]), (22, 2, np.nextafter(hi[22, 2], np.float32(np.inf))),
                              (23, 3, np.nextafter(lo[23, 3], np.float32(-np.inf)))):
                if np.isfinite(val):
                    Xc[r, c] = val
            ctx = vsom_amd.Context(W, H, J, tr)
            push(ctx, o)
            ctx.upload_chunk(Xc)
            valid = rng.random((B, J)) < 0.8
            for min_hits in (0, 1, 2):
                bmu = oracle_bmus(o, Xc, min_hits)
                for v in (None, valid):
                    got = ctx.similarity(min_hits, ns, capi.SIGMA_FLOOR if floor else capi.SIGMA_AS_WRITTEN, valid=v, delta=True)
                    check(got, expected(o, Xc, bmu, ns, floor, v), bmu, (tr, ns, floor, min_hits, v is not None))
            ctx.close()


def test_on_the_interval_bounds_counts_as_inside():
    W, H, J = 3, 3, 8
    o = po.OracleSom(W, H, J)
    m = gen.random_map(W * H, J, seed=2)
    sg = (np.abs(gen.random_map(W * H, J, seed=3)) + np.float32(0.01)).astype(np.float32)
    o.set_state(map=m, sigma=sg, hits=np.ones(W * H, np.uint64))
    k = np.float32(3)
    sk = (sg * k).astype(np.float32)
    up = np.float32(np.inf)
    X = np.concatenate([(m + sk).astype(np.float32), (m - sk).astype(np.float32),
                        np.nextafter((m + sk).astype(np.float32), up), np.nextafter((m - sk).astype(np.float32), -up)])
    ctx = vsom_amd.Context(W, H, J)
    push(ctx, o)
    ctx.upload_chunk(X)
    got = ctx.similarity(1, 3, capi.SIGMA_FLOOR, delta=True)
    bmu = oracle_bmus(o, X, 1)
    exp = expected(o, X, bmu, 3, True)
    check(got, exp, bmu, "bounds")
    own = bmu[:9] == np.arange(9)                      # rows whose BMU is the node they were built from
    assert own.any()
    assert (got["outside"][:9][own] == 0).all() and (got["outside"][9:18][bmu[9:18] == np.arange(9)] == 0).all()
    assert (got["outside"][18:27][bmu[18:27] == np.arange(9)] == J).all()
    ctx.close()


@pytest.mark.parametrize("tr", [po.STANDARD, po.CLR])
def test_nan_node_zero_pins_the_bmu(tr):
    ctx, o, X = trained(tr, 6, 5, 7, 30)
    o.map[0, 1] = np.nan
    push(ctx, o)
    for min_hits in (0, 1):
        bmu = oracle_bmus(o, X, min_hits)
        assert (bmu == 0).all()
        got = ctx.similarity(min_hits, 3, capi.SIGMA_AS_WRITTEN, delta=True)
        check(got, expected(o, X, bmu, 3, False), bmu, ("nan0", min_hits))
        assert np.isnan(got["dist"]).all()
        assert (got["delta"][:, 1] == 0).all() and (got["dmax_col"] != 1).all()
    ctx.close()


# ---- 4. search modes; agreement with the search calls --------------------------------------------------------------------
@pytest.mark.parametrize("tr", [po.STANDARD, po.MEDIAN, po.CLR])
def test_every_search_mode_and_the_state_the_search_leaves(tr):
    W, H, J, B = (24, 20, 40, 600) if tr != po.CLR else (16, 12, 8, 300)
    ctx, o, X = trained(tr, W, H, J, B, epochs=2, seed=5)
    base = None
    for mode in (capi.BMU_AUTO, capi.BMU_EXACT, capi.BMU_SHORTLIST):
        ctx.set_bmu_mode(mode)
        bi, bd = ctx.bmu_batch()
        ctx.set_last_bmu(np.zeros(B, np.uint64))
        got = ctx.similarity(0, 3, delta=True)
        assert (got["bmu"] == bi).all() and beq(got["dist"], bd), mode
        assert (ctx.get_last_bmu() == bi).all() and beq(ctx.get_sqres(), bd), mode
        ri, rd = ctx.bmu_restricted_batch(0)
        assert (ri == bi).all() and beq(rd, bd), mode
        if base is None:
            base = got
            bmu = oracle_bmus(o, X, 0)
            check(got, expected(o, X, bmu, 3, True), bmu, "auto")
        same(got, base)
        for min_hits in (1, 3):
            ri, rd = ctx.bmu_restricted_batch(min_hits)
            ctx.set_last_bmu(np.zeros(B, np.uint64))
            got = ctx.similarity(min_hits, 3, r0=5, r1=9)      # the search covers the whole chunk whatever the range
            assert (got["bmu"] == ri[5:9]).all() and beq(got["dist"], rd[5:9])
            assert (ctx.get_last_bmu() == ri).all() and beq(ctx.get_sqres(), rd)
    ctx.close()


# ---- 5. read-only ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", [po.STANDARD, po.CLR])
def test_read_only_and_an_epoch_afterwards(tr):
    W, H, J, B = 9, 8, 10, 120
    ctx, o, X = trained(tr, W, H, J, B)
    before = ctx.get_state()
    chunk = ctx.device_ptr(capi.BUF_CHUNK)
    for min_hits in (0, 2):
        ctx.similarity(min_hits, 3, valid=np.ones((B, J)), delta=True)
    after = ctx.get_state()
    for k in before:
        assert beq(before[k], after[k]), k
    assert ctx.device_ptr(capi.BUF_CHUNK) == chunk and ctx.chunk_size == B
    mse = ctx.batch_epoch(2.5, True)
    lbo = np.zeros(B, np.uint64)
    mse_o = o.batch_epoch(X, lbo, 2.5, True)
    st = ctx.get_state()
    assert (ctx.get_last_bmu() == lbo).all()
    for k, r in (("map", o.map), ("sigma", o.sigma), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], r), k
    assert np.float32(mse) == np.float32(mse_o)
    ctx.close()


# ---- 6. refusals, determinism ----------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    W, H, J, B = 6, 5, 7, 20
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=gen.random_map(W * H, J, seed=1), sigma=np.abs(gen.random_map(W * H, J, seed=2)))
    L = capi.lib()
    out = capi.SimilarityOut()
    amax = np.zeros(B, np.float32)
    out.amax = amax.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def rc(r0, r1, rule=capi.SIGMA_FLOOR, o=out):
        return L.vsom_similarity_batch(ctx._h, 1, 3, rule, r0, r1, None, None if o is None else ctypes.byref(o))

    assert rc(0, 0) == -1                              # no chunk loaded
    assert "no chunk" in L.vsom_last_error().decode()
    X = gen.blobs(B, J, 3, 1, 2)
    ctx.upload_chunk(X)
    good = ctx.similarity(1, 3, delta=True)
    for args in ((5, 4), (0, B + 1), (B + 1, B + 2), (0, B, 2), (0, B, -1), (0, B, capi.SIGMA_FLOOR, None)):
        assert rc(*args) == -1, args
        same(ctx.similarity(1, 3, delta=True), good)
    assert rc(3, 3) == 0                               # an empty range
    assert rc(0, B) == 0 and beq(amax, good["amax"])   # a single output pointer
    assert L.vsom_similarity_batch(ctx._h, 1, 3, 0, 0, B, None, ctypes.byref(capi.SimilarityOut())) == 0    # none at all
    for _ in range(3):                                 # repeated calls are deterministic
        same(ctx.similarity(1, 3, delta=True), good)
    ctx.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_similarity_batch"):
        cu.similarity(1, 3)
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
        big.similarity(0, 3)
    big.commit_chunk()
    got = big.similarity(0, 3, r0=0, r1=4)
    bi, bd = big.bmu_batch()
    assert (got["bmu"] == bi[:4]).all() and beq(got["dist"], bd[:4])
    big.close()
    pb.free()


# ---- 7. Som mirror ---------------------------------------------------------------------------------------------------------
class ValidDataSet(vs.ArrayDataSet):
    """an ArrayDataSet with validity flags"""

    def __init__(self, X, validity):
        super().__init__(X)
        self.validity = validity


def restated_measure(o, X, num_sigmas, min_hits, valid=None):
    """Som::measureSimilarity: the literal loop over the restated columns"""
    C = min(o.in_len, o.depth)
    b = oracle_bmus(o, X, min_hits).astype(np.int64)
    delta, lo, hi = ref.columns(X[:, :C], o.map[b][:, :C], o.sigma[b][:, :C], num_sigmas, False)
    return ref.literal_loop(delta, X[:, :C], lo, hi, None if valid is None else np.asarray(valid)[:, :C])


@pytest.mark.parametrize("tr, W, H, J, B", [(po.STANDARD, 9, 11, 13, 70), (po.MEDIAN, 7, 11, 3, 33), (po.CLR, 5, 9, 7, 40),
                                            (po.STANDARD, 10, 10, 9, 20)])
def test_som_measure_similarity(tr, W, H, J, B):
    ctx, o, X = trained(tr, W, H, J, B)
    ctx.close()
    t = {po.STANDARD: vs.Transformation.Standard(), po.MEDIAN: vs.Transformation.StandardMedianEstimator(),
         po.CLR: vs.Transformation.CombinatorialLinearRegression()}[tr]
    s = vs.Som(W, H, o.depth, t)
    s.setState(map=o.map, sigma=o.sigma, S=o.S, weight=o.weight, hits=o.hits)
    valid = np.random.default_rng(5).random((B, J)) < 0.5
    seen = set()
    for ns in (1, 3, 1000000):
        for min_hits in (0, 1, NEVER):
            row, ok = restated_measure(o, X, ns, min_hits)
            assert s.measureSimilarity(X, ns, min_hits) == ok, (ns, min_hits)
            ds = ValidDataSet(X, valid)
            ds.loadNextDataFromStream()
            rowv, okv = restated_measure(o, X, ns, min_hits, valid)
            assert s.measureSimilarity(ds, ns, min_hits) == okv, (ns, min_hits, "valid")
            rep = s.similarityRows(X, ns, min_hits, floor=False)
            assert vs.measure_similarity_from_rows(rep["first"], rep["dmax"], rep["outside"])[0] == row
            seen.update((ok, okv))
    # the user's mode: floor, anomaly score per row
    rep = s.similarityRows(X, 3, 1, valid=valid, delta=True)
    bmu = oracle_bmus(o, X, 1)
    check(rep, expected(o, X, bmu, 3, True, valid), bmu, "similarityRows")
    s.close()


def test_som_measure_similarity_engineered():
    """states where the verdict is True, where it is False, and where the first trigger is negative"""
    W, H, J = 4, 3, 5
    o = po.OracleSom(W, H, J)
    m = gen.random_map(W * H, J, seed=6)
    X = (m[[1, 5, 7, 10]] + np.float32(1e-7)).astype(np.float32)
    s = vs.Som(W, H, J)
    results = set()
    for sg in (0.0, 1e-42, 1e-6, 0.5, np.nan):
        sig = np.full((W * H, J), sg, np.float32)
        o.set_state(map=m, sigma=sig, hits=np.ones(W * H, np.uint64))
        s.setState(map=m, sigma=sig, hits=np.ones(W * H, np.uint64))
        for Xc in (X, m[[2, 3]].copy(), (X - np.float32(0.5)).astype(np.float32)):
            for ns in (1, 1000000):
                ok = restated_measure(o, Xc, ns, 1)[1]
                assert s.measureSimilarity(Xc, ns, 1) == ok, (sg, ns)
                results.add(ok)
    assert results == {True, False}
    s.close()
