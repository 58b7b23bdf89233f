"""GPU: vsom_bmu_topk_batch -- the k best matching units of chunk rows [r0, r1) in one call.  Lists are held bit for bit
against a numpy sort of the key (d, node) (NaN after +inf) over the oracle's distances of every node, with findBmu's
node-0 rule in front, and column 0 against vsom_bmu_batch in every search mode."""
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
import ties  # noqa: E402

pytestmark = pytest.mark.gpu
QNAN = np.uint32(0x7FC00000)


def beq(a, b):
    """bitwise equality; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()
    return (a == b).all()


def keys(d):
    """vsom_key over a row of fp32 distances: (bits, node), NaN -> 0xFFFFFFFF"""
    bits = d.view(np.uint32).astype(np.uint64)
    bits[np.isnan(d)] = 0xFFFFFFFF
    return (bits << np.uint64(32)) | np.arange(d.size, dtype=np.uint64)


def expected_row(d, k):
    """the contract on one row of distances d (fp32 of every node)"""
    order = np.argsort(keys(d), kind="stable")
    if np.isnan(d[0]):
        order = np.concatenate([[0], order[order != 0]])
    idx = order[:k].astype(np.uint64)
    dist = d[idx.astype(np.int64)].copy()
    dist[np.isnan(dist)] = QNAN.view(np.float32)
    return idx, dist


def oracle_dists(o, X):
    N = o.map.shape[0]
    return np.array([[o.dist(i, x) for i in range(N)] for x in X], np.float32)


def expected(D, k):
    idx = np.zeros((D.shape[0], k), np.uint64)
    dist = np.zeros((D.shape[0], k), np.float32)
    for r in range(D.shape[0]):
        idx[r], dist[r] = expected_row(D[r], k)
    return idx, dist


def check_list(ctx, D, k, r0=0, r1=None):
    r1 = D.shape[0] if r1 is None else r1
    idx, dist = ctx.bmu_topk(k, r0, r1)
    ei, ed = expected(D[r0:r1], k)
    assert (idx == ei).all(), (k, np.argwhere(idx != ei)[:4])
    assert beq(dist, ed), k
    assert (dist.view(np.uint32)[np.isnan(dist)] == QNAN).all()
    return idx, dist


def make(W, H, J, tr, B, seed=3):
    X = gen.blobs(B, J, 4, seed, 2) if tr != po.CLR else np.abs(gen.blobs(B, J, 4, seed, 2)) + 0.5
    o = po.OracleSom(W, H, J, tr)
    init = gen.random_map(W * H, o.depth, seed=seed + 10)
    o.set_state(map=init)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=init)
    ctx.upload_chunk(X)
    return ctx, o, X


# ---- 1. oracle parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J, B", [(po.STANDARD, 9, 11, 13, 70), (po.MEDIAN, 7, 11, 3, 33),
                                            (po.CLR, 5, 9, 7, 40), (po.STANDARD, 10, 9, 794, 20),
                                            (po.STANDARD, 8, 8, 5, 17), (po.CLR, 4, 4, 3, 9)])
def test_oracle_parity(tr, W, H, J, B):
    ctx, o, X = make(W, H, J, tr, B)
    D = oracle_dists(o, X)
    N = W * H
    for k in sorted({1, 2, 7, min(64, N), N if N <= 64 else 64}):
        check_list(ctx, D, k)
    ctx.close()


# ---- 2. agreement with vsom_bmu_batch --------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", [po.STANDARD, po.MEDIAN, po.CLR])
def test_column0_every_mode(tr):
    W, H, J, B = (24, 20, 40, 600) if tr != po.CLR else (16, 12, 8, 300)
    ctx, o, X = make(W, H, J, tr, B, seed=5)
    for mode in (capi.BMU_AUTO, capi.BMU_EXACT, capi.BMU_SHORTLIST):
        ctx.set_bmu_mode(mode)
        bi, bd = ctx.bmu_batch()
        for k in (1, 2, 16):
            idx, dist = ctx.bmu_topk(k)
            assert (idx[:, 0] == bi).all(), (mode, k)
            assert beq(dist[:, 0], bd), (mode, k)
    ctx.close()


def test_column0_compaction_and_dedupe():
    W, H, J, B = 32, 32, 64, 2048
    X = gen.blobs(B, J, 4, 9, 2)
    X[:, 10:30] = 0.0                                  # columns the compaction retires
    init = gen.random_map(W * H, J, seed=4)
    init[100:140] = init[7]                            # bit-identical rows: the dedupe pass's classes
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    ctx.set_column_compaction(1)
    ctx.set_row_dedupe(0)
    ctx.upload_chunk(X)
    for mode in (capi.BMU_AUTO, capi.BMU_EXACT):
        ctx.set_bmu_mode(mode)
        bi, bd = ctx.bmu_batch()
        idx, dist = ctx.bmu_topk(8)
        assert (idx[:, 0] == bi).all() and beq(dist[:, 0], bd)
    # a sample equal to the duplicated row: every copy appears, in index order
    ctx.upload_chunk(np.ascontiguousarray(init[[7, 7]]))
    idx, dist = ctx.bmu_topk(41)
    assert idx[0].tolist() == [7] + list(range(100, 140)) and (dist[0] == 0).all()
    ctx.close()


def test_c3_agreement_and_sampled_lists():
    W, H, J, B = 128, 128, 784, 4096
    X = gen.mnist_like(B, seed=2)
    init = gen.random_map(W * H, J, seed=8)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    ctx.upload_chunk(X)
    bi, bd = ctx.bmu_batch()
    for k in (2, 16):
        idx, dist = ctx.bmu_topk(k)
        assert (idx[:, 0] == bi).all() and beq(dist[:, 0], bd), k
    rows = np.random.RandomState(1).choice(B, 32, replace=False)
    idx, dist = ctx.bmu_topk(64)
    for r in rows:
        ei, ed = expected_row(ctx.distances_row(int(r)), 64)
        assert (idx[r] == ei).all() and beq(dist[r], ed), r
    ctx.close()


# ---- 3. ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data, tr", [("float", po.STANDARD), ("uint8", po.STANDARD), ("u8edge", po.STANDARD),
                                      ("cancel", po.STANDARD), ("float", po.CLR), ("float", po.MEDIAN)])
def test_ties_winner_and_runner_up(data, tr):
    if tr == po.CLR:
        case = ties.batch_case(16, 16, 6, 64, 7, tr=tr)
    else:
        case = ties.batch_case(32, 16, 40, 128, 7, data=data, tr=tr, decoys=3)
    ctx = vsom_amd.Context(case.W, case.H, case.J, case.tr)
    ctx.set_state(map=case.init)
    ctx.set_row_dedupe(0)
    ctx.upload_chunk(case.X)
    idx, dist = ctx.bmu_topk(3)
    bi, bd = ctx.bmu_batch()
    checked = 0
    for s, c in enumerate(case.certs):
        if c is None:
            continue
        assert int(idx[s, 0]) == c["winner"] and int(idx[s, 1]) == c["runner_up"], (s, c)
        assert beq(dist[s, :2], np.array(c["d32"], np.float32)), (s, c)
        checked += 1
    assert checked > 0
    assert (idx[:, 0] == bi).all() and beq(dist[:, 0], bd)
    ctx.close()


# ---- 4. NaN and inf --------------------------------------------------------------------------------------------------
def test_nan_and_inf():
    W, H, J, B = 9, 8, 12, 24
    ctx, o, X = make(W, H, J, po.STANDARD, B, seed=12)
    X = X.copy()
    X[3, 4] = np.nan                                    # a NaN row: every distance NaN -> node 0 first, then 1, 2, ...
    X[5, 0] = 3e38                                      # infinite distances
    init = o.map.copy()
    init[17, 2] = np.nan                                # a NaN model row elsewhere
    init[40, :] = 3e38                                  # infinite to every sample
    o.set_state(map=init)
    ctx.set_state(map=init)
    ctx.upload_chunk(X)
    D = oracle_dists(o, X)
    assert np.isnan(D[3]).all() and np.isinf(D).any()
    for k in (1, 2, 7, 64):
        idx, _ = check_list(ctx, D, k)
    assert idx[3].tolist()[:5] == [0, 1, 2, 3, 4]
    # node 0 NaN: entry 0 is node 0 with NaN, the rest in key order
    init0 = init.copy()
    init0[0, 1] = np.nan
    o.set_state(map=init0)
    ctx.set_state(map=init0)
    ctx.upload_chunk(X)
    D = oracle_dists(o, X)
    for k in (1, 2, 9, 64):
        idx, dist = check_list(ctx, D, k)
        assert (idx[:, 0] == 0).all() and np.isnan(dist[:, 0]).all()
    bi, bd = ctx.bmu_batch()
    assert (idx[:, 0] == bi).all() and beq(dist[:, 0], bd)
    ctx.close()


# ---- 5. edges --------------------------------------------------------------------------------------------------------
def test_ranges_and_tiny_shapes():
    ctx, o, X = make(12, 7, 10, po.STANDARD, 150, seed=21)
    D = oracle_dists(o, X)
    for r0, r1 in ((0, 1), (5, 70), (64, 128), (149, 150), (37, 37)):
        check_list(ctx, D, 5, r0, r1)
    idx, dist = ctx.bmu_topk(5, 40, 40)
    assert idx.shape == (0, 5) and dist.shape == (0, 5)
    ctx.upload_chunk(X[:1])
    check_list(ctx, D[:1], 64)
    ctx.close()
    one = vsom_amd.Context(1, 1, 4)
    one.set_state(map=np.ones((1, 4), np.float32))
    one.upload_chunk(np.zeros((3, 4), np.float32))
    idx, dist = one.bmu_topk(1)
    assert (idx == 0).all() and (dist == 4.0).all()
    one.close()


def test_several_slices():
    W, H, J, B = 128, 128, 24, 8192                    # k = 64: 2048 rows per slice
    X = gen.blobs(B, J, 6, 4, 2)
    init = gen.random_map(W * H, J, seed=6)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    ctx.upload_chunk(X)
    bi, bd = ctx.bmu_batch()
    idx, dist = ctx.bmu_topk(64)
    assert (idx[:, 0] == bi).all() and beq(dist[:, 0], bd)
    for r in (0, 2047, 2048, 4100, 8191):
        ei, ed = expected_row(ctx.distances_row(r), 64)
        assert (idx[r] == ei).all() and beq(dist[r], ed), r
    i2, d2 = ctx.bmu_topk(64, 2040, 6150)
    assert (i2 == idx[2040:6150]).all() and beq(d2, dist[2040:6150])
    ctx.close()


# ---- 6. read-only, deterministic -------------------------------------------------------------------------------------
def test_read_only_and_deterministic():
    W, H, J, B = 20, 16, 30, 500
    X = gen.blobs(B, J, 4, 8, 2)
    init = gen.random_map(W * H, J, seed=9)
    a, b = vsom_amd.Context(W, H, J), vsom_amd.Context(W, H, J)
    for c in (a, b):
        c.set_state(map=init)
        c.upload_chunk(X)
        c.batch_epoch(3.0, True)
    before = a.get_state()
    lb, sq = a.get_last_bmu(), a.get_sqres()
    i1, d1 = a.bmu_topk(10)
    i2, d2 = a.bmu_topk(10)
    assert (i1 == i2).all() and (d1.view(np.uint32) == d2.view(np.uint32)).all()
    after = a.get_state()
    for key in before:
        assert beq(before[key], after[key]), key
    assert (a.get_last_bmu() == lb).all() and beq(a.get_sqres(), sq)
    ma, mb = a.batch_epoch(2.0, False), b.batch_epoch(2.0, False)
    assert np.float32(ma) == np.float32(mb)
    sa, sb = a.get_state(), b.get_state()
    for key in sa:
        assert beq(sa[key], sb[key]), key
    assert (a.get_last_bmu() == b.get_last_bmu()).all()
    a.close()
    b.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    W, H, J, B = 6, 5, 7, 20
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=gen.random_map(W * H, J, seed=1))
    L = capi.lib()
    idx = np.zeros(64 * B, np.uint64)

    def rc(k, r0, r1, out=idx):
        return L.vsom_bmu_topk_batch(ctx._h, k, r0, r1, capi._u(out), None)

    assert rc(2, 0, 0) == -1                           # no chunk loaded
    X = gen.blobs(B, J, 3, 1, 2)
    ctx.upload_chunk(X)
    good = ctx.bmu_topk(3)
    for args in ((2, 5, 4), (2, 0, B + 1), (0, 0, B), (65, 0, B), (31, 0, B)):
        assert rc(*args) == -1, args
        i, d = ctx.bmu_topk(3)
        assert (i == good[0]).all() and beq(d, good[1])
    assert L.vsom_bmu_topk_batch(ctx._h, 2, 0, B, None, None) == -1    # no idx_out
    assert rc(2, 3, 3) == 0                            # an empty range
    i, d = ctx.bmu_topk(3)
    assert (i == good[0]).all() and beq(d, good[1])
    ctx.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_bmu_topk_batch"):
        cu.bmu_topk(2)
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
        big.bmu_topk(2)
    big.commit_chunk()
    i, d = big.bmu_topk(2, 0, 4)
    bi, bd = big.bmu_batch()
    assert (i[:, 0] == bi[:4]).all() and beq(d[:, 0], bd[:4])
    big.close()
    pb.free()


# ---- Som mirror ------------------------------------------------------------------------------------------------------
def test_som_mirror():
    W, H, J, B = 11, 6, 9, 90
    X = gen.blobs(B, J, 3, 2, 2)
    s = vs.Som(W, H, J)
    init = gen.random_map(W * H, J, seed=3)
    s.setState(map=init)
    o = po.OracleSom(W, H, J, po.STANDARD)
    o.set_state(map=init)
    D = oracle_dists(o, X)
    idx, dist = s.findBestMatchingUnits(X, 4, dist=True)
    ei, ed = expected(D, 4)
    assert (idx == ei).all() and beq(dist, ed)
    te = s.topographicError(X)
    assert te == vs.topographic_error(ei[:, :2], W)
    assert 0.0 <= te <= 1.0
    s.close()
