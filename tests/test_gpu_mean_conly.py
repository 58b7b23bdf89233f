"""GPU: deferred batch epochs on the c-only operand array (csrc/vsom_update.hip: cwp_kernel's c-only form, the mean-only
chain kernels of csrc/gen_nt_asm.py that stage it, and the materialisation that runs the neighbourhood pass again in its full
form from the epoch's sigma and an owned copy of its lastBMU) -- against the oracle AND against a VSOM_SIGMA_EAGER context,
bit for bit (NaN == NaN).

The map is 41x39x300, LAZY: 1599 nodes = 24 full node groups and one of 63; 25 x 22 = 550 > VSOM_CHAIN_MAX_WAVES, so phase 2
takes the lane = node kernels.
  * B in {1, 2, 3, 4, 5, 31, 32, 33, 34, 35, 63, 64, 65, 130}: every sample-quad tail of the float4 packing, both sides of a
    32-sample block boundary, a lone last block, one block exactly.
  * sparse rows (column compaction on) whose live columns are cut to 269 = 4k+1 (68 quads: a dead quad inside a live
    block), 100 = 8k+4 (25 quads: an odd count) and 257 = 32k+1 (65 quads: a block with one live quad); dense signed rows
    (compaction off) at B in {3, 33, 65}.  Two epochs on alternating chunks, then get_state.
  * Standard strict / sigma-contracted / contracted, and Median, at B in {5, 77}, sigma 10 and 1.5 (NaN rows from c = 0/0).
  * the owned lastBMU and the epoch's table are what the materialisation uses: another chunk is staged, committed and
    searched (none of which reads sigmaMap) before get_state; and a partial-range phase 2 at another sigma materialises first.
Every case asserts through vsom_sigma_stats that the epochs WERE deferred and one record materialised.

"Equal to the oracle" per arithmetic is what tests/test_gpu_sigma_deferred.py's docstring says, with the same bounds:
strict and Median every bit; sigma-contracted every bit but sigmaMap, which lies within 1e-5 relative plus the underflow
term (_close_sigma); contracted: ONE deferred epoch, lastBMU / MSE / weightMap / bmuHits every bit, map and sigmaMap within
1e-5 of max(|reference|, largest |sample value| of the column), at sigma 1.5 plus the underflow term for sigmaMap.  LAZY
against EAGER is every bit of everything in every arithmetic."""
import numpy as np
import pytest
import torch

import gen
import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
THREADS = max(1, min(64, po.max_threads()))
W, H, J = 41, 39, 300
N = W * H
BS = (1, 2, 3, 4, 5, 31, 32, 33, 34, 35, 63, 64, 65, 130)
CUTS = (269, 100, 257)                     # live columns: 4k+1, 8k+4, 32k+1
DEAD = (8, 20)                             # dead columns inside the live range
INIT_SPARSE = gen.random_map(N, J, 42) * np.float32(100)
INIT_DENSE = gen.random_map(N, J, 42)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def _close_sigma(a, b, weight, B):
    """tests/test_gpu_sigma_deferred.py, _close_sigma: |S' - S| <= 2e-5 S + B 2^-149, compared on sigmaMap^2 = S / W"""
    a64, b64 = a.astype(np.float64) ** 2, b.astype(np.float64) ** 2
    nan = np.isnan(b64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = 2.0001e-5 * b64 + (B * 2.0 ** -149 / weight.astype(np.float64))[:, None]
    ok = np.abs(a64 - b64)[~nan] <= tol[~nan]
    return bool(ok.all() and np.isnan(a64[nan]).all())


def _within_fma_bound(a, b, X, extra=None):
    """tests/test_gpu_sigma_deferred.py, _within_fma_bound: the contracted arithmetic's documented bound after ONE epoch"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    sd = np.abs(X).max(axis=0)[None, :].astype(np.float64)
    tol = 1e-5 * np.maximum(np.abs(b64), sd)
    if extra is not None:
        tol = tol + extra
    nan = np.isnan(b64)
    return bool((np.abs(a64 - b64)[~nan] <= np.broadcast_to(tol, b64.shape)[~nan]).all() and np.isnan(a64[nan]).all())


def sparse_rows(B, seed, live):
    """uint8-valued rows with all-zero quads whose live columns are exactly [0, live + 12) without DEAD: `live` of them"""
    X = gen.mnist_like(B, seed, J)
    end = live + DEAD[1] - DEAD[0]
    for d in np.nonzero(~(X[:, :end] != 0).any(axis=0))[0]:      # every column below the cut is live in some row
        X[d % B, d] = np.float32(1 + d % 7)
    X[:, DEAD[0]:DEAD[1]] = 0.0
    X[:, end:] = 0.0
    assert gen.column_occupancy(X)[0] == live
    return X


def dense_rows(B, seed):
    return gen.blobs(B, J, 8, 1, seed, sigma=0.5)


def _context(tr, mode, sigma_mode, compaction, init):
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_sigma_mode(sigma_mode)
    ctx.set_update_mode(mode)
    ctx.set_column_compaction(compaction)
    ctx.set_state(map=init)
    return ctx


def _run(ctx, chunks, sigma, epochs):
    out = []
    for e in range(epochs):
        ctx.upload_chunk(chunks[e % 2])
        mse = ctx.batch_epoch(sigma, e == 0)
        out.append((ctx.get_last_bmu(), mse))
    return out


_oracle = {}


def oracle_run(key, tr, init, chunks, sigma, epochs):
    """the oracle after `epochs` epochs on alternating chunks, computed once per key: ([(lastBMU, MSE)], state)"""
    if key not in _oracle:
        orc = po.OracleSom(W, H, J, tr)
        orc.set_state(map=init)
        res = []
        for e in range(epochs):
            X = chunks[e % 2]
            lb = np.zeros(X.shape[0], np.uint64)
            mse = orc.batch_epoch(X, lb, sigma, e == 0, nthreads=THREADS)
            res.append((lb, np.float32(mse)))
        _oracle[key] = (res, {"map": orc.map.copy(), "sigma": orc.sigma.copy(), "weight": orc.weight.copy(),
                              "hits": orc.hits.copy()})
    return _oracle[key]


def _two_epochs(tag, tr, mode, compaction, init, chunks, sigma, epochs=2):
    """LAZY and EAGER through `epochs` epochs and a get_state; the stats prove the deferral; -> (lazy results, lazy state)"""
    lazy = _context(tr, mode, capi.SIGMA_LAZY, compaction, init)
    eager = _context(tr, mode, capi.SIGMA_EAGER, compaction, init)
    got, ref = _run(lazy, chunks, sigma, epochs), _run(eager, chunks, sigma, epochs)
    stats = lazy.sigma_stats()
    assert stats == {"deferred": epochs, "dropped": epochs - 1, "materialised": 0, "pending": True}, (tag, stats)
    st = lazy.get_state(S=False)
    stats = lazy.sigma_stats()
    assert stats == {"deferred": epochs, "dropped": epochs - 1, "materialised": 1, "pending": False}, (tag, stats)
    assert eager.sigma_stats()["deferred"] == 0, tag
    st_e = eager.get_state(S=False)
    for e in range(epochs):
        assert _same(got[e][0], ref[e][0]) and _same(got[e][1], ref[e][1]), (tag, "eager", e)
    for k in ("map", "sigma", "weight", "hits"):
        assert _same(st[k], st_e[k]), (tag, "eager", k)
    lazy.close()
    eager.close()
    return got, st


def _equals_oracle(tag, got, st, orc_res, orc_st):
    for e in range(len(got)):
        assert _same(got[e][0], orc_res[e][0]) and _same(got[e][1], orc_res[e][1]), (tag, "oracle", e)
    for k in ("map", "sigma", "weight", "hits"):
        assert _same(st[k], orc_st[k]), (tag, "oracle", k)


@pytest.mark.parametrize("live", CUTS)
def test_sample_quad_tails_sparse(live):
    for B in BS:
        chunks = [sparse_rows(B, 3, live), sparse_rows(B, 4, live)]
        tag = ("sparse", live, B)
        got, st = _two_epochs(tag, po.STANDARD, capi.UPDATE_STRICT, 1, INIT_SPARSE, chunks, 10.0)
        _equals_oracle(tag, got, st, *oracle_run(tag, po.STANDARD, INIT_SPARSE, chunks, 10.0, 2))


def test_sample_quad_tails_dense():
    for B in (3, 33, 65):
        chunks = [dense_rows(B, 3), dense_rows(B, 4)]
        tag = ("dense", B)
        got, st = _two_epochs(tag, po.STANDARD, capi.UPDATE_STRICT, -1, INIT_DENSE, chunks, 10.0)
        _equals_oracle(tag, got, st, *oracle_run(tag, po.STANDARD, INIT_DENSE, chunks, 10.0, 2))


ARITH = {"strict": (po.STANDARD, capi.UPDATE_STRICT), "sigma": (po.STANDARD, capi.UPDATE_FMA_SIGMA),
         "contracted": (po.STANDARD, capi.UPDATE_FMA), "median": (po.MEDIAN, capi.UPDATE_STRICT)}


@pytest.mark.parametrize("arith", list(ARITH))
def test_arithmetics(arith):
    tr, mode = ARITH[arith]
    for B in (5, 77):
        chunks = [sparse_rows(B, 3, CUTS[0]), sparse_rows(B, 4, CUTS[0])]
        for sigma in (10.0, 1.5):
            tag = (arith, B, sigma)
            got, st = _two_epochs(tag, tr, mode, 1, INIT_SPARSE, chunks, sigma)
            if sigma == 1.5:
                assert np.isnan(st["map"]).all(axis=1).any()        # the 0/0 rows are there
            if arith == "contracted":
                # bit equality with the oracle is impossible for fused arithmetic: ONE deferred epoch within the mode's bound
                (lb, mse_o), = oracle_run(("arith1", B, sigma), tr, INIT_SPARSE, chunks, sigma, 1)[0]
                orc = oracle_run(("arith1", B, sigma), tr, INIT_SPARSE, chunks, sigma, 1)[1]
                one = _context(tr, mode, capi.SIGMA_LAZY, 1, INIT_SPARSE)
                one.upload_chunk(chunks[0])
                mse_g = one.batch_epoch(sigma, True)
                lb_g = one.get_last_bmu()
                assert one.sigma_stats() == {"deferred": 1, "dropped": 0, "materialised": 0, "pending": True}, tag
                st1 = one.get_state(S=False)
                assert one.sigma_stats()["materialised"] == 1, tag
                one.close()
                assert _same(lb_g, lb) and _same(mse_g, mse_o), (tag, "oracle")
                assert _same(lb_g, got[0][0]) and _same(mse_g, got[0][1]), (tag, "first of two")
                assert _same(st1["weight"], orc["weight"]) and _same(st1["hits"], orc["hits"]), (tag, "oracle")
                assert _within_fma_bound(st1["map"], orc["map"], chunks[0]), (tag, "oracle", "map")
                with np.errstate(divide="ignore", invalid="ignore"):
                    under = np.sqrt(B * 2.0 ** -149 / orc["weight"].astype(np.float64))[:, None]
                under = np.where(np.isfinite(under), under, 0.0)
                assert _within_fma_bound(st1["sigma"], orc["sigma"], chunks[0], under), (tag, "oracle", "sigma")
                continue
            key = ("arith2", "median" if arith == "median" else "standard", B, sigma)
            orc_res, orc_st = oracle_run(key, tr, INIT_SPARSE, chunks, sigma, 2)
            for e in range(2):
                assert _same(got[e][0], orc_res[e][0]) and _same(got[e][1], orc_res[e][1]), (tag, "oracle", e)
            for k in ("map", "weight", "hits"):
                assert _same(st[k], orc_st[k]), (tag, "oracle", k)
            if arith == "sigma":
                assert _close_sigma(st["sigma"], orc_st["sigma"], orc_st["weight"], B), (tag, "oracle", "sigma")
            else:
                assert _same(st["sigma"], orc_st["sigma"]), (tag, "oracle", "sigma")


# ---- the materialisation takes the epoch's OWN lastBMU and table ---------------------------------------------------
B3 = 77
XA, XB = sparse_rows(B3, 3, CUTS[0]), sparse_rows(B3, 4, 200)


def _pair_after_epoch(sigma):
    lazy = _context(po.STANDARD, capi.UPDATE_STRICT, capi.SIGMA_LAZY, 1, INIT_SPARSE)
    eager = _context(po.STANDARD, capi.UPDATE_STRICT, capi.SIGMA_EAGER, 1, INIT_SPARSE)
    for c in (lazy, eager):
        c.upload_chunk(XA)
        c.batch_epoch(sigma, True)
    s = lazy.sigma_stats()
    assert s == {"deferred": 1, "dropped": 0, "materialised": 0, "pending": True}, s
    assert eager.sigma_stats()["deferred"] == 0
    return lazy, eager


def test_materialisation_uses_the_owned_last_bmu():
    """a DIFFERENT chunk staged ahead, committed and searched while the record is pending: lastBMU, the live-column record
    and the staged rows are all the second chunk's when get_state materialises the FIRST chunk's epoch"""
    lazy, eager = _pair_after_epoch(10.0)
    t = torch.from_numpy(XB).cuda()
    lbs = []
    for c in (lazy, eager):
        c.stage_next_device(t.data_ptr(), B3)
        c.commit_chunk()
        c.batch_phase1_async(0, B3, False)
        c.synchronize()
        lbs.append(c.get_last_bmu())
    s = lazy.sigma_stats()
    assert s["pending"] and s["materialised"] == 0, s             # all three calls are on the keep list
    assert _same(lbs[0], lbs[1])
    orc_res, orc_st = oracle_run(("own", 10.0), po.STANDARD, INIT_SPARSE, [XA, XA], 10.0, 1)
    assert not _same(lbs[0], orc_res[0][0])                       # lastBMU really is another chunk's now
    a, b = lazy.get_state(S=False), eager.get_state(S=False)
    s = lazy.sigma_stats()
    assert s == {"deferred": 1, "dropped": 0, "materialised": 1, "pending": False}, s
    for k in ("map", "sigma", "weight"):
        assert _same(a[k], b[k]), ("eager", k)
        assert _same(a[k], orc_st[k]), ("oracle", k)
    lazy.close()
    eager.close()


def test_partial_phase2_at_another_sigma_materialises_first():
    """a deferred epoch at sigma 3, then a partial-range phase 2 at sigma 7: a new table -- the pending epoch's sigmaMap
    must come from the table of sigma 3.  Outside the range the rows are the oracle's epoch; inside, the EAGER context's."""
    lazy, eager = _pair_after_epoch(3.0)
    n0, n1 = 64, 640
    for c in (lazy, eager):
        c.batch_phase2_async(7.0, n0, n1)
        c.synchronize()
    s = lazy.sigma_stats()
    assert s == {"deferred": 1, "dropped": 0, "materialised": 1, "pending": False}, s
    a, b = lazy.get_state(S=False), eager.get_state(S=False)
    for k in ("map", "sigma", "weight", "hits"):
        assert _same(a[k], b[k]), ("eager", k)
    orc_st = oracle_run(("own", 3.0), po.STANDARD, INIT_SPARSE, [XA, XA], 3.0, 1)[1]
    out = np.r_[0:n0, n1:N]
    for k in ("map", "sigma", "weight"):
        assert _same(a[k][out], orc_st[k][out]), ("oracle", k)
    assert not _same(a["sigma"][n0:n1], orc_st["sigma"][n0:n1])   # the range itself was rewritten at sigma 7
    lazy.close()
    eager.close()
