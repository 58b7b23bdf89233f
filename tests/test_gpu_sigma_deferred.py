"""GPU: batch epochs whose sigmaMap stays pending (VSOM_SIGMA_LAZY; csrc/vsom_update.hip, include/vsom_hip.h) -- the
mean-only chain kernels run in place of the full ones and the last epoch's sigmaMap is produced when get_state asks for
it -- against the oracle and against a VSOM_SIGMA_EAGER context, bit for bit (NaN == NaN).

The map is 40x40x300: 25 node groups x 22 = 550 > VSOM_CHAIN_MAX_WAVES, so phase 2 takes the lane = node kernels.
  * B in {1, 33, 77, 200}: a last block of 1 / 1 / 13 / 8 samples, one block, several blocks of 32.
  * rows with dead columns and all-zero quads (column compaction on: cc_expand_kernel's map-only and sigma-only forms),
    and dense signed rows (compaction off: sigma_finalize_kernel at the materialisation).
  * sigma 10, and 1.5, where most nodes start with W = 0, c = 0/0: NaN rows, NaN in the dead columns too.
  * Standard in the three arithmetics, and Median.
Four epochs on alternating chunks without a read of the state in between (the MSE and lastBMU read-backs do not
count), then get_state.  Every case asserts through vsom_sigma_stats that the four epochs WERE deferred, three records
dropped and one materialised: a run that silently stayed eager fails.

What "equal to the oracle" means per arithmetic (the oracle has the reference's one arithmetic; include/vsom_hip.h,
vsom_update_mode): strict and Median -- everything, every bit; sigma-contracted -- lastBMU, MSE, map, weightMap, bmuHits
every bit, sigmaMap within 1e-5 relative plus what underflowing products may differ by (_close_sigma); contracted --
bit equality is impossible for fused arithmetic, and from the second epoch on the search runs on a map that differs by
rounding, so this REPLACES "bit for bit" there: a further LAZY context runs ONE epoch from the same map (deferred, then
get_state) and lastBMU, MSE, weightMap, bmuHits equal the oracle's every bit, map and sigmaMap lie within the mode's
documented bound, 1e-5 of max(|reference|, largest |sample value| of the column), element by element, NaN where NaN
(include/vsom_hip.h, VSOM_UPDATE_FMA; tests/test_gpu_fma_mode.py) -- at sigma = 1.5 with the underflow term of
_close_sigma added for sigmaMap.  LAZY against EAGER is every bit of everything over the four epochs in every arithmetic:
both run M's own operation sequence."""
import numpy as np
import pytest

import gen
import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
THREADS = max(1, min(64, po.max_threads()))
W, H, J = 40, 40, 300
SIGMAS = (10.0, 1.5)
BS = (1, 33, 77, 200)
EPOCHS = 4


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def _close_sigma(a, b, weight, B):
    """sigmaMap of the sigma-contracted arithmetic against the oracle's.  S = sum of (w*d)*d: the contracted chain fuses
    the last product into the addition, so per term it skips one rounding of the product -- relative 2^-24 where the
    product is a normal number, at most 2^-149 absolute where it underflows (sigma = 1.5: weights down to the denormals) --
    and rounds the sum as the strict chain does.  Hence |S' - S| <= 2e-5 S + B 2^-149 with the documented 1e-5 on
    sigmaMap = sqrt(S / W) (include/vsom_hip.h: proven (B+1) 2^-24), compared here on sigmaMap^2 = S / W; NaN where NaN."""
    a64, b64 = a.astype(np.float64) ** 2, b.astype(np.float64) ** 2
    nan = np.isnan(b64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = 2.0001e-5 * b64 + (B * 2.0 ** -149 / weight.astype(np.float64))[:, None]
    ok = np.abs(a64 - b64)[~nan] <= tol[~nan]
    return bool(ok.all() and np.isnan(a64[nan]).all())


def _within_fma_bound(a, b, X, extra=None):
    """the contracted arithmetic's documented bound after ONE epoch from a given map (include/vsom_hip.h, VSOM_UPDATE_FMA):
    |err| <= 1e-5 * max(|reference|, scale of the chain's operands = largest |sample value| of the column); NaN where NaN"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    sd = np.abs(X).max(axis=0)[None, :].astype(np.float64)
    tol = 1e-5 * np.maximum(np.abs(b64), sd)
    if extra is not None:
        tol = tol + extra
    nan = np.isnan(b64)
    return bool((np.abs(a64 - b64)[~nan] <= np.broadcast_to(tol, b64.shape)[~nan]).all() and np.isnan(a64[nan]).all())


def sparse_rows(B, seed):
    """uint8-valued rows, 19 % of the entries non-zero (43 % of the quads all zero), 56 columns dead in every row"""
    X = gen.mnist_like(B, seed, J)
    X[:, :24] = 0.0
    X[:, 140:152] = 0.0
    X[:, 280:] = 0.0
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


def _run(ctx, chunks, sigma):
    """the epochs with nothing between them but what leaves a sigmaMap pending: [(lastBMU, MSE)]"""
    out = []
    for e in range(EPOCHS):
        ctx.upload_chunk(chunks[e % 2])
        mse = ctx.batch_epoch(sigma, e == 0)
        out.append((ctx.get_last_bmu(), mse))
    return out


ARITH = {"strict": (po.STANDARD, capi.UPDATE_STRICT), "sigma": (po.STANDARD, capi.UPDATE_FMA_SIGMA),
         "contracted": (po.STANDARD, capi.UPDATE_FMA), "median": (po.MEDIAN, capi.UPDATE_STRICT)}


@pytest.mark.parametrize("arith", list(ARITH))
@pytest.mark.parametrize("data", ["sparse", "dense"])
def test_four_deferred_epochs_then_get_state(data, arith):
    tr, mode = ARITH[arith]
    rows, compaction = (sparse_rows, 1) if data == "sparse" else (dense_rows, -1)
    scale = np.float32(100) if data == "sparse" else np.float32(1)
    init = gen.random_map(W * H, J, 42) * scale
    for B in BS:
        chunks = [rows(B, 3), rows(B, 4)]
        if data == "sparse":
            assert all(gen.column_occupancy(X)[0] <= J - 56 for X in chunks)
        for sigma in SIGMAS:
            tag = (data, arith, B, sigma)
            lazy = _context(tr, mode, capi.SIGMA_LAZY, compaction, init)
            eager = _context(tr, mode, capi.SIGMA_EAGER, compaction, init)
            got, ref = _run(lazy, chunks, sigma), _run(eager, chunks, sigma)
            stats = lazy.sigma_stats()
            assert stats == {"deferred": EPOCHS, "dropped": EPOCHS - 1, "materialised": 0, "pending": True}, (tag, stats)
            st = lazy.get_state(S=False)
            stats = lazy.sigma_stats()
            assert stats == {"deferred": EPOCHS, "dropped": EPOCHS - 1, "materialised": 1, "pending": False}, (tag, stats)
            assert eager.sigma_stats()["deferred"] == 0, tag
            st_e = eager.get_state(S=False)
            for e in range(EPOCHS):
                assert _same(got[e][0], ref[e][0]) and _same(got[e][1], ref[e][1]), (tag, "eager", e)
            for k in ("map", "sigma", "weight", "hits"):
                assert _same(st[k], st_e[k]), (tag, "eager", k)
            lazy.close()
            eager.close()

            orc = po.OracleSom(W, H, J, tr)
            orc.set_state(map=init)
            if arith == "contracted":
                one = _context(tr, mode, capi.SIGMA_LAZY, compaction, init)
                one.upload_chunk(chunks[0])
                mse_g = one.batch_epoch(sigma, True)
                lb_g = one.get_last_bmu()
                assert one.sigma_stats() == {"deferred": 1, "dropped": 0, "materialised": 0, "pending": True}, tag
                st1 = one.get_state(S=False)
                assert one.sigma_stats()["materialised"] == 1, tag
                one.close()
                lb = np.zeros(B, np.uint64)
                mse_o = orc.batch_epoch(chunks[0], lb, sigma, True, nthreads=THREADS)
                assert _same(lb_g, lb) and _same(mse_g, np.float32(mse_o)), (tag, "oracle")
                assert _same(lb_g, got[0][0]) and _same(mse_g, got[0][1]), (tag, "first of four")
                assert _same(st1["weight"], orc.weight) and _same(st1["hits"], orc.hits), (tag, "oracle")
                assert _within_fma_bound(st1["map"], orc.map, chunks[0]), (tag, "oracle", "map")
                # sigmaMap^2 = S / W: where products underflow (sigma = 1.5) S may differ by B 2^-149 (_close_sigma), i.e.
                # sigmaMap by at most sqrt(B 2^-149 / W)
                with np.errstate(divide="ignore", invalid="ignore"):
                    under = np.sqrt(B * 2.0 ** -149 / orc.weight.astype(np.float64))[:, None]
                under = np.where(np.isfinite(under), under, 0.0)
                assert _within_fma_bound(st1["sigma"], orc.sigma, chunks[0], under), (tag, "oracle", "sigma")
                continue
            for e in range(EPOCHS):
                lb = np.zeros(B, np.uint64)
                mse_o = orc.batch_epoch(chunks[e % 2], lb, sigma, e == 0, nthreads=THREADS)
                assert _same(got[e][0], lb) and _same(got[e][1], np.float32(mse_o)), (tag, "oracle", e)
            for k, o in (("map", orc.map), ("weight", orc.weight), ("hits", orc.hits)):
                assert _same(st[k], o), (tag, "oracle", k)
            if arith == "sigma":
                assert _close_sigma(st["sigma"], orc.sigma, orc.weight, B), (tag, "oracle", "sigma")
            else:
                assert _same(st["sigma"], orc.sigma), (tag, "oracle", "sigma")
            if sigma == 1.5:
                assert np.isnan(st["map"]).all(axis=1).any()        # the 0/0 rows are there
