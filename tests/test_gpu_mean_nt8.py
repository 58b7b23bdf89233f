"""GPU: the mean-only chain kernels with TWO column quads per wavefront (csrc/gen_nt_asm.py, layout K2: the `_nt8` kernels
that vsom_update.hip launches for a deferred epoch) -- LAZY against a VSOM_SIGMA_EAGER context and against the oracle, bit for
bit (NaN == NaN), after one epoch and after a schedule of three, get_state after vsom_sigma_flush.

Every test runs on two maps.
  * 41x39 (1599 nodes = 24 full node groups and one of 63), depth 300 for the sparse rows.  vsom_phase2_plan chooses the kernel by
    launch size (`_nt8` above two thirds of a round of 1024 workgroups): this map's launches are at most 25 x 10 workgroups
    and take the one-quad `_nt4` kernels.
  * 210x209 (43890 nodes = 685 full node groups and one of 50), depth 96 for the sparse rows: 686 workgroups per column
    block, so every launch, also of a single column block, takes the `_nt8` kernels.  This is the map that tests them.
`geometry` asserts both statements from a mirror of the rule.  What the library cannot tell a test is WHICH kernel ran: the
cases prove through vsom_sigma_stats that the epochs were deferred, which implies `_nt8` on the large map in a release
build -- not in a development build run with VSOM_MEAN_NT4 set, which forces `_nt4`.

Phase 2 must take the lane = node kernels: at depth 300 the small map does (25 x 22 = 550 > VSOM_CHAIN_MAX_WAVES), the large one
at every depth from 4 on (686 > 448); the small map's dense cases at small depths run with VSOM_NO_CHAIN=1 (read when the
context is created), which sends small maps down the same path.  Every context asserts through vsom_small_map_chains that
the small-map kernel is NOT taken.

  * quad counts: 1 (one wavefront, its second quad dead), 9 (odd: a live / dead wavefront in the second block), 8 (one full
    block), 10 = 8k + 2 (three all-dead wavefronts in the last block) -- as live-column counts 3, 36, 32, 40 of sparse rows
    with the column compaction, and as dense rows of depth 4, 36, 32, 40 without it (36 and 4 are 0 mod 4 but not mod 8).
  * B in {1, 3, 4, 5, 31, 32, 33, 64, 67}: the last block's exits at every position of a group, a lone block, one and two
    blocks exactly.
  * the zero-form dispatch: rows in which, sample by sample, quads 2k and 2k+1 are all zero / not, in all four combinations
    at each of the four positions of a group (asserted from the inputs), zero quads holding -0.0, and NaN / +-inf in one
    quad of a pair only.
  * strict, sigma-contracted, contracted (one epoch within the documented 1e-5 of the oracle, every bit against EAGER) and
    Median.
  * after a mean-only epoch the materialisation runs the full `_nt4` kernel from the rebuilt (c,w) array: sigmaMap AND map
    (which that kernel stores again) equal EAGER's, every bit -- checked by _lazy_eager in every case.

Bounds per arithmetic are those of tests/test_gpu_mean_conly.py's docstring."""
import numpy as np
import pytest

import gen
import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
THREADS = max(1, min(64, po.max_threads()))
MAPS = {"41x39": (41, 39, 300), "210x209": (210, 209, 96)}     # W, H, depth of the sparse rows
W, H, J = MAPS["41x39"]
N = W * H
BS = (1, 3, 4, 5, 31, 32, 33, 64, 67)
QUAD_CASES = {1: 3, 9: 36, 8: 32, 10: 40}            # quads -> live columns (sparse) / depth (dense; 1 quad: depth 4)
SCHEDULE = (10.0, 6.0, 3.0)


def two_quad_form(workgroups):
    """csrc/vsom_phase2_plan.hpp, vsom_phase2_plan (pinned by tests/test_phase2_plan.py): more than two thirds of a round of 1024 workgroups"""
    return 3 * workgroups > 2 * 1024


@pytest.fixture(params=list(MAPS), autouse=True)
def geometry(request):
    global W, H, J, N
    W, H, J = MAPS[request.param]
    N = W * H
    groups = (N + 63) // 64
    if request.param == "41x39":
        assert not two_quad_form(groups * ((300 // 4 + 7) // 8))    # the most column blocks any case here launches
    else:
        assert two_quad_form(groups)                                # one column block already
    yield request.param
    W, H, J = MAPS["41x39"]
    N = W * H


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


def init_map(depth, sparse):
    m = gen.random_map(N, depth, 42)
    return m * np.float32(100) if sparse else m


def sparse_rows(B, seed, live):
    """uint8-valued rows with all-zero quads whose live columns are exactly [0, live)"""
    X = gen.mnist_like(B, seed, J)
    for d in np.nonzero(~(X[:, :live] != 0).any(axis=0))[0]:      # every column below the cut is live in some row
        X[d % B, d] = np.float32(1 + d % 7)
    X[:, live:] = 0.0
    assert gen.column_occupancy(X)[0] == live
    return X


def dense_rows(B, seed, depth):
    return gen.blobs(B, depth, 8, 1, seed, sigma=0.5)


def _context(tr, mode, sigma_mode, compaction, init):
    depth = init.shape[1]
    ctx = vsom_amd.Context(W, H, depth, tr)
    assert capi.lib().vsom_small_map_chains(ctx._h, N) == 0, "phase 2 would take the small-map chain kernel"
    ctx.set_sigma_mode(sigma_mode)
    ctx.set_update_mode(mode)
    ctx.set_column_compaction(compaction)
    ctx.set_state(map=init)
    return ctx


def _run(ctx, chunks, sigmas):
    out = []
    for e, sigma in enumerate(sigmas):
        ctx.upload_chunk(chunks[e % 2])
        mse = ctx.batch_epoch(sigma, e == 0)
        out.append((ctx.get_last_bmu(), mse))
    return out


_oracle = {}


def oracle_run(key, tr, init, chunks, sigmas):
    """the oracle after the epochs of `sigmas` on alternating chunks, computed once per key: ([(lastBMU, MSE)], state)"""
    key = (W, H, key)
    if key not in _oracle:
        orc = po.OracleSom(W, H, init.shape[1], tr)
        orc.set_state(map=init)
        res = []
        for e, sigma in enumerate(sigmas):
            X = chunks[e % 2]
            lb = np.zeros(X.shape[0], np.uint64)
            mse = orc.batch_epoch(X, lb, sigma, e == 0, nthreads=THREADS)
            res.append((lb, np.float32(mse)))
        _oracle[key] = (res, {"map": orc.map.copy(), "sigma": orc.sigma.copy(), "weight": orc.weight.copy(),
                              "hits": orc.hits.copy()})
    return _oracle[key]


def _lazy_eager(tag, tr, mode, compaction, init, chunks, sigmas):
    """LAZY and EAGER through the epochs, vsom_sigma_flush and a get_state; the stats prove the deferral (so a mean-only
    kernel ran every epoch: `_nt8` on the large map) and that the flush materialised with the full kernel; -> (lazy results, lazy state)"""
    n = len(sigmas)
    lazy = _context(tr, mode, capi.SIGMA_LAZY, compaction, init)
    eager = _context(tr, mode, capi.SIGMA_EAGER, compaction, init)
    got, ref = _run(lazy, chunks, sigmas), _run(eager, chunks, sigmas)
    stats = lazy.sigma_stats()
    assert stats == {"deferred": n, "dropped": n - 1, "materialised": 0, "pending": True}, (tag, stats)
    lazy.sigma_flush()
    stats = lazy.sigma_stats()
    assert stats == {"deferred": n, "dropped": n - 1, "materialised": 1, "pending": False}, (tag, stats)
    st = lazy.get_state(S=False)
    assert lazy.sigma_stats()["materialised"] == 1, tag
    assert eager.sigma_stats()["deferred"] == 0, tag
    st_e = eager.get_state(S=False)
    for e in range(n):
        assert _same(got[e][0], ref[e][0]) and _same(got[e][1], ref[e][1]), (tag, "eager", e)
    for k in ("map", "sigma", "weight", "hits"):
        assert _same(st[k], st_e[k]), (tag, "eager", k)
    lazy.close()
    eager.close()
    return got, st


def _equals_oracle(tag, got, st, orc_res, orc_st, sigma_close=None):
    for e in range(len(got)):
        assert _same(got[e][0], orc_res[e][0]) and _same(got[e][1], orc_res[e][1]), (tag, "oracle", e)
    for k in ("map", "weight", "hits"):
        assert _same(st[k], orc_st[k]), (tag, "oracle", k)
    if sigma_close is not None:
        assert _close_sigma(st["sigma"], orc_st["sigma"], orc_st["weight"], sigma_close), (tag, "oracle", "sigma")
    else:
        assert _same(st["sigma"], orc_st["sigma"]), (tag, "oracle", "sigma")


def _one_and_three(tag, tr, mode, compaction, init, chunks):
    for sigmas in (SCHEDULE[:1], SCHEDULE):
        t = tag + (len(sigmas),)
        got, st = _lazy_eager(t, tr, mode, compaction, init, chunks, sigmas)
        _equals_oracle(t, got, st, *oracle_run(t, tr, init, chunks, sigmas))


# ---- quad-count edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quads", list(QUAD_CASES))
def test_quad_counts_sparse(quads):
    live = QUAD_CASES[quads]
    assert (live + 3) // 4 == quads
    B = 37
    init = init_map(J, True)
    chunks = [sparse_rows(B, 3, live), sparse_rows(B, 4, live)]
    _one_and_three(("sparse", quads), po.STANDARD, capi.UPDATE_STRICT, 1, init, chunks)


@pytest.mark.parametrize("quads", list(QUAD_CASES))
def test_quad_counts_dense(quads, monkeypatch):
    depth = 4 if quads == 1 else QUAD_CASES[quads]
    assert depth % 4 == 0 and depth // 4 == quads
    monkeypatch.setenv("VSOM_NO_CHAIN", "1")          # small depth: keep phase 2 on the lane = node kernels
    B = 37
    init = init_map(depth, False)
    chunks = [dense_rows(B, 3, depth), dense_rows(B, 4, depth)]
    _one_and_three(("dense", quads), po.STANDARD, capi.UPDATE_STRICT, -1, init, chunks)


# ---- sample-count edges ----------------------------------------------------------------------------------------------
def test_sample_counts():
    """9 quads with the compaction (a live / dead wavefront), every B; two epochs on alternating chunks"""
    init = init_map(J, True)
    for B in BS:
        chunks = [sparse_rows(B, 3, 36), sparse_rows(B, 4, 36)]
        tag = ("samples", B)
        got, st = _lazy_eager(tag, po.STANDARD, capi.UPDATE_STRICT, 1, init, chunks, SCHEDULE[:2])
        _equals_oracle(tag, got, st, *oracle_run(tag, po.STANDARD, init, chunks, SCHEDULE[:2]))


# ---- zero-form dispatch ----------------------------------------------------------------------------------------------
ZQ = 18                                                   # quads of the engineered rows: 72 columns = 8k + 2 quads
ZB = 67


def engineered_rows(seed, depth):
    """rows over ZQ quads (the columns beyond stay zero): sample j, wavefront pair k -> combination (j / 4 + j + k) % 4 of
    (quad 2k all zero?, quad 2k+1 all zero?) -- every combination at every position j % 4 of a group for every k.  Zero
    quads of odd samples hold -0.0; NaN, +inf and -inf each sit in ONE quad of a pair whose other quad is zero / non-zero"""
    rs = np.random.RandomState(seed)
    X = np.zeros((ZB, depth), np.float32)
    for j in range(ZB):
        for k in range(ZQ // 2):
            combo = (j // 4 + j + k) % 4
            for i in range(2):
                q = 2 * k + i
                if (combo >> i) & 1:
                    X[j, 4 * q:4 * q + 4] = -0.0 if j & 1 else 0.0
                else:
                    v = rs.randint(1, 256, 4).astype(np.float32)
                    v[rs.rand(4) < 0.3] = 0.0                     # partly zero quads are NOT zero quads
                    v[int(rs.randint(4))] = np.float32(1 + (j + q) % 9)
                    X[j, 4 * q:4 * q + 4] = v
    # non-finite values in one quad of a pair only: (sample, quad) chosen among the non-zero quads whose partner is zero
    # (combination 2: quad 2k live, 2k+1 zero; combination 1: the other way round) and whose partner is not (0)
    placed = 0
    for val, want in ((np.nan, 2), (np.inf, 1), (-np.inf, 0), (np.nan, 1)):
        for j in range(8 + 3 * placed, ZB):
            k = (want - j // 4 - j) % 4
            if k < ZQ // 2:
                q = 2 * k + (1 if want == 1 else 0)
                X[j, 4 * q + placed % 4] = val
                placed += 1
                break
    assert placed == 4
    return X


def combination_counts(X, live):
    """[position in the group][combination] -> occurrences over samples and wavefront pairs, from the inputs: the quads are
    those of the columns the kernel sees (`live`: the gathered live columns, or all of them)"""
    Xl = X[:, live]
    nq = (Xl.shape[1] + 3) // 4
    Xp = np.zeros((X.shape[0], 8 * ((nq + 7) // 8) * 4), np.float32)
    Xp[:, :Xl.shape[1]] = Xl
    z = (Xp.reshape(X.shape[0], -1, 4) == 0).all(axis=2)          # NaN == 0 is false, -0.0 == 0 is true
    cnt = np.zeros((4, 4), np.int64)
    for j in range(X.shape[0]):
        for k in range((nq + 1) // 2):
            cnt[j % 4, int(z[j, 2 * k]) + 2 * int(z[j, 2 * k + 1])] += 1
    return cnt


@pytest.mark.parametrize("compaction", (1, -1))
def test_zero_form_dispatch(compaction, monkeypatch):
    depth = J if compaction > 0 else 4 * ZQ
    if compaction < 0:
        monkeypatch.setenv("VSOM_NO_CHAIN", "1")
    chunks = [engineered_rows(5, depth), engineered_rows(6, depth)]
    for X in chunks:
        live = (X != 0).any(axis=0) if compaction > 0 else np.ones(depth, bool)
        assert int(live.sum()) == 4 * ZQ                            # every engineered column is live in some row
        cnt = combination_counts(X, live)
        assert (cnt > 0).all(), cnt                                 # all four combinations at all four positions
        assert np.isnan(X).any() and np.isposinf(X).any() and np.isneginf(X).any()
        assert (np.signbit(X) & (X == 0)).any()                     # -0.0 in zero quads
    init = init_map(depth, True)
    for tr, mode, name in ((po.STANDARD, capi.UPDATE_STRICT, "strict"), (po.MEDIAN, capi.UPDATE_STRICT, "median")):
        tag = ("zero", compaction, name)
        got, st = _lazy_eager(tag, tr, mode, compaction, init, chunks, SCHEDULE[:2])
        _equals_oracle(tag, got, st, *oracle_run(tag, tr, init, chunks, SCHEDULE[:2]))
    # the contracted kernel has a zero form of its own (meanfma): every bit against EAGER contracted
    _lazy_eager(("zero", compaction, "contracted"), po.STANDARD, capi.UPDATE_FMA, compaction, init, chunks, SCHEDULE[:2])


# ---- arithmetics -----------------------------------------------------------------------------------------------------
ARITH = {"strict": (po.STANDARD, capi.UPDATE_STRICT), "sigma": (po.STANDARD, capi.UPDATE_FMA_SIGMA),
         "contracted": (po.STANDARD, capi.UPDATE_FMA), "median": (po.MEDIAN, capi.UPDATE_STRICT)}


@pytest.mark.parametrize("arith", list(ARITH))
def test_arithmetics(arith):
    tr, mode = ARITH[arith]
    B, live = 67, 36
    init = init_map(J, True)
    chunks = [sparse_rows(B, 3, live), sparse_rows(B, 4, live)]
    for sigma in (10.0, 1.5):
        tag = (arith, sigma)
        if arith == "contracted":
            # bit equality with the oracle is impossible for fused arithmetic: ONE deferred epoch within the mode's bound
            got, st = _lazy_eager(tag, tr, mode, 1, init, chunks, (sigma,))
            orc_res, orc = oracle_run(("arith", "standard", sigma, 1), tr, init, chunks, (sigma,))
            assert _same(got[0][0], orc_res[0][0]) and _same(got[0][1], orc_res[0][1]), (tag, "oracle")
            assert _same(st["weight"], orc["weight"]) and _same(st["hits"], orc["hits"]), (tag, "oracle")
            assert _within_fma_bound(st["map"], orc["map"], chunks[0]), (tag, "oracle", "map")
            with np.errstate(divide="ignore", invalid="ignore"):
                under = np.sqrt(B * 2.0 ** -149 / orc["weight"].astype(np.float64))[:, None]
            under = np.where(np.isfinite(under), under, 0.0)
            assert _within_fma_bound(st["sigma"], orc["sigma"], chunks[0], under), (tag, "oracle", "sigma")
            _lazy_eager(tag + (2,), tr, mode, 1, init, chunks, (sigma, sigma))      # two epochs: every bit against EAGER
            continue
        got, st = _lazy_eager(tag, tr, mode, 1, init, chunks, (sigma, sigma))
        if sigma == 1.5:
            assert np.isnan(st["map"]).all(axis=1).any()            # the 0/0 rows are there
        key = ("arith", "median" if arith == "median" else "standard", sigma, 2)
        _equals_oracle(tag, got, st, *oracle_run(key, tr, init, chunks, (sigma, sigma)),
                       sigma_close=B if arith == "sigma" else None)


# ---- materialisation -------------------------------------------------------------------------------------------------
def test_materialisation_after_mean_only_epoch():
    """one mean-only epoch, then get_state as the reader (no explicit flush): the full `_nt4` kernel runs from the rebuilt
    (c,w) array, stores M over the mean-only kernel's and turns its S into sigmaMap.  Everything equals EAGER and the oracle.
    (_lazy_eager checks the same after vsom_sigma_flush in every other case.)"""
    B, live = 67, 40
    init = init_map(J, True)
    X = sparse_rows(B, 3, live)
    lazy = _context(po.STANDARD, capi.UPDATE_STRICT, capi.SIGMA_LAZY, 1, init)
    eager = _context(po.STANDARD, capi.UPDATE_STRICT, capi.SIGMA_EAGER, 1, init)
    for c in (lazy, eager):
        c.upload_chunk(X)
        c.batch_epoch(10.0, True)
    assert lazy.sigma_stats() == {"deferred": 1, "dropped": 0, "materialised": 0, "pending": True}
    a = lazy.get_state(S=False)                                       # the reader
    assert lazy.sigma_stats() == {"deferred": 1, "dropped": 0, "materialised": 1, "pending": False}
    b = eager.get_state(S=False)
    orc = oracle_run(("mat",), po.STANDARD, init, [X, X], (10.0,))[1]
    for k in ("map", "sigma", "weight", "hits"):
        assert _same(a[k], b[k]), ("eager", k)
        assert _same(a[k], orc[k]), ("oracle", k)
    lazy.close()
    eager.close()
