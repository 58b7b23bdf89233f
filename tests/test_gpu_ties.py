"""GPU: every BMU search path on engineered ties and one-ulp near-ties (tests/ties.py), bit for bit against the oracle.

Mirror pairs tie exactly between rows that are not bit-identical (the dedupe pass cannot merge them: the lower index must
win), one-ulp pairs are won by either index by a few ulps, order-decided pairs only by a search that sums in the
reference's order; cancellation cases put every node inside the bound.  Each test also checks that its input holds those
cases at the BMU and that the path it means to reach was taken (shortlist / online-search counters)."""
import numpy as np
import pytest

import custom_hooks as hooks
import ties
import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
KEYS = ("map", "S", "sigma", "weight", "hits")


def beq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()
    return (a == b).all()


def _want(case):
    idx = np.array([c["winner"] for c in case.certs], np.uint64)
    dist = np.array([c["d32"][0] for c in case.certs], np.float32)
    return idx, dist


def _not_vacuous(case):
    live = [c for c in case.certs if c is not None]
    assert live and all(c["margin_ok"] for c in live), case.name
    assert case.exact_ties() >= 2, case.name
    if not case.name.startswith(("cancel", "u8edge")):      # those two kinds are exact mirror ties only
        assert case.hi_wins() >= 1 and case.order_decided() >= 1, case.name


def _ctx(case, mode, custom=None):
    if custom is not None:
        d, r = hooks.shape(custom, case.J)
        ctx = capi.Context(case.W, case.H, case.J, capi.CUSTOM, source=hooks.SOURCES[custom], depth=d, residual_len=r)
    else:
        ctx = vsom_amd.Context(case.W, case.H, case.J, case.tr)
    ctx.set_bmu_mode(mode)
    ctx.set_state(map=case.init)
    ctx.upload_chunk(case.X)
    return ctx


def _search(case, ctx):
    idx, dist = ctx.bmu_batch()
    w_idx, w_dist = _want(case)
    bad = np.nonzero(idx != w_idx)[0]
    assert bad.size == 0, (case.name, [(int(s), int(idx[s]), case.certs[s]) for s in bad[:4]])
    assert beq(dist, w_dist), case.name


def _epoch_against_oracle(case, ctx, sigma):
    o = po.OracleSom(case.W, case.H, case.J, case.tr)
    o.set_state(map=case.init)
    lb = np.zeros(case.X.shape[0], np.uint64)
    mse_o = o.batch_epoch(case.X, lb, sigma, True, nthreads=16)
    ctx.set_state(map=case.init)
    ctx.upload_chunk(case.X)
    mse = ctx.batch_epoch(sigma, True)
    assert beq(ctx.get_last_bmu(), lb) and beq(lb, _want(case)[0]), case.name
    st = ctx.get_state()
    for k in KEYS:
        assert beq(st[k], getattr(o, k)), (case.name, k)
    assert beq(np.float32(mse), mse_o), case.name
    o.close()


@pytest.mark.parametrize("dedupe", [0, -1], ids=["representatives", "every_node"])
@pytest.mark.parametrize("name", ["float_40x36x24", "median_40x36x24", "general_40x36x784", "clr_34x34x10"])
def test_exact_tile_kernel(name, dedupe):
    case = ties.batch(name)
    _not_vacuous(case)
    ctx = _ctx(case, capi.BMU_EXACT)
    ctx.set_row_dedupe(dedupe)
    _search(case, ctx)
    ctx.close()


PRUNED = ["u8_40x36x784", "general_40x36x784", "u8edge_40x36x784", "u8_128x128x784", "general_128x128x784",
          "u8edge_128x128x784", "k64_64x64x32", "float_40x36x24", "median_40x36x24", "clr_34x34x10"]
# the form of the integer contraction each case is there for (ties.ring_plan restates sl_i8_plan's rule)
PLAN = {"u8_40x36x784": 0, "general_40x36x784": 0, "u8edge_40x36x784": 0, "u8_128x128x784": 2, "general_128x128x784": 2,
        "u8edge_128x128x784": 2, "k64_64x64x32": 1, "float_40x36x24": 1, "median_40x36x24": 1}


@pytest.mark.parametrize("name", PRUNED)
def test_shortlist_search(name):
    """the integer shortlist (uint8 and general kind; G and 64-node tiles at 40 x 36, the G-less ring kernel at 128 x 128
    with 2048 rows, sl_k64 at 24 and 32 values; pairs at the edge of the digit grid through both refinements) and the CLR fp32
    shortlist: pruned searches that keep both members of every pair, and an epoch that trains on them"""
    case = ties.batch(name)
    _not_vacuous(case)
    if name in PLAN:
        assert ties.ring_plan(case.W * case.H, case.X.shape[0], case.J) == PLAN[name], name
    if name.startswith("u8edge"):
        # digit-edge pairs in different 64-node tiles: only a threshold of the full bound keeps the lower node
        assert sum(c["pair"][0] // 64 != c["pair"][1] // 64 for c in case.certs) >= 50
    ctx = _ctx(case, capi.BMU_SHORTLIST)
    _search(case, ctx)
    st = ctx.shortlist_stats()
    B = case.X.shape[0]
    assert st["searches"] >= 1 and st["candidates"] > B and st["redo_samples"] == 0, (name, st)
    if case.W * case.H <= 1600:
        _epoch_against_oracle(case, ctx, 4.0)
    ctx.close()


@pytest.mark.parametrize("name", ["dead_40x40x64", "dead_u8_40x40x64"])
def test_shortlist_with_retired_columns(name):
    case = ties.batch(name)
    _not_vacuous(case)
    ctx = vsom_amd.Context(case.W, case.H, case.J, case.tr)
    ctx.set_column_compaction(1)
    ctx.set_bmu_mode(capi.BMU_SHORTLIST)
    ctx.set_state(map=case.init)
    ctx.upload_chunk(case.X)
    _search(case, ctx)
    st = ctx.shortlist_stats()
    assert st["candidates"] > case.X.shape[0] and st["redo_samples"] == 0, st
    _epoch_against_oracle(case, ctx, 6.0)
    ctx.close()


def test_candidate_tiles_around_tmax():
    """sl_pick_kernel keeps at most tmax = 64 candidate tiles per sample and redoes the others exactly: near-tie decoys in
    0 .. 127 tiles of their own per sample put the chunk on both sides of that limit, and both sides give the oracle's bits"""
    case = ties.batch("tmax_64x64x32")
    _not_vacuous(case)
    assert ties.ring_plan(case.W * case.H, case.X.shape[0], case.J) == 1
    assert min(case.decoys) == 0 and max(case.decoys) > 64
    ctx = _ctx(case, capi.BMU_SHORTLIST)
    _search(case, ctx)
    st = ctx.shortlist_stats()
    B = case.X.shape[0]
    assert 0 < st["redo_samples"] < B and st["candidates"] > B, st
    ctx.close()


def test_cancellation_sends_every_sample_to_the_redo_list():
    """values around 1e3..1e4 with a spread of 1e-2: the bound's u (|M|^2 + |x|^2) term covers every node, the search
    falls back to the exact-order kernel, and the mirror ties still go to the lower index"""
    case = ties.batch("cancel_40x36x64")
    _not_vacuous(case)
    for dedupe in (0, -1):
        ctx = _ctx(case, capi.BMU_SHORTLIST)
        ctx.set_row_dedupe(dedupe)
        _search(case, ctx)
        assert ctx.shortlist_stats()["redo_samples"] > 0, ctx.shortlist_stats()
        ctx.close()
    ctx = _ctx(case, capi.BMU_EXACT)
    _search(case, ctx)
    ctx.close()


@pytest.mark.parametrize("name", ["tiny_10x10x9", "tiny_32x32x4", "float_40x36x24", "median_40x36x24"])
def test_batch_epoch(name):
    """the tiny batch epoch (one workgroup, LDS atomicMin of the argmin key) and the general batch epoch"""
    case = ties.batch(name)
    _not_vacuous(case)
    for mode in (capi.BMU_AUTO, capi.BMU_EXACT):
        ctx = _ctx(case, mode)
        _epoch_against_oracle(case, ctx, 2.5)
        ctx.close()


def _online(case, mode, ctx=None):
    o, lb, mse = ties.replay_online(case)
    assert beq(lb, case.lb)
    own = ctx is None
    if own:
        ctx = vsom_amd.Context(case.W, case.H, case.J, case.tr)
    ctx.set_bmu_mode(mode)
    ctx.set_state(map=case.init)
    ctx.upload_chunk(case.X)
    ctx.online_search_stats(reset=True)
    run, lb_g = ctx.train_online_chunk_fetch(case.eta, case.sigma, case.decay_fn)
    for j, c in enumerate(case.certs):
        if c is not None:
            assert int(lb_g[j]) == c["winner"], (case.name, mode, j, int(lb_g[j]), c)
    assert beq(lb_g, lb), case.name
    st = ctx.get_state()
    for k in KEYS:
        assert beq(st[k], getattr(o, k)), (case.name, mode, k)
    assert beq(np.float32(run), mse), case.name
    stats = ctx.online_search_stats()
    o.close()
    if own:
        ctx.close()
    return stats


@pytest.mark.parametrize("name", list(ties.ONLINE))
def test_online_chunk(name):
    """the exact scan (16 key slots), the image-bounded search (the window node re-digited in registers, the other node
    scored from the image) and, on tiny maps, the one-launch chunk"""
    case = ties.online(name)
    _not_vacuous_online(case)
    B = case.X.shape[0]
    _online(case, capi.BMU_EXACT)
    stats = _online(case, capi.BMU_SHORTLIST)
    assert stats["samples"] == B and stats["exact_evaluations"] >= 2 * B, stats
    if case.W * case.H * case.J <= 4096:
        _online(case, capi.BMU_AUTO)


@pytest.mark.parametrize("name", list(ties.ONLINE_EDGE))
def test_online_image_search_at_the_digit_edge(name):
    """pairs whose image approximations err by about slack_n in opposite directions (ties.online_edge_case): the image
    interval has to be as wide as the bound says to keep the lower node, and the oracle's bits come out"""
    case = ties.online_edge(name)
    assert all(c["margin_ok"] for c in case.certs) and case.exact_ties() == case.X.shape[0]
    B = case.X.shape[0]
    stats = _online(case, capi.BMU_SHORTLIST)
    assert stats["samples"] == B and stats["exact_evaluations"] >= 2 * B, stats
    _online(case, capi.BMU_EXACT)


def _not_vacuous_online(case):
    live = [c for c in case.certs if c is not None]
    assert len(live) >= 6 and all(c["margin_ok"] for c in live) and case.exact_ties() >= 2, case.name
    assert all(c["window_node"] == case.lb[j - 1] for j, c in enumerate(case.certs) if c is not None)


def test_single_vector_searches():
    """findBmu, findLocalBmu (the walk, sigma <= 1), findRestrictedBmu and trainSingle on tie samples"""
    case = ties.batch("float_40x36x24")
    _not_vacuous(case)
    o = po.OracleSom(case.W, case.H, case.J, case.tr)
    o.set_state(map=case.init, hits=np.ones(case.W * case.H, np.uint64))
    ctx = vsom_amd.Context(case.W, case.H, case.J, case.tr)
    ctx.set_state(map=case.init, hits=np.ones(case.W * case.H, np.uint64))
    for s in range(0, case.X.shape[0], 3):
        x, c = case.X[s], case.certs[s]
        i, d = ctx.find_bmu(x)
        assert i == c["winner"] and beq(d, c["d32"][0]), (s, i, c)
        for start in c["pair"] + (0, case.W * case.H - 1, (c["pair"][0] + c["pair"][1]) // 2):
            i, d = ctx.find_local_bmu(x, start)
            w = o.find_local_bmu(x, start)
            assert i == w and beq(d, np.float32(o.dist(w, x))), (s, start)
        i, d = ctx.find_restricted_bmu(x, 1)
        assert i == o.find_restricted_bmu(x, 1) == c["winner"], s
    # trainSingle: both decay functions, the full search and the local walk
    for s in range(0, 24):
        x = case.X[s]
        for sigma in (1.8, 0.9):
            r_o = o.train_single(x, 0.05, sigma, case.certs[s]["pair"][1], capi.EXPONENTIAL)
            r_g = ctx.train_single(x, 0.05, sigma, case.certs[s]["pair"][1], capi.EXPONENTIAL)
            assert r_g[0] == r_o[0] and beq(r_g[1], r_o[1]) and beq(r_g[2], r_o[2]) and r_g[3] == r_o[3], (s, sigma)
    st = ctx.get_state()
    for k in KEYS:
        assert beq(st[k], getattr(o, k)), k
    ctx.close()
    o.close()


def test_ensemble_members_with_tie_maps():
    """Ensemble.bmu_batch, batch_epoch and the online chunk (one workgroup per map, the LDS atomicMin key)"""
    names = ["tiny_10x10x9", "tiny_32x32x4"]
    cases = [ties.batch(n) for n in names]
    for c in cases:
        _not_vacuous(c)
    ctxs = [vsom_amd.Context(c.W, c.H, c.J, c.tr) for c in cases]
    for ctx, c in zip(ctxs, cases):
        ctx.set_state(map=c.init)
    ens = vsom_amd.Ensemble(ctxs)
    ens.upload_chunks([c.X for c in cases])
    idx, dist = ens.bmu_batch()
    for k, c in enumerate(cases):
        w_idx, w_dist = _want(c)
        assert beq(idx[k], w_idx) and beq(dist[k], w_dist), c.name
    mse = ens.batch_epoch(2.5, True)
    for k, c in enumerate(cases):
        o = po.OracleSom(c.W, c.H, c.J, c.tr)
        o.set_state(map=c.init)
        lb = np.zeros(c.X.shape[0], np.uint64)
        mse_o = o.batch_epoch(c.X, lb, 2.5, True, nthreads=8)
        assert beq(ctxs[k].get_last_bmu(), lb) and beq(lb, _want(c)[0]) and beq(mse[k], mse_o), c.name
        st = ctxs[k].get_state()
        for key in KEYS:
            assert beq(st[key], getattr(o, key)), (c.name, key)
        o.close()
    ens.close()
    for ctx in ctxs:
        ctx.close()
    # the online chunk of tie members
    oc = [ties.online(n) for n in ("online_10x10x9", "online_32x32x4")]
    for c in oc:
        _not_vacuous_online(c)
    ctxs = [vsom_amd.Context(c.W, c.H, c.J, c.tr) for c in oc]
    for ctx, c in zip(ctxs, oc):
        ctx.set_state(map=c.init)
    ens = vsom_amd.Ensemble(ctxs)
    ens.upload_chunks([c.X for c in oc])
    mse, lbs = ens.train_online_chunk_fetch([c.eta for c in oc], [c.sigma for c in oc], [c.decay_fn for c in oc])
    for k, c in enumerate(oc):
        o, lb, mse_o = ties.replay_online(c)
        assert beq(lbs[k], lb) and beq(mse[k], mse_o), c.name
        st = ctxs[k].get_state()
        for key in KEYS:
            assert beq(st[key], getattr(o, key)), (c.name, key)
        o.close()
    ens.close()
    for ctx in ctxs:
        ctx.close()


def test_custom_standard_hook_on_ties():
    case = ties.batch("float_40x36x24")
    _not_vacuous(case)
    ctx = _ctx(case, capi.BMU_AUTO, custom="standard")
    _search(case, ctx)
    _epoch_against_oracle(case, ctx, 3.0)
    ctx.close()


def test_group_members_on_one_device():
    case = ties.batch("float_40x36x24")
    _not_vacuous(case)
    g = vsom_amd.Group(case.W, case.H, case.J, case.tr, devices=[0, 0])
    g.set_state(map=case.init)
    g.upload_chunk(case.X)
    mse = g.batch_epoch(3.0, True)
    o = po.OracleSom(case.W, case.H, case.J, case.tr)
    o.set_state(map=case.init)
    lb = np.zeros(case.X.shape[0], np.uint64)
    mse_o = o.batch_epoch(case.X, lb, 3.0, True, nthreads=16)
    assert beq(g.get_last_bmu(), lb) and beq(lb, _want(case)[0]) and beq(np.float32(mse), mse_o)
    for r in range(2):
        st = g.member(r).get_state()
        for k in KEYS:
            assert beq(st[k], getattr(o, k)), (r, k)
    o.close()
    g.close()
