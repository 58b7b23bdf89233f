"""GPU: the ensemble calls around training (include/vsom_hip.h) -- vsom_ensemble_upload_chunks gives every member its
rows from one host buffer, vsom_ensemble_bmu_batch scores every member's chunk.  Every comparison is bitwise against twin
contexts driven one call at a time (vsom_upload_chunk, vsom_bmu_batch), and against the oracle for a subset: mixed members
(tiny maps of the three kinds, maps above the tiny bound, a chunk that gets the column compaction, a custom member, no
rows, shared and distinct offsets with gaps), the asynchronous form on both stream layouts, a member with a chunk staged
ahead, the search's NaN / tie rules at chunk sizes around the tile and at the tiny bound, more members than the chip has
CUs, all six ensemble calls back to back on one ensemble, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import custom_hooks as hooks
import gen
import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

KEYS = ("map", "S", "sigma", "weight", "hits")
EXP = capi.EXPONENTIAL


def beq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()
    return (a == b).all()


def rows(B, J, seed, special=True):
    """blobs with repeated rows and, when asked, a NaN value and an inf row"""
    X = gen.blobs(max(B, 1), J, 4, seed, seed + 1, sigma=0.3)[:B]
    if special and B >= 6:
        X[B // 3] = X[0]
        X[B // 2, J // 2] = np.nan
        X[B - 2, 0] = np.inf
    return np.ascontiguousarray(X, dtype=np.float32)


class Pair:
    """a member and its twin: the same map and settings; the twin is driven by the single-context calls"""

    def __init__(self, W, H, J, tr, seed, custom=None, cc=None, mode=None):
        self.W, self.H, self.J, self.tr = W, H, J, tr
        D = po.length(tr, J) if custom is None else hooks.shape(custom, J)[0]
        self.init = gen.random_map(W * H, D, seed=seed)

        def make():
            if custom is not None:
                d, r = hooks.shape(custom, J)
                ctx = capi.Context(W, H, J, capi.CUSTOM, source=hooks.SOURCES[custom], depth=d, residual_len=r)
            else:
                ctx = vsom_amd.Context(W, H, J, tr)
            if cc is not None:
                ctx.set_column_compaction(cc)
            if mode is not None:
                ctx.set_bmu_mode(mode)
            ctx.set_state(map=self.init)
            return ctx

        self.m, self.t = make(), make()

    def same(self, what, mse=None, mse_t=None):
        a, b = self.m.get_state(), self.t.get_state()
        for k in KEYS:
            assert beq(a[k], b[k]), (what, k)
        assert beq(self.m.get_last_bmu(), self.t.get_last_bmu()), (what, "lastBMU")
        if mse is not None:
            assert beq(np.float32(mse), np.float32(mse_t)), (what, "mse", mse, mse_t)

    def close(self):
        self.m.close()
        self.t.close()


def pack(chunks, share, gap=5, seed=0):
    """one host buffer: chunks[k] at offset[k]; share[k] = j < k: member k names member j's rows; `gap` floats of junk
    between the ranges (copied too, never read as rows)"""
    rs = np.random.RandomState(seed)
    offs, parts, at = [], [], gap
    for k, X in enumerate(chunks):
        if share[k] is not None:
            offs.append(offs[share[k]])
            continue
        offs.append(at)
        parts.append((at, X))
        at += X.size + gap
    buf = rs.standard_normal(at).astype(np.float32)
    for o, X in parts:
        buf[o:o + X.size] = X.reshape(-1)
    return buf, offs


def upload(ens, buf, offs, Bs, wait=1):
    n = len(offs)
    off = (C.c_size_t * n)(*offs)
    bs = (C.c_size_t * n)(*Bs)
    capi.check(capi.lib().vsom_ensemble_upload_chunks(ens._h, capi._f(buf), buf.size, off, bs, int(wait)))


def score_twins(pairs, what):
    """Ensemble.bmu_batch against vsom_bmu_batch on every twin, then the values left on the device"""
    ens_idx, ens_dist = what
    for k, p in enumerate(pairs):
        if p.t.chunk_size == 0:
            assert ens_idx[k].size == 0
            continue
        idx, dist = p.t.bmu_batch()
        assert beq(ens_idx[k], idx) and beq(ens_dist[k], dist), k
        assert beq(p.m.get_last_bmu(), p.t.get_last_bmu()) and beq(p.m.get_sqres(), p.t.get_sqres()), k


def mixed_pairs():
    return [Pair(10, 10, 9, po.STANDARD, 1),
            Pair(10, 10, 9, po.STANDARD, 2),                  # the same rows as member 0
            Pair(8, 8, 12, po.MEDIAN, 3),
            Pair(6, 6, 5, po.CLR, 4),
            Pair(40, 40, 16, po.STANDARD, 5),                 # above the tiny bound, no compaction: the one staging launch
            Pair(32, 32, 64, po.STANDARD, 6, cc=16),          # a chunk that gets the column compaction
            Pair(10, 10, 9, po.STANDARD, 7, custom="standard"),
            Pair(7, 7, 6, po.MEDIAN, 8),                      # no rows
            Pair(16, 16, 16, po.MEDIAN, 9)]                   # N * D = 4096


def test_upload_parity_mixed_members():
    pairs = mixed_pairs()
    Bs = [20, 20, 50, 40, 300, 300, 20, 0, 70]
    share = [None, 0, None, None, None, None, None, None, None]
    chunks = []
    for k, (p, B) in enumerate(zip(pairs, Bs)):
        X = gen.correlated(B, p.J, 20 + k) if p.tr == po.CLR else rows(B, p.J, 20 + k)
        if k == 5:
            X[:, 40:] = 0.0                                   # all-zero columns for the compaction to retire
        chunks.append(X if share[k] is None else chunks[share[k]])
    buf, offs = pack(chunks, share)
    ens = vsom_amd.Ensemble([p.m for p in pairs])
    upload(ens, buf, offs, Bs)
    for p, X in zip(pairs, chunks):
        p.t.upload_chunk(X)
    for k, p in enumerate(pairs):
        assert p.m.chunk_size == Bs[k]
        p.same(("upload", k))
    n = len(pairs)
    eta, sigma, fn = [0.05] * n, [2.0 + 0.25 * k for k in range(n)], [EXP] * n
    mse, lbs = ens.train_online_chunk_fetch(eta, sigma, fn, first_chunk=True)
    for k, p in enumerate(pairs):
        mse_t, lb_t = p.t.train_online_chunk_fetch(eta[k], sigma[k], fn[k], first_chunk=True)
        assert beq(lbs[k], lb_t), ("online", k)
        p.same(("online", k), mse[k], mse_t)
    mse = ens.batch_epoch(sigma, True)
    for k, p in enumerate(pairs):
        p.same(("batch", k), mse[k], p.t.batch_epoch(sigma[k], True))
    # member 0 (and 1, on the same rows) against the oracle
    o = po.OracleSom(10, 10, 9, po.STANDARD)
    o.set_state(map=pairs[1].init)
    lb = np.zeros(20, np.uint64)
    o.train_online_chunk(chunks[1], lb, eta[1], sigma[1], fn[1])
    mse_o = o.batch_epoch(chunks[1], lb, sigma[1], True)
    assert beq(np.float32(mse[1]), np.float32(mse_o)) and beq(pairs[1].m.get_last_bmu(), lb)
    st = pairs[1].m.get_state()
    for key in ("map", "sigma", "weight"):
        assert beq(st[key], getattr(o, key)), key
    ens.close()
    for p in pairs:
        p.close()


@pytest.mark.parametrize("layout", ["shared", "one_apart"])
def test_async_upload_then_train_at_once(layout):
    """wait = 0 from pinned memory, a batch epoch right behind it; then two back-to-back wait = 0 uploads of different
    rows and a batch epoch.  Members on one stream, or one member on a stream of its own (the ensemble's own launch
    stream joins them)."""
    import torch
    specs = [(10, 10, 9, po.STANDARD), (8, 8, 12, po.MEDIAN), (6, 6, 5, po.CLR), (40, 40, 16, po.STANDARD),
             (12, 9, 20, po.MEDIAN)]
    pairs = [Pair(W, H, J, tr, 40 + i) for i, (W, H, J, tr) in enumerate(specs)]
    dev = torch.device("cuda", 0)
    shared, apart = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for k, p in enumerate(pairs):
        p.m.set_stream((apart if layout == "one_apart" and k == 3 else shared).cuda_stream)
    ens = vsom_amd.Ensemble([p.m for p in pairs])
    Bs = [20, 50, 40, 300, 37]
    bufs = []
    for rnd in range(3):
        chunks = [gen.correlated(B, p.J, 60 + 10 * rnd + k) if p.tr == po.CLR else rows(B, p.J, 60 + 10 * rnd + k)
                  for k, (p, B) in enumerate(zip(pairs, Bs))]
        flat, offs = pack(chunks, [None] * len(pairs), seed=rnd)
        pin = capi.PinnedBuffer(flat.shape)
        pin.array[:] = flat
        bufs.append((pin, offs, chunks))
    sigma = [3.0 + 0.5 * k for k in range(len(pairs))]
    # one upload, the epoch right behind it
    pin, offs, chunks = bufs[0]
    ens.upload_chunks_async(pin, offs, Bs)
    mse = ens.batch_epoch(sigma, True)
    for k, p in enumerate(pairs):
        p.t.upload_chunk(chunks[k])
        p.same(("first", k), mse[k], p.t.batch_epoch(sigma[k], True))
    # two uploads back to back: the second's copy must wait for the first's staging
    ens.upload_chunks_async(bufs[1][0], bufs[1][1], Bs)
    ens.upload_chunks_async(bufs[2][0], bufs[2][1], Bs)
    mse = ens.batch_epoch(sigma, True)
    for k, p in enumerate(pairs):
        p.t.upload_chunk(bufs[2][2][k])
        p.same(("second", k), mse[k], p.t.batch_epoch(sigma[k], True))
    score_twins(pairs, ens.bmu_batch())
    ens.close()
    for p in pairs:
        p.m.synchronize()
        p.close()
    for pin, _, _ in bufs:
        pin.free()


@pytest.mark.parametrize("layout", ["shared", "one_apart", "each_own"])
def test_all_calls_back_to_back_on_one_ensemble(layout):
    """the six calls share the ensemble's two descriptor slots and its launch stream, each with a descriptor size of its
    own: two rounds of upload (wait = 0), schedule, batch epoch, online chunk, scoring, U-matrix on one ensemble of tiny
    maps of the three kinds, a map just above the tiny bound and a member without rows in the first round -- every returned
    array and every member's state after each call equal the twins' driven one single-context call at a time"""
    import torch
    specs = [(10, 10, 9, po.STANDARD), (12, 9, 20, po.MEDIAN), (7, 7, 6, po.CLR),
             (33, 32, 4, po.STANDARD),                        # N * D = 4224: the ordinary way in every call
             (8, 8, 12, po.MEDIAN)]                           # no rows in the first round
    pairs = [Pair(W, H, J, tr, 160 + i) for i, (W, H, J, tr) in enumerate(specs)]
    n = len(pairs)
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(device=dev) for _ in range(n)]
    for k, p in enumerate(pairs):
        own = layout == "each_own" or (layout == "one_apart" and k == 3)
        p.m.set_stream(streams[k if own else 0].cuda_stream)
    ens = vsom_amd.Ensemble([p.m for p in pairs])
    eta, fn = [0.05] * n, [EXP] * n
    pins = []
    for rnd, Bs in enumerate(([20, 37, 40, 500, 0], [20, 37, 40, 500, 50])):
        # (the NaN and inf rows only in the last round: no state is compared as NaN against NaN before it)
        chunks = [gen.correlated(B, p.J, 170 + 10 * rnd + k) if p.tr == po.CLR
                  else rows(B, p.J, 170 + 10 * rnd + k, special=rnd == 1) for k, (p, B) in enumerate(zip(pairs, Bs))]
        flat, offs = pack(chunks, [None] * n, seed=rnd)
        pin = capi.PinnedBuffer(flat.shape)
        pin.array[:] = flat
        pins.append(pin)
        what = (layout, rnd)
        ens.upload_chunks_async(pin, offs, Bs)
        for k, p in enumerate(pairs):
            p.t.upload_chunk(chunks[k])
        sched = [[3.0 - 0.5 * ep + 0.1 * k for ep in range(3)] for k in range(n)]
        mses = ens.batch_schedule(sched)
        for k, p in enumerate(pairs):
            assert beq(mses[k], p.t.batch_schedule(sched[k])), (what, "schedule mse", k)
            p.same((what, "schedule", k))
        sigma = [2.0 + 0.25 * k for k in range(n)]
        mse = ens.batch_epoch(sigma, False)
        for k, p in enumerate(pairs):
            p.same((what, "batch", k), mse[k], p.t.batch_epoch(sigma[k], False))
        mse, lbs = ens.train_online_chunk_fetch(eta, sigma, fn, first_chunk=rnd == 0)
        for k, p in enumerate(pairs):
            mse_t, lb_t = p.t.train_online_chunk_fetch(eta[k], sigma[k], fn[k], first_chunk=rnd == 0)
            assert beq(lbs[k], lb_t), (what, "online lastBMU", k)
            p.same((what, "online", k), mse[k], mse_t)
        score_twins(pairs, ens.bmu_batch())
        for k, p in enumerate(pairs):
            p.same((what, "score", k))
        um = ens.umatrix()
        for k, p in enumerate(pairs):
            um_t = p.t.umatrix()
            assert um[k].dtype == um_t.dtype == np.float64, (what, "umatrix", k)
            assert ((um[k].view(np.uint64) == um_t.view(np.uint64)) | (np.isnan(um[k]) & np.isnan(um_t))).all(), (what, "umatrix", k)
            p.same((what, "umatrix", k))
    ens.close()
    for p in pairs:
        p.m.synchronize()
        p.close()
    for pin in pins:
        pin.free()


def test_upload_over_a_chunk_staged_ahead():
    """the next chunk prefetched beside a running epoch (staged ahead over the current rows), not committed: the ensemble
    upload gives what vsom_upload_chunk gives after the same calls, and a later commit stages the prefetched rows anew"""
    pairs = [Pair(40, 40, 16, po.STANDARD, 81), Pair(10, 10, 9, po.STANDARD, 82)]
    X0, X1, X2 = rows(300, 16, 83), rows(300, 16, 84), rows(256, 16, 85)
    Y = rows(20, 9, 86)
    pin = capi.PinnedBuffer(X1.shape)
    pin.array[:] = X1
    p = pairs[0]
    for ctx in (p.m, p.t):
        ctx.upload_chunk(X0)
        ctx.batch_epoch_async(3.0, True)
        ctx.prefetch_chunk(pin.array)
    ens = vsom_amd.Ensemble([q.m for q in pairs])
    buf, offs = pack([X2, Y], [None, None])
    upload(ens, buf, offs, [256, 20])
    p.t.upload_chunk(X2)
    pairs[1].t.upload_chunk(Y)
    mse = ens.batch_epoch([2.5, 2.5], True)
    for k, q in enumerate(pairs):
        q.same(("after upload", k), mse[k], q.t.batch_epoch(2.5, True))
    for ctx in (p.m, p.t):
        ctx.commit_chunk()
    mse = ens.batch_epoch([2.0, 2.0], True)
    for k, q in enumerate(pairs):
        q.same(("after commit", k), mse[k], q.t.batch_epoch(2.0, True))
    assert p.m.chunk_size == 300
    ens.close()
    for q in pairs:
        q.close()
    pin.free()


def scoring_pairs():
    """(pair, B, rows) for the scoring cases"""
    out = []

    def add(p, X):
        out.append((p, X.shape[0], X))

    p = Pair(10, 10, 9, po.STANDARD, 101)                     # NaN / inf rows; duplicate model rows (ties)
    X = rows(20, 9, 102)
    p.init[17] = X[2]
    p.init[5] = X[2]
    p.init[40] = p.init[41]
    for c in (p.m, p.t):
        c.set_state(map=p.init)
    add(p, X)
    p = Pair(5, 5, 4, po.STANDARD, 103)                       # a NaN at node 0: every BMU pinned to 0
    p.init[0, 1] = np.nan
    for c in (p.m, p.t):
        c.set_state(map=p.init)
    add(p, rows(30, 4, 104))
    for i, B in enumerate((1, 255, 256, 257, 1024, 5000)):   # around the tile, the chunk cap, many tiles
        add(Pair(9, 7, 11, (po.STANDARD, po.MEDIAN, po.CLR)[i % 3], 110 + i),
            gen.correlated(B, 11, 120 + i) if i % 3 == 2 else rows(B, 11, 120 + i))
    add(Pair(16, 16, 16, po.MEDIAN, 130), rows(100, 16, 131))           # N * part_len = 4096: the launch
    add(Pair(16, 16, 17, po.STANDARD, 132), rows(100, 17, 133))         # 4352: vsom_bmu_batch
    add(Pair(8, 8, 17, po.CLR, 134), gen.correlated(90, 17, 135))       # CLR: 64 * 136 = 8704, vsom_bmu_batch
    add(Pair(4, 4, 9, po.CLR, 136), gen.correlated(70, 9, 137))         # CLR 16 * 36: the launch
    add(Pair(10, 10, 9, po.STANDARD, 138, custom="standard"), rows(20, 9, 139))
    add(Pair(10, 10, 9, po.STANDARD, 140, mode=capi.BMU_SHORTLIST), rows(64, 9, 141))
    add(Pair(8, 8, 12, po.MEDIAN, 142, mode=capi.BMU_EXACT), rows(33, 12, 143))
    return out


def test_scoring_parity():
    cases = scoring_pairs()
    pairs = [c[0] for c in cases]
    ens = vsom_amd.Ensemble([p.m for p in pairs])
    ens.upload_chunks([X for _, _, X in cases])
    for p, _, X in cases:
        p.t.upload_chunk(X)
    idx, dist = ens.bmu_batch()
    score_twins(pairs, (idx, dist))
    # the rules themselves
    assert (idx[1] == 0).all() and np.isnan(dist[1]).all()
    assert idx[0][2] == 5 and dist[0][2] == 0.0 and idx[0][20 // 2] == 0 and np.isnan(dist[0][20 // 2])
    # Standard, Median and CLR against the oracle
    for k in (2, 3, 4, 8, 11):
        p, B, X = cases[k]
        o = po.OracleSom(p.W, p.H, p.J, p.tr)
        o.set_state(map=p.init)
        lb, sq = np.zeros(B, np.uint64), np.zeros(B, np.float32)
        o.batch_phase1_range(X, 0, B, lb, sq, True)
        assert beq(idx[k], lb) and beq(dist[k], sq), k
    # what a following is_first = 0 epoch reads
    sigma = [2.5] * len(pairs)
    mse = ens.batch_epoch(sigma, False)
    for k, p in enumerate(pairs):
        p.same(("epoch", k), mse[k], p.t.batch_epoch(2.5, False))
    ens.close()
    for p in pairs:
        p.close()


def test_more_members_than_compute_units():
    K = 600
    pairs = [Pair(10, 10, 9, po.STANDARD if k % 5 else po.MEDIAN, 1000 + k) for k in range(K)]
    ens = vsom_amd.Ensemble([p.m for p in pairs])
    shared = rows(20, 9, 7)
    chunks = [shared if k % 3 == 0 else rows(20 + k % 7, 9, 2000 + k) for k in range(K)]
    ens.upload_chunks(chunks)
    for p, X in zip(pairs, chunks):
        p.t.upload_chunk(X)
    idx, dist = ens.bmu_batch()
    score_twins(pairs, (idx, dist))
    mse = ens.batch_epoch([3.0] * K, False)
    for k in range(0, K, 37):
        pairs[k].same(("epoch", k), mse[k], pairs[k].t.batch_epoch(3.0, False))
    ens.close()
    for p in pairs:
        p.close()


def test_refusals_change_nothing():
    pairs = [Pair(10, 10, 9, po.STANDARD, 301), Pair(8, 8, 12, po.MEDIAN, 302), Pair(40, 40, 16, po.STANDARD, 303)]
    chunks = [rows(20, 9, 304), rows(50, 12, 305), rows(300, 16, 306)]
    for p, X in zip(pairs, chunks):
        p.m.upload_chunk(X)
        p.t.upload_chunk(X)
    ens = vsom_amd.Ensemble([p.m for p in pairs])
    L = capi.lib()
    others = [rows(20, 9, 307), rows(50, 12, 308), rows(300, 16, 309)]
    other, offs = pack(others, [None] * 3)
    n = 3

    def call(buf, size, offsets, Bs):
        off = None if offsets is None else (C.c_size_t * n)(*offsets)
        bs = None if Bs is None else (C.c_size_t * n)(*Bs)
        return L.vsom_ensemble_upload_chunks(ens._h, None if buf is None else capi._f(buf), size, off, bs, 1)

    def refused(rc, pattern):
        assert rc != 0
        msg = L.vsom_last_error().decode()
        assert pattern in msg, msg

    refused(call(other, other.size, None, [20, 50, 300]), "null array")
    refused(call(other, other.size, offs, None), "null array")
    refused(call(None, other.size, offs, [20, 50, 300]), "member 0: x_host is null")
    end = offs[2] + 300 * 16                                  # (the buffer holds a gap behind the last range)
    refused(call(other, end - 1, offs, [20, 50, 300]), "member 2: rows beyond n_floats")
    # (accepted: the last member's range ends exactly at n_floats; the twins follow)
    assert call(other, end, offs, [20, 50, 300]) == 0, L.vsom_last_error()
    for p, X in zip(pairs, others):
        p.t.upload_chunk(X)
    refused(call(other, end - 1, offs, [20, 50, 300]), "member 2: rows beyond n_floats")
    refused(call(other, other.size, [offs[0], offs[1] + 10 ** 9, offs[2]], [20, 50, 300]), "member 1: rows beyond")
    refused(call(other, other.size, offs, [20, 0x80000000, 300]), "member 1: chunk too large")
    # scoring: a member whose next chunk is staged ahead over its rows; a member without a chunk
    p = pairs[2]
    pin = capi.PinnedBuffer((300, 16))
    pin.array[:] = rows(300, 16, 310)
    for ctx in (p.m, p.t):
        ctx.batch_epoch_async(3.0, True)
        ctx.prefetch_chunk(pin.array)
    try:
        ens.bmu_batch()
        staged_ahead = False
    except vsom_amd.VsomError as err:
        assert "member 2" in str(err) and "staged ahead" in str(err), err
        staged_ahead = True
    for ctx in (p.m, p.t):
        ctx.commit_chunk()
    fresh = vsom_amd.Context(10, 10, 9)
    ens2 = vsom_amd.Ensemble([pairs[0].m, fresh])
    with pytest.raises(vsom_amd.VsomError, match="member 1: no chunk loaded"):
        ens2.bmu_batch()
    ens2.close()
    fresh.close()
    # nothing changed: the next scoring and training step equal the untouched twins'
    idx, dist = ens.bmu_batch()
    score_twins(pairs, (idx, dist))
    mse = ens.batch_epoch([2.0] * n, False)
    for k, q in enumerate(pairs):
        q.same(("after refusals", k, staged_ahead), mse[k], q.t.batch_epoch(2.0, False))
    ens.close()
    for q in pairs:
        q.close()
    pin.free()
