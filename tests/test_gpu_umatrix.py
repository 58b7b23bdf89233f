"""GPU: vsom_umatrix -- Som::updateUMatrix (Som.cpp:999-1111) as one stencil launch -- against the CPU oracle's
restatement, bit for bit (float64 bit patterns; NaN in the same places, payloads not compared), and against the earlier
route (vsom_distances_raw over a pair list, combined on the host)."""
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

SHAPES = [(2, 2), (2, 3), (3, 2), (3, 3), (5, 4), (10, 10), (17, 33), (64, 64)]
DEPTHS = [1, 3, 4, 7, 8, 9, 12, 15, 784, 794]
CLR_J = [3, 4, 9]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(((na & nb) | (~na & ~nb & (a.view(np.uint64) == b.view(np.uint64)))).all())


def feq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        w = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return bool(((a.view(w) == b.view(w)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def random_state(N, D, seed):
    rs = np.random.RandomState(seed)
    m = gen.random_map(N, D, seed=seed)
    s = (rs.rand(N, D) * 0.5).astype(np.float32)
    s[rs.rand(N, D) < 0.1] = 0.0                          # the 1e-5 floor
    return m, s


def pair(W, H, J, tr, m, s):
    ctx = vsom_amd.Context(W, H, J, tr)
    o = po.OracleSom(W, H, J, tr)
    ctx.set_state(map=m, sigma=s)
    o.set_state(map=m, sigma=s)
    return ctx, o


def pair_list_umatrix(ctx):
    """the earlier route: (node, neighbour) pairs through vsom_distances_raw, combined in double on the host in the
    reference's order of additions"""
    W, H = ctx.width, ctx.height
    DI = (0, 0, 1, -1, -1, 1, -1, 1)       # W, E, S(i+1), N(i-1), NW, SW, NE, SE
    DJ = (-1, 1, 0, 0, -1, -1, 1, 1)
    nodes, nbrs, slot = [], [], {}
    for i in range(H):
        for j in range(W):
            for k in range(8):
                ni, nj = i + DI[k], j + DJ[k]
                if 0 <= ni < H and 0 <= nj < W:
                    slot[(i * W + j, k)] = len(nodes)
                    nodes.append(i * W + j)
                    nbrs.append(ni * W + nj)
    d = ctx.distances_raw(nodes, nbrs, True).astype(np.float64)
    f = 0.3
    Wk, Ek, Sk, Nk, NWk, SWk, NEk, SEk = range(8)
    U = np.zeros(W * H, np.float64)
    for i in range(H):
        for j in range(W):
            n = i * W + j
            R = lambda k: float(d[slot[(n, k)]])   # noqa: E731
            if 0 < j < W - 1 and 0 < i < H - 1:
                u = (R(Wk) + R(Ek) + R(Sk) + R(Nk) + R(NWk) * f + R(SWk) * f + R(NEk) * f + R(SEk) * f) / 8
            elif i == 0 and 0 < j < W - 1:
                u = (R(Wk) + R(Ek) + R(Sk) + R(SWk) * f + R(SEk) * f) / 5
            elif i == H - 1 and 0 < j < W - 1:
                u = (R(Wk) + R(Ek) + R(Nk) + R(NWk) * f + R(NEk) * f) / 5
            elif j == 0 and 0 < i < H - 1:
                u = (R(Ek) + R(Sk) + R(Nk) + R(NEk) * f + R(SEk) * f) / 5
            elif j == W - 1 and 0 < i < H - 1:
                u = (R(Wk) + R(Sk) + R(Nk) + R(NWk) * f + R(SWk) * f) / 5
            elif j == 0 and i == 0:
                u = (R(Ek) + R(Sk) + R(SEk) * f) / 3
            elif j == W - 1 and i == 0:
                u = (R(Wk) + R(Sk) + R(SWk) * f) / 3
            elif j == 0 and i == H - 1:
                u = (R(Ek) + R(Nk) + R(NEk) * f) / 3
            else:
                u = (R(Wk) + R(Nk) + R(NWk) * f) / 3
            U[n] = u
    return U


@pytest.mark.parametrize("W, H", SHAPES)
def test_matches_the_oracle_every_position_class_and_tail(W, H):
    """Standard and Median over every depth (reduction tails D mod 8 in {0, 1, 3, 4, 7}, D < 4, several LDS blocks), CLR
    with J in {3, 4, 9} (D = J(J-1): the A | pad | B layout); the shapes put a node in each of the nine position classes"""
    for tr, Js in ((po.STANDARD, DEPTHS), (po.MEDIAN, DEPTHS), (po.CLR, CLR_J)):
        for J in Js:
            D = po.length(tr, J)
            m, s = random_state(W * H, D, seed=1000 * tr + J)
            ctx, o = pair(W, H, J, tr, m, s)
            u, uo = ctx.umatrix(), o.update_umatrix()
            ctx.close()
            o.close()
            assert u.dtype == np.float64 and u.shape == (W * H,)
            assert np.isfinite(uo).all() and (uo > 0).all()
            assert same_bits(u, uo), (tr, J, np.flatnonzero(u != uo)[:8])


@pytest.mark.parametrize("W, H, J, tr", [(128, 128, 784, po.STANDARD), (130, 129, 5, po.STANDARD), (131, 127, 4, po.CLR)])
def test_large_maps(W, H, J, tr):
    """the headline shape, and large maps whose last tiles are partial in both directions"""
    D = po.length(tr, J)
    m, s = random_state(W * H, D, seed=5)
    ctx, o = pair(W, H, J, tr, m, s)
    u, uo = ctx.umatrix(), o.update_umatrix()
    ctx.close()
    assert same_bits(u, uo)


def engineered(N, D, seed):
    """sigma values around the select and outside the numbers; map rows with NaN, +-inf and exact duplicates"""
    rs = np.random.RandomState(seed)
    m, s = random_state(N, D, seed)
    t = np.float32(0.00001)
    special = np.array([0.0, -0.0, -1.0, t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)),
                        1e-40, -1e-40, np.float32(1.4e-45), -np.inf], np.float32)
    pick = rs.rand(N, D) < 0.3
    s[pick] = special[rs.randint(0, special.size, size=int(pick.sum()))]
    for n in rs.choice(N, size=max(1, N // 5), replace=False):
        m[n] = m[(n + 1) % N]                             # a neighbour (or the wrap) bit for bit
    for n in rs.choice(N, size=max(1, N // 8), replace=False):          # (a few: most results stay numbers)
        s[n, rs.randint(0, D)] = [np.nan, np.inf][rs.randint(0, 2)]
    for k, n in enumerate(rs.choice(N, size=max(1, N // 8), replace=False)):
        m[n, rs.randint(0, D)] = [np.nan, np.inf, -np.inf][k % 3]
    return m, s


@pytest.mark.parametrize("W, H, J, tr", [(3, 3, 9, po.STANDARD), (10, 10, 15, po.MEDIAN), (9, 7, 4, po.CLR),
                                         (17, 33, 70, po.STANDARD), (6, 5, 9, po.CLR)])
def test_engineered_sigma_and_map_values(W, H, J, tr):
    D = po.length(tr, J)
    m, s = engineered(W * H, D, seed=77 + J)
    ctx, o = pair(W, H, J, tr, m, s)
    u, uo = ctx.umatrix(), o.update_umatrix()
    ctx.close()
    assert (~np.isfinite(uo)).any() and np.isfinite(uo).any()
    assert same_bits(u, uo)


def test_all_rows_equal_gives_exact_zero():
    W, H, J = 7, 6, 12
    m = np.tile(gen.random_map(1, J, seed=3), (W * H, 1))
    s = (np.random.RandomState(1).rand(W * H, J) * 0.5).astype(np.float32)
    ctx, o = pair(W, H, J, po.STANDARD, m, s)
    u = ctx.umatrix()
    ctx.close()
    assert (u.view(np.uint64) == 0).all() and same_bits(u, o.update_umatrix())


def test_poisoned_map_after_a_batch_epoch_with_small_sigma():
    """a batch epoch with a small sigma leaves nodes whose first weight is 0/0: NaN rows in map and sigmaMap"""
    W, H, J = 36, 36, 16
    X = gen.blobs(200, J, 5, 1, 2, sigma=0.2)
    init = gen.random_map(W * H, J, seed=9)
    ctx = vsom_amd.Context(W, H, J)
    o = po.OracleSom(W, H, J)
    ctx.set_state(map=init)
    o.set_state(map=init)
    ctx.upload_chunk(X)
    ctx.batch_epoch(0.05, True)
    o.batch_epoch(X, np.zeros(200, np.uint64), 0.05, True)
    st = ctx.get_state()
    assert np.isnan(st["map"]).any() and feq(st["map"], o.map) and feq(st["sigma"], o.sigma)
    u, uo = ctx.umatrix(), o.update_umatrix()
    ctx.close()
    assert np.isnan(uo).any() and same_bits(u, uo)


@pytest.mark.parametrize("W, H, J, tr", [(12, 9, 13, po.STANDARD), (8, 8, 6, po.CLR), (20, 20, 40, po.MEDIAN)])
def test_after_real_training(W, H, J, tr):
    """two batch epochs and one online chunk, then umatrix() == the oracle's on its own trained state"""
    X = gen.correlated(120, J, 5) if tr == po.CLR else gen.blobs(120, J, 4, 1, 2, sigma=0.4)
    init = gen.random_map(W * H, po.length(tr, J), seed=21)
    ctx = vsom_amd.Context(W, H, J, tr)
    o = po.OracleSom(W, H, J, tr)
    ctx.set_state(map=init)
    o.set_state(map=init)
    lb = np.zeros(120, np.uint64)
    ctx.upload_chunk(X)
    for e in range(2):
        ctx.batch_epoch(3.0 - e, e == 0)
        o.batch_epoch(X, lb, 3.0 - e, e == 0)
    ctx.train_online_chunk(0.3, 2.0, capi.EXPONENTIAL)
    o.train_online_chunk(X, lb, 0.3, 2.0, capi.EXPONENTIAL)
    st = ctx.get_state()
    assert feq(st["map"], o.map) and feq(st["sigma"], o.sigma)
    u = ctx.umatrix()
    ctx.close()
    assert same_bits(u, o.update_umatrix())


def test_enqueue_only_then_get_returns_the_first_state():
    W, H, J = 40, 30, 50
    m1, s1 = random_state(W * H, J, seed=1)
    m2, s2 = random_state(W * H, J, seed=2)
    ctx, o = pair(W, H, J, po.STANDARD, m1, s1)
    assert ctx.device_ptr(capi.BUF_UMATRIX) == 0
    assert ctx.umatrix(fetch=False) is None
    ctx.set_state(map=m2, sigma=s2)
    u = ctx.get_umatrix()
    assert same_bits(u, o.update_umatrix())
    assert ctx.device_ptr(capi.BUF_UMATRIX) != 0
    assert same_bits(ctx.get_umatrix(), u)                   # still the last call's
    o.set_state(map=m2, sigma=s2)
    u2 = ctx.umatrix()
    assert same_bits(u2, o.update_umatrix()) and not same_bits(u2, u)
    ctx.close()


def test_read_only_with_no_chunk_and_with_a_chunk_staged_ahead():
    W, H, J = 64, 64, 784
    m, s = random_state(W * H, J, seed=4)
    ctx, o = pair(W, H, J, po.STANDARD, m, s)
    uo = o.update_umatrix()
    assert same_bits(ctx.umatrix(), uo)                       # no chunk loaded
    X0, X1 = gen.mnist_like(256, 3, J), gen.mnist_like(256, 4, J)
    ctx.upload_chunk(X0)
    ctx.batch_epoch(8.0, True)
    before, lb, sq = ctx.get_state(), ctx.get_last_bmu(), ctx.get_sqres()
    u = ctx.umatrix()
    after = ctx.get_state()
    for k in before:
        assert feq(before[k], after[k]), k
    assert feq(lb, ctx.get_last_bmu()) and feq(sq, ctx.get_sqres())
    # the next chunk staged beside a running epoch: the rows are the next chunk's, the U-matrix does not read them
    pin = capi.PinnedBuffer(X1.shape)
    pin.array[:] = X1
    ctx.batch_epoch_async(6.0, False)
    ctx.prefetch_chunk(pin.array)
    u_ahead = ctx.umatrix()
    st = ctx.get_state()
    ctx.commit_chunk()
    o.set_state(map=st["map"], sigma=st["sigma"])
    assert same_bits(u_ahead, o.update_umatrix())
    o.set_state(map=before["map"], sigma=before["sigma"])
    assert same_bits(u, o.update_umatrix())
    ctx.batch_epoch(5.0, False)                               # the committed chunk trains
    ctx.close()
    pin.free()


@pytest.mark.parametrize("W, H, J, tr", [(9, 7, 13, po.STANDARD), (6, 5, 5, po.CLR), (12, 12, 32, po.MEDIAN),
                                         (2, 2, 3, po.STANDARD), (3, 2, 9, po.CLR)])
def test_equals_the_pair_list_route(W, H, J, tr):
    """Som.updateUMatrix (the new path) == the combination of Context.distances_raw pairs (the route it replaces)"""
    D = po.length(tr, J)
    m, s = engineered(W * H, D, seed=31) if W > 3 else random_state(W * H, D, seed=31)
    som = vs.Som(W, H, D, vs.Transformation(tr))
    som.setState(map=m, sigma=s)
    u = som.updateUMatrix()
    assert u is som.uMatrix and same_bits(som.getUMatrix(), u)
    assert same_bits(u, pair_list_umatrix(som.ctx))
    som.close()


def test_refusals_leave_the_context_usable():
    W, H, J = 6, 5, 7
    d, r = hooks.shape("standard", J)
    cu = capi.Context(W, H, J, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=d, residual_len=r)
    plain = vsom_amd.Context(W, H, J)
    X = gen.blobs(40, J, 3, 1, 2, sigma=0.3)
    init = gen.random_map(W * H, J, seed=2)
    for ctx in (cu, plain):
        ctx.set_state(map=init)
    with pytest.raises(vsom_amd.VsomError, match="custom"):
        cu.umatrix()
    with pytest.raises(vsom_amd.VsomError, match="custom"):
        cu.umatrix(fetch=False)
    with pytest.raises(vsom_amd.VsomError, match="no vsom_umatrix"):
        plain.get_umatrix()
    assert plain.device_ptr(capi.BUF_UMATRIX) == 0 and cu.device_ptr(capi.BUF_UMATRIX) == 0
    # degenerate maps: the C call itself refuses (the wrapper would, before it)
    thin = vsom_amd.Context(1, 5, J)
    u = np.zeros(5, np.float64)
    rc = capi.lib().vsom_umatrix(thin._h, u.ctypes.data_as(capi.C.POINTER(capi.C.c_double)))
    assert rc == -1
    with pytest.raises(vsom_amd.VsomError, match="width >= 2 and height >= 2"):
        capi.check(rc)
    thin.close()
    # both train as usual afterwards, to the same state
    mses = []
    for ctx in (cu, plain):
        ctx.upload_chunk(X)
        mses.append(ctx.batch_epoch(2.0, True))
    a, b = cu.get_state(), plain.get_state()
    assert feq(mses[0], mses[1]) and feq(a["map"], b["map"]) and feq(a["sigma"], b["sigma"])
    o = po.OracleSom(W, H, J)
    o.set_state(map=b["map"], sigma=b["sigma"])
    assert same_bits(plain.umatrix(), o.update_umatrix())
    cu.close()
    plain.close()


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401  (before the first vsom_amd call: one HIP runtime)
import test_gpu_umatrix as t
from oracle import pyoracle as po
for (W, H, J, tr) in ((17, 33, 15, po.STANDARD), (10, 10, 4, po.CLR), (5, 4, 794, po.MEDIAN), (2, 2, 3, po.STANDARD)):
    m, s = t.engineered(W * H, po.length(tr, J), seed=3)
    ctx, o = t.pair(W, H, J, tr, m, s)
    assert t.same_bits(ctx.umatrix(), o.update_umatrix()), (W, H, J, tr)
    ctx.close()
print("umatrix child ok")
"""


@pytest.mark.parametrize("env", [{"VSOM_NO_TINY": "1"}, {"VSOM_NO_CHAIN": "1"}, {"VSOM_NO_COMPACT": "1"},
                                 {"VSOM_COMPACT_MIN_ROWS": "1"}, {"VSOM_NO_DEDUPE": "1"}])
def test_switches_leave_the_result_unchanged(env):
    """every kernel-selection switch of the README (a fresh child process per setting: the switches are read once)"""
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert r.returncode == 0 and "umatrix child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
