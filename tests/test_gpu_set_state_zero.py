"""GPU: vsom_set_state turns an array whose bits are all zero into a device fill (csrc/vsom_capi.hip, all_zero_bits) and
copies anything else.  The test walks the edges of that check -- one non-zero element at the first position, at the
first 64-byte boundary, in the last word of the 64-byte blocks, at the last float, a single -0.0 (zero by value, not by
bits) -- for map, sigmaMap, SMap and weightMap, also from views 4 bytes off an 8-byte boundary.  After each set the state
reads back bit for bit and a batch epoch gives the oracle's bits (the fill also covers the rows' pad columns)."""
import numpy as np
import pytest

import gen
import vsom_amd
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

W, H, J = 10, 7, 13            # N * D = 910 floats: 56 blocks of 64 bytes and a tail of 14 floats; D = 13 leaves pads
N = W * H


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _cases(n):
    """(label, position, value) of the one non-zero element of an n-float array"""
    last_block = (n * 4 // 64) * 16 - 1          # last float of the last whole 64-byte block
    out = [("first", 0, 1.5), ("boundary", 16, 2.0), ("last-block", last_block, -3.0), ("last", n - 1, 0.25),
           ("minus-zero", n // 2, -0.0)]
    return [c for c in out if 0 <= c[1] < n]


def _array(n, pos, value, offset):
    buf = np.zeros(n + 2, np.float32)
    base = 2 if buf.ctypes.data % 8 == 0 else 1
    base = base - 1 if offset else base          # offset 1: the view starts 4 bytes off an 8-byte boundary
    a = buf[base:base + n]
    assert (a.ctypes.data % 8 == 4) == bool(offset)
    if pos is not None:
        a[pos] = np.float32(value)
    return a


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("what", ["map", "sigma", "S", "weight"])
def test_zero_fill_edges_of_set_state(what, offset):
    rs = np.random.RandomState(5)
    D = J
    init = gen.random_map(N, D, seed=3)
    X = gen.blobs(90, J, 4, 1, 2)
    ctx = vsom_amd.Context(W, H, J, po.STANDARD)
    n = N if what == "weight" else N * D
    shape = (N,) if what == "weight" else (N, D)
    for label, pos, value in _cases(n) + [("all-zero", None, 0.0)]:
        full = {"map": init, "sigma": (rs.rand(N, D) + 0.5).astype(np.float32),
                "S": (rs.rand(N, D) + 0.5).astype(np.float32), "weight": (rs.rand(N) + 0.5).astype(np.float32),
                "hits": rs.randint(0, 5, size=N).astype(np.uint64)}
        ctx.set_state(**full)                                   # every element non-zero first
        a = _array(n, pos, value, offset)
        ctx.set_state(**{what: a.reshape(shape)})
        st = ctx.get_state()
        assert (_bits(st[what].reshape(-1)) == _bits(a)).all(), (what, label, offset)
        for k in ("map", "sigma", "S", "weight"):
            if k != what:
                assert (_bits(st[k]) == _bits(full[k])).all(), (what, label, k)
        orc = po.OracleSom(W, H, J, po.STANDARD)
        want = dict(full)
        want[what] = np.array(a).reshape(shape)
        orc.set_state(**want)
        ctx.upload_chunk(X)
        lb = np.zeros(X.shape[0], np.uint64)
        mse_o = orc.batch_epoch(X, lb, 2.0, True)
        mse_g = ctx.batch_epoch(2.0, True)
        st = ctx.get_state()
        assert np.float32(mse_g) == np.float32(mse_o) or (np.isnan(mse_g) and np.isnan(mse_o)), (what, label)
        assert (ctx.get_last_bmu() == lb).all(), (what, label)
        # (the batch epoch leaves SMap as it was set -- Som.cpp's phase 2 sums into a local -- and adds to bmuHits)
        for k, ref in (("map", orc.map), ("sigma", orc.sigma), ("S", orc.S), ("weight", orc.weight)):
            assert _same(st[k], ref), (what, label, k)
        assert (st["hits"] == orc.hits).all(), (what, label)
        orc.close()
    ctx.close()
