"""GPU: vsom_ensemble_umatrix -- every member's U-matrix in one call: small members in one launch per kind, the others
through vsom_umatrix.  Each member's matrix must equal that member's own vsom_umatrix and the oracle's, bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_hooks as hooks  # noqa: E402
from test_gpu_umatrix import engineered, random_state, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

# (W, H, J, kind): small Standard / Median / CLR members (N * part_len <= 4096), one member above that limit
# (40 x 40 x 16), a CLR member above it (12 x 12 x 9: 144 * 36), non-square and 2-wide maps
SPECS = [(10, 10, 9, po.STANDARD), (8, 8, 12, po.MEDIAN), (6, 6, 5, po.CLR), (40, 40, 16, po.STANDARD),
         (12, 9, 20, po.MEDIAN), (2, 3, 7, po.STANDARD), (7, 5, 4, po.CLR), (12, 12, 9, po.CLR), (64, 64, 1, po.STANDARD)]


def members(specs):
    out = []
    for k, (W, H, J, tr) in enumerate(specs):
        D = po.length(tr, J)
        m, s = engineered(W * H, D, seed=50 + k) if k % 2 else random_state(W * H, D, seed=50 + k)
        ctx = vsom_amd.Context(W, H, J, tr)
        ctx.set_state(map=m, sigma=s)
        o = po.OracleSom(W, H, J, tr)
        o.set_state(map=m, sigma=s)
        out.append((ctx, o))
    return out


@pytest.mark.parametrize("layout", ["own_streams", "shared", "two_streams"])
def test_every_member_equals_its_single_call_and_the_oracle(layout):
    import torch
    ms = members(SPECS)
    if layout != "own_streams":
        dev = torch.device("cuda", 0)
        shared, apart = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        for k, (ctx, _) in enumerate(ms):
            ctx.set_stream((apart if layout == "two_streams" and k in (1, 3) else shared).cuda_stream)
    ens = vsom_amd.Ensemble([c for c, _ in ms])
    us = ens.umatrix()
    assert len(us) == len(ms)
    for k, ((ctx, o), u) in enumerate(zip(ms, us)):
        assert same_bits(u, o.update_umatrix()), k
        assert ctx.device_ptr(capi.BUF_UMATRIX) != 0
        assert same_bits(ctx.get_umatrix(), u), k          # left in the member's own buffer
        assert same_bits(ctx.umatrix(), u), k
    # a second call after a member's state changed
    m, s = random_state(100, 9, seed=99)
    ms[0][0].set_state(map=m, sigma=s)
    ms[0][1].set_state(map=m, sigma=s)
    us = ens.umatrix()
    for k, ((ctx, o), u) in enumerate(zip(ms, us)):
        assert same_bits(u, o.update_umatrix()), k
    ens.close()
    for ctx, _ in ms:
        ctx.synchronize()
        ctx.set_stream(None)
        ctx.close()


def test_null_entries_are_skipped():
    ms = members(SPECS[:5])
    ens = vsom_amd.Ensemble([c for c, _ in ms])
    dp = C.POINTER(C.c_double)
    out = [np.full(c.n_nodes, -7.0, np.float64) for c, _ in ms]
    want = [True, False, True, False, True]                  # (member 3 is the large one: skipped; member 4 wanted)
    ptrs = (dp * len(ms))(*[a.ctypes.data_as(dp) if w else None for a, w in zip(out, want)])
    capi.check(capi.lib().vsom_ensemble_umatrix(ens._h, ptrs))
    for k, ((ctx, o), a, w) in enumerate(zip(ms, out, want)):
        if w:
            assert same_bits(a, o.update_umatrix()), k
        else:
            assert (a == -7.0).all(), k
        assert same_bits(ctx.get_umatrix(), o.update_umatrix()), k      # computed all the same
    # no output array at all
    m, s = random_state(64, 12, seed=98)
    ms[1][0].set_state(map=m, sigma=s)
    ms[1][1].set_state(map=m, sigma=s)
    capi.check(capi.lib().vsom_ensemble_umatrix(ens._h, None))
    assert same_bits(ms[1][0].get_umatrix(), ms[1][1].update_umatrix())
    ens.close()
    for ctx, _ in ms:
        ctx.close()


def test_a_custom_member_refuses_the_call_and_nothing_changes():
    ms = members(SPECS[:4])
    W, H, J = 6, 5, 7
    d, r = hooks.shape("standard", J)
    cu = capi.Context(W, H, J, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=d, residual_len=r)
    thin = vsom_amd.Context(1, 4, 5)
    ctxs = [ms[0][0], ms[1][0], cu, ms[2][0], thin, ms[3][0]]
    ens = vsom_amd.Ensemble(ctxs)
    first = ms[0][0].umatrix()
    m, s = random_state(100, 9, seed=97)
    ms[0][0].set_state(map=m, sigma=s)
    states = [c.get_state() for c, _ in ms]
    dp = C.POINTER(C.c_double)
    out = [np.full(c.n_nodes, -7.0, np.float64) for c in ctxs]
    ptrs = (dp * len(ctxs))(*[a.ctypes.data_as(dp) for a in out])
    rc = capi.lib().vsom_ensemble_umatrix(ens._h, ptrs)
    assert rc == -1
    with pytest.raises(vsom_amd.VsomError, match="member 2.*custom"):
        capi.check(rc)
    assert all((a == -7.0).all() for a in out)
    assert same_bits(ms[0][0].get_umatrix(), first)          # nothing was enqueued for the others
    for k in (1, 2, 3):
        assert ms[k][0].device_ptr(capi.BUF_UMATRIX) == 0
    for (c, _), st in zip(ms, states):
        now = c.get_state()
        for key in st:
            a, b = st[key], now[key]
            assert ((a == b) | ((a != a) & (b != b))).all(), key
    with pytest.raises(ValueError, match="member 4"):         # the Python wrapper names the degenerate member first
        ens.umatrix()
    ens.close()
    # without the custom member the degenerate one is named by the library
    ens = vsom_amd.Ensemble([ms[1][0], thin])
    rc = capi.lib().vsom_ensemble_umatrix(ens._h, None)
    assert rc == -1
    with pytest.raises(vsom_amd.VsomError, match="member 1.*width >= 2"):
        capi.check(rc)
    ens.close()
    cu.close()
    thin.close()
    for c, _ in ms:
        c.close()
