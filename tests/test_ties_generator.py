"""CPU: tests/ties.py delivers the tie cases tests/test_gpu_ties.py relies on -- exact ties between rows that are not
bit-identical, one-ulp cases won by the higher index, cases the fp32 summation order decides, the boundary placements --
and the oracle's own searches name every certified winner."""
import numpy as np
import pytest

import ties
from oracle import pyoracle as po


def _live(case):
    return [c for c in case.certs if c is not None]


def _check_certs(case):
    for c in _live(case):
        a, b = c["pair"]
        assert c["margin_ok"], (case.name, c["pair"])                  # the pair holds the two nearest rows
        assert c["winner"] in (a, b) and c["runner_up"] in (a, b) and c["winner"] != c["runner_up"]
        dw, dr = c["d32"]
        assert dw <= dr and c["gap_ulps"] == ties.ulps(dw, dr) >= 0
        if dw == dr:
            assert c["winner"] == a < b                                 # strict <: the lower index
        assert c["rows_differ"]
        if c["kind"] == "mirror":
            assert c["gap_ulps"] == 0
            assert c["d64"][0] == c["d64"][1], (case.name, c)           # a tie in plain float64 arithmetic too
        if c["kind"] in ("ulp_lo", "ulp_hi"):
            assert c["gap_ulps"] <= 4


@pytest.mark.parametrize("name", list(ties.BATCH))
def test_batch_cases(name):
    case = ties.batch(name)
    W, H, J, B = case.W, case.H, case.J, case.X.shape[0]
    N = W * H
    _check_certs(case)
    K = 5 if B >= 100 else 2
    assert case.exact_ties() >= K, name
    if name.startswith("cancel"):
        # around 1e3: every distance is tiny beside |M|^2, the mirrors are the point
        assert case.count("mirror") == B
        assert np.abs(case.X).min() > 1e3 and np.ptp(case.X, axis=0).max() < 0.05
    elif name.startswith("u8edge"):
        # every value of a pair's rows 7/16 of a digit step (2^-12) off the grid, the lower node above it, the higher below
        assert case.count("mirror") == B
        for c in case.certs[:64]:
            a, b = c["pair"]
            ra = case.init[a].astype(np.float64) - np.round(case.init[a].astype(np.float64) * 4096) / 4096
            rb = case.init[b].astype(np.float64) - np.round(case.init[b].astype(np.float64) * 4096) / 4096
            assert (ra == 7 * 2.0 ** -16).all() and (rb == -7 * 2.0 ** -16).all()
            assert 128 <= np.abs(case.init[a]).max() < 256 and 128 <= np.abs(case.init[b]).max() < 256
    else:
        assert case.hi_wins() >= K, name
        assert case.order_decided() >= K, name
    if name.startswith(("u8", "dead_u8")):
        assert (case.X == np.round(case.X)).all() and case.X.min() >= 0 and case.X.max() <= 255
    # the placements: node 0 and node N-1, the 64-node tile / wavefront, the refinement's 32 nodes and 16 slots,
    # pairs whose lower index lies in the winner's tile and far from it
    pairs = {c["pair"] for c in case.certs}
    assert any(a == 0 for a, _ in pairs) and any(b == N - 1 for _, b in pairs)
    assert (63, 64) in pairs and (31, 32) in pairs
    assert any(a // 64 != b // 64 and b - a < 4 for a, b in pairs) and any(b - a > N // 2 for a, b in pairs)
    assert any(a % 16 == b % 16 for a, b in pairs)
    hi = [c["pair"] for c in case.certs if c["winner"] == c["pair"][1] and c["gap_ulps"] > 0]
    if hi:
        assert any(b // 64 - a // 64 <= 1 for a, b in hi) and any(b // 64 - a // 64 > 1 for a, b in hi) or N <= 128
    zero = [c for c in case.certs if c["pair"][0] == 0 and c["gap_ulps"] == 0]
    assert all(c["winner"] == 0 for c in zero)
    # the oracle's searches name the certified winners, with the certified distances
    B = B // case.repeat                      # a repeated chunk: its first block holds every planted sample
    o = po.OracleSom(W, H, J, case.tr)
    o.set_state(map=case.init)
    lb, sq = np.zeros(B, np.uint64), np.zeros(B, np.float32)
    o.batch_phase1_range(case.X, 0, B, lb, sq, True, nthreads=8)
    want = np.array([c["winner"] for c in case.certs[:B]], np.uint64)
    assert (lb == want).all(), name
    assert (sq == np.array([c["d32"][0] for c in case.certs[:B]], np.float32)).all()
    for s in range(0, B, max(1, B // 8)):
        assert o.find_bmu(case.X[s]) == case.certs[s]["winner"]
    o.close()


@pytest.mark.parametrize("name", list(ties.ONLINE))
def test_online_cases(name):
    case = ties.online(name)
    _check_certs(case)
    live = _live(case)
    assert len(live) >= 6 and case.exact_ties() >= 2, name
    assert case.hi_wins() >= 1 or case.W * case.H <= 1024, name
    # replayed from the final initial map, the oracle takes the path the construction took, and every planted sample's
    # BMU is its certified winner
    o, lb, mse = ties.replay_online(case)
    assert (lb == case.lb).all() and np.array_equal(o.map.view(np.uint32), case.final_map.view(np.uint32))
    for j, c in enumerate(case.certs):
        if c is None:
            continue
        a, b = c["window_node"], c["image_node"]
        assert lb[j] == c["winner"], (name, j)
        assert lb[j - 1] == a                                  # a: the previous sample's BMU, rewritten by its window
        assert not np.array_equal(case.init[a], o.map[a])
        # b never changed before sample j: its row in the initial map is the one sample j meets
        o2 = po.OracleSom(case.W, case.H, case.J, case.tr)
        o2.set_state(map=case.init)
        o2.train_online_chunk(case.X[:j], np.zeros(j, np.uint64), case.eta, case.sigma, case.decay_fn)
        assert np.array_equal(o2.map[b].view(np.uint32), case.init[b].view(np.uint32)), (name, j)
        assert o2.find_bmu(case.X[j]) == c["winner"]
        assert np.float32(o2.dist(c["winner"], case.X[j])) == c["d32"][0]
        o2.close()
    o.close()


def test_eigen_order_sum_is_the_oracles():
    rs = np.random.RandomState(0)
    for n in (1, 3, 4, 5, 7, 8, 9, 12, 33, 784):
        R = (rs.randn(6, n) * 10.0 ** rs.randint(-3, 4, size=(6, 1))).astype(np.float32)
        got = ties.eigen_sq(R)
        for r, g in zip(R, got):
            assert po.dot_self(r).view(np.uint32) == np.float32(g).view(np.uint32), n


@pytest.mark.parametrize("name", list(ties.ONLINE_EDGE))
def test_online_edge_cases(name):
    case = ties.online_edge(name)
    _check_certs(case)
    assert len(case.certs) == case.X.shape[0] and case.exact_ties() == len(case.certs)
    o, lb, _ = ties.replay_online(case)
    assert (lb == case.lb).all() and np.array_equal(o.map.view(np.uint32), case.final_map.view(np.uint32))
    assert all(lb[j] == c["winner"] == c["pair"][0] for j, c in enumerate(case.certs))
    # the strides of the online kernels: neighbouring refinement workgroups (1), the 16 key slots, one workgroup's
    # 32 lanes, nref = ceil(N / 32) (the same refinement workgroup), the 64-node wavefront
    nref = -(-case.W * case.H // 32)
    steps = {c["pair"][1] - c["pair"][0] for c in case.certs}
    assert {1, 16, 32, nref, 64} <= steps
    for c in case.certs:
        a, b = c["pair"]
        assert (case.init[a] - np.round(case.init[a]) == np.float32(31 / 64)).all()
        assert (case.init[b] - np.round(case.init[b]) == np.float32(-31 / 64)).all()
        assert 64 <= case.init[a].max() < 128 and 64 <= case.init[b].max() < 128
    o.close()
