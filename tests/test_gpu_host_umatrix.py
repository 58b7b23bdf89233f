"""GPU: Som::updateUMatrix of the C++ mirror (host/tests/host_umatrix_test.cpp) on what the other C++ dump tests do not
reach -- non-square maps in both directions (node n sits at row n // W, column n % W), a
StandardMedianEstimator map and a non-square CLR map -- on one GPU and through a three-member group on one device
(VSOM_DEVICES=0,0,0).  The mirror's matrix must equal the oracle's on the dumped state and the Python binding's, bit for
bit (NaN in the same places)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import vsom_amd
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")


def same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return bool(((na & nb) | (~na & ~nb & (a.view(np.uint64) == b.view(np.uint64)))).all())


def read_case(path):
    raw = open(path, "rb").read()
    W, H, J, kind, D = (int(x) for x in np.frombuffer(raw[:40], np.uint64))
    N, off = W * H, 40
    out = {"W": W, "H": H, "J": J, "kind": kind, "D": D}
    for key, dt, cnt in (("map", np.float32, N * D), ("sigma", np.float32, N * D), ("U", np.float64, N)):
        out[key] = np.frombuffer(raw, dt, cnt, off).copy()
        off += cnt * np.dtype(dt).itemsize
    assert off == len(raw)
    return out


@pytest.mark.parametrize("mode", ["single", "group3"])
def test_cpp_umatrix_nonsquare_and_median(mode):
    exe = os.path.join(HOST, "host_umatrix_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    d = tempfile.mkdtemp(prefix="vsom_um_")
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    if mode == "group3":
        env["VSOM_DEVICES"] = "0,0,0"
    res = subprocess.run([exe, d], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert ("group_members=3" if mode == "group3" else "group_members=1") in res.stdout
    assert "cases=4" in res.stdout and "host_umatrix_test ok" in res.stdout
    seen = set()
    for k in range(4):
        f = read_case(os.path.join(d, f"umatrix_{k}.bin"))
        W, H, J, kind, D = f["W"], f["H"], f["J"], f["kind"], f["D"]
        assert D == po.length(kind, J)
        seen.add((kind, W > H, W < H))
        m, s = f["map"].reshape(W * H, D), f["sigma"].reshape(W * H, D)
        o = po.OracleSom(W, H, J, kind)
        o.set_state(map=m, sigma=s)
        uo = o.update_umatrix()
        assert np.isfinite(uo).any()
        assert same_bits(f["U"], uo), k
        ctx = vsom_amd.Context(W, H, J, kind)
        ctx.set_state(map=m, sigma=s)
        assert same_bits(ctx.umatrix(), f["U"]), k
        ctx.close()
        # the transposed reading of the grid (H columns) is a different matrix: the comparison above can tell
        ot = po.OracleSom(H, W, J, kind)
        ot.set_state(map=m, sigma=s)
        assert not same_bits(ot.update_umatrix(), uo), k
    assert {(0, True, False), (0, False, True), (1, False, True), (2, True, False)} <= seen
