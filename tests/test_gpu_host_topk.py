"""GPU: Som::findBestMatchingUnits and Som::topographicError of the C++ mirror (host/tests/host_topk_test.cpp), on one
GPU and through a three-member group on one device (VSOM_DEVICES=0,0,0).  The mirror's lists, distances and topographic
error must equal the Python binding's bit for bit, and the error that of the oracle's top-2."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import vsom_amd
from vsom_amd import som as vs
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")


def read_topk(path):
    raw = open(path, "rb").read()
    W, H, J, n, k = (int(x) for x in np.frombuffer(raw[:40], np.uint64))
    N, off = W * H, 40
    out = {"W": W, "H": H, "J": J, "n": n, "k": k}
    for key, dt, cnt in (("map", np.float32, N * J), ("rows", np.float32, n * J), ("idx", np.uint64, n * k),
                         ("dist", np.float32, n * k), ("te", np.float64, 1)):
        out[key] = np.frombuffer(raw, dt, cnt, off)
        off += cnt * np.dtype(dt).itemsize
    assert off == len(raw)
    return out


@pytest.mark.parametrize("mode", ["single", "group3"])
def test_cpp_topk_and_topographic_error(mode):
    exe = os.path.join(HOST, "host_topk_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    d = tempfile.mkdtemp(prefix="vsom_topk_")
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    if mode == "group3":
        env["VSOM_DEVICES"] = "0,0,0"
    res = subprocess.run([exe, d], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert ("group_members=3" if mode == "group3" else "group_members=1") in res.stdout
    assert "refusals ok" in res.stdout
    f = read_topk(os.path.join(d, "topk.bin"))
    W, H, J, n, k = f["W"], f["H"], f["J"], f["n"], f["k"]
    rows = f["rows"].reshape(n, J)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=f["map"].reshape(W * H, J))
    ctx.upload_chunk(rows)
    idx, dist = ctx.bmu_topk(k)
    ctx.close()
    assert (idx.ravel() == f["idx"]).all()
    assert (dist.ravel().view(np.uint32) == f["dist"].view(np.uint32)).all()
    te = float(f["te"][0])
    assert te == vs.topographic_error(idx[:, :2], W)
    # the oracle's top-2 of every row
    o = po.OracleSom(W, H, J)
    o.set_state(map=f["map"].reshape(W * H, J))
    top2 = np.zeros((n, 2), np.uint64)
    for r in range(n):
        dd = np.array([o.dist(i, rows[r]) for i in range(W * H)], np.float32)
        key = (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(W * H, dtype=np.uint64)
        top2[r] = np.argsort(key)[:2]
    assert te == vs.topographic_error(top2, W)
