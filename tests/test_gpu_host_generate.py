"""GPU: Som::generateRows, Som::decodeUnits and Som::autoEncoder of the C++ mirror (host/tests/host_generate_test.cpp) on a
10x10x9 state over 20 rows.  The mirror's units and records, for the random numbers the driver prints, must equal the Python
binding's on the same state bit for bit and lie within the stated bound of the float64 restatement.  autoEncoder seeds itself
from the clock and does not print its L, so its text is held to the reference's line structure, and every printed value to
the range any unit's record can take with L on the reference's grid (node 0's alone where no row has mass); the driver itself
asserts that the call downloads no model state."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generate_ref as ref  # noqa: E402
from generate_ref import beq  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")
W, H, J, B = 10, 10, 9, 20
ZMAX = math.log(999.0) / 1.6               # |log(L / (1 - L)) / 1.6| at L = 0.001 and L = 0.999, the ends of the grid


def floats(tok, dtype):
    return np.array([float.fromhex(t) for t in tok], dtype)


def ints(tok):
    return np.array([int(t) for t in tok], np.uint64)


def check_text(lines, X, lo, hi):
    """Som.cpp:598-619: per row, per column the value and `name \\t sample \\t`, then an empty line"""
    assert len(lines) == B * (2 * J + 1)
    at = 0
    for r in range(B):
        for k in range(J):
            assert np.float32(float(lines[at])) == np.float32(float(f"{X[r, k]:.6g}")), (r, k, lines[at])
            name, value, rest = lines[at + 1].split("\t")
            assert name == f"c{k}" and rest == ""
            v = float(value)                            # (six significant digits)
            assert not math.isnan(v)
            if math.isinf(v):
                assert v < 0                            # L = 0 is on the grid (one value in a thousand), L = 1 is not
            else:
                slack = 1e-5 * max(abs(lo[k]), abs(hi[k]), 1.0)
                assert lo[k] - slack <= v <= hi[k] + slack, (r, k, v, lo[k], hi[k])
            at += 2
        assert lines[at] == ""
        at += 1


def test_cpp_generate_rows_and_auto_encoder():
    exe = os.path.join(HOST, "host_generate_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_generate_test ok" in res.stdout and "state_downloads_by_autoencoder=0" in res.stdout
    lines = res.stdout.split("\n")
    f = {}
    for ln in lines[:lines.index("autoencoder_begin")]:
        tok = ln.split()
        if len(tok) >= 2 and "=" not in tok[0]:
            f[tok[0]] = tok[1:]
    M = floats(f["map"], np.float32).reshape(W * H, J)
    S = floats(f["sigma"], np.float32).reshape(W * H, J)
    hits = ints(f["hits"])
    X = floats(f["rows"], np.float32).reshape(B, J)
    u = floats(f["u"], np.float64)
    L = floats(f["l"], np.float64).reshape(B, J)
    assert L[0, 0] == 0.5 and L[1, 1] == 0.0 and L[2, 2] == 1.0 and (hits == 0).any()

    # the rows against the C-ABI call on the same state, and against the restatement
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=M, sigma=S, hits=hits)
    ctx.upload_chunk(X)
    for key, rule in (("per_row", capi.GENERATE_PER_ROW), ("as_written", capi.GENERATE_AS_WRITTEN)):
        unit = ints(f["unit_" + key])
        record = floats(f["record_" + key], np.float64).reshape(B, J)
        got = ctx.generate(2, u, L, rule)
        assert (got["unit"] == unit).all() and beq(got["record"], record), key
        assert (unit < W * H).all() and (hits[unit.astype(int)] >= 2).all()
        want, zs = ref.decode(M, S, unit, L)
        ok, worst = ref.within(record, want, zs)
        print(f"{key}: worst error {worst:.3f} of its bound")
        assert ok, (key, worst)
        assert record[0, 0] == np.float64(M[int(unit[0]), 0])                       # L = 0.5
        assert record[1, 1] == -np.inf and record[2, 2] == np.inf                   # L = 0, L = 1
    assert (ints(f["unit_per_row"]) == ctx.restricted_bmd(2, u=u)["draw"]).all()
    assert len(set(f["unit_per_row"])) > 1 and f["unit_per_row"] != f["unit_as_written"]
    nodes = ints(f["decode_units"])
    dec = floats(f["decode_record"], np.float64).reshape(len(nodes), J)
    assert list(nodes) == [0, 37, 99] and beq(dec, ctx.decode_nodes(nodes, L[:3]))
    want, zs = ref.decode(M, S, nodes, L[:3])
    assert ref.within(dec, want, zs)[0]
    ctx.close()

    # autoEncoder's text
    m, s = M.astype(np.float64), S.astype(np.float64)
    ok = hits >= 2
    text = lines[lines.index("autoencoder_begin") + 1:lines.index("autoencoder_end")]
    check_text(text, X, (m - ZMAX * s)[ok].min(axis=0), (m + ZMAX * s)[ok].max(axis=0))
    text = lines[lines.index("autoencoder_nomass_begin") + 1:lines.index("autoencoder_nomass_end")]
    check_text(text, X, m[0] - ZMAX * s[0], m[0] + ZMAX * s[0])
