#!/bin/bash
# End-to-end numbers through the reference API (Som::train via ArrayDataLoader / MnistDataLoader -> DataSet -> the C ABI),
# one JSON line per run into $1 (default gpurun_out/e2e.jsonl).  Rows: tests/gen.py mnist_like (uint8-valued MNIST-like
# pixels), 16384 x 784 for the array loader, an MNIST-sized IDX pair (60000 x 784 + labels) for the reference's loader.
#   usage: tools/e2e_bench.sh [out.jsonl] [sigma]      (sigma: only the pending-sigmaMap section at the end)
set -e
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${1:-$R/gpurun_out/e2e.jsonl}
mkdir -p "$(dirname "$OUT")"
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
python3 - "$D" "$R" <<'PY'
import struct, sys, numpy as np
d, root = sys.argv[1], sys.argv[2]
sys.path.insert(0, root + "/tests")
import gen
x = gen.mnist_like(16384, seed=3, dim=784)
x.tofile(d + "/rows.f32")
n = 60000
img = np.concatenate([gen.mnist_like(4096, seed=10 + i, dim=784) for i in range(15)])[:n].astype(np.uint8)
lab = np.random.RandomState(3).randint(0, 10, size=n).astype(np.uint8)
open(d + "/train-images-idx3-ubyte", "wb").write(struct.pack(">IIII", 0x803, n, 28, 28) + img.tobytes())
open(d + "/train-labels-idx1-ubyte", "wb").write(struct.pack(">II", 0x801, n) + lab.tobytes())
PY
T=$R/variational-self-organizing-maps_amd/host/host_api_test
: > "$OUT"
if [ "${2:-}" != sigma ]; then
for mode in strict sigma; do
    VSOM_UPDATE_MODE=$mode $T perf_e2e array "$D/rows.f32" 16384 784 4096 | grep '^{' >> "$OUT"
    VSOM_UPDATE_MODE=$mode $T perf_e2e mnist "$D" 4096 | grep '^{' >> "$OUT"
done
# the online drivers (Som::train(Exponential | InverseProportional): one trainSingle per sample, Som.cpp:1135-1187)
$T perf_e2e_online "$D/rows.f32" 16384 784 4096 | grep '^{' >> "$OUT"
fi
# Pending sigmaMap, AUTO against EAGER in real use: Som::train(BatchMap) of one epoch, a read of sigmaMap
# through the mirror, two more epochs, and the read again -- under AUTO the one that materialises (`read_ms`).  The
# state behind either read must equal the oracle's, bit for bit (8192 of the rows above, two chunks of 4096).
for mode in eager auto eager auto; do
    mkdir -p "$D/$mode"
    VSOM_SIGMA_MODE=$mode $T sigma "$D/rows.f32" 8192 784 4096 128 128 2 "$D/$mode" | grep '^{' | sed "s/^{/{\"sigma_mode\": \"$mode\", /" >> "$OUT"
done
python3 - "$D" "$R" >> "$OUT" <<'PY'
import json, sys, numpy as np
d, root = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, root + "/tests")
from oracle import pyoracle as po
from test_gpu_host_cpp import read_dump
rows = np.fromfile(d + "/rows.f32", np.float32).reshape(16384, 784)[:8192]
o = po.OracleSom(128, 128, 784, po.STANDARD)
o.random_initialize(5, 1.0)
same = lambda a, b: bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
res = {}
for name, epochs in (("sigma_a.bin", 1), ("sigma_b.bin", 2)):
    o.train_batch(rows, [0, 4096, 8192], epochs, 8.0, 0.2, nthreads=max(1, min(64, po.max_threads())))
    for mode in ("eager", "auto"):
        g = read_dump(f"{d}/{mode}/{name}")
        res[f"{mode}/{name}"] = {k: (same(g[k], r) if r.dtype.kind == "f" else bool((g[k] == r).all()))
                                 for k, r in (("map", o.map), ("sigma", o.sigma), ("weight", o.weight), ("hits", o.hits))}
ok = all(all(v.values()) for v in res.values())
print(json.dumps({"sigma_reader_equals_oracle": ok, "detail": res}))
sys.exit(0 if ok else 1)
PY
cat "$OUT"
