#!/bin/bash
# Builds libvsom_hip.so for gfx950 (cross-compiles without a GPU).
# -ffp-contract=off + correctly rounded div/sqrt: the strict kernels must reproduce the
# reference's SSE2 (non-FMA) fp32 results bit for bit.
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="${1:-$here/../libvsom_hip.so}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="-O3 --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -Wall -Wno-unused-function"
# hand-scheduled update kernel: generator -> .s -> code object -> C array included by vsom_update.hip
LLVM="${LLVM_BIN:-/opt/rocm/lib/llvm/bin}"
if [ ! -f "$here/vsom_update_hsaco.inc" ] || [ "$here/gen_update_asm.py" -nt "$here/vsom_update_hsaco.inc" ] || [ "$here/gen_nt_asm.py" -nt "$here/vsom_update_hsaco.inc" ]; then
  python3 "$here/gen_update_asm.py" "$here/vsom_update_gfx950.s"
  "$LLVM/clang" -x assembler -target amdgcn-amd-amdhsa -mcpu=gfx950 -c "$here/vsom_update_gfx950.s" -o "$here/vsom_update_gfx950.o"
  "$LLVM/ld.lld" -shared "$here/vsom_update_gfx950.o" -o "$here/vsom_update_gfx950.hsaco"
  python3 - "$here/vsom_update_gfx950.hsaco" "$here/vsom_update_hsaco.inc" <<'PY'
import sys
b = open(sys.argv[1], "rb").read()
open(sys.argv[2], "w").write(",".join(str(x) for x in b) + "\n")
PY
  rm -f "$here/vsom_update.o"
fi
objs=()
for f in vsom_capi vsom_bmu vsom_shortlist vsom_update vsom_online vsom_online_i8 vsom_online_tiny vsom_online_masked vsom_single vsom_tiny vsom_tiny_masked vsom_group vsom_compact vsom_xq vsom_sl_i8 vsom_custom vsom_ensemble vsom_bmd vsom_topk vsom_umatrix vsom_similarity vsom_masked vsom_masked_train vsom_accum vsom_accum_masked vsom_evaluate vsom_generate; do
  o="$here/$f.o"
  stale=0
  for d in "$here/$f.hip" "$here"/*.hpp "$here"/*.inc "$here/../../include/vsom_hip.h"; do   # any header may reach any object
    if [ ! -f "$o" ] || [ "$d" -nt "$o" ]; then stale=1; fi
  done
  if [ $stale = 1 ]; then
    $HIPCC $FLAGS -c "$here/$f.hip" -o "$o" &
  fi
  objs+=("$o")
done
wait
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$out" "${objs[@]}" -lhiprtc -ldl
echo "built $out"
