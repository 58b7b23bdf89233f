#!/bin/bash
# Device code of two source trees, kernel by kernel: bash tools/kernel_diff.sh TREE_A TREE_B
# Every csrc/*.hip of each tree is compiled device-only for gfx950 with the flags of that tree's csrc/build.sh and
# disassembled; the instruction streams (mnemonics, operands and encodings, without addresses) are compared per demangled
# function name.  Prints the kernels that differ or exist in one tree only, the files whose whole device objects are
# byte-identical (descriptors and metadata included), and the counts.  Needs hipcc and llvm-objdump, no GPU, no built library.
set -euo pipefail
[ $# = 2 ] || { echo "usage: $0 TREE_A TREE_B" >&2; exit 2; }
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
LLVM="${LLVM_BIN:-/opt/rocm/lib/llvm/bin}"
work="$(mktemp -d)"
trap 'rm -rf "$work"' EXIT
# vsom_update.hip includes a generated host array (the assembled update kernel); a tree that has not been built gets a stub
mkdir "$work/stub" && echo 0 > "$work/stub/vsom_update_hsaco.inc"
side=a
for tree in "$1" "$2"; do
  csrc="$tree/variational-self-organizing-maps_amd/csrc"
  flags="$(sed -n 's/^FLAGS="\(.*\)"$/\1/p' "$csrc/build.sh")"
  mkdir "$work/$side"
  # -fuse-cuid=none: no symbol derived from the source path, so equal code gives equal objects
  ls "$csrc"/*.hip | xargs -P "${JOBS:-8}" -I{} sh -c \
    "$HIPCC $flags -I$work/stub -fuse-cuid=none --cuda-device-only --no-gpu-bundle-output -c {} -o $work/$side/\$(basename {} .hip).o"
  for o in "$work/$side"/*.o; do
    # "<address> <name>:" opens a function; "\tinsn // address: encoding" is one instruction; "\t\t..." is the zero padding up
    # to the next function's alignment, which only a function that is not the last of its object has: no instruction
    "$LLVM/llvm-objdump" -d -C "$o" | awk '/^[0-9a-f]+ <.*>:$/ { sub(/^[0-9a-f]+ </, ""); sub(/>:$/, ""); k = $0; next }
      /^\t+\.\.\.$/ { next }
      /^\t/ && k != "" { sub(/\/\/ [0-9A-F]+:/, "//"); print k "\t" $0 }'
  done > "$work/$side.txt"
  side=b
done
for o in "$work"/a/*.o; do
  f="$(basename "$o")"
  if [ -f "$work/b/$f" ] && cmp -s "$o" "$work/b/$f"; then same+=" ${f%.o}"; fi
done
echo "device objects byte-identical:${same:- none}"
awk -F'\t' 'FNR == NR { a[$1] = a[$1] "\n" $2; na[$1]++; next } { b[$1] = b[$1] "\n" $2; nb[$1]++ }
  END { for (k in a) if (!(k in b)) { oa++; print "only in A: " k } else { n++; if (a[k] != b[k]) { d++; print "differs (" na[k] " -> " nb[k] " instructions): " k } }
        for (k in b) if (!(k in a)) { ob++; print "only in B: " k }
        printf "kernels compared %d, differing %d, only in A %d, only in B %d\n", n, d, oa, ob }' "$work/a.txt" "$work/b.txt"
