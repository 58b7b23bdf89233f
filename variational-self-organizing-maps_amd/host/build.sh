#!/bin/bash
# Builds the host-side C++ mirror (libsom_hip.so) and its test program against libvsom_hip.so.
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
CXX="${CXX:-g++}"
FLAGS="-std=c++20 -O2 -fPIC -Wall -Wextra -Wno-unused-parameter -I$here/include -I$here/../../include"
$CXX $FLAGS -shared "$here/src/vsom_host.cpp" "$here/src/vsom_custom.cpp" "$here/src/vsom_loaders.cpp" "$here/src/vsom_checkpoint.cpp" -o "$here/libsom_hip.so" -L"$here/.." -lvsom_hip -ldl -pthread -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_api_test.cpp" -o "$here/host_api_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_loader_test.cpp" -o "$here/host_loader_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_custom_test.cpp" -o "$here/host_custom_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_custom_device_test.cpp" -o "$here/host_custom_device_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_custom_validity_test.cpp" -o "$here/host_custom_validity_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_bmd_test.cpp" -o "$here/host_bmd_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_topk_test.cpp" -o "$here/host_topk_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_umatrix_test.cpp" -o "$here/host_umatrix_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_similarity_test.cpp" -o "$here/host_similarity_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_masked_test.cpp" -o "$here/host_masked_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_evaluate_test.cpp" -o "$here/host_evaluate_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_generate_test.cpp" -o "$here/host_generate_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_masked_train_test.cpp" -o "$here/host_masked_train_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_schedule_test.cpp" -o "$here/host_schedule_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_resident_masked_test.cpp" -o "$here/host_resident_masked_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_accum_test.cpp" -o "$here/host_accum_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_accum_masked_test.cpp" -o "$here/host_accum_masked_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_online_masked_test.cpp" -o "$here/host_online_masked_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_masked_score_test.cpp" -o "$here/host_masked_score_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_bmd_masked_test.cpp" -o "$here/host_bmd_masked_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
$CXX $FLAGS "$here/tests/host_topk_masked_test.cpp" -o "$here/host_topk_masked_test" -L"$here" -lsom_hip -L"$here/.." -lvsom_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,'$ORIGIN/..'
echo "built $here/libsom_hip.so and host_api_test"
