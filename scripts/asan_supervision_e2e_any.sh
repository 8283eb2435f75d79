#!/bin/bash
# Development aid (CPU): tc_supervision_create_e2e_any and tc_supervision_e2e_stats (csrc/supervision_e2e.cpp) under
# AddressSanitizer and UBSan, as a stand-alone program: sequences at the resident kernel's limits, one past each, at the new LDS
# rule and one past it, malformed FSTs beside them, and 3000 corrupted copies of a small valid batch.
set -e
set -o pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d); cd $tmp
# (host code only: chain_internal.h names device builtins, so the files go through hipcc's host pass, sanitized there alone)
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
for src in $root/scripts/asan_supervision_e2e_any.cpp $root/torchain_amd/csrc/supervision.cpp $root/torchain_amd/csrc/supervision_e2e.cpp; do
  $hipcc -std=c++17 -g -O1 -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -I$root/include \
      -I$root/torchain_amd/csrc -c $src -o $(basename $src).o
done
clang=$(dirname $($hipcc --version | sed -n 's/^InstalledDir: //p'))/bin/clang++
$clang -fsanitize=address,undefined *.o -L/opt/rocm/lib -lamdhip64 -Wl,--unresolved-symbols=ignore-all -o e2e_any
LD_LIBRARY_PATH=/opt/rocm/lib ASAN_OPTIONS=detect_leaks=0 ./e2e_any 2>&1 | tail -80
