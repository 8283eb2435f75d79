#!/bin/bash
# Development aid (CPU): tc_supervision_create_ragged and the per-sequence table builder it shares with tc_supervision_create
# (csrc/supervision.cpp) under AddressSanitizer and UBSan, as a stand-alone program: over 4000 corrupted copies of a valid ragged
# batch (offsets, labels, next states, weights, final weights, lengths, sequence boundaries and label_dim off by a few).
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d); cd $tmp
# (host code only: chain_internal.h names device builtins, so the files go through hipcc's host pass, sanitized there alone)
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
for src in $root/scripts/asan_supervision_ragged.cpp $root/torchain_amd/csrc/supervision.cpp $root/torchain_amd/csrc/supervision_e2e.cpp; do
  $hipcc -std=c++17 -g -O1 -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -I$root/include \
      -I$root/torchain_amd/csrc -c $src -o $(basename $src).o
done
clang=$(dirname $($hipcc --version | sed -n 's/^InstalledDir: //p'))/bin/clang++
$clang -fsanitize=address,undefined *.o -L/opt/rocm/lib -lamdhip64 -Wl,--unresolved-symbols=ignore-all -o fuzz_ragged
python3 - <<PY
import struct, sys
sys.path.insert(0, "$root")
import numpy as np
from torchain_amd import synth
fst = synth.random_den_fst(40, 4, 24, seed=1)
lens = (8, 1, 5)
pieces = [synth.random_supervision(fst, 1, t, 3, seed=5 + i, final_weights=True) for i, t in enumerate(lens)]
sb = np.concatenate([[0], np.cumsum([p.num_states for p in pieces])])
arcs = np.concatenate([[0], np.cumsum([len(p.ilabel) for p in pieces])])
ab = np.concatenate([[0]] + [np.asarray(p.arc_begin[1:]) + arcs[i] for i, p in enumerate(pieces)])
cat = lambda k: np.concatenate([np.asarray(getattr(p, k)) for p in pieces])
with open("$tmp/ragged.bin", "wb") as f:
    f.write(struct.pack("<4if", len(lens), pieces[0].label_dim, int(sb[-1]), int(arcs[-1]), pieces[0].weight))
    for a, dt in ((lens, np.int32), (sb, np.int32), (ab, np.int32), (cat("ilabel"), np.int32), (cat("nextstate"), np.int32),
                  (cat("arc_weight"), np.float32), (cat("final"), np.float32)):
        f.write(np.ascontiguousarray(a, dt).tobytes())
PY
LD_LIBRARY_PATH=/opt/rocm/lib ASAN_OPTIONS=detect_leaks=0 ./fuzz_ragged $tmp/ragged.bin 2>&1 | tail -5
