#!/bin/bash
# Development aid (CPU): tc_den_compose (csrc/den_compose.cpp) under AddressSanitizer and UBSan, as a stand-alone program:
# over 2 x 4000 corrupted copies of a valid batch in the regular and the end-to-end form (offsets, labels, next states,
# costs, final costs, starts, sequence boundaries, label_dim, scale and max_states off by a few); every accepted output goes
# through tc_supervision_create_ragged / tc_supervision_create_e2e.  The graph handle is built by tc_den_graph_create.
set -e -o pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d); cd $tmp
# (host code only: chain_internal.h names device builtins, so the files go through hipcc's host pass, sanitized there alone)
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
csrc=$root/torchain_amd/csrc
for src in $root/scripts/asan_den_compose.cpp $csrc/den_compose.cpp $csrc/den_graph.cpp $csrc/den_layout.cpp $csrc/schedule_general.cpp \
    $csrc/schedule_owner.cpp $csrc/supervision.cpp $csrc/supervision_e2e.cpp; do
  $hipcc -std=c++17 -g -O1 -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -I$root/include \
      -I$csrc -c $src -o $(basename $src).o
done
clang=$(dirname $($hipcc --version | sed -n 's/^InstalledDir: //p'))/bin/clang++
$clang -fsanitize=address,undefined *.o -L/opt/rocm/lib -lamdhip64 -Wl,--unresolved-symbols=ignore-all -o fuzz_compose
python3 - <<PY
import struct, sys
sys.path.insert(0, "$root")
import numpy as np
from torchain_amd import synth
fst = synth.random_den_fst(40, 4, 24, seed=1)
lens = (8, 1, 5)
# supervisions without the graph's weights: the paths of synth.random_supervision at cost 0, plus one label the graph may not allow
pieces = [synth.random_supervision(fst, 1, t, 3, seed=5 + i, final_weights=True) for i, t in enumerate(lens)]
sb = np.concatenate([[0], np.cumsum([p.num_states for p in pieces])])
arcs = np.concatenate([[0], np.cumsum([len(p.ilabel) for p in pieces])])
ab = np.concatenate([[0]] + [np.asarray(p.arc_begin[1:]) + arcs[i] for i, p in enumerate(pieces)])
cat = lambda k: np.concatenate([np.asarray(getattr(p, k)) for p in pieces])
with open("$tmp/compose.bin", "wb") as f:
    f.write(struct.pack("<6i", fst.num_states, len(fst.src), fst.num_pdfs, len(lens), int(sb[-1]), int(arcs[-1])))
    for a, dt in ((fst.src, np.int32), (fst.dst, np.int32), (fst.ilabel, np.int32), (fst.weight, np.float32), (fst.final, np.float32),
                  (lens, np.int32), (sb, np.int32), (ab, np.int32), (cat("ilabel"), np.int32), (cat("nextstate"), np.int32),
                  (np.zeros(int(arcs[-1])), np.float32), (cat("final"), np.float32)):
        f.write(np.ascontiguousarray(a, dt).tobytes())
PY
LD_LIBRARY_PATH=/opt/rocm/lib ASAN_OPTIONS=detect_leaks=0 ./fuzz_compose $tmp/compose.bin 2>&1 | tail -5
