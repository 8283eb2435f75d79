"""Wall and device time of chain_loss forward + backward with end-to-end supervisions (num_e2e_kernels.hip) beside the
same batch with a regular supervision, on a BASELINE config's den graph (development aid).

    python scripts/time_e2e.py [C3] [S]

The e2e FSTs are the Kaldi-chain-like left-to-right graphs of tests/e2e_reference.py (words of 1-4 phones, one
forward and one self-loop pdf per phone, optional silence); their sizes are printed."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import e2e_reference as ref  # noqa: E402
from torchain_amd import io, synth  # noqa: E402
from torchain_amd.functions import chain_loss  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "C3"
cfg = synth.CONFIGS[name]
S = int(sys.argv[2]) if len(sys.argv) > 2 else cfg["S"]
T, P = cfg["T"], cfg["P"]
fst = synth.config_den_fst(name)
dev = torch.device("cuda", 0)
graph = io.DenominatorGraph(fst, P).prepare(0)
rng = np.random.default_rng(7)
words = max(1, T // 15)  # about one phone per 4 frames of 30 ms
fsts = [ref.chain_fst(P, rng, words=words, max_phones=4) for _ in range(S)]
states = [len(f[5]) for f in fsts]
arcs = [int(f[1][-1]) for f in fsts]
pdfs = [len(set(f[2])) for f in fsts]
sups = dict(e2e=io.Supervision.from_e2e_fsts(1.0, T, P, fsts),
            regular=io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=7,
                                                                       initial_probs=graph.initial_probs())))
x = torch.randn(S * T, P, device=dev).requires_grad_(True)
print("%s S=%d T=%d P=%d; e2e FSTs per sequence: states %d..%d (mean %.1f), arcs %d..%d (mean %.1f), pdfs %d..%d" % (
    name, S, T, P, min(states), max(states), np.mean(states), min(arcs), max(arcs), np.mean(arcs), min(pdfs), max(pdfs)))
for kind, sup in sups.items():
    def step():
        loss, res = chain_loss(x, graph, sup, l2_regularize=cfg.get("l2", 0.0), leaky_hmm_coefficient=cfg["leaky"])
        torch.autograd.grad(loss, x)
        return res

    for _ in range(10):
        step()
    torch.cuda.synchronize()
    n = 50
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / n * 1e3
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    e1.synchronize()
    print("%s S=%d %-7s: chain_loss + backward  wall %.3f ms/step, device (events) %.3f ms/step" % (
        name, S, kind, wall, e0.elapsed_time(e1) / n), flush=True)
