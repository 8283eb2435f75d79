"""Device time of the end-to-end numerator and of the whole training step on the resident kernel (num_e2e_kernels.hip), on
the same batch forced onto the large kernel (num_e2e_large_kernels.hip, tc_debug_set("force_num_e2e_large", 1)), and on a
batch only the large kernel takes (development aid; results: profiles/e2e_large/README.md).

    python scripts/time_e2e_large.py [--config C3] [--sequences 256] [--rounds 7] [--steps 40] [--root CHECKOUT]

Rows: ``numerator`` is tc_num_forward_backward alone (forward, backward, posteriors added into a derivative matrix),
``step`` is chain_loss + backward.  The variants are timed in alternation, ``--rounds`` windows of ``--steps`` calls each
between two device events after a warm-up of every variant; a row is the median window with the lowest and the highest one.
``--root``: the checkout whose torchain_amd is imported -- a build of the parent commit gives the parent's resident rows with the
same script (it has neither the switch nor the any-size entry: the other rows are left out there).

The chain batch is time_e2e.py's (Kaldi-chain-like FSTs of tests/e2e_reference.py, about one phone per 4 frames).  The
large-only batch: every sequence a random acceptor with cycles of 3000 states, 9000 arcs and 256 distinct pdfs (four
different ones, repeated)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--sequences", type=int, default=0)
ap.add_argument("--large-sequences", type=int, default=64)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))  # (e2e_reference: the FSTs)
sys.path.insert(0, os.path.abspath(args.root))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import e2e_reference as ref  # noqa: E402
from torchain_amd import io, synth  # noqa: E402
from torchain_amd._lib import check, lib  # noqa: E402
from torchain_amd.functions import chain_loss  # noqa: E402

cfg = synth.CONFIGS[args.config]
S = args.sequences or cfg["S"]
T, P = cfg["T"], cfg["P"]
dev = torch.device("cuda", 0)
graph = io.DenominatorGraph(synth.config_den_fst(args.config), P).prepare(0)
has_large = lib.tc_debug_set(b"force_num_e2e_large", 0) == 0


def sizes(fsts):
    return "states %d..%d, arcs %d..%d, distinct pdfs %d..%d" % tuple(
        f(v) for v in ([len(x[5]) for x in fsts], [int(x[1][-1]) for x in fsts], [len(set(x[2].tolist())) for x in fsts])
        for f in (min, max))


def num_call(sup, S_):
    y = torch.randn(S_ * T, P, device=dev)
    deriv = torch.zeros(S_ * T, P, device=dev)
    nbytes = 256 * ((S_ * 8 + 255) // 256) + 256
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lp = torch.zeros(1, dtype=torch.float64, device=dev)

    def call():
        check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y.data_ptr()), S_ * T, P, P, C.c_void_p(deriv.data_ptr()), P,
                                          C.c_void_p(lp.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, 0,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tc_num_forward_backward")
    return call


def step_call(sup, S_):
    x = torch.randn(S_ * T, P, device=dev).requires_grad_(True)

    def call():
        loss, _ = chain_loss(x, graph, sup, l2_regularize=cfg.get("l2", 0.0), leaky_hmm_coefficient=cfg["leaky"])
        torch.autograd.grad(loss, x)
    return call


def window(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / args.steps


def force(on):
    if has_large:
        check(lib.tc_debug_set(b"force_num_e2e_large", int(on)), "tc_debug_set")


rng = np.random.default_rng(7)
chain = [ref.chain_fst(P, rng, words=max(1, T // 15), max_phones=4) for _ in range(S)]
print("%s [%s] S=%d T=%d P=%d; chain batch: %s" % (args.config, args.label, S, T, P, sizes(chain)), flush=True)
variants = {}  # name -> (forced, {row: call})
resident = io.Supervision.from_e2e_fsts(1.0, T, P, chain)
variants["chain, resident"] = (False, dict(numerator=num_call(resident, S), step=step_call(resident, S)))
if has_large:
    force(True)  # (the handle's pool slot gets the arc occupations when it first reaches the device: warm it under the switch)
    forced = io.Supervision.from_e2e_fsts(1.0, T, P, chain, any_size=True)
    variants["chain, forced large"] = (True, dict(numerator=num_call(forced, S), step=step_call(forced, S)))
    for c in variants["chain, forced large"][1].values():
        c()
    force(False)
    SL = args.large_sequences
    four = [ref.distinct_pdfs_fst(3000, 9000, P, 256, rng) for _ in range(4)]
    big = [four[i % 4] for i in range(SL)]
    print("%s [%s] large-only batch S=%d: %s" % (args.config, args.label, SL, sizes(big)), flush=True)
    large = io.Supervision.from_e2e_fsts(1.0, T, P, big, any_size=True)
    assert large.e2e_stats()["kernel"] == "large"
    variants["large only, S=%d" % SL] = (False, dict(numerator=num_call(large, SL), step=step_call(large, SL)))

counter = lambda: int(lib.tc_debug_counter(b"num_e2e_large_launches"))  # noqa: E731
times = {(v, r): [] for v, (_, rows) in variants.items() for r in rows}
for rnd in range(-1, args.rounds):  # (round -1: warm-up of every variant)
    for v, (forced_on, rows) in variants.items():
        force(forced_on)
        for r, call in rows.items():
            before = counter()
            t = window(call)
            moved = counter() - before
            assert (moved > 0) == (v != "chain, resident"), (v, r, moved)
            if rnd >= 0:
                times[(v, r)].append(t)
        force(False)
for (v, r), ts in times.items():
    print("%s [%s] %-22s %-9s median %.3f ms  (min %.3f, max %.3f; %d windows of %d calls)" % (
        args.config, args.label, v, r, statistics.median(ts), min(ts), max(ts), len(ts), args.steps), flush=True)
print(json.dumps({"label": args.label, "config": args.config, "S": S, "T": T,
                  "ms": {"%s / %s" % k: statistics.median(v) for k, v in times.items()}}), flush=True)
