"""What ragged REGULAR supervisions (io.Supervision.from_sequences) cost and buy at C3's shape: 256 sequences, up to 150
frames, 4096 pdfs, tries of 3 and of 40 paths a sequence.

Two kinds of child process take turns, ``--rounds`` of each: ``parent`` (another checkout of this repository, ``--parent-root``,
built there) and ``this``, by the method of scripts/time_num_windowed.py and scripts/time_ragged.py.  Two builds of the library
cannot share a process, hence the children; the process that starts them never opens the GPU.  Every case is ``--warmup``
untimed and ``--iters`` event-timed calls; the report gives per case and kind the median over the rounds of each round's
median and the spread (max - min) of the rounds' medians -- the spread of a kind is its run-to-run noise, and the parent's
spread is the bound on "this is not slower".

    num_uniform_<paths>    tc_num_forward_backward on the uniform 256 x 150 supervision (both kinds; SHA-1 of the derivative)
    step_uniform_<paths>   chain_loss + backward on it, (B, C, T) float32 (both kinds; SHA-1 of the gradient)
    num_ragged_<paths>     tc_num_forward_backward on ONE ragged handle: 256 sequences of lengths drawn uniformly from 50 .. 150
                           at a fixed seed, each a trie of <paths> paths of its own length (this)
    step_ragged_<paths>    chain_loss + backward on it, the tensors (256, C, 150) (this)

    python scripts/time_ragged_regular.py [--parent-root DIR] [--rounds 3] [--iters 20] [--warmup 5] [--cases num_ragged_40,...]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATHS = (3, 40)
LENGTH_SEED, LENGTH_LO, LENGTH_HI = 17, 50, 150


def ragged_lengths(S):
    return np.random.default_rng(LENGTH_SEED).integers(LENGTH_LO, LENGTH_HI + 1, size=S).tolist()


def child(args):
    sys.path.insert(0, args.root)
    import torch

    from torchain_amd import io, synth
    from torchain_amd._lib import check, lib
    from torchain_amd.functions import chain_loss

    dev = "cuda:0"
    this = args.kind == "this"
    wanted = set(args.cases.split(",")) if args.cases else None

    def timed(name, make, digest=None):
        if wanted is not None and name not in wanted:
            return
        step, out = make()
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        times.sort()
        row = dict(kind=args.kind, case=name, iters=args.iters, median_ms=round(times[len(times) // 2], 4), min_ms=round(times[0], 4))
        if args.hash:
            row["sha1"] = hashlib.sha1(out().contiguous().view(torch.int32).cpu().numpy().tobytes()).hexdigest()
        print(json.dumps(row), flush=True)

    cfg = synth.CONFIGS["C3"]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    fst = synth.config_den_fst("C3")
    graph = io.DenominatorGraph(fst, P).prepare(dev)
    gen = torch.Generator(device=dev).manual_seed(4)
    y = torch.randn(S * T, P, device=dev, generator=gen)
    x = y.view(T, S, P).permute(1, 2, 0).contiguous().requires_grad_(True)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kw = dict(l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"])
    pi = synth.initial_probs_f64(fst)

    def num_call(sup):
        def make():
            deriv = torch.zeros_like(y)
            nbytes = 256 * ((S * 8 + 255) // 256) + 256
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            lp = torch.zeros(1, dtype=torch.float64, device=dev)

            def step():
                deriv.zero_()  # (the call adds to the matrix; the memset is in every case's time)
                check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y.data_ptr()), S * T, P, P, C.c_void_p(deriv.data_ptr()), P,
                                                  C.c_void_p(lp.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, 0, stream), "num")
            return step, lambda: deriv
        return make

    def step_call(sup):
        def make():
            def step():
                x.grad = None
                loss, _ = chain_loss(x, graph, sup, **kw)
                loss.backward()
            return step, lambda: x.grad
        return make

    for paths in PATHS:
        uniform = io.Supervision.from_synth(synth.random_supervision(fst, S, T, paths, seed=3, initial_probs=pi))
        timed("num_uniform_%d" % paths, num_call(uniform))
        timed("step_uniform_%d" % paths, step_call(uniform))
        if not this:
            continue
        lens = ragged_lengths(S)
        ragged = io.Supervision.from_sequences(
            [synth.random_supervision(fst, 1, t, paths, seed=1000 + s, initial_probs=pi) for s, t in enumerate(lens)])
        timed("num_ragged_%d" % paths, num_call(ragged))
        timed("step_ragged_%d" % paths, step_call(ragged))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit to compare with (kind 'parent')")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--cases", default="", help="comma-separated case names; default: all")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kind", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--hash", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.join(HERE, ".."), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    roots = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", os.path.abspath(args.root))]
    rows, hashes = {}, {}
    for rnd in range(args.rounds):
        for kind, root in roots:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--kind", kind, "--root", root, "--iters", str(args.iters),
                   "--warmup", str(args.warmup), "--cases", args.cases] + (["--hash"] if rnd == 0 else [])
            # (a child that fails or hangs ends the run: nothing more is started on the GPU behind it)
            out = subprocess.run(cmd, check=True, timeout=args.timeout, stdout=subprocess.PIPE, text=True, cwd=root).stdout
            for line in out.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    r["round"] = rnd
                    print(json.dumps(r), flush=True)
                    rows.setdefault((r["case"], kind), []).append(r["median_ms"])
                    if "sha1" in r:
                        hashes[(r["case"], kind)] = r["sha1"]
    print("# lengths of the ragged cases: %d sequences, %d .. %d frames, %d in all (the uniform batch: %d)" % (
        256, min(ragged_lengths(256)), max(ragged_lengths(256)), sum(ragged_lengths(256)), 256 * 150))
    print("# case kind: median over %d rounds of the rounds' medians (ms), spread max - min, the rounds" % args.rounds)
    for key, v in sorted(rows.items()):
        s = sorted(v)
        print("# %-18s %-6s %.3f  spread %.3f  %s" % (key[0], key[1], s[len(s) // 2], s[-1] - s[0], " ".join("%.3f" % x for x in v)))
    print("# SHA-1 of the outputs (derivative of the numerator call, gradient of the step):")
    for (case, kind), h in sorted(hashes.items()):
        if kind == "this" and (case, "parent") in hashes:
            print("# %-18s this == parent: %s" % (case, "identical" if h == hashes[(case, "parent")] else "DIFFERENT"))
    for (case, kind), v in sorted(rows.items()):
        if kind == "this" and (case, "parent") in rows:
            p = sorted(rows[(case, "parent")])
            t = sorted(v)
            bound = p[len(p) // 2] + (p[-1] - p[0])
            print("# %-18s this %.3f against the parent's %.3f + its spread %.3f = %.3f: %s" % (
                case, t[len(t) // 2], p[len(p) // 2], p[-1] - p[0], bound, "within" if t[len(t) // 2] <= bound else "ABOVE"))


if __name__ == "__main__":
    main()
