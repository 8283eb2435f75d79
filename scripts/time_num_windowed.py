"""What the level-windowed numerator kernel costs, and that nothing else moved: the numerator alone
(``tc_num_forward_backward`` with a derivative) and the training step (``chain_loss`` + backward, (B, C, T) float32) at C3's
shape on C3's denominator graph, for four supervisions:

    trie3     three paths a sequence: the usual one (resident kernel)
    trie40    40 paths: the largest trie that still fits the resident kernel
    trie64    64 paths: refused before the windowed kernel existed
    lattice   a lattice-like supervision (tests/wide_supervisions.py, 30-60 states a level): refused likewise

and four kinds of child process, taking turns, ``--rounds`` of each:

    parent    another checkout of this repository (``--parent-root``, built there): trie3, trie40
    alone     this checkout as it ships, on the same two (timed exactly as ``parent`` is)
    forced    this checkout with tc_debug_set("force_num_windowed", 1): trie3, trie40
    wide      this checkout as it ships: trie64, lattice

Two builds of the library cannot share a process, hence the children; the process that starts them never opens the GPU.  It
builds the supervisions once (``--cache-dir`` keeps them), prints per case, kind and quantity the median over the rounds of
each round's median and the spread (max - min) of the rounds' medians -- the spread of ``parent`` is the run-to-run noise --
and the oracle's CPU time for the numerators.  Every child also writes the numerator's log-prob and derivative and the step's
gradient for trie3 and trie40 to ``.npy`` files, which the starting process compares byte for byte: parent against alone (the
resident kernel's results did not move) and alone against forced (the two kernels give the same bits).

    python scripts/time_num_windowed.py [--parent-root DIR] [--rounds 3] [--iters 20] [--warmup 5] [--cache-dir DIR]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("trie3", "trie40", "trie64", "lattice")
FITTING = ("trie3", "trie40")
WIDE = ("trie64", "lattice")
FIELDS = ("weight", "num_sequences", "frames_per_sequence", "label_dim", "num_states", "arc_begin", "ilabel", "arc_weight",
          "nextstate", "final")


def make_supervisions(config, cache_dir):
    """The four supervisions as .npz files in cache_dir (built only where missing); host only."""
    sys.path.insert(0, os.path.join(HERE, ".."))
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    from torchain_amd import synth
    import wide_supervisions as ws
    cfg = synth.CONFIGS[config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    fst = None
    for case in CASES:
        path = os.path.join(cache_dir, "%s_%s.npz" % (config, case))
        if os.path.exists(path):
            continue
        if case == "lattice":
            sup = ws.lattice_supervision(S, T, P, lambda q, t, r: r.integers(30, 61), 2, seed=5, final_weights=True)
        else:
            fst = fst or synth.config_den_fst(config)
            sup = synth.random_supervision(fst, S, T, int(case[4:]), seed=3)
        np.savez_compressed(path, **dict(zip(FIELDS, sup)))


def load_supervision(synth, config, cache_dir, case):
    z = np.load(os.path.join(cache_dir, "%s_%s.npz" % (config, case)))
    return synth.SupFst(float(z["weight"]), int(z["num_sequences"]), int(z["frames_per_sequence"]), int(z["label_dim"]),
                        int(z["num_states"]), z["arc_begin"], z["ilabel"], z["arc_weight"], z["nextstate"], z["final"])


def child(args):
    sys.path.insert(0, args.root)
    import torch

    from torchain_amd import io, synth
    from torchain_amd._lib import check, lib
    from torchain_amd.functions import chain_loss

    if args.kind == "forced":
        check(lib.tc_debug_set(b"force_num_windowed", 1), "tc_debug_set")
    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    dev = "cuda:0"
    graph = io.DenominatorGraph(synth.config_den_fst(args.config), P).prepare(dev)
    y2d = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = 256 * ((S * 8 + 255) // 256) + 256

    def make(case):
        """(numerator alone, training step) on the case's supervision, each with tensors of its own"""
        sup = io.Supervision.from_synth(load_supervision(synth, args.config, args.cache_dir, case))
        deriv = torch.zeros_like(y2d)
        ws_ = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        lp = torch.zeros(1, dtype=torch.float64, device=dev)
        x = y2d.view(T, S, P).permute(1, 2, 0).contiguous().requires_grad_(True)

        def num():
            check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y2d.data_ptr()), S * T, P, y2d.stride(0),
                                              C.c_void_p(deriv.data_ptr()), P, C.c_void_p(lp.data_ptr()),
                                              C.c_void_p(ws_.data_ptr()), nbytes, torch.cuda.current_device(),
                                              C.c_void_p(stream)), "tc_num_forward_backward")

        def step():
            x.grad = None
            loss, _ = chain_loss(x, graph, sup, l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"])
            loss.backward()

        if case in FITTING:  # the results, for the byte-for-byte comparison
            num()
            step()
            torch.cuda.synchronize()
            for what, t in (("num_lp", lp), ("num_deriv", deriv), ("grad", x.grad)):
                np.save(os.path.join(args.out_dir, "%s_%s_%s.npy" % (args.kind, case, what)), t.detach().cpu().numpy())
        return num, step

    timed = {}
    for case in (WIDE if args.kind == "wide" else FITTING):
        timed[(case, "num")], timed[(case, "step")] = make(case)
        for fn in (timed[(case, "num")], timed[(case, "step")]):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
    times = {k: [] for k in timed}
    for _ in range(args.iters):  # (the cases and quantities take turns)
        for k, fn in timed.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    for (case, what), v in times.items():
        t = sorted(v)
        print(json.dumps(dict(config=args.config, kind=args.kind, case=case, what=what, iters=args.iters,
                              median_ms=round(t[len(t) // 2], 4), min_ms=round(t[0], 4))), flush=True)
    print(json.dumps(dict(kind=args.kind, num_windowed_launches=int(lib.tc_debug_counter(b"num_windowed_launches")))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit to compare with (kind 'parent')")
    ap.add_argument("--cache-dir", default=None, help="where the supervisions are kept (default: a temporary directory)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kind", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out-dir", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.join(HERE, ".."), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    this = os.path.abspath(args.root)
    tmp = tempfile.mkdtemp(prefix="time_num_windowed_")
    cache = os.path.abspath(args.cache_dir) if args.cache_dir else tmp
    os.makedirs(cache, exist_ok=True)
    t0 = time.time()
    make_supervisions(args.config, cache)
    print("# supervisions ready in %.1f s" % (time.time() - t0), flush=True)
    roots = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("alone", this), ("forced", this), ("wide", this)]
    rows = {}
    for rnd in range(args.rounds):
        for kind, root in roots:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--kind", kind, "--root", root, "--config", args.config,
                   "--iters", str(args.iters), "--warmup", str(args.warmup), "--cache-dir", cache, "--out-dir", tmp]
            # (a child that fails or hangs ends the run: nothing more is started on the GPU behind it)
            out = subprocess.run(cmd, check=True, timeout=args.timeout, stdout=subprocess.PIPE, text=True, cwd=root).stdout
            for line in out.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    r["round"] = rnd
                    print(json.dumps(r), flush=True)
                    if "median_ms" in r:
                        rows.setdefault((r["case"], r["what"], r["kind"]), []).append(r["median_ms"])
    print("# case quantity kind: median over %d rounds of the rounds' medians (ms), spread max - min" % args.rounds)
    for (case, what, kind), v in sorted(rows.items()):
        s = sorted(v)
        print("# %-8s %-5s %-7s %.3f  spread %.3f  %s" % (case, what, kind, s[len(s) // 2], s[-1] - s[0],
                                                         " ".join("%.3f" % x for x in v)))
    print("# results byte for byte (numerator log-prob, numerator derivative, step gradient):")
    for case in FITTING:
        for a, b in (("parent", "alone"), ("alone", "forced")):
            for what in ("num_lp", "num_deriv", "grad"):
                pa, pb = (os.path.join(tmp, "%s_%s_%s.npy" % (k, case, what)) for k in (a, b))
                if not (os.path.exists(pa) and os.path.exists(pb)):
                    continue
                same = open(pa, "rb").read() == open(pb, "rb").read()
                print("# %-7s %-9s %s == %s: %s" % (case, what, a, b, "identical" if same else "DIFFERENT"))
    try:  # the oracle's CPU time for the same numerators (single thread, as Kaldi's NumeratorComputation)
        sys.path.insert(0, this)
        from oracle import pyoracle
        from torchain_amd import synth
        cfg = synth.CONFIGS[args.config]
        y = synth.random_nnet_output(cfg["S"], cfg["T"], cfg["P"], seed=4)
        for case in CASES:
            sup = load_supervision(synth, args.config, cache, case)
            t0 = time.time()
            pyoracle.num_forward_backward(sup, y)
            print("# oracle (CPU) numerator %-8s %.1f ms" % (case, 1e3 * (time.time() - t0)))
    except Exception as e:  # (no compiler for the oracle: the GPU figures stand without it)
        print("# oracle not timed: %r" % (e,))


if __name__ == "__main__":
    main()
