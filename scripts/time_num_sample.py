"""What drawing alignments from a supervision's path posterior costs (``tc_supervision_sample_paths``), in both forms of its
traceback, beside ``tc_supervision_best_path`` and the numerator's forward-backward (``tc_num_forward_backward`` with a
derivative) on the same handle from the same run, at a config's shape (C3: 256 x 150, 4096 pdfs), for four supervisions:

    trie3     three paths a sequence: the usual regular supervision
    trie40    40 paths: the largest trie that still fits the resident numerator kernel
    lattice   lattice-like, 30-60 states a level (``tests/wide_supervisions.py: lattice_supervision``)
    e2e       the end-to-end ``chain`` batch of scripts/time_best_path.py (words of 1-4 phones, about one phone per 4 frames)

All calls take the 2-D float32 output.  Per case and ``K`` in ``--samples`` the calls take turns -- staged, streamed
(``tc_debug_set("force_num_sample_streamed", 1)``), best path, numerator -- ``--iters`` timed calls of each after ``--warmup``,
device events around every call, the uniforms and the workspace made outside the timed region; one JSON line a (case, K) with
the medians and the minima.  The two forms' outputs are compared here as well (they are equal, bit for bit).  Last, one
``sampled_risk_surrogate(..., fused=True)`` forward and backward on the e2e case's numerator samples, a risk of the number of
frames on pdf 0.

    python scripts/time_num_sample.py [--config C3] [--iters 20] [--warmup 5] [--samples 1,8,32]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--samples", default="1,8,32")
    args = ap.parse_args()

    import torch

    import e2e_reference as ref
    import wide_supervisions as ws
    from torchain_amd import io, synth
    from torchain_amd._lib import check, lib
    from torchain_amd.functions import sampled_risk_surrogate

    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    dev = "cuda:0"
    t0 = time.time()
    fst = synth.config_den_fst(args.config)
    rng = np.random.default_rng(0)
    sups = {
        "trie3": io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=3)),
        "trie40": io.Supervision.from_synth(synth.random_supervision(fst, S, T, 40, seed=3)),
        "lattice": io.Supervision.from_sequences([ws.lattice_supervision(1, T, P, lambda q, t, r: r.integers(30, 61), 2, seed=5 + s,
                                                                         final_weights=True) for s in range(S)]),
        "e2e": io.Supervision.from_e2e_fsts(1.0, T, P, [ref.chain_fst(P, rng, words=max(1, T // 15), max_phones=4)
                                                        for _ in range(S)]),
    }
    print("# supervisions ready in %.1f s" % (time.time() - t0), flush=True)
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = 256 * ((S * 8 + 255) // 256) + 256
    deriv = torch.zeros_like(y)
    num_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lp = torch.zeros(1, dtype=torch.float64, device=dev)

    def numerator(sup):
        check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y.data_ptr()), S * T, P, y.stride(0), C.c_void_p(deriv.data_ptr()), P,
                                          C.c_void_p(lp.data_ptr()), C.c_void_p(num_ws.data_ptr()), nbytes, torch.cuda.current_device(),
                                          C.c_void_p(stream)), "tc_num_forward_backward")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    last = None
    for case, sup in sups.items():
        buf = torch.empty(int(lib.tc_supervision_sample_paths_workspace_bytes(sup.ptr)), dtype=torch.uint8, device=dev)
        keep = lambda device, cur, need: buf  # noqa: E731  (no allocation in the timed region)
        for K in [int(k) for k in args.samples.split(",")]:
            u = torch.rand((S, K, T + 1), generator=torch.Generator(dev).manual_seed(7), device=dev)

            def sample(streamed):
                check(lib.tc_debug_set(b"force_num_sample_streamed", int(streamed)), "tc_debug_set")
                try:
                    return sup.sample_paths(y, K, uniforms=u, workspace=keep)
                finally:
                    check(lib.tc_debug_set(b"force_num_sample_streamed", 0), "tc_debug_set")

            for _ in range(args.warmup):
                numerator(sup)
                sup.best_path(y)
                a, b = sample(False), sample(True)
            torch.cuda.synchronize()
            assert sup.sample_paths_kernel() == 0 and bool((a.pdfs >= 0).all()) and bool(torch.isfinite(a.scores).all()), case
            assert torch.equal(a.pdfs, b.pdfs) and torch.equal(a.scores, b.scores) and torch.equal(a.logprob, b.logprob), case
            times = {"staged": [], "streamed": [], "best_path": [], "numerator": []}
            for _ in range(args.iters):  # (the four take turns)
                times["staged"].append(timed(lambda: sample(False)))
                times["streamed"].append(timed(lambda: sample(True)))
                times["best_path"].append(timed(lambda: sup.best_path(y)))
                times["numerator"].append(timed(lambda: numerator(sup)))
            row = dict(config=args.config, case=case, K=K, iters=args.iters)
            for k, v in times.items():
                row[k + "_median_ms"], row[k + "_min_ms"] = round(sorted(v)[len(v) // 2], 4), round(min(v), 4)
            print(json.dumps(row), flush=True)
            last = a
    # the fused risk surrogate on numerator samples: the e2e case's last draw, risk = frames on pdf 0
    risks = (last.pdfs == 0).sum(-1).double()
    x = y.clone().requires_grad_(True)

    def surrogate():
        x.grad = None
        sampled_risk_surrogate(x, last.pdfs, risks, fused=True).sum().backward()

    for _ in range(args.warmup):
        surrogate()
    torch.cuda.synchronize()
    v = sorted(timed(surrogate) for _ in range(args.iters))
    print(json.dumps(dict(config=args.config, case="e2e", K=int(last.pdfs.shape[1]), sampled_risk_surrogate_fused_median_ms=round(v[len(v) // 2], 4),
                          sampled_risk_surrogate_fused_min_ms=round(v[0], 4))), flush=True)
    print(json.dumps({k.decode(): int(lib.tc_debug_counter(k)) for k in (b"num_sample_launches", b"num_sample_streamed_launches")}), flush=True)


if __name__ == "__main__":
    main()
