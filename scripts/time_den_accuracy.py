"""What the expected frame accuracy over the denominator graph costs (``tc_den_expected_accuracy``: the denominator
forward-backward and the row kernel) and what its gradient costs (``tc_den_expected_accuracy_grad``: the accuracy-carrying
forward-backward), beside the denominator forward-backward (``tc_den_forward_backward`` with a derivative) on the same graph
and the same outputs, in the same run:

    C3      256 x 150 frames, 4096 pdfs, 8192 states / 65536 arcs
    R4      the phone-LM-structured graph of config R4 (2928 pdfs), 64 sequences of 150 frames

All three take the 2-D float32 output and preallocated buffers; the reference is the graph's own best path
(``io.DenominatorGraph.best_path``), state-level classes.  The three take turns, ``--iters`` timed calls of each after
``--warmup``; device events around every call; per case one JSON line with the medians, the minima, the quartiles and the
ratios to the denominator.  The values' checks are tests/test_gpu_den_accuracy.py's; here only that every sequence got a
finite accuracy in ``0 .. T`` and a finite gradient.

    python scripts/time_den_accuracy.py [--iters 10] [--warmup 2]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="C3:256,R4:64")
    args = ap.parse_args()

    import torch

    from torchain_amd import io, synth
    from torchain_amd._lib import check, lib

    dev = "cuda:0"
    for item in args.configs.split(","):
        config, S = item.split(":")[0], int(item.split(":")[1])
        cfg = synth.CONFIGS[config]
        T, P = cfg["T"], cfg["P"]
        t0 = time.time()
        fst = synth.config_den_fst(config)
        graph = io.DenominatorGraph(fst, P).prepare(dev)
        print("# %s: %d states, %d arcs, ready in %.1f s" % (config, graph.num_states, graph.num_arcs, time.time() - t0), flush=True)
        y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
        ref = graph.best_path(y, n_batch=S)[0]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        den_bytes = int(lib.tc_chain_workspace_bytes(graph.ptr, S, T))
        grad_bytes = int(lib.tc_den_expected_accuracy_grad_workspace_bytes(graph.ptr, S, T))
        ws = torch.empty(max(den_bytes, grad_bytes), dtype=torch.uint8, device=dev)
        gamma, grad = torch.empty((S * T, P), device=dev), torch.empty((S * T, P), device=dev)
        fa, acc = torch.empty((S, T), device=dev), torch.empty((S,), dtype=torch.float64, device=dev)
        lp, status = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        device = torch.cuda.current_device()

        def den():
            check(lib.tc_den_forward_backward(graph.ptr, S, p(y), S * T, P, P, cfg["leaky"], 1.0, 0.0, 0, p(gamma), P, p(lp),
                                              p(status), p(ws), ws.numel(), device, stream), "tc_den_forward_backward")

        def accuracy():
            check(lib.tc_den_expected_accuracy(graph.ptr, S, p(y), S * T, P, P, None, T, cfg["leaky"], p(ref), None, p(gamma), P,
                                               p(fa), p(acc), p(ws), ws.numel(), device, stream), "tc_den_expected_accuracy")

        def gradient():
            check(lib.tc_den_expected_accuracy_grad(graph.ptr, S, p(y), S * T, P, P, None, T, cfg["leaky"], p(ref), None, p(fa),
                                                    None, p(grad), P, p(ws), ws.numel(), device, stream),
                  "tc_den_expected_accuracy_grad")

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        streamed = int(lib.tc_debug_counter(b"den_accuracy_grad_streamed_launches"))
        for _ in range(args.warmup):
            den()
            accuracy()
            gradient()
        torch.cuda.synchronize()
        streamed = int(lib.tc_debug_counter(b"den_accuracy_grad_streamed_launches")) > streamed
        assert int(status.item()) == 0 and bool(torch.isfinite(grad).all()), config
        assert bool((acc >= 0).all()) and bool((acc <= T).all()), config
        times = {"den": [], "accuracy": [], "gradient": []}
        for _ in range(args.iters):  # (the three take turns)
            times["den"].append(timed(den))
            times["accuracy"].append(timed(accuracy))
            times["gradient"].append(timed(gradient))
        row = dict(config=config, S=S, T=T, pdfs=P, states=graph.num_states, arcs=graph.num_arcs, iters=args.iters,
                   den_workspace_bytes=den_bytes, grad_workspace_bytes=grad_bytes, grad_vectors_in_workspace=bool(streamed),
                   mean_accuracy=round(float(acc.mean()), 3), largest_gradient=float(grad.abs().max()))
        for k, v in times.items():
            v = sorted(v)
            row.update({k + "_median_ms": round(v[len(v) // 2], 4), k + "_min_ms": round(v[0], 4),
                        k + "_q1_ms": round(v[len(v) // 4], 4), k + "_q3_ms": round(v[(3 * len(v)) // 4], 4)})
        row["accuracy_ratio"] = round(row["accuracy_median_ms"] / row["den_median_ms"], 3)
        row["gradient_ratio"] = round(row["gradient_median_ms"] / row["den_median_ms"], 3)
        print(json.dumps(row), flush=True)
        del ws, y, gamma, grad


if __name__ == "__main__":
    main()
