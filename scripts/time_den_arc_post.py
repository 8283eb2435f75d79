"""What the arc and entry occupations of the denominator graph cost (``tc_den_arc_posteriors``: the slot-owned
forward-backward, and the reduction over the sequences timed by itself through ``tc_den_arc_posteriors_reduce``), beside
the denominator forward-backward (``tc_den_forward_backward`` with a derivative) and the accuracy-carrying forward-backward
(``tc_den_expected_accuracy_grad``) on the same graph and the same outputs, in the same run:

    C3      256 x 150 frames, 4096 pdfs, 8192 states / 65536 arcs (64 slots a thread: accumulators in registers)
    R4      the phone-LM-structured graph of config R4 (2928 pdfs), 64 sequences of 150 frames (accumulators and per-state
            vectors in the workspace)

All take the 2-D float32 output and preallocated buffers.  The four take turns, ``--iters`` timed calls of each after
``--warmup``; device events around every call; per case one JSON line with the medians, the minima, the quartiles and the
ratios to the denominator.  The values' checks are tests/test_gpu_den_arc_post.py's; here only that the arc occupations sum
to the frames.

    python scripts/time_den_arc_post.py [--iters 10] [--warmup 2]
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
        arc_bytes = int(lib.tc_den_arc_posteriors_workspace_bytes(graph.ptr, S, T))
        ws = torch.empty(max(den_bytes, grad_bytes, arc_bytes), dtype=torch.uint8, device=dev)
        A, H = graph.num_arcs, graph.num_states
        rows_a, rows_e = torch.empty((S, A), device=dev), torch.empty((S, H), device=dev)
        arcs, entries = torch.empty(A, dtype=torch.float64, device=dev), torch.empty(H, dtype=torch.float64, device=dev)
        seq_lp, leaks = torch.empty(S, dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.float64, device=dev)
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

        def arc_post():
            check(lib.tc_den_arc_posteriors(graph.ptr, S, p(y), S * T, P, P, None, T, cfg["leaky"], None, None, p(seq_lp), p(leaks),
                                            p(rows_a), p(rows_e), p(ws), ws.numel(), device, stream), "tc_den_arc_posteriors")

        def reduce():
            check(lib.tc_den_arc_posteriors_reduce(S, A, H, p(rows_a), p(rows_e), p(arcs), p(entries), device, stream),
                  "tc_den_arc_posteriors_reduce")

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        streamed = int(lib.tc_debug_counter(b"den_arc_post_streamed_launches"))
        accuracy()  # (the gradient's centring constants)
        for _ in range(args.warmup):
            den()
            gradient()
            arc_post()
            reduce()
        torch.cuda.synchronize()
        streamed = int(lib.tc_debug_counter(b"den_arc_post_streamed_launches")) > streamed
        assert int(status.item()) == 0 and abs(float(arcs.sum()) - S * T) <= 1e-4 * S * T, (config, float(arcs.sum()))
        times = {"den": [], "gradient": [], "arc_post": [], "reduce": []}
        for _ in range(args.iters):  # (the four take turns)
            times["den"].append(timed(den))
            times["gradient"].append(timed(gradient))
            times["arc_post"].append(timed(arc_post))
            times["reduce"].append(timed(reduce))
        row = dict(config=config, S=S, T=T, pdfs=P, states=graph.num_states, arcs=graph.num_arcs, iters=args.iters,
                   den_workspace_bytes=den_bytes, grad_workspace_bytes=grad_bytes, arc_post_workspace_bytes=arc_bytes,
                   accumulators_in_workspace=bool(streamed), arcs_sum=float(arcs.sum()), mean_leaks=float(leaks.mean()))
        for k, v in times.items():
            v = sorted(v)
            row.update({k + "_median_ms": round(v[len(v) // 2], 4), k + "_min_ms": round(v[0], 4),
                        k + "_q1_ms": round(v[len(v) // 4], 4), k + "_q3_ms": round(v[(3 * len(v)) // 4], 4)})
        row["arc_post_ratio"] = round(row["arc_post_median_ms"] / row["den_median_ms"], 3)
        row["arc_post_to_gradient"] = round(row["arc_post_median_ms"] / row["gradient_median_ms"], 3)
        print(json.dumps(row), flush=True)
        del ws, y, gamma, grad, rows_a, rows_e


if __name__ == "__main__":
    main()
