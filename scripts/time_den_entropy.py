"""What the entropy of the denominator graph's path posterior costs (``tc_den_path_entropy``: the value alone, a forward pass,
and the value with its gradient), beside the denominator forward-backward (``tc_den_forward_backward`` with a derivative), the
accuracy-carrying forward-backward (``tc_den_expected_accuracy_grad``) and the arc occupations (``tc_den_arc_posteriors``) on
the same graph and the same outputs, in the same run:

    C3      256 x 150 frames, 4096 pdfs, 8192 states / 65536 arcs (the entropy's per-frame vectors in LDS)
    R4      the phone-LM-structured graph of config R4 (2928 pdfs), 64 sequences of 150 frames (vectors in the workspace)

All take the 2-D float32 output and preallocated buffers.  The five take turns, ``--iters`` timed calls of each after
``--warmup``; device events around every call; per case one JSON line with the medians, the minima and the quartiles.  The
values' checks are tests/test_gpu_den_entropy.py's; here only that the two entropy launches agree bit for bit.

    python scripts/time_den_entropy.py [--iters 10] [--warmup 2]
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
        sizes = dict(den=int(lib.tc_chain_workspace_bytes(graph.ptr, S, T)),
                     accuracy_grad=int(lib.tc_den_expected_accuracy_grad_workspace_bytes(graph.ptr, S, T)),
                     arc_post=int(lib.tc_den_arc_posteriors_workspace_bytes(graph.ptr, S, T)),
                     entropy_value=int(lib.tc_den_path_entropy_workspace_bytes(graph.ptr, S, T, 0)),
                     entropy_grad=int(lib.tc_den_path_entropy_workspace_bytes(graph.ptr, S, T, 1)))
        ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device=dev)
        A, H = graph.num_arcs, graph.num_states
        rows_a, rows_e = torch.empty((S, A), device=dev), torch.empty((S, H), device=dev)
        f64 = lambda: torch.empty(S, dtype=torch.float64, device=dev)  # noqa: E731
        seq_lp, leaks, acc, ent, ent_lp, ent_v, ent_lp_v = f64(), f64(), f64(), f64(), f64(), f64(), f64()
        gamma, grad = torch.empty((S * T, P), device=dev), torch.empty((S * T, P), device=dev)
        fa = torch.empty((S, T), device=dev)
        lp, status = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        device = torch.cuda.current_device()

        def den():
            check(lib.tc_den_forward_backward(graph.ptr, S, p(y), S * T, P, P, cfg["leaky"], 1.0, 0.0, 0, p(gamma), P, p(lp),
                                              p(status), p(ws), ws.numel(), device, stream), "tc_den_forward_backward")

        def accuracy():
            check(lib.tc_den_expected_accuracy(graph.ptr, S, p(y), S * T, P, P, None, T, cfg["leaky"], p(ref), None, p(gamma), P,
                                               p(fa), p(acc), p(ws), ws.numel(), device, stream), "tc_den_expected_accuracy")

        def accuracy_grad():
            check(lib.tc_den_expected_accuracy_grad(graph.ptr, S, p(y), S * T, P, P, None, T, cfg["leaky"], p(ref), None, p(fa),
                                                    None, p(grad), P, p(ws), ws.numel(), device, stream),
                  "tc_den_expected_accuracy_grad")

        def arc_post():
            check(lib.tc_den_arc_posteriors(graph.ptr, S, p(y), S * T, P, P, None, T, cfg["leaky"], None, None, p(seq_lp), p(leaks),
                                            p(rows_a), p(rows_e), p(ws), ws.numel(), device, stream), "tc_den_arc_posteriors")

        def entropy_value():
            check(lib.tc_den_path_entropy(graph.ptr, S, p(y), S * T, P, P, None, T, cfg["leaky"], p(ent_v), p(ent_lp_v), None, 0,
                                          None, p(ws), ws.numel(), device, stream), "tc_den_path_entropy")

        def entropy_grad():
            check(lib.tc_den_path_entropy(graph.ptr, S, p(y), S * T, P, P, None, T, cfg["leaky"], p(ent), p(ent_lp), p(grad), P,
                                          None, p(ws), ws.numel(), device, stream), "tc_den_path_entropy")

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        calls = dict(den=den, accuracy_grad=accuracy_grad, arc_post=arc_post, entropy_value=entropy_value, entropy_grad=entropy_grad)
        streamed = int(lib.tc_debug_counter(b"den_entropy_streamed_launches"))
        accuracy()  # (the accuracy gradient's centring constants)
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        streamed = int(lib.tc_debug_counter(b"den_entropy_streamed_launches")) > streamed
        assert int(status.item()) == 0 and torch.equal(ent.view(torch.int64), ent_v.view(torch.int64)), config
        times = {k: [] for k in calls}
        for _ in range(args.iters):  # (the five take turns)
            for k, fn in calls.items():
                times[k].append(timed(fn))
        row = dict(config=config, S=S, T=T, pdfs=P, states=H, arcs=A, iters=args.iters, workspace_bytes=sizes,
                   vectors_in_workspace=bool(streamed), mean_entropy=float(ent.mean()), mean_logprob=float(ent_lp.mean()),
                   grad_abs_max=float(grad.abs().max()))
        for k, v in times.items():
            v = sorted(v)
            row.update({k + "_median_ms": round(v[len(v) // 2], 4), k + "_min_ms": round(v[0], 4),
                        k + "_q1_ms": round(v[len(v) // 4], 4), k + "_q3_ms": round(v[(3 * len(v)) // 4], 4)})
        print(json.dumps(row), flush=True)
        del ws, y, gamma, grad, rows_a, rows_e


if __name__ == "__main__":
    main()
