"""What drawing paths from the denominator's posterior costs (``tc_den_sample_paths``, ``K = 1`` and ``K = 8`` samples a
sequence) beside, on the same graph and the same outputs, in the same run and taking turns:

    best_path   tc_den_best_path (the same forward pass with a max for the sum, one traceback)
    den         tc_den_forward_backward with a derivative (the chain step's denominator)
    gradient    tc_den_expected_accuracy_grad (the exact sMBR gradient's kernel alone)

and one full sMBR step of each kind, from the network output to its gradient, through ``torchain_amd.functions``:

    sampled_step  den_sample_paths (K = 8) -> frame-accuracy risks -> sampled_risk_surrogate(...).sum().backward()
    exact_step    den_expected_accuracy(...).sum().backward()

    C3      256 x 150 frames, 4096 pdfs, 8192 states / 65536 arcs
    R4      the phone-LM-structured graph of config R4 (2928 pdfs), 64 sequences of 150 frames

The kernel entries take the 2-D float32 output and preallocated buffers; the uniforms are drawn outside the timed calls.
The reference of the sMBR steps is the graph's own best path.  ``--iters`` timed calls of each after ``--warmup``; device
events around every call (the steps end in a synchronise); per case one JSON line with the medians, the minima and the
quartiles.  The values' checks are tests/test_gpu_den_sample.py's; here only that every slot got a pdf.

    python scripts/time_den_sample.py [--iters 10] [--warmup 2] [--configs C3:256,R4:64]
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
    from torchain_amd.functions import den_expected_accuracy, den_sample_paths, sampled_risk_surrogate

    if not torch.cuda.is_available():
        raise SystemExit("time_den_sample.py measures on the GPU: none is available")
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
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        sizes = dict(sample=int(lib.tc_den_sample_paths_workspace_bytes(graph.ptr, S, T)),
                     best_path=int(lib.tc_den_best_path_workspace_bytes(graph.ptr, S, T)),
                     den=int(lib.tc_chain_workspace_bytes(graph.ptr, S, T)),
                     gradient=int(lib.tc_den_expected_accuracy_grad_workspace_bytes(graph.ptr, S, T)))
        ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device=dev)
        gamma, grad = torch.empty((S * T, P), device=dev), torch.empty((S * T, P), device=dev)
        fa, acc = torch.empty((S, T), device=dev), torch.empty((S,), dtype=torch.float64, device=dev)
        lp, status = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        ref, score = torch.empty((S, T), dtype=torch.int32, device=dev), torch.empty((S,), dtype=torch.float64, device=dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        uni = {K: torch.rand((S, K, T + 1, 3), generator=gen, device=dev) for K in (1, 8)}
        out = {K: torch.empty((S, K, T), dtype=torch.int32, device=dev) for K in (1, 8)}
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        device = torch.cuda.current_device()
        leaky = cfg["leaky"]

        def sample(K):
            check(lib.tc_den_sample_paths(graph.ptr, S, p(y), S * T, P, P, None, T, leaky, K, p(uni[K]), p(out[K]), None, p(ws),
                                          ws.numel(), device, stream), "tc_den_sample_paths")

        def best_path():
            check(lib.tc_den_best_path(graph.ptr, S, p(y), 0, 0, S * T, P, P, None, T, p(ref), None, p(score), p(ws), ws.numel(),
                                       device, stream), "tc_den_best_path")

        def den():
            check(lib.tc_den_forward_backward(graph.ptr, S, p(y), S * T, P, P, leaky, 1.0, 0.0, 0, p(gamma), P, p(lp), p(status),
                                              p(ws), ws.numel(), device, stream), "tc_den_forward_backward")

        def gradient():
            check(lib.tc_den_expected_accuracy_grad(graph.ptr, S, p(y), S * T, P, P, None, T, leaky, p(ref), None, p(fa), None,
                                                    p(grad), P, p(ws), ws.numel(), device, stream), "tc_den_expected_accuracy_grad")

        def accuracy():  # (not timed: leaves the centring constants the gradient kernel reads)
            check(lib.tc_den_expected_accuracy(graph.ptr, S, p(y), S * T, P, P, None, T, leaky, p(ref), None, p(gamma), P, p(fa),
                                               p(acc), p(ws), ws.numel(), device, stream), "tc_den_expected_accuracy")

        def sampled_step():
            x = y.detach().requires_grad_(True)
            pdfs = den_sample_paths(x, graph, 8, n_batch=S, leaky_hmm_coefficient=leaky, generator=gen)
            risks = (pdfs == ref.unsqueeze(1)).sum(dim=2)
            sampled_risk_surrogate(x, pdfs, risks).sum().backward()
            return x.grad

        def exact_step():
            x = y.detach().requires_grad_(True)
            den_expected_accuracy(x, graph, ref, n_batch=S, leaky_hmm_coefficient=leaky).sum().backward()
            return x.grad

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        calls = {"sample_k1": lambda: sample(1), "sample_k8": lambda: sample(8), "best_path": best_path, "den": den,
                 "gradient": gradient, "sampled_step": sampled_step, "exact_step": exact_step}
        best_path()
        accuracy()
        streamed = int(lib.tc_debug_counter(b"den_sample_streamed_launches"))
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        streamed = int(lib.tc_debug_counter(b"den_sample_streamed_launches")) > streamed
        assert int(status.item()) == 0 and bool(torch.isfinite(grad).all()), config
        assert bool((out[1] >= 0).all()) and bool((out[8] >= 0).all()) and bool((ref >= 0).all()), config
        times = {k: [] for k in calls}
        for _ in range(args.iters):  # (they take turns)
            for k, fn in calls.items():
                times[k].append(timed(fn))
        row = dict(config=config, S=S, T=T, pdfs=P, states=graph.num_states, arcs=graph.num_arcs, iters=args.iters, leaky=leaky,
                   workspace_bytes=sizes, alpha_from_workspace=bool(streamed),
                   sampled_accuracy_k8=round(float((out[8] == ref.unsqueeze(1)).float().mean()), 4))
        for k, v in times.items():
            v = sorted(v)
            row.update({k + "_median_ms": round(v[len(v) // 2], 4), k + "_min_ms": round(v[0], 4),
                        k + "_q1_ms": round(v[len(v) // 4], 4), k + "_q3_ms": round(v[(3 * len(v)) // 4], 4)})
        row["traceback_7_samples_ms"] = round(row["sample_k8_median_ms"] - row["sample_k1_median_ms"], 4)
        row["sample_k8_over_den"] = round(row["sample_k8_median_ms"] / row["den_median_ms"], 3)
        row["sample_k8_over_best_path"] = round(row["sample_k8_median_ms"] / row["best_path_median_ms"], 3)
        row["exact_step_over_sampled_step"] = round(row["exact_step_median_ms"] / row["sampled_step_median_ms"], 3)
        print(json.dumps(row), flush=True)
        del ws, y, gamma, grad, uni, out


if __name__ == "__main__":
    main()
