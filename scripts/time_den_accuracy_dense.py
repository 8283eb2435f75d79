"""What lattice-free sMBR against a dense accuracy matrix costs (``tc_den_expected_accuracy_dense`` and ``_dense_grad``) beside
the hard-reference entries (``tc_den_expected_accuracy`` and ``_grad``) on the same graph, the same outputs and the same
reference, in the same run:

    C3      256 x 150 frames, 4096 pdfs, 8192 states / 65536 arcs
    R4      the phone-LM-structured graph of config R4 (2928 pdfs), 64 sequences of 150 frames

The reference is the graph's own best path, state-level classes; the dense matrix is its float32 indicator, so the two pairs
compute the same numbers, and the script checks that they are the same bits before it times anything.  The four entries take
turns, ``--iters`` timed calls of each after ``--warmup``; device events around every call; per case one JSON line with the
medians, the minima, the quartiles and the ratios dense / hard.  All take the 2-D float32 output and preallocated buffers.

Then, at C3's shape, ``Supervision.posteriors`` -- the matrix Kaldi's chain-sMBR passes -- on the three-path and the 40-path
supervision of scripts/time_best_path.py, beside ``tc_num_forward_backward`` alone into a zeroed matrix (what it is built on):
a host clock around calls that end in a device synchronise, since the method allocates and runs torch kernels of its own.

    python scripts/time_den_accuracy_dense.py [--iters 10] [--warmup 2] [--configs C3:256,R4:64] [--posteriors C3]

scripts/time_den_accuracy.py times the hard entries alone; it runs unchanged on the commit before this one, which is how the
two builds were compared (profiles/den_accuracy_dense/README.md).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def summary(row, key, v):
    v = sorted(v)
    row.update({key + "_median_ms": round(v[len(v) // 2], 4), key + "_min_ms": round(v[0], 4),
                key + "_q1_ms": round(v[len(v) // 4], 4), key + "_q3_ms": round(v[(3 * len(v)) // 4], 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="C3:256,R4:64")
    ap.add_argument("--posteriors", default="C3", help="the config at whose shape Supervision.posteriors is timed ('' for none)")
    args = ap.parse_args()

    import torch

    from torchain_amd import io, synth
    from torchain_amd._lib import check, lib

    dev = "cuda:0"
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for item in [i for i in args.configs.split(",") if i]:
        config, S = item.split(":")[0], int(item.split(":")[1])
        cfg = synth.CONFIGS[config]
        T, P = cfg["T"], cfg["P"]
        t0 = time.time()
        fst = synth.config_den_fst(config)
        graph = io.DenominatorGraph(fst, P).prepare(dev)
        print("# %s: %d states, %d arcs, ready in %.1f s" % (config, graph.num_states, graph.num_arcs, time.time() - t0), flush=True)
        y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
        ref = graph.best_path(y, n_batch=S)[0]  # (S, T)
        dense = torch.zeros((T * S, P), device=dev)  # row t*S + s: the indicator of ref[s, t]
        dense.view(T, S, P).scatter_(2, ref.t().long().unsqueeze(2), 1.0)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        den_bytes = int(lib.tc_den_expected_accuracy_workspace_bytes(graph.ptr, S, T))
        grad_bytes = int(lib.tc_den_expected_accuracy_grad_workspace_bytes(graph.ptr, S, T))
        ws = torch.empty(max(den_bytes, grad_bytes), dtype=torch.uint8, device=dev)
        gamma, grad = torch.empty((S * T, P), device=dev), torch.empty((S * T, P), device=dev)
        fa, acc = torch.empty((S, T), device=dev), torch.empty((S,), dtype=torch.float64, device=dev)
        device = torch.cuda.current_device()
        leaky = cfg["leaky"]

        def hard_value():
            check(lib.tc_den_expected_accuracy(graph.ptr, S, p(y), S * T, P, P, None, T, leaky, p(ref), None, p(gamma), P,
                                               p(fa), p(acc), p(ws), ws.numel(), device, stream), "tc_den_expected_accuracy")

        def dense_value():
            check(lib.tc_den_expected_accuracy_dense(graph.ptr, S, p(y), S * T, P, P, None, T, leaky, p(dense), P, p(gamma), P,
                                                     p(fa), p(acc), p(ws), ws.numel(), device, stream),
                  "tc_den_expected_accuracy_dense")

        def hard_gradient():
            check(lib.tc_den_expected_accuracy_grad(graph.ptr, S, p(y), S * T, P, P, None, T, leaky, p(ref), None, p(fa),
                                                    None, p(grad), P, p(ws), ws.numel(), device, stream),
                  "tc_den_expected_accuracy_grad")

        def dense_gradient():
            check(lib.tc_den_expected_accuracy_dense_grad(graph.ptr, S, p(y), S * T, P, P, None, T, leaky, p(dense), P, p(fa),
                                                          None, p(grad), P, p(ws), ws.numel(), device, stream),
                  "tc_den_expected_accuracy_dense_grad")

        calls = (("hard_value", hard_value), ("dense_value", dense_value), ("hard_gradient", hard_gradient),
                 ("dense_gradient", dense_gradient))
        # the same bits from the two pairs, and the warm-up
        streamed = int(lib.tc_debug_counter(b"den_accuracy_grad_streamed_launches"))
        kept = {}
        for _ in range(max(1, args.warmup)):
            for name, fn in calls:
                fn()
                torch.cuda.synchronize()
                kept[name] = [o.clone() for o in ((acc, fa) if name.endswith("value") else (grad,))]
        streamed = int(lib.tc_debug_counter(b"den_accuracy_grad_streamed_launches")) > streamed
        for kind in ("value", "gradient"):
            for u, v in zip(kept["hard_" + kind], kept["dense_" + kind]):
                assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (config, kind)
        assert bool(torch.isfinite(grad).all()) and bool((acc >= 0).all()) and bool((acc <= T).all()), config
        times = {name: [] for name, _ in calls}
        for _ in range(args.iters):  # (the four take turns)
            for name, fn in calls:
                times[name].append(timed(fn))
        row = dict(config=config, S=S, T=T, pdfs=P, states=graph.num_states, arcs=graph.num_arcs, iters=args.iters,
                   den_workspace_bytes=den_bytes, grad_workspace_bytes=grad_bytes, grad_vectors_in_workspace=bool(streamed),
                   same_bits=True, mean_accuracy=round(float(acc.mean()), 3), largest_gradient=float(grad.abs().max()))
        for name, v in times.items():
            summary(row, name, v)
        row["value_ratio"] = round(row["dense_value_median_ms"] / row["hard_value_median_ms"], 3)
        row["gradient_ratio"] = round(row["dense_gradient_median_ms"] / row["hard_gradient_median_ms"], 3)
        print(json.dumps(row), flush=True)
        del ws, y, gamma, grad, dense, kept

    if args.posteriors:
        cfg = synth.CONFIGS[args.posteriors]
        S, T, P = cfg["S"], cfg["T"], cfg["P"]
        fst = synth.config_den_fst(args.posteriors)
        y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        nbytes = 256 * ((S * 8 + 255) // 256) + 256
        ws, deriv = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty((S * T, P), device=dev)
        for name, paths in (("trie3", 3), ("trie40", 40)):
            sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, paths, seed=3))

            def numerator():
                deriv.zero_()
                check(lib.tc_num_forward_backward(sup.ptr, p(y), S * T, P, P, p(deriv), P, None, p(ws), nbytes,
                                                  torch.cuda.current_device(), stream), "tc_num_forward_backward")

            def host_timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0), out

            for _ in range(max(1, args.warmup)):
                numerator()
                post = sup.posteriors(y)
            torch.cuda.synchronize()
            assert float((post.sum(dim=1) - 1).abs().max()) <= 1e-5, name
            times = {"numerator": [], "posteriors": []}
            for _ in range(args.iters):  # (the two take turns)
                times["numerator"].append(host_timed(numerator)[0])
                times["posteriors"].append(host_timed(lambda: sup.posteriors(y))[0])
            row = dict(config=args.posteriors, supervision=name, S=S, T=T, pdfs=P, iters=args.iters, kernel=sup.stats()["kernel"])
            for k, v in times.items():
                summary(row, k, v)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
