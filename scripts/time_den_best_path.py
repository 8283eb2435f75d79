"""What the best path through the denominator graph costs (``tc_den_best_path``), beside the forward-only denominator
(``tc_den_forward_backward`` with ``deriv == NULL``) on the same graph and the same outputs, in the same run:

    C3      256 x 150 frames, 4096 pdfs, 8192 states / 65536 arcs
    R4      the phone-LM-structured graph of config R4 (2928 pdfs), 64 sequences of 150 frames

Both calls take the 2-D float32 output.  The two take turns, ``--iters`` timed calls of each after ``--warmup``; device events
around every call; per case one JSON line with the medians, the minima, the quartiles (the run-to-run spread) and the ratio
best path / forward-only denominator.  The best path runs as ``io.DenominatorGraph.best_path`` runs it: under the default
workspace cap of 1 GiB, so C3's 1.3 GB of history goes in two groups.  The path's checks are tests/test_gpu_den_best_path.py's;
here only that every sequence got a finite score.

    python scripts/time_den_best_path.py [--iters 20] [--warmup 5]
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch

    from torchain_amd import io, synth
    from torchain_amd._lib import check, lib

    dev = "cuda:0"
    for config, S in (("C3", 256), ("R4", 64)):
        cfg = synth.CONFIGS[config]
        T, P = cfg["T"], cfg["P"]
        t0 = time.time()
        fst = synth.config_den_fst(config)
        graph = io.DenominatorGraph(fst, P).prepare(dev)
        print("# %s: %d states, %d arcs, ready in %.1f s" % (config, graph.num_states, graph.num_arcs, time.time() - t0), flush=True)
        y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
        stream = torch.cuda.current_stream().cuda_stream
        den_bytes = int(lib.tc_chain_workspace_bytes(graph.ptr, S, T))
        den_ws = torch.empty(den_bytes, dtype=torch.uint8, device=dev)
        lp = torch.zeros(1, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        need = int(lib.tc_den_best_path_workspace_bytes(graph.ptr, S, T))
        ws = torch.empty(min(need, 1 << 30), dtype=torch.uint8, device=dev)
        out = (torch.empty((S, T), dtype=torch.int32, device=dev), torch.empty((S,), dtype=torch.float64, device=dev))

        def den_forward():
            check(lib.tc_den_forward_backward(graph.ptr, S, C.c_void_p(y.data_ptr()), S * T, P, y.stride(0), cfg["leaky"], 1.0, 0.0,
                                              0, None, 0, C.c_void_p(lp.data_ptr()), C.c_void_p(status.data_ptr()),
                                              C.c_void_p(den_ws.data_ptr()), den_bytes, torch.cuda.current_device(),
                                              C.c_void_p(stream)), "tc_den_forward_backward")

        def best_path():
            return graph.best_path(y, n_batch=S, workspace=ws, out=out)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        launches = int(lib.tc_debug_counter(b"den_best_path_launches"))
        for _ in range(args.warmup):
            den_forward()
            best_path()
        torch.cuda.synchronize()
        groups = (int(lib.tc_debug_counter(b"den_best_path_launches")) - launches) // max(1, args.warmup)
        assert bool(torch.isfinite(out[1]).all()) and bool((out[0] >= 0).all()) and int(status.item()) == 0, config
        times = {"best_path": [], "den_forward": []}
        for _ in range(args.iters):  # (the two take turns)
            times["den_forward"].append(timed(den_forward))
            times["best_path"].append(timed(best_path))
        row = dict(config=config, S=S, T=T, pdfs=P, states=graph.num_states, arcs=graph.num_arcs, iters=args.iters,
                   workspace_bytes=need, groups=groups)
        for k, v in times.items():
            v = sorted(v)
            row.update({k + "_median_ms": round(v[len(v) // 2], 4), k + "_min_ms": round(v[0], 4),
                        k + "_q1_ms": round(v[len(v) // 4], 4), k + "_q3_ms": round(v[(3 * len(v)) // 4], 4)})
        row["ratio"] = round(row["best_path_median_ms"] / row["den_forward_median_ms"], 3)
        print(json.dumps(row), flush=True)
        del den_ws, ws, y


if __name__ == "__main__":
    main()
