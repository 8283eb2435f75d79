"""What the best-path alignment costs (``tc_supervision_best_path``), beside the numerator's forward-backward
(``tc_num_forward_backward`` with a derivative) on the same handle, at a config's shape (C3: 256 x 150, 4096 pdfs), for three
supervisions:

    trie3     three paths a sequence: the usual regular supervision
    trie40    40 paths: the largest trie that still fits the resident numerator kernel
    e2e       the end-to-end ``chain`` batch of scripts/time_e2e.py (words of 1-4 phones, about one phone per 4 frames)

Both calls take the 2-D float32 output.  The two take turns, ``--iters`` timed calls of each after ``--warmup``; device events
around every call; per case one JSON line with the medians, the minima, the ratio best_path / numerator and which numerator
kernel ran.  Where that is the resident kernel, the level-windowed one -- the kernel the regular best path is shaped after -- is
timed on the handle as well (``tc_debug_set("force_num_windowed", 1)``).  The alignment's checks (the path is one of the
acceptor's, its score is optimal to the derived bound) are tests/test_gpu_best_path.py's; here only that every sequence got a
path.

    python scripts/time_best_path.py [--config C3] [--iters 20] [--warmup 5]
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
    args = ap.parse_args()

    import torch

    import e2e_reference as ref
    from torchain_amd import io, synth
    from torchain_amd._lib import check, lib

    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    dev = "cuda:0"
    t0 = time.time()
    fst = synth.config_den_fst(args.config)
    rng = np.random.default_rng(0)
    sups = {
        "trie3": io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=3)),
        "trie40": io.Supervision.from_synth(synth.random_supervision(fst, S, T, 40, seed=3)),
        "e2e": io.Supervision.from_e2e_fsts(1.0, T, P, [ref.chain_fst(P, rng, words=max(1, T // 15), max_phones=4)
                                                        for _ in range(S)]),
    }
    print("# supervisions ready in %.1f s" % (time.time() - t0), flush=True)
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = 256 * ((S * 8 + 255) // 256) + 256
    deriv = torch.zeros_like(y)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lp = torch.zeros(1, dtype=torch.float64, device=dev)

    def numerator(sup):
        check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y.data_ptr()), S * T, P, y.stride(0), C.c_void_p(deriv.data_ptr()), P,
                                          C.c_void_p(lp.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, torch.cuda.current_device(),
                                          C.c_void_p(stream)), "tc_num_forward_backward")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for case, sup in sups.items():
        windowed = int(lib.tc_debug_counter(b"num_windowed_launches"))
        for _ in range(args.warmup):
            numerator(sup)
            pdfs, scores = sup.best_path(y)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(scores).all()) and bool((pdfs >= 0).all()), case
        times = {"best_path": [], "numerator": []}
        for _ in range(args.iters):  # (the two take turns)
            times["numerator"].append(timed(lambda: numerator(sup)))
            times["best_path"].append(timed(lambda: sup.best_path(y)))
        kernel = "e2e" if sup.is_e2e else ("windowed" if int(lib.tc_debug_counter(b"num_windowed_launches")) > windowed
                                           else "resident")
        if kernel == "resident":  # ... and the level-windowed numerator, the kernel the regular best path is shaped after
            check(lib.tc_debug_set(b"force_num_windowed", 1), "tc_debug_set")
            for _ in range(args.warmup):
                numerator(sup)
            times["numerator_windowed"] = [timed(lambda: numerator(sup)) for _ in range(args.iters)]
            check(lib.tc_debug_set(b"force_num_windowed", 0), "tc_debug_set")
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        row = dict(config=args.config, case=case, iters=args.iters, numerator_kernel=kernel,
                   best_path_median_ms=round(med["best_path"], 4), best_path_min_ms=round(min(times["best_path"]), 4),
                   numerator_median_ms=round(med["numerator"], 4), numerator_min_ms=round(min(times["numerator"]), 4),
                   ratio=round(med["best_path"] / med["numerator"], 3))
        if "numerator_windowed" in med:
            row.update(numerator_windowed_median_ms=round(med["numerator_windowed"], 4),
                       ratio_windowed=round(med["best_path"] / med["numerator_windowed"], 3))
        print(json.dumps(row), flush=True)
    print(json.dumps(dict(best_path_launches=int(lib.tc_debug_counter(b"best_path_launches")))), flush=True)


if __name__ == "__main__":
    main()
