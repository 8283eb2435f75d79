"""What the alignment entropy of an end-to-end supervision costs (``tc_supervision_path_entropy``): the value alone (the
kernel's forward pass) and the value with its gradient, beside the numerator's forward-backward (``tc_num_forward_backward``
with a derivative, the kernel of the parent commit) on the same handle, at a config's shape (C3: 256 x 150, 4096 pdfs) on the
end-to-end ``chain`` batch of scripts/time_best_path.py (words of 1-4 phones, about one phone per 4 frames).

All three take the 2-D float32 output and write a (T*S, P) float32 matrix where they write one.  They take turns, ``--iters``
timed calls of each after ``--warmup``; device events around every call; one JSON line with the medians, the minima and the
ratios to the numerator.  The values are tests/test_gpu_num_entropy.py's business; here only that every sequence got a
finite entropy and that ``logprob`` is the numerator's.

    python scripts/time_num_entropy.py [--config C3] [--iters 20] [--warmup 5]
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
    rng = np.random.default_rng(0)
    sup = io.Supervision.from_e2e_fsts(1.0, T, P, [ref.chain_fst(P, rng, words=max(1, T // 15), max_phones=4) for _ in range(S)])
    print("# supervision ready in %.1f s: %s" % (time.time() - t0, sup.e2e_stats()), flush=True)
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    device = torch.cuda.current_device()
    out = torch.zeros_like(y)  # the numerator's derivative / the entropy's gradient
    num_bytes = 256 * ((S * 8 + 255) // 256) + 256
    ent_bytes = int(lib.tc_supervision_path_entropy_workspace_bytes(sup.ptr, 1))
    check(min(ent_bytes, 0), "tc_supervision_path_entropy_workspace_bytes")
    ws = torch.empty(max(num_bytes, ent_bytes), dtype=torch.uint8, device=dev)
    lp = torch.zeros(1, dtype=torch.float64, device=dev)
    ent, elp = (torch.zeros(S, dtype=torch.float64, device=dev) for _ in range(2))

    def numerator():
        check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y.data_ptr()), S * T, P, y.stride(0), C.c_void_p(out.data_ptr()), P,
                                          C.c_void_p(lp.data_ptr()), C.c_void_p(ws.data_ptr()), num_bytes, device,
                                          C.c_void_p(stream)), "tc_num_forward_backward")

    def entropy(grad):
        check(lib.tc_supervision_path_entropy(sup.ptr, C.c_void_p(y.data_ptr()), 0, 0, S * T, P, y.stride(0),
                                              C.c_void_p(ent.data_ptr()), C.c_void_p(elp.data_ptr()),
                                              C.c_void_p(out.data_ptr()) if grad else None, P, None,
                                              C.c_void_p(ws.data_ptr()) if grad else None, ent_bytes if grad else 0, device,
                                              C.c_void_p(stream)), "tc_supervision_path_entropy")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    calls = {"numerator": numerator, "entropy_value": lambda: entropy(False), "entropy_value_grad": lambda: entropy(True)}
    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ent).all()) and bool((ent >= 0).all())
    assert abs(float(elp.sum()) - float(lp[0])) <= 1e-9 * abs(float(lp[0]))  # (weight 1: the numerator's log Z)
    times = {k: [] for k in calls}
    for _ in range(args.iters):  # (the three take turns)
        for k, fn in calls.items():
            times[k].append(timed(fn))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    row = dict(config=args.config, S=S, T=T, P=P, iters=args.iters, workspace_mb=round(ent_bytes / 2 ** 20, 1),
               mean_entropy=round(float(ent.mean()), 3))
    for k in calls:
        row.update({k + "_median_ms": round(med[k], 4), k + "_min_ms": round(min(times[k]), 4)})
    row.update(value_over_numerator=round(med["entropy_value"] / med["numerator"], 3),
               value_grad_over_numerator=round(med["entropy_value_grad"] / med["numerator"], 3))
    print(json.dumps(row), flush=True)
    print(json.dumps(dict(num_entropy_launches=int(lib.tc_debug_counter(b"num_entropy_launches")))), flush=True)


if __name__ == "__main__":
    main()
