"""What the arc occupations of an end-to-end supervision cost (``tc_supervision_arc_posteriors``): the resident form and, with
``tc_debug_set("force_num_arc_post_large", 1)``, the large form, beside the numerator's forward-backward
(``tc_num_forward_backward`` with a derivative) on the same handle, at a config's shape (C3: 256 x 150, 4096 pdfs) on the
end-to-end ``chain`` batch of scripts/time_best_path.py (words of 1-4 phones, about one phone per 4 frames).

All take the 2-D float32 output.  They take turns, ``--iters`` timed calls of each after ``--warmup``; device events around
every call; one JSON line with the medians, the minima and the ratios to the numerator.  The values are
tests/test_gpu_num_arc_post.py's business; here only that every sequence's arcs sum to its frames, that the two forms agree
bit for bit and that ``logprob`` is the numerator's.

    python scripts/time_num_arc_post.py [--config C3] [--iters 20] [--warmup 5]
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
    out = torch.zeros_like(y)  # the numerator's derivative
    num_bytes = 256 * ((S * 8 + 255) // 256) + 256
    check(lib.tc_debug_set(b"force_num_arc_post_large", 1), "tc_debug_set")
    arc_bytes = int(lib.tc_supervision_arc_posteriors_workspace_bytes(sup.ptr))  # (the large form's: the larger one)
    check(lib.tc_debug_set(b"force_num_arc_post_large", 0), "tc_debug_set")
    check(min(arc_bytes, 0), "tc_supervision_arc_posteriors_workspace_bytes")
    ws = torch.empty(max(num_bytes, arc_bytes), dtype=torch.uint8, device=dev)
    lp = torch.zeros(1, dtype=torch.float64, device=dev)
    arc_off, state_off = np.zeros(S + 1, np.int64), np.zeros(S + 1, np.int64)
    check(lib.tc_supervision_arc_posteriors_offsets(sup.ptr, arc_off.ctypes.data_as(C.c_void_p), state_off.ctypes.data_as(C.c_void_p)),
          "tc_supervision_arc_posteriors_offsets")
    arcs = {k: torch.zeros(int(arc_off[-1]), dtype=torch.float64, device=dev) for k in ("resident", "large")}
    finals = torch.zeros(int(state_off[-1]), dtype=torch.float64, device=dev)
    alp = torch.zeros(S, dtype=torch.float64, device=dev)

    def numerator():
        check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y.data_ptr()), S * T, P, y.stride(0), C.c_void_p(out.data_ptr()), P,
                                          C.c_void_p(lp.data_ptr()), C.c_void_p(ws.data_ptr()), num_bytes, device,
                                          C.c_void_p(stream)), "tc_num_forward_backward")

    def arc_post(kind):
        check(lib.tc_debug_set(b"force_num_arc_post_large", int(kind == "large")), "tc_debug_set")
        try:
            check(lib.tc_supervision_arc_posteriors(sup.ptr, C.c_void_p(y.data_ptr()), 0, 0, S * T, P, y.stride(0),
                                                    C.c_void_p(arcs[kind].data_ptr()), C.c_void_p(finals.data_ptr()),
                                                    C.c_void_p(alp.data_ptr()), C.c_void_p(ws.data_ptr()), arc_bytes, device,
                                                    C.c_void_p(stream)), "tc_supervision_arc_posteriors")
        finally:
            check(lib.tc_debug_set(b"force_num_arc_post_large", 0), "tc_debug_set")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    calls = {"numerator": numerator, "arc_post_resident": lambda: arc_post("resident"), "arc_post_large": lambda: arc_post("large")}
    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    sums = np.add.reduceat(arcs["resident"].cpu().numpy(), arc_off[:-1])
    assert np.abs(sums - T).max() <= 1e-4 * T and torch.equal(arcs["resident"], arcs["large"])
    assert abs(float(alp.sum()) - float(lp[0])) <= 1e-9 * abs(float(lp[0]))  # (weight 1: the numerator's log Z)
    times = {k: [] for k in calls}
    for _ in range(args.iters):  # (the three take turns)
        for k, fn in calls.items():
            times[k].append(timed(fn))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    row = dict(config=args.config, S=S, T=T, P=P, iters=args.iters, arcs=int(arc_off[-1]), states=int(state_off[-1]),
               workspace_mb=round(arc_bytes / 2 ** 20, 1), worst_arc_sum_error=float(np.abs(sums - T).max()))
    for k in calls:
        row.update({k + "_median_ms": round(med[k], 4), k + "_min_ms": round(min(times[k]), 4)})
    row.update(resident_over_numerator=round(med["arc_post_resident"] / med["numerator"], 3),
               large_over_numerator=round(med["arc_post_large"] / med["numerator"], 3))
    print(json.dumps(row), flush=True)
    print(json.dumps({k: int(lib.tc_debug_counter(k.encode())) for k in ("num_arc_post_launches", "num_arc_post_large_launches")}), flush=True)


if __name__ == "__main__":
    main()
