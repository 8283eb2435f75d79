"""What the large alignment-entropy kernel costs (``num_entropy_large_kernels.hip``), two measurements:

``--what both``: one handle that fits both kernels -- a config's shape (C3: 256 x 150, 4096 pdfs) on the end-to-end ``chain``
batch of scripts/time_num_entropy.py -- on the resident kernel and, with ``tc_debug_set("force_num_entropy_large", 1)``, on the
large one: the value alone and the value with its gradient.  The price of keeping the means in L2; the two give the same bits,
which is checked.

``--what large``: 256 sequences of 8000 states (four distinct ``random_fst(8000, 24000, 64)`` in turn), 20 frames, which only
the large kernel serves, beside the large numerator's forward-backward (``tc_num_forward_backward``) on the same handle.

The calls take turns, ``--iters`` timed calls of each after ``--warmup``; device events around every call; one JSON line with
the medians, the minima and the quartiles' spread.

    python scripts/time_num_entropy_large.py [--what both|large] [--config C3] [--iters 20] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="both", choices=("both", "large"))
    ap.add_argument("--config", default="C3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch

    import e2e_reference as ref
    from torchain_amd import io, synth
    from torchain_amd._lib import check, lib

    dev, rng = "cuda:0", np.random.default_rng(0)
    if args.what == "both":
        cfg = synth.CONFIGS[args.config]
        S, T, P = cfg["S"], cfg["T"], cfg["P"]
        sup = io.Supervision.from_e2e_fsts(1.0, T, P, [ref.chain_fst(P, rng, words=max(1, T // 15), max_phones=4) for _ in range(S)])
    else:
        S, T, P = 256, 20, 64
        four = [ref.random_fst(8000, 24000, P, rng) for _ in range(4)]
        sup = io.Supervision.from_e2e_fsts(1.0, T, P, [four[s % 4] for s in range(S)], any_size=True)
    print("# %s" % sup.e2e_stats(), flush=True)
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    stream, device = torch.cuda.current_stream().cuda_stream, torch.cuda.current_device()
    out = {k: torch.zeros_like(y) for k in ("resident", "large", "numerator")}
    ent, elp = ({k: torch.zeros(S, dtype=torch.float64, device=dev) for k in out} for _ in range(2))
    lp = torch.zeros(1, dtype=torch.float64, device=dev)
    num_bytes = 256 * ((S * 8 + 255) // 256) + 256

    def need(grad):
        n = int(lib.tc_supervision_path_entropy_workspace_bytes(sup.ptr, grad))
        check(min(n, 0), "tc_supervision_path_entropy_workspace_bytes")
        return n

    check(lib.tc_debug_set(b"force_num_entropy_large", 1), "tc_debug_set")
    ws_bytes = max(need(1), num_bytes)  # (the large kernel's is the larger)
    check(lib.tc_debug_set(b"force_num_entropy_large", 0), "tc_debug_set")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def numerator():
        check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y.data_ptr()), S * T, P, y.stride(0), C.c_void_p(out["numerator"].data_ptr()),
                                          P, C.c_void_p(lp.data_ptr()), C.c_void_p(ws.data_ptr()), num_bytes, device, C.c_void_p(stream)),
              "tc_num_forward_backward")

    def entropy(kind, grad):
        check(lib.tc_debug_set(b"force_num_entropy_large", int(kind == "large")), "tc_debug_set")
        try:
            assert sup.path_entropy_kernel() == int(kind == "large")
            check(lib.tc_supervision_path_entropy(sup.ptr, C.c_void_p(y.data_ptr()), 0, 0, S * T, P, y.stride(0),
                                                  C.c_void_p(ent[kind].data_ptr()), C.c_void_p(elp[kind].data_ptr()),
                                                  C.c_void_p(out[kind].data_ptr()) if grad else None, P, None, C.c_void_p(ws.data_ptr()),
                                                  ws_bytes, device, C.c_void_p(stream)), "tc_supervision_path_entropy")
        finally:
            check(lib.tc_debug_set(b"force_num_entropy_large", 0), "tc_debug_set")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    calls = {"large_value": lambda: entropy("large", False), "large_value_grad": lambda: entropy("large", True)}
    if args.what == "both":
        calls.update(resident_value=lambda: entropy("resident", False), resident_value_grad=lambda: entropy("resident", True))
    else:
        calls.update(numerator=numerator)
    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ent["large"]).all()) and bool((ent["large"] >= 0).all())
    if args.what == "both":
        assert all(torch.equal(a["resident"], a["large"]) for a in (ent, elp, out))
    times = {k: [] for k in calls}
    for _ in range(args.iters):  # (the calls take turns)
        for k, fn in calls.items():
            times[k].append(timed(fn))
    row = dict(what=args.what, S=S, T=T, P=P, iters=args.iters, workspace_mb=round(ws_bytes / 2 ** 20, 1),
               mean_entropy=round(float(ent["large"].mean()), 3))
    for k, v in times.items():
        v = sorted(v)
        row.update({k + "_median_ms": round(v[len(v) // 2], 4), k + "_min_ms": round(v[0], 4),
                    k + "_iqr_ms": round(v[(3 * len(v)) // 4] - v[len(v) // 4], 4)})
    print(json.dumps(row), flush=True)
    print(json.dumps({k: int(lib.tc_debug_counter(k.encode())) for k in ("num_entropy_launches", "num_entropy_large_launches")}), flush=True)


if __name__ == "__main__":
    main()
