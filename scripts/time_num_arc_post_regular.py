"""What the arc occupations of a regular supervision cost (``tc_supervision_arc_posteriors_regular``): the kernel with the terms
of a level's arcs in LDS and with the spill form forced on the same handle (``force_num_arc_post_regular_spill``), beside the
numerator's forward-backward (``tc_num_forward_backward`` with a derivative) on whichever kernel the handle takes and with
``force_num_windowed`` -- the level-windowed numerator, which does the same walk -- at a config's shape (C3: 256 x 150, 4096
pdfs), on the three supervisions of ``scripts/time_num_entropy_regular.py`` (its pieces and its cache):

    trie3    three paths a sequence
    trie40   forty paths a sequence
    lattice  lattice-like, 30-60 states a level

All entries take the 2-D float32 output.  ``--rounds`` rounds; in a round the entries take turns, ``--iters`` timed calls of
each, device events around every call, the round's figure the median; one JSON line per supervision with the median of the
rounds' medians and the smallest and largest of them.

    python scripts/time_num_arc_post_regular.py [--config C3] [--rounds 5] [--iters 10] [--warmup 5] [--cache DIR]
"""
import argparse
import ctypes as C
import json
import os

import numpy as np

from time_num_entropy_regular import CASES, ROOT, pieces  # (and its sys.path: the package and tests/)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cache", default=os.path.join(ROOT, "build", "time_num_entropy_regular"))
    args = ap.parse_args()

    import torch

    from torchain_amd import egs, io, synth
    from torchain_amd._lib import check, lib

    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    dev = "cuda:0"
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    device = torch.cuda.current_device()
    deriv = torch.zeros_like(y)
    lp = torch.zeros(1, dtype=torch.float64, device=dev)
    num_bytes = 256 * ((S * 8 + 255) // 256) + 256

    def switch(key, value):
        assert lib.tc_debug_set(key, value) == 0

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for case in CASES:
        sup = io.Supervision.from_synth(egs.append_supervisions(pieces(synth, args.config, args.cache, case)))
        stats = sup.stats()
        off = np.zeros((2, S + 1), np.int64)  # where each sequence's arcs and states begin
        check(lib.tc_supervision_arc_posteriors_offsets(sup.ptr, off[0].ctypes.data_as(C.c_void_p), off[1].ctypes.data_as(C.c_void_p)),
              "tc_supervision_arc_posteriors_offsets")
        switch(b"force_num_arc_post_regular_spill", 1)
        need = int(lib.tc_supervision_arc_posteriors_regular_workspace_bytes(sup.ptr))  # (the spill form's: the larger one)
        switch(b"force_num_arc_post_regular_spill", 0)
        check(min(need, 0), "tc_supervision_arc_posteriors_regular_workspace_bytes")
        ws = torch.empty(max(num_bytes, need), dtype=torch.uint8, device=dev)
        arcs = torch.zeros(int(off[0, -1]), dtype=torch.float64, device=dev)
        finals = torch.zeros(int(off[1, -1]), dtype=torch.float64, device=dev)
        elp = torch.zeros(S, dtype=torch.float64, device=dev)

        def numerator(windowed):
            switch(b"force_num_windowed", windowed)
            check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y.data_ptr()), S * T, P, y.stride(0), C.c_void_p(deriv.data_ptr()), P,
                                              C.c_void_p(lp.data_ptr()), C.c_void_p(ws.data_ptr()), num_bytes, device,
                                              C.c_void_p(stream)), "tc_num_forward_backward")
            switch(b"force_num_windowed", 0)

        def occupations(spill):
            switch(b"force_num_arc_post_regular_spill", spill)
            check(lib.tc_supervision_arc_posteriors_regular(sup.ptr, C.c_void_p(y.data_ptr()), 0, 0, S * T, P, y.stride(0),
                                                            C.c_void_p(arcs.data_ptr()), C.c_void_p(finals.data_ptr()),
                                                            C.c_void_p(elp.data_ptr()), C.c_void_p(ws.data_ptr()), need, device,
                                                            C.c_void_p(stream)), "tc_supervision_arc_posteriors_regular")
            switch(b"force_num_arc_post_regular_spill", 0)

        calls = {"numerator": lambda: numerator(0), "numerator_windowed": lambda: numerator(1),
                 "arc_post": lambda: occupations(0), "arc_post_spill": lambda: occupations(1)}
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        deriv.zero_()
        numerator(1)
        occupations(0)
        torch.cuda.synchronize()
        assert abs(float(elp.sum()) - float(lp[0])) <= 1e-9 * abs(float(lp[0]))  # (weight 1: the numerator's log Z)
        assert abs(float(arcs.sum()) - S * T) <= 1e-5 * S * T
        rounds = {k: [] for k in calls}
        for _ in range(args.rounds):
            times = {k: [] for k in calls}
            for _ in range(args.iters):  # (the entries take turns)
                for k, fn in calls.items():
                    times[k].append(timed(fn))
            for k, v in times.items():
                rounds[k].append(sorted(v)[len(v) // 2])
        row = dict(config=args.config, case=case, S=S, T=T, P=P, rounds=args.rounds, iters=args.iters, kernel=stats["kernel"],
                   arcs=int(off[0, -1]), max_level_states=stats["max_level_states"], max_level_arcs=stats["max_level_arcs"],
                   form=sup.arc_posteriors_kernel(), workspace_mb=round(need / 2 ** 20, 2))
        for k, v in rounds.items():
            row.update({k + "_ms": round(sorted(v)[len(v) // 2], 4), k + "_ms_range": [round(min(v), 4), round(max(v), 4)]})
        print(json.dumps(row), flush=True)
    print(json.dumps({k: int(lib.tc_debug_counter(k.encode())) for k in ("num_arc_post_regular_launches",
                                                                         "num_arc_post_regular_spill_launches", "num_windowed_launches")}),
          flush=True)


if __name__ == "__main__":
    main()
