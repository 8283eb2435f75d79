"""What the alignment entropy of a regular supervision costs (``tc_supervision_path_entropy_regular``): the value alone (the
kernel's forward pass) and the value with its gradient, beside the numerator's forward-backward (``tc_num_forward_backward``
with a derivative) on the same handle, at a config's shape (C3: 256 x 150, 4096 pdfs), on three supervisions built piece by
piece and merged (``egs.append_supervisions``):

    trie3    three paths a sequence (``synth.random_supervision``)
    trie40   forty paths a sequence
    lattice  lattice-like, 30-60 states a level (``tests/wide_supervisions.py: lattice_supervision``)

and, where the pieces fit it (about 5000 states a sequence), the same acceptors handed to ``from_e2e_fsts`` and
``tc_supervision_path_entropy``, which walks every state at every frame.

All entries take the 2-D float32 output and write a (T*S, P) float32 matrix where they write one.  ``--rounds`` rounds; in a
round the entries take turns, ``--iters`` timed calls of each, device events around every call, the round's figure the median;
one JSON line per supervision with the median of the rounds' medians and the smallest and largest of them.  The pieces are kept
as .npz files in ``--cache`` (built where missing: host work only, a minute or two at C3).

    python scripts/time_num_entropy_regular.py [--config C3] [--rounds 5] [--iters 10] [--warmup 5] [--cache DIR] [--build-only]
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
CASES = ("trie3", "trie40", "lattice")
E2E_MAX_STATES = 5000


def pieces(synth, config, cache, case):
    """the case's S single-sequence supervisions, from the cache or built into it"""
    import wide_supervisions as ws
    cfg = synth.CONFIGS[config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    path = os.path.join(cache, "entropy_regular_%s_%s.npz" % (config, case))
    if not os.path.exists(path):
        if case == "lattice":
            made = [ws.lattice_supervision(1, T, P, lambda q, t, r: r.integers(30, 61), 2, seed=5 + s, final_weights=True)
                    for s in range(S)]
        else:
            fst = synth.config_den_fst(config)
            pi = synth.initial_probs_f64(fst)
            made = [synth.random_supervision(fst, 1, T, int(case[4:]), seed=3 + s, initial_probs=pi) for s in range(S)]
        os.makedirs(cache, exist_ok=True)
        np.savez_compressed(path, **{"%s_%d" % (f, s): np.asarray(getattr(p, f)) for s, p in enumerate(made) for f in p._fields})
    z = np.load(path)
    out = []
    for s in range(S):
        v = {f: z["%s_%d" % (f, s)] for f in synth.SupFst._fields}
        out.append(synth.SupFst(float(v["weight"]), 1, T, P, int(v["num_states"]), v["arc_begin"], v["ilabel"], v["arc_weight"],
                                v["nextstate"], v["final"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cache", default=os.path.join(ROOT, "build", "time_num_entropy_regular"))
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()

    from torchain_amd import egs, io, synth

    if args.build_only:
        for case in CASES:
            pieces(synth, args.config, args.cache, case)
        return

    import torch

    from torchain_amd._lib import check, lib

    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    dev = "cuda:0"
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    device = torch.cuda.current_device()
    out = torch.zeros_like(y)  # the numerator's derivative / the entropy's gradient
    lp = torch.zeros(1, dtype=torch.float64, device=dev)
    ent, elp = (torch.zeros(S, dtype=torch.float64, device=dev) for _ in range(2))
    num_bytes = 256 * ((S * 8 + 255) // 256) + 256

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for case in CASES:
        made = pieces(synth, args.config, args.cache, case)
        sup = io.Supervision.from_synth(egs.append_supervisions(made))
        stats = sup.stats()
        handles = {"": (sup, "tc_supervision_path_entropy_regular")}
        if max(p.num_states for p in made) <= E2E_MAX_STATES:
            fsts = [(0, p.arc_begin, p.ilabel, p.arc_weight, p.nextstate, p.final) for p in made]
            handles["e2e_"] = (io.Supervision.from_e2e_fsts(1.0, T, P, fsts, any_size=True), "tc_supervision_path_entropy")
        need = {}
        for k, (h, name) in handles.items():
            need[k] = int(getattr(lib, name + "_workspace_bytes")(h.ptr, 1))
            check(min(need[k], 0), name + "_workspace_bytes")
        ws = torch.empty(max([num_bytes] + list(need.values())), dtype=torch.uint8, device=dev)

        def numerator():
            check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y.data_ptr()), S * T, P, y.stride(0), C.c_void_p(out.data_ptr()), P,
                                              C.c_void_p(lp.data_ptr()), C.c_void_p(ws.data_ptr()), num_bytes, device,
                                              C.c_void_p(stream)), "tc_num_forward_backward")

        def entropy(k, grad):
            h, name = handles[k]
            check(getattr(lib, name)(h.ptr, C.c_void_p(y.data_ptr()), 0, 0, S * T, P, y.stride(0), C.c_void_p(ent.data_ptr()),
                                     C.c_void_p(elp.data_ptr()), C.c_void_p(out.data_ptr()) if grad else None, P, None,
                                     C.c_void_p(ws.data_ptr()) if grad else None, need[k] if grad else 0, device,
                                     C.c_void_p(stream)), name)

        calls = {"numerator": numerator}
        for k in handles:
            calls[k + "entropy_value"] = lambda k=k: entropy(k, False)
            calls[k + "entropy_value_grad"] = lambda k=k: entropy(k, True)
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        numerator()
        entropy("", True)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ent).all()) and bool((ent >= 0).all())
        assert abs(float(elp.sum()) - float(lp[0])) <= 1e-9 * abs(float(lp[0]))  # (weight 1: the numerator's log Z)
        rounds = {k: [] for k in calls}
        for _ in range(args.rounds):
            times = {k: [] for k in calls}
            for _ in range(args.iters):  # (the entries take turns)
                for k, fn in calls.items():
                    times[k].append(timed(fn))
            for k, v in times.items():
                rounds[k].append(sorted(v)[len(v) // 2])
        row = dict(config=args.config, case=case, S=S, T=T, P=P, rounds=args.rounds, iters=args.iters, kernel=stats["kernel"],
                   max_states=stats["max_states"], max_level_states=stats["max_level_states"], max_level_arcs=stats["max_level_arcs"],
                   history_mb=round(need[""] / 2 ** 20, 2), mean_entropy=round(float(ent.mean()), 3))
        if "e2e_" in need:
            row["e2e_history_mb"] = round(need["e2e_"] / 2 ** 20, 2)
        for k, v in rounds.items():
            row.update({k + "_ms": round(sorted(v)[len(v) // 2], 4), k + "_ms_range": [round(min(v), 4), round(max(v), 4)]})
        print(json.dumps(row), flush=True)
    print(json.dumps({k: int(lib.tc_debug_counter(k.encode())) for k in ("num_entropy_regular_launches", "num_entropy_launches")}),
          flush=True)


if __name__ == "__main__":
    main()
