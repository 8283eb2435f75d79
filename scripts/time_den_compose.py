"""What putting the denominator graph's weights on caller-built supervisions costs on the host
(``io.DenominatorGraph.normalize_fsts`` -> ``tc_den_compose``), and how much the supervisions grow, at a config's shape
(C3: 256 sequences x 150 frames, 4096 pdfs, 8192 states / 65536 arcs), for four minibatches whose FSTs carry no weights:

    trie3     three paths a sequence (``synth.random_supervision`` with its costs stripped)
    trie40    40 paths a sequence, the same way
    e2e       end-to-end acceptors of the ``chain`` shape of scripts/time_e2e.py -- one state per phone, entered on its
              forward pdf, looping on its self-loop pdf, about one phone per 4 frames -- along random walks through the
              graph (time_e2e.py's own batch draws its pdfs at random: none of its paths is in the graph)
    linear    one alignment a sequence (what ``Supervision.from_alignments`` builds)

No GPU is touched.  ``--iters`` timed calls after one warm-up call, wall clock around the whole Python call (concatenating
the inputs, the library's composition, splitting the outputs); per case one JSON line: median and minimum in ms per
minibatch, the library call alone, states and arcs before and after (sums over the minibatch, and the largest sequence), the
statuses, and which numerator the composed minibatch takes (``Supervision.stats()``; end-to-end: whether it fits the limits).

    python scripts/time_den_compose.py [--config C3] [--iters 5] [--sequences N]
"""
import argparse
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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sequences", type=int, default=0, help="0: the config's")
    args = ap.parse_args()

    import den_compose_reference as dr
    from torchain_amd import io, synth
    from torchain_amd._lib import lib

    cfg = synth.CONFIGS[args.config]
    S, T, P = args.sequences or cfg["S"], cfg["T"], cfg["P"]
    t0 = time.time()
    fst = synth.config_den_fst(args.config)
    g = io.DenominatorGraph(fst, P)
    pi = g.initial_probs()
    rng = np.random.default_rng(0)
    first = np.searchsorted(fst.src, np.arange(fst.num_states + 1))

    def walk_fst():
        """one state per phone along a random walk over the graph's non-self-loop arcs, each looping on its self-loop pdf"""
        h = int(rng.integers(0, fst.num_states))
        arcs, n = [], 1
        for _ in range(max(1, T // 4)):
            out = np.arange(first[h], first[h + 1])
            fwd = out[fst.dst[out] != h]
            a = int(fwd[rng.integers(0, len(fwd))])
            h = int(fst.dst[a])
            out = np.arange(first[h], first[h + 1])
            loop = out[fst.dst[out] == h]
            arcs.append((n - 1, n, int(fst.ilabel[a])))
            if len(loop):
                arcs.append((n, n, int(fst.ilabel[loop[0]])))
            n += 1
        arcs.sort(key=lambda x: x[0])
        ab = np.concatenate([[0], np.cumsum(np.bincount([x[0] for x in arcs], minlength=n))]).astype(np.int32)
        final = np.full(n, np.inf, np.float32)
        final[n - 1] = 0.0
        return (0, ab, np.array([x[2] for x in arcs], np.int32), np.zeros(len(arcs), np.float32),
                np.array([x[1] for x in arcs], np.int32), final)

    cases = {
        "trie3": (False, [dr.strip_weights(synth.random_supervision(fst, 1, T, 3, seed=3 + s, initial_probs=pi)) for s in range(S)]),
        "trie40": (False, [dr.strip_weights(synth.random_supervision(fst, 1, T, 40, seed=3 + s, initial_probs=pi)) for s in range(S)]),
        "e2e": (True, [walk_fst() for _ in range(S)]),
        "linear": (False, [dr.union_of_paths([dr.graph_path(fst, T, rng)]) for _ in range(S)]),
    }
    print("# graph and supervisions ready in %.1f s" % (time.time() - t0), flush=True)

    real = lib.tc_den_compose
    inner = []

    def timed_compose(*a):
        t = time.perf_counter()
        rc = real(*a)
        inner.append((time.perf_counter() - t) * 1e3)
        return rc

    lib.tc_den_compose = timed_compose
    for case, (e2e, fsts) in cases.items():
        outs, info = g.normalize_fsts(fsts, e2e=e2e)
        del inner[:]
        times = []
        for _ in range(args.iters):
            t = time.perf_counter()
            outs, info = g.normalize_fsts(fsts, e2e=e2e)
            times.append((time.perf_counter() - t) * 1e3)
        ok = [o for o in outs if o is not None]
        row = dict(config=args.config, case=case, sequences=S, frames=T, iters=args.iters,
                   ms_median=round(sorted(times)[len(times) // 2], 2), ms_min=round(min(times), 2),
                   library_ms_median=round(sorted(inner)[len(inner) // 2], 2),
                   status=[int((info["status"] == k).sum()) for k in (0, 1, 2)],
                   states_in=int(info["states_in"].sum()), states_out=int(info["states_out"].sum()),
                   arcs_in=int(info["arcs_in"].sum()), arcs_out=int(info["arcs_out"].sum()),
                   max_states_in=int(info["states_in"].max()), max_states_out=int(info["states_out"].max()),
                   max_arcs_in=int(info["arcs_in"].max()), max_arcs_out=int(info["arcs_out"].max()))
        row["states_growth"] = round(row["states_out"] / max(1, row["states_in"]), 3)
        row["arcs_growth"] = round(row["arcs_out"] / max(1, row["arcs_in"]), 3)
        if e2e:
            row["fits_e2e_limits"] = bool(row["max_states_out"] <= 2048 and row["max_arcs_out"] <= 8192)
        elif len(ok) == S:
            before = io.Supervision.from_fsts(1.0, [T] * S, P, fsts).stats()["kernel"]
            row["numerator"] = "%s -> %s" % (before, io.Supervision.from_fsts(1.0, [T] * S, P, outs).stats()["kernel"])
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
