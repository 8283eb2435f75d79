"""Numerator supervisions around and beyond the resident numerator kernel's limit (a helper, not a test module).

``csrc/num_kernels.hip`` keeps a whole sequence in LDS: ``16 * states + 4 * arcs + 4 * unique (frame, pdf)`` bytes, at most
160 KB.  Sequences beyond that take the level-windowed kernel (``csrc/num_windowed_kernels.hip``), whose LDS is sized by the
widest time level.  Here: the trie cases (``synth.random_supervision`` with many paths or many frames), a lattice-like generator
whose states have several in-arcs and whose (frame, pdf) entries sum many arcs, and a plain-numpy count of the quantities
``io.Supervision.stats()`` reports, taken from the merged FST alone."""
import functools

import numpy as np

from torchain_amd import synth

P = 200
LDS_LIMIT = 160 * 1024
RESIDENT, WINDOWED = "resident", "windowed"


@functools.lru_cache(maxsize=None)
def den_fst():
    return synth.random_den_fst(300, 6, P, seed=3)


# name -> (sequences, frames, paths per sequence, final weights, expected kernel)
TRIE = {
    "trie_150x3": (2, 150, 3, False, RESIDENT),
    "trie_150x40": (2, 150, 40, True, RESIDENT),
    "trie_150x64": (2, 150, 64, False, WINDOWED),
    "trie_600x16": (2, 600, 16, True, WINDOWED),
    "trie_1500x8": (2, 1500, 8, False, WINDOWED),
    "trie_3000x4": (2, 3000, 4, False, WINDOWED),
}


def lattice_supervision(S, T, num_pdfs, width, fan, seed, weight=1.0, final_weights=False):
    """Per sequence a layered DAG: level 0 is one root, level t >= 1 has ``width(q, t, rng)`` states; every state of level
    t + 1 has at least one in-arc, every state of level t at least one and up to ``fan`` + 1 out-arcs, so arcs merge; four in
    five arcs of a frame draw their pdf from 24, so a (frame, pdf) entry sums many occupations.  The sequences are merged the
    way ``synth.random_supervision`` merges them: every final state of sequence q - 1 carries a copy of sequence q's start
    arcs, with the final weight of that state folded in when ``final_weights``."""
    rng = np.random.default_rng(seed)
    seq_nodes, seq_arcs = [], []
    for q in range(S):
        nodes = [1] + [int(width(q, t, rng)) for t in range(1, T + 1)]
        arcs_by_t = []
        for t in range(T):
            n0, n1 = nodes[t], nodes[t + 1]
            pairs = set(zip(rng.integers(n0, size=n1).tolist(), range(n1)))  # every destination is reached
            for a in range(n0):                                              # every source leaves
                for b in rng.integers(n1, size=int(rng.integers(1, fan + 1))).tolist():
                    pairs.add((a, b))
            pairs = sorted(pairs)
            few = rng.integers(1, min(num_pdfs, 24) + 1, size=len(pairs))
            any_ = rng.integers(1, num_pdfs + 1, size=len(pairs))
            pdf = np.where(rng.random(len(pairs)) < 0.8, few, any_)
            w = rng.uniform(0.0, 3.0, size=len(pairs))
            arcs_by_t.append([(a, b, int(pdf[i]), float(w[i])) for i, (a, b) in enumerate(pairs)])
        seq_nodes.append(nodes)
        seq_arcs.append(arcs_by_t)
    state_base, n = [], 0
    for q in range(S):
        bases = []
        for t in range(T + 1):
            if t == 0 and q > 0:
                bases.append(state_base[q - 1][T])
                continue
            bases.append(n)
            n += seq_nodes[q][t]
        state_base.append(bases)
    num_states = n
    fw = [rng.uniform(0.1, 2.0, size=seq_nodes[q][T]) if final_weights else np.zeros(seq_nodes[q][T]) for q in range(S)]
    out = [[] for _ in range(num_states)]
    for q in range(S):
        for t in range(T):
            for (a, b, il, w) in seq_arcs[q][t]:
                dst = state_base[q][t + 1] + b
                if t == 0 and q > 0:
                    for f in range(seq_nodes[q - 1][T]):
                        out[state_base[q][0] + f].append((il, w + float(fw[q - 1][f]), dst))
                else:
                    out[state_base[q][t] + a].append((il, w, dst))
    arc_begin = np.zeros(num_states + 1, np.int32)
    il_, aw, nx = [], [], []
    for i, lst in enumerate(out):
        arc_begin[i + 1] = arc_begin[i] + len(lst)
        for (il, w, d) in lst:
            il_.append(il)
            aw.append(w)
            nx.append(d)
    final = np.full(num_states, np.inf, np.float32)
    final[state_base[S - 1][T]: state_base[S - 1][T] + seq_nodes[S - 1][T]] = fw[S - 1]
    return synth.SupFst(float(weight), S, T, num_pdfs, num_states, arc_begin, np.array(il_, np.int32),
                        np.array(aw, np.float32), np.array(nx, np.int32), final)


EDGE_WIDTHS = (63, 64, 65, 127, 128, 129, 1)

# name -> (sequences, frames, width(q, t, rng), fan, final weights, supervision weight, expected kernel)
LATTICE = {
    "lattice_fits": (3, 60, lambda q, t, r: r.integers(20, 41), 3, True, 1.0, RESIDENT),
    "lattice_bursty": (2, 150, lambda q, t, r: 400 if t % 50 == 25 else r.integers(2, 12), 2, True, 1.0, RESIDENT),
    "lattice_wide": (3, 150, lambda q, t, r: r.integers(40, 121), 3, True, 0.75, WINDOWED),
    "lattice_long": (2, 1200, lambda q, t, r: r.integers(8, 25), 2, False, 1.0, WINDOWED),
    # an empty-ish extreme: one level of a single state between levels of 60-100
    "lattice_pinch": (2, 150, lambda q, t, r: 1 if t == 70 else r.integers(60, 101), 3, False, 1.0, WINDOWED),
    # sequences of very different size in one minibatch: one wide, the rest of three states per level
    "lattice_mixed": (4, 150, lambda q, t, r: r.integers(40, 121) if q == 1 else 3, 2, True, 1.0, WINDOWED),
    # level widths either side of the kernels' lane strides (64 states a pass; 128 arcs and 128 (frame, pdf) entries a pass)
    "lattice_edge": (2, 21, lambda q, t, r: EDGE_WIDTHS[(t - 1) % len(EDGE_WIDTHS)], 3, True, 0.75, RESIDENT),
}

CASES = tuple(TRIE) + tuple(LATTICE)
FITTING = tuple(k for k in CASES if (TRIE.get(k) or LATTICE[k])[-1] == RESIDENT)
WIDE = tuple(k for k in CASES if k not in FITTING)


def expected_kernel(name):
    return (TRIE.get(name) or LATTICE[name])[-1]


@functools.lru_cache(maxsize=None)
def supervision(name):
    """The case's merged supervision FST (``synth.SupFst``), built once per process."""
    if name in TRIE:
        S, T, paths, fw, _ = TRIE[name]
        return synth.random_supervision(den_fst(), S, T, paths, seed=11, final_weights=fw)
    S, T, width, fan, fw, weight, _ = LATTICE[name]
    return lattice_supervision(S, T, P, width, fan, seed=5, weight=weight, final_weights=fw)


def nnet_output(name, seed=5, scale=1.0):
    sup = supervision(name)
    return synth.random_nnet_output(sup.num_sequences, sup.frames_per_sequence, P, seed=seed, scale=scale)


def state_times(sup):
    """Time of every state of the merged FST (states are numbered in time order)."""
    times = np.full(sup.num_states, -1, np.int64)
    times[0] = 0
    ab, nx = sup.arc_begin, sup.nextstate
    for s in range(sup.num_states):
        times[nx[ab[s]:ab[s + 1]]] = times[s] + 1
    assert (times >= 0).all() and (np.diff(times) >= 0).all()
    return times


def count_stats(sup):
    """What ``io.Supervision.stats()`` reports, counted from the merged FST in numpy.  Sequence q owns the states of times
    q*T + 1 .. (q + 1)*T and one start state; its start arcs are those of the FIRST state at time q*T (the other states of
    that time carry copies); its frame t is the arcs leaving its level t."""
    S, T = sup.num_sequences, sup.frames_per_sequence
    times = state_times(sup)
    src = np.repeat(np.arange(sup.num_states), np.diff(sup.arc_begin))
    first_at = np.searchsorted(times, np.arange(S * T + 2))
    arc_time = times[src]
    own = np.ones(len(src), bool)  # drop the copies of a sequence's start arcs on all but the first boundary state
    for q in range(1, S):
        own &= ~((arc_time == q * T) & (src != first_at[q * T]))
    keys = ("max_states", "max_arcs", "max_uniq", "max_level_states", "max_level_arcs", "max_frame_uniq")
    best = dict.fromkeys(keys, 0)
    total_states = 0
    for q in range(S):
        lo, hi = q * T, (q + 1) * T
        nst = 1 + int(first_at[hi + 1] - first_at[lo + 1])
        m = own & (arc_time >= lo) & (arc_time < hi)
        t_rel, il = arc_time[m] - lo, sup.ilabel[m]
        pairs = np.unique(t_rel * (sup.label_dim + 1) + il)
        level_states = np.diff(first_at[lo:hi + 2])
        level_states[0] = 1
        got = dict(max_states=nst, max_arcs=int(m.sum()), max_uniq=len(pairs), max_level_states=int(level_states.max()),
                   max_level_arcs=int(np.bincount(t_rel).max()),
                   max_frame_uniq=int(np.bincount(pairs // (sup.label_dim + 1)).max()))
        for k in keys:
            best[k] = max(best[k], got[k])
        total_states += nst
    r4 = lambda x: (x + 3) & ~3  # noqa: E731
    r2 = lambda x: (x + 1) & ~1  # noqa: E731
    best.update(sequences=S, frames=T, history_bytes=8 * total_states,
                resident_lds_bytes=16 * r2(best["max_states"]) + 4 * r4(best["max_arcs"]) + 4 * r4(best["max_uniq"]),
                windowed_lds_bytes=32 * r2(best["max_level_states"]) + 4 * r4(best["max_level_arcs"])
                + 4 * r4(best["max_frame_uniq"]))
    best["kernel"] = RESIDENT if best["resident_lds_bytes"] <= LDS_LIMIT else WINDOWED
    return best
