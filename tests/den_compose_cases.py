"""Graphs and caller-built supervisions (no denominator weights on them) of the ``tc_den_compose`` tests: a helper, not a
test module.  ``test_den_compose_host.py`` runs them without a GPU, ``test_gpu_den_compose.py`` on one.  The float64
references of the GPU tests are here too: ``e2e_reference``'s log-semiring forward pass on the RESTATED composition
(``den_compose_reference``) beside the CPU oracle's denominator, one sequence at a time.  Nothing here is computed by the
code under test.  Importing this module needs no GPU."""
import functools

import numpy as np

from torchain_amd import io, synth

import den_compose_reference as dr
import e2e_reference as er

P = 24
LEAKY, L2 = 1e-5, 0.0
LENGTHS = (9, 7, 12, 8, 10)  # B = 5, ragged, 7 .. 12


@functools.lru_cache(maxsize=None)
def den_fst(name):
    if name == "random":
        return synth.random_den_fst(40, 4, P)
    assert name == "phone_lm"
    return synth.phone_lm_den_fst(6, 12, 3, P)


@functools.lru_cache(maxsize=None)
def graph(name):
    """One handle per graph and process (host side only; the GPU tests prepare it themselves)."""
    return io.DenominatorGraph(den_fst(name), P)


@functools.lru_cache(maxsize=None)
def oracle_graph(name):
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle.DenGraph(den_fst(name))


def small_den_fst():
    """6 states, 3 pdfs: state 0 has two arcs with label 1 (to 1 and to 2), state 5 has no in-arc and is not the start,
    so pi(5) = 0, and only state 5 can read label 3 twice in a row."""
    arcs = [(0, 1, 1, .3), (0, 2, 1, .2), (0, 0, 2, .5),
            (1, 1, 2, .4), (1, 3, 3, .6),
            (2, 3, 1, .7), (2, 2, 2, .3),
            (3, 4, 2, .5), (3, 0, 1, .5),
            (4, 4, 1, .25), (4, 0, 3, .25), (4, 1, 2, .5),
            (5, 5, 3, .5), (5, 0, 3, .5)]
    src, dst, lab, pr = (np.array([a[i] for a in arcs]) for i in range(4))
    return synth.DenFst(6, src.astype(np.int32), dst.astype(np.int32), lab.astype(np.int32),
                        (-np.log(pr)).astype(np.float32), np.zeros(6, np.float32), 0, 3)


def regular_fst(fst, rng, T=None, in_graph=None, junk=None, costs=True):
    """A union of 1 to 4 label paths of T (1 to 12) frames, ``in_graph`` of them through the graph and ``junk`` of them
    random labels; with ``costs`` random arc and final costs, else all 0."""
    T = int(rng.integers(1, 13)) if T is None else T
    k = int(rng.integers(1, 5))
    junk = int(rng.integers(0, k + 1)) if junk is None else junk
    in_graph = k - junk if in_graph is None else in_graph
    paths = [dr.graph_path(fst, T, rng) for _ in range(in_graph)]
    paths += [[int(x) for x in rng.integers(1, fst.num_pdfs + 1, size=T)] for _ in range(junk)]
    table = rng.uniform(0.0, 3.0, size=(T, fst.num_pdfs + 1))
    return dr.union_of_paths(paths, final_costs=rng.uniform(0.0, 2.0, size=len(paths)) if costs else None,
                             cost=(lambda t, lab: table[t, lab]) if costs else None), T


def e2e_fst(fst, rng, n=6, junk=3, costs=True):
    """An end-to-end acceptor with self-loops and cycles: up to ``n`` states of the graph found breadth-first from a
    random one, the graph's arcs among them (their labels, random costs), ``junk`` more arcs of random labels, random final
    costs.  The start is not state 0."""
    h0 = int(rng.integers(0, fst.num_states))
    order, seen = [h0], {h0}
    for h in order:
        for a in np.flatnonzero(fst.src == h):
            d = int(fst.dst[a])
            if d not in seen and len(order) < n:
                seen.add(d), order.append(d)
    local = {h: (i + 1) % len(order) for i, h in enumerate(order)}  # (the start becomes state 1, or 0 when alone)
    arcs = [(local[int(fst.src[a])], local[int(fst.dst[a])], int(fst.ilabel[a]) - 1, float(rng.uniform(0, 2)) if costs else 0.0)
            for a in range(len(fst.src)) if int(fst.src[a]) in local and int(fst.dst[a]) in local]
    for _ in range(junk):
        arcs.append((int(rng.integers(0, len(order))), int(rng.integers(0, len(order))), int(rng.integers(0, fst.num_pdfs)),
                     float(rng.uniform(0, 2)) if costs else 0.0))
    final = np.where(rng.random(len(order)) < 0.5, rng.uniform(0, 2, len(order)) if costs else 0.0, np.inf).astype(np.float32)
    final[local[order[-1]]] = 0.5 if costs else 0.0
    return er._csr(len(order), arcs, final, start=local[h0])


# ---- the GPU tests' batches and their float64 references ---------------------------------------------------------------------
def frame_paths(fst, lens, seed):
    """Per sequence three label paths of its length: two through the graph, the third of random labels (outside it)."""
    rng = np.random.default_rng(seed)
    out = []
    for T in lens:
        out.append([dr.graph_path(fst, T, rng), dr.graph_path(fst, T, rng),
                    [int(x) for x in rng.integers(1, fst.num_pdfs + 1, size=T)]])
    return out


def bound_batch(name, e2e, seed):
    """The bound test's supervisions at cost 0: per sequence the union of three label paths, one of them outside the graph
    -- as a time-unfolded trie, or (end-to-end) the same trie handed over as an end-to-end acceptor.  Returns (fsts, the
    paths)."""
    fst = den_fst(name)
    paths = frame_paths(fst, LENGTHS, seed)
    fsts = [dr.union_of_paths(p) for p in paths]
    if e2e:
        fsts = [(0,) + f for f in fsts]
    return fsts, paths


def nnet_output(seed, lens=LENGTHS, scale=1.0):
    T, S = max(lens), len(lens)
    return (np.random.default_rng(seed).standard_normal((T * S, P)) * scale).astype(np.float32)


def valid_rows(lens, s):
    return np.arange(int(lens[s])) * len(lens) + s


def reference(name, fsts, lens, y, weight=1.0, e2e=False):
    """The float64 objective of supervisions ``fsts`` (tuples; regular ones are taken as end-to-end acceptors starting at
    state 0 -- the same sum over paths of exactly T_s arcs), one sequence at a time: dict(objf [S], num_logprob [S],
    deriv (Tmax * S, P) with zeros in the padding, total)."""
    og = oracle_graph(name)
    S = len(lens)
    out = dict(objf=np.zeros(S), num_logprob=np.zeros(S), deriv=np.zeros(y.shape), l2_term=0.0)
    for s in range(S):
        f = fsts[s] if e2e else (0,) + tuple(fsts[s])
        rows = valid_rows(lens, s)
        one = er.e2e_objective(og, [f], int(lens[s]), y[rows], weight=weight, l2=L2, leaky=LEAKY)
        assert one["ok"], s
        out["objf"][s] = one["objf"]
        out["num_logprob"][s] = float(one["logz"][0])
        out["deriv"][rows] = one["deriv"]
    out["total"] = float(out["objf"].sum())
    out["weight"] = weight * float(sum(lens))
    return out
