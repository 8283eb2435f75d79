"""Plain-Python float64 restatement of ``tc_den_compose`` (``io.DenominatorGraph.normalize_fsts``): a helper, not a test
module.  It shares no code with ``csrc/den_compose.cpp``: dictionaries and lists, one state at a time.

The normalization acceptor N of a graph: the states of den.fst plus a start ``q0``; every arc ``h -> h'`` (pdf ``p``,
probability ``w``) at cost ``-log w``; for every ``h`` with ``pi(h) > 0`` and every arc ``h -> h'`` an arc ``q0 -> h'`` with label
``p`` at cost ``-log pi(h) - log w``; every state final at cost 0.  ``pi`` and ``w`` are the HANDLE's float32 values
(``initial_probs()``, ``arcs()``), so that only the logarithm's last bit can differ between this file and the library; an
arc with ``w == 0`` is left out.

The product with a supervision acceptor: start ``(s_0, q0)``, arcs ``(s, h) --p--> (s', h')`` at cost
``float32(float64(c_sup) + scale * c_N)``, final cost that of ``s``, trimmed.  The order: breadth-first from the start, states
in increasing new id, their supervision arcs in input order, for each the matching arcs of N in the order the handle keeps
the graph's arcs (``q0``: ``h`` ascending, then its arcs), a new state gets the next id when first reached, trimming keeps
the relative order.  ``max_states`` bounds the states before trimming.

FSTs are the tuples of ``io.Supervision.from_fsts`` -- ``(arc_begin, ilabel, arc_weight, nextstate, final)`` -- or, end-to-end,
``from_e2e_fsts`` -- ``(start, arc_begin, ...)``.  Importing this module needs no GPU."""
import itertools
import math

import numpy as np

OK, EMPTY, TOO_LARGE = 0, 1, 2


class NormFst:
    """N as ``out[h]`` = list of ``(pdf, h', cost)`` in order, ``h == H`` being ``q0``."""

    def __init__(self, graph):
        src, dst, pdf, prob = graph.arcs()
        pi = graph.initial_probs()
        self.H = H = int(graph.num_states)
        assert (np.diff(src) >= 0).all()  # state-major: "h ascending, then its arcs" is the arc list's own order
        self.out = [[] for _ in range(H + 1)]
        for a in range(len(src)):
            if not prob[a] > 0:
                continue
            self.out[int(src[a])].append((int(pdf[a]), int(dst[a]), -math.log(float(prob[a]))))
        for a in range(len(src)):
            p = float(pi[src[a]])
            if not prob[a] > 0 or not p > 0:
                continue
            self.out[H].append((int(pdf[a]), int(dst[a]), -math.log(p) - math.log(float(prob[a]))))


def _parts(fst, e2e):
    start, rest = (int(fst[0]), fst[1:]) if e2e else (0, fst)
    ab, il, aw, nx, fin = (np.asarray(x) for x in rest)
    return start, ab, il, aw, nx, fin


def compose(norm, fst, e2e=False, scale=1.0, max_states=200000):
    """``(fst_out or None, status)``: one sequence."""
    start, ab, il, aw, nx, fin = _parts(fst, e2e)
    ids = {(start, norm.H): 0}
    states = [(start, norm.H)]
    arcs = []  # per state: list of (label, next id, float32 cost)
    q = 0
    while q < len(states):
        s, h = states[q]
        mine = []
        for a in range(int(ab[s]), int(ab[s + 1])):
            for pdf, h2, c in norm.out[h]:
                if pdf != int(il[a]) - 1:
                    continue
                key = (int(nx[a]), h2)
                if key not in ids:
                    if len(states) >= max_states:
                        return None, TOO_LARGE
                    ids[key] = len(states)
                    states.append(key)
                mine.append((int(il[a]), ids[key], np.float32(np.float64(aw[a]) + np.float64(scale) * np.float64(c))))
        arcs.append(mine)
        q += 1
    # trim: states from which a final state is reached (all are reachable)
    alive = [bool(np.isfinite(fin[s])) for s, _ in states]
    changed = True
    while changed:
        changed = False
        for i in range(len(states) - 1, -1, -1):
            if not alive[i] and any(alive[n] for _, n, _ in arcs[i]):
                alive[i] = changed = True
    if not alive[0]:
        return None, EMPTY
    new = {}
    for i in range(len(states)):
        if alive[i]:
            new[i] = len(new)
    o_ab, o_il, o_aw, o_nx, o_fin = [0], [], [], [], []
    for i in range(len(states)):
        if not alive[i]:
            continue
        for lab, n, c in arcs[i]:
            if alive[n]:
                o_il.append(lab), o_aw.append(c), o_nx.append(new[n])
        o_ab.append(len(o_il))
        o_fin.append(fin[states[i][0]])
    out = (np.array(o_ab, np.int32), np.array(o_il, np.int32), np.array(o_aw, np.float32), np.array(o_nx, np.int32),
           np.array(o_fin, np.float32))
    return ((0,) + out if e2e else out), OK


def normalize(graph, fsts, e2e=False, scale=1.0, max_states=200000):
    """``(list of FSTs or None, list of statuses)``."""
    norm = NormFst(graph)
    res = [compose(norm, f, e2e, scale, max_states) for f in fsts]
    return [r[0] for r in res], [r[1] for r in res]


# ---- path weights by enumeration -------------------------------------------------------------------------------------------
def path_logsum(fst, labels, e2e=False):
    """Log of the sum over the FST's paths that read ``labels`` (1-based) of exp(-cost), final costs included; -inf: none.
    float64, a forward pass over state sets."""
    start, ab, il, aw, nx, fin = _parts(fst, e2e)
    cur = {start: 0.0}
    for lab in labels:
        nxt = {}
        for s, lp in cur.items():
            for a in range(int(ab[s]), int(ab[s + 1])):
                if int(il[a]) == lab and np.isfinite(aw[a]):
                    nxt.setdefault(int(nx[a]), []).append(lp - float(aw[a]))
        cur = {s: _lse(v) for s, v in nxt.items()}
    return _lse([lp - float(fin[s]) for s, lp in cur.items() if np.isfinite(fin[s])])


def norm_logsum(norm, labels, scale=1.0):
    """The same for N with its costs times ``scale`` (every state final at 0)."""
    cur = {norm.H: 0.0}
    for lab in labels:
        nxt = {}
        for h, lp in cur.items():
            for pdf, h2, c in norm.out[h]:
                if pdf == lab - 1:
                    nxt.setdefault(h2, []).append(lp - scale * c)
        cur = {h: _lse(v) for h, v in nxt.items()}
    return _lse(list(cur.values()))


def _lse(v):
    v = [x for x in v if x != -math.inf]
    if not v:
        return -math.inf
    m = max(v)
    return m + math.log(sum(math.exp(x - m) for x in v))


def label_sequences(num_pdfs, T):
    return itertools.product(range(1, num_pdfs + 1), repeat=T)


def on_accepted_path(fst, e2e=False):
    """Whether every state of the FST is reachable from the start and reaches a final state."""
    start, ab, il, aw, nx, fin = _parts(fst, e2e)
    n = len(fin)
    fwd = {start}
    stack = [start]
    while stack:
        s = stack.pop()
        for a in range(int(ab[s]), int(ab[s + 1])):
            if int(nx[a]) not in fwd:
                fwd.add(int(nx[a])), stack.append(int(nx[a]))
    alive = [bool(np.isfinite(fin[s])) for s in range(n)]
    changed = True
    while changed:
        changed = False
        for s in range(n):
            if not alive[s] and any(alive[int(nx[a])] for a in range(int(ab[s]), int(ab[s + 1]))):
                alive[s] = changed = True
    return len(fwd) == n and all(alive)


# ---- synthetic supervisions without the graph's weights ---------------------------------------------------------------------
def union_of_paths(paths, final_costs=None, cost=None):
    """A time-unfolded trie acceptor of equal-length label paths (1-based labels), states in time order, state 0 the start:
    the tuple ``from_fsts`` takes.  ``cost(t, label)`` gives an arc's cost (default 0); ``final_costs``: one per distinct leaf."""
    T = len(paths[0])
    assert all(len(p) == T for p in paths)
    levels = [{(): 0}]
    for t in range(T):
        lv = {}
        for p in paths:
            lv.setdefault(tuple(p[:t + 1]), len(lv))
        levels.append(lv)
    base = np.concatenate([[0], np.cumsum([len(lv) for lv in levels])])
    n = int(base[-1])
    out = [[] for _ in range(n)]
    for t in range(T):
        for pre, i in levels[t + 1].items():
            out[base[t] + levels[t][pre[:-1]]].append((pre[-1], 0.0 if cost is None else float(cost(t, pre[-1])), base[t + 1] + i))
    ab, il, aw, nx = [0], [], [], []
    for lst in out:
        for lab, c, d in lst:
            il.append(lab), aw.append(c), nx.append(d)
        ab.append(len(il))
    final = np.full(n, np.inf, np.float32)
    leaves = len(levels[T])
    final[base[T]:] = 0.0 if final_costs is None else np.asarray(final_costs, np.float32)[:leaves]
    return (np.array(ab, np.int32), np.array(il, np.int32), np.array(aw, np.float32), np.array(nx, np.int32), final)


def graph_path(fst, T, rng):
    """Labels (1-based) of a random path of T arcs through a ``synth.DenFst``, from a random state."""
    h = int(rng.integers(0, fst.num_states))
    labels = []
    for _ in range(T):
        arcs = np.flatnonzero(fst.src == h)
        a = int(arcs[rng.integers(0, len(arcs))])
        labels.append(int(fst.ilabel[a]))
        h = int(fst.dst[a])
    return labels


def strip_weights(sup):
    """A single-sequence ``synth.SupFst`` as the ``from_fsts`` tuple with every arc and final cost set to 0."""
    return (np.asarray(sup.arc_begin, np.int32), np.asarray(sup.ilabel, np.int32), np.zeros(len(sup.ilabel), np.float32),
            np.asarray(sup.nextstate, np.int32), np.where(np.isfinite(sup.final), 0.0, np.inf).astype(np.float32))
