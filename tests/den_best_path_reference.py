"""Float64 reference of the best path through a denominator graph (``io.DenominatorGraph.best_path`` / ``tc_den_best_path``).
A helper, not a test module; plain numpy, no GPU.

The stated arithmetic in float64.  The score of a path of states ``h_0 .. h_T`` joined by arcs ``a_1 .. a_T`` of an FST of
``torchain_amd.synth`` is

    log pi(h_0) + sum_{t = 1 .. T} ( log w(a_t) + y[t - 1, pdf(a_t)] )

with ``pi`` the graph's initial probabilities (``io.DenominatorGraph.initial_probs()``), every state final at cost 0 and
``y`` as it is.  ``log w`` and ``log pi`` are the library's table entries: the float64 logarithm of the float32 probability
the graph holds (``exp(-weight)`` rounded to float32, as the denominator takes it), rounded to float32 once.  Everything
after that -- every sum and every comparison -- is float64 here, where the kernel's are float32.
"""
import numpy as np


def tables(fst, initial_probs):
    """``(logw, logpi)``: float64 arrays holding the float32 table entries (``-inf`` for a probability of 0)."""
    prob = np.exp(-fst.weight.astype(np.float64)).astype(np.float32)
    with np.errstate(divide="ignore"):
        logw = np.log(prob.astype(np.float64)).astype(np.float32).astype(np.float64)
        logpi = np.log(np.asarray(initial_probs, np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    return logw, logpi


def viterbi(fst, initial_probs, y):
    """``(states, pdfs, score)`` of one best path under ``y`` (``(T, P)``): int arrays of ``T + 1`` and ``T`` entries and a
    float64.  Among equal scores: the lowest last state, then the first in-arc in the FST's arc order (the library's rule,
    though float64 and float32 ties need not coincide)."""
    logw, logpi = tables(fst, initial_probs)
    y = np.asarray(y, np.float64)
    T, H = y.shape[0], fst.num_states
    pdf = fst.ilabel.astype(np.int64) - 1
    src, dst = fst.src.astype(np.int64), fst.dst.astype(np.int64)
    order = np.argsort(dst, kind="stable")  # in-arcs of a state in arc-list order
    score = np.full((T + 1, H), -np.inf)
    back = np.full((T + 1, H), -1, np.int64)
    score[0] = logpi
    for t in range(1, T + 1):
        cand = score[t - 1, src] + (logw + y[t - 1, pdf])
        np.maximum.at(score[t], dst, cand)
        rev = order[::-1]  # (of duplicate indices the last assignment stays: the first arc in arc-list order)
        rev = rev[(cand[rev] == score[t, dst[rev]]) & (cand[rev] > -np.inf)]
        back[t, dst[rev]] = rev
    h = int(np.argmax(score[T]))
    best = float(score[T, h])
    states, pdfs = np.full(T + 1, -1, np.int64), np.full(T, -1, np.int64)
    if best == -np.inf:
        return states, pdfs, best
    for t in range(T, 0, -1):
        states[t] = h
        a = back[t, h]
        pdfs[t - 1] = pdf[a]
        h = int(src[a])
    states[0] = h
    return states, pdfs, best


def rescore(fst, initial_probs, states, pdfs, y, running=False):
    """The float64 score of the path ``states`` / ``pdfs`` (``T + 1`` and ``T`` entries) under ``y``; ``-inf`` when it is no
    path of the FST (a consecutive pair without an arc of that pdf, or ``pi(h_0) == 0``).  Of parallel arcs of one pdf the
    strongest counts.  ``running``: ``(score, M)`` with ``M`` the largest running ``|score|`` along the path."""
    logw, logpi = tables(fst, initial_probs)
    y = np.asarray(y, np.float64)
    pdf = fst.ilabel.astype(np.int64) - 1
    total = logpi[int(states[0])]
    peak = abs(total)
    for t in range(1, len(states)):
        arcs = np.nonzero((fst.src == states[t - 1]) & (fst.dst == states[t]) & (pdf == pdfs[t - 1]))[0]
        step = max((logw[a] for a in arcs), default=-np.inf)
        total = total + (step + y[t - 1, int(pdfs[t - 1])])
        peak = max(peak, abs(total))
    return (float(total), float(peak)) if running else float(total)


def bound(T, peak):
    """The library's stated bound on a float32 score: ``T * 2^-23 * M``."""
    return T * 2.0 ** -23 * peak


def brute_force(fst, initial_probs, y):
    """``(best score, set of (states, pdfs) that reach it)`` by enumeration of every start state and every arc sequence."""
    logw, logpi = tables(fst, initial_probs)
    y = np.asarray(y, np.float64)
    T = y.shape[0]
    pdf = fst.ilabel.astype(np.int64) - 1
    out_arcs = [np.nonzero(fst.src == h)[0] for h in range(fst.num_states)]
    best, arg = -np.inf, set()

    def walk(h, t, total, states, pdfs):
        nonlocal best, arg
        if t == T:
            if total > best:
                best, arg = total, set()
            if total == best and total > -np.inf:
                arg.add((tuple(states), tuple(pdfs)))
            return
        for a in out_arcs[h]:
            walk(int(fst.dst[a]), t + 1, total + (logw[a] + y[t, pdf[a]]), states + [int(fst.dst[a])], pdfs + [int(pdf[a])])

    for h0 in range(fst.num_states):
        if logpi[h0] > -np.inf:
            walk(h0, 0, logpi[h0], [h0], [])
    return float(best), arg


def random_path(fst, initial_probs, T, rng):
    """A random path of ``T`` arcs from a state with ``pi > 0``: ``(states, pdfs)``."""
    starts = np.nonzero(np.asarray(initial_probs) > 0)[0]
    while True:
        h = int(rng.choice(starts))
        states, pdfs = [h], []
        for _ in range(T):
            arcs = np.nonzero(fst.src == h)[0]
            if len(arcs) == 0:
                break
            a = int(rng.choice(arcs))
            h = int(fst.dst[a])
            states.append(h)
            pdfs.append(int(fst.ilabel[a]) - 1)
        if len(pdfs) == T:
            return np.array(states), np.array(pdfs)


def runner_up(fst, initial_probs, y, states, pdfs):
    """The best float64 score of any path that differs from ``(states, pdfs)``: a Viterbi over (state, still on the given
    path or not)."""
    logw, logpi = tables(fst, initial_probs)
    y = np.asarray(y, np.float64)
    T, H = y.shape[0], fst.num_states
    pdf = fst.ilabel.astype(np.int64) - 1
    src, dst = fst.src.astype(np.int64), fst.dst.astype(np.int64)
    off = np.array(logpi)  # best score of a prefix that has left the given path
    off[int(states[0])] = -np.inf
    on = logpi[int(states[0])]
    for t in range(1, T + 1):
        step = logw + y[t - 1, pdf]
        on_arc = (src == states[t - 1]) & (dst == states[t]) & (pdf == pdfs[t - 1])
        new = np.full(H, -np.inf)
        np.maximum.at(new, dst, off[src] + step)
        leave = (src == states[t - 1]) & ~on_arc  # arcs that leave the path here
        if leave.any():
            np.maximum.at(new, dst[leave], on + step[leave])
        # parallel arcs of the path's own pdf and pair: the strongest is the path, the others tie with or lose to it
        on = on + step[on_arc].max()
        off = new
    return float(off.max())
