"""Float64 Viterbi over one acceptor and one (T, P) score matrix: the reference of the best-path tests
(``io.Supervision.best_path`` / ``tc_supervision_best_path``).  A helper, not a test module; plain numpy, no GPU.

A path takes one arc per frame, exactly ``T`` arcs, from the start to a final state; its score is the sum over its arcs of
``y[t, pdf] - cost`` minus the final cost, all in float64 (the float32 inputs widened exactly).  The same code serves
end-to-end acceptors ``(start, arc_begin, ilabel, arc_weight, nextstate, final)`` and time-unfolded ones, which are the same
tuple without ``start`` (state 0).  Nothing here shares code or formulation with the kernels: the walk below is over arrays of
all arcs at once, by destination, with ``np.maximum.at``.

``split_merged`` cuts the merged FST of a uniform regular supervision (``synth.SupFst`` of S sequences) into its
per-sequence acceptors, for supervisions without final weights on the sequence boundaries."""
import numpy as np


def _arrays(fst):
    if len(fst) == 5:
        fst = (0,) + tuple(fst)
    start, ab, il, aw, nx, final = fst
    ab = np.asarray(ab, np.int64)
    n = len(ab) - 1
    src = np.repeat(np.arange(n), np.diff(ab))
    return (int(start), n, src, np.asarray(nx, np.int64), np.asarray(il, np.int64) - 1,
            np.asarray(aw, np.float32).astype(np.float64), np.asarray(final, np.float32).astype(np.float64))


def _walk(fst, y, pdfs):
    start, n, src, dst, pdf, cost, final = _arrays(fst)
    y = np.asarray(y, np.float32).astype(np.float64)
    alpha = np.full(n, -np.inf)
    alpha[start] = 0.0
    for t in range(y.shape[0]):
        keep = np.ones(len(src), bool) if pdfs is None else pdf == int(pdfs[t])
        nxt = np.full(n, -np.inf)
        with np.errstate(invalid="ignore"):
            np.maximum.at(nxt, dst[keep], alpha[src[keep]] + (y[t, pdf[keep]] - cost[keep]))
        alpha = nxt
    with np.errstate(invalid="ignore"):
        return float(np.max(alpha - final))  # (final = +inf: not final)


def best_score64(fst, y):
    """The best float64 score over all paths of exactly ``len(y)`` arcs to a final state; ``-inf`` without one."""
    return _walk(fst, y, None)


def path_score64(fst, y, pdfs):
    """The best float64 score over the state paths that emit the pdf sequence ``pdfs`` (0-based, ``len(y)`` entries), by a
    set-of-states walk: frame t keeps only the arcs of pdf ``pdfs[t]``.  ``-inf`` if the acceptor has no such path."""
    pdfs = np.asarray(pdfs)
    assert pdfs.shape == (np.asarray(y).shape[0],)
    return _walk(fst, y, pdfs)


def magnitude(fst, y):
    """``M`` of the tests' bound: the maximum over the acceptor's arcs and the frames of ``|y[t, pdf]| + |cost|``."""
    _, _, _, _, pdf, cost, _ = _arrays(fst)
    y = np.asarray(y, np.float32).astype(np.float64)
    return float(np.max(np.abs(y[:, pdf]) + np.abs(cost)[None, :]))


def brute_force(fst, y):
    """``best_score64`` by enumeration of every path (tiny acceptors only): (score, set of the pdf sequences that reach it)."""
    start, n, src, dst, pdf, cost, final = _arrays(fst)
    y = np.asarray(y, np.float32).astype(np.float64)
    T = y.shape[0]
    out_arcs = [np.flatnonzero(src == s) for s in range(n)]
    best, arg = -np.inf, set()

    def go(state, t, score, seq):
        nonlocal best, arg
        if t == T:
            if np.isfinite(final[state]):
                total = score - final[state]
                if total > best:
                    best, arg = total, {seq}
                elif total == best:
                    arg.add(seq)
            return
        for a in out_arcs[state]:
            go(int(dst[a]), t + 1, score + (y[t, pdf[a]] - cost[a]), seq + (int(pdf[a]),))

    go(start, 0, 0.0, ())
    return best, arg


def state_times(sup):
    """Time of every state of a merged time-unfolded FST (states are numbered in time order)."""
    times = np.full(sup.num_states, -1, np.int64)
    times[0] = 0
    for s in range(sup.num_states):
        times[sup.nextstate[sup.arc_begin[s]:sup.arc_begin[s + 1]]] = times[s] + 1
    assert (times >= 0).all() and (np.diff(times) >= 0).all()
    return times


def split_merged(sup):
    """The per-sequence acceptors ``(arc_begin, ilabel, arc_weight, nextstate, final)`` of a merged uniform supervision
    whose boundary states carry no final weights (``final_weights=False``): sequence q is the first state of time q*T as its
    start -- the other states of that time carry copies of the same arcs -- and the states of times q*T + 1 .. (q + 1)*T,
    those of the last time final at cost 0 (the last sequence: at their own final cost)."""
    S, T = int(sup.num_sequences), int(sup.frames_per_sequence)
    times = state_times(sup)
    first_at = np.searchsorted(times, np.arange(S * T + 2))
    out = []
    for q in range(S):
        lo, hi = q * T, (q + 1) * T
        body0, end = int(first_at[lo + 1]), int(first_at[hi + 1])
        states = [int(first_at[lo])] + list(range(body0, end))
        local = {g: i for i, g in enumerate(states)}
        ab, il, aw, nx, fin = [0], [], [], [], []
        for g in states:
            if times[g] < hi:
                for a in range(sup.arc_begin[g], sup.arc_begin[g + 1]):
                    il.append(int(sup.ilabel[a]))
                    aw.append(float(sup.arc_weight[a]))
                    nx.append(local[int(sup.nextstate[a])])
                fin.append(np.inf)
            else:
                fin.append(float(sup.final[g]) if q == S - 1 else 0.0)
            ab.append(len(il))
        out.append((np.asarray(ab, np.int32), np.asarray(il, np.int32), np.asarray(aw, np.float32), np.asarray(nx, np.int32),
                    np.asarray(fin, np.float32)))
    return out
