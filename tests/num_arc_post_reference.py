"""Float64 statement of an end-to-end supervision's arc occupations (``tc_supervision_arc_posteriors``) in plain numpy, twice: by
listing every path of a tiny FST, and by the log-domain forward-backward for everything else.  An FST is
``tests/e2e_reference.py``'s CSR tuple; arcs are in its order.  A path is exactly T arcs from the start to a final state, ``log W =
sum_t (y_t(pdf_t) - cost_t) - final``; ``arcs[a]`` is the expected number of times the path takes arc ``a``, ``finals[i]`` the
probability that it ends in state ``i``."""
import numpy as np

from num_entropy_reference import _arcs


def _logsum_at(x, index, n):
    """``logsumexp`` of ``x`` per group of ``index``, ``-inf`` for a group without a finite member"""
    mx = np.full(n, -np.inf)
    np.maximum.at(mx, index, x)
    safe = np.where(np.isfinite(mx), mx, 0.0)
    s = np.zeros(n)
    np.add.at(s, index, np.exp(x - safe[index]))
    with np.errstate(divide="ignore"):
        return np.where(s > 0, safe + np.log(s), -np.inf)


def by_recursion(fst, y, cost=None):
    """``dict(arcs (A,), finals (N,), logprob)`` of one sequence; ``y``: its rows, ``(T, P)`` float64.  ``cost`` replaces the
    FST's arc costs (the finite difference of the host test)."""
    start, src, dst, pdf, cost0, final = _arcs(fst)
    n, T = len(final), y.shape[0]
    r = y[:, pdf] - (cost0 if cost is None else cost)  # (T, arcs)
    la = np.full((T + 1, n), -np.inf)
    la[0, start] = 0.0
    for t in range(T):
        la[t + 1] = _logsum_at(la[t, src] + r[t], dst, n)
    logz = float(_logsum_at(la[T] - final, np.zeros(n, np.int64), 1)[0])
    arcs, finals = np.zeros(len(src)), np.zeros(n)
    if np.isfinite(logz):
        lb = -final
        finals = np.exp(la[T] + lb - logz)
        for t in range(T - 1, -1, -1):
            term = r[t] + lb[dst]
            arcs += np.exp(la[t, src] + term - logz)
            lb = _logsum_at(term, src, n)
    return dict(arcs=arcs, finals=finals, logprob=logz)


def by_enumeration(fst, y):
    """the same from the list of the FST's paths"""
    start, src, dst, pdf, cost, final = _arcs(fst)
    T, paths = y.shape[0], []

    def walk(state, t, lw, used):
        if t == T:
            if np.isfinite(final[state]):
                paths.append((lw - final[state], used, state))
            return
        for a in np.flatnonzero(src == state):
            walk(int(dst[a]), t + 1, lw + y[t, pdf[a]] - cost[a], used + [int(a)])

    walk(start, 0, 0.0, [])
    lw = np.array([p[0] for p in paths])
    logz = lw.max() + np.log(np.exp(lw - lw.max()).sum())
    arcs, finals = np.zeros(len(src)), np.zeros(len(final))
    for w, used, end in paths:
        np.add.at(arcs, used, np.exp(w - logz))
        finals[end] += np.exp(w - logz)
    return dict(arcs=arcs, finals=finals, logprob=float(logz))


def batch(fsts, y, frames):
    """A minibatch, ``y`` ``(Tmax * S, P)`` with row ``t * S + s``: one ``by_recursion`` per sequence on its valid frames"""
    S = len(fsts)
    return [by_recursion(fst, np.asarray(y[s::S][:frames[s]], np.float64)) for s, fst in enumerate(fsts)]
