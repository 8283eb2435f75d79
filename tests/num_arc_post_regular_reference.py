"""Float64 statement of a regular supervision's arc occupations (``tc_supervision_arc_posteriors_regular``) in plain numpy: the
log-domain forward-backward of one sequence on the caller's own acceptor ``(start 0, arc_begin, ilabel, cost, nextstate, final
cost)``, states in time order.  ``arcs[a] = P(the path takes arc a)`` in the CSR order, ``finals[i] = P(it ends in state i)``."""
import numpy as np


def _logsum_at(x, index, n):
    """``logsumexp`` of ``x`` per group of ``index``, ``-inf`` for a group without a finite member"""
    mx = np.full(n, -np.inf)
    np.maximum.at(mx, index, x)
    safe = np.where(np.isfinite(mx), mx, 0.0)
    s = np.zeros(n)
    np.add.at(s, index, np.exp(x - safe[index]))
    with np.errstate(divide="ignore"):
        return np.where(s > 0, safe + np.log(s), -np.inf)


def one(fst, y):
    """``dict(arcs (A,), finals (N,), logprob)`` of one sequence; ``y``: its rows, ``(T, P)`` float64"""
    _, ab, il, cost, nxt, final = fst
    n, final = len(final), np.asarray(final, np.float64)
    src, dst = np.repeat(np.arange(n), np.diff(ab)), np.asarray(nxt, np.int64)
    time = np.zeros(n, np.int64)
    for a in range(len(src)):  # (states in time order: a source's time is known when its arcs come up)
        time[dst[a]] = time[src[a]] + 1
    r = np.asarray(y, np.float64)[time[src], np.asarray(il, np.int64) - 1] - np.asarray(cost, np.float64)
    la = np.full(n, -np.inf)
    la[0] = 0.0
    for t in range(y.shape[0]):
        m = time[src] == t
        la[time == t + 1] = _logsum_at(la[src[m]] + r[m], dst[m], n)[time == t + 1]
    ends = time == y.shape[0]
    logz = float(_logsum_at((la - final)[ends], np.zeros(ends.sum(), np.int64), 1)[0])
    arcs, finals = np.zeros(len(src)), np.zeros(n)
    if np.isfinite(logz):
        lb = np.where(ends, -final, -np.inf)
        finals[ends] = np.exp((la + lb - logz)[ends])
        for t in range(y.shape[0] - 1, -1, -1):
            m = time[src] == t
            arcs[m] = np.exp(la[src[m]] + r[m] + lb[dst[m]] - logz)
            lb[time == t] = _logsum_at(r[m] + lb[dst[m]], src[m], n)[time == t]
    return dict(arcs=arcs, finals=finals, logprob=logz)


def batch(fsts, y, frames):
    """A minibatch, ``y`` ``(Tmax * S, P)`` with row ``t * S + s``: ``one`` per sequence on its valid frames"""
    S = len(fsts)
    return [one(fst, np.asarray(y[s::S][:frames[s]], np.float64)) for s, fst in enumerate(fsts)]
