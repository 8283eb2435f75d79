"""Float64 statement of the entropy of an end-to-end supervision's path posterior (``tc_supervision_path_entropy``) in plain
numpy, twice: by listing every path of a tiny FST, and by the mean-form forward-backward for everything else.  An FST is
``tests/e2e_reference.py``'s CSR tuple.  A path is exactly T arcs from the start to a final state, ``log W = sum_t (y_t(pdf_t)
- cost_t) - final``, ``H = log Z - E[log W]``, ``dH / dy_t(j) = -(E[log W 1(pdf j at t)] - E[log W] gamma_t(j))``."""
import numpy as np

from e2e_reference import _csr


def _arcs(fst):
    start, ab, il, aw, nx, final = fst
    src = np.repeat(np.arange(len(final)), np.diff(ab))
    return int(start), src, np.asarray(nx, np.int64), np.asarray(il, np.int64) - 1, np.asarray(aw, np.float64), np.asarray(final, np.float64)


def tiny_fst():
    """Three states: a self-loop, two parallel arcs of one pdf, a cycle through the start, two non-zero final costs."""
    return _csr(3, [(0, 1, 0, 0.3), (0, 1, 0, 1.1), (0, 1, 1, 0.2), (0, 2, 2, 0.9), (1, 1, 0, 0.5), (1, 0, 2, 0.1), (1, 2, 1, 0.4),
                    (2, 2, 3, 0.6), (2, 0, 1, 0.8)], [np.inf, 0.7, 0.25])  # (source, destination, pdf, cost)


def by_enumeration(fst, y):
    """``(entropy, log Z, grad (T, P))`` of one sequence from the list of its paths; ``y``: its rows, ``(T, P)`` float64."""
    start, src, dst, pdf, cost, final = _arcs(fst)
    T, logw, pdfs = y.shape[0], [], []

    def walk(state, t, lw, used):
        if t == T:
            if np.isfinite(final[state]):
                logw.append(lw - final[state])
                pdfs.append(used)
            return
        for a in np.flatnonzero(src == state):
            walk(int(dst[a]), t + 1, lw + y[t, pdf[a]] - cost[a], used + [int(pdf[a])])

    walk(start, 0, 0.0, [])
    lw = np.asarray(logw)
    logz = lw.max() + np.log(np.exp(lw - lw.max()).sum())
    p = np.exp(lw - logz)
    elw, grad = (p * lw).sum(), np.zeros_like(y)
    for k, used in enumerate(pdfs):
        grad[np.arange(T), used] -= p[k] * (lw[k] - elw)
    return logz - elw, logz, grad


def _softmax_mean(x, val, index, n):
    """Per group of ``index``: ``(logsumexp(x), softmax(x)-weighted mean of val)``, ``(-inf, 0)`` without a finite ``x``; a
    member of weight 0 does not enter the mean."""
    mx = np.full(n, -np.inf)
    np.maximum.at(mx, index, x)
    safe = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.exp(x - safe[index])
        s, num = np.zeros(n), np.zeros(n)
        np.add.at(s, index, e)
        np.add.at(num, index, np.where(e > 0, e * val, 0.0))
        return np.where(s > 0, safe + np.log(s), -np.inf), np.where(s > 0, num / s, 0.0)


def by_recursion(fst, y):
    """One sequence by the mean-form forward-backward: ``dict(entropy, logprob, grad (T, P), elw, dev)``, ``elw = E[log W]``
    and ``dev`` the largest ``|Abar + r + Bbar - E[log W]|`` over the arcs a path takes, the scale of a gradient element."""
    start, src, dst, pdf, cost, final = _arcs(fst)
    n, T = len(final), y.shape[0]
    r = y[:, pdf] - cost  # (T, arcs)
    la, ma = np.full((T + 1, n), -np.inf), np.zeros((T + 1, n))
    la[0, start] = 0.0
    for t in range(T):
        la[t + 1], ma[t + 1] = _softmax_mean(la[t, src] + r[t], ma[t, src] + r[t], dst, n)
    lb, mb = -final, np.where(np.isfinite(final), -final, 0.0)
    logz, elw = (float(v[0]) for v in _softmax_mean(la[T] + lb, ma[T] + mb, np.zeros(n, np.int64), 1))
    grad, dev = np.zeros_like(y), 0.0
    if not np.isfinite(logz):
        return dict(entropy=np.nan, logprob=-np.inf, grad=grad, elw=np.nan, dev=dev)
    for t in range(T - 1, -1, -1):
        x = r[t] + lb[dst]
        with np.errstate(invalid="ignore"):
            occ = np.exp(la[t, src] + x - logz)
            live = occ > 0
            d = (ma[t, src] + r[t] + mb[dst] - elw)[live]
        np.add.at(grad[t], pdf[live], -occ[live] * d)
        dev = max(dev, float(np.abs(d).max()))
        lb, mb = _softmax_mean(x, r[t] + mb[dst], src, n)
    return dict(entropy=logz - elw, logprob=logz, grad=grad, elw=elw, dev=dev)


def batch(fsts, y, frames):
    """A minibatch, ``y`` ``(Tmax * S, P)`` with row ``t * S + s``: ``by_recursion``'s entries as arrays over the sequences,
    ``grad`` in ``y``'s layout with zeros in the padding."""
    S = len(fsts)
    ones = [by_recursion(fst, np.asarray(y[s::S][:frames[s]], np.float64)) for s, fst in enumerate(fsts)]
    out = {k: np.array([o[k] for o in ones]) for k in ("entropy", "logprob", "elw", "dev")}
    out["grad"] = np.zeros(y.shape)
    for s, o in enumerate(ones):
        out["grad"][s::S][:frames[s]] = o["grad"]
    return out
