"""Float64 reference of the expected frame accuracy over a denominator graph and of its gradient
(``io.DenominatorGraph.expected_accuracy`` / ``functions.den_expected_accuracy``, lattice-free sMBR).  A helper, not a test
module; numpy, and torch autograd for the oracle; no GPU.

Per sequence, with the denominator's own model: ``p_t(j) = exp(clamp(y_t(j), +-30))``, initial probabilities ``pi``, leaky
coefficient ``c``, every state final.  ``a_t(j) = 1`` where ``0 <= ref_t < P`` and ``class(j) == class(ref_t)``, else 0.

    E[A] = sum_paths P(path | y) * sum_t a_t(pdf_t(path)) = sum_t m_t,     m_t = sum_j gamma_t(j) * a_t(j)

``recursion`` states the two forward-backward passes of ``include/torchain_hip.h`` (Kaldi's scaling, the accuracy mass
``A`` beside ``alpha`` and ``B`` beside ``beta``, centred with ``m_t``) in float64.  ``oracle`` reaches the same numbers
another way: a double backward through ``oracle/independent_f64.den_logprob`` -- ``grad(den, y, create_graph=True)`` is
``gamma``, ``(gamma * a).sum()`` is ``E[A]``, and ``grad`` of that is the gradient.
"""
import numpy as np
import torch

from oracle import independent_f64

OUTPUT_LIMIT = 30.0


def arcs_of(fst, prob=None):
    """``(src, dst, pdf, w)`` of an FST of ``torchain_amd.synth``: ``w = exp(-weight)`` in float64, or ``prob`` (the
    float32 probabilities a graph handle holds, ``io.DenominatorGraph.arcs()[3]``)."""
    w = np.exp(-fst.weight.astype(np.float64)) if prob is None else np.asarray(prob, np.float64)
    return fst.src.astype(np.int64), fst.dst.astype(np.int64), fst.ilabel.astype(np.int64) - 1, w


def accuracy(ref, pdf_class, P):
    """``a[t, j]`` (float64 ``(T, P)``) of a reference ``ref`` (``T`` ints) and a class map (``P`` ints or ``None``)."""
    ref = np.asarray(ref, np.int64)
    cls = np.arange(P, dtype=np.int64) if pdf_class is None else np.asarray(pdf_class, np.int64)
    a = np.zeros((len(ref), P))
    ok = (ref >= 0) & (ref < P)
    a[ok] = cls[None, :] == cls[ref[ok]][:, None]
    return a


def recursion(arcs, pi, y, ref, pdf_class, leaky, centre=None):
    """One sequence.  ``y``: ``(T, P)``.  Returns a dict: ``acc`` (``E[A]``), ``frame_acc`` (``m_t``), ``gamma`` (``(T, P)``),
    ``grad`` (``dE[A]/dy``, ``(T, P)``), ``residual`` (``E~``: what the centred recursion is left with, 0 when ``centre`` is
    ``m_t``).  ``centre``: the per-frame constants subtracted from ``a_t`` in the accuracy passes (``None``: ``m_t``)."""
    src, dst, pdf, w = arcs
    pi = np.asarray(pi, np.float64)
    y = np.asarray(y, np.float64)
    T, P = y.shape
    H = len(pi)
    c = float(leaky)
    p = np.exp(np.clip(y, -OUTPUT_LIMIT, OUTPUT_LIMIT))
    a = accuracy(ref, pdf_class, P)

    def scatter(index, values, size):
        out = np.zeros(size)
        np.add.at(out, index, values)
        return out

    # ---- the denominator's own forward-backward: gamma, m_t ----
    alpha_d = np.zeros((T + 1, H))  # alpha'_t
    asum = np.zeros(T + 1)
    alpha = pi.copy()
    for t in range(T + 1):
        asum[t] = alpha.sum()
        alpha_d[t] = alpha + c * pi * asum[t]
        if t < T:
            alpha = scatter(dst, alpha_d[t, src] * w * p[t, pdf] / asum[t], H)
    Z = alpha_d[T].sum()
    beta = np.zeros((T + 1, H))  # beta_t (with the leak)
    bd = np.full(H, 1.0 / Z)
    beta[T] = bd + c * (pi * bd).sum()
    gamma = np.zeros((T, P))
    for t in range(T - 1, -1, -1):
        f = w * p[t, pdf] / asum[t]
        gamma[t] = scatter(pdf, alpha_d[t, src] * f * beta[t + 1, dst], P)
        bd = scatter(src, f * beta[t + 1, dst], H)
        beta[t] = bd + c * (pi * bd).sum()
    m = (gamma * a).sum(axis=1)
    ct = m if centre is None else np.asarray(centre, np.float64)
    at = a - ct[:, None]

    # ---- the accuracy mass beside alpha ----
    A_d = np.zeros((T + 1, H))  # A'_t
    A = np.zeros(H)
    for t in range(T + 1):
        A_d[t] = A + c * pi * A.sum()
        if t < T:
            f = w * p[t, pdf] / asum[t]
            A = scatter(dst, (A_d[t, src] + alpha_d[t, src] * at[t, pdf]) * f, H)
    E = A_d[T].sum() / Z

    # ---- ... and beside beta; the gradient ----
    Bd = np.zeros(H)
    B = Bd + c * (pi * Bd).sum()
    grad = np.zeros((T, P))
    for t in range(T - 1, -1, -1):
        f = w * p[t, pdf] / asum[t]
        b1, B1 = beta[t + 1, dst], B[dst]
        al, Al = alpha_d[t, src], A_d[t, src]
        grad[t] = scatter(pdf, f * (Al * b1 + al * at[t, pdf] * b1 + al * B1 - al * b1 * E), P)
        Bd = scatter(src, f * (B1 + at[t, pdf] * b1), H)
        B = Bd + c * (pi * Bd).sum()
    return dict(acc=float(m.sum()), frame_acc=m, gamma=gamma, grad=grad, residual=float(E + ct.sum() - m.sum()))


def batch(arcs, pi, y2d, S, ref, pdf_class, leaky, frames=None):
    """``recursion`` for every sequence of a frame-major matrix (row ``t*S + s``); ``ref``: ``(S, T)``.  Returns ``(acc (S,),
    frame_acc (S, T), grad (T*S, P))``, zero in padding frames."""
    y2d = np.asarray(y2d, np.float64)
    T, P = y2d.shape[0] // S, y2d.shape[1]
    acc, fa, grad = np.zeros(S), np.zeros((S, T)), np.zeros((T * S, P))
    for s in range(S):
        Ts = T if frames is None else int(frames[s])
        r = recursion(arcs, pi, y2d[s::S][:Ts], np.asarray(ref)[s, :Ts], pdf_class, leaky)
        acc[s], fa[s, :Ts] = r["acc"], r["frame_acc"]
        grad[s::S][:Ts] = r["grad"]
    return acc, fa, grad


def oracle(fst, pi, y2d, S, ref, pdf_class, leaky):
    """``(acc (S,), grad (T*S, P))`` by a double backward through ``oracle/independent_f64.den_logprob`` (uniform lengths;
    ``|y|`` below the output limit, which the oracle does not apply)."""
    yt = torch.tensor(np.asarray(y2d, np.float64), requires_grad=True)
    T, P = yt.shape[0] // S, yt.shape[1]
    den = independent_f64.den_logprob(fst, pi, yt, S, leaky)
    (gamma,) = torch.autograd.grad(den, yt, create_graph=True)
    acc, grad = np.zeros(S), np.zeros((T * S, P))
    for s in range(S):
        a = torch.as_tensor(accuracy(np.asarray(ref)[s], pdf_class, P))
        e = (gamma[s::S] * a).sum()
        (g,) = torch.autograd.grad(e, yt, retain_graph=True, allow_unused=True)
        acc[s] = float(e.detach())
        grad += 0.0 if g is None else g.numpy()
    return acc, grad


def random_path(fst, pi, T, rng):
    """The pdfs of a random path of ``T`` arcs from a state with ``pi > 0``."""
    starts = np.nonzero(np.asarray(pi) > 0)[0]
    while True:
        h, pdfs = int(rng.choice(starts)), []
        for _ in range(T):
            out = np.nonzero(fst.src == h)[0]
            if len(out) == 0:
                break
            k = int(rng.choice(out))
            h = int(fst.dst[k])
            pdfs.append(int(fst.ilabel[k]) - 1)
        if len(pdfs) == T:
            return np.array(pdfs, np.int32)
