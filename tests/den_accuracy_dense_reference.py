"""Float64 reference of the expected accuracy over a denominator graph against a DENSE per-pdf accuracy and of its two
gradients (``io.DenominatorGraph.expected_accuracy_dense`` / ``functions.den_expected_accuracy_dense``: lattice-free sMBR
against soft references).  A helper, not a test module; numpy, and torch autograd for the oracle; no GPU.

The model is ``tests/den_accuracy_reference.py``'s; ``a_t(j)`` is entry ``(t, j)`` of a matrix of any finite values:

    E[A] = sum_paths P(path | y) * sum_t a_t(pdf_t(path)) = sum_t m_t,     m_t = sum_j gamma_t(j) * a_t(j)

``recursion`` is that module's recursion -- the two forward-backward passes of ``include/torchain_hip.h``, centred with
``m_t`` -- with the matrix in place of the indicator; on an indicator it gives that module's numbers.  ``dE/da_t(j)`` is
``gamma_t(j)``.  ``oracle`` reaches the three results by a double backward through ``oracle/independent_f64.den_logprob``.
"""
import numpy as np
import torch

from oracle import independent_f64

from den_accuracy_reference import OUTPUT_LIMIT


def recursion(arcs, pi, y, a, leaky):
    """One sequence.  ``y``, ``a``: ``(T, P)``.  Returns a dict: ``acc`` (``E[A]``), ``frame_acc`` (``m_t``), ``gamma``
    (``(T, P)``: the denominator posteriors, ``dE[A]/da``), ``grad`` (``dE[A]/dy``, ``(T, P)``), ``residual`` (``E~``)."""
    src, dst, pdf, w = arcs
    pi = np.asarray(pi, np.float64)
    y = np.asarray(y, np.float64)
    a = np.asarray(a, np.float64)
    T, P = y.shape
    assert a.shape == (T, P)
    H = len(pi)
    c = float(leaky)
    p = np.exp(np.clip(y, -OUTPUT_LIMIT, OUTPUT_LIMIT))

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
    at = a - m[:, None]

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
    return dict(acc=float(m.sum()), frame_acc=m, gamma=gamma, grad=grad, residual=float(E))


def batch(arcs, pi, y2d, S, a2d, leaky, frames=None):
    """``recursion`` for every sequence of two frame-major matrices (row ``t*S + s``).  Returns ``(acc (S,), frame_acc (S, T),
    grad (T*S, P), gamma (T*S, P))``, zero in padding frames."""
    y2d, a2d = np.asarray(y2d, np.float64), np.asarray(a2d, np.float64)
    T, P = y2d.shape[0] // S, y2d.shape[1]
    acc, fa, grad, gamma = np.zeros(S), np.zeros((S, T)), np.zeros((T * S, P)), np.zeros((T * S, P))
    for s in range(S):
        Ts = T if frames is None else int(frames[s])
        r = recursion(arcs, pi, y2d[s::S][:Ts], a2d[s::S][:Ts], leaky)
        acc[s], fa[s, :Ts] = r["acc"], r["frame_acc"]
        grad[s::S][:Ts] = r["grad"]
        gamma[s::S][:Ts] = r["gamma"]
    return acc, fa, grad, gamma


def oracle(fst, pi, y2d, S, a2d, leaky):
    """``(acc (S,), dE/dy (T*S, P), dE/da (T*S, P))`` by a double backward through ``oracle/independent_f64.den_logprob``
    (uniform lengths; ``|y|`` below the output limit, which the oracle does not apply).  ``E`` is the sum over the sequences:
    a sequence's rows of the two gradients are its own."""
    yt = torch.tensor(np.asarray(y2d, np.float64), requires_grad=True)
    at = torch.tensor(np.asarray(a2d, np.float64), requires_grad=True)
    den = independent_f64.den_logprob(fst, pi, yt, S, leaky)
    (gamma,) = torch.autograd.grad(den, yt, create_graph=True)
    per_seq = torch.stack([(gamma[s::S] * at[s::S]).sum() for s in range(S)])
    gy, ga = torch.autograd.grad(per_seq.sum(), (yt, at))
    return per_seq.detach().numpy(), gy.numpy(), ga.numpy()


def indicator(ref, pdf_class, P, S):
    """The float32 frame-major indicator matrix ``(T*S, P)`` of a reference ``(S, T)`` and a class map."""
    from den_accuracy_reference import accuracy
    ref = np.asarray(ref)
    T = ref.shape[1]
    a = np.zeros((T * S, P), np.float32)
    for s in range(S):
        a[s::S] = accuracy(ref[s], pdf_class, P)
    return a
