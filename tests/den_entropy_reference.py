"""Float64 reference of the entropy of the denominator graph's path posterior (``io.DenominatorGraph.path_entropy`` /
``tc_den_path_entropy``): the log-semiring recursion of ``tests/den_arc_post_reference.py`` with ``y``, ``log w``, ``log pi``
and ``log c`` as leaf tensors.  ``log W`` of a latent path is linear in those leaves with the path's counts as coefficients, so
``E[log W] = sum_theta theta * d log Z / d theta`` and ``H = log Z - E[log W]``; the first derivatives are taken with
``create_graph=True`` and ``dH/dy`` is what autograd says it is.  No backward pass is written here."""
import numpy as np
import torch

from oracle.independent_f64 import _segment_logsumexp


def path_entropy(arcs, pi, y, num_sequences, leaky, frames=None):
    """``arcs``: ``(src, dst, pdf, prob)`` as ``DenominatorGraph.arcs()`` gives them; ``pi``: the handle's initial
    probabilities; ``y``: float ``(T*S, P)``, row ``t*S + s``, inside the clamp.  Returns float64 numpy arrays ``entropy (S,)``,
    ``logprob (S,)`` and ``grad (T*S, P)`` (row ``t*S + s``: ``d entropy[s] / d y``, 0 in padding rows)."""
    src, dst, pdf = (torch.as_tensor(np.asarray(a, np.int64)) for a in arcs[:3])
    S, H = num_sequences, len(pi)
    T = y.shape[0] // S
    # (pi(h) = 0 is floored as in oracle/independent_f64: its count is 0, and so is its term of E[log W])
    leaves = [torch.tensor(np.asarray(y, np.float64).reshape(T, S, -1), requires_grad=True),
              torch.tensor(np.log(np.asarray(arcs[3], np.float64)), requires_grad=True),
              torch.tensor(np.log(np.maximum(np.asarray(pi, np.float64), 1e-300)), requires_grad=True),
              torch.tensor(float(np.log(leaky)), dtype=torch.float64, requires_grad=True)]
    yy, logw, logpi, logc = leaves

    def dash(la):
        return torch.logaddexp(la, logc + logpi + torch.logsumexp(la, dim=0))

    entropy, logprob, grad = np.zeros(S), np.zeros(S), np.zeros((T, S, yy.shape[2]))
    for s in range(S):
        la = logpi
        for t in range(T if frames is None else int(frames[s])):
            la = _segment_logsumexp((dash(la)[src] + logw + yy[t, s][pdf]).unsqueeze(0), dst.unsqueeze(0), H)[0]
        logz = torch.logsumexp(dash(la), dim=0)
        counts = torch.autograd.grad(logz, leaves, create_graph=True)
        h = logz - sum((theta * n).sum() for theta, n in zip(leaves, counts))
        grad += torch.autograd.grad(h, yy)[0].numpy()
        entropy[s], logprob[s] = float(h.detach()), float(logz.detach())
    return {"entropy": entropy, "logprob": logprob, "grad": grad.reshape(T * S, -1)}
