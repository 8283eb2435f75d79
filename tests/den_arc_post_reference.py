"""Float64 reference of the denominator graph's arc and entry occupations (``io.DenominatorGraph.arc_posteriors`` /
``tc_den_arc_posteriors``): the log-semiring recursion of ``oracle/independent_f64.den_logprob`` restated with ``log w``,
``log pi`` and ``log c`` as leaf tensors and a length per sequence, so that the occupations are what autograd says they are --
``d log Z_s / d log w_a``, ``d log Z_s / d log pi(h)`` and ``d log Z_s / d log c``.  No backward pass is written here."""
import numpy as np
import torch

from oracle.independent_f64 import _segment_logsumexp


def occupations(arcs, pi, y, num_sequences, leaky, frames=None):
    """``arcs``: ``(src, dst, pdf, prob)`` as ``DenominatorGraph.arcs()`` gives them; ``pi``: the handle's initial
    probabilities; ``y``: float ``(T*S, P)``, row ``t*S + s``, inside the clamp.  Returns float64 numpy arrays ``arcs (S, A)``,
    ``entries (S, H)``, ``leaks (S,)`` and ``logprob (S,)``."""
    src, dst, pdf = (torch.as_tensor(np.asarray(a, np.int64)) for a in arcs[:3])
    S, H = num_sequences, len(pi)
    T = y.shape[0] // S
    yy = torch.as_tensor(np.asarray(y, np.float64)).view(T, S, -1)
    # (pi(h) = 0 is floored as in oracle/independent_f64: autograd never meets logaddexp(-inf, -inf))
    leaves = [torch.tensor(np.log(np.asarray(arcs[3], np.float64)), requires_grad=True),
              torch.tensor(np.log(np.maximum(np.asarray(pi, np.float64), 1e-300)), requires_grad=True),
              torch.tensor(float(np.log(leaky)), dtype=torch.float64, requires_grad=True)]
    logw, logpi, logc = leaves

    def dash(la):
        return torch.logaddexp(la, logc + logpi + torch.logsumexp(la, dim=0))

    out = [[], [], [], []]
    for s in range(S):
        la = logpi
        for t in range(T if frames is None else int(frames[s])):
            la = _segment_logsumexp((dash(la)[src] + logw + yy[t, s][pdf]).unsqueeze(0), dst.unsqueeze(0), H)[0]
        logz = torch.logsumexp(dash(la), dim=0)
        for got, grad in zip(out, torch.autograd.grad(logz, leaves) + (logz.detach(),)):
            got.append(grad.numpy())
    return dict(zip(("arcs", "entries", "leaks", "logprob"), (np.stack(o) for o in out)))
