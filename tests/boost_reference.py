"""The statement of boosted LF-MMI (``chain_loss(..., boost=b, boost_ref= / boost_accuracy=)``) that the tests
hold the library to.

    a_t(j)   hard: 1 iff 0 <= ref[s, t] < P and class(j) == class(ref[s, t]), else 0;  dense: the float32 matrix, row t*S + s
    y_b      = fl32(y32 - fl32(b32 * a))                      numpy float32, two roundings
    objf     = w * (num_logprob(y) - den_logprob(y_b))
    deriv    = w * (gamma_num(y) - gamma_den(y_b)) - l2 * w * y           l2_term = -0.5 * w * l2 * sum(y^2): on the true y

``float64``: the numerator of ``oracle/independent_f64.py`` on ``y`` and its denominator on ``y_b`` (regular supervisions of
one length).  ``oracle32``: the same composition from ``oracle/pyoracle.py`` (``num_forward_backward(sup, y)``,
``den_forward_backward(graph, y_b)``), the float32 CPU oracle.  Rows are frame-major, ``t*S + s``."""
import numpy as np


def indicator(ref, pdf_class, P):
    """The float32 indicator (T*S, P) of a hard reference ``ref`` (int (S, T); -1 or out of range: the frame scores nothing)
    and an optional class map (int (P,))."""
    ref = np.asarray(ref)
    S, T = ref.shape
    cls = np.arange(P) if pdf_class is None else np.asarray(pdf_class)
    a = np.zeros((T * S, P), np.float32)
    for s in range(S):
        for t in range(T):
            r = int(ref[s, t])
            if 0 <= r < P:
                a[t * S + s] = (cls == cls[r]).astype(np.float32)
    return a


def boosted(y, boost, a):
    """y_b in numpy float32: the product rounded, then the difference rounded."""
    y32 = np.asarray(y).astype(np.float32)
    d = (np.float32(boost) * np.asarray(a, np.float32)).astype(np.float32)
    return (y32 - d).astype(np.float32)


def float64(fst, initial_probs, sup, y, boost, a, l2=0.0, leaky=1e-5):
    """dict(objf, l2_term, weight, num, den, deriv, xent_deriv) in float64; ``den`` is the boosted denominator's log-prob."""
    from oracle import independent_f64 as ind
    y32 = np.asarray(y, np.float32)
    yb = boosted(y32, boost, a)
    plain = ind.chain_objf_and_deriv(fst, initial_probs, sup, y32, l2, leaky)  # (its numerator and l2 term: on y)
    den, gden = ind.den_logprob_and_deriv(fst, initial_probs, np.clip(yb.astype(np.float64), -30.0, 30.0), sup.num_sequences, leaky)
    w = float(sup.weight)
    y64 = y32.astype(np.float64)
    # (gden: the occupation of the clamped value, which is what [K] and the kernels return for an output beyond +-30)
    deriv = plain["xent_deriv"] - w * gden - w * l2 * y64
    return dict(objf=w * plain["num"] - w * den, l2_term=plain["l2_term"], weight=plain["weight"], num=plain["num"], den=den,
                deriv=deriv, xent_deriv=plain["xent_deriv"], den_deriv=gden, yb=yb)


def oracle32(pyoracle, graph, sup, y, boost, a, l2=0.0, leaky=1e-5):
    """The same composition from the float32 CPU oracle ([K]'s recursions): dict(objf, l2_term, weight, deriv, xent_deriv)."""
    y32 = np.asarray(y, np.float32)
    yb = boosted(y32, boost, a)
    w = float(sup.weight)
    num = pyoracle.num_forward_backward(sup, y32)
    den = pyoracle.den_forward_backward(graph, yb, sup.num_sequences, leaky=leaky, deriv_weight=-w)
    y64 = y32.astype(np.float64)
    deriv = num["deriv"].astype(np.float64) + den["deriv"].astype(np.float64) - w * l2 * y64
    return dict(objf=float(num["logprob_weighted"]) - w * float(den["logprob"]), l2_term=-0.5 * w * l2 * float((y64 * y64).sum()),
                weight=w * sup.num_sequences * sup.frames_per_sequence, deriv=deriv, xent_deriv=num["deriv"].astype(np.float64),
                den=float(den["logprob"]), ok=den["ok"])


def enumerate_den_logprob(fst, initial_probs, y_seq, frame_acc, boost):
    """log sum over every path of T arcs through ``fst`` (any start state, weighted by initial_probs; every state final; leaky
    coefficient 0) of exp(score(path) - boost * A(path)), by plain enumeration in float64: score = log pi(start) + sum_t
    (log w(arc_t) + y_seq[t, pdf(arc_t)]), A = sum_t frame_acc[t, pdf(arc_t)].  One sequence: ``y_seq``, ``frame_acc`` are
    (T, P)."""
    y_seq, frame_acc = np.asarray(y_seq, np.float64), np.asarray(frame_acc, np.float64)
    T = y_seq.shape[0]
    src, dst = np.asarray(fst.src), np.asarray(fst.dst)
    pdf, logw = np.asarray(fst.ilabel) - 1, -np.asarray(fst.weight, np.float64)
    out = [[] for _ in range(fst.num_states)]
    for k in range(len(src)):
        out[int(src[k])].append(k)
    terms = []

    def walk(state, t, score, acc):
        if t == T:
            terms.append(score - boost * acc)
            return
        for k in out[state]:
            walk(int(dst[k]), t + 1, score + logw[k] + y_seq[t, pdf[k]], acc + frame_acc[t, pdf[k]])

    for h in range(fst.num_states):
        if initial_probs[h] > 0:
            walk(h, 0, float(np.log(initial_probs[h])), 0.0)
    terms = np.asarray(terms)
    m = terms.max()
    return float(m + np.log(np.exp(terms - m).sum()))
