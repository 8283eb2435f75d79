"""Reference of the path sampler of a denominator graph (``io.DenominatorGraph.sample_paths`` / ``tc_den_sample_paths``).  A
helper, not a test module; plain numpy, no GPU.

The model and the selection rule of ``include/torchain_hip.h``, literally.  With ``c`` the leaky coefficient, per sequence:

    alpha_0 = pi;   asum_t = sum_h alpha_t(h);   alpha'_t(h) = alpha_t(h) + c pi(h) asum_t
    alpha_{t+1}(g) = sum_{h->g} alpha'_t(h) w p_t(pdf) / asum_t,          p_t(j) = exp(clamp(y_t(j), +-30))

A latent path has levels ``t = 0 .. T``; at each it holds the state it entered (``pre_t``) and the state it leaves from
(``post_t``).  ``pick(weights, u)``: the first index whose inclusive cumulative sum exceeds ``u * total``, in doubles; the
last index of positive weight when rounding leaves none.  ``post_T = pick(alpha'_T, u[T, 2])``; then for ``t = T .. 0`` with
``j = post_t``: no leak iff ``u[t, 0] * alpha'_t(j) < alpha_t(j)``; ``pre_t = j`` or ``pick(alpha_t, u[t, 1])``; and for
``t > 0`` the in-arcs of ``pre_t`` in arc-list order, weighted ``alpha'_{t-1}(src) * w * p_{t-1}(pdf)``, picked with
``u[t-1, 2]``.

``forward`` keeps the library's stated roundings: ``alpha_t`` and ``asum_t`` are float32 where they are stored, sums are
float64 rounded once, ``p`` is a float32 exponential, ``w`` and ``pi`` the handle's float32 probabilities.  What is left
between this and the kernel is the last bit of ``expf`` and the association of the float64 sums, so a decision can differ
only where its threshold is *close* to an end of the chosen interval.  ``sample`` flags such samples:

    delta(T) = 16 * (T + 2) * 2^-24

-- the float32 forward pass puts at most about 8 roundings of 2^-24 on an alpha per level (exp, two products, the division
by asum, the leak add, the store); the linear worst case over T + 1 levels, doubled.  Derived, not tuned.
"""
import numpy as np

import den_accuracy_reference as dar

OUTPUT_LIMIT = 30.0
FLT_MIN = float(np.finfo(np.float32).tiny)


def delta(T):
    return 16.0 * (T + 2) * 2.0 ** -24


def tables(fst, initial_probs, prob=None):
    """``(src, dst, pdf, w, pi, in_begin, in_order)``: ``w`` and ``pi`` float64 arrays holding the float32 table entries
    (``exp(-weight)`` rounded to float32, or ``prob``: ``io.DenominatorGraph.arcs()[3]``); ``in_order[in_begin[h] :
    in_begin[h + 1]]`` are the in-arcs of state ``h`` in arc-list order."""
    w = (np.exp(-fst.weight.astype(np.float64)) if prob is None else np.asarray(prob)).astype(np.float32).astype(np.float64)
    pi = np.asarray(initial_probs).astype(np.float32).astype(np.float64)
    src, dst = fst.src.astype(np.int64), fst.dst.astype(np.int64)
    pdf = fst.ilabel.astype(np.int64) - 1
    order = np.argsort(dst, kind="stable")
    begin = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=len(pi)))])
    return src, dst, pdf, w, pi, begin, order


def _leak_alpha(alpha, pi, c, asum):
    """alpha' from the stored float32 alpha, pi and asum: one float64 expression rounded to float32 (held as float64)."""
    return (alpha + pi * (c * asum)).astype(np.float32).astype(np.float64)


def forward(tab, y, leaky):
    """``(alpha (T + 1, H), asum (T + 1,), p (T, P), ok)``, float64 arrays holding the stored float32 values.  ``ok`` is
    False for a NaN or an infinity in ``y`` and for an ``asum_t`` that is zero, subnormal or not finite."""
    src, dst, pdf, w, pi, _, _ = tab
    y = np.asarray(y, np.float32)
    T, H = y.shape[0], len(pi)
    c = float(np.float32(leaky))
    alpha, asum = np.zeros((T + 1, H)), np.zeros(T + 1)
    if not np.isfinite(y).all():
        return alpha, asum, np.zeros(y.shape), False
    p = np.exp(np.clip(y, np.float32(-OUTPUT_LIMIT), np.float32(OUTPUT_LIMIT))).astype(np.float32).astype(np.float64)
    alpha[0] = pi
    for t in range(T + 1):
        asum[t] = float(np.float32(alpha[t].sum()))
        if not (FLT_MIN <= asum[t] <= np.finfo(np.float32).max):
            return alpha, asum, p, False
        if t < T:
            ad = _leak_alpha(alpha[t], pi, c, asum[t])
            nxt = np.zeros(H)
            np.add.at(nxt, dst, ad[src] * (w * p[t, pdf]))
            alpha[t + 1] = (nxt * (1.0 / asum[t])).astype(np.float32).astype(np.float64)
    return alpha, asum, p, True


def pick(weights, u, d):
    """``(index, close)``: the selection rule on float64 ``weights`` with the uniform ``u``; ``close`` when the threshold lies
    within ``d * total`` of either end of the chosen interval.  ``(-1, False)`` when the total is not positive."""
    weights = np.asarray(weights, np.float64)
    cum = np.cumsum(weights)
    total = float(cum[-1]) if len(cum) else 0.0
    if not total > 0.0:
        return -1, False
    thr = float(u) * total
    over = np.nonzero((cum > thr) & (weights > 0))[0]
    i = int(over[0]) if len(over) else int(np.nonzero(weights > 0)[0][-1])
    lo, hi = float(cum[i] - weights[i]), float(cum[i])
    return i, bool(thr - lo < d * total or hi - thr < d * total)


def sample(tab, fwd, leaky, u, d=None):
    """One sample: ``(pdfs (T,), states (T + 1, 2), close, leaks)`` for the uniforms ``u`` (``(>= T + 1, 3)``); ``-1``
    everywhere when the sequence failed."""
    src, dst, pdf, w, pi, begin, order = tab
    alpha, asum, p, ok = fwd
    T = alpha.shape[0] - 1
    d = delta(T) if d is None else d
    c = float(np.float32(leaky))
    u = np.asarray(u, np.float32).astype(np.float64)
    pdfs, states = np.full(T, -1, np.int64), np.full((T + 1, 2), -1, np.int64)
    if not ok:
        return pdfs, states, False, 0
    post, close = pick(_leak_alpha(alpha[T], pi, c, asum[T]), u[T, 2], d)
    if post < 0:
        return pdfs, states, False, 0
    leaks = 0
    for t in range(T, -1, -1):
        al = alpha[t, post]
        ap = float(_leak_alpha(alpha[t, post:post + 1], pi[post:post + 1], c, asum[t])[0])
        close |= abs(u[t, 0] * ap - al) < d * ap
        pre = post
        if not u[t, 0] * ap < al:
            leaks += 1
            pre, near = pick(alpha[t], u[t, 1], d)
            close |= near
        states[t] = pre, post
        if t == 0:
            break
        arcs = order[begin[pre]:begin[pre + 1]]
        ad = _leak_alpha(alpha[t - 1, src[arcs]], pi[src[arcs]], c, asum[t - 1])
        i, near = pick(ad * w[arcs] * p[t - 1, pdf[arcs]], u[t - 1, 2], d)
        close |= near
        pdfs[t - 1] = pdf[arcs[i]]
        post = int(src[arcs[i]])
    return pdfs, states, bool(close), leaks


def batch(tab, y2d, S, leaky, uniforms, frames=None):
    """``sample`` for every sequence of a frame-major matrix (row ``t*S + s``) and every sample of ``uniforms`` ``(S, K,
    T + 1, 3)``: ``(pdfs (S, K, T), states (S, K, T + 1, 2), close (S, K), leaks (S, K))``, ``-1`` in padding slots."""
    y2d = np.asarray(y2d, np.float32)
    T = y2d.shape[0] // S
    K = uniforms.shape[1]
    pdfs, states = np.full((S, K, T), -1, np.int64), np.full((S, K, T + 1, 2), -1, np.int64)
    close, leaks = np.zeros((S, K), bool), np.zeros((S, K), np.int64)
    for s in range(S):
        Ts = T if frames is None else int(frames[s])
        fwd = forward(tab, y2d[s::S][:Ts], leaky)
        for k in range(K):
            pd, st, close[s, k], leaks[s, k] = sample(tab, fwd, leaky, uniforms[s, k])
            pdfs[s, k, :Ts], states[s, k, :Ts + 1] = pd, st
    return pdfs, states, close, leaks


def enumerate_paths(tab, y, leaky):
    """Every latent path of a tiny graph, leaks included, in float64: a dict ``pdf sequence (tuple) -> probability``.  A path
    enters level ``t`` in ``pre_t`` and leaves it from ``post_t`` with weight ``[pre_t == post_t] + c pi(post_t)``; the
    per-frame ``1 / asum_t`` is common to all paths."""
    src, dst, pdf, w, pi, _, _ = tab
    y = np.asarray(y, np.float64)
    T, H = y.shape[0], len(pi)
    c = float(leaky)
    p = np.exp(np.clip(y, -OUTPUT_LIMIT, OUTPUT_LIMIT))
    out_arcs = [np.nonzero(src == h)[0] for h in range(H)]
    mass = {}

    def walk(pre, t, weight, pdfs):
        for post in range(H):
            step = (1.0 if post == pre else 0.0) + c * pi[post]
            if step == 0.0:
                continue
            if t == T:
                mass[pdfs] = mass.get(pdfs, 0.0) + weight * step
                continue
            for a in out_arcs[post]:
                walk(int(dst[a]), t + 1, weight * step * w[a] * p[t, pdf[a]], pdfs + (int(pdf[a]),))

    for h in range(H):
        if pi[h] > 0:
            walk(h, 0, pi[h], ())
    total = sum(mass.values())
    return {k: v / total for k, v in mass.items()}


def valid_sample(tab, pdfs, states, leaky):
    """Whether ``(pdfs (T,), states (T + 1, 2))`` is a latent path of the graph: ``pi(pre_0) > 0``, every
    ``(post_t -> pre_{t+1})`` an arc carrying ``pdf_t``, and ``pre_t == post_t`` wherever the coefficient is 0."""
    src, dst, pdf, w, pi, _, _ = tab
    T = len(pdfs)
    if (np.asarray(pdfs) < 0).any() or (np.asarray(states) < 0).any() or not pi[int(states[0, 0])] > 0:
        return False
    for t in range(T):
        if not ((src == states[t, 1]) & (dst == states[t + 1, 0]) & (pdf == pdfs[t]) & (w > 0)).any():
            return False
    return bool(leaky > 0 or (states[:, 0] == states[:, 1]).all())


def estimator_terms(pdfs, risks, T, P):
    """The centred estimator's per-sample terms for one sequence: ``(K, T, P)`` arrays ``g_k = K / (K - 1) * (r_k - mean r)
    * onehot(pdfs_k)`` whose mean over ``k`` is the estimate of ``grad E[r]`` (the gradient of
    ``functions.sampled_risk_surrogate``)."""
    K = len(risks)
    g = np.zeros((K, T, P))
    centred = (np.asarray(risks, np.float64) - np.mean(risks)) * K / (K - 1)
    for k in range(K):
        g[k, np.arange(T), pdfs[k]] = centred[k]
    return g


def boosted_reference(fst, tab, T, leaky, path_seed, y_seed):
    """A case for the estimator tests: ``(y (T, P) float32, ref (T,), exact)`` with ``ref`` a random path's pdfs, ``y`` a random
    output whose entries at ``ref`` are raised (steps of 1/8) until ``E[A] / T`` lies in 0.3 .. 0.7, and ``exact`` the float64
    ``den_accuracy_reference.recursion`` there (``acc``, ``gamma``, ``grad``)."""
    from torchain_amd import synth
    P = fst.num_pdfs
    arcs = dar.arcs_of(fst, tab[3])
    ref = dar.random_path(fst, tab[4], T, np.random.default_rng(path_seed))
    y0 = synth.random_nnet_output(1, T, P, seed=y_seed)
    for boost in np.arange(0.0, 12.0, 0.125):
        y = y0.copy()
        y[np.arange(T), ref] += np.float32(boost)
        exact = dar.recursion(arcs, tab[4], y, ref, None, leaky)
        if 0.3 <= exact["acc"] / T <= 0.7:
            break
    return y, ref, exact


def projections(terms, exact_grad, seed=77):
    """``[(estimate, exact, standard error)]`` of the estimator's per-sample ``terms`` ``(K, T, P)`` projected on the exact
    gradient's direction and on 8 fixed Gaussian directions; the standard error is that of the mean of the projected terms."""
    rng = np.random.default_rng(seed)
    dirs = [exact_grad / np.linalg.norm(exact_grad)] + [rng.normal(size=exact_grad.shape) for _ in range(8)]
    out = []
    for d in dirs:
        x = (terms * d[None]).sum(axis=(1, 2))
        out.append((float(x.mean()), float((exact_grad * d).sum()), float(x.std(ddof=1) / np.sqrt(len(x)))))
    return out
