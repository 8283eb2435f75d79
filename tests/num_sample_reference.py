"""Reference of the alignment sampler of a supervision (``io.Supervision.sample_paths`` / ``tc_supervision_sample_paths``).  A
helper, not a test module; plain numpy, no GPU.  An FST is ``tests/e2e_reference.py``'s CSR tuple ``(start, arc_begin, ilabel,
cost, nextstate, final cost)``; a regular sequence's acceptor has its states in time order, which are the handle's local states.

The model and the selection rule of ``include/torchain_hip.h``, literally.  The paths are those of exactly T arcs from the start
to a final state; ``lw = -cost`` and ``final_lw = -final cost`` are the handle's float32 values, ``sc_t(a) = lw_a + y_t(pdf_a)``
ONE float32 sum.  ``pick(weights, u)``: the first index whose inclusive cumulative sum exceeds ``u * total``, in doubles; the last
index of positive weight when rounding leaves none.  ``j_T = pick(exp(la_T(i) + final_lw(i) - log Z) over the states i, u[T])``
(a state that is not final, or not of the last level, weighs 0 and is never picked, so all states in state order serve both
kinds); for ``t = T - 1 .. 0`` the in-arcs of ``j_{t+1}`` -- by destination, stable by CSR position: the handle's in-lists --
each weighted ``exp((sc_t(a) + la_t(src_a)) - la_{t+1}(j_{t+1}))``, picked with ``u[t]``.  ``score = final_lw(j_T) + sum of
sc_t(a)`` in the order ``t = T - 1 .. 0``, float64: exact on both sides.

``forward`` keeps the library's stated arithmetic.  A regular handle's ``la`` is Kaldi's float64 ``LogAdd`` over the in-list in
order (``num_device.h``); an end-to-end handle's is ``max + log(float32 sum, in list order, of float32 exp(term - max))``
(``num_e2e_kernel``).  What is left between this and the kernel decides nothing unless a threshold is *close* to an end of the
chosen interval; ``sample`` flags such samples with ``delta``, derived, not tuned:

  regular: ``la`` is float64 on both sides.  A ``LogAdd`` is an ``exp`` and a ``log1p`` of at most 1 ulp each and an add, < 4 *
  2^-53 relative to a state's sum; a state's value takes D of them (D the largest in-degree) and hands its error on to the
  next level, so after T + 1 levels ``la`` is off by < 4 (T + 1) D 2^-53.  A weight is the ``exp`` of a difference of two such
  values, and a cumulative sum's share of its total moves by no more than twice a weight's relative error:
  ``delta = 8 (T + 2) D 2^-53``.
  end-to-end: the same argument with the numerator's float32 terms.  The device's float32 ``exp`` is within 2 ulp, and its
  argument, rounded to float32 on both sides, turns the incoming error into at most one more ulp of a term that matters (|x|
  e^-|x| < 1): < 4 * 2^-24 relative to a state's sum per level whatever the in-degree -- the float32 additions are the same on
  both sides -- so ``delta = 8 (T + 2) 4 * 2^-24`` (log Z's float32 sum, in another order on the device, is one more level)."""
import numpy as np

MIN_LOG_DIFF = -36.04365338911715  # Kaldi's kMinLogDiffDouble


def delta(T, max_in_degree, e2e):
    return 8.0 * (T + 2) * (4 * 2.0 ** -24 if e2e else max_in_degree * 2.0 ** -53)


def tables(fst):
    """``(start, src, dst, pdf, lw, final_lw, in_begin, in_order)``; ``lw``, ``final_lw`` float32; ``in_order[in_begin[j] :
    in_begin[j + 1]]`` are the in-arcs of state ``j`` in CSR order."""
    start, ab, il, cost, nx, final = fst
    n = len(final)
    src = np.repeat(np.arange(n), np.diff(ab))
    dst = np.asarray(nx, np.int64)
    begin = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    with np.errstate(invalid="ignore"):
        return (int(start), src, dst, np.asarray(il, np.int64) - 1, -np.asarray(cost, np.float32), -np.asarray(final, np.float32),
                begin, np.argsort(dst, kind="stable"))


def log_add(x, y):
    if x < y:
        x, y = y, x
    diff = y - x
    return x + np.log1p(np.exp(diff)) if diff >= MIN_LOG_DIFF else x


def forward(tab, y, e2e):
    """``(la (T + 1, n) float64, sc (T, arcs) float32, log Z)`` for the sequence's rows ``y`` ``(T, P)``, taken as float32"""
    start, src, dst, pdf, lw, final_lw, begin, order = tab
    y = np.asarray(y, np.float32)
    T, n = y.shape[0], len(final_lw)
    sc = lw[None, :] + y[:, pdf]  # float32, rounded once
    la = np.full((T + 1, n), -np.inf)
    la[0, start] = 0.0
    for t in range(T):
        term = la[t, src] + sc[t].astype(np.float64)
        live = np.zeros(n, bool)
        live[dst[np.isfinite(term)]] = True
        for j in np.flatnonzero(live):
            x = term[order[begin[j]:begin[j + 1]]]
            if e2e:
                mx = x.max()
                la[t + 1, j] = mx + np.log(np.float64(np.cumsum(np.exp((x - mx).astype(np.float32)), dtype=np.float32)[-1]))
            else:
                acc = -np.inf
                for v in x:
                    acc = log_add(acc, v)
                la[t + 1, j] = acc
    end = la[T] + final_lw.astype(np.float64)
    if e2e:
        mx = end.max()
        logz = mx + np.log(np.exp((end - mx).astype(np.float32)).astype(np.float64).sum()) if np.isfinite(mx) else -np.inf
    else:
        logz = -np.inf
        for v in end[np.isfinite(final_lw)]:
            logz = log_add(logz, v)
    return la, sc, float(logz)


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


def sample(tab, fwd, u, d):
    """One sample for the uniforms ``u`` (``>= T + 1``): ``(pdfs (T,), states (T + 1,), score, close, arcs (T,))``, ``arcs`` the
    CSR positions of the arcs taken"""
    start, src, dst, pdf, lw, final_lw, begin, order = tab
    la, sc, logz = fwd
    T = la.shape[0] - 1
    u = np.asarray(u, np.float32).astype(np.float64)
    pdfs, states, arcs = np.full(T, -1, np.int64), np.full(T + 1, -1, np.int64), np.full(T, -1, np.int64)
    with np.errstate(over="ignore"):
        j, close = pick(np.exp((la[T] + final_lw.astype(np.float64)) - logz), u[T], d)
    states[T], score = j, float(final_lw[j])
    for t in range(T - 1, -1, -1):
        ins = order[begin[j]:begin[j + 1]]
        i, c = pick(np.exp((sc[t, ins].astype(np.float64) + la[t, src[ins]]) - la[t + 1, j]), u[t], d)
        a = int(ins[i])
        close |= c
        score += float(sc[t, a])
        pdfs[t], arcs[t], j = pdf[a], a, int(src[a])
        states[t] = j
    return pdfs, states, score, close, arcs
