"""Float64 statement of the end-to-end numerator ([K] GenericNumeratorComputation, chain-generic-numerator.cc) and of the
e2e chain objective ([K] ComputeChainObjfAndDerivE2e, chain-training.cc), plus synthetic e2e FSTs.

The numerator is a plain log-semiring forward over the per-sequence FSTs in torch float64, one frame at a time for
the whole batch; the posteriors are its gradient (autograd).  It shares nothing with the kernel's formulation
(probability domain, per-frame rescaling, hand-written backward).  The objective combines it with the denominator
oracle (oracle.pyoracle):  objf = w * sum_s log Z_s - w * den,  deriv = w * gamma_num - w * gamma_den - w * l2 * y,
xent_deriv = w * gamma_num;  any failure (numerator log Z not finite, denominator not ok, objf not finite) gives
objf = -10 * weight, deriv = -w * l2 * y, xent_deriv = 0.

An FST is ``(start, arc_begin, ilabel, arc_weight, nextstate, final)`` in CSR form: ilabel = pdf + 1, tropical
costs, final = inf for a state that is not final (``io.Supervision.from_e2e_fsts``)."""
import numpy as np
import torch

from oracle.independent_f64 import _segment_logsumexp


# ---- synthetic FSTs ------------------------------------------------------------------------------------------
def _csr(n, arcs, final, start=0):
    """arcs: list of (src, dst, pdf, cost) -> the CSR tuple (arcs sorted by source, stable)."""
    arcs = sorted(arcs, key=lambda a: a[0])
    counts = np.bincount([a[0] for a in arcs], minlength=n)
    arc_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ilabel = np.array([a[2] + 1 for a in arcs], np.int32)
    cost = np.array([a[3] for a in arcs], np.float32)
    nxt = np.array([a[1] for a in arcs], np.int32)
    return (int(start), arc_begin, ilabel, cost, nxt, np.asarray(final, np.float32))


def chain_fst(num_pdfs, rng, words=3, max_phones=3, silence=True, start_state=0):
    """Kaldi-chain-like left-to-right graph: every phone is one state entered by an arc of its forward pdf and left
    over a self-loop of its self-loop pdf; optional silence (its own forward / self-loop pdfs) between words and at the
    ends; small transition costs.  The shortest path has one arc per phone.  ``start_state`` renumbers the states so
    that the start is not state 0."""
    arcs = []
    n = 1
    cur_ends = [0]  # states a word may start from
    sil_f, sil_s = 0, 1

    def cost():
        return float(rng.uniform(0.0, 2.0))

    for w in range(words):
        if silence:
            sil = n
            n += 1
            for e in cur_ends:
                arcs.append((e, sil, sil_f, cost()))
            arcs.append((sil, sil, sil_s, cost()))
            cur_ends = cur_ends + [sil]
        prev = None
        for k in range(int(rng.integers(1, max_phones + 1))):
            st = n
            n += 1
            f, s = (int(x) for x in rng.integers(2, num_pdfs, size=2))
            for src in (cur_ends if prev is None else [prev]):
                arcs.append((src, st, f, cost()))
            arcs.append((st, st, s, cost()))
            prev = st
        cur_ends = [prev]
    final = np.full(n, np.inf, np.float32)
    final[cur_ends[-1]] = float(rng.uniform(0.0, 1.0))
    if silence:
        sil = n
        n += 1
        arcs.append((cur_ends[-1], sil, sil_f, cost()))
        arcs.append((sil, sil, sil_s, cost()))
        final = np.append(final, np.float32(0.5))
    # renumber so that the start becomes `start_state` (a rotation of the state ids)
    perm = (np.arange(n) + start_state) % n
    arcs = [(int(perm[a]), int(perm[b]), p, c) for a, b, p, c in arcs]
    fin = np.empty(n, np.float32)
    fin[perm] = final
    return _csr(n, arcs, fin, start=int(perm[0]))


def random_fst(num_states, num_arcs, num_pdfs, rng, pdf_pool=None):
    """Random epsilon-free acceptor with cycles: a ring through every state, a self-loop on the start (so every T
    has a path), random extra arcs; random final states including the start."""
    pool = np.arange(num_pdfs) if pdf_pool is None else np.asarray(pdf_pool)
    start = int(rng.integers(0, num_states))
    arcs = [(i, (i + 1) % num_states, int(rng.choice(pool)), float(rng.uniform(0, 3))) for i in range(num_states)]
    arcs.append((start, start, int(rng.choice(pool)), float(rng.uniform(0, 1))))
    for _ in range(max(0, num_arcs - len(arcs))):
        arcs.append((int(rng.integers(0, num_states)), int(rng.integers(0, num_states)), int(rng.choice(pool)),
                     float(rng.uniform(0, 3))))
    final = np.where(rng.random(num_states) < 0.3, rng.uniform(0, 2, num_states), np.inf).astype(np.float32)
    final[start] = 0.25
    return _csr(num_states, arcs, final, start=start)


def with_unreachable_states(fst, pdfs, rng, extra=4):
    """``fst`` plus ``extra`` states that no arc enters (so the start cannot reach them), each with arcs into the old states
    that carry ``pdfs`` -- pdfs no other arc carries, so they are among the FST's distinct pdfs and their posteriors are
    exactly 0 -- and one of them final."""
    start, ab, il, aw, nx, final = fst
    n = len(final)
    assert not np.isin(np.asarray(pdfs) + 1, il).any()
    new_il, new_aw, new_nx, new_ab = [], [], [], [int(ab[-1])]
    for _ in range(extra):
        for p in pdfs:
            new_il.append(int(p) + 1)
            new_aw.append(float(rng.uniform(0, 1)))
            new_nx.append(int(rng.integers(0, n)))
        new_ab.append(new_ab[-1] + len(pdfs))
    more_final = np.full(extra, np.inf, np.float32)
    more_final[-1] = 0.5
    return (start, np.concatenate([ab, new_ab[1:]]).astype(np.int32), np.concatenate([il, new_il]).astype(np.int32),
            np.concatenate([aw, new_aw]).astype(np.float32), np.concatenate([nx, new_nx]).astype(np.int32),
            np.concatenate([final, more_final]).astype(np.float32))


def distinct_pdfs_fst(num_states, num_arcs, num_pdfs, distinct, rng):
    """``random_fst`` whose arcs carry exactly the pdfs 0 .. ``distinct`` - 1, every one of them present."""
    fst = random_fst(num_states, num_arcs, num_pdfs, rng, pdf_pool=np.arange(distinct))
    fst[2][:distinct] = rng.permutation(distinct) + 1
    assert len(set(fst[2].tolist())) == distinct
    return fst


def batch(kind, S, num_pdfs, seed, **kw):
    rng = np.random.default_rng(seed)
    if kind == "chain":
        return [chain_fst(num_pdfs, rng, start_state=int(rng.integers(0, 3)), **kw) for _ in range(S)]
    return [random_fst(int(rng.integers(3, 12)), int(rng.integers(8, 40)), num_pdfs, rng, **kw) for _ in range(S)]


def shortest_path_arcs(fst):
    """Fewest arcs from the start to a final state (BFS)."""
    start, ab, _, _, nx, final = fst
    dist = {start: 0}
    frontier = [start]
    while frontier:
        nxt = []
        for s in frontier:
            if np.isfinite(final[s]):
                return dist[s]
            for a in range(ab[s], ab[s + 1]):
                if nx[a] not in dist:
                    dist[nx[a]] = dist[s] + 1
                    nxt.append(int(nx[a]))
        frontier = nxt
    return None


# ---- the numerator --------------------------------------------------------------------------------------------
def num_logz(fsts, y, T, want_gamma=True):
    """log Z_s of every sequence (float64 numpy [S]) and, with want_gamma, the posteriors d sum_s' log Z_s' / d y
    over the sequences whose log Z is finite ([S*T, P] float64; rows t*S + s)."""
    S = len(fsts)
    src, dst, pdf, cost, seq = [], [], [], [], []
    fin, st_seq, starts = [], [], []
    base = 0
    for s, (start, ab, il, aw, nx, final) in enumerate(fsts):
        n = len(final)
        src.append(np.repeat(np.arange(n), np.diff(ab)) + base)
        dst.append(np.asarray(nx) + base)
        pdf.append(np.asarray(il) - 1)
        cost.append(np.asarray(aw, np.float64))
        seq.append(np.full(len(il), s))
        fin.append(np.asarray(final, np.float64))
        st_seq.append(np.full(n, s))
        starts.append(base + start)
        base += n
    N = base
    src, dst, pdf, seq = (torch.from_numpy(np.concatenate(x).astype(np.int64)) for x in (src, dst, pdf, seq))
    cost = torch.from_numpy(np.concatenate(cost))
    fin = torch.from_numpy(np.concatenate(fin))
    st_seq = torch.from_numpy(np.concatenate(st_seq).astype(np.int64))
    yt = torch.tensor(np.asarray(y, np.float64), requires_grad=want_gamma)
    la = torch.full((N,), -np.inf, dtype=torch.float64)
    la[torch.tensor(starts)] = 0.0
    for t in range(T):
        term = la[src] - cost + yt[t * S + seq, pdf]
        la = _segment_logsumexp(term, dst, N)
    logz = _segment_logsumexp(la - fin, st_seq, S)
    gamma = None
    if want_gamma:
        ok = torch.isfinite(logz)
        if bool(ok.any()):
            (gamma,) = torch.autograd.grad(logz[ok].sum(), yt)
            gamma = gamma.numpy()
        else:
            gamma = np.zeros(yt.shape)
    return logz.detach().numpy(), gamma


def e2e_objective(den_graph, fsts, T, y, weight=1.0, l2=0.0, leaky=1e-5):
    """The full e2e objective; returns dict(objf, l2_term, weight, deriv, xent_deriv, logz, ok) in float64 (den
    graph: oracle.pyoracle.DenGraph)."""
    from oracle import pyoracle
    S = len(fsts)
    y = np.asarray(y, np.float32)
    logz, gamma = num_logz(fsts, y.astype(np.float64), T)
    den = pyoracle.den_forward_backward(den_graph, y, S, leaky=leaky, deriv_weight=-weight)
    num = weight * float(logz.sum())
    objf = num - weight * float(den["logprob"])
    tot_weight = weight * S * T
    y64 = y.astype(np.float64)
    l2_term = -0.5 * weight * l2 * float((y64 ** 2).sum()) if l2 else 0.0
    ok = bool(np.isfinite(logz).all()) and den["ok"] and np.isfinite(objf)
    if ok:
        deriv = weight * gamma + den["deriv"].astype(np.float64) - weight * l2 * y64
        xent = weight * gamma
    else:
        objf = -10.0 * tot_weight
        deriv = -weight * l2 * y64
        xent = np.zeros_like(y64)
    return dict(objf=objf, l2_term=l2_term, weight=tot_weight, deriv=deriv, xent_deriv=xent, logz=logz, ok=ok)


# ---- the end-to-end kernel's arithmetic, restated -----------------------------------------------------------------------------
def kernel_arithmetic(fst, y, weight=1.0):
    """What ``csrc/num_e2e_kernels.hip`` computes for one sequence, in numpy with the kernel's number formats: log alpha and
    log beta in double, an arc's score ``y - cost`` a float32 sum, every log-sum a maximum and a float32 sum (in arc order) of
    float32 ``exp`` of the float32 difference, occupations float32 ``exp`` of the float32 log-occupation summed per pdf in
    float32, and every frame divided by its own total.  ``y``: the sequence's rows, (T, P) float32.  Returns (log Z,
    weight * posteriors (T, P) float32).  ``exp`` is rounded correctly, so only the device's own is missing: what this differs from float64 by is what the
    kernel's formats cost, and the tolerance of the GPU test is set from it."""
    start, ab, il, aw, nx, final = fst
    f32, n, T = np.float32, len(final), y.shape[0]
    src, dst, pdf = np.repeat(np.arange(n), np.diff(ab)), np.asarray(nx), np.asarray(il) - 1
    lw, flw = -np.asarray(aw, f32), -np.asarray(final, f32).astype(np.float64)

    def exp32(x):
        """exp of a float32, rounded to float32 once (numpy's own float32 exp is a few ulp off)"""
        return np.exp(x.astype(f32).astype(np.float64)).astype(f32)

    def log_sum(x, index):
        """per index: max + log(float32 sum of float32 exp(x - max)); -inf for an empty or all -inf group"""
        mx = np.full(n, -np.inf)
        np.maximum.at(mx, index, x)
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.where(np.isfinite(mx[index]), exp32(x - mx[index]), f32(0))
            sm = np.zeros(n, f32)
            np.add.at(sm, index, e.astype(f32))
            return np.where(np.isfinite(mx), mx + np.log(sm.astype(np.float64)), -np.inf)

    alpha = np.full((T + 1, n), -np.inf)
    alpha[0, start] = 0.0
    score = [(lw + y[t, pdf]).astype(f32).astype(np.float64) for t in range(T)]
    for t in range(T):
        alpha[t + 1] = log_sum(alpha[t, src] + score[t], dst)
    x = alpha[T] + flw
    logz = x.max() + np.log(np.float64(exp32(x - x.max()).sum(dtype=f32)))
    beta = flw
    post = np.zeros(y.shape, f32)
    for t in range(T - 1, -1, -1):
        x = score[t] + beta[dst]
        with np.errstate(invalid="ignore"):
            occ = exp32((alpha[t, src] - logz) + x)
        g = np.zeros(y.shape[1], f32)
        np.add.at(g, pdf, np.where(np.isnan(occ), f32(0), occ).astype(f32))
        post[t] = g * (f32(weight) / g.sum(dtype=f32))
        beta = log_sum(x, src)
    return float(logz), post
