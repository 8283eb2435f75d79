"""Cases, oracle values and the host restatement of the per-sequence tests (``chain_loss(..., per_sequence=True,
on_failure="sequence")``, ``tc_chain_step_per_sequence``): a helper, not a test module.  ``test_per_sequence_host.py`` runs
without a GPU, ``test_gpu_per_sequence.py`` on one.

The graph is a tied one of 80 states over P = 64 pdfs, of the kind ``ragged_cases`` uses.  A case is a list of sequences,
regular (single-sequence ``synth.SupFst`` pieces) or end-to-end (per-sequence FSTs of ``e2e_reference``), in a uniform or a
ragged handle, T <= 11:

  reg_uniform   5 x 9      ``egs.append_supervisions`` of the pieces: the uniform regular handle
  e2e_uniform   5 x 9      ``from_e2e_fsts`` with one length
  reg_ragged    (7, 3, 4, 2, 7)              ``from_sequences``; 5 < 8: one workgroup per sequence
  e2e_ragged    (7, 3, 4, 2, 7)              ``from_e2e_fsts`` with the lengths
  reg_ragged8   (6, 3, 11, 5, 10, 4, 9, 11)  a ragged batch of 8: the denominator's two-workgroup route
  e2e_ragged8   the same lengths
  reg_uniform8, e2e_uniform8   8 x 6: the two two-workgroup forms of a uniform batch

``BAD[name]`` is the sequence the failure tests break (never the first, never the last, and in the ragged cases not the
longest, so that the tensors keep their shape).  Sequences do not interact, so the oracle (``oracle/pyoracle.py``; the float64
numerator of ``e2e_reference`` for end-to-end FSTs) is run on each sequence alone, on its own rows.

``finalize`` restates the masked scalar epilogue (``finalize_per_sequence_kernel``) in numpy: status bits, the kernel's
summation order and its float32 roundings.  Importing this module needs no GPU."""
import functools
from fractions import Fraction

import numpy as np

from torchain_amd import egs, io, synth

import e2e_reference as ref
import ragged_cases as rc

P = 64
WEIGHT, L2, LEAKY, XREG = 0.7, 5e-4, 0.1, 0.1
FIVE = (7, 3, 4, 2, 7)
EIGHT = (6, 3, 11, 5, 10, 4, 9, 11)

# name -> (kind, lengths, uniform handle)
CASES = {
    "reg_uniform": ("regular", (9,) * 5, True),
    "e2e_uniform": ("e2e", (9,) * 5, True),
    "reg_ragged": ("regular", FIVE, False),
    "e2e_ragged": ("e2e", FIVE, False),
    "reg_ragged8": ("regular", EIGHT, False),
    "e2e_ragged8": ("e2e", EIGHT, False),
    "reg_uniform8": ("regular", (6,) * 8, True),
    "e2e_uniform8": ("e2e", (6,) * 8, True),
}
BAD = {"reg_uniform": 2, "e2e_uniform": 1, "reg_ragged": 2, "e2e_ragged": 1, "reg_ragged8": 4, "e2e_ragged8": 6,
       "reg_uniform8": 3, "e2e_uniform8": 5}
HEALTHY = tuple(CASES)


def kind(name):
    return CASES[name][0]


def lengths(name):
    return CASES[name][1]


def uniform(name):
    return CASES[name][2]


@functools.lru_cache(maxsize=None)
def den_fst():
    return synth.random_den_fst(80, 4, P, seed=31)


@functools.lru_cache(maxsize=None)
def oracle_graph():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle.DenGraph(den_fst())


@functools.lru_cache(maxsize=None)
def pieces(name):
    """The case's sequences: single-sequence ``SupFst`` for a regular case, ``e2e_reference`` FSTs for an end-to-end one."""
    lens = lengths(name)
    seed0 = 1000 * (1 + sorted(CASES).index(name))
    if kind(name) == "e2e":
        return tuple(ref.batch("random", len(lens), P, seed=seed0))
    pi = oracle_graph().initial_probs()
    return tuple(synth.random_supervision(den_fst(), 1, T, 3, seed=seed0 + i, weight=WEIGHT, initial_probs=pi)
                 for i, T in enumerate(lens))


def no_path_fst(frames):
    """An end-to-end FST that is a chain of ``frames + 3`` states without self-loops, the last one final: its one path has
    ``frames + 2`` arcs, so no path has exactly ``frames`` -- a transcript too long for its utterance."""
    n = frames + 3
    arcs = [(i, i + 1, (5 * i + 3) % P, 0.5) for i in range(n - 1)]
    final = np.full(n, np.inf, np.float32)
    final[-1] = 0.0
    return ref._csr(n, arcs, final, start=0)


def handle(name, replace=None):
    """A fresh handle of the case; ``replace``: {sequence: piece} put in the place of the case's own."""
    seq = list(pieces(name))
    for s, piece in (replace or {}).items():
        seq[s] = piece
    lens = lengths(name)
    if kind(name) == "e2e":
        return io.Supervision.from_e2e_fsts(WEIGHT, lens[0] if uniform(name) else np.asarray(lens, np.int32), P, seq)
    if uniform(name):
        return io.Supervision.from_synth(egs.append_supervisions(seq))
    return io.Supervision.from_sequences(seq)


@functools.lru_cache(maxsize=None)
def nnet_output(name, scale=1.5):
    """(Tmax * S, P) float32 rows ``t * S + s``, finite everywhere; read-only (the tests change copies)."""
    lens = lengths(name)
    y = synth.random_nnet_output(len(lens), max(lens), P, seed=300 + sorted(CASES).index(name), scale=scale)
    y.setflags(write=False)
    return y


def rows_of(name, s):
    return rc.valid_rows(lengths(name), s)


def carried_pdf(name, s):
    """``(frame, pdf)``: a pdf that a numerator arc of sequence ``s`` carries in its frame 1 (every sequence of every case has
    two frames or more, so frame 1 is no padding)."""
    piece = pieces(name)[s]
    if kind(name) == "e2e":
        start, ab, il, _, nx, _ = piece
        first = {int(nx[a]) for a in range(ab[start], ab[start + 1])}
        for st in sorted(first):
            if ab[st + 1] > ab[st]:
                return 1, int(il[ab[st]]) - 1
        raise AssertionError("no second arc")
    # a regular piece is time-sorted: the arcs out of the states the start reaches are frame 1's
    nxt = {int(piece.nextstate[a]) for a in range(piece.arc_begin[0], piece.arc_begin[1])}
    st = min(nxt)
    return 1, int(piece.ilabel[piece.arc_begin[st]]) - 1


def uncarried_pdf(name, s):
    """A pdf no numerator arc of sequence ``s`` carries."""
    piece = pieces(name)[s]
    il = np.asarray(piece[2] if kind(name) == "e2e" else piece.ilabel) - 1
    free = np.setdiff1d(np.arange(P), il)
    assert free.size
    return int(free[0])


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    """The oracle on each sequence alone: float64 (S, 3) of (num_logprob, den_logprob, sum y^2), unweighted; read-only."""
    from oracle import pyoracle
    og = oracle_graph()
    y = nnet_output(name)
    out = np.zeros((len(lengths(name)), 3))
    for s, T in enumerate(lengths(name)):
        ys = np.ascontiguousarray(y[rows_of(name, s)])
        if kind(name) == "e2e":
            out[s, 0] = float(ref.num_logz([pieces(name)[s]], ys.astype(np.float64), T, want_gamma=False)[0][0])
        else:
            out[s, 0] = pyoracle.num_forward_backward(pieces(name)[s], ys, want_deriv=False)["logprob_weighted"] / WEIGHT
        den = pyoracle.den_forward_backward(og, ys, 1, leaky=LEAKY, want_deriv=False)
        assert den["ok"]
        out[s, 1] = den["logprob"]
        out[s, 2] = float((ys.astype(np.float64) ** 2).sum())
    out.setflags(write=False)
    return out


def oracle_objective(name, keep):
    """The oracle's batch objective of the sub-batch ``keep`` (sequence indices): dict(objf, l2_term, weight) in float64, the
    sum of the objective of each kept sequence alone, on its own rows."""
    from oracle import pyoracle
    og = oracle_graph()
    y = nnet_output(name)
    out = dict(objf=0.0, l2_term=0.0, weight=0.0)
    for s in keep:
        T = lengths(name)[s]
        ys = np.ascontiguousarray(y[rows_of(name, s)])
        if kind(name) == "e2e":
            one = ref.e2e_objective(og, [pieces(name)[s]], T, ys, weight=WEIGHT, l2=L2, leaky=LEAKY)
            assert one["ok"]
        else:
            one = pyoracle.compute_chain_objf_and_deriv(og, pieces(name)[s], ys, L2, LEAKY, want_deriv=False)
            assert np.isfinite(one["objf"]) and one["objf"] != -10.0 * one["weight"]
        for k in out:
            out[k] += float(one[k])
    return out


# ---- the masked scalar epilogue, restated -------------------------------------------------------------------------------------------
STATUS_NUM, STATUS_DEN, STATUS_AB = 1, 2, 4


def status_bits(num, den, y2, xent, ab=None, gs=None):
    """The kernel's rule: a scalar is bad when ``x - x != 0`` (NaN, +-inf).  1: numerator log-prob or cross-entropy sum; 2:
    denominator log-prob or sum y^2; 4: an alpha-beta check value (only when a derivative is formed)."""
    def bad(x):
        return ~np.isfinite(np.asarray(x, np.float64))
    st = np.zeros(len(num), np.int64)
    st |= np.where(bad(num) | bad(xent), STATUS_NUM, 0)
    st |= np.where(bad(den) | bad(y2), STATUS_DEN, 0)
    if ab is not None:
        st |= np.where(bad(ab) | bad(gs), STATUS_AB, 0)
    return st


def _ordered_sum(values, keep):
    """finalize_kernel's order: thread i adds sequences i, i + 256, ... to 0.0 in float64, thread 0 then adds the 256 partials in
    order; a masked-out term is an exact +0.0."""
    part = np.zeros(256)
    for s, v in enumerate(values):
        part[s % 256] = part[s % 256] + (np.float64(v) if keep[s] else np.float64(0.0))
    total = np.float64(0.0)
    for i in range(256):
        total = total + part[i]
    return total


def _round_f32(exact):
    """A Fraction rounded to float32 once, to nearest, ties to even."""
    c = np.float32(float(exact))
    best = None
    for cand in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - exact)
        even = (int(np.float32(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, cand, even)
    return np.float32(best[1])


def _scalars(D, N, Q, weight_f32, w, l2, checks_ok):
    f32 = np.float32
    with np.errstate(all="ignore"):
        numw = f32(np.float64(N) * np.float64(f32(w)))
        den = f32(D)
        if np.isfinite(numw) and np.isfinite(den):
            # one fused multiply-add, as the compiler contracts ``numw - w * den``: rounded once
            objf = _round_f32(Fraction(float(numw)) - Fraction(float(f32(w))) * Fraction(float(den)))
        else:
            objf = f32(numw - f32(w) * den)
        fail = int(not np.isfinite(objf) or not checks_ok)
        if fail:
            objf = f32(-10.0) * weight_f32
        l2_term = f32(0.0)
        if f32(l2) != 0:
            l2_term = f32(np.float64(-0.5) * np.float64(f32(w) * f32(l2)) * np.float64(f32(Q)))
    return objf, l2_term, fail


def finalize(num, den, y2, xent, frames, w, l2, T, ragged, isolate, status=None, checks_ok=True, survivors_ok=True):
    """``finalize_per_sequence_kernel`` on the sequences' own values (float64 arrays of S entries; ``frames``: their own
    lengths).  ``status``: the kernel's bits when they are known (they carry the alpha-beta bit, whose inputs
    ``per_sequence`` does not report), else formed from the values.  ``checks_ok`` / ``survivors_ok``: whether Kaldi's sum
    check |sum - count| <= 2 holds over all sequences / over the survivors -- the restatement is told, the sums of alpha-beta
    products are not among the reported values.  Returns dict(results float32[3], loss float32, xent float64, fail, masked,
    alive_frames int64[S], status)."""
    f32 = np.float32
    S = len(num)
    st = status_bits(num, den, y2, xent) if status is None else np.asarray(status, np.int64)
    alive = st == 0
    everyone = np.ones(S, bool)
    frames = np.asarray(frames, np.int64)
    total = int(frames.sum())
    weight_all = f32(w) * f32(total) if ragged else f32(w) * f32(S) * f32(T)
    all_checks = checks_ok and not (st & STATUS_AB).any()
    objf, l2_term, fail = _scalars(_ordered_sum(den, everyone), _ordered_sum(num, everyone), _ordered_sum(y2, everyone),
                                   weight_all, w, l2, all_checks)
    weight, X, masked = weight_all, _ordered_sum(xent, everyone), False
    n_alive = int(alive.sum())
    if isolate and 0 < n_alive < S:
        alive_frames = int(frames[alive].sum())
        weight_m = f32(w) * f32(alive_frames) if ragged else f32(w) * f32(n_alive) * f32(T)
        m_objf, m_l2, m_fail = _scalars(_ordered_sum(den, alive), _ordered_sum(num, alive), _ordered_sum(y2, alive), weight_m,
                                        w, l2, survivors_ok)
        if not m_fail:
            objf, l2_term, fail, weight, X, masked = m_objf, m_l2, 0, weight_m, _ordered_sum(xent, alive), True
    with np.errstate(all="ignore"):
        loss = f32(-objf) / f32(weight)
    return dict(results=np.array([objf, l2_term, weight], np.float32), loss=f32(loss), xent=0.0 if fail else float(X), fail=fail,
                masked=masked, alive_frames=np.where(alive, frames, 0) if masked else frames.copy(), status=st)


def finalize_from(seq, w, l2, T, ragged, isolate, mask=()):
    """``finalize`` fed with a ``PerSequence`` (``ChainResults.per_sequence``); ``mask``: sequences to treat as failed on top of
    the reported statuses (run B's values with the broken sequence masked out)."""
    st = seq.status.numpy().copy()
    for s in mask:
        st[s] |= STATUS_NUM
    return finalize(seq.num_logprob.numpy(), seq.den_logprob.numpy(), seq.sum_y2.numpy(), seq.xent_sum.numpy(), seq.frames.numpy(),
                    w, l2, T, ragged, isolate, status=st)
