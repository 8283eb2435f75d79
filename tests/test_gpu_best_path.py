"""Best-path alignment on the GPU (``csrc/num_best_path_kernels.hip`` through ``io.Supervision.best_path``) against the
float64 Viterbi of ``tests/best_path_reference.py``.  For every sequence:

(a) valid path: ``pdfs[s, :T_s]`` is emitted by some path of the acceptor (``path_score64 > -inf``), ``pdfs[s, T_s:] == -1``;
(b) optimal, by a derived bound: with ``M`` the maximum over the sequence's arcs and frames of ``|y| + |cost|`` and
    ``eps = T_s * 2**-23 * M``, ``|scores[s] - path_score64(pdfs[s])| <= eps`` and ``path_score64(pdfs[s]) >= best_score64 -
    2 * eps``.  The kernel rounds each ``y + logw`` once in float32 (``2**-24`` relative, so ``2**-24 * M`` a frame: half the
    bound); everything else is double.
(c) deterministic: two calls give identical ``pdfs`` and bit-identical ``scores``.

Which path is returned among paths of exactly equal score is not part of the contract.  Except where a sequence is built
without a path, ``best_score64`` is asserted finite for every sequence first, so that no test passes by skipping."""
import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import best_path, chain_loss

import best_path_reference as bp
import e2e_reference as ref
import wide_supervisions as ws

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PE = 60  # pdfs of the end-to-end cases


def _launches():
    return int(lib.tc_debug_counter(b"best_path_launches"))


def _call(sup, y):
    """(pdfs, scores) as numpy, from two calls that must agree to the bit (contract c); one launch each."""
    yt = y if isinstance(y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y)).to(DEV)
    before = _launches()
    p1, s1 = sup.best_path(yt)
    p2, s2 = sup.best_path(yt)
    torch.cuda.synchronize()
    assert _launches() == before + 2
    assert p1.dtype == torch.int32 and tuple(p1.shape) == (sup.n_batch, sup.n_frame) and p1.device == yt.device
    assert s1.dtype == torch.float64 and tuple(s1.shape) == (sup.n_batch,) and s1.device == yt.device
    assert torch.equal(p1, p2)
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    return p1.cpu().numpy(), s1.cpu().numpy()


def _rows(y, lens, s):
    """Sequence s's own frames of the (Tmax * S, P) matrix, as (T_s, P)."""
    return np.asarray(y)[np.arange(int(lens[s])) * len(lens) + s]


def _check(fsts, lens, y, pdfs, scores, no_path=()):
    """Contracts (a) and (b) for every sequence; the sequences in ``no_path`` must come back empty."""
    S = len(fsts)
    assert pdfs.shape == (S, max(lens)) and scores.shape == (S,)
    for s in range(S):
        T = int(lens[s])
        ys = _rows(y, lens, s)
        assert np.isfinite(ys).all()
        best = bp.best_score64(fsts[s], ys)
        if s in no_path:
            assert best == -np.inf
            assert scores[s] == -np.inf and (pdfs[s] == -1).all()
            continue
        assert np.isfinite(best), (s, best)  # (the input has a path: the kernel must find one)
        assert (pdfs[s, T:] == -1).all()
        row = pdfs[s, :T]
        assert (row >= 0).all(), (s, row)
        emitted = bp.path_score64(fsts[s], ys, row)
        eps = T * 2.0 ** -23 * bp.magnitude(fsts[s], ys)
        print("seq %d: T %d score %.17g emitted %.17g best %.17g eps %.3g" % (s, T, scores[s], emitted, best, eps))
        assert emitted > -np.inf, (s, row)
        assert abs(scores[s] - emitted) <= eps, (s, scores[s], emitted, eps)
        assert emitted >= best - 2 * eps, (s, emitted, best, eps)


def _y(S, T, P, seed, scale=2.0):
    return (np.random.default_rng(seed).normal(size=(S * T, P)) * scale).astype(np.float32)


def _nan_padding(y, lens):
    S, T = len(lens), max(lens)
    out = np.array(y, copy=True)
    out[(np.arange(T)[:, None] >= np.asarray(lens)[None, :]).reshape(T * S)] = np.nan
    return out


# ---- end-to-end supervisions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,T", [("chain", 37), ("chain", 38), ("random", 37), ("random", 38), ("random", 1)])
def test_e2e_uniform(kind, T):
    """Both parities of the score vectors' ping-pong, and one frame (the chain family's shortest path is longer than 1)."""
    S = 5
    fsts = ref.batch(kind, S, PE, seed=100 + T)
    y = _y(S, T, PE, seed=T)
    sup = io.Supervision.from_e2e_fsts(0.7, T, PE, fsts)
    pdfs, scores = _call(sup, y)
    _check(fsts, [T] * S, y, pdfs, scores)


def test_e2e_many_states_and_unreachable_states():
    """600 states and 2400 arcs: the loops over states strided by 256 and the lanes' loops over in-arcs run more than once;
    and states that the start cannot reach, one of them final (their scores stay -inf)."""
    rng = np.random.default_rng(3)
    T = 38
    big = ref.random_fst(600, 2400, PE, rng)
    assert len(big[5]) == 600 and big[1][-1] == 2400
    small = ref.random_fst(7, 20, PE, rng, pdf_pool=np.arange(50))
    cut = ref.with_unreachable_states(small, [55, 56], rng)
    fsts = [big, cut, ref.random_fst(5, 12, PE, rng)]
    y = _y(len(fsts), T, PE, seed=4)
    sup = io.Supervision.from_e2e_fsts(1.0, T, PE, fsts)
    pdfs, scores = _call(sup, y)
    _check(fsts, [T] * len(fsts), y, pdfs, scores)
    assert not np.isin(pdfs[1], [55, 56]).any()


def test_e2e_ragged_reads_nothing_in_the_padding():
    lens = [37, 9, 1, 20]
    fsts = ref.batch("random", len(lens), PE, seed=9)
    y = _y(len(lens), max(lens), PE, seed=10)
    sup = io.Supervision.from_e2e_fsts(1.0, lens, PE, fsts)
    assert sup.is_ragged
    pdfs, scores = _call(sup, _nan_padding(y, lens))
    _check(fsts, lens, y, pdfs, scores)
    clean, clean_scores = _call(sup, y)
    assert np.array_equal(pdfs, clean) and np.array_equal(scores, clean_scores)


def test_e2e_sequence_without_a_path_leaves_the_others_alone():
    S, T = 4, 12
    fsts = ref.batch("random", S, PE, seed=12)
    n = T + 4  # a linear acceptor longer than T: its only path has T + 3 arcs
    fsts[2] = ref._csr(n, [(i, i + 1, (3 * i) % PE, 0.25) for i in range(n - 1)], [np.inf] * (n - 1) + [0.0])
    y = _y(S, T, PE, seed=13)
    sup = io.Supervision.from_e2e_fsts(1.0, T, PE, fsts)
    pdfs, scores = _call(sup, y)
    _check(fsts, [T] * S, y, pdfs, scores, no_path=(2,))
    assert np.isfinite(scores[[0, 1, 3]]).all()


# ---- regular supervisions ----------------------------------------------------------------------------------------------
def test_regular_three_paths():
    S, T = 4, 20
    sup = synth.random_supervision(ws.den_fst(), S, T, 3, seed=21)
    y = synth.random_nnet_output(S, T, ws.P, seed=22, scale=2.0)
    pdfs, scores = _call(io.Supervision.from_synth(sup), y)
    _check(bp.split_merged(sup), [T] * S, y, pdfs, scores)


def test_regular_one_path_is_the_alignment():
    """One path a sequence: the answer is forced, which pins the traceback's indexing."""
    S, T = 4, 20
    sup = synth.random_supervision(ws.den_fst(), S, T, 1, seed=23)
    assert sup.num_states == S * T + 1 and len(sup.ilabel) == S * T  # (the merged FST is one line)
    y = synth.random_nnet_output(S, T, ws.P, seed=24, scale=2.0)
    pdfs, scores = _call(io.Supervision.from_synth(sup), y)
    assert np.array_equal(pdfs, (sup.ilabel - 1).reshape(S, T))
    _check(bp.split_merged(sup), [T] * S, y, pdfs, scores)


def test_regular_level_wider_than_the_workgroup():
    S, T = 2, 6
    sup = ws.lattice_supervision(S, T, ws.P, lambda q, t, r: 300, 3, seed=25)
    h = io.Supervision.from_synth(sup)
    assert h.stats()["max_level_states"] > 256
    y = synth.random_nnet_output(S, T, ws.P, seed=26, scale=2.0)
    pdfs, scores = _call(h, y)
    _check(bp.split_merged(sup), [T] * S, y, pdfs, scores)


def test_regular_ragged_gives_each_sequence_what_it_gets_alone():
    lens = [20, 7, 1, 13]
    pieces = [synth.random_supervision(ws.den_fst(), 1, T, 3, seed=30 + i, final_weights=True) for i, T in enumerate(lens)]
    fsts = [(p.arc_begin, p.ilabel, p.arc_weight, p.nextstate, p.final) for p in pieces]
    h = io.Supervision.from_fsts(1.0, lens, ws.P, fsts)
    assert h.is_ragged and not h.is_e2e
    y = synth.random_nnet_output(len(lens), max(lens), ws.P, seed=31, scale=2.0)
    pdfs, scores = _call(h, _nan_padding(y, lens))
    _check(fsts, lens, y, pdfs, scores)
    for s, piece in enumerate(pieces):
        alone, alone_score = _call(io.Supervision.from_synth(piece), np.ascontiguousarray(_rows(y, lens, s)))
        assert np.array_equal(pdfs[s, :lens[s]], alone[0])
        assert scores[s].tobytes() == alone_score[0].tobytes()


# ---- layouts -----------------------------------------------------------------------------------------------------------
def _handles():
    S, T = 4, 20
    reg = synth.random_supervision(ws.den_fst(), S, T, 3, seed=21)
    yield io.Supervision.from_synth(reg), ws.P
    yield io.Supervision.from_e2e_fsts(1.0, T, PE, ref.batch("random", S, PE, seed=41)), PE
    yield io.Supervision.from_e2e_fsts(1.0, [T, 3, 11, 1], PE, ref.batch("random", S, PE, seed=41)), PE


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def test_layouts_and_dtypes_give_the_2d_answer():
    for sup, P in _handles():
        S, T = sup.n_batch, sup.n_frame
        y2d = torch.from_numpy(_y(S, T, P, seed=42)).to(DEV)
        want = _call(sup, y2d)
        assert np.isfinite(want[1]).all()
        bct = y2d.view(T, S, P).permute(1, 2, 0).contiguous()  # (B, C, T)
        assert _same(_call(sup, bct), want)
        # a padded 2-D matrix: a row stride beyond the columns
        wide = torch.zeros(S * T, P + 5, device=DEV)
        wide[:, :P] = y2d
        assert _same(_call(sup, wide[:, :P]), want)
        # a (B, T, C) tensor passed as its transpose goes through .contiguous() in the Python entry
        btc = bct.permute(0, 2, 1).contiguous()
        got = best_path(btc.transpose(1, 2), sup)
        assert _same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
        for dtype in (torch.bfloat16, torch.float16):
            half = bct.to(dtype)
            rounded = half.float().permute(2, 0, 1).reshape(T * S, P).contiguous()  # the same values, 2-D float32
            assert _same(_call(sup, half), _call(sup, rounded))


# ---- the history is shared scratch -------------------------------------------------------------------------------------
def _step(den, sup, y):
    x = y.clone().requires_grad_(True)
    loss, res = chain_loss(x, den, sup, l2_regularize=5e-4, leaky_hmm_coefficient=0.1)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), res.data.clone(), x.grad.clone()


@pytest.mark.parametrize("kind", ["regular", "regular_windowed", "e2e"])
def test_training_step_is_the_same_after_best_path(kind, kernel_family):
    S, T = 4, 20
    if kind == "e2e":
        P = PE
        den = io.DenominatorGraph(synth.random_den_fst(80, 4, P, seed=31), P)
        sup = io.Supervision.from_e2e_fsts(0.7, T, P, ref.batch("random", S, P, seed=51))
    else:
        P = ws.P
        den = io.DenominatorGraph(ws.den_fst(), P)
        sup = io.Supervision.from_synth(synth.random_supervision(ws.den_fst(), S, T, 3, seed=52))
        if kind == "regular_windowed":  # (the numerator kernel that uses the history)
            kernel_family("force_num_windowed", 1)
    y = torch.from_numpy(_y(S, T, P, seed=53)).to(DEV)
    first = _step(den, sup, y)
    before = _launches()
    pdfs, scores = sup.best_path(y)
    assert _launches() == before + 1
    second = _step(den, sup, y)
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
    again = sup.best_path(y)  # ... and the other way round: the step leaves the alignment alone
    assert torch.equal(pdfs, again[0]) and torch.equal(scores.view(torch.int64), again[1].view(torch.int64))
    assert bool(torch.isfinite(scores).all())
