"""Alignments sampled from a supervision's path posterior on the GPU (``csrc/num_sample_kernels.hip`` through
``functions.num_sample_paths`` / ``io.Supervision.sample_paths``) against the rule's float64 statement in
``tests/num_sample_reference.py``, on the end-to-end cases of ``test_gpu_num_entropy`` and the regular ones of
``test_gpu_num_entropy_regular`` and ``test_gpu_num_arc_post_regular``.

A sample the reference does not flag -- no threshold within ``delta * total`` of an end of its interval, ``delta`` derived in the
helper's docstring -- is held to EQUALITY: pdfs, states, and the score, which is exact by construction.  Flagged samples may be
at most 1 % of a case's samples; that the reference alone stays within that is checked without a GPU.  Inputs are multiples of
1/8 in +-4, exact in 16 bits, so one reference serves both layouts."""
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss, num_path_entropy, num_sample_paths

import e2e_large_cases as lc
import e2e_reference as e2e
import num_sample_reference as nsr
import test_gpu_num_entropy as ent
import test_gpu_num_entropy_regular as reg
from test_gpu_num_arc_post_regular import EXTRA

gpu = pytest.mark.gpu
DEV = "cuda:0"
K, K_MORE = 5, 9  # (5: not a multiple of the four waves)
ALL = ["e2e-" + c for c in ent.CASES] + ["reg-" + c for c in tuple(reg.CASES) + tuple(EXTRA)]
LAYOUTS = ("2d", "bct_bf16")
COUNTERS = (b"num_sample_launches", b"num_sample_streamed_launches", b"num_launches", b"best_path_launches")
counters = lambda: np.array([int(lib.tc_debug_counter(k)) for k in COUNTERS])  # noqa: E731


@functools.lru_cache(maxsize=None)
def _setup(case):
    """(handle, y (Tmax * S, P) float32 with row t * S + s, frames, FSTs, end-to-end?), made once"""
    kind, name = case.split("-")
    if kind == "e2e":
        sup, y, frames, _ = ent._setup(name)
        return sup, y, frames, ent.CASES[name](np.random.default_rng(11))[0], True
    if name in reg.CASES:
        sup, y, frames, _, fsts = reg._setup(name)
        return sup, y, frames, fsts, False
    piece = EXTRA[name]()
    sup = io.Supervision.from_synth(piece)
    y = np.random.default_rng(77).normal(0.0, 2.0, size=(piece.frames_per_sequence, sup.n_pdf))
    return sup, (np.clip(np.round(y * 8), -32, 32) / 8).astype(np.float32), [piece.frames_per_sequence], [reg._fst(piece)], False


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(uniforms (S, K_MORE, Tmax + 1) float32, per sequence and sample the reference's (pdfs, states, score, close)), made once"""
    _, y, frames, fsts, e2e_kind = _setup(case)
    S, u = len(fsts), np.random.default_rng(21).random((len(fsts), K_MORE, max(frames) + 1), dtype=np.float32)
    out = []
    for s, fst in enumerate(fsts):
        tab = nsr.tables(fst)
        fwd = nsr.forward(tab, y[s::S][:frames[s]], e2e_kind)
        d = nsr.delta(frames[s], int(np.diff(tab[6]).max()), e2e_kind)
        out.append([nsr.sample(tab, fwd, u[s, k], d)[:4] for k in range(K_MORE)])
    return u, out


def _call(case, layout="2d", k=K, seqs=None, sup=None):
    """``sample_paths`` with the first ``k`` of the case's uniforms (of the sequences ``seqs`` on the handle ``sup``)"""
    handle, y, frames, _, _ = _setup(case)
    x, u = ent._input(y, len(frames), layout, frames), torch.from_numpy(_reference(case)[0][:, :k]).to(DEV)
    if seqs is not None:  # (on their own handle: as many frames as the longest of them)
        T = max(frames[s] for s in seqs)
        x = x.view(max(frames), len(frames), -1)[:T, seqs].reshape(T * len(seqs), -1) if layout == "2d" else x[seqs][:, :, :T]
        u = u[seqs][:, :, :T + 1]
    got = num_sample_paths(x, handle if sup is None else sup, k, uniforms=u.contiguous(), return_states=True)
    torch.cuda.synchronize()
    assert (got.pdfs.dtype, got.states.dtype, got.scores.dtype, got.logprob.dtype) == (torch.int32, torch.int32, torch.float64, torch.float64)
    return got, x


def _same(a, b):
    return all(torch.equal(p.view(torch.int64) if p.dtype == torch.float64 else p, q.view(torch.int64) if q.dtype == torch.float64 else q)
               for p, q in zip(a, b))


@pytest.mark.parametrize("case", ALL)
def test_the_reference_alone_flags_at_most_one_percent(case):
    flagged = sum(smp[3] for seq in _reference(case)[1] for smp in seq)
    total = len(_reference(case)[1]) * K_MORE
    print("MEASURED %s: %d of %d samples flagged" % (case, flagged, total))
    assert flagged <= 0.01 * total


@gpu
@pytest.mark.parametrize("case,layout", [(c, k) for c in ALL for k in LAYOUTS])
def test_unflagged_samples_equal_the_reference(case, layout):
    sup, _, frames, _, _ = _setup(case)
    (got, x), want, Tm = _call(case, layout), _reference(case)[1], max(frames)
    pdfs, states, scores = got.pdfs.cpu().numpy(), got.states.cpu().numpy(), got.scores.cpu().numpy()
    assert pdfs.shape == (len(frames), K, Tm) and states.shape == (len(frames), K, Tm + 1) and scores.shape == (len(frames), K)
    assert torch.equal(got.logprob, num_path_entropy(x, sup)[1])  # the numerator's bits
    flagged = 0
    for s, T in enumerate(frames):
        assert (pdfs[s, :, T:] == -1).all() and (states[s, :, T + 1:] == -1).all()  # a ragged handle's padding
        for k in range(K):
            ref_pdfs, ref_states, ref_score, close = want[s][k]
            flagged += close
            assert close or ((pdfs[s, k, :T] == ref_pdfs).all() and (states[s, k, :T + 1] == ref_states).all()
                             and scores[s, k] == ref_score), (s, k)
    print("MEASURED %s %s: %d of %d samples flagged" % (case, layout, flagged, len(frames) * K))
    assert flagged <= 0.01 * len(frames) * K


@gpu
@pytest.mark.parametrize("case", ["e2e-t7_cycles", "reg-arcs1025"])  # (a full fan between wide levels: many paths)
def test_occupancies_follow_the_numerators_posteriors(case):
    sup, y, frames, _, _ = _setup(case)
    S, Tm, n = len(frames), max(frames), 4096
    x = ent._input(y, S, "2d", frames)
    got = sup.sample_paths(x, n, generator=torch.Generator(DEV).manual_seed(5))
    p = sup.posteriors(torch.nan_to_num(x)).double().view(Tm, S, -1)  # (the padding rows are not read)
    freq = torch.zeros_like(p)
    for s, T in enumerate(frames):
        t = torch.arange(T, device=DEV).repeat(n)
        freq[:, s].index_put_((t, got.pdfs[s, :, :T].reshape(-1).long()), torch.ones((), dtype=p.dtype, device=DEV), accumulate=True)
        p[T:, s] = 0
    err = ((freq / n - p).abs() - 5 * (p * (1 - p)).clamp_min(0).div(n).sqrt()).max().item()
    informative = int(((p > 0.05) & (p < 0.95)).sum())
    print("MEASURED %s: largest excess over 5 standard errors %.3e, %d informative cells" % (case, err, informative))
    assert err <= 1e-6 and informative >= 4  # (1e-6: the posteriors are float32)


@gpu
@pytest.mark.parametrize("case", ALL)
def test_one_sample_one_answer(case):
    sup, _, frames, fsts, e2e_kind = _setup(case)
    before = counters()
    staged, more = _call(case)[0], _call(case, k=K_MORE)[0]
    assert (counters() - before).tolist() == [2, 0, 0, 0] and sup.sample_paths_kernel() == 0
    assert lib.tc_debug_set(b"force_num_sample_streamed", 1) == 0
    try:
        assert sup.sample_paths_kernel() == 1
        streamed = _call(case)[0]
    finally:
        assert lib.tc_debug_set(b"force_num_sample_streamed", 0) == 0
    assert (counters() - before).tolist() == [3, 1, 0, 0]
    assert _same(staged, streamed)  # the two forms
    assert _same(staged, (more.pdfs[:, :K], more.scores[:, :K], more.logprob, more.states[:, :K]))  # sample k whatever K
    if len(frames) > 1:  # a sequence alone (the last: not the first of its batch)
        s = len(frames) - 1
        pad = (1.0, frames[s] if e2e_kind else [frames[s]], sup.n_pdf, [fsts[s] if e2e_kind else fsts[s][1:]])
        alone = _call(case, seqs=[s], sup=io.Supervision.from_e2e_fsts(*pad) if e2e_kind else io.Supervision.from_fsts(*pad))[0]
        T = frames[s]
        assert _same((staged.pdfs[s:, :, :T], staged.scores[s:], staged.logprob[s:], staged.states[s:, :, :T + 1]),
                     (alone.pdfs[..., :T], alone.scores, alone.logprob, alone.states[..., :T + 1]))


@gpu
def test_failed_sequences_leave_their_neighbours_alone():
    T, P, rng = 5, 9, np.random.default_rng(5)
    fsts = [e2e.random_fst(6, 20, P, rng), lc.no_path(T + 2, 20, P, seed=6), e2e.random_fst(7, 25, P, rng)]
    x = ent._input(ent._setup("t7_cycles")[1][:T * 3].copy(), 3, "bct_f32")
    x[2, int(fsts[2][2][0]) - 1, T - 2] = float("nan")  # a valid frame of sequence 2, a pdf it reads
    u = torch.rand((3, K, T + 1), generator=torch.Generator(DEV).manual_seed(9), device=DEV)
    got = num_sample_paths(x, io.Supervision.from_e2e_fsts(1.0, T, P, fsts), K, uniforms=u, return_states=True)
    alone = num_sample_paths(x[:1], io.Supervision.from_e2e_fsts(1.0, T, P, fsts[:1]), K, uniforms=u[:1], return_states=True)
    assert got.logprob[1] == -np.inf and torch.isnan(got.logprob[2]) and torch.isnan(got.scores[1:]).all()
    assert (got.pdfs[1:] == -1).all() and (got.states[1:] == -1).all()
    assert _same(tuple(v[:1] for v in got), alone) and (alone.pdfs >= 0).all() and torch.isfinite(alone.scores).all()


@gpu
@pytest.mark.parametrize("case", ["e2e-t7_cycles", "reg-merged"])
def test_the_pool_slot_is_left_alone(case):
    sup, y, frames, _, _ = _setup(case)
    x, den = ent._input(y, len(frames), "bct_f32"), io.DenominatorGraph(synth.random_den_fst(40, 3, sup.n_pdf, seed=31), sup.n_pdf)

    def step():
        z = x.clone().requires_grad_(True)
        loss, _ = chain_loss(z, den, sup, l2_regularize=1e-4, leaky_hmm_coefficient=0.1)
        loss.backward()
        return loss.detach(), z.grad

    before = step()
    assert (sup.sample_paths(x, K).pdfs >= 0).all()
    assert all(torch.equal(a, b) for a, b in zip(before, step()))
