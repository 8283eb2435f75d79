"""The arc occupations of regular supervisions on the GPU (``csrc/num_arc_post_regular_kernels.hip`` through
``functions.num_arc_posteriors(..., regular=True)``) against the float64 recursion of ``tests/num_arc_post_regular_reference.py``
on each sequence's own acceptor and rows, element by element in the caller's CSR order: also the test of the output order.

Tolerances.  An occupation is the float32 ``exp`` of a log-difference, as the numerator's.  ``E_POST = 1.2558e-07`` is the measured
float64 error of the parent NUMERATOR's posteriors (``test_gpu_num_entropy_regular``): other code than the code under test.  Every
figure is held to ``8 * E_POST``, absolute below 1 and relative above.  Inputs are multiples of 1/8 in +-4, exact in 16 bits."""
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import TorchainHipError, lib
from torchain_amd.functions import chain_loss, num_arc_posteriors, num_path_entropy

import e2e_reference as e2e
import num_arc_post_regular_reference as ref
import wide_supervisions as ws
from test_gpu_num_entropy_regular import CASES, E_POST, _fst, _input, _setup, trie

pytestmark = pytest.mark.gpu


def spill_only(m=13, L=40, P=64):
    """1 -> L -> L -> L states, every pair of the middle levels joined by ``m`` parallel arcs: 20800 arcs leave one level"""
    rng = np.random.default_rng(9)
    nxt = np.r_[1 + np.arange(L), np.tile(np.repeat(1 + L + np.arange(L), m), L), (1 + 2 * L + (np.arange(L)[:, None] + [0, 1]) % L).ravel()]
    ab = np.cumsum(np.r_[0, L, np.full(L, L * m), np.full(L, 2), np.zeros(L, int)])
    final = np.r_[np.full(1 + 2 * L, np.inf), rng.integers(0, 16, L) / 8]
    return synth.SupFst(1.0, 1, 3, P, 1 + 3 * L, ab.astype(np.int32), rng.integers(1, P + 1, len(nxt)).astype(np.int32),
                        (rng.integers(0, 24, len(nxt)) / 8).astype(np.float32), nxt.astype(np.int32), final.astype(np.float32))


EXTRA = {
    # 25 x 41 = 1025 arcs leave level 1 (every pair: the fan is far beyond the widths): one past four register records a thread
    "arcs1025": lambda: ws.lattice_supervision(1, 3, 30, lambda q, t, r: (25, 41, 5)[t - 1], 100000, seed=4, final_weights=True),
    "spill_only": spill_only,
}
ALL = tuple(CASES) + tuple(EXTRA)
LAYOUTS = ("2d", "bct_bf16")
COUNTERS = (b"num_arc_post_regular_launches", b"num_arc_post_regular_spill_launches", b"num_launches")
counters = lambda: [int(lib.tc_debug_counter(k)) for k in COUNTERS]  # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(case):
    """(handle, y (Tmax * S, P) float32 with row t * S + s, frames, float64 reference, the form that serves it), made once"""
    if case in CASES:
        sup, y, frames, _, fsts = _setup(case)
    else:
        piece = EXTRA[case]()
        sup, fsts, frames = io.Supervision.from_synth(piece), [_fst(piece)], [piece.frames_per_sequence]
        y = np.random.default_rng(77).normal(0.0, 2.0, size=(frames[0], sup.n_pdf))
        y = (np.clip(np.round(y * 8), -32, 32) / 8).astype(np.float32)
    st = sup.stats()
    spill = 24 * (st["max_level_states"] + 1 & ~1) + 8 * (st["max_level_arcs"] + 3 & ~3) + 4 * (st["max_frame_uniq"] + 3 & ~3) + 2048 > 163840
    assert spill == (case == "spill_only") and st["kernel"] in ("resident", "windowed")  # (the numerator serves every case)
    assert case != "arcs1025" or st["max_level_arcs"] == 1025
    return sup, y, frames, ref.batch(fsts, y.astype(np.float64), frames), int(spill)


@pytest.mark.parametrize("case,layout", [(c, k) for c in ALL for k in LAYOUTS])
def test_against_float64(case, layout):
    sup, y, frames, want, spill = _case(case)
    x, n0 = _input(y, len(frames), layout, frames), counters()
    assert sup.arc_posteriors_kernel() == spill
    post = num_arc_posteriors(x, sup, regular=True)
    assert counters() == [n0[0] + 1 - spill, n0[1] + spill, n0[2]]
    assert torch.equal(post.logprob, num_path_entropy(x, sup)[1])
    arcs, finals, ao, so = post.arcs.cpu().numpy(), post.finals.cpu().numpy(), post.arc_offsets.tolist(), post.state_offsets.tolist()
    assert post.arcs.dtype == post.finals.dtype == post.logprob.dtype == torch.float64 and len(ao) == len(so) == len(frames) + 1
    for s, w in enumerate(want):
        a, f = arcs[ao[s]:ao[s + 1]], finals[so[s]:so[s + 1]]
        assert a.shape == w["arcs"].shape and f.shape == w["finals"].shape
        assert (w["arcs"] > 1e-2).sum() >= 2  # (the comparison is of something)
        err_a = (np.abs(a - w["arcs"]) / np.maximum(1.0, w["arcs"])).max()
        err_f = (np.abs(f - w["finals"]) / np.maximum(1.0, w["finals"])).max()
        err_s, err_1 = abs(a.sum() - frames[s]) / frames[s], abs(f.sum() - 1.0)
        print("MEASURED %s seq %d arcs %.3e finals %.3e arc sum %.3e final sum %.3e (bound %.3e)" % (case, s, err_a, err_f, err_s, err_1, 8 * E_POST))
        assert max(err_a, err_f, err_s, err_1) <= 8 * E_POST


@pytest.mark.parametrize("case,layout", [(c, k) for c in ALL for k in LAYOUTS])
def test_same_bits_from_both_forms(case, layout):
    sup, y, frames, _, spill = _case(case)
    x = _input(y, len(frames), layout, frames)
    plain, n0 = num_arc_posteriors(x, sup, regular=True), counters()
    assert sup.arc_posteriors_kernel() == spill and lib.tc_debug_set(b"force_num_arc_post_regular_spill", 1) == 0
    try:
        assert sup.arc_posteriors_kernel() == 1
        forced = num_arc_posteriors(x, sup, regular=True)
    finally:
        assert lib.tc_debug_set(b"force_num_arc_post_regular_spill", 0) == 0
    assert counters() == [n0[0], n0[1] + 1, n0[2]]
    assert all(torch.equal(a, b) for a, b in zip(plain[:3], forced[:3]))


@pytest.mark.parametrize("case,layout", [(c, k) for c in ALL for k in LAYOUTS])
def test_pooled_by_frame_and_pdf(case, layout):
    sup, y, frames, _, _ = _case(case)
    x, S, arc = _input(y, len(frames), layout, frames), len(frames), sup.arcs()
    post, want = num_arc_posteriors(x, sup, regular=True), sup.posteriors(x).double().cpu()
    index = torch.from_numpy((arc.frame.astype(np.int64) * S + arc.seq) * sup.n_pdf + arc.pdf)
    got = torch.zeros(want.numel(), dtype=torch.float64).index_add_(0, index, post.arcs.cpu()).view_as(want)
    err = float(((got - want).abs() / want.clamp(min=1.0)).max())
    print("MEASURED %s pooled %.3e (bound %.3e)" % (case, err, 8 * E_POST))
    assert float(want.sum()) > sum(frames) - 1e-3 and err <= 8 * E_POST


def test_failed_sequences_leave_their_neighbours_alone():
    pieces = [trie(5, 3, 20), trie(3, 3, 21), trie(4, 3, 22)]
    dead = pieces[1]  # every arc out of the start state at an infinite cost: no path
    pieces[1] = dead._replace(arc_weight=np.where(np.arange(len(dead.arc_weight)) < dead.arc_begin[1], np.inf, dead.arc_weight))
    x = _input(_setup("ragged")[1][:5 * 3].copy(), 3, "bct_f32")
    x[2, int(pieces[2].ilabel[-1]) - 1, 3] = float("nan")  # the last valid frame of sequence 2, a pdf it reads there
    post = num_arc_posteriors(x, io.Supervision.from_sequences(pieces), regular=True)
    alone = num_arc_posteriors(x[:1], io.Supervision.from_sequences(pieces[:1]), regular=True)
    a1, s1 = int(post.arc_offsets[1]), int(post.state_offsets[1])
    assert post.logprob[1] == -np.inf and torch.isnan(post.logprob[2])
    assert not post.arcs[a1:].view(torch.int64).any() and not post.finals[s1:].view(torch.int64).any()
    assert torch.equal(post.arcs[:a1], alone.arcs) and torch.equal(post.finals[:s1], alone.finals) and torch.equal(post.logprob[:1], alone.logprob)
    assert float(alone.arcs.sum()) > 5 - 1e-3


def test_the_pool_slot_is_left_alone():
    sup, y, frames, _, _ = _case("windowed")
    x, den = _input(y, 1, "bct_f32"), io.DenominatorGraph(synth.random_den_fst(40, 3, sup.n_pdf, seed=31), sup.n_pdf)

    def step():
        z = x.clone().requires_grad_(True)
        loss, _ = chain_loss(z, den, sup, l2_regularize=1e-4, leaky_hmm_coefficient=0.1)
        loss.backward()
        return loss.detach(), z.grad

    before = step()
    num_arc_posteriors(x, sup, regular=True)
    assert all(torch.equal(a, b) for a, b in zip(before, step()))


def test_the_keyword():
    sup, y, frames, _, _ = _case("trie7")
    with pytest.raises(TorchainHipError, match="regular") as err:
        num_arc_posteriors(_input(y, 1, "2d"), sup)
    assert err.value.code == -3  # TC_ERR_UNSUPPORTED, as before
    fsts = [e2e.random_fst(6, 20, 9, np.random.default_rng(5))]
    x, e2e_sup = _input(y[:5], 1, "2d"), io.Supervision.from_e2e_fsts(1.0, 5, 9, fsts)
    assert all(torch.equal(a, b) for a, b in zip(num_arc_posteriors(x, e2e_sup), num_arc_posteriors(x, e2e_sup, regular=True)))
