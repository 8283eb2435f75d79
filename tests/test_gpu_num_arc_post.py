"""The arc occupations of end-to-end supervisions on the GPU (``csrc/num_arc_post_kernels.hip`` through
``functions.num_arc_posteriors`` / ``io.Supervision.arc_posteriors``) against the float64 recursion of
``tests/num_arc_post_reference.py``.

Tolerances.  An occupation is the numerator's: the float32 ``exp`` of a log-difference.  ``E_POST`` (``test_gpu_num_entropy``) and
``E`` (``test_gpu_num_entropy_large``) are the measured float64 errors of the NUMERATOR kernels' posteriors -- other code than
the code under test.  An arc's count and a final are held to ``8 * E * max(1, want)``, a sequence's ``arcs.sum()`` to ``8 * E *
T_s`` of ``T_s``, ``logprob`` with ``torch.equal`` to ``num_path_entropy``'s.  Inputs are multiples of 1/8 in +-4, exact in 16 bits,
so the reference of a 16-bit layout is the float32 one.  Which form serves a case follows from the resident limits (2048 states /
8192 arcs / 1024 distinct pdfs a sequence): ``terms_in_workspace``, 40000 arcs, takes the large form with or without the switch."""
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import TorchainHipError, lib
from torchain_amd.functions import chain_loss, num_arc_posteriors, num_path_entropy

import e2e_large_cases as lc
import e2e_reference as e2e
import num_arc_post_reference as apr
from test_gpu_num_entropy import CASES, E_POST, _input
from test_gpu_num_entropy_large import E, LARGE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the last register slot of the resident form beside an arc count that is no multiple of the workgroup
RESIDENT = dict(CASES, arcs8192=lambda r: ([e2e.random_fst(700, 8192, 30, r), e2e.random_fst(90, 1000, 30, r)], 5, 30, False))
BEYOND = ("states_past", "ragged", "states_at_limit")
counters = lambda: [int(lib.tc_debug_counter(k)) for k in (b"num_arc_post_launches", b"num_arc_post_large_launches")]  # noqa: E731


@functools.lru_cache(maxsize=None)
def _setup(case, beyond=False):
    """(handle, y (Tmax * S, P) float32 with row t * S + s, frames, reference, the form that serves it), made once"""
    fsts, frames, P, any_size = LARGE[case](np.random.default_rng(11)) + (True,) if beyond else RESIDENT[case](np.random.default_rng(11))
    sup = io.Supervision.from_e2e_fsts(1.0, frames if np.isscalar(frames) else np.asarray(frames, np.int32), P, fsts, any_size=any_size)
    frames = [frames] * len(fsts) if np.isscalar(frames) else list(frames)
    y = np.random.default_rng(77).normal(0.0, 2.0, size=(max(frames) * len(fsts), P))
    y = (np.clip(np.round(y * 8), -32, 32) / 8).astype(np.float32)
    large = any(n > lc.MAX_STATES or a > lc.MAX_ARCS or d > lc.MAX_PDFS for n, a, d in map(lc.sizes, fsts))
    return sup, y, frames, apr.batch(fsts, y.astype(np.float64), frames), int(large)


def _hold(post, want, frames, eps):
    """a call's arcs and finals against the reference's, each figure printed before it is held"""
    arcs, finals, ao, so = post.arcs.cpu().numpy(), post.finals.cpu().numpy(), post.arc_offsets.tolist(), post.state_offsets.tolist()
    assert post.arcs.dtype == post.finals.dtype == post.logprob.dtype == torch.float64 and len(ao) == len(so) == len(frames) + 1
    for s, ref in enumerate(want):
        a, f = arcs[ao[s]:ao[s + 1]], finals[so[s]:so[s + 1]]
        assert a.shape == ref["arcs"].shape and f.shape == ref["finals"].shape
        assert (ref["arcs"] > 1e-2).sum() >= 2  # (the comparison is of something)
        err_a = (np.abs(a - ref["arcs"]) / np.maximum(1.0, ref["arcs"])).max()
        err_f = (np.abs(f - ref["finals"]) / np.maximum(1.0, ref["finals"])).max()
        err_s = abs(a.sum() - frames[s]) / frames[s]
        print("MEASURED seq %d arcs %.3e finals %.3e sum %.3e (bound %.3e)" % (s, err_a, err_f, err_s, 8 * eps))
        assert err_a <= 8 * eps and err_f <= 8 * eps and err_s <= 8 * eps


@pytest.mark.parametrize("case,layout", [(c, k) for c in RESIDENT for k in ("2d", "bct_bf16")])
def test_against_float64(case, layout):
    sup, y, frames, want, large = _setup(case)
    x, n0 = _input(y, len(frames), layout, frames), counters()
    assert sup.arc_posteriors_kernel() == large
    post = num_arc_posteriors(x, sup)
    assert counters() == [n0[0] + 1 - large, n0[1] + large]
    assert torch.equal(post.logprob, num_path_entropy(x, sup)[1])
    _hold(post, want, frames, E_POST)
    assert torch.equal(sup.arc_posteriors(x).arcs, post.arcs)  # the method and the function: one entry


@pytest.mark.parametrize("case,layout", [(c, k) for c in RESIDENT for k in ("2d", "bct_bf16")])
def test_same_bits_from_both_forms(case, layout):
    sup, y, frames, _, large = _setup(case)
    x = _input(y, len(frames), layout, frames)
    plain, n0 = num_arc_posteriors(x, sup), counters()
    assert sup.arc_posteriors_kernel() == large and lib.tc_debug_set(b"force_num_arc_post_large", 1) == 0
    try:
        assert sup.arc_posteriors_kernel() == 1
        forced = num_arc_posteriors(x, sup)
    finally:
        assert lib.tc_debug_set(b"force_num_arc_post_large", 0) == 0
    assert counters() == [n0[0], n0[1] + 1]
    assert all(torch.equal(a, b) for a, b in zip(plain[:3], forced[:3]))


@pytest.mark.parametrize("case", BEYOND)
def test_against_float64_beyond_the_resident_limits(case):
    sup, y, frames, want, large = _setup(case, beyond=True)
    x = _input(y, len(frames), "2d", frames)
    assert large == 1 and sup.arc_posteriors_kernel() == 1
    if case == "states_past":
        den = io.DenominatorGraph(synth.random_den_fst(40, 3, 8, seed=31), 8)

        def step():
            z = x.clone().requires_grad_(True)
            loss, _ = chain_loss(z, den, sup, l2_regularize=1e-4, leaky_hmm_coefficient=0.1)
            loss.backward()
            return loss.detach(), z.grad

        before = step()
    post = num_arc_posteriors(x, sup)
    if case == "states_past":
        assert all(torch.equal(a, b) for a, b in zip(before, step()))  # the pool slot was left alone
    assert torch.equal(post.logprob, num_path_entropy(x, sup)[1])
    _hold(post, want, frames, E)


def test_failed_sequences_leave_their_neighbours_alone():
    T, P, rng = 5, 9, np.random.default_rng(5)
    fsts = [e2e.random_fst(6, 20, P, rng), lc.no_path(T + 2, 20, P, seed=6), e2e.random_fst(7, 25, P, rng)]
    x = _input(_setup("t7_cycles")[1][:T * 3].copy(), 3, "bct_f32")
    x[2, int(fsts[2][2][0]) - 1, T - 2] = float("nan")  # a valid frame of sequence 2, a pdf it reads
    post = num_arc_posteriors(x, io.Supervision.from_e2e_fsts(1.0, T, P, fsts))
    alone = num_arc_posteriors(x[:1], io.Supervision.from_e2e_fsts(1.0, T, P, fsts[:1]))
    a1, s1 = int(post.arc_offsets[1]), int(post.state_offsets[1])
    assert post.logprob[1] == -np.inf and torch.isnan(post.logprob[2])
    assert not post.arcs[a1:].view(torch.int64).any() and not post.finals[s1:].view(torch.int64).any()
    assert torch.equal(post.arcs[:a1], alone.arcs) and torch.equal(post.finals[:s1], alone.finals) and torch.equal(post.logprob[:1], alone.logprob)
    assert float(alone.arcs.sum()) > T - 1e-3


def test_a_regular_handle_is_refused():
    regular = io.Supervision.from_synth(synth.random_supervision(synth.random_den_fst(20, 3, 10, seed=3), 2, 6, 2, seed=4))
    with pytest.raises(TorchainHipError, match="regular") as err:
        num_arc_posteriors(torch.zeros(regular.n_batch * regular.n_frame, regular.n_pdf, device=DEV), regular)
    assert err.value.code == -3 and lib.tc_supervision_arc_posteriors_kernel(regular.ptr) == -3  # TC_ERR_UNSUPPORTED
