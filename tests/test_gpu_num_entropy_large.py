"""The alignment entropy of end-to-end supervisions beyond the resident kernel's size rule (``csrc/num_entropy_large_kernels.hip``
through ``functions.num_path_entropy`` / ``io.Supervision.path_entropy``): bit for bit against the resident kernel on the handles
that fit both, and against the float64 recursion of ``tests/num_entropy_reference.py`` at sizes only it serves.

Tolerances are ``test_gpu_num_entropy.py``'s in form: the entropy to ``8 * E * max(1, |E[log W]|)``, a gradient element to ``8 * E *
D * |grad_output|`` plus the 16-bit format's roundoff, ``logprob`` to ``1e-4 * max(1, |log Z|)``.  ``E`` is the largest error of
``Supervision.posteriors`` -- the large NUMERATOR kernel, not the code under test -- against float64 on ``LARGE``'s first three
cases, measured on the MI355X (``profiles/num_entropy_large/README.md``; the fourth case alone gives 1.98e-07 and is held to the
three's ``E`` all the same)."""
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss, num_path_entropy

import e2e_large_cases as lc
import e2e_reference as e2e
import num_entropy_reference as ner
from test_gpu_num_entropy import CASES, LAYOUTS, _call, _input, _rows, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = 1.2671e-07
PAST = lambda r: [e2e.random_fst(5060, 16000, 8, r), e2e.random_fst(5, 12, 8, r)]  # noqa: E731
# name: (FSTs, frames, pdfs); each large sequence beside a 5-state FST
LARGE = {
    "states_past": lambda r: (PAST(r), 10, 8),
    "at_limit": lambda r: (list(lc.mixed_fsts()) + [e2e.random_fst(5, 12, 7680, r)], 6, 7680),  # the rule met by two sequences
    "ragged": lambda r: (PAST(r), (10, 4), 8),
    "states_at_limit": lambda r: ([e2e.random_fst(10108, 32000, 4, r), e2e.random_fst(5, 12, 4, r)], 10, 4),  # SINGLE_PATH's stand-in
}
# at_limit's 10108-state sequence (``e2e_large_cases.MIXED[0]``: 1.2 arcs a state) has ONE path of 6 arcs, so its reference is
# H = 0 with no gradient whatever y is: it is held to its bounds like the others but cannot show that "the comparison is of
# something"; states_at_limit is that state count with three arcs a state, where it can.
SINGLE_PATH = ("at_limit", 0)
counters = lambda: [int(lib.tc_debug_counter(k)) for k in (b"num_entropy_launches", b"num_entropy_large_launches")]  # noqa: E731


@functools.lru_cache(maxsize=None)
def _large(case):
    """(handle, y (Tmax * S, P) float32 with row t * S + s, frames, reference), made once"""
    fsts, frames, P = LARGE[case](np.random.default_rng(11))
    sup = io.Supervision.from_e2e_fsts(1.0, frames if np.isscalar(frames) else np.asarray(frames, np.int32), P, fsts, any_size=True)
    frames = [frames] * len(fsts) if np.isscalar(frames) else list(frames)
    y = np.random.default_rng(77).normal(0.0, 2.0, size=(max(frames) * len(fsts), P))
    y = (np.clip(np.round(y * 8), -32, 32) / 8).astype(np.float32)
    return sup, y, frames, ner.batch(fsts, y.astype(np.float64), frames)


@pytest.mark.parametrize("case,layout", [(c, k) for c in CASES for k in ("2d", "bct_bf16")])
def test_same_bits_as_the_resident_kernel(case, layout):
    sup, y, frames, _ = _setup(case)
    S = len(frames)
    x, go = _input(y, S, layout, frames), 1.5 - 1.25 * np.arange(S)
    plain, n0 = _call(sup, x, go), counters()
    assert sup.path_entropy_kernel() == 0 and lib.tc_debug_set(b"force_num_entropy_large", 1) == 0
    try:
        assert sup.path_entropy_kernel() == 1
        forced = _call(sup, x, go)
        with torch.no_grad():
            quiet = num_path_entropy(x, sup)
    finally:
        assert lib.tc_debug_set(b"force_num_entropy_large", 0) == 0
    assert counters() == [n0[0], n0[1] + 3]  # (forward, the whole kernel in backward, the value under no_grad)
    assert all(torch.equal(a, b) for a, b in zip(plain + plain[:2], forced + quiet))


@pytest.mark.parametrize("case,layout", [(c, k) for c in LARGE for k in ("2d", "bct_bf16")])
def test_against_float64_beyond_the_resident_rule(case, layout):
    sup, y, frames, want = _large(case)
    S, fmt = len(frames), LAYOUTS[layout][1]
    assert sup.path_entropy_kernel() == 1
    spread = np.array([(case, s) != SINGLE_PATH for s in range(S)])
    assert (want["entropy"][spread] > 0.05).all() and (want["entropy"][~spread] == 0).all()  # (the comparison is of something)
    assert all(np.abs(want["grad"][s::S]).max() > 1e-3 for s in np.flatnonzero(spread))
    go = 1.5 - 1.25 * np.arange(S)
    x, n0 = _input(y, S, layout, frames), counters()
    if case == "states_past":
        den = io.DenominatorGraph(synth.random_den_fst(40, 3, 8, seed=31), 8)

        def step():
            z = x.clone().requires_grad_(True)
            loss, _ = chain_loss(z, den, sup, l2_regularize=1e-4, leaky_hmm_coefficient=0.1)
            loss.backward()
            return loss.detach(), z.grad

        before = step()
    h, lp, grad = _call(sup, x, go)
    assert counters() == [n0[0], n0[1] + 2]
    if case == "states_past":
        assert all(torch.equal(a, b) for a, b in zip(before, step()))  # the pool slot was left alone
    h, lp, g = h.cpu().numpy(), lp.cpu().numpy(), _rows(grad, layout)
    for s in range(S):
        ref, err_h, err_lp = go[s] * want["grad"][s::S], abs(h[s] - want["entropy"][s]), abs(lp[s] - want["logprob"][s])
        bound = abs(go[s]) * 8 * E * max(want["dev"][s], 1e-300) + fmt * np.abs(ref)  # (a single path: dev = 0, an exact 0 asked)
        of_bound = (np.abs(g[s::S] - ref) / bound).max()
        print("MEASURED seq %d entropy %.3e logprob %.3e grad %.3e, %.3f of its bound" % (s, err_h, err_lp, np.abs(g[s::S] - ref).max(), of_bound))
        assert err_h <= 8 * E * max(1.0, abs(want["elw"][s])) and err_lp <= 1e-4 * max(1.0, abs(want["logprob"][s]))
        assert of_bound <= 1.0
    pad = torch.from_numpy(np.arange(max(frames))[:, None] >= np.asarray(frames)[None, :]).to(DEV)  # (T, S)
    gv = grad.view(max(frames), S, -1) if layout == "2d" else grad.permute(2, 0, 1)
    assert not gv[pad].float().view(torch.int32).any()  # +0 in the padding, NaN planted there or not


def test_failed_sequences_leave_a_large_neighbour_alone():
    T, P, rng = 10, 8, np.random.default_rng(5)
    fsts = [e2e.random_fst(5060, 16000, P, rng), lc.no_path(T + 2, 20, P, seed=6), e2e.random_fst(5060, 16000, P, rng)]
    x = _input(_large("states_past")[1][:T * 2].reshape(T, 2, P)[:, [0, 1, 0]].reshape(T * 3, P).copy(), 3, "bct_f32")
    x[2, int(fsts[2][2][0]) - 1, T - 2] = float("nan")  # a valid frame of sequence 2, a pdf it reads
    sup = io.Supervision.from_e2e_fsts(1.0, T, P, fsts, any_size=True)
    h, lp, g = _call(sup, x)
    assert sup.path_entropy_kernel() == 1
    assert torch.isnan(h[1]) and lp[1] == -np.inf and torch.isnan(h[2]) and torch.isnan(lp[2]) and not g[1:3].view(torch.int32).any()
    alone = _call(io.Supervision.from_e2e_fsts(1.0, T, P, fsts[:1], any_size=True), x[:1])
    assert float(alone[0][0]) > 0.05 and all(torch.equal(a[:1], b) for a, b in zip((h, lp, g), alone))
