"""The alignment entropy of end-to-end supervisions on the GPU (``csrc/num_entropy_kernels.hip`` through
``functions.num_path_entropy`` / ``io.Supervision.path_entropy``) against the float64 recursion of
``tests/num_entropy_reference.py``.

Tolerances.  The error source is the numerator kernels' float32 ``exp`` of a log-difference.  ``E_POST`` is the largest error
of ``Supervision.posteriors`` -- the parent's numerator -- against float64 on ``CASES``, measured on the MI355X
(``profiles/num_entropy/README.md``).  A gradient element, a posterior times a deviation summed over a few arcs, is held to ``8 *
E_POST * D * |grad_output|``, ``D`` the reference's largest ``|Abar + r + Bbar - E[log W]|`` of the sequence; the entropy to ``8 *
E_POST * max(1, |E[log W]|)``; ``logprob``, the numerator's bits, to its ``1e-4 * max(1, |log Z|)``.  Inputs are
multiples of 1/8 in +-4, exact in 16 bits; a 16-bit gradient adds its format's unit roundoff (2**-8, 2**-11; float16: 2**-25)."""
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss, num_path_entropy

import e2e_reference as e2e
import num_entropy_reference as ner

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_POST = 1.1764e-07
LAYOUTS = {"2d": (torch.float32, 0.0), "bct_f32": (torch.float32, 0.0), "bct_bf16": (torch.bfloat16, 2.0 ** -8),
           "bct_f16": (torch.float16, 2.0 ** -11)}
# name: (FSTs, frames, pdfs, any_size), the smallest shapes at which the kernel takes another path
CASES = {
    "t1": lambda r: ([e2e.random_fst(6, 20, 9, r) for _ in range(2)], 1, 9, False),
    "t7_cycles": lambda r: ([e2e.random_fst(int(r.integers(3, 12)), 30, 9, r) for _ in range(3)], 7, 9, False),
    "states257": lambda r: ([e2e.random_fst(257, 700, 40, r), e2e.random_fst(5, 12, 40, r)], 6, 40, False),  # a thread owns two
    "pdfs257": lambda r: ([e2e.distinct_pdfs_fst(60, 500, 300, 257, r)], 4, 300, False),  # the second register slot
    "shared_pdf": lambda r: ([e2e.random_fst(8, 60, 5, r, pdf_pool=[0, 1, 2]), ner.tiny_fst()], 6, 5, False),  # and parallel arcs
    "ragged": lambda r: ([e2e.random_fst(7, 25, 9, r), ner.tiny_fst(), e2e.random_fst(7, 25, 9, r)], (7, 1, 7), 9, False),
    "terms_in_workspace": lambda r: ([e2e.random_fst(300, 40000, 50, r), e2e.random_fst(5, 12, 50, r)], 3, 50, True),  # 4 * 40000 > LDS
}


@functools.lru_cache(maxsize=None)
def _setup(case):
    """(handle, y (Tmax * S, P) float32 with row t * S + s, frames, reference), made once"""
    fsts, frames, P, any_size = CASES[case](np.random.default_rng(11))
    sup = io.Supervision.from_e2e_fsts(1.0, frames if np.isscalar(frames) else np.asarray(frames, np.int32), P, fsts, any_size=any_size)
    frames = [frames] * len(fsts) if np.isscalar(frames) else list(frames)
    y = np.random.default_rng(77).normal(0.0, 2.0, size=(max(frames) * len(fsts), P))
    y = (np.clip(np.round(y * 8), -32, 32) / 8).astype(np.float32)
    return sup, y, frames, ner.batch(fsts, y.astype(np.float64), frames)


def _input(y, S, layout, frames=()):
    """``y`` as the layout's tensor on the device, NaN in the frames behind ``frames[s]`` of sequence s"""
    x = torch.from_numpy(y).view(-1, S, y.shape[1]).clone()
    for s, n in enumerate(frames):
        x[n:, s] = float("nan")
    return (x.view(y.shape) if layout == "2d" else x.permute(1, 2, 0).contiguous()).to(device=DEV, dtype=LAYOUTS[layout][0])


def _rows(g, layout):
    """a tensor of the layout in float64 as (T * S, P), row t * S + s"""
    g = g.detach().double().cpu()
    return (g if layout == "2d" else g.permute(2, 0, 1).reshape(-1, g.shape[1])).numpy()


def _call(sup, x, grad_output=None):
    x = x.clone().requires_grad_(True)
    h, lp = num_path_entropy(x, sup)
    h.backward(torch.ones_like(h) if grad_output is None else torch.as_tensor(grad_output).to(DEV))
    torch.cuda.synchronize()
    assert h.dtype == lp.dtype == torch.float64 and not lp.requires_grad and x.grad.shape == x.shape and x.grad.dtype == x.dtype
    return h.detach(), lp, x.grad


def _hold(got, want, layout, go):
    """the three outputs of a call against ``ner.batch``'s, each figure printed before it is held"""
    h, lp, g, S = got[0].cpu().numpy(), got[1].cpu().numpy(), _rows(got[2], layout), len(go)
    for s in range(S):
        ref, err_h, err_lp = go[s] * want["grad"][s::S], abs(h[s] - want["entropy"][s]), abs(lp[s] - want["logprob"][s])
        bound = abs(go[s]) * 8 * E_POST * want["dev"][s] + LAYOUTS[layout][1] * np.abs(ref) + (2.0 ** -25 if layout == "bct_f16" else 0)
        of_bound = (np.abs(g[s::S] - ref) / bound).max()
        print("MEASURED seq %d entropy %.3e logprob %.3e grad %.3e, %.3f of its bound" % (s, err_h, err_lp, np.abs(g[s::S] - ref).max(), of_bound))
        assert err_h <= 8 * E_POST * max(1.0, abs(want["elw"][s])) and err_lp <= 1e-4 * max(1.0, abs(want["logprob"][s]))
        assert of_bound <= 1.0


@pytest.mark.parametrize("case,layout", [(c, k) for c in CASES for k in LAYOUTS])
def test_against_float64(case, layout):
    sup, y, frames, want = _setup(case)
    S = len(frames)
    go = np.ones(S) if layout == "2d" else 1.5 - 1.25 * np.arange(S)  # (exact in every format; negative ones too)
    got = _call(sup, _input(y, S, layout, frames), go)
    assert (want["entropy"] > 0.05).all() and np.abs(want["grad"]).max() > 1e-3  # (the comparison is of something)
    _hold(got, want, layout, go)
    pad = torch.from_numpy(np.arange(max(frames))[:, None] >= np.asarray(frames)[None, :]).to(DEV)  # (T, S)
    g = got[2].view(max(frames), S, -1) if layout == "2d" else got[2].permute(2, 0, 1)
    assert not g[pad].float().view(torch.int32).any()  # +0 in the padding, NaN planted there or not


@pytest.mark.parametrize("kind", ["single_path", "equal_parallel"])
def test_closed_forms(kind):
    T, P, m = 5, 4, 3
    if kind == "single_path":  # H = 0 up to the rounding of its one path, T float32 sums y - cost; no gradient
        fst = e2e._csr(T + 1, [(t, t + 1, t % P, 0.3 * t) for t in range(T)], [np.inf] * T + [0.4])
        y, want, eps = _setup("t7_cycles")[1][:T, :P].copy(), 0.0, T * 2.0 ** -23 * (4 + 0.3 * T)
    else:  # m equal arcs a frame and equal y: m ** T equally likely paths, so no covariance either
        fst = e2e._csr(1, [(0, 0, 1, 0.25)] * m, [0.125])
        y, want, eps = np.full((T, P), 0.5, np.float32), T * np.log(m), 8 * E_POST * max(1.0, abs(T * 0.25 - 0.125))
    h, _, g = _call(io.Supervision.from_e2e_fsts(1.0, T, P, [fst]), torch.from_numpy(y).to(DEV))
    print("MEASURED entropy error %.3e grad %.3e (bound %.3e)" % (abs(float(h[0]) - want), float(g.abs().max()), eps))
    assert abs(float(h[0]) - want) <= eps and float(g.abs().max()) <= eps


def test_failed_sequences_leave_their_neighbours_alone():
    T, P, rng = 5, 9, np.random.default_rng(5)
    no_path = e2e._csr(3, [(0, 1, 0, 0.1), (1, 2, 1, 0.2)], [np.inf, np.inf, 0.3])  # two arcs at most
    fsts = [e2e.random_fst(6, 20, P, rng), no_path, e2e.random_fst(7, 25, P, rng), e2e.random_fst(5, 15, P, rng)]
    x = _input(_setup("t7_cycles")[1][:T * 4].copy(), 4, "bct_f32")
    x[2, int(fsts[2][2][0]) - 1, T - 2] = float("nan")  # a valid frame of sequence 2, a pdf it reads
    h, lp, g = _call(io.Supervision.from_e2e_fsts(1.0, T, P, fsts), x)
    assert torch.isnan(h[1]) and lp[1] == -np.inf and torch.isnan(h[2]) and torch.isnan(lp[2]) and not g[1:3].view(torch.int32).any()
    alone = _call(io.Supervision.from_e2e_fsts(1.0, T, P, [fsts[0], fsts[3]]), x[[0, 3]])
    assert all(torch.equal(a[[0, 3]], b) for a, b in zip((h, lp, g), alone))
    _hold(alone, ner.batch([fsts[0], fsts[3]], _rows(x[[0, 3]], "bct_f32"), [T, T]), "bct_f32", np.ones(2))


def test_value_only_under_no_grad_and_the_handle_is_left_alone():
    sup, y, frames, _ = _setup("t7_cycles")
    x, den = _input(y, len(frames), "bct_f32"), io.DenominatorGraph(synth.random_den_fst(40, 3, 9, seed=31), 9)
    counter = lambda: int(lib.tc_debug_counter(b"num_entropy_launches"))  # noqa: E731

    def step():
        z = x.clone().requires_grad_(True)
        loss, _ = chain_loss(z, den, sup, l2_regularize=1e-4, leaky_hmm_coefficient=0.1)
        loss.backward()
        return loss.detach(), z.grad

    before, n0 = step(), counter()
    with torch.no_grad():
        quiet = num_path_entropy(x.clone().requires_grad_(True), sup)
    plain = sup.path_entropy(x)
    assert counter() == n0 + 2 and not quiet[0].requires_grad  # one launch each: the forward pass
    h, lp, _ = _call(sup, x)
    assert counter() == n0 + 4  # (forward, and the whole kernel in backward)
    assert all(torch.equal(a, b) for a, b in zip(quiet + plain, (h, lp, h, lp)))
    assert all(torch.equal(a, b) for a, b in zip(before, step()))
