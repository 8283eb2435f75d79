"""The alignment entropy of regular supervisions on the GPU (``csrc/num_entropy_regular_kernels.hip`` through
``functions.num_path_entropy`` / ``io.Supervision.path_entropy``) against the float64 recursion of
``tests/num_entropy_reference.py`` on each sequence's own acceptor and rows.

Tolerances, in the forms of ``tests/test_gpu_num_entropy.py``: the error source is the float32 ``exp`` of a log-difference.
``E_POST`` is the largest error of ``Supervision.posteriors`` -- the parent's regular numerator -- against float64 on ``CASES``,
measured on the MI355X (``profiles/num_entropy_regular/README.md``).  A gradient element is held to ``8 * E_POST * D *
|grad_output|``, ``D`` the reference's largest ``|Abar + r + Bbar - E[log W]|`` of the sequence, plus the output format's unit
roundoff (2**-8, 2**-11; float16: 2**-25); the entropy to ``8 * E_POST * max(1, |E[log W]|)``; ``logprob`` to EQUALITY with the
numerator's, whose device functions form it.  Inputs are multiples of 1/8 in +-4, exact in 16 bits."""
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss, num_path_entropy

import best_path_reference as bpr
import num_entropy_reference as ner
import wide_supervisions as ws

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_POST = 1.2558e-07
LAYOUTS = {"2d": (torch.float32, 0.0), "bct_f32": (torch.float32, 0.0), "bct_bf16": (torch.bfloat16, 2.0 ** -8),
           "bct_f16": (torch.float16, 2.0 ** -11)}
P = 9
trie = lambda T, k, seed, P=P, fw=True: synth.random_supervision(synth.random_den_fst(20, 3, P, seed=3), 1, T, k, seed=seed,  # noqa: E731
                                                                 final_weights=fw)


def _parallel(piece):
    """``piece`` with every third arc doubled at another cost: parallel arcs of one (frame, pdf) entry"""
    src = np.repeat(np.arange(piece.num_states), np.diff(piece.arc_begin))
    order = np.sort(np.r_[np.arange(len(src)), np.arange(0, len(src), 3)], kind="stable")
    cost = piece.arc_weight[order] + 0.375 * (np.r_[1, np.diff(order)] == 0)
    return piece._replace(arc_begin=np.searchsorted(src[order], np.arange(piece.num_states + 1)).astype(np.int32),
                          ilabel=piece.ilabel[order], arc_weight=cost.astype(np.float32), nextstate=piece.nextstate[order])


# name: (pieces, "single" | "ragged" | the merged SupFst), the smallest shapes at which the kernel takes another path
CASES = {
    "t1": lambda: ([trie(1, 4, 1)], "single"),
    "trie7": lambda: ([trie(7, 3, 5)], "single"),  # three paths, non-zero final weights
    # a level of 257 states -- a thread owns two -- beside a narrow sequence
    "states257": lambda: ([ws.lattice_supervision(1, 4, P, lambda q, t, r: 257 if t == 2 else 5, 2, seed=3, final_weights=True),
                           trie(4, 3, 4)], "ragged"),
    "uniq257": lambda: ([synth.random_supervision(synth.random_den_fst(300, 6, 400, seed=3), 1, 3, 600, seed=5)], "single"),
    "shared_pdf": lambda: ([_parallel(ws.lattice_supervision(1, 6, 3, lambda q, t, r: 4, 2, seed=6, final_weights=True))], "single"),
    "ragged": lambda: ([trie(7, 3, 7), trie(1, 4, 8), trie(4, 3, 9)], "ragged"),  # the longest not last
    "merged": lambda: (None, synth.random_supervision(synth.random_den_fst(20, 3, P, seed=3), 3, 5, 3, seed=14)),
    "windowed": lambda: ([ws.lattice_supervision(1, 40, 200, lambda q, t, r: 160, 3, seed=5, final_weights=True)], "single"),
}


def _fst(piece):
    return (0, piece.arc_begin, piece.ilabel, piece.arc_weight, piece.nextstate, piece.final)


@functools.lru_cache(maxsize=None)
def _setup(case):
    """(handle, y (Tmax * S, P) float32 with row t * S + s, frames, reference), made once"""
    pieces, kind = CASES[case]()
    if kind == "ragged":
        sup = io.Supervision.from_sequences(pieces)
    else:
        sup = io.Supervision.from_synth(pieces[0] if kind == "single" else kind)
    fsts = [_fst(p) for p in pieces] if pieces else [(0,) + f for f in bpr.split_merged(kind)]
    frames, stats = [int(f) for f in sup.frames], sup.stats()
    assert (case != "states257" or stats["max_level_states"] == 257) and (case != "uniq257" or stats["max_frame_uniq"] == 257)
    assert stats["kernel"] == ("windowed" if case == "windowed" else "resident")
    y = np.random.default_rng(77).normal(0.0, 2.0, size=(max(frames) * len(fsts), sup.n_pdf))
    y = (np.clip(np.round(y * 8), -32, 32) / 8).astype(np.float32)
    return sup, y, frames, ner.batch(fsts, y.astype(np.float64), frames), fsts


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
    sup, y, frames, want, _ = _setup(case)
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
    T, P4, m = 5, 4, 3
    if kind == "single_path":  # H = 0 up to the rounding of its one path, T float32 sums y + logw; no gradient
        sup = io.Supervision.from_alignments(1.0, np.arange(T)[None, :] % P4, P4)
        y, want, eps = _setup("trie7")[1][:T, :P4].copy(), 0.0, T * 2.0 ** -23 * 4
    else:  # m equal arcs a frame and equal y: m ** T equally likely paths, so no covariance either
        fst = (m * np.minimum(np.arange(T + 2), T), np.tile(np.arange(m) + 1, T), np.full(m * T, 0.25), np.repeat(np.arange(T) + 1, m),
               np.r_[np.full(T, np.inf), 0.125])
        sup = io.Supervision.from_fsts(1.0, [T], P4, [fst])
        y, want, eps = np.full((T, P4), 0.5, np.float32), T * np.log(m), 8 * E_POST * max(1.0, abs(T * 0.25 - 0.125))
    h, _, g = _call(sup, torch.from_numpy(y).to(DEV))
    print("MEASURED entropy error %.3e grad %.3e (bound %.3e)" % (abs(float(h[0]) - want), float(g.abs().max()), eps))
    assert abs(float(h[0]) - want) <= eps and float(g.abs().max()) <= eps


def test_failed_sequences_leave_their_neighbours_alone():
    T, pieces = 5, [trie(5, 3, 20 + s) for s in range(4)]
    dead = pieces[1]  # every arc out of the start state at an infinite cost: no path
    pieces[1] = dead._replace(arc_weight=np.where(np.arange(len(dead.arc_weight)) < dead.arc_begin[1], np.inf, dead.arc_weight))
    x = _input(_setup("ragged")[1][:T * 4].copy(), 4, "bct_f32")
    x[2, int(pieces[2].ilabel[-1]) - 1, T - 1] = float("nan")  # the last frame of sequence 2, a pdf it reads there
    h, lp, g = _call(io.Supervision.from_sequences(pieces), x)
    assert torch.isnan(h[1]) and lp[1] == -np.inf and torch.isnan(h[2]) and torch.isnan(lp[2]) and not g[1:3].view(torch.int32).any()
    alone = _call(io.Supervision.from_sequences([pieces[0], pieces[3]]), x[[0, 3]])
    assert all(torch.equal(a[[0, 3]], b) for a, b in zip((h, lp, g), alone))
    _hold(alone, ner.batch([_fst(pieces[0]), _fst(pieces[3])], _rows(x[[0, 3]], "bct_f32"), [T, T]), "bct_f32", np.ones(2))


@pytest.mark.parametrize("case", ["merged", "ragged"])
def test_value_only_under_no_grad_and_the_handle_is_left_alone(case):
    sup, y, frames, _, _ = _setup(case)
    x, den = _input(y, len(frames), "bct_f32"), io.DenominatorGraph(synth.random_den_fst(40, 3, P, seed=31), P)
    counter = lambda: int(lib.tc_debug_counter(b"num_entropy_regular_launches"))  # noqa: E731

    def step():
        z = x.clone().requires_grad_(True)
        loss, res = chain_loss(z, den, sup, l2_regularize=1e-4, leaky_hmm_coefficient=0.1, per_sequence=True)
        loss.backward()
        return loss.detach(), z.grad, res.per_sequence.num_logprob

    before, n0 = step(), counter()
    with torch.no_grad():
        quiet = num_path_entropy(x.clone().requires_grad_(True), sup)
    plain = sup.path_entropy(x)
    assert counter() == n0 + 2 and not quiet[0].requires_grad  # one launch each: the forward pass
    h, lp, _ = _call(sup, x)
    assert counter() == n0 + 4  # (forward, and the whole kernel in backward)
    assert all(torch.equal(a, b) for a, b in zip(quiet + plain, (h, lp, h, lp)))
    assert all(torch.equal(a, b) for a, b in zip(before, step()))
    assert torch.equal(lp.cpu(), before[2])  # the numerator's own bits (the supervision's weight is 1)
