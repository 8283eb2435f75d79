"""The alignment entropy of regular supervisions with levels of any width on the GPU (``csrc/num_entropy_wide_kernels.hip``,
handles built with ``any_width=True``, through ``functions.num_path_entropy``): against the float64 recursion of
``tests/num_entropy_reference.py`` where the level-windowed entropy kernel refuses, and against that kernel bit for bit where
both serve (``force_num_entropy_wide``, ``force_num_entropy_wide_streamed``).  Inputs, layouts and calls are those of
``tests/test_gpu_num_entropy_regular.py``.

Tolerances, in that test's forms: a gradient element is held to ``8 * E_WIDE * D * |grad_output|`` plus the output format's
unit roundoff, the entropy to ``8 * E_WIDE * max(1, |E[log W]|)``.  ``E_WIDE`` is the largest error of
``Supervision.posteriors`` -- the parent commit's numerator (wide-level or resident, as the handle takes it), not the code
under test -- against a float64 forward-backward on ``WIDE``'s cases and inputs, measured on the MI355X
(``profiles/num_entropy_wide/README.md``, which also lists each case's MEASURED figures)."""
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss

import num_entropy_reference as ner
import test_gpu_num_entropy_regular as reg
import wide_supervisions as ws
from helpers import hip_num

pytestmark = pytest.mark.gpu
E_WIDE = 2.5591e-07  # profiles/num_entropy_wide/README.md
P = reg.P
ODD = 5 * 1024 + 37  # a thread owns several states, no multiple of the workgroup
_lattice = lambda widths, seed: ws.lattice_supervision(1, len(widths), P, lambda q, t, r: widths[t - 1], 1, seed=seed,  # noqa: E731
                                                       final_weights=True)
# name: (the pieces' level widths, or an int for a three-path trie of that many frames; the kernel's form)
WIDE = {
    "mid": ([(4, 3500, 4)], 1),
    "first_level": ([(3500, 4, 4)], 1),
    "last_level": ([(4, 4, 3500)], 1),  # the final-state loop is wide
    "adjacent": ([(4, ODD, ODD, 4)], 1),
    "beyond_lds": ([(4, 10500, 4)], 2),  # the slot form, by size
    "ragged": ([3, (4, 3500, 4, 4), 2], 1),  # the longest not last
}
_kernel = lambda sup: int(lib.tc_supervision_path_entropy_regular_kernel(sup.ptr))  # noqa: E731
_launches = lambda: tuple(int(lib.tc_debug_counter(k)) for k in (b"num_entropy_wide_launches", b"num_entropy_regular_launches"))  # noqa: E731


@functools.lru_cache(maxsize=None)
def _setup(case):
    """(handle, y (Tmax * S, P) float32 with row t * S + s, frames, reference), made once"""
    shapes, form = WIDE[case]
    pieces = [reg.trie(w, 3, 70 + i) if isinstance(w, int) else _lattice(w, 20 + i) for i, w in enumerate(shapes)]
    sup = io.Supervision.from_sequences(pieces, any_width=True) if len(pieces) > 1 else io.Supervision.from_synth(pieces[0], any_width=True)
    frames = [int(f) for f in sup.frames]
    y = np.random.default_rng(78).normal(0.0, 2.0, size=(max(frames) * len(pieces), P))
    y = (np.clip(np.round(y * 8), -32, 32) / 8).astype(np.float32)
    assert _kernel(sup) == form
    return sup, y, frames, ner.batch([reg._fst(p) for p in pieces], y.astype(np.float64), frames)


@pytest.mark.parametrize("case,layout", [(c, "2d") for c in WIDE] + [("adjacent", k) for k in reg.LAYOUTS if k != "2d"])
def test_against_float64_where_the_regular_kernel_refuses(case, layout):
    sup, y, frames, want = _setup(case)
    S, unit = len(frames), reg.LAYOUTS[layout][1]
    go = 1.5 - 1.25 * np.arange(S) if S > 1 else np.array([-1.25])  # (exact in every format; negative ones too)
    before = _launches()
    h, lp, g = reg._call(sup, reg._input(y, S, layout, frames), go)
    assert _launches() == (before[0] + 2, before[1])  # (forward, and the whole kernel in backward)
    assert (want["entropy"] > 0.05).all() and np.abs(want["grad"]).max() > 1e-3  # (the comparison is of something)
    h, lp, rows = h.cpu().numpy(), lp.cpu().numpy(), reg._rows(g, layout)
    for s in range(S):
        ref, err_h, err_lp = go[s] * want["grad"][s::S], abs(h[s] - want["entropy"][s]), abs(lp[s] - want["logprob"][s])
        bound = abs(go[s]) * 8 * E_WIDE * want["dev"][s] + unit * np.abs(ref) + (2.0 ** -25 if layout == "bct_f16" else 0)
        of_bound = (np.abs(rows[s::S] - ref) / bound).max()
        print("MEASURED seq %d entropy %.3e logprob %.3e grad %.3e, %.3f of its bound" % (s, err_h, err_lp, np.abs(rows[s::S] - ref).max(), of_bound))
        assert err_h <= 8 * E_WIDE * max(1.0, abs(want["elw"][s])) and err_lp <= 1e-4 * max(1.0, abs(want["logprob"][s]))
        assert of_bound <= 1.0
    pad = torch.from_numpy(np.arange(max(frames))[:, None] >= np.asarray(frames)[None, :]).to(reg.DEV)  # (T, S)
    g = g.view(max(frames), S, -1) if layout == "2d" else g.permute(2, 0, 1)
    assert not g[pad].float().view(torch.int32).any()  # +0 in the padding, NaN planted there


@pytest.mark.parametrize("layout", ["2d", "bct_bf16"])
@pytest.mark.parametrize("case", ["t1", "trie7", "states257", "uniq257", "shared_pdf", "ragged"])
def test_forced_gives_the_regular_kernels_bits(kernel_family, case, layout):
    sup, y, frames, _, _ = reg._setup(case)
    S = len(frames)
    x, go = reg._input(y, S, layout, frames), 1.5 - 1.25 * np.arange(S)
    assert _kernel(sup) == 0
    want = reg._call(sup, x, go)
    for form, switch in ((1, "force_num_entropy_wide"), (2, "force_num_entropy_wide_streamed")):
        kernel_family(switch, 1)
        before = _launches()
        got = reg._call(sup, x, go)
        assert _kernel(sup) == form and _launches() == (before[0] + 2, before[1])
        for a, b in zip(got, want):
            assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), (form, a, b)
    pad = torch.from_numpy(np.arange(max(frames))[:, None] >= np.asarray(frames)[None, :]).to(reg.DEV)
    g = got[2].view(max(frames), S, -1) if layout == "2d" else got[2].permute(2, 0, 1)
    assert not g[pad].float().view(torch.int32).any()


def test_logprob_is_the_numerators_and_the_handle_is_left_alone():
    sup, y, frames, _ = _setup("mid")
    x, den = reg._input(y, 1, "bct_f32"), io.DenominatorGraph(synth.random_den_fst(40, 3, P, seed=31), P)

    def step():
        z = x.clone().requires_grad_(True)
        loss, _ = chain_loss(z, den, sup, l2_regularize=1e-4, leaky_hmm_coefficient=0.1)
        loss.backward()
        return loss.detach(), z.grad

    before = step()
    _, lp, _ = reg._call(sup, x)
    assert all(torch.equal(a, b) for a, b in zip(before, step()))
    assert float(lp[0]) == hip_num(sup, y)["logprob_weighted"]  # (the supervision's weight is 1)


def test_failed_sequences_leave_their_neighbours_alone(kernel_family):
    T, pieces = 5, [reg.trie(5, 3, 20 + s) for s in range(4)]
    dead = pieces[1]  # every arc out of the start state at an infinite cost: no path
    pieces[1] = dead._replace(arc_weight=np.where(np.arange(len(dead.arc_weight)) < dead.arc_begin[1], np.inf, dead.arc_weight))
    x = reg._input(reg._setup("ragged")[1][:T * 4].copy(), 4, "bct_f32")
    x[2, int(pieces[2].ilabel[-1]) - 1, T - 1] = float("nan")  # the last frame of sequence 2, a pdf it reads there
    kernel_family("force_num_entropy_wide", 1)
    before = _launches()
    h, lp, g = reg._call(io.Supervision.from_sequences(pieces), x)
    assert torch.isnan(h[1]) and lp[1] == -np.inf and torch.isnan(h[2]) and torch.isnan(lp[2]) and not g[1:3].view(torch.int32).any()
    alone = reg._call(io.Supervision.from_sequences([pieces[0], pieces[3]]), x[[0, 3]])
    assert _launches() == (before[0] + 4, before[1])
    assert all(torch.equal(a[[0, 3]], b) for a, b in zip((h, lp, g), alone))
    assert torch.isfinite(alone[0]).all() and bool(alone[2].abs().max() > 0)
