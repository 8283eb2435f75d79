"""The wide-level numerator kernel (``csrc/num_wide_kernels.hip``, ``any_width=True``) on the GPU, against the CPU oracle's
float64 numerator and objective under ``REL`` where every other kernel refuses, and against the windowed kernel bit for bit
where both serve (``force_num_wide``).  Every case states its size through ``stats()``; the launch counter shows the kernel."""
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import ChainResults, chain_loss, compute_chain_objf_and_deriv

import ragged_cases as rc
import wide_supervisions as ws
from helpers import REL, hip_num, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = ws.P
ODD = 5 * 1024 + 37  # beyond the window (32 bytes a state), no multiple of the workgroup
# (a sequence takes the wide kernel when it is also beyond the resident kernel: 16 bytes a state and 4 an arc of all its levels)
FORMS = [("2d", torch.float32), ("3d", torch.float32), ("3d", torch.bfloat16), ("3d", torch.float16)]
# name -> the widths of levels 1 .. T
SHAPES = dict(case1=(4, 12000, 4), first_level=(9000, 4, 4), last_level=(4, 4, 9000), adjacent=(4, ODD, ODD, 4),
              odd_width=(1500, ODD, 1500), narrow_neighbours=(3, 9000, 5), beyond_lds=(4, 21000, 4))


_wide = functools.partial(lib.tc_debug_counter, b"num_wide_launches")


@functools.lru_cache(maxsize=None)
def _graph():
    return io.DenominatorGraph(ws.den_fst(), P).prepare(DEV)


@functools.lru_cache(maxsize=None)
def _case(name, seed=1):
    """(the supervision FST, its outputs): one sequence with the widths of SHAPES[name]."""
    widths = SHAPES[name]
    sup = ws.lattice_supervision(1, len(widths), P, lambda q, t, r: widths[t - 1], 1, seed=seed, final_weights=True)
    return sup, synth.random_nnet_output(1, len(widths), P, seed=seed + 7)


def _handle(sup, form="lds"):
    h = io.Supervision.from_synth(sup, any_width=True)
    st = h.stats()
    print(st, h.wide_stats())
    assert (st["kernel"], h.wide_stats()["form"]) == ("wide", form), st
    return h


def _against_the_oracle(oracle, sup, y, h):
    ref = oracle.num_forward_backward(sup, y)
    before = _wide()
    out, fwd = hip_num(h, y), hip_num(h, y, want_deriv=False)
    assert _wide() - before == 2
    assert abs(out["logprob_weighted"] - ref["logprob_weighted"]) <= REL * abs(ref["logprob_weighted"])
    assert fwd["logprob_weighted"] == out["logprob_weighted"] and fwd["deriv"] is None
    assert rel_err(out["deriv"], ref["deriv"], floor=sup.weight) <= REL
    assert np.abs(out["deriv"].sum(axis=1, dtype=np.float64) / sup.weight - 1).max() <= 1e-4  # a frame's posteriors sum to one
    return out


@pytest.mark.parametrize("name", [k for k in SHAPES if k != "beyond_lds"])
def test_numerator_matches_the_oracle_where_the_others_refuse(oracle, name):
    """case1 is the 12000-state level the host test pins as unsupported without the flag; the others move the wide level."""
    sup, y = _case(name)
    assert io.Supervision.from_synth(sup).stats()["kernel"] == "unsupported"
    _against_the_oracle(oracle, sup, y, _handle(sup))


def test_slot_form(oracle, kernel_family):
    """A 21000-state level is beyond the LDS form; and forced onto case1, the slot form gives the LDS form's bits."""
    sup, y = _case("beyond_lds")
    _against_the_oracle(oracle, sup, y, _handle(sup, "slot"))
    sup, y = _case("case1")
    a = hip_num(_handle(sup), y)
    kernel_family("force_num_wide_streamed", 1)
    before = _wide()
    b = hip_num(_handle(sup, "slot"), y)
    assert _wide() - before == 1
    assert a["logprob_weighted"] == b["logprob_weighted"] and np.array_equal(a["deriv"].view(np.int32), b["deriv"].view(np.int32))


def test_ragged_batch_has_each_sequence_alone_bits():
    """Three sequences of lengths 3, 5, 2 with their wide level at frames 2, 5 and 1: every sequence's rows are the call's
    on it alone, the padding stays +0, and a NaN in a padding frame reaches nothing."""
    lens = (3, 5, 2)
    widths = [(4, 9001, 4), (4, 4, 4, 4, 9000), (9500, 4)]
    pieces = [ws.lattice_supervision(1, len(w), P, lambda q, t, r, w=w: w[t - 1], 1, seed=20 + i, final_weights=True)
              for i, w in enumerate(widths)]
    h = io.Supervision.from_sequences(pieces, any_width=True)
    assert h.stats()["kernel"] == "wide" and h.is_ragged
    y = synth.random_nnet_output(len(lens), max(lens), P, seed=31)
    before = _wide()
    out = hip_num(h, y)
    assert _wide() - before == 1
    valid = np.zeros(len(y), bool)
    total = 0.0
    for s, piece in enumerate(pieces):
        rows = rc.valid_rows(lens, s)
        valid[rows] = True
        alone = hip_num(_handle(piece), np.ascontiguousarray(y[rows]))
        assert np.array_equal(out["deriv"][rows].view(np.int32), alone["deriv"].view(np.int32)), s
        total += alone["logprob_weighted"]
    assert abs(out["logprob_weighted"] - total) <= 1e-12 * abs(total)
    assert not valid.all() and not out["deriv"][~valid].view(np.int32).any()
    poisoned = y.copy()
    poisoned[~valid] = np.nan
    again = hip_num(h, poisoned)
    assert again["logprob_weighted"] == out["logprob_weighted"]
    assert np.array_equal(again["deriv"].view(np.int32), out["deriv"].view(np.int32))


def _layout(y2d, S, T, layout, dtype):
    y = torch.as_tensor(y2d).to(DEV).to(dtype)
    return (y.view(T, S, -1).permute(1, 2, 0).contiguous() if layout == "3d" else y.clone()).requires_grad_(True)


def _step(h, name, form, xent):
    sup, (layout, dtype) = ws.supervision(name), form
    S, T = sup.num_sequences, sup.frames_per_sequence
    x, xe = (_layout(ws.nnet_output(name, seed=s), S, T, layout, dtype) for s in (5, 6))
    kw = dict(xent_regularize=0.1, xent_input=xe, kaldi_way=True) if xent else {}
    loss, res = chain_loss(x, _graph(), h, l2_regularize=5e-5, leaky_hmm_coefficient=0.1, **kw)
    loss.sum().backward()
    return [loss.detach(), res.data.clone(), torch.tensor(float(res.xent_objf) if xent else 0.0, dtype=torch.float64), x.grad,
            xe.grad if xent else torch.zeros(1)]


@pytest.mark.parametrize("xent", [False, True], ids=["mmi", "kaldi_way"])
@pytest.mark.parametrize("form", FORMS, ids=["2d-f32", "3d-f32", "3d-bf16", "3d-f16"])
def test_forced_chain_loss_gives_the_windowed_bits(kernel_family, form, xent):
    """lattice_bursty fits the resident kernel: with any_width and no switch it takes the kernel it took (no wide launch);
    under force_num_wide every output of chain_loss + backward has the bits of the windowed kernel (force_num_windowed)."""
    name = "lattice_bursty"
    plain = io.Supervision.from_synth(ws.supervision(name), any_width=True)
    assert plain.stats()["kernel"] == ws.expected_kernel(name)
    before = _wide(), lib.tc_debug_counter(b"num_windowed_launches")
    unforced = _step(plain, name, form, xent)
    kernel_family("force_num_windowed", 1)
    windowed = _step(io.Supervision.from_synth(ws.supervision(name)), name, form, xent)
    assert (_wide(), lib.tc_debug_counter(b"num_windowed_launches")) == (before[0], before[1] + 1)
    kernel_family("force_num_windowed", 0)
    kernel_family("force_num_wide", 1)
    wide = _step(_handle(ws.supervision(name)), name, form, xent)
    assert (_wide(), lib.tc_debug_counter(b"num_windowed_launches")) == (before[0] + 1, before[1] + 1)
    for what, u, w, v in zip(("loss", "results", "xent objective", "grad", "xent grad"), unforced, windowed, wide):
        for got in (u, v):  # (byte for byte)
            assert got.dtype == w.dtype and torch.equal(got.reshape(-1).view(torch.uint8), w.reshape(-1).view(torch.uint8)), what
    assert float(wide[1][0]) != -10.0 * float(wide[1][2])  # (not the soft failure: the gradients are the numerator's)


def test_full_objective_matches_the_oracle(oracle):
    """tests/test_gpu_num_windowed.py's _check_against_oracle on case1's handle: xent, l2 and leaky-HMM."""
    (sup, y), l2, leaky = _case("case1"), 5e-5, 0.1
    ref = oracle.compute_chain_objf_and_deriv(oracle.DenGraph(ws.den_fst()), sup, y, l2, leaky, want_xent=True)
    yt = torch.from_numpy(y).to(DEV)
    deriv, xd, res, before = torch.full_like(yt, 7.0), torch.full_like(yt, 7.0), ChainResults(), _wide()
    compute_chain_objf_and_deriv(_graph(), _handle(sup), yt, res.data, deriv, xd, l2, leaky, 0.1)
    torch.cuda.synchronize()
    got = res.data.numpy()
    assert _wide() - before == 1
    assert abs(got[0] - ref["objf"]) <= REL * abs(ref["objf"]), (got, ref["results"])
    assert abs(got[1] - ref["l2_term"]) <= REL * max(abs(ref["l2_term"]), 1e-30), (got, ref["results"])
    assert got[2] == ref["weight"] == np.float32(sup.weight * len(SHAPES["case1"]))
    assert rel_err(deriv.cpu().numpy(), ref["deriv"], floor=sup.weight) <= REL
    assert rel_err(xd.cpu().numpy(), ref["xent_deriv"], floor=sup.weight) <= REL
