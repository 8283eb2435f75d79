"""Cases and float64 references of the tests of ragged batches on two workgroups per sequence (tests/test_gpu_ragged_two_cu.py
on the GPU, tests/test_ragged_two_cu_host.py without one): a helper, not a test module.

A ragged batch of 8 sequences up to half the chip's CUs takes the RAGGED instantiation of its graph class's meet-in-the-middle
kernel: sequence s meets at frame ``lengths[s] // 2``.  The batch is 8 sequences -- the smallest the route takes -- of lengths
(7, 2, 5, 1, 3, 6, 2, 4): odd and even lengths; one frame (no meeting frame: role F alone), two and three frames (meeting frame
1, one pure frame on one or both sides); the longest sequence not last; a repeated length.  The graphs are those of
``row_contract_cases.GRAPHS``; the references are ``ragged_cases.den_reference`` (the oracle on each sequence alone) and, for
the training step, ``ragged_cases.ragged_objective`` on the 80-state graph of ``ragged_cases``.  Importing needs no GPU."""
import functools

import numpy as np

from torchain_amd import synth

import e2e_reference as ref
import ragged_cases as rc
import row_contract_cases as rcc

LENGTHS = (7, 2, 5, 1, 3, 6, 2, 4)
S, TMAX = len(LENGTHS), max(LENGTHS)
DERIV_WEIGHT = -0.8

# form -> family.  The tied graphs with default launch switches (a uniform batch of 8 would take the two-pass form there: a
# ragged one has none), the plane-wise kernel and its split-source form.  pdfs2 / pdfs3 have no default-switch family in
# row_contract_cases (their two-CU forms are covered there through tied8): made here.
FORMS = {
    "tied8_two_cu": rcc.BY_NAME["tied8_two_cu"],
    "tied12_two_cu": rcc.BY_NAME["tied12_two_cu"],
    "tied16_two_cu": rcc.BY_NAME["tied16_two_cu"],
    "pdfs2": rcc.Family("pdfs2_two_cu", "pdfs2", (), (), 1, S, TMAX),
    "pdfs3": rcc.Family("pdfs3_two_cu", "pdfs3", (), (), 1, S, TMAX),
    "planes_two_cu": rcc.BY_NAME["planes_two_cu"],
    "split_two_cu": rcc.BY_NAME["split_two_cu"],
}
PLANEWISE = ("planes_two_cu", "split_two_cu")  # a uniform batch takes two workgroups by default; the others need force_mitm


@functools.lru_cache(maxsize=None)
def oracle_graph(graph):
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle.DenGraph(rcc.den_fst(graph))


@functools.lru_cache(maxsize=None)
def den_output(graph, lens=LENGTHS, seed=140):
    """(Tmax * S, P) float32, finite everywhere, read-only (the tests put what they want into the padding of a copy)"""
    y = synth.random_nnet_output(len(lens), max(lens), rcc.den_fst(graph).num_pdfs, seed=seed + len(lens))
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def den_reference(graph, lens=LENGTHS, seed=140, deriv_weight=DERIV_WEIGHT):
    """(sum of the sequences' log-probs, derivative with zeros in the padding), float64, computed once; leave it unchanged.
    ``ragged_cases.den_reference`` asserts the oracle's ``ok`` for every sequence."""
    lp, d = rc.den_reference(oracle_graph(graph), lens, den_output(graph, lens, seed), rcc.LEAKY, deriv_weight)
    d.setflags(write=False)
    return lp, d


def boundary_lengths(n):
    """The chip-boundary batches: lengths cycling 1 .. 5"""
    return tuple(1 + i % 5 for i in range(n))


# ---- the training step: 8 sequences of the ``random`` end-to-end family (a final start state with a self-loop: every length
# is feasible) on ragged_cases' 80-state denominator graph
STEP_SEED = 17


@functools.lru_cache(maxsize=None)
def step_fsts():
    return tuple(ref.batch("random", S, rc.P, seed=STEP_SEED))


@functools.lru_cache(maxsize=None)
def step_output(scale=2.0):
    y = (np.random.default_rng(300 + S + TMAX).normal(size=(TMAX * S, rc.P)) * scale).astype(np.float32)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def step_reference(bfloat16=False):
    """``ragged_cases.ragged_objective`` of the step's batch (on the outputs rounded to bfloat16: what that step is given)"""
    y = step_output()
    if bfloat16:
        import torch
        y = torch.from_numpy(np.array(y)).to(torch.bfloat16).float().numpy()
    out = rc.ragged_objective(rc.oracle_graph(), step_fsts(), LENGTHS, y)
    for k in ("deriv", "xent_deriv"):
        out[k].setflags(write=False)
    return out
