"""Six resident forward chunks in the fused tied kernel's full-layout twin (den_tied_kernel.hip: TC_RESF_FULL).

The twin keeps the first six chunks of every wave's forward stream in registers and streams the rest through two buffers; how a
walk ends depends on the wave's chunk count (den_tied_device.h: walk):

    6 chunks   nothing is streamed; the frame's look-ahead load reads the chunk behind the wave's range and nobody uses it
    7          the single peeled chunk
    8          the peeled pair
    9, 10      the loop once, then the single chunk / the pair
    11 ...     the loop more than once

The C2 / C3 graph (tests/test_gpu_full_layout.py) has waves of 6, 7 and 8 chunks.  The graphs here are
``synth.random_den_fst(8192, d, 4096, seed=42)`` -- 8192 positions and 4096 pdfs are the smallest shape the twin takes -- at
three densities, all with C3's LDS layout (148352 bytes):

    d = 3    17920 forward slots, 35 chunks for 16 waves: every stream is padded to the six-chunk minimum
    d = 10   74432 slots, about 9.1 chunks a wave: the loop once plus either peel
    d = 12   91072 slots, about 11.1 chunks a wave: the loop more than once

For each graph, S in {1, 3} and T in {1, 2, 7}: the call takes the twin (tc_debug_counter("tied_full_layout_launches") moves by
one, and by zero under ``no_full_layout``); derivative, log-prob and status of the two forms are the same bits -- the general
instantiation keeps four resident chunks, and the same cells go through the same fmaf chain --; the twin is within
helpers.REL of the oracle (log-prob relative, derivative matrix-wise); every frame's derivative row sums to 1."""
import functools
import struct

import numpy as np
import pytest

from torchain_amd import io, synth
from torchain_amd._lib import check, lib

from helpers import REL, hip_den, rel_err

pytestmark = pytest.mark.gpu
LEAKY = 0.1
SWITCHES = ("no_tune", "no_phase_split", "no_mitm")  # the fused kernel, whatever the batch
SLOTS = {3: 17920, 10: 74432, 12: 91072}  # density -> forward slots of the schedule (64 lanes x 8 cells to a chunk)


def counter(name="tied_full_layout_launches"):
    return int(lib.tc_debug_counter(name.encode()))


def bits64(x):
    return struct.pack("<d", float(x))


@pytest.fixture(scope="module")
def switches():
    for key in SWITCHES:
        check(lib.tc_debug_set(key.encode(), 1), key)
    yield
    for key in SWITCHES + ("no_full_layout",):
        lib.tc_debug_set(key.encode(), 0)


@functools.lru_cache(maxsize=None)
def graph_of(d):
    """(fst, graph handle) of one density, built once"""
    fst = synth.random_den_fst(8192, d, 4096, seed=42)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    st = graph.stats()
    assert st["tied"] == 1 and st["lds_bytes"] == 148352 and st["fwd_rows"] <= 8192
    assert st["fwd_slots"] == SLOTS[d]  # which ends of the walk the graph reaches (module docstring)
    return fst, graph


@functools.lru_cache(maxsize=None)
def outputs(S, T):
    return synth.random_nnet_output(S, T, 4096, seed=100 * S + T)


_refs = {}


def reference(oracle, d, S, T):
    """the oracle's (log-prob, occupation matrix) of the case, computed once"""
    if (d, S, T) not in _refs:
        ref = oracle.den_forward_backward(oracle.DenGraph(graph_of(d)[0]), outputs(S, T), S, leaky=LEAKY, deriv_weight=1.0)
        assert ref["ok"]
        ref["deriv"].setflags(write=False)
        _refs[d, S, T] = ref
    return _refs[d, S, T]


@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("d", sorted(SLOTS))
def test_six_resident_chunks_bits_and_oracle(oracle, switches, d, S, T):
    fst, graph = graph_of(d)
    y = outputs(S, T)
    lib.tc_debug_set(b"no_full_layout", 0)
    n0 = counter()
    full = hip_den(fst, y, S, leaky=LEAKY, deriv_weight=1.0, graph=graph)
    n1 = counter()
    lib.tc_debug_set(b"no_full_layout", 1)
    try:
        general = hip_den(fst, y, S, leaky=LEAKY, deriv_weight=1.0, graph=graph)
    finally:
        lib.tc_debug_set(b"no_full_layout", 0)
    assert (n1 - n0, counter() - n1) == (1, 0)  # the twin ran, and only where it was allowed to

    a, b = full["deriv"].view(np.int32), general["deriv"].view(np.int32)
    assert a.shape == b.shape
    found = (full["status"], bits64(full["logprob"]), 0)
    want = (general["status"], bits64(general["logprob"]), int((a != b).sum()))
    assert found == want, "status, log-prob, differing elements of %d: %r / %r; log-probs %r / %r" % (
        a.size, found, want, full["logprob"], general["logprob"])

    ref = reference(oracle, d, S, T)
    err_lp, err_d = abs(full["logprob"] - ref["logprob"]) / abs(ref["logprob"]), rel_err(full["deriv"], ref["deriv"])
    rows = np.abs(full["deriv"].sum(axis=1, dtype=np.float64) - 1.0).max()
    print("d=%d S=%d T=%d: log-prob rel %.2e, derivative rel %.2e, row sums off 1 by %.2e" % (d, S, T, err_lp, err_d, rows))
    assert full["status"] == 0
    assert err_lp <= REL
    assert err_d <= REL
    assert rows <= 1e-4  # [K]: sum_pdf gamma_t = 1 in every frame
