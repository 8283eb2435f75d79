"""The fused tied kernel's full-layout twin (den_tied_kernel.hip: tied_full_layout): the instantiation that
takes for granted what the general one asks every frame -- all 8192 positions and 4096 pdfs in use, 16-byte rows, no
cross-entropy output to zero, no hub states -- and does a plane's per-state arithmetic on float4.

Bit for bit: the same call with ``tc_debug_set("no_full_layout", 1)`` runs the general instantiation; derivative, log-prob and
status must be the same bits.  (The two t = 0 checks -- sum alpha'_0 beta'_0 and sum gamma_0 per sequence -- reach the caller
as the status word; the sum of gamma_0 is the derivative's row 0.)  Against the oracle: the bounds of tests/test_gpu_tied.py
for the same kernel (REL = 1e-4; log-prob relative, derivative matrix-wise).  Routing: tc_debug_counter(
"tied_full_layout_launches") moves in exactly the eligible calls.

The graph is the C2 / C3 synthetic one: 8192 positions and 4096 pdfs are the smallest shape the twin takes.  Batches of 1 and 3
sequences (a lone workgroup; an odd number), T = 1 (no loop frame on either side), 2 (the first that stores a history row and
defers a derivative row), 7."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import check, lib
from torchain_amd.functions import ChainResults, compute_chain_objf_and_deriv

import row_contract_cases as rcc
from helpers import REL, hip_den, hip_den_on, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEAKY = 0.1
SWITCHES = ("no_tune", "no_phase_split", "no_mitm")  # the fused kernel, whatever the batch


def counter(name="tied_full_layout_launches"):
    return int(lib.tc_debug_counter(name.encode()))


def bits64(x):
    return struct.pack("<d", float(x))


@pytest.fixture(scope="module")
def c3(oracle):
    """(fst, graph handle, oracle graph) of the C2 / C3 graph, built once; the module's launch switches stay set while its tests
    run."""
    for key in SWITCHES:
        check(lib.tc_debug_set(key.encode(), 1), key)
    fst = synth.config_den_fst("C3")
    assert fst.num_pdfs == 4096
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    assert graph.stats()["tied"] == 1
    yield fst, graph, oracle.DenGraph(fst)
    for key in SWITCHES + ("no_full_layout",):
        lib.tc_debug_set(key.encode(), 0)


@functools.lru_cache(maxsize=None)
def outputs(S, T):
    y = synth.random_nnet_output(S, T, 4096, seed=100 * S + T)
    return y


_refs = {}


def reference(oracle, og, S, T):
    """the oracle's (log-prob, occupation matrix) of the case at deriv_weight 1, computed once"""
    if (S, T) not in _refs:
        ref = oracle.den_forward_backward(og, outputs(S, T), S, leaky=LEAKY, deriv_weight=1.0)
        assert ref["ok"]
        ref["deriv"].setflags(write=False)
        _refs[S, T] = ref
    return _refs[S, T]


def both_forms(c3, y, S, **kw):
    """the call on the twin and on the general instantiation; the counter says which ran"""
    fst, graph, _ = c3
    lib.tc_debug_set(b"no_full_layout", 0)
    n0 = counter()
    full = hip_den(fst, y, S, leaky=LEAKY, graph=graph, **kw)
    n1 = counter()
    lib.tc_debug_set(b"no_full_layout", 1)
    try:
        general = hip_den(fst, y, S, leaky=LEAKY, graph=graph, **kw)
    finally:
        lib.tc_debug_set(b"no_full_layout", 0)
    assert (n1 - n0, counter() - n1) == (1, 0)
    return full, general


def same_bits(full, general):
    a, b = full["deriv"].view(np.int32), general["deriv"].view(np.int32)
    assert a.shape == b.shape
    found = (full["status"], bits64(full["logprob"]), 0)
    want = (general["status"], bits64(general["logprob"]), int((a != b).sum()))
    assert found == want, "status, log-prob, differing elements of %d: %r / %r; log-probs %r / %r" % (
        a.size, found, want, full["logprob"], general["logprob"])


@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("S", [1, 3])
def test_full_layout_bits_and_oracle(oracle, c3, S, T):
    y = outputs(S, T)
    full, general = both_forms(c3, y, S, deriv_weight=1.0)
    same_bits(full, general)
    ref = reference(oracle, c3[2], S, T)
    err_lp, err_d = abs(full["logprob"] - ref["logprob"]) / abs(ref["logprob"]), rel_err(full["deriv"], ref["deriv"])
    print("S=%d T=%d: log-prob rel %.2e, derivative rel %.2e" % (S, T, err_lp, err_d))
    assert full["status"] == 0
    assert err_lp <= REL
    assert err_d <= REL
    assert np.abs(full["deriv"].sum(axis=1, dtype=np.float64) - 1.0).max() <= 1e-4  # [K]: sum_pdf gamma_t = 1 in every frame


VARIANTS = {  # name -> (accumulate, l2_scale, deriv_weight, what the derivative holds before the call)
    "accumulate": (True, 0.0, 1.0, 0.25),
    "l2": (False, 1e-3, 1.0, None),
    "accumulate_l2_half_weight": (True, 5e-5, 0.5, 0.25),
    "half_weight": (False, 0.0, 0.5, None),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_full_layout_variants(oracle, c3, variant):
    """ACCUM (the row's store follows the load of the same row), the l2 term, a derivative weight"""
    S, T = 3, 7
    accumulate, l2, weight, init = VARIANTS[variant]
    y = outputs(S, T)
    full, general = both_forms(c3, y, S, deriv_weight=weight, l2_scale=l2, accumulate=accumulate, init=init)
    same_bits(full, general)
    ref = reference(oracle, c3[2], S, T)
    want = weight * ref["deriv"] - l2 * y + (init if accumulate else 0.0)
    assert full["status"] == 0
    assert abs(full["logprob"] - ref["logprob"]) <= REL * abs(ref["logprob"])
    assert rel_err(full["deriv"], want) <= REL


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_full_layout_non_finite_row(c3, bad):
    """one bad element in a middle frame of the middle sequence: both forms fail alike (a non-finite log-prob), bit for bit"""
    S, T = 3, 7
    y = outputs(S, T).copy()
    y[3 * S + 1, 1234] = bad
    full, general = both_forms(c3, y, S, deriv_weight=1.0)
    same_bits(full, general)
    assert not np.isfinite(full["logprob"])


# ---- routing: what the twin does not take -----------------------------------------------------------------------------------
def launches():
    return counter("den_launches"), counter()


def test_unaligned_row_stride_runs_the_general_form(oracle, c3):
    """a derivative whose rows are P + 1 floats apart: d_vec = 0"""
    fst, graph, og = c3
    S, T, P = 3, 2, fst.num_pdfs
    y = outputs(S, T)
    yt = torch.from_numpy(y).to(DEV)
    dbuf, dview = rcc.strided(S * T, P, P + 1, 0, rcc.SENTINEL, device=DEV)
    assert rcc.vector_path(yt) and not rcc.vector_path(dview)
    d0, f0 = launches()
    out = hip_den_on(graph, S, yt, dview, leaky=LEAKY, deriv_weight=1.0)
    d1, f1 = launches()
    assert (d1 - d0, f1 - f0) == (1, 0)
    ref = reference(oracle, og, S, T)
    assert out["status"] == 0
    assert rel_err(dview.cpu().numpy(), ref["deriv"]) <= REL
    assert np.all(rcc.outside(dbuf, dview).cpu().numpy() == np.float32(rcc.SENTINEL).view(np.int32))
    # ... and the same matrix with aligned rows does take the twin
    dbuf, dview = rcc.strided(S * T, P, P + 4, 0, rcc.SENTINEL, device=DEV)
    assert rcc.vector_path(dview)
    hip_den_on(graph, S, yt, dview, leaky=LEAKY, deriv_weight=1.0)
    assert launches() == (d1 + 1, f1 + 1)
    assert rel_err(dview.cpu().numpy(), ref["deriv"]) <= REL
    assert np.all(rcc.outside(dbuf, dview).cpu().numpy() == np.float32(rcc.SENTINEL).view(np.int32))


def test_cross_entropy_output_runs_the_general_form(oracle, c3):
    """the objective with a cross-entropy output: the fused kernel writes that output's zero rows, which the twin does not"""
    fst, graph, og = c3
    S, T, P = 3, 2, fst.num_pdfs
    sup = synth.random_supervision(fst, S, T, 2, seed=80, weight=0.5, initial_probs=og.initial_probs())
    y = outputs(S, T)
    ref = oracle.compute_chain_objf_and_deriv(og, sup, y, 0.0, LEAKY, want_xent=True)
    yt = torch.from_numpy(y).to(DEV)
    deriv = torch.full((S * T, P), 7.0, device=DEV)
    xd = torch.full((S * T * P * 4,), 255, dtype=torch.uint8, device=DEV).view(torch.float32).view(S * T, P)
    res = ChainResults()
    d0, f0 = launches()
    compute_chain_objf_and_deriv(graph, io.Supervision.from_synth(sup), yt, res.data, deriv, xd, 0.0, LEAKY, 0.1)
    torch.cuda.synchronize()
    d1, f1 = launches()
    assert (d1 - d0, f1 - f0) == (1, 0)
    got = xd.cpu().numpy()
    assert np.isfinite(got).all() and not got[~rcc.carried(sup)].view(np.int32).any()
    assert rel_err(got, ref["xent_deriv"], floor=0.5) <= REL
    assert rel_err(deriv.cpu().numpy(), ref["deriv"], floor=0.5) <= REL


def test_partial_last_float4_runs_the_general_form(oracle, c3):
    """P = 4095: the same layout class, but the last float4 of pdfs is not whole (and no row takes 16-byte accesses)"""
    fst = synth.random_den_fst(8192, 8, 4095, seed=42)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    assert graph.stats()["tied"] == 1
    S, T = 3, 2
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=31)
    ref = oracle.den_forward_backward(oracle.DenGraph(fst), y, S, leaky=LEAKY, deriv_weight=1.0)
    d0, f0 = launches()
    out = hip_den(fst, y, S, leaky=LEAKY, deriv_weight=1.0, graph=graph)
    d1, f1 = launches()
    assert (d1 - d0, f1 - f0) == (1, 0)
    assert out["status"] == 0 and ref["ok"]
    assert abs(out["logprob"] - ref["logprob"]) <= REL * abs(ref["logprob"])
    assert rel_err(out["deriv"], ref["deriv"]) <= REL


def test_ragged_batch_runs_the_general_form(oracle, c3):
    """a ragged handle (tc_den_forward_backward_ragged) runs the RAGGED instantiation, also when every sequence has all T
    frames; the uniform call on the same matrices takes the twin"""
    fst, graph, og = c3
    S, T, P = 3, 2, fst.num_pdfs
    y = outputs(S, T)
    yt = torch.from_numpy(y).to(DEV)
    deriv = torch.full((S * T, P), 7.0, device=DEV)
    graph.prepare(yt.device)
    frames = torch.tensor([T] * S, dtype=torch.int32, device=DEV)
    nbytes = lib.tc_chain_workspace_bytes(graph.ptr, S, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    lp = torch.full((1,), -123.0, dtype=torch.float64, device=DEV)
    st = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    d0, f0 = launches()
    rcode = lib.tc_den_forward_backward_ragged(
        graph.ptr, S, C.c_void_p(yt.data_ptr()), S * T, P, yt.stride(0), LEAKY, 1.0, 0.0, 0,
        C.c_void_p(deriv.data_ptr()), deriv.stride(0), C.c_void_p(frames.data_ptr()), T, C.c_void_p(lp.data_ptr()),
        C.c_void_p(st.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, torch.cuda.current_device(),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rcode == 0, rcode
    d1, f1 = launches()
    assert (d1 - d0, f1 - f0) == (1, 0)
    uniform = hip_den(fst, y, S, leaky=LEAKY, deriv_weight=1.0, graph=graph)
    assert launches() == (d1 + 1, f1 + 1)
    ref = reference(oracle, og, S, T)
    assert int(st.item()) == uniform["status"] == 0
    assert abs(lp.item() - ref["logprob"]) <= REL * abs(ref["logprob"])
    assert rel_err(deriv.cpu().numpy(), ref["deriv"]) <= REL
    assert rel_err(uniform["deriv"], ref["deriv"]) <= REL
