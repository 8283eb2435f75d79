"""Kaldi's per-frame derivative weights (``deriv_weights``) at the C ABI and in the Python signatures, host side only: the
weighted entry is declared and exported, it refuses null handles, an unknown element type and a misaligned weight vector
before it touches a device, the public functions take ``deriv_weights=None`` as a trailing keyword, and
``shard_deriv_weights`` is the frame-major slice.  The computation itself: tests/test_gpu_deriv_weights.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import torchain.functions
from torchain_amd import functions, io, ops, parallel, synth
from torchain_amd._lib import LIB_PATH, TC_DTYPE_BF16, TC_DTYPE_F32, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "torchain_hip.h")
TC_ERR_INVALID_ARGUMENT = -1


@pytest.fixture(scope="module")
def graph_and_sup():
    fst = synth.random_den_fst(500, 4, 200, seed=1)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, 2, 8, 2, seed=3))
    return graph, sup


def test_weighted_entry_is_declared_and_exported():
    text = open(HEADER).read()
    m = re.search(r"int tc_chain_step_weighted\s*\(([^)]*)\)", text)
    assert m, "tc_chain_step_weighted is not declared"
    params = [p.split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
    # the parameters of tc_chain_step_typed, with the weights in front of the element type
    assert params[params.index("deriv_weights") + 1] == "dtype"
    assert "const float *deriv_weights" in m.group(1)
    typed = re.search(r"int tc_chain_step_typed\s*\(([^)]*)\)", text).group(1)
    typed_params = [p.split()[-1].lstrip("*") for p in typed.replace("\n", " ").split(",")]
    assert [p for p in params if p != "deriv_weights"] == typed_params
    assert hasattr(C.CDLL(LIB_PATH), "tc_chain_step_weighted")
    argtypes = lib.tc_chain_step_weighted.argtypes
    assert lib.tc_chain_step_weighted.restype is C.c_int
    assert len(argtypes) == len(lib.tc_chain_step_typed.argtypes) + 1
    assert argtypes[15] is C.c_void_p and argtypes[16] is C.c_int  # (deriv_weights, dtype)


def _call(graph, sup, weights, dtype, ws):
    p = C.cast(ws, C.c_void_p)
    return lib.tc_chain_step_weighted(graph, sup, p, None, 1, 0, 0.0, 0.1, 0.0, 1, None, None, p, None, None, weights,
                                      dtype, p, 256, 0, None)


def test_weighted_entry_refuses_bad_arguments_without_a_device(graph_and_sup):
    graph, sup = graph_and_sup
    ws = (C.c_char * 256)()
    w = C.cast(ws, C.c_void_p)
    assert _call(None, sup.ptr, w, TC_DTYPE_F32, ws) == TC_ERR_INVALID_ARGUMENT
    assert _call(graph.ptr, None, w, TC_DTYPE_F32, ws) == TC_ERR_INVALID_ARGUMENT
    assert _call(None, None, None, TC_DTYPE_BF16, ws) == TC_ERR_INVALID_ARGUMENT
    for bad in (-1, 3, 1 << 20):
        assert _call(graph.ptr, sup.ptr, w, bad, ws) == TC_ERR_INVALID_ARGUMENT
        assert _call(graph.ptr, sup.ptr, None, bad, ws) == TC_ERR_INVALID_ARGUMENT
    # a weight vector that is not 4-byte aligned
    assert _call(graph.ptr, sup.ptr, C.c_void_p(w.value + 2), TC_DTYPE_F32, ws) == TC_ERR_INVALID_ARGUMENT


def _positional(fn):
    code = fn.__code__
    return list(code.co_varnames[:code.co_argcount])


REFERENCE = ["input", "den_graph", "supervision", "l2_regularize", "leaky_hmm_coefficient", "xent_regularize", "xent_input",
             "kaldi_way"]


@pytest.mark.parametrize("fn,before", [
    (functions.chain_loss, REFERENCE),
    (torchain.functions.chain_loss, REFERENCE),
    (ops.chain_loss_op, REFERENCE),
    (parallel.chain_loss_data_parallel, REFERENCE + ["group", "even_if_alone"]),
])
def test_deriv_weights_is_a_trailing_keyword(fn, before):
    """The earlier parameters keep their order and defaults; ``deriv_weights`` follows them, keyword-only, default None."""
    assert _positional(fn) == before
    assert fn.__kwdefaults__ == {"deriv_weights": None}
    assert fn.__code__.co_kwonlyargcount == 1


def test_chain_loss_still_shows_the_reference_signature():
    """Introspection of chain_loss keeps reporting the reference's parameters (tests/test_host_api.py pins them)."""
    assert list(inspect.signature(functions.chain_loss).parameters) == REFERENCE
    assert functions.chain_loss is torchain.functions.chain_loss
    assert list(inspect.signature(parallel.chain_loss_data_parallel).parameters)[-1] == "deriv_weights"


def test_registered_operator_takes_optional_weights():
    schema = str(torch.ops.torchain_amd.chain_step.default._schema)
    assert schema.split("(", 1)[1].split(")")[0].split(", ")[-1] == "Tensor? deriv_weights=None", schema
    assert "bool want_grad, Tensor? deriv_weights=None" in schema


def test_weights_are_checked_on_the_host():
    S, T = 3, 5
    assert functions._deriv_weights(None, S * T) is None
    for ok in (torch.ones(S * T), torch.ones(S * T, dtype=torch.float64), torch.arange(S * T)):
        assert functions._deriv_weights(ok, S * T) is ok
    for bad in (torch.ones(S * T + 1), torch.ones(S, T), torch.ones(S * T, dtype=torch.complex64),
                torch.ones(S * T, dtype=torch.bool), np.ones(S * T, np.float32), [1.0] * (S * T)):
        with pytest.raises(ValueError):
            functions._deriv_weights(bad, S * T)
    assert functions._rows_of(torch.zeros(S, 7, T)) == S * T
    assert functions._rows_of(torch.zeros(S * T, 7)) == S * T


@pytest.mark.parametrize("S,T,lo,hi", [(4, 6, 0, 2), (4, 6, 2, 4), (5, 3, 1, 4), (7, 1, 0, 7), (3, 4, 2, 3)])
def test_shard_deriv_weights_is_the_frame_major_slice(S, T, lo, hi):
    w = np.random.default_rng(S * 100 + T).random(S * T).astype(np.float32)
    want = np.array([w[t * S + s] for t in range(T) for s in range(lo, hi)], np.float32)
    np.testing.assert_array_equal(parallel.shard_deriv_weights(w, S, lo, hi), want)
    got = parallel.shard_deriv_weights(torch.from_numpy(w), S, lo, hi)
    assert isinstance(got, torch.Tensor) and got.shape == (T * (hi - lo),)
    np.testing.assert_array_equal(got.numpy(), want)
    # the rows shard_rows keeps for the same sequences
    rows = parallel.shard_rows(torch.arange(S * T, dtype=torch.float32).reshape(S * T, 1), S, lo, hi)
    np.testing.assert_array_equal(parallel.shard_deriv_weights(np.arange(S * T), S, lo, hi), rows[:, 0].numpy())
