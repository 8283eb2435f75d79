"""bfloat16 / float16 network outputs at the C ABI (tc_chain_step_typed), host side only: the typed entries are declared
and exported, the float32 case keeps tc_chain_step's workspace, the 16-bit cases add exactly the float32 scratch the
header documents, and an unknown element type is refused.  The computation itself: tests/test_gpu_half.py."""
import ctypes as C
import os
import re

import pytest
import torch

from torchain_amd import functions, io, synth
from torchain_amd._lib import LIB_PATH, TC_DTYPE_BF16, TC_DTYPE_F16, TC_DTYPE_F32, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "torchain_hip.h")
TC_ERR_INVALID_ARGUMENT = -1


def _align256(n):
    return (n + 255) // 256 * 256


@pytest.fixture(scope="module")
def graph():
    fst = synth.random_den_fst(500, 4, 200, seed=1)
    return io.DenominatorGraph(fst, fst.num_pdfs)


def test_typed_entries_are_declared_and_exported():
    text = open(HEADER).read()
    for name in ("tc_chain_step_typed", "tc_chain_step_typed_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(C.CDLL(LIB_PATH), name), name
    for name, value in (("TC_DTYPE_F32", 0), ("TC_DTYPE_BF16", 1), ("TC_DTYPE_F16", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert (TC_DTYPE_F32, TC_DTYPE_BF16, TC_DTYPE_F16) == (0, 1, 2)


@pytest.mark.parametrize("S,T", [(4, 40), (64, 150), (3, 7)])
def test_float32_workspace_is_tc_chain_steps(graph, S, T):
    for three_d in (0, 1):
        for xent in (0, 1):
            want = lib.tc_chain_step_workspace_bytes(graph.ptr, S, T, three_d, xent)
            assert want > 0
            assert lib.tc_chain_step_typed_workspace_bytes(graph.ptr, S, T, three_d, xent, TC_DTYPE_F32) == want


@pytest.mark.parametrize("dtype", [TC_DTYPE_BF16, TC_DTYPE_F16])
@pytest.mark.parametrize("S,T", [(4, 40), (64, 150), (3, 7)])
def test_half_workspace_adds_the_documented_scratch(graph, dtype, S, T):
    """M = align256(S * T * num_pdfs * 4): (B, C, T) adds M for the xent gradient with the xent branch, nothing without;
    2-D adds 2 M (the float32 input and gradient), 4 M with the xent branch (and xent_input and its gradient)."""
    M = _align256(S * T * lib.tc_den_graph_num_pdfs(graph.ptr) * 4)
    extra = {(1, 0): 0, (1, 1): 1, (0, 0): 2, (0, 1): 4}
    for (three_d, xent), k in extra.items():
        f32 = lib.tc_chain_step_workspace_bytes(graph.ptr, S, T, three_d, xent)
        got = lib.tc_chain_step_typed_workspace_bytes(graph.ptr, S, T, three_d, xent, dtype)
        assert got == f32 + k * M, (three_d, xent, got, f32, M)


@pytest.mark.parametrize("bad", [-1, 3, 7, 1 << 20])
def test_unknown_dtype_is_refused(graph, bad):
    assert lib.tc_chain_step_typed_workspace_bytes(graph.ptr, 4, 40, 1, 0, bad) == TC_ERR_INVALID_ARGUMENT
    # (refused before anything is looked at: no device, no workspace needed)
    ws = (C.c_char * 256)()
    rc = lib.tc_chain_step_typed(graph.ptr, None, C.cast(ws, C.c_void_p), None, 1, 0, 0.0, 0.1, 0.0, 1, None, None,
                                 C.cast(ws, C.c_void_p), None, None, bad, C.cast(ws, C.c_void_p), 256, 0, None)
    assert rc == TC_ERR_INVALID_ARGUMENT
    sup = synth.random_supervision(synth.random_den_fst(20, 3, 10, seed=2), 2, 8, 2, seed=3)
    s = io.Supervision.from_synth(sup)
    rc = lib.tc_chain_step_typed(graph.ptr, s.ptr, C.cast(ws, C.c_void_p), None, 1, 0, 0.0, 0.1, 0.0, 1, None, None,
                                 C.cast(ws, C.c_void_p), None, None, bad, C.cast(ws, C.c_void_p), 256, 0, None)
    assert rc == TC_ERR_INVALID_ARGUMENT


def test_step_dtypes_of_the_python_wrapper():
    """The wrapper sends bfloat16 / float16 to the typed entry and keeps float32 on tc_chain_step."""
    assert functions._STEP_DTYPES == {torch.float32: TC_DTYPE_F32, torch.bfloat16: TC_DTYPE_BF16,
                                      torch.float16: TC_DTYPE_F16}
    x = torch.zeros(2, 3, 4, dtype=torch.bfloat16)
    # CPU tensors are not taken (no CPU fallback, as for float32)
    assert functions._step_plan(x, None) is None
    # different dtypes: the 16-bit one(s) are up-cast, a lone 16-bit tensor is not (the planner, applied as chain_loss does)
    spec = functions._spec

    def apply(t, ops):
        for op in ops:
            t = functions._OPS[op](t)
        return t
    for other, ops in ((torch.zeros(2, 3, 4), (("float",), ())), (x.half(), (("float",), ("float",)))):
        got = functions.plan_step_inputs(spec(x), spec(other))
        assert got[:2] == ops
        assert apply(x, got[0]).dtype == apply(other, got[1]).dtype == torch.float32
    assert functions.plan_step_inputs(spec(x)) == ((), (), ("bct", 0, 0))
