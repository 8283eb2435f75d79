"""The best path through the denominator graph without a GPU: the float64 reference of the GPU tests
(``tests/den_best_path_reference.py``) against brute-force enumeration of every path, the export and binding of
``tc_den_best_path`` / ``tc_den_best_path_workspace_bytes``, and the checks the library and the Python wrappers make before
any device call."""
import ctypes as C

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import TC_DTYPE_BF16, TC_DTYPE_F32, lib
from torchain_amd.functions import den_best_path

import den_best_path_reference as dbp

TC_ERR_INVALID_ARGUMENT = -1
TC_ERR_WORKSPACE = -4


def _cut(fst, n):
    """``fst`` cut to its first ``n`` states (arcs between them only)."""
    keep = (fst.src < n) & (fst.dst < n)
    return synth.DenFst(n, fst.src[keep], fst.dst[keep], fst.ilabel[keep], fst.weight[keep], fst.final[:n], 0, fst.num_pdfs)


def _small_graphs():
    out = [synth.left_to_right_den_fst(5, seed=s) for s in (1, 2, 3)]
    out.append(_cut(synth.left_to_right_den_fst(5, seed=4), 2))  # 0->0, 0->1, 1->1: state 1 is a sink with a self-loop
    out += [synth.random_den_fst(4, 3, 6, seed=s) for s in (5, 6)]  # parallel arcs, several pdfs
    return out


@pytest.mark.parametrize("T", [1, 2, 4])
def test_reference_agrees_with_enumeration_of_all_paths(T):
    rng = np.random.default_rng(200 + T)
    for fst in _small_graphs():
        graph = io.DenominatorGraph(fst, fst.num_pdfs)
        pi = graph.initial_probs()
        assert fst.num_states <= 4 and (pi >= 0).all() and pi.sum() > 0.99
        for _ in range(4):
            y = (rng.normal(size=(T, fst.num_pdfs)) * 2.0).astype(np.float32)
            want, arg = dbp.brute_force(fst, pi, y)
            states, pdfs, got = dbp.viterbi(fst, pi, y)
            # (both add the same float64 terms in the same order along a path: no tolerance)
            assert got == want
            assert (tuple(int(h) for h in states), tuple(int(p) for p in pdfs)) in arg
            assert dbp.rescore(fst, pi, states, pdfs, y) == want
            score, peak = dbp.rescore(fst, pi, states, pdfs, y, running=True)
            assert score == want and peak >= abs(want)
            # a pdf sequence the path's states do not carry is no path
            wrong = (pdfs + 1) % fst.num_pdfs
            assert dbp.rescore(fst, pi, states, wrong, y) <= want
            # the runner-up of a best path scores no more than it, and boosting the path's own outputs widens the gap by the boost
            second = dbp.runner_up(fst, pi, y, states, pdfs)
            assert second <= want
            if len(arg) == 1:
                assert second < want


def test_reference_respects_the_initial_probabilities():
    """A state with pi == 0 starts no path, however good its arcs."""
    fst = synth.left_to_right_den_fst(5, seed=1)
    pi = np.array([0.0, 1.0, 0.0], np.float32)
    y = np.zeros((3, 5), np.float32)
    states, _, score = dbp.viterbi(fst, pi, y)
    assert states[0] == 1 and score == dbp.brute_force(fst, pi, y)[0]
    assert dbp.rescore(fst, pi, np.array([0, 0, 0, 0]), np.array([fst.ilabel[0] - 1] * 3), y) == -np.inf


def test_symbols_are_exported_and_bound():
    """Fails where the library lacks the call."""
    for name in ("tc_den_best_path", "tc_den_best_path_workspace_bytes"):
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.tc_den_best_path.restype is C.c_int and lib.tc_den_best_path_workspace_bytes.restype is C.c_int64
    assert lib.tc_debug_counter(b"den_best_path_launches") >= 0  # (-1: an unknown key)
    assert lib.tc_debug_counter(b"den_best_path_streamed_launches") >= 0
    from torchain import functions as shim
    assert shim.den_best_path is den_best_path and hasattr(shim, "best_path")


def test_workspace_bytes():
    fst = synth.random_den_fst(301, 3, 40, seed=1)
    graph = io.DenominatorGraph(fst, 40)
    # (T + 1) rows of the states rounded up to 4, float32, a sequence; the whole rounded up to 256
    assert lib.tc_den_best_path_workspace_bytes(graph.ptr, 3, 11) == (3 * 12 * 304 * 4 + 255) // 256 * 256
    assert lib.tc_den_best_path_workspace_bytes(graph.ptr, 1, 1) == (2 * 304 * 4 + 255) // 256 * 256
    assert lib.tc_den_best_path_workspace_bytes(graph.ptr, 0, 11) == TC_ERR_INVALID_ARGUMENT
    assert lib.tc_den_best_path_workspace_bytes(graph.ptr, 3, 0) == TC_ERR_INVALID_ARGUMENT
    assert lib.tc_den_best_path_workspace_bytes(None, 3, 11) == TC_ERR_INVALID_ARGUMENT


def test_library_checks_arguments_before_any_device_call():
    """No device exists here: a call that got past the checks would fail otherwise (TC_ERR_HIP)."""
    P, S, T = 40, 3, 5
    graph = io.DenominatorGraph(synth.random_den_fst(30, 3, P, seed=1), P)
    need = lib.tc_den_best_path_workspace_bytes(graph.ptr, S, T)
    launches = lib.tc_debug_counter(b"den_best_path_launches")
    ptr = C.c_void_p(4096)  # never dereferenced on the host

    def call(g=graph.ptr, s=S, y=ptr, dtype=TC_DTYPE_F32, bct=0, rows=S * T, cols=P, stride=P, frames=None, tmax=T, pdf=ptr,
             states=None, score=ptr, ws=ptr, ws_bytes=need):
        return lib.tc_den_best_path(g, s, y, dtype, bct, rows, cols, stride, frames, tmax, pdf, states, score, ws, ws_bytes, 0,
                                    None)

    assert call(g=None) == TC_ERR_INVALID_ARGUMENT
    assert call(y=None) == TC_ERR_INVALID_ARGUMENT
    assert call(pdf=None) == TC_ERR_INVALID_ARGUMENT
    assert call(score=None) == TC_ERR_INVALID_ARGUMENT
    assert call(s=0) == TC_ERR_INVALID_ARGUMENT
    assert call(tmax=0) == TC_ERR_INVALID_ARGUMENT
    assert call(rows=S * T + 1) == TC_ERR_INVALID_ARGUMENT
    assert call(cols=P + 1) == TC_ERR_INVALID_ARGUMENT
    assert call(stride=P - 1) == TC_ERR_INVALID_ARGUMENT
    assert call(dtype=7, bct=1) == TC_ERR_INVALID_ARGUMENT
    assert call(dtype=TC_DTYPE_BF16, bct=0) == TC_ERR_INVALID_ARGUMENT  # (2-D tensors are float32)
    assert call(frames=C.c_void_p(4098)) == TC_ERR_INVALID_ARGUMENT  # (lengths that are not 4-byte aligned)
    assert call(ws=None) == TC_ERR_WORKSPACE
    assert call(ws_bytes=need - 1) == TC_ERR_WORKSPACE
    assert call(ws=C.c_void_p(4096 + 8)) == TC_ERR_WORKSPACE  # (not 16-byte aligned)
    assert lib.tc_debug_counter(b"den_best_path_launches") == launches


def test_wrappers_refuse_before_any_library_call(monkeypatch):
    P = 40
    graph = io.DenominatorGraph(synth.random_den_fst(30, 3, P, seed=1), P)
    calls = []
    monkeypatch.setattr(lib, "tc_den_best_path", lambda *a: calls.append(a) or 0)
    monkeypatch.setattr(lib, "tc_den_best_path_workspace_bytes", lambda *a: calls.append(a) or 0)
    with pytest.raises(ValueError, match="CUDA tensor"):
        graph.best_path(torch.zeros(2, P, 5))  # not a CUDA tensor
    with pytest.raises(ValueError, match="CUDA tensor"):
        den_best_path(torch.zeros(10, P), graph, n_batch=2)
    with pytest.raises(TypeError):
        den_best_path(torch.zeros(2, P, 5), graph.ptr)
    # the remaining checks come after the device check: a meta tensor carries shape and dtype and says it is on a device
    meta = lambda *shape, dtype=torch.float32: _as_cuda(torch.empty(*shape, dtype=dtype, device="meta"))  # noqa: E731
    with pytest.raises(ValueError, match="is not"):
        graph.best_path(meta(2, P + 1, 5))  # a wrong pdf count
    with pytest.raises(ValueError, match="is not"):
        graph.best_path(meta(10, P - 1), n_batch=2)
    with pytest.raises(ValueError, match="1 .. 5"):
        graph.best_path(meta(2, P, 5), frames=[5, 0])
    with pytest.raises(ValueError, match="1 .. 5"):
        graph.best_path(meta(2, P, 5), frames=torch.tensor([6, 1]))
    with pytest.raises(ValueError, match="lengths for"):
        graph.best_path(meta(2, P, 5), frames=[5, 5, 5])
    with pytest.raises(ValueError, match="lengths for"):
        den_best_path(meta(2, P, 5), graph, frames=np.array([5], np.int32))
    with pytest.raises(TypeError):
        graph.best_path(meta(2, P, 5), frames=[2.5, 1.0])
    with pytest.raises(TypeError):
        graph.best_path(meta(2, P, 5, dtype=torch.float64))
    with pytest.raises(TypeError):
        graph.best_path(meta(10, P, dtype=torch.bfloat16), n_batch=2)
    with pytest.raises(ValueError, match="frames. or .n_batch"):
        graph.best_path(meta(10, P))
    with pytest.raises(ValueError):
        graph.best_path(meta(10, P), n_batch=3)  # 10 rows are not 3 sequences
    assert calls == []


def _as_cuda(t):
    """``t`` (a meta tensor: shape and dtype, no storage) answering True to ``is_cuda``."""

    class OnDevice(torch.Tensor):
        is_cuda = True

    return t.as_subclass(OnDevice)
