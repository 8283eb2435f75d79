"""The expected frame accuracy over the denominator graph without a GPU: the float64 recursion of
``tests/den_accuracy_reference.py`` (what the GPU tests compare with) against a double backward through
``oracle/independent_f64.den_logprob``, its exact properties, the export and binding of the ``tc_den_expected_accuracy*``
entries, and the checks the library and the Python wrappers make before any device call."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import den_expected_accuracy

import den_accuracy_reference as dar

TC_ERR_INVALID_ARGUMENT = -1
TC_ERR_UNSUPPORTED = -3
TC_ERR_WORKSPACE = -4
S, T = 3, 11


@functools.lru_cache(maxsize=None)
def _case(kind):
    fst = {"left_to_right": lambda: synth.left_to_right_den_fst(20),
           "random": lambda: synth.random_den_fst(40, 4, 24)}[kind]()
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    pi = graph.initial_probs().astype(np.float64)
    rng = np.random.default_rng(17)
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=3).astype(np.float64)
    ref = rng.integers(0, fst.num_pdfs, size=(S, T)).astype(np.int32)
    ref[1, 4] = -1  # a frame that scores nothing
    cls = rng.integers(0, 5, size=fst.num_pdfs).astype(np.int32)
    return fst, graph, pi, y, ref, cls


@pytest.mark.parametrize("leaky", [1e-5, 0.2])
@pytest.mark.parametrize("with_class", [False, True])
@pytest.mark.parametrize("kind", ["left_to_right", "random"])
def test_recursion_agrees_with_the_double_backward_oracle(kind, with_class, leaky):
    fst, graph, pi, y, ref, cls = _case(kind)
    cls = cls if with_class else None
    acc, fa, grad = dar.batch(dar.arcs_of(fst), pi, y, S, ref, cls, leaky)
    want_acc, want_grad = dar.oracle(fst, pi, y, S, ref, cls, leaky)
    print("acc err %.3g, grad err %.3g, row sums %.3g" % (np.abs(acc - want_acc).max(), np.abs(grad - want_grad).max(),
                                                         np.abs(grad.sum(axis=1)).max()))
    assert np.abs(acc - want_acc).max() <= 1e-12
    assert np.abs(grad - want_grad).max() <= 1e-12
    assert np.abs(fa.sum(axis=1) - acc).max() <= 1e-12 and (fa >= 0).all() and (fa <= 1 + 1e-12).all()
    assert np.abs(want_grad).max() > 1e-3  # (the comparison is of something)
    # every row of the gradient sums to 0: a constant added to a frame's outputs changes no posterior
    assert np.abs(grad.sum(axis=1)).max() <= 1e-12


@pytest.mark.parametrize("leaky", [1e-5, 0.2])
@pytest.mark.parametrize("kind", ["left_to_right", "random"])
def test_gradient_does_not_change_with_the_centring_constants(kind, leaky):
    fst, graph, pi, y, ref, cls = _case(kind)
    arcs = dar.arcs_of(fst)
    rng = np.random.default_rng(5)
    for s in range(S):
        ys = y[s::S]
        base = dar.recursion(arcs, pi, ys, ref[s], cls, leaky)
        assert abs(base["residual"]) <= 1e-12
        for centre in (np.zeros(T), rng.normal(size=T)):
            other = dar.recursion(arcs, pi, ys, ref[s], cls, leaky, centre=centre)
            assert np.abs(other["grad"] - base["grad"]).max() <= 1e-12
            assert abs(other["residual"]) <= 1e-12 and other["acc"] == base["acc"]


@pytest.mark.parametrize("leaky", [1e-5, 0.2])
@pytest.mark.parametrize("kind", ["left_to_right", "random"])
def test_one_class_and_no_reference(kind, leaky):
    fst, graph, pi, y, ref, cls = _case(kind)
    arcs = dar.arcs_of(fst)
    full = np.where(ref < 0, 0, ref)
    acc, fa, grad = dar.batch(arcs, pi, y, S, full, np.zeros(fst.num_pdfs, np.int32), leaky, frames=[11, 7, 1])
    assert np.abs(acc - np.array([11, 7, 1])).max() <= 1e-12  # every path is right in every frame
    assert np.abs(grad).max() <= 1e-12
    acc, fa, grad = dar.batch(arcs, pi, y, S, np.full((S, T), -1), cls, leaky)
    assert (acc == 0).all() and (fa == 0).all() and (grad == 0).all()
    # a reference outside 0 .. P-1 scores nothing either
    acc, fa, grad = dar.batch(arcs, pi, y, S, np.full((S, T), fst.num_pdfs), None, leaky)
    assert (acc == 0).all() and (grad == 0).all()


# ---- the library's and the wrappers' checks in front of any device call ----
def test_entries_are_exported_and_check_their_arguments():
    fst, graph, pi, y, ref, cls = _case("random")
    P = fst.num_pdfs
    need = int(lib.tc_den_expected_accuracy_workspace_bytes(graph.ptr, S, T))
    need_grad = int(lib.tc_den_expected_accuracy_grad_workspace_bytes(graph.ptr, S, T))
    assert need == int(lib.tc_chain_workspace_bytes(graph.ptr, S, T)) and need_grad > 2 * 4 * S * (T + 1) * fst.num_states
    assert int(lib.tc_den_expected_accuracy_workspace_bytes(None, S, T)) == TC_ERR_INVALID_ARGUMENT
    assert int(lib.tc_den_expected_accuracy_grad_workspace_bytes(graph.ptr, 0, T)) == TC_ERR_INVALID_ARGUMENT
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails before a device call
    keys = (b"den_accuracy_launches", b"den_accuracy_grad_launches", b"den_accuracy_grad_streamed_launches", b"den_launches")
    before = [int(lib.tc_debug_counter(key)) for key in keys]
    assert min(before) >= 0

    def acc(g=graph.ptr, s=S, y=fake, rows=S * T, cols=P, stride=P, fr=None, t=T, leaky=1e-5, ref=fake, cl=None, gam=fake,
            gs=P, fa=fake, out=fake, ws=fake, nbytes=need):
        return lib.tc_den_expected_accuracy(g, s, y, rows, cols, stride, fr, t, leaky, ref, cl, gam, gs, fa, out, ws, nbytes, 0, None)

    def grad(g=graph.ptr, s=S, y=fake, rows=S * T, cols=P, stride=P, fr=None, t=T, leaky=1e-5, ref=fake, cl=None, fa=fake,
             sc=None, out=fake, gs=P, ws=fake, nbytes=need_grad):
        return lib.tc_den_expected_accuracy_grad(g, s, y, rows, cols, stride, fr, t, leaky, ref, cl, fa, sc, out, gs, ws, nbytes,
                                                 0, None)

    for call in (acc, grad):
        assert call(g=None) == TC_ERR_INVALID_ARGUMENT
        assert call(y=None) == TC_ERR_INVALID_ARGUMENT
        assert call(ref=None) == TC_ERR_INVALID_ARGUMENT
        assert call(fa=None) == TC_ERR_INVALID_ARGUMENT
        assert call(out=None) == TC_ERR_INVALID_ARGUMENT
        assert call(s=0) == TC_ERR_INVALID_ARGUMENT
        assert call(t=0) == TC_ERR_INVALID_ARGUMENT
        assert call(rows=S * T + 1) == TC_ERR_INVALID_ARGUMENT
        assert call(cols=P + 1) == TC_ERR_INVALID_ARGUMENT
        assert call(stride=P - 1) == TC_ERR_INVALID_ARGUMENT
        assert call(gs=P - 1) == TC_ERR_INVALID_ARGUMENT
        assert call(fr=C.c_void_p(4098)) == TC_ERR_INVALID_ARGUMENT  # lengths not 4-byte aligned
        assert call(leaky=-0.5) == TC_ERR_INVALID_ARGUMENT
        assert call(ws=None) == TC_ERR_WORKSPACE
        assert call(ws=C.c_void_p(4100)) == TC_ERR_WORKSPACE
    assert acc(gam=None) == TC_ERR_INVALID_ARGUMENT
    assert acc(nbytes=need - 1) == TC_ERR_WORKSPACE and grad(nbytes=need_grad - 1) == TC_ERR_WORKSPACE
    assert [int(lib.tc_debug_counter(key)) for key in keys] == before  # nothing was launched
    assert lib.tc_debug_set(b"force_den_accuracy_streamed", 0) == 0


def test_lengths_on_a_streamed_path_graph_are_refused_by_the_value_entry(kernel_family):
    kernel_family("force_streamed")
    fst = synth.random_den_fst(40, 4, 24)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    P, fake = fst.num_pdfs, C.c_void_p(4096)
    need = int(lib.tc_den_expected_accuracy_workspace_bytes(graph.ptr, S, T))
    before = int(lib.tc_debug_counter(b"den_launches"))
    assert lib.tc_den_expected_accuracy(graph.ptr, S, fake, S * T, P, P, fake, T, 1e-5, fake, None, fake, P, fake, fake, fake, need,
                                        0, None) == TC_ERR_UNSUPPORTED
    assert int(lib.tc_debug_counter(b"den_launches")) == before


def test_wrappers_check_before_any_library_call():
    fst, graph, pi, y, ref, cls = _case("random")
    P = fst.num_pdfs
    x = torch.zeros(S * T, P)
    with pytest.raises(ValueError, match="CUDA tensor"):
        graph.expected_accuracy(x, torch.zeros(S, T, dtype=torch.int32), n_batch=S)
    with pytest.raises(TypeError, match="io.DenominatorGraph"):
        den_expected_accuracy(x, fst, torch.zeros(S, T, dtype=torch.int32), n_batch=S)
    import torchain.functions
    import torchain.io
    assert torchain.functions.den_expected_accuracy is den_expected_accuracy
    assert torchain.io.DenominatorGraph.expected_accuracy is io.DenominatorGraph.expected_accuracy
