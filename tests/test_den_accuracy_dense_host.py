"""The expected accuracy over the denominator graph against a dense per-pdf accuracy, without a GPU: the float64 recursion of
``tests/den_accuracy_dense_reference.py`` (what the GPU tests compare with) against ``den_accuracy_reference.recursion`` on
indicator matrices and against a double backward through ``oracle/independent_f64.den_logprob`` on soft ones, the export and
binding of the ``tc_den_expected_accuracy_dense*`` entries, and the checks the library and the Python wrappers make before any
device call."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib

import den_accuracy_dense_reference as ddr
import den_accuracy_reference as dar

TC_ERR_INVALID_ARGUMENT = -1
TC_ERR_UNSUPPORTED = -3
TC_ERR_WORKSPACE = -4
S, T = 2, 7


@functools.lru_cache(maxsize=None)
def _case(kind):
    fst = {"random": lambda: synth.random_den_fst(60, 4, 30, seed=21),
           "skewed_tied": lambda: synth.skewed_tied_den_fst(80, 700, 40, seed=22)}[kind]()
    assert 60 <= fst.num_states <= 80 and 30 <= fst.num_pdfs <= 40
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    pi = graph.initial_probs().astype(np.float64)
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=3).astype(np.float64)
    return fst, graph, pi, y


def _accuracy(kind, P, rng):
    if kind == "dirichlet":
        return rng.dirichlet(np.full(P, 0.3), size=S * T)
    return rng.normal(scale=3.0, size=(S * T, P))  # signed rewards, N(0, 9)


@pytest.mark.parametrize("leaky", [1e-5, 0.1])
@pytest.mark.parametrize("with_class", [False, True])
@pytest.mark.parametrize("kind", ["random", "skewed_tied"])
def test_indicator_matrix_gives_the_hard_recursion(kind, with_class, leaky):
    fst, graph, pi, y = _case(kind)
    P = fst.num_pdfs
    rng = np.random.default_rng(5)
    ref = rng.integers(0, P, size=(S, T)).astype(np.int32)
    ref[1, 3] = -1  # a frame that scores nothing
    cls = rng.integers(0, 5, size=P).astype(np.int32) if with_class else None
    a = ddr.indicator(ref, cls, P, S)
    assert a.dtype == np.float32 and set(np.unique(a)) == {0.0, 1.0} and not a[1::S][3].any()
    arcs = dar.arcs_of(fst)
    for s in range(S):
        want = dar.recursion(arcs, pi, y[s::S], ref[s], cls, leaky)
        got = ddr.recursion(arcs, pi, y[s::S], a[s::S], leaky)
        for key in ("acc", "frame_acc", "gamma", "grad"):
            assert np.abs(np.asarray(got[key]) - np.asarray(want[key])).max() <= 1e-12, key
        assert abs(got["residual"]) <= 1e-12


@pytest.mark.parametrize("leaky", [1e-5, 0.1])
@pytest.mark.parametrize("soft", ["dirichlet", "rewards"])
@pytest.mark.parametrize("kind", ["random", "skewed_tied"])
def test_recursion_agrees_with_the_double_backward_oracle(kind, soft, leaky):
    fst, graph, pi, y = _case(kind)
    a = _accuracy(soft, fst.num_pdfs, np.random.default_rng(9))
    acc, fa, grad, gamma = ddr.batch(dar.arcs_of(fst), pi, y, S, a, leaky)
    want_acc, want_grad, want_gamma = ddr.oracle(fst, pi, y, S, a, leaky)
    print("acc err %.3g, dE/dy err %.3g, dE/da err %.3g, row sums %.3g" % (
        np.abs(acc - want_acc).max(), np.abs(grad - want_grad).max(), np.abs(gamma - want_gamma).max(),
        np.abs(grad.sum(axis=1)).max()))
    assert np.abs(acc - want_acc).max() <= 1e-12
    assert np.abs(grad - want_grad).max() <= 1e-12
    assert np.abs(gamma - want_gamma).max() <= 1e-12  # dE/da == gamma
    assert np.abs(fa.sum(axis=1) - acc).max() <= 1e-12
    assert np.abs(want_grad).max() > 1e-3  # (the comparison is of something)
    # every row of the gradient sums to 0, and the posteriors' rows to 1
    assert np.abs(grad.sum(axis=1)).max() <= 1e-12 and np.abs(gamma.sum(axis=1) - 1).max() <= 1e-12
    if soft == "dirichlet":
        assert (fa >= 0).all() and (fa <= 1 + 1e-12).all()
    else:
        assert a.min() < -3 and a.max() > 3  # nothing assumes [0, 1]


# ---- the library's and the wrappers' checks in front of any device call ----
def test_entries_are_exported_and_check_their_arguments():
    fst, graph, pi, y = _case("random")
    P = fst.num_pdfs
    need = int(lib.tc_den_expected_accuracy_workspace_bytes(graph.ptr, S, T))
    need_grad = int(lib.tc_den_expected_accuracy_grad_workspace_bytes(graph.ptr, S, T))
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails before a device call
    keys = (b"den_accuracy_launches", b"den_accuracy_grad_launches", b"den_accuracy_grad_streamed_launches",
            b"den_accuracy_dense_launches", b"den_accuracy_dense_grad_launches", b"den_launches")
    before = [int(lib.tc_debug_counter(key)) for key in keys]
    assert min(before) >= 0

    def acc(g=graph.ptr, s=S, y=fake, rows=S * T, cols=P, stride=P, fr=None, t=T, leaky=1e-5, a=fake, a_stride=P, gam=fake,
            gs=P, fa=fake, out=fake, ws=fake, nbytes=need):
        return lib.tc_den_expected_accuracy_dense(g, s, y, rows, cols, stride, fr, t, leaky, a, a_stride, gam, gs, fa, out, ws,
                                                  nbytes, 0, None)

    def grad(g=graph.ptr, s=S, y=fake, rows=S * T, cols=P, stride=P, fr=None, t=T, leaky=1e-5, a=fake, a_stride=P, fa=fake,
             sc=None, out=fake, gs=P, ws=fake, nbytes=need_grad):
        return lib.tc_den_expected_accuracy_dense_grad(g, s, y, rows, cols, stride, fr, t, leaky, a, a_stride, fa, sc, out, gs,
                                                       ws, nbytes, 0, None)

    for call in (acc, grad):
        assert call(g=None) == TC_ERR_INVALID_ARGUMENT
        assert call(y=None) == TC_ERR_INVALID_ARGUMENT
        assert call(a=None) == TC_ERR_INVALID_ARGUMENT
        assert call(a=C.c_void_p(4098)) == TC_ERR_INVALID_ARGUMENT  # accuracy not 4-byte aligned
        assert call(a_stride=P - 1) == TC_ERR_INVALID_ARGUMENT
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
        assert call(leaky=float("inf")) == TC_ERR_INVALID_ARGUMENT
        assert call(ws=None) == TC_ERR_WORKSPACE
        assert call(ws=C.c_void_p(4100)) == TC_ERR_WORKSPACE
    assert acc(gam=None) == TC_ERR_INVALID_ARGUMENT
    assert acc(out=C.c_void_p(4100)) == TC_ERR_INVALID_ARGUMENT  # acc_dev: doubles
    assert grad(sc=C.c_void_p(4098)) == TC_ERR_INVALID_ARGUMENT
    assert acc(nbytes=need - 1) == TC_ERR_WORKSPACE and grad(nbytes=need_grad - 1) == TC_ERR_WORKSPACE
    assert [int(lib.tc_debug_counter(key)) for key in keys] == before  # nothing was launched


def test_lengths_on_a_streamed_path_graph_are_refused_by_the_value_entry(kernel_family):
    kernel_family("force_streamed")
    fst = synth.random_den_fst(40, 4, 24)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    P, fake = fst.num_pdfs, C.c_void_p(4096)
    need = int(lib.tc_den_expected_accuracy_workspace_bytes(graph.ptr, S, T))
    before = int(lib.tc_debug_counter(b"den_launches"))
    assert lib.tc_den_expected_accuracy_dense(graph.ptr, S, fake, S * T, P, P, fake, T, 1e-5, fake, P, fake, P, fake, fake, fake,
                                              need, 0, None) == TC_ERR_UNSUPPORTED
    assert int(lib.tc_debug_counter(b"den_launches")) == before


def test_header_documents_the_entries():
    import os
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "torchain_hip.h")).read()
    doc = text[:text.index("int tc_den_expected_accuracy_dense(")].rsplit("/*", 1)[1]
    for phrase in ("accuracy_stride", "TC_ERR_INVALID_ARGUMENT", "TC_ERR_WORKSPACE", "TC_ERR_UNSUPPORTED",
                   "den_accuracy_dense_launches", "den_accuracy_dense_grad_launches", "force_den_accuracy_streamed"):
        assert phrase in doc, phrase
    assert "int tc_den_expected_accuracy_dense_grad(" in text


def test_wrappers_check_before_any_library_call():
    from torchain_amd.functions import den_expected_accuracy_dense, num_posteriors
    fst, graph, pi, y = _case("random")
    P = fst.num_pdfs
    x, a = torch.zeros(S * T, P), torch.zeros(S * T, P)
    with pytest.raises(ValueError, match="CUDA tensor"):
        graph.expected_accuracy_dense(x, a, n_batch=S)
    with pytest.raises(ValueError, match="CUDA tensor"):
        den_expected_accuracy_dense(x, graph, a, n_batch=S)
    with pytest.raises(TypeError, match="io.DenominatorGraph"):
        den_expected_accuracy_dense(x, fst, a, n_batch=S)
    # the checks of `accuracy` need a device tensor in front of them: a meta tensor has shape, dtype and is_cuda of one
    # and no memory, so a library call on it cannot be reached without raising

    class Fake(torch.Tensor):
        is_cuda = True

    xf = torch.zeros(S * T, P, device="meta").as_subclass(Fake)
    for bad, error, match in ((torch.zeros(S * T, P + 1, device="meta"), ValueError, "accuracy of shape"),
                              (torch.zeros(S * T + S, P, device="meta"), ValueError, "accuracy of shape"),
                              (torch.zeros(S, P, T + 1, device="meta"), ValueError, "accuracy of shape"),
                              (torch.zeros(S * T, device="meta"), ValueError, "accuracy must be"),
                              (torch.zeros(S * T, P, dtype=torch.float64, device="meta"), TypeError, "2-D accuracy must be float32"),
                              (torch.zeros(S * T, P, dtype=torch.bfloat16, device="meta"), TypeError, "2-D accuracy must be float32"),
                              (torch.zeros(S, P, T, dtype=torch.int32, device="meta"), TypeError, "accuracy must be float32"),
                              (torch.zeros(S * T, P), ValueError, "on the output's device"),
                              (np.zeros((S * T, P), np.float32), ValueError, "on the output's device")):
        with pytest.raises(error, match=match):
            graph.expected_accuracy_dense(xf, bad, n_batch=S)
    with pytest.raises(ValueError, match="is not"):
        graph.expected_accuracy_dense(torch.zeros(S * T, P + 1, device="meta").as_subclass(Fake), a, n_batch=S)
    # Supervision.posteriors / num_posteriors
    sup = synth.random_supervision(fst, S, T, 3, seed=4)
    hsup = io.Supervision.from_synth(sup)
    with pytest.raises(ValueError, match="CUDA tensor"):
        hsup.posteriors(x)
    with pytest.raises(TypeError, match="io.Supervision"):
        num_posteriors(x, sup)
    with pytest.raises(ValueError, match="does not match the supervision"):
        hsup.posteriors(torch.zeros(S * T, P + 1, device="meta").as_subclass(Fake))
    with pytest.raises(TypeError, match="float32"):
        hsup.posteriors(torch.zeros(S * T, P, dtype=torch.float16, device="meta").as_subclass(Fake))
    with pytest.raises(ValueError, match="pdf_class"):
        hsup.posteriors(xf, pdf_class=np.zeros(P + 1, np.int32))
    sup0 = synth.random_supervision(fst, S, T, 3, seed=4, weight=0.0)
    with pytest.raises(ValueError, match="weight"):
        io.Supervision.from_synth(sup0).posteriors(xf)
    import torchain.functions
    import torchain.io
    assert torchain.functions.den_expected_accuracy_dense is den_expected_accuracy_dense
    assert torchain.functions.num_posteriors is num_posteriors
    assert torchain.io.DenominatorGraph.expected_accuracy_dense is io.DenominatorGraph.expected_accuracy_dense
    assert torchain.io.Supervision.posteriors is io.Supervision.posteriors
