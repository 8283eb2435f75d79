"""The expected frame accuracy over the denominator graph and its gradient on the GPU (``csrc/den_accuracy_kernels.hip``
through ``io.DenominatorGraph.expected_accuracy`` / ``functions.den_expected_accuracy``) against the float64 recursion of
``tests/den_accuracy_reference.py``, which ``tests/test_den_accuracy_host.py`` holds to a double backward through
``oracle/independent_f64``.

Tolerances.  The figures are, per sequence, ``max |gradient - reference| / max |reference gradient of the sequence|``,
``|acc - reference| / T_s`` and ``max_t |frame_acc - reference|``.  The largest measured on the MI355X over the graph
families and the cancellation case below (``profiles/den_accuracy/README.md``) were 1.504e-6, 1.322e-6 and 2.321e-6, all
three in the cancellation case (the families stay below 1.7e-7, 4.4e-8 and 1.3e-7); every bound is 4 x its figure -- the arithmetic is deterministic, the margin covers other seeds and
compilers -- and none is above the project's parity bound of 1e-4.

Ragged batches, non-finite inputs, repeated calls, the form that keeps the per-frame vectors in the workspace, layouts and
dtypes, ``grad_output``, ``no_grad``, an untouched graph handle and allocation-free warm calls are held bit for bit."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import check, lib
from torchain_amd.functions import chain_loss, den_expected_accuracy

import den_accuracy_reference as dar

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAD_MEASURED, ACC_MEASURED, FRAME_MEASURED = 1.504e-6, 1.322e-6, 2.321e-6
GRAD_BOUND, ACC_BOUND, FRAME_BOUND = 4 * GRAD_MEASURED, 4 * ACC_MEASURED, 4 * FRAME_MEASURED
assert max(GRAD_BOUND, ACC_BOUND, FRAME_BOUND) <= 1e-4
# 16 * Hs + 8 * Ps + 1024 <= 163840 (include/torchain_hip.h): the per-frame vectors stay in LDS
RESIDENT_BYTES = 160 * 1024 - 1024


def _counter(key):
    return int(lib.tc_debug_counter(key))


def _counters():
    return tuple(_counter(k) for k in (b"den_accuracy_launches", b"den_accuracy_grad_launches", b"den_accuracy_grad_streamed_launches"))


@functools.lru_cache(maxsize=None)
def _graph(kind):
    fst = {
        "random": lambda: synth.random_den_fst(300, 5, 100, seed=32),
        "nearly_tied": lambda: synth.nearly_tied_den_fst(500, 5, 90, seed=7),
        "skewed_tied": lambda: synth.skewed_tied_den_fst(400, 7000, 150, seed=8),  # hub states: long state and pdf lists
        "skewed": lambda: synth.skewed_den_fst(300, 6000, 120, seed=4),
        "cancel": lambda: synth.random_den_fst(300, 8, 200, seed=11),
    }[kind]()
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    # the reference takes the float32 probabilities the handle holds: the kernel's own table entries
    return fst, graph, graph.initial_probs().astype(np.float64), dar.arcs_of(fst, graph.arcs()[3])


@functools.lru_cache(maxsize=None)
def _inputs(kind, S, T, seed):
    fst = _graph(kind)[0]
    rng = np.random.default_rng(seed)
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=seed)
    ref = rng.integers(0, fst.num_pdfs, size=(S, T)).astype(np.int32)
    ref[S - 1, T // 2] = -1
    cls = rng.integers(0, 5, size=fst.num_pdfs).astype(np.int32)
    return y, ref, cls


@functools.lru_cache(maxsize=None)
def _reference(kind, S, T, seed, leaky, with_class, frames=None):
    fst, graph, pi, arcs = _graph(kind)
    y, ref, cls = _inputs(kind, S, T, seed)
    return dar.batch(arcs, pi, y, S, ref, cls if with_class else None, leaky, frames)


def _run(graph, y, ref, cls, leaky, frames=None, n_batch=None, scale=None):
    """``(acc, frame_acc, grad)`` of one forward call of each entry and one backward call."""
    x = (torch.from_numpy(y) if isinstance(y, np.ndarray) else y).to(DEV).clone().requires_grad_(True)
    if x.dim() == 3:
        n_batch = None
    acc = den_expected_accuracy(x, graph, ref, pdf_class=cls, frames=frames, leaky_hmm_coefficient=leaky, n_batch=n_batch)
    (acc.sum() if scale is None else (acc * scale).sum()).backward()
    acc2, frame_acc = graph.expected_accuracy(x, ref, pdf_class=cls, frames=frames, leaky_hmm_coefficient=leaky, n_batch=n_batch)
    torch.cuda.synchronize()
    assert acc.dtype == torch.float64 and torch.equal(_bits(acc.detach()), _bits(acc2))
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype
    return acc.detach(), frame_acc, x.grad


def _bits(t):
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def _same(a, b):
    return all(u.dtype == v.dtype and u.shape == v.shape and torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))


def _figures(got, want, S, frames=None):
    """The three figures of the module's docstring, the largest over the sequences; printed before anything is asserted."""
    acc, fa, grad = (g.cpu().numpy().astype(np.float64) for g in got)
    wacc, wfa, wgrad = want
    T = fa.shape[1]
    out = np.zeros(3)
    for s in range(S):
        Ts = T if frames is None else int(frames[s])
        peak = np.abs(wgrad[s::S]).max()
        assert peak > 0
        out = np.maximum(out, [np.abs(grad[s::S] - wgrad[s::S]).max() / peak, abs(acc[s] - wacc[s]) / Ts,
                               np.abs(fa[s] - wfa[s]).max()])
    print("MEASURED grad %.3e acc %.3e frame %.3e (E[A] %s, largest gradient %.3g)"
          % (out[0], out[1], out[2], np.array2string(wacc, precision=4), np.abs(wgrad).max()))
    return out


def _hold(figures):
    assert figures[0] <= GRAD_BOUND and figures[1] <= ACC_BOUND and figures[2] <= FRAME_BOUND, figures


# ---- 1. graph families ----
@pytest.mark.parametrize("leaky", [1e-5, 0.1])
@pytest.mark.parametrize("kind", ["random", "nearly_tied", "skewed_tied", "skewed"])
def test_value_and_gradient_agree_with_float64(kind, leaky):
    fst, graph, pi, arcs = _graph(kind)
    S, T = 3, 11
    with_class = leaky > 1e-3  # the identity map with one coefficient, a 5-class map with the other
    y, ref, cls = _inputs(kind, S, T, 61)
    before = _counters()
    got = _run(graph, y, ref, cls if with_class else None, leaky, n_batch=S)
    assert _counters() == (before[0] + 2, before[1] + 1, before[2])
    assert got[0].shape == (S,) and got[1].shape == (S, T) and got[1].dtype == torch.float32
    figures = _figures(got, _reference(kind, S, T, 61, leaky, with_class), S)
    # the reference's rows sum to 0 and every element is within GRAD_BOUND * peak of it: so do these, to P times that
    assert float(got[2].double().sum(dim=1).abs().max()) <= GRAD_BOUND * float(got[2].abs().max()) * fst.num_pdfs
    _hold(figures)


# ---- 2. the case an uncentred float32 recursion fails ----
def test_cancellation_case_with_the_reference_almost_certain():
    fst, graph, pi, arcs = _graph("cancel")
    S, T = 2, 150
    rng = np.random.default_rng(71)
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=72)
    ref = np.stack([dar.random_path(fst, pi, T, rng) for _ in range(S)])
    for s in range(S):
        y[s::S][np.arange(T), ref[s]] += np.float32(6.0)
    want = dar.batch(arcs, pi, y, S, ref, None, 1e-5)
    assert (want[0] > 0.95 * T).all(), want[0]  # (on the CPU, with the reference alone)
    figures = _figures(_run(graph, y, ref, None, 1e-5, n_batch=S), want, S)
    _hold(figures)


# ---- 3. exact properties ----
def test_no_reference_gives_zero():
    fst, graph, pi, arcs = _graph("random")
    S, T = 3, 11
    y, ref, cls = _inputs("random", S, T, 61)
    acc, fa, grad = _run(graph, y, np.full((S, T), -1, np.int32), cls, 0.1, n_batch=S)
    assert bool((acc == 0).all()) and bool((fa == 0).all()) and bool((grad == 0).all())


def test_ragged_batch_padding_is_zero_and_is_not_read():
    fst, graph, pi, arcs = _graph("skewed_tied")
    frames = (11, 7, 1, 4)
    S, T = len(frames), 11
    y, ref, cls = _inputs("skewed_tied", S, T, 62)
    got = _run(graph, y, ref, cls, 0.1, frames=list(frames))
    figures = _figures(got, _reference("skewed_tied", S, T, 62, 0.1, True, frames), S, frames)
    grad = got[2].view(T, S, -1)
    for s, Ts in enumerate(frames):
        assert bool((_bits(grad[Ts:, s]) == 0).all())  # exactly +0
        assert bool((_bits(got[1][s, Ts:]) == 0).all())
        assert bool((grad[:Ts, s] != 0).any())
    planted, ref2 = y.copy(), ref.copy()
    for s, Ts in enumerate(frames):
        planted[s::S][Ts:] = np.nan
        ref2[s, Ts:] = 12345
    assert _same(_run(graph, planted, ref2, cls, 0.1, frames=torch.tensor(frames, device=DEV)), got)
    _hold(figures)


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_input_fails_its_sequence_alone(value):
    fst, graph, pi, arcs = _graph("nearly_tied")
    S, T = 3, 11
    frames = [11, 8, 11]
    y, ref, cls = _inputs("nearly_tied", S, T, 63)
    clean = _run(graph, y, ref, None, 1e-5, frames=frames)
    bad = y.copy()
    bad[5 * S + 1, fst.num_pdfs - 1] = value  # a valid frame of sequence 1
    got = _run(graph, bad, ref, None, 1e-5, frames=frames)
    assert bool(torch.isnan(got[0][1])) and bool(torch.isfinite(clean[0]).all())
    grad, want = got[2].view(T, S, -1), clean[2].view(T, S, -1)
    assert bool((_bits(grad[:, 1]) == 0).all())  # every row of the sequence exactly +0
    for s in (0, 2):
        assert _same((got[0][s], got[1][s], grad[:, s].contiguous()), (clean[0][s], clean[1][s], want[:, s].contiguous()))


def test_repeated_call_gives_the_same_bits():
    fst, graph, pi, arcs = _graph("skewed")
    y, ref, cls = _inputs("skewed", 3, 11, 61)
    assert _same(_run(graph, y, ref, cls, 0.1, n_batch=3), _run(graph, y, ref, cls, 0.1, n_batch=3))


# ---- 4. the form that keeps the per-frame vectors in the workspace ----
@pytest.mark.parametrize("kind", ["random", "skewed_tied"])
def test_both_forms_give_the_same_bits(kernel_family, kind):
    fst, graph, pi, arcs = _graph(kind)
    frames = [11, 4, 8]
    y, ref, cls = _inputs(kind, 3, 11, 61)
    resident = _run(graph, y, ref, cls, 0.1, frames=frames)
    kernel_family("force_den_accuracy_streamed")
    before = _counters()
    assert _same(_run(graph, y, ref, cls, 0.1, frames=frames), resident)
    assert _counters() == (before[0] + 2, before[1] + 1, before[2] + 1)


@pytest.mark.parametrize("H, streamed", [(9824, False), (9828, True)])
def test_graphs_either_side_of_the_lds_bound(kernel_family, H, streamed):
    """700 pdfs: 16 * 9824 + 8 * 700 is the last size that fits the bound, 9828 states are past it; each on its own form."""
    kernel_family("force_streamed")  # (the denominator's own tables: built in a fraction of a second; not what is tested)
    fst = synth.random_den_fst(H, 3, 700, seed=31)
    assert (16 * H + 8 * fst.num_pdfs <= RESIDENT_BYTES) == (not streamed) and H % 4 == 0 and fst.num_pdfs % 4 == 0
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    S, T = 2, 6
    rng = np.random.default_rng(81)
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=82)
    ref = rng.integers(0, fst.num_pdfs, size=(S, T)).astype(np.int32)
    before = _counters()
    got = _run(graph, y, ref, None, 1e-5, n_batch=S)
    assert _counters() == (before[0] + 2, before[1] + 1, before[2] + int(streamed))
    want = dar.batch(dar.arcs_of(fst, graph.arcs()[3]), graph.initial_probs().astype(np.float64), y, S, ref, None, 1e-5)
    _hold(_figures(got, want, S))


# ---- 5. layouts, dtypes, grad_output, no_grad ----
def test_bct_layout_and_bfloat16_match_the_2d_float32_call():
    fst, graph, pi, arcs = _graph("nearly_tied")
    S, T, P = 3, 10, fst.num_pdfs
    y, ref, cls = _inputs("nearly_tied", S, T, 64)
    y2d = torch.from_numpy(y).to(DEV)
    want = _run(graph, y2d, ref, cls, 0.1, n_batch=S)
    x = y2d.view(T, S, P).permute(1, 2, 0).contiguous()  # (S, P, T)
    got = _run(graph, x, ref, cls, 0.1)
    assert _same(got[:2], want[:2]) and _same([got[2]], [want[2].view(T, S, P).permute(1, 2, 0).contiguous()])
    # bfloat16: the call on .float(), the gradient cast
    xb = x.to(torch.bfloat16)
    want = _run(graph, xb.float(), ref, cls, 0.1)
    got = _run(graph, xb, ref, cls, 0.1)
    assert got[2].dtype == torch.bfloat16 and _same(got[:2], want[:2]) and _same([got[2]], [want[2].to(torch.bfloat16)])
    xh = x.to(torch.float16)
    assert _same(_run(graph, xh, ref, cls, 0.1)[:2], _run(graph, xh.float(), ref, cls, 0.1)[:2])


def test_grad_output_scales_each_sequence():
    fst, graph, pi, arcs = _graph("random")
    S, T = 3, 11
    y, ref, cls = _inputs("random", S, T, 61)
    ones = _run(graph, y, ref, cls, 0.1, n_batch=S)
    v = torch.tensor([0.75, -2.0, 1.5], dtype=torch.float64, device=DEV)  # (float32 numbers: the product is one rounding)
    scaled = _run(graph, y, ref, cls, 0.1, n_batch=S, scale=v)
    want = (ones[2].view(T, S, -1).double() * v.view(1, S, 1)).float().view(T * S, -1)
    assert _same([scaled[2]], [want]) and _same(scaled[:2], ones[:2])


def test_no_grad_and_inputs_without_grad_launch_no_gradient_kernel():
    fst, graph, pi, arcs = _graph("random")
    S, T = 3, 11
    y, ref, cls = _inputs("random", S, T, 61)
    x = torch.from_numpy(y).to(DEV)
    before = _counters()
    plain = den_expected_accuracy(x, graph, ref, n_batch=S)
    with torch.no_grad():
        quiet = den_expected_accuracy(x.clone().requires_grad_(True), graph, ref, n_batch=S)
    torch.cuda.synchronize()
    assert _counters() == (before[0] + 2, before[1], before[2])
    assert not plain.requires_grad and not quiet.requires_grad and _same([plain], [quiet])
    with pytest.raises(ValueError, match="bytes of workspace"):
        den_expected_accuracy(x.clone().requires_grad_(True), graph, ref, n_batch=S, max_workspace_bytes=1000)
    assert _counters() == (before[0] + 2, before[1], before[2])


# ---- 6. the graph handle is left alone ----
def _step(den, sup, y):
    x = y.clone().requires_grad_(True)
    loss, res = chain_loss(x, den, sup, l2_regularize=5e-4, leaky_hmm_coefficient=0.1)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), res.data.clone(), x.grad.clone()


@pytest.mark.parametrize("kind", ["random", "skewed"])
def test_training_step_is_the_same_after_the_calls(kind):
    fst = {"random": lambda: synth.random_den_fst(300, 5, 100, seed=32),
           "skewed": lambda: synth.skewed_den_fst(300, 6000, 120, seed=4)}[kind]()
    den = io.DenominatorGraph(fst, fst.num_pdfs)  # a handle of this test's own: the first calls on it are made here
    S, T = 4, 12
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=52))
    y = torch.from_numpy(synth.random_nnet_output(S, T, fst.num_pdfs, seed=53)).to(DEV)
    ref = np.random.default_rng(54).integers(0, fst.num_pdfs, size=(S, T)).astype(np.int32)
    first = _step(den, sup, y)
    before = _counters()
    whole = _run(den, y, ref, None, 0.1, n_batch=S)
    assert _counters()[:2] == (before[0] + 2, before[1] + 1) and bool(torch.isfinite(whole[0]).all())
    second = _step(den, sup, y)
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert _same(_run(den, y, ref, None, 0.1, n_batch=S), whole)  # ... and the step leaves the accuracy alone


# ---- 7. warm calls allocate nothing ----
def test_warm_calls_allocate_nothing():
    fst, graph, pi, arcs = _graph("random")
    S, T, P = 4, 10, fst.num_pdfs
    y, ref, cls = _inputs("random", S, T, 65)
    y, ref, cls = torch.from_numpy(y).to(DEV), torch.from_numpy(ref).to(DEV), torch.from_numpy(cls).to(DEV)
    ws = torch.empty(max(int(lib.tc_den_expected_accuracy_workspace_bytes(graph.ptr, S, T)),
                         int(lib.tc_den_expected_accuracy_grad_workspace_bytes(graph.ptr, S, T))), dtype=torch.uint8, device=DEV)
    gamma, grad = torch.empty((T * S, P), device=DEV), torch.empty((T * S, P), device=DEV)
    fa, acc = torch.empty((S, T), device=DEV), torch.empty((S,), dtype=torch.float64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        check(lib.tc_den_expected_accuracy(graph.ptr, S, p(y), S * T, P, P, None, T, 0.1, p(ref), p(cls), p(gamma), P, p(fa),
                                           p(acc), p(ws), ws.numel(), 0, stream), "tc_den_expected_accuracy")
        check(lib.tc_den_expected_accuracy_grad(graph.ptr, S, p(y), S * T, P, P, None, T, 0.1, p(ref), p(cls), p(fa), None,
                                                p(grad), P, p(ws), ws.numel(), 0, stream), "tc_den_expected_accuracy_grad")
        torch.cuda.synchronize()

    call()
    first = [o.clone() for o in (acc, fa, grad)]
    gc.collect()  # (what earlier tests left to the collector goes now, not during the calls below)
    level = torch.cuda.memory_allocated(), _counter(b"pool_device_allocs")
    for _ in range(3):
        for o in (acc, fa, grad, gamma):
            o.fill_(-7)
        call()
        assert (torch.cuda.memory_allocated(), _counter(b"pool_device_allocs")) == level
        assert _same((acc, fa, grad), first)
    # gamma is the by-product the header documents: the denominator posteriors, rows that sum to 1
    assert float((gamma.sum(dim=1) - 1).abs().max()) <= 1e-4
    assert _same(first, _run(graph, y, ref, cls, 0.1, n_batch=S))  # the wrappers add nothing to the bits
