"""Lattice-free sMBR against soft references on the GPU: the dense instantiations of ``csrc/den_accuracy_kernels.hip`` through
``io.DenominatorGraph.expected_accuracy_dense`` / ``functions.den_expected_accuracy_dense``, and the numerator posteriors of
``io.Supervision.posteriors`` that Kaldi's chain-sMBR feeds them.

Two yardsticks.  Where the dense matrix is the float32 indicator of a hard reference, the hard entries of
``tests/test_gpu_den_accuracy.py`` are the reference, bit for bit (``g * 1 + m`` and ``g * 0 + m`` are exact, fused or not).
Where it is soft -- Dirichlet rows, numerator posteriors, signed rewards -- the float64 recursion of
``tests/den_accuracy_dense_reference.py`` is, which ``tests/test_den_accuracy_dense_host.py`` holds to a double backward
through ``oracle/independent_f64``.  The figures and the bounds are the hard module's: per sequence
``max |gradient - reference| / max |reference gradient of the sequence|``, ``|acc - reference| / T_s`` and
``max_t |frame_acc - reference|`` against ``GRAD_BOUND``, ``ACC_BOUND`` and ``FRAME_BOUND`` (restated below, held equal to that
module's).  With ``|a - m| <= 1`` the error analysis is the hard form's; the rewards, which are not, are held on the
gradient figure alone, which does not change with the scale of ``a``.  The largest figures measured on the MI355X are in
``profiles/den_accuracy_dense/README.md``.

Scaling by 4, the gradient in ``accuracy``, ragged batches, non-finite values, the two forms of the gradient kernel, layouts
and dtypes, groups of sequences, repeated and warm calls and an untouched graph or supervision handle are held bit for bit."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import check, lib
from torchain_amd.functions import chain_loss, den_expected_accuracy_dense, num_posteriors

import den_accuracy_dense_reference as ddr
import den_accuracy_reference as dar
import e2e_reference
import num_elementwise_cases as nc
import test_gpu_den_accuracy as hard  # the hard entries' module: its graphs, inputs and bounds
import wide_supervisions as ws
from helpers import posteriors_elementwise

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAD_BOUND, ACC_BOUND, FRAME_BOUND = 4 * 1.504e-6, 4 * 1.322e-6, 4 * 2.321e-6
assert (GRAD_BOUND, ACC_BOUND, FRAME_BOUND) == (hard.GRAD_BOUND, hard.ACC_BOUND, hard.FRAME_BOUND)
KINDS = ["random", "nearly_tied", "skewed_tied", "skewed"]
KEYS = (b"den_accuracy_launches", b"den_accuracy_grad_launches", b"den_accuracy_grad_streamed_launches",
        b"den_accuracy_dense_launches", b"den_accuracy_dense_grad_launches")
_bits, _same = hard._bits, hard._same


def _counters():
    return tuple(int(lib.tc_debug_counter(k)) for k in KEYS)


def _plus(before, value=0, grad=0, streamed=0):
    return (before[0] + value, before[1] + grad, before[2] + streamed, before[3] + value, before[4] + grad)


def _dev(v):
    # (an array is copied first: the shared ones are read-only)
    return (torch.from_numpy(np.array(v)) if isinstance(v, np.ndarray) else v).to(DEV)


def _run(graph, y, a, leaky, frames=None, n_batch=None, scale=None, **kw):
    """``(acc, frame_acc, grad)`` of one forward call of each entry and one backward call in ``input``."""
    x = _dev(y).clone().requires_grad_(True)
    a = _dev(a)
    if x.dim() == 3:
        n_batch = None
    kw.update(frames=frames, leaky_hmm_coefficient=leaky, n_batch=n_batch)
    acc = den_expected_accuracy_dense(x, graph, a, **kw)
    (acc.sum() if scale is None else (acc * scale).sum()).backward()
    acc2, frame_acc = graph.expected_accuracy_dense(x, a, **kw)
    torch.cuda.synchronize()
    assert acc.dtype == torch.float64 and torch.equal(_bits(acc.detach()), _bits(acc2))
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype
    return acc.detach(), frame_acc, x.grad


def _figures(got, want, S, frames=None, what=""):
    """The three figures of the module's docstring, the largest over the sequences; printed before anything is asserted."""
    acc, fa, grad = (g.cpu().numpy().astype(np.float64) for g in got[:3])
    wacc, wfa, wgrad = want[:3]
    T = fa.shape[1]
    out = np.zeros(3)
    for s in range(S):
        Ts = T if frames is None else int(frames[s])
        peak = np.abs(wgrad[s::S]).max()
        assert peak > 0
        out = np.maximum(out, [np.abs(grad[s::S] - wgrad[s::S]).max() / peak, abs(acc[s] - wacc[s]) / Ts,
                               np.abs(fa[s] - wfa[s]).max()])
    print("MEASURED %s grad %.3e acc %.3e frame %.3e (E[A] %s, largest gradient %.3g)"
          % (what, out[0], out[1], out[2], np.array2string(wacc, precision=4), np.abs(wgrad).max()))
    return out


def _hold(figures):
    assert figures[0] <= GRAD_BOUND and figures[1] <= ACC_BOUND and figures[2] <= FRAME_BOUND, figures


@functools.lru_cache(maxsize=None)
def _supervision(kind, S, T):
    return io.Supervision.from_synth(synth.random_supervision(hard._graph(kind)[0], S, T, 3, seed=52))


@functools.lru_cache(maxsize=None)
def _soft(kind, soft, S, T, seed):
    """A float32 accuracy matrix ``(T*S, P)`` for the outputs ``hard._inputs(kind, S, T, seed)``: Dirichlet rows, the numerator
    posteriors of a three-path supervision under those outputs (from the GPU), or signed rewards N(0, 9)."""
    fst = hard._graph(kind)[0]
    P = fst.num_pdfs
    rng = np.random.default_rng(seed + 100)
    if soft == "dirichlet":
        a = rng.dirichlet(np.full(P, 0.3), size=S * T).astype(np.float32)
    elif soft == "rewards":
        a = rng.normal(scale=3.0, size=(S * T, P)).astype(np.float32)
    else:
        y = hard._inputs(kind, S, T, seed)[0]
        a = _supervision(kind, S, T).posteriors(_dev(y)).cpu().numpy()
        assert np.abs(a.sum(axis=1) - 1).max() <= 1e-5 and (a >= 0).all()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _reference(kind, soft, S, T, seed, leaky, frames=None):
    fst, graph, pi, arcs = hard._graph(kind)
    return ddr.batch(arcs, pi, hard._inputs(kind, S, T, seed)[0], S, _soft(kind, soft, S, T, seed), leaky, frames)


# ---- 1. an indicator matrix gives the hard entries' bits ----
@pytest.mark.parametrize("with_class", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_one_hot_matrix_equals_the_hard_reference_bit_for_bit(kind, with_class):
    fst, graph, pi, arcs = hard._graph(kind)
    S, T = 3, 11
    y, ref, cls = hard._inputs(kind, S, T, 61)
    assert ref[S - 1, T // 2] == -1  # one frame without a reference
    cls = cls if with_class else None
    a = ddr.indicator(ref, cls, fst.num_pdfs, S)
    leaky = 0.1 if with_class else 1e-5
    want = hard._run(graph, y, ref, cls, leaky, n_batch=S)
    before = _counters()
    got = _run(graph, y, a, leaky, n_batch=S)
    assert _counters() == _plus(before, value=2, grad=1)
    assert bool((got[2] != 0).any()) and _same(got, want)


# ---- 2. soft references against float64 ----
@pytest.mark.parametrize("leaky", [1e-5, 0.1])
@pytest.mark.parametrize("soft", ["dirichlet", "numerator"])
@pytest.mark.parametrize("kind", KINDS)
def test_soft_references_agree_with_float64(kind, soft, leaky):
    fst, graph, pi, arcs = hard._graph(kind)
    S, T = 3, 11
    y = hard._inputs(kind, S, T, 61)[0]
    a = _soft(kind, soft, S, T, 61)
    got = _run(graph, y, a, leaky, n_batch=S)
    assert got[0].shape == (S,) and got[1].shape == (S, T) and got[1].dtype == torch.float32
    figures = _figures(got, _reference(kind, soft, S, T, 61, leaky), S, what="%s %s c=%g" % (kind, soft, leaky))
    assert float(got[2].double().sum(dim=1).abs().max()) <= GRAD_BOUND * float(got[2].abs().max()) * fst.num_pdfs
    _hold(figures)


# ---- 3. scaling ----
@pytest.mark.parametrize("kind", ["random", "skewed_tied"])
def test_four_times_the_matrix_gives_four_times_every_output(kind):
    fst, graph, pi, arcs = hard._graph(kind)
    S, T = 3, 11
    y = hard._inputs(kind, S, T, 61)[0]
    a = _soft(kind, "dirichlet", S, T, 61)
    one, four = _run(graph, y, a, 0.1, n_batch=S), _run(graph, y, a * np.float32(4), 0.1, n_batch=S)
    assert _same(four, [o * 4 for o in one])


@pytest.mark.parametrize("leaky", [1e-5, 0.1])
@pytest.mark.parametrize("kind", KINDS)
def test_signed_rewards_agree_with_float64_on_the_gradient(kind, leaky):
    fst, graph, pi, arcs = hard._graph(kind)
    S, T = 3, 11
    y = hard._inputs(kind, S, T, 61)[0]
    a = _soft(kind, "rewards", S, T, 61)
    assert a.min() < -6 and a.max() > 6
    got = _run(graph, y, a, leaky, n_batch=S)
    figures = _figures(got, _reference(kind, "rewards", S, T, 61, leaky), S, what="%s rewards c=%g" % (kind, leaky))
    assert figures[0] <= GRAD_BOUND, figures


# ---- 4. the gradient in `accuracy` ----
def test_gradient_in_accuracy_is_grad_output_times_the_denominator_posteriors():
    kind, frames = "nearly_tied", [11, 8, 11, 5]
    fst, graph, pi, arcs = hard._graph(kind)
    S, T, P = 4, 11, fst.num_pdfs
    y = hard._inputs(kind, S, T, 63)[0].copy()
    y[5 * S + 2, 3] = np.nan  # sequence 2 fails
    a = _soft(kind, "dirichlet", S, T, 63)
    v = torch.tensor([0.75, -2.0, 1.5, -0.5], dtype=torch.float64, device=DEV)  # (float32 numbers: one rounding a product)
    x, at = _dev(y).requires_grad_(True), _dev(a).requires_grad_(True)
    acc = den_expected_accuracy_dense(x, graph, at, frames=frames, leaky_hmm_coefficient=0.1)
    (acc * v).sum().backward()
    acc2, fa, gamma = graph.expected_accuracy_dense(x, at, frames=frames, leaky_hmm_coefficient=0.1, return_posteriors=True)
    torch.cuda.synchronize()
    assert _same([acc.detach()], [acc2]) and bool(torch.isnan(acc[2])) and int(torch.isnan(acc).sum()) == 1
    assert at.grad.shape == at.shape and at.grad.dtype == torch.float32 and gamma.shape == (T * S, P)
    ga, gm = at.grad.view(T, S, P), gamma.view(T, S, P)
    want = ddr.batch(arcs, pi, np.nan_to_num(y), S, a, 0.1, frames)[3].reshape(T, S, P)
    for s, Ts in enumerate(frames):
        assert bool((_bits(ga[Ts:, s]) == 0).all())  # padding rows: exactly +0, whatever grad_output's sign
        assert bool((_bits(gm[Ts:, s]) == 0).all())
        if s == 2:
            assert bool((_bits(ga[:, s]) == 0).all()) and bool((_bits(x.grad.view(T, S, P)[:, s]) == 0).all())
            continue
        assert _same([ga[:Ts, s].contiguous()], [(gm[:Ts, s] * v[s].float()).contiguous()])
        err = np.abs(gm[:Ts, s].cpu().numpy().astype(np.float64) - want[:Ts, s]).max()
        print("MEASURED gamma sequence %d: %.3e" % (s, err))
        assert err <= FRAME_BOUND
        assert bool((ga[:Ts, s] != 0).any())


def test_each_gradient_runs_only_where_it_is_asked_for():
    fst, graph, pi, arcs = hard._graph("random")
    S, T = 3, 11
    y, a = _dev(hard._inputs("random", S, T, 61)[0]), _dev(_soft("random", "dirichlet", S, T, 61))
    both = _run(graph, y, a, 0.1, n_batch=S)
    # input alone: one gradient launch, and no gradient in the matrix
    x, at = y.clone().requires_grad_(True), a.clone()
    before = _counters()
    den_expected_accuracy_dense(x, graph, at, n_batch=S, leaky_hmm_coefficient=0.1).sum().backward()
    torch.cuda.synchronize()
    assert _counters() == _plus(before, value=1, grad=1) and at.grad is None and _same([x.grad], [both[2]])
    # the matrix alone: no gradient launch
    x, at = y.clone(), a.clone().requires_grad_(True)
    before = _counters()
    den_expected_accuracy_dense(x, graph, at, n_batch=S, leaky_hmm_coefficient=0.1).sum().backward()
    gamma = graph.expected_accuracy_dense(x, at, n_batch=S, leaky_hmm_coefficient=0.1, return_posteriors=True)[2]
    torch.cuda.synchronize()
    assert _counters() == _plus(before, value=2, grad=0) and x.grad is None and _same([at.grad], [gamma])
    # neither, and no_grad: the value alone
    before = _counters()
    plain = den_expected_accuracy_dense(y, graph, a, n_batch=S, leaky_hmm_coefficient=0.1)
    with torch.no_grad():
        quiet = den_expected_accuracy_dense(y.clone().requires_grad_(True), graph, a.clone().requires_grad_(True), n_batch=S,
                                            leaky_hmm_coefficient=0.1)
    torch.cuda.synchronize()
    assert _counters() == _plus(before, value=2, grad=0)
    assert not plain.requires_grad and not quiet.requires_grad and _same([plain, quiet], [both[0], both[0]])


# ---- 5. ragged batches ----
def test_ragged_batch_every_sequence_has_the_bits_of_the_call_on_it_alone():
    kind, frames = "skewed_tied", (11, 7, 1, 9)
    fst, graph, pi, arcs = hard._graph(kind)
    S, T, P = len(frames), 11, fst.num_pdfs
    y = hard._inputs(kind, S, T, 62)[0]
    a = _soft(kind, "dirichlet", S, T, 62)
    got = _run(graph, y, a, 0.1, frames=list(frames))
    figures = _figures(got, _reference(kind, "dirichlet", S, T, 62, 0.1, frames), S, frames, what="ragged")
    grad = got[2].view(T, S, P)
    for s, Ts in enumerate(frames):
        assert bool((_bits(grad[Ts:, s]) == 0).all())  # exactly +0
        assert bool((_bits(got[1][s, Ts:]) == 0).all())
        assert bool((grad[:Ts, s] != 0).any())
    # padding of y and of the matrix filled with NaN reaches nothing
    py, pa = y.copy(), a.copy()
    for s, Ts in enumerate(frames):
        py[s::S][Ts:] = np.nan
        pa[s::S][Ts:] = np.nan
    assert _same(_run(graph, py, pa, 0.1, frames=torch.tensor(frames, device=DEV)), got)
    # ... and each sequence alone: its own rows (the padding still NaN), its own length
    for s, Ts in enumerate(frames):
        alone = _run(graph, py[s::S], pa[s::S], 0.1, frames=[Ts])
        assert _same(alone, (got[0][s:s + 1], got[1][s:s + 1], grad[:, s].contiguous())), s
    _hold(figures)


# ---- 6. non-finite values ----
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["accuracy", "output"])
def test_non_finite_value_fails_its_sequence_alone(where, value):
    kind = "nearly_tied"
    fst, graph, pi, arcs = hard._graph(kind)
    S, T, P = 3, 11, fst.num_pdfs
    frames = [11, 8, 11]
    y = hard._inputs(kind, S, T, 63)[0]
    a = _soft(kind, "dirichlet", S, T, 63)
    clean = _run(graph, y, a, 1e-5, frames=frames)
    by, ba = y.copy(), a.copy()
    (ba if where == "accuracy" else by)[5 * S + 1, P - 1] = value  # a valid frame of sequence 1
    got = _run(graph, by, ba, 1e-5, frames=frames)
    assert bool(torch.isnan(got[0][1])) and bool(torch.isfinite(clean[0]).all())
    assert bool(torch.isnan(got[1][1, :8]).all()) and bool((_bits(got[1][1, 8:]) == 0).all())
    grad, want = got[2].view(T, S, -1), clean[2].view(T, S, -1)
    assert bool((_bits(grad[:, 1]) == 0).all())  # every row of the sequence exactly +0
    for s in (0, 2):
        assert _same((got[0][s], got[1][s], grad[:, s].contiguous()), (clean[0][s], clean[1][s], want[:, s].contiguous()))
    # past the sequence's length the same value is padding
    by, ba = y.copy(), a.copy()
    (ba if where == "accuracy" else by)[9 * S + 1, 0] = value
    assert _same(_run(graph, by, ba, 1e-5, frames=frames), clean)


# ---- 7. the two forms of the gradient kernel ----
@pytest.mark.parametrize("kind", ["random", "skewed_tied"])
def test_both_forms_give_the_same_bits(kernel_family, kind):
    fst, graph, pi, arcs = hard._graph(kind)
    frames = [11, 4, 8]
    y = hard._inputs(kind, 3, 11, 61)[0]
    a = _soft(kind, "dirichlet", 3, 11, 61)
    resident = _run(graph, y, a, 0.1, frames=frames)
    kernel_family("force_den_accuracy_streamed")
    before = _counters()
    assert _same(_run(graph, y, a, 0.1, frames=frames), resident)
    assert _counters() == _plus(before, value=2, grad=1, streamed=1)


@pytest.mark.parametrize("H, streamed", [(9824, False), (9828, True)])
def test_graphs_either_side_of_the_lds_bound(kernel_family, H, streamed):
    """The two sizes of the hard module's test: 700 pdfs, 16 * 9824 + 8 * 700 is the last size that fits the bound."""
    kernel_family("force_streamed")  # (the denominator's own tables: built in a fraction of a second; not what is tested)
    fst = synth.random_den_fst(H, 3, 700, seed=31)
    assert (16 * H + 8 * fst.num_pdfs <= hard.RESIDENT_BYTES) == (not streamed)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    S, T = 2, 5
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=82)
    a = np.random.default_rng(83).dirichlet(np.full(fst.num_pdfs, 0.3), size=S * T).astype(np.float32)
    before = _counters()
    got = _run(graph, y, a, 1e-5, n_batch=S)
    assert _counters() == _plus(before, value=2, grad=1, streamed=int(streamed))
    want = ddr.batch(dar.arcs_of(fst, graph.arcs()[3]), graph.initial_probs().astype(np.float64), y, S, a, 1e-5)
    figures = _figures(got, want, S, what="%d states" % H)
    kernel_family("force_den_accuracy_streamed")
    before = _counters()
    assert _same(_run(graph, y, a, 1e-5, n_batch=S), got)  # (the other form where there is one)
    assert _counters() == _plus(before, value=2, grad=1, streamed=1)
    _hold(figures)


# ---- 8. layouts and dtypes, of the two arguments independently ----
@pytest.mark.parametrize("a_form", ["2d", "bct", "bct_bf16"])
@pytest.mark.parametrize("x_form", ["2d", "bct", "bct_bf16"])
def test_layouts_and_dtypes_match_the_2d_float32_call(x_form, a_form):
    kind = "nearly_tied"
    fst, graph, pi, arcs = hard._graph(kind)
    S, T, P = 3, 10, fst.num_pdfs
    y2d = _dev(hard._inputs(kind, S, T, 64)[0])
    a2d = _dev(_soft(kind, "dirichlet", S, T, 64))

    def form(m2d, kind_):
        if kind_ == "2d":
            return m2d
        t = m2d.view(T, S, P).permute(1, 2, 0).contiguous()  # (S, P, T)
        return t.to(torch.bfloat16) if kind_ == "bct_bf16" else t

    def back(t):  # the widened values as a 2-D float32 matrix
        return t if t.dim() == 2 else t.float().permute(2, 0, 1).reshape(T * S, P).contiguous()

    x, a = form(y2d, x_form), form(a2d, a_form)
    xw, aw = back(x).clone().requires_grad_(True), back(a).clone().requires_grad_(True)
    v = torch.tensor([0.75, -2.0, 1.5], dtype=torch.float64, device=DEV)
    (den_expected_accuracy_dense(xw, graph, aw, n_batch=S, leaky_hmm_coefficient=0.1) * v).sum().backward()
    want_acc, want_fa = graph.expected_accuracy_dense(xw, aw, n_batch=S, leaky_hmm_coefficient=0.1)
    x, a = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
    kw = dict(leaky_hmm_coefficient=0.1, n_batch=S if x.dim() == 2 else None)
    acc = den_expected_accuracy_dense(x, graph, a, **kw)
    (acc * v).sum().backward()
    fa = graph.expected_accuracy_dense(x, a, **kw)[1]
    torch.cuda.synchronize()
    assert _same([acc.detach(), fa], [want_acc, want_fa])
    for got, want in ((x.grad, xw.grad), (a.grad, aw.grad)):  # the float32 gradient in the argument's layout, rounded once
        if got.dim() == 3:
            want = want.view(T, S, P).permute(1, 2, 0).contiguous()
        assert bool((want != 0).any()) and _same([got], [want.to(got.dtype)])


# ---- 9. groups of sequences ----
def test_groups_of_sequences_give_the_bits_of_one_call():
    kind = "random"
    fst, graph, pi, arcs = hard._graph(kind)
    S, T = 5, 11
    frames = [11, 7, 11, 3, 9]
    y = _dev(hard._inputs(kind, S, T, 66)[0])
    a = _dev(_soft(kind, "dirichlet", S, T, 66))
    need = lambda n: max(int(lib.tc_den_expected_accuracy_workspace_bytes(graph.ptr, n, T)),  # noqa: E731
                         int(lib.tc_den_expected_accuracy_grad_workspace_bytes(graph.ptr, n, T)))
    assert need(3) > need(2) > need(1)
    for fr in (None, frames):
        def run(cap):
            x, at = y.clone().requires_grad_(True), a.clone().requires_grad_(True)
            kw = dict(frames=fr, n_batch=S, leaky_hmm_coefficient=0.1, max_workspace_bytes=cap)
            before = _counters()
            acc = den_expected_accuracy_dense(x, graph, at, **kw)
            value = _counters()[3] - before[3]
            acc.sum().backward()
            grads = _counters()[4] - before[4]
            out = graph.expected_accuracy_dense(x, at, return_posteriors=True, **kw)
            torch.cuda.synchronize()
            assert _same([acc.detach()], [out[0]])
            return (acc.detach(), out[1], out[2], x.grad, at.grad), value, grads

        whole, value, grads = run(8 << 30)
        assert (value, grads) == (1, 1)
        capped, value, grads = run(need(2))
        assert (value, grads) == (3, 3)  # two, two and one sequence
        assert _same(capped, whole)
    # a cap below one sequence's need: refused before anything is launched
    before = _counters()
    with pytest.raises(ValueError, match="bytes of workspace"):
        den_expected_accuracy_dense(y.clone().requires_grad_(True), graph, a, n_batch=S, max_workspace_bytes=need(1) - 1)
    with pytest.raises(ValueError, match="bytes of workspace"):
        graph.expected_accuracy_dense(y, a, n_batch=S, max_workspace_bytes=1000)
    assert _counters() == before


# ---- 10. Supervision.posteriors ----
def _check_posteriors(what, hsup, y, ref, rel):
    """posteriors() of the 2-D float32 output against the float64 posteriors ``ref`` (not weighted), element by element."""
    got = hsup.posteriors(_dev(y))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == y.shape and not got.requires_grad
    posteriors_elementwise(got.cpu().numpy(), ref, 1.0, what + " [posteriors]", rel)
    return got


@pytest.mark.parametrize("scale", nc.SCALES)
@pytest.mark.parametrize("name", nc.RESIDENT + nc.WINDOWED)
def test_posteriors_of_regular_supervisions(name, scale):
    sup, y, want_lp, ref = nc.regular_case(name, scale)
    hsup = io.Supervision.from_synth(sup)
    assert hsup.stats()["kernel"] == (ws.WINDOWED if name in nc.WINDOWED else ws.RESIDENT)
    got = _check_posteriors("%s scale %g" % (name, scale), hsup, y, ref / sup.weight, nc.REL_REGULAR)
    assert _same([num_posteriors(_dev(y), hsup)], [got])


@pytest.mark.parametrize("scale", nc.SCALES)
@pytest.mark.parametrize("name", nc.FORCED)
def test_posteriors_on_the_windowed_kernel_forced(kernel_family, name, scale):
    sup, y, want_lp, ref = nc.regular_case(name, scale)
    hsup = io.Supervision.from_synth(sup)
    kernel_family("force_num_windowed", 1)
    before = int(lib.tc_debug_counter(b"num_windowed_launches"))
    _check_posteriors("%s scale %g, windowed" % (name, scale), hsup, y, ref / sup.weight, nc.REL_REGULAR)
    assert int(lib.tc_debug_counter(b"num_windowed_launches")) == before + 1


@pytest.mark.parametrize("scale", nc.E2E_SCALES)
@pytest.mark.parametrize("name", tuple(nc.E2E))
def test_posteriors_of_end_to_end_supervisions(name, scale):
    fsts, T, P, y, want_lp, ref = nc.e2e_case(name, scale)
    hsup = io.Supervision.from_e2e_fsts(nc.E2E_WEIGHT, T, P, fsts)
    assert hsup.is_e2e
    _check_posteriors("%s scale %g" % (name, scale), hsup, y, ref / nc.E2E_WEIGHT, nc.e2e_rel(name))


def _step(den, sup, y):
    x = y.clone().requires_grad_(True)
    loss, res = chain_loss(x, den, sup, l2_regularize=5e-4, leaky_hmm_coefficient=0.1)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), res.data.clone(), x.grad.clone()


def _same_step(first, second):
    for u, v in zip(first, second):
        assert u.dtype == v.dtype and torch.equal(u.view(torch.int32), v.view(torch.int32))


def _has_path_of(fst, n):
    """Whether an end-to-end acceptor ``(start, arc_begin, ilabel, weight, nextstate, final)`` has a path of ``n`` arcs from
    its start to a final state."""
    start, ab, _, _, nx, final = fst
    at = {int(start)}
    for _ in range(n):
        at = {int(nx[i]) for h in at for i in range(int(ab[h]), int(ab[h + 1]))}
    return any(np.isfinite(final[h]) for h in at)


@pytest.mark.parametrize("e2e", [False, True])
def test_posteriors_of_ragged_handles_layouts_classes_and_an_untouched_handle(e2e):
    fst = synth.random_den_fst(80, 4, 60, seed=31)
    P, frames = 60, [12, 7, 1, 9]
    S, T = len(frames), max(frames)
    den = io.DenominatorGraph(fst, P)
    if e2e:
        rng, fsts = np.random.default_rng(77), []
        while len(fsts) < S:  # random acceptors that have a path of their sequence's length
            f = e2e_reference.random_fst(int(rng.integers(3, 12)), int(rng.integers(8, 40)), P, rng)
            if _has_path_of(f, frames[len(fsts)]):
                fsts.append(f)
        hsup = io.Supervision.from_e2e_fsts(0.7, frames, P, fsts)
    else:
        hsup = io.Supervision.from_sequences([synth.random_supervision(fst, 1, n, 3, seed=20 + n, weight=0.5) for n in frames])
    assert hsup.is_ragged and hsup.is_e2e == e2e and list(hsup.frames) == frames
    y = _dev(synth.random_nnet_output(S, T, P, seed=53))
    first = _step(den, hsup, y)
    post = hsup.posteriors(y)
    torch.cuda.synchronize()
    p3 = post.view(T, S, P)
    for s, Ts in enumerate(frames):
        assert float((p3[:Ts, s].double().sum(dim=1) - 1).abs().max()) <= 1e-5  # valid frames: rows sum to 1
        assert bool((_bits(p3[Ts:, s]) == 0).all())  # padding rows: +0
    assert bool((post >= 0).all())
    assert _same([hsup.posteriors(y)], [post])  # a repeated call
    # (B, C, T) float32 and bfloat16: the 2-D call on the widened values
    bct = y.view(T, S, P).permute(1, 2, 0).contiguous()
    assert _same([hsup.posteriors(bct)], [post])
    half = bct.to(torch.bfloat16)
    assert _same([hsup.posteriors(half)], [hsup.posteriors(half.float().permute(2, 0, 1).reshape(T * S, P).contiguous())])
    # pooled by class: a numpy restatement
    cls = np.random.default_rng(5).integers(-3, 4, size=P).astype(np.int64)  # any values
    pooled = hsup.posteriors(y, pdf_class=cls).cpu().numpy()
    g = post.cpu().numpy().astype(np.float64)
    want = np.stack([g[:, cls == cls[j]].sum(axis=1) for j in range(P)], axis=1)
    assert pooled.dtype == np.float32 and np.abs(pooled - want).max() <= 1e-6 and np.array_equal(pooled == 0, want == 0)
    assert _same([hsup.posteriors(y, pdf_class=torch.from_numpy(cls).to(DEV))], [torch.from_numpy(pooled).to(DEV)])
    # Kaldi's recipe runs, and leaves the training step on the two handles alone
    x = y.clone().requires_grad_(True)
    acc = den_expected_accuracy_dense(x, den, num_posteriors(x, hsup), frames=hsup.frames, leaky_hmm_coefficient=0.1)
    acc.sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(acc).all()) and bool((acc > 0).all()) and bool((acc.cpu() <= torch.tensor(frames)).all())
    assert bool((x.grad != 0).any())
    _same_step(first, _step(den, hsup, y))
    assert _same([hsup.posteriors(y)], [post])


# ---- 11. repeated and warm calls; the graph handle is left alone ----
def test_repeated_call_gives_the_same_bits():
    fst, graph, pi, arcs = hard._graph("skewed")
    y, a = hard._inputs("skewed", 3, 11, 61)[0], _soft("skewed", "numerator", 3, 11, 61)
    assert _same(_run(graph, y, a, 0.1, n_batch=3), _run(graph, y, a, 0.1, n_batch=3))


@pytest.mark.parametrize("kind", ["random", "skewed"])
def test_training_step_is_the_same_after_the_calls(kind):
    fst = {"random": lambda: synth.random_den_fst(300, 5, 100, seed=32),
           "skewed": lambda: synth.skewed_den_fst(300, 6000, 120, seed=4)}[kind]()
    den = io.DenominatorGraph(fst, fst.num_pdfs)  # a handle of this test's own: the first calls on it are made here
    S, T = 4, 12
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=52))
    y = _dev(synth.random_nnet_output(S, T, fst.num_pdfs, seed=53))
    first = _step(den, sup, y)
    a = sup.posteriors(y)
    before = _counters()
    whole = _run(den, y, a, 0.1, n_batch=S)
    assert _counters() == _plus(before, value=2, grad=1) and bool(torch.isfinite(whole[0]).all())
    _same_step(first, _step(den, sup, y))
    assert _same([sup.posteriors(y)], [a]) and _same(_run(den, y, a, 0.1, n_batch=S), whole)


def test_warm_calls_allocate_nothing():
    fst, graph, pi, arcs = hard._graph("random")
    S, T, P = 4, 10, fst.num_pdfs
    y, a = _dev(hard._inputs("random", S, T, 65)[0]), _dev(_soft("random", "dirichlet", S, T, 65))
    nbytes = max(int(lib.tc_den_expected_accuracy_workspace_bytes(graph.ptr, S, T)),
                 int(lib.tc_den_expected_accuracy_grad_workspace_bytes(graph.ptr, S, T)))
    wsp = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    gamma, grad = torch.empty((T * S, P), device=DEV), torch.empty((T * S, P), device=DEV)
    fa, acc = torch.empty((S, T), device=DEV), torch.empty((S,), dtype=torch.float64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        check(lib.tc_den_expected_accuracy_dense(graph.ptr, S, p(y), S * T, P, P, None, T, 0.1, p(a), P, p(gamma), P, p(fa),
                                                 p(acc), p(wsp), wsp.numel(), 0, stream), "tc_den_expected_accuracy_dense")
        check(lib.tc_den_expected_accuracy_dense_grad(graph.ptr, S, p(y), S * T, P, P, None, T, 0.1, p(a), P, p(fa), None,
                                                      p(grad), P, p(wsp), wsp.numel(), 0, stream),
              "tc_den_expected_accuracy_dense_grad")
        torch.cuda.synchronize()

    call()
    first = [o.clone() for o in (acc, fa, grad)]
    gc.collect()  # (what earlier tests left to the collector goes now, not during the calls below)
    level = torch.cuda.memory_allocated(), int(lib.tc_debug_counter(b"pool_device_allocs"))
    for _ in range(3):
        for o in (acc, fa, grad, gamma):
            o.fill_(-7)
        call()
        assert (torch.cuda.memory_allocated(), int(lib.tc_debug_counter(b"pool_device_allocs"))) == level
        assert _same((acc, fa, grad), first)
    assert float((gamma.sum(dim=1) - 1).abs().max()) <= 1e-4
    assert _same(first, _run(graph, y, a, 0.1, n_batch=S))  # the wrappers add nothing to the bits
    # a row stride beyond the columns: the same bits
    wide = torch.full((T * S, P + 4), float("nan"), device=DEV)
    wide[:, :P] = a
    check(lib.tc_den_expected_accuracy_dense_grad(graph.ptr, S, p(y), S * T, P, P, None, T, 0.1, p(wide), P + 4, p(fa), None,
                                                  p(gamma), P, p(wsp), wsp.numel(), 0, stream),
          "tc_den_expected_accuracy_dense_grad")
    torch.cuda.synchronize()
    assert _same([gamma], [first[2]])
