"""Arc and entry occupations of the denominator graph on the GPU (``csrc/den_arc_post_kernels.hip`` through
``io.DenominatorGraph.arc_posteriors`` / ``functions.den_arc_posteriors``) against the float64 autograd recursion of
``tests/den_arc_post_reference.py``.

Tolerances.  A figure is ``max |got - reference| / max |reference|`` over one output: the totals ``arcs`` and ``entries``, the
rows ``per_seq_arcs`` and ``per_seq_entries``, ``leaks`` and ``logprob``.  The largest measured on the MI355X over the cases
below are in ``MEASURED`` (``profiles/den_arc_post/README.md``); every bound is 4 x its figure -- the arithmetic is
deterministic, the margin covers other seeds and compilers.  The identities are held to the same bounds scaled by the sums.
Everything else is held bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import check, lib
from torchain_amd.functions import chain_loss, den_arc_posteriors

import den_arc_post_reference as dap
from fixtures import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S, T, RAGGED = 3, 7, (7, 4, 1)
MEASURED = {"arcs": 1.571e-7, "entries": 1.588e-7, "per_seq_arcs": 1.693e-7, "per_seq_entries": 2.182e-7, "leaks": 1.434e-7,
            "logprob": 1.89e-8}
BOUND = {k: 4 * v for k, v in MEASURED.items()}
GRAPHS = ["one_wave", "hubs", "many_states", "skewed"]
CASES = [(k, c, r) for k in GRAPHS for c in (1e-5, 0.2) for r in (False, True)]


def _hub_fst():
    """200 states of two arcs each, state 3 with an arc to every state and every state with an arc to state 5: one list of
    more than 128 out-arcs, one of more than 128 in-arcs."""
    base = synth.random_den_fst(200, 2, 40, seed=9)
    H, rng = 200, np.random.default_rng(10)
    src = np.concatenate([base.src, np.full(H, 3), np.arange(H)]).astype(np.int32)
    dst = np.concatenate([base.dst, np.arange(H), np.full(H, 5)]).astype(np.int32)
    ilabel = np.concatenate([base.ilabel, rng.integers(1, 41, size=2 * H)]).astype(np.int32)
    prob = np.concatenate([np.exp(-base.weight.astype(np.float64)), rng.uniform(0.1, 1.0, size=2 * H)])
    order = np.argsort(src, kind="stable")
    src, dst, ilabel, prob = src[order], dst[order], ilabel[order], prob[order]
    prob /= np.bincount(src, weights=prob, minlength=H)[src]
    return synth.DenFst(H, src, dst, ilabel, (-np.log(prob)).astype(np.float32), np.zeros(H, np.float32), 0, 40)


@functools.lru_cache(maxsize=None)
def _graph(kind):
    fst = {"one_wave": lambda: synth.random_den_fst(37, 3, 11),
           "hubs": _hub_fst,
           "many_states": lambda: synth.random_den_fst(1100, 2, 70),
           "skewed": lambda: load_golden([g for g in GOLDEN if g.endswith("skewed_graph.npz")][0])[1]}[kind]()
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    y = np.random.default_rng(77).normal(0.0, 2.0, size=(T * S, fst.num_pdfs)).astype(np.float32)
    return fst, graph, y


@functools.lru_cache(maxsize=None)
def _want(kind, leaky, ragged):
    _, graph, y = _graph(kind)
    return dap.occupations(graph.arcs(), graph.initial_probs(), y, S, leaky, RAGGED if ragged else None)


def _call(kind, leaky, ragged, y=None, **kw):
    _, graph, y0 = _graph(kind)
    x = torch.from_numpy(y0).to(DEV) if y is None else y
    post = den_arc_posteriors(x, graph, frames=list(RAGGED) if ragged else None, leaky_hmm_coefficient=leaky, per_sequence=True,
                              n_batch=None if ragged or x.dim() == 3 else S, **kw)
    torch.cuda.synchronize()
    return post


@functools.lru_cache(maxsize=None)
def _got(kind, leaky, ragged):
    return _call(kind, leaky, ragged)


def _bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return all(u.dtype == v.dtype and u.shape == v.shape and torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))


def _counter(key):
    return int(lib.tc_debug_counter(key))


# ---- 1. against float64 ----
@pytest.mark.parametrize("kind,leaky,ragged", CASES)
def test_against_float64(kind, leaky, ragged):
    got, want = _got(kind, leaky, ragged), dict(_want(kind, leaky, ragged))
    want["per_seq_arcs"], want["per_seq_entries"] = want["arcs"], want["entries"]
    want["arcs"], want["entries"] = want["arcs"].sum(0), want["entries"].sum(0)
    figures = {k: np.abs(getattr(got, k).cpu().numpy().astype(np.float64) - w).max() / np.abs(w).max() for k, w in want.items()}
    print("MEASURED " + " ".join("%s %.3e" % kv for kv in figures.items()))
    assert got.arcs.dtype == got.entries.dtype == got.leaks.dtype == got.logprob.dtype == torch.float64
    assert all(figures[k] <= BOUND[k] for k in BOUND), figures


# ---- 2. identities ----
@pytest.mark.parametrize("kind,leaky,ragged", CASES)
def test_identities(kind, leaky, ragged):
    fst, graph, y = _graph(kind)
    got, lens = _got(kind, leaky, ragged), RAGGED if ragged else (T,) * S
    assert abs(float(got.arcs.sum()) - sum(lens)) <= BOUND["arcs"] * sum(lens)
    assert abs(float(got.entries.sum()) - S - float(got.leaks.sum())) <= BOUND["entries"] * (S + float(got.leaks.sum()))
    # the arcs of a pdf against the denominator posteriors of the tuned kernels, summed over the frames
    yt = torch.from_numpy(y).to(DEV)
    gamma = torch.zeros_like(yt)
    graph.prepare(yt.device)
    frames = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.tc_chain_workspace_bytes(graph.ptr, S, T), dtype=torch.uint8, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    check(lib.tc_den_forward_backward_ragged(graph.ptr, S, ptr(yt), S * T, yt.shape[1], yt.stride(0), leaky, 1.0, 0.0, 0, ptr(gamma),
                                             gamma.stride(0), ptr(frames), T, None, None, ptr(ws), ws.numel(),
                                             torch.cuda.current_device(), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "tc_den_forward_backward_ragged")
    torch.cuda.synchronize()
    by_pdf = torch.zeros(fst.num_pdfs, dtype=torch.float64, device=DEV)
    by_pdf.index_add_(0, torch.as_tensor(graph.arcs()[2]).long().to(DEV), got.arcs)
    assert float((by_pdf - gamma.double().sum(0)).abs().max()) <= BOUND["arcs"] * sum(lens)


# ---- 3. bit for bit ----
@pytest.mark.parametrize("kind", GRAPHS)
def test_rows_totals_forms_groups_dtypes_and_warm_calls(kind):
    _, graph, y = _graph(kind)
    whole = _got(kind, 0.2, True)
    assert _same(_call(kind, 0.2, True), whole)  # a warm call
    # a sequence alone gives its row of the batch
    x = torch.from_numpy(y).to(DEV).view(T, S, -1)
    for s, n in enumerate(RAGGED):
        one = den_arc_posteriors(x[:, s].contiguous(), graph, frames=[n], leaky_hmm_coefficient=0.2, per_sequence=True)
        assert _same((one.per_seq_arcs[0], one.per_seq_entries[0], one.leaks[0], one.logprob[0]),
                     (whole.per_seq_arcs[s], whole.per_seq_entries[s], whole.leaks[s], whole.logprob[s]))
    # the totals are the double sums of the rows in sequence order
    for total, rows in ((whole.arcs, whole.per_seq_arcs), (whole.entries, whole.per_seq_entries)):
        acc = torch.zeros_like(total)
        for s in range(S):
            acc = acc + rows[s].double()
        assert _same((total,), (acc,))
    # the accumulators in the workspace (1), and the per-state vectors there too (3)
    for value in (1, 3):
        before = _counter(b"den_arc_post_streamed_launches")
        check(lib.tc_debug_set(b"force_den_arc_post_streamed", value), "tc_debug_set")
        try:
            forced = _call(kind, 0.2, True)
        finally:
            check(lib.tc_debug_set(b"force_den_arc_post_streamed", 0), "tc_debug_set")
        assert _counter(b"den_arc_post_streamed_launches") == before + 1 and _same(forced, whole)
    # two groups of sequences
    need = int(lib.tc_den_arc_posteriors_workspace_bytes(graph.ptr, 2, T))
    before = _counter(b"den_arc_post_launches")
    assert _same(_call(kind, 0.2, True, max_workspace_bytes=need), whole) and _counter(b"den_arc_post_launches") == before + 2
    # a bfloat16 (B, C, T) tensor against its float32 rows
    xb = x.permute(1, 2, 0).contiguous().to(torch.bfloat16)
    assert _same(_call(kind, 0.2, True, y=xb), _call(kind, 0.2, True, y=xb.float().permute(2, 0, 1).reshape(T * S, -1).contiguous()))


def test_training_step_is_the_same_after_a_call():
    fst = synth.random_den_fst(300, 5, 100, seed=32)
    den = io.DenominatorGraph(fst, fst.num_pdfs)  # a handle of this test's own: the first calls on it are made here
    sup = io.Supervision.from_synth(synth.random_supervision(fst, 4, 12, 3, seed=52))
    y = torch.from_numpy(synth.random_nnet_output(4, 12, fst.num_pdfs, seed=53)).to(DEV)

    def step():
        x = y.clone().requires_grad_(True)
        loss, res = chain_loss(x, den, sup, l2_regularize=5e-4, leaky_hmm_coefficient=0.1)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), res.data.clone(), x.grad.clone()

    first = step()
    post = den_arc_posteriors(y, den, n_batch=4, leaky_hmm_coefficient=0.1)
    assert abs(float(post.arcs.sum()) - 48) <= BOUND["arcs"] * 48
    assert _same(step(), first)


# ---- 4. non-finite ----
def test_a_nan_costs_its_sequence_alone():
    kind = "hubs"
    whole, y = _got(kind, 0.2, True), torch.from_numpy(_graph(kind)[2]).to(DEV)
    pad = y.clone()
    pad[5 * S + 1, 3] = float("nan")  # frame 5 of sequence 1, which has 4
    assert _same(_call(kind, 0.2, True, y=pad), whole)
    bad = y.clone()
    bad[2 * S + 1, 3] = float("nan")
    got = _call(kind, 0.2, True, y=bad)
    for rows, ok in ((got.per_seq_arcs, whole.per_seq_arcs), (got.per_seq_entries, whole.per_seq_entries)):
        assert int(_bits(rows[1]).abs().max()) == 0 and _same((rows[0], rows[2]), (ok[0], ok[2]))
    assert bool(got.logprob[1].isnan()) and bool(got.leaks[1].isnan())
    assert _same((got.logprob[[0, 2]], got.leaks[[0, 2]]), (whole.logprob[[0, 2]], whole.leaks[[0, 2]]))
    assert _same((got.arcs,), (got.per_seq_arcs[0].double() + got.per_seq_arcs[2].double(),))
