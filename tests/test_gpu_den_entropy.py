"""The entropy of the denominator graph's path posterior on the GPU (``csrc/den_entropy_kernels.hip`` through
``io.DenominatorGraph.path_entropy`` / ``functions.den_path_entropy``) against the float64 autograd reference of
``tests/den_entropy_reference.py``.

Tolerances.  A figure is ``max |got - reference| / max |reference|`` over one output: ``entropy``, ``logprob`` and the gradient.
The largest measured on the MI355X over the cases of a group are in ``MEASURED`` (``profiles/den_entropy/README.md``); every
bound is 4 x its figure -- the arithmetic is deterministic, the margin covers other seeds and compilers.  Everything else
is held bit for bit."""
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import check, lib
from torchain_amd.functions import den_path_entropy

import den_entropy_reference as der
from test_gpu_den_arc_post import _hub_fst
from fixtures import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S, T, RAGGED = 3, 7, (7, 4, 1)
MEASURED = {"graphs": {"entropy": 8.319e-8, "logprob": 2.003e-8, "grad": 1.896e-6},  # the four graphs and the 8192-state one
            "sharp": {"entropy": 1.344e-7, "logprob": 3.700e-10, "grad": 1.918e-5}}  # the cancellation case
BOUND = {group: {k: 4 * v for k, v in figures.items()} for group, figures in MEASURED.items()}
GRAPHS = ["one_wave", "hubs", "many_states", "skewed"]


@functools.lru_cache(maxsize=None)
def _graph(kind):
    fst = {"one_wave": lambda: synth.random_den_fst(37, 3, 11),
           "hubs": _hub_fst,
           "many_states": lambda: synth.random_den_fst(1100, 2, 70),
           "skewed": lambda: load_golden([g for g in GOLDEN if g.endswith("skewed_graph.npz")][0])[1],
           "c3_class": lambda: synth.random_den_fst(8192, 2, 4096, seed=3)}[kind]()
    return io.DenominatorGraph(fst, fst.num_pdfs)


def _y(kind, seqs=S, frames=T):
    return np.random.default_rng(77).normal(0.0, 2.0, size=(frames * seqs, _graph(kind).n_pdf)).astype(np.float32)


def _call(graph, y, lens=None, leaky=0.2, grad_output=None, **kw):
    """(entropy, logprob, gradient) of one differentiable call on a 2-D float32 matrix or a (B, C, T) tensor"""
    x = y.clone().requires_grad_(True)
    n = None if lens is not None or x.dim() == 3 else x.shape[0] // T
    h, lp = den_path_entropy(x, graph, frames=lens, leaky_hmm_coefficient=leaky, n_batch=n, **kw)
    h.backward(torch.ones_like(h) if grad_output is None else grad_output)
    torch.cuda.synchronize()
    assert h.dtype == lp.dtype == torch.float64 and x.grad.shape == x.shape and x.grad.dtype == x.dtype
    return h.detach(), lp, x.grad


@functools.lru_cache(maxsize=None)
def _got(kind, leaky=0.2, ragged=True):
    return _call(_graph(kind), torch.from_numpy(_y(kind)).to(DEV), list(RAGGED) if ragged else None, leaky)


def _figures(got, want):
    got = dict(zip(("entropy", "logprob", "grad"), (g.cpu().numpy().astype(np.float64) for g in got)))
    figures = {k: np.abs(got[k] - want[k]).max() / np.abs(want[k]).max() for k in got}
    print("MEASURED " + " ".join("%s %.3e" % kv for kv in figures.items()))
    return figures


def _bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def _same(a, b):
    return all(u.dtype == v.dtype and u.shape == v.shape and torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))


# ---- 1. against float64 ----
@pytest.mark.parametrize("kind,leaky,ragged", [(k, c, r) for k in GRAPHS for c in (1e-5, 0.2) for r in (False, True)])
def test_against_float64(kind, leaky, ragged):
    graph = _graph(kind)
    want = der.path_entropy(graph.arcs(), graph.initial_probs(), _y(kind), S, float(np.float32(leaky)), RAGGED if ragged else None)
    figures = _figures(_got(kind, leaky, ragged), want)
    assert all(figures[k] <= BOUND["graphs"][k] for k in figures), figures
    # the value alone: the forward pass gives the same bits, and no gradient launch ran
    with torch.no_grad():
        alone = graph.path_entropy(torch.from_numpy(_y(kind)).to(DEV), frames=list(RAGGED) if ragged else None,
                                   leaky_hmm_coefficient=leaky, n_batch=S)
    assert _same(alone, _got(kind, leaky, ragged)[:2])


# ---- 2. cancellation: H small beside |E[log W]| ----
def test_sharp_posterior_of_150_frames():
    graph, frames = _graph("one_wave"), 150
    src, dst, pdf, _ = (np.asarray(a) for a in graph.arcs())
    y = np.random.default_rng(5).normal(0.0, 2.0, size=(frames, 2, graph.n_pdf)).astype(np.float32)
    state = 0
    for t in range(frames):  # one path's pdfs stand out by 12, in both sequences
        a = np.flatnonzero(src == state)[t % 3 % max(1, (src == state).sum())]
        y[t, :, pdf[a]] += 12.0
        state = dst[a]
    y = y.reshape(frames * 2, -1)
    want = der.path_entropy(graph.arcs(), graph.initial_probs(), y, 2, float(np.float32(1e-5)))
    assert np.abs(want["entropy"]).max() < 0.02 * np.abs(want["logprob"] - want["entropy"]).min()  # H beside |E[log W]|
    figures = _figures(_call(graph, torch.from_numpy(y).to(DEV), [frames, frames], 1e-5), want)
    assert all(figures[k] <= BOUND["sharp"][k] for k in figures), figures


# ---- 4. bit for bit ----
@pytest.mark.parametrize("kind", GRAPHS)
def test_forms_batches_scales_groups_and_dtypes(kind):
    graph, whole = _graph(kind), _got(kind)
    y = torch.from_numpy(_y(kind)).to(DEV)
    lens = list(RAGGED)
    # the per-frame vectors in the workspace
    before = int(lib.tc_debug_counter(b"den_entropy_streamed_launches"))
    check(lib.tc_debug_set(b"force_den_entropy_streamed", 1), "tc_debug_set")
    try:
        forced = _call(graph, y, lens)
    finally:
        check(lib.tc_debug_set(b"force_den_entropy_streamed", 0), "tc_debug_set")
    assert int(lib.tc_debug_counter(b"den_entropy_streamed_launches")) == before + 1 and _same(forced, whole)
    # a sequence alone gives its part of the batch
    x = y.view(T, S, -1)
    for s, n in enumerate(RAGGED):
        h, lp, g = _call(graph, x[:, s].contiguous(), [n])
        assert _same((h[0], lp[0], g), (whole[0][s], whole[1][s], whole[2].view(T, S, -1)[:, s]))
    # grad_output = 4
    assert _same((_call(graph, y, lens, grad_output=torch.full((S,), 4.0, dtype=torch.float64, device=DEV))[2],), (4 * whole[2],))
    # two groups of sequences
    need = int(lib.tc_den_path_entropy_workspace_bytes(graph.ptr, 2, T, 1))
    before = int(lib.tc_debug_counter(b"den_entropy_launches"))
    assert _same(_call(graph, y, lens, max_workspace_bytes=need), whole)
    assert int(lib.tc_debug_counter(b"den_entropy_launches")) == before + 2
    # a bfloat16 (B, C, T) tensor against its float32 rows
    xb = x.permute(1, 2, 0).contiguous().to(torch.bfloat16)
    hb, lpb, gb = _call(graph, xb, lens)
    h2, lp2, g2 = _call(graph, xb.float().permute(2, 0, 1).reshape(T * S, -1).contiguous(), lens)
    assert _same((hb, lpb, gb), (h2, lp2, g2.view(T, S, -1).permute(1, 2, 0).contiguous().to(torch.bfloat16)))


def test_a_nan_costs_its_sequence_alone():
    graph, whole = _graph("hubs"), _got("hubs")
    y = torch.from_numpy(_y("hubs")).to(DEV)
    pad = y.clone()
    pad[5 * S + 1, 3] = float("nan")  # frame 5 of sequence 1, which has 4
    assert _same(_call(graph, pad, list(RAGGED)), whole)
    bad = y.clone()
    bad[2 * S + 1, 3] = float("nan")
    h, lp, g = _call(graph, bad, list(RAGGED))
    g, ok = g.view(T, S, -1), whole[2].view(T, S, -1)
    assert bool(h[1].isnan()) and bool(lp[1].isnan()) and int(_bits(g[:, 1]).abs().max()) == 0
    assert _same((h[[0, 2]], lp[[0, 2]], g[:, [0, 2]]), (whole[0][[0, 2]], whole[1][[0, 2]], ok[:, [0, 2]]))


# ---- 5. C3's class stays on chip ----
def test_8192_states_and_4096_pdfs_are_resident():
    graph, y = _graph("c3_class"), _y("c3_class", 1, 3)
    assert graph.num_states == 8192 and graph.n_pdf == 4096
    want = der.path_entropy(graph.arcs(), graph.initial_probs(), y, 1, float(np.float32(0.2)))
    before = int(lib.tc_debug_counter(b"den_entropy_streamed_launches"))
    x = torch.from_numpy(y).to(DEV).requires_grad_(True)
    h, lp = den_path_entropy(x, graph, frames=[3], leaky_hmm_coefficient=0.2)
    h.backward(torch.ones_like(h))
    torch.cuda.synchronize()
    assert int(lib.tc_debug_counter(b"den_entropy_streamed_launches")) == before
    figures = _figures((h.detach(), lp, x.grad), want)
    assert all(figures[k] <= BOUND["graphs"][k] for k in figures), figures
